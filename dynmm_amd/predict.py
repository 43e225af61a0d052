"""python -m dynmm_amd.predict --dynamic --global-gate [--baseline] --hard --ckpt_path CKPT --out DIR
       (--dataset nyuv2 --dataset_dir DIR | --dataset synthetic) ...

Label images from a trained network: the forward ends in the uint8 label map on the device (engine.InferStep.segment — with
the learned up-samplings the decoder's tail and the arg-max are one kernel, csrc/segment.hip), the map is what is copied to the
host (160x smaller than the logits), and every image is written as DIR/NAME.png, 8-bit single channel, stored value = class + 1:
the layout of NYUv2's `labels_40` (0, void, is never written).  The model flags are those of `dynmm_amd.eval`; with
--dataset_dir the NYUv2 test split is predicted, with --dataset synthetic a synthetic NYUv2-shaped set; other data sets have
no reader and are refused."""
import os
import sys
import time

import numpy as np
import torch

from . import engine
from .data import SyntheticRGBD, nyuv2_split
from .src.args import ArgumentParserRGBDSegmentation
from .src.build_model import build_for_args


def _png_writer():
    """8-bit single-channel PNG writer with cv2 or PIL, whichever imports (the pair data._png_reader reads with)."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        def write(path, im):
            if not cv2.imwrite(path, im):
                raise OSError(f'cannot write {path}')
        return write
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('writing label images needs cv2 or PIL (Pillow); neither is importable') from None

    def write(path, im):
        Image.fromarray(im).save(path)                # (2-D uint8 -> mode 'L')
    return write


def run(args, model, loader, device=None, use_graph=True, out_dir=None, names=None):
    """Label maps for a model the caller built and ANY loader the caller brings (an iterable of dicts with `image` and `depth`,
    as eval.run takes).  Sets the gate flags from `args` (hard / ini / baseline), runs InferStep.segment per batch and returns
    the list of uint8 [H,W] numpy maps (class indices 0..C-1), one per image in loader order.  With `out_dir` every map is also
    written as out_dir/NAME.png with stored value = class + 1; NAME comes from `names`, else the loader's `filenames`, else the
    running index.  Prints images/s (forward + copy to the host; the PNG encoding is not counted)."""
    device = next(model.parameters()).device if device is None else device
    model.eval()
    model.hard_gate, model.ini_stage, model.baseline = args.hard, args.ini, args.baseline
    step = engine.InferStep(model, policy='auto') if use_graph else None
    names = names if names is not None else getattr(loader, 'filenames', None)
    write = None
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        write = _png_writer()
    maps, busy = [], 0.0
    for s in loader:
        image, depth = s['image'].to(device), s['depth'].to(device)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        pred = step.segment(image, depth) if step is not None else model.segment(image, depth)
        host = pred.cpu().numpy()                                 # (the copy synchronises: the forward is inside the interval)
        busy += time.perf_counter() - t0
        for m in host:
            k = len(maps)
            maps.append(np.ascontiguousarray(m))
            if write is not None:
                name = names[k] if names is not None and k < len(names) else f'{k:06d}'
                write(os.path.join(out_dir, f'{name}.png'), (m + 1).astype(np.uint8))
    print(f'{len(maps)} images, {len(maps) / max(busy, 1e-9):0.1f} images/s' + (f', written to {out_dir}' if out_dir else ''))
    return maps


def main(argv=None):
    p = ArgumentParserRGBDSegmentation(description='Efficient RGBD Indoor Semantic Segmentation (Prediction, MI355X)')
    p.set_common_args()
    p.set_eval_args()
    p.add_argument('--out', type=str, required=True, help='directory the label images are written to')
    p.add_argument('--synthetic_samples', type=int, default=8)
    p.add_argument('--no_hip_graph', action='store_true', help='eager launches instead of hipGraph replays of the forward')
    args = p.parse_args(argv)
    args.pretrained_on_imagenet = False
    if args.dataset not in ('nyuv2', 'synthetic'):
        raise NotImplementedError(f'--dataset {args.dataset}: only nyuv2 (and synthetic) have a reader on the HIP path')
    if args.dataset == 'nyuv2' and args.dataset_dir is None:
        raise NotImplementedError('--dataset nyuv2 needs --dataset_dir (or use --dataset synthetic)')
    model, device = build_for_args(args, n_classes=40)
    if args.ckpt_path:
        ckpt = torch.load(args.ckpt_path, map_location=device)
        model.load_state_dict(ckpt['state_dict'])               # strict, as eval.py
        print(f'Loaded checkpoint from {args.ckpt_path}')
    if args.dataset == 'nyuv2':
        data = nyuv2_split(args, 'test', device)
    else:
        data = SyntheticRGBD(args.synthetic_samples, args.batch_size_valid or args.batch_size, args.height, args.width,
                             seed=77, device=device)
    return run(args, model, data, device, use_graph=not args.no_hip_graph, out_dir=args.out)


if __name__ == '__main__':
    main(sys.argv[1:])

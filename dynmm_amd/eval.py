"""python -m dynmm_amd.eval --dynamic --global-gate [--baseline] --hard --ckpt_path CKPT --dataset nyuv2 --dataset_dir DIR ...

Counterpart of FusionDynMM/eval.py:35-151: load a (reference-format) checkpoint strictly, set the gate
flags, optional Gaussian-noise robustness runs (modes 0/1/2), mIoU*100 per run.  With --dataset_dir the NYUv2 test split is
evaluated (dynmm_amd.data.NYUv2); without one, a synthetic NYUv2-shaped set; other data sets have no reader and are refused."""
import random
import sys

import numpy as np
import torch

from . import engine
from .data import SyntheticRGBD, nyuv2_split
from .src.args import ArgumentParserRGBDSegmentation
from .src.build_model import build_for_args


def set_seed(seed):
    """src/utils.py set_seed as eval.py uses it before every noise-robustness run."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def run(args, model, valid_loader, device=None, use_graph=True, fused_labels=False, per_camera=None):
    """eval.py:63-151 for a model the caller built and ANY loader the caller brings — an iterable of dicts with `image` [N,3,H,W],
    `depth` [N,1,H,W] (normalised as src/preprocessing.py does) and `label_orig` [N,H0,W0] (0 = void), on the host or the device:
    the entry `python -m dynmm_amd.eval` calls with the NYUv2 test split (dynmm_amd.data.NYUv2) or the synthetic set, and the one
    a user with another loader calls.  Sets the gate flags from `args` (hard / ini / baseline), runs
    `args.num_runs` passes with the reference's per-run seeds and Gaussian-noise modes 0 / 1 / 2, prints and returns mIoU*100 per
    run.  `use_graph`: the forward is replayed as hipGraphs (engine.InferStep; eager where that does not apply).

    A loader with by_camera() (dynmm_amd.data.SUNRGBD) is evaluated camera by camera — ALL of them, where the reference's
    eval.py stops at cameras[0] — with the loader's class count: one line per camera and one for all per run, and the run's
    result is the mIoU*100 of the summed confusion matrices.  `per_camera` (a list) receives each run's {camera: mIoU*100}."""
    device = next(model.parameters()).device if device is None else device
    model.eval()
    if hasattr(model, 'start_weight'):
        model.start_weight()
    model.hard_gate, model.ini_stage, model.baseline = args.hard, args.ini, args.baseline
    step = engine.InferStep(model, policy='auto') if use_graph else None      # (replay or eager launches: whichever this host runs faster)
    results = []
    for r in range(args.num_runs):
        set_seed(r)                                              # eval.py: per-run seed -> reproducible noise runs

        def batches(loader):
            for s in loader:
                image, depth = s['image'].to(device), s['depth'].to(device)
                u = random.random()                              # eval.py:91-102
                if args.mode in (0, 2) and u < 0.33:
                    image = image + args.noise * image.abs().mean() * torch.randn_like(image)
                elif (args.mode == 1 and u < 0.33) or (args.mode == 2 and u < 0.66):
                    depth = depth + args.noise * depth.abs().mean() * torch.randn_like(depth)
                yield image, depth, s['label_orig'].to(device)
        if hasattr(valid_loader, 'by_camera'):
            by, cms = {}, []
            for camera, loader in valid_loader.by_camera().items():
                by[camera], cm = engine.evaluate(model, batches(loader), num_classes=valid_loader.n_classes_without_void,
                                                 hard=args.hard, infer_step=step, fused_labels=fused_labels)
                cms.append(cm)
                print(f'Run {r}, {camera} mIoU: {by[camera]:0.2f}')
            miou = engine.miou_of(sum(cms))
            print(f'Run {r}, all cameras mIoU: {miou:0.2f}')
            if per_camera is not None:
                per_camera.append(by)
        else:
            miou, _ = engine.evaluate(model, batches(valid_loader), num_classes=getattr(valid_loader, 'n_classes_without_void', 40),
                                      hard=args.hard, infer_step=step, fused_labels=fused_labels)
            print(f'Run {r}, mIoU: {miou:0.2f}')
        results.append(miou)
    if hasattr(model, 'end_weight'):
        model.end_weight(print_flop=args.hard)
    print(results)
    return results


def parse_args(argv=None):
    p = ArgumentParserRGBDSegmentation(description='Efficient RGBD Indoor Semantic Segmentation (Evaluation, MI355X)')
    p.set_common_args()
    p.set_eval_args()
    p.add_argument('--synthetic_samples', type=int, default=8)
    p.add_argument('--no_hip_graph', action='store_true', help='eager launches instead of hipGraph replays of the forward')
    p.add_argument('--fused_labels', action='store_true',
                   help='end the forward in the label map (decoder tail fused with the arg-max) where the labels have the '
                        "network's size")
    args = p.parse_args(argv)
    args.pretrained_on_imagenet = False
    return args


def load_weights(model, args, device):
    if args.ckpt_path:
        ckpt = torch.load(args.ckpt_path, map_location=device)
        model.load_state_dict(ckpt['state_dict'])               # strict, eval.py:60-61
        print(f'Loaded checkpoint from {args.ckpt_path}')


def main(argv=None):
    args = parse_args(argv)
    if args.dataset_dir is not None and args.dataset not in ('nyuv2', 'synthetic'):
        raise NotImplementedError(f'--dataset {args.dataset}: only nyuv2 (and synthetic) have a reader on the HIP path here; '
                                  'SUNRGB-D is evaluated through python -m dynmm_amd.sunrgbd eval')
    model, device = build_for_args(args, n_classes=40)
    load_weights(model, args, device)
    if args.dataset_dir is not None and args.dataset == 'nyuv2':
        data = nyuv2_split(args, 'test', device)
    else:
        data = SyntheticRGBD(args.synthetic_samples, args.batch_size_valid or args.batch_size, args.height, args.width,
                             seed=77, device=device)
    return run(args, model, data, device, use_graph=not args.no_hip_graph, fused_labels=args.fused_labels)


if __name__ == '__main__':
    main(sys.argv[1:])

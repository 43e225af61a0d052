"""python -m dynmm_amd.sunrgbd train --dataset_dir DIR [train.py's flags]
   python -m dynmm_amd.sunrgbd eval  --dataset_dir DIR --ckpt_path CKPT [eval.py's flags]

SUNRGB-D (37 classes, four cameras with four image sizes) on the HIP path: what FusionDynMM's train.py / eval.py do under
`--dataset sunrgbd`.  The flags are those of dynmm_amd.train / dynmm_amd.eval; the data set is fixed here, the model is built with
37 classes, and the data comes from dynmm_amd.data.prepare_sunrgbd (decoded once into a ragged store on the device, one input
kernel per batch).  train validates every camera and keeps the best checkpoint by the all-cameras mIoU; eval reports every camera
and all.  `python -m dynmm_amd.train / eval / predict --dataset sunrgbd` keep refusing."""
import os
import sys

import torch
import torch.distributed as dist

from . import eval as ev
from . import train
from .data import prepare_sunrgbd, sunrgbd_split
from .src.build_model import build_for_args

DATASET = 'sunrgbd'
N_CLASSES = 37


def _fix_dataset(args):
    if args.dataset_dir is None:
        raise SystemExit('python -m dynmm_amd.sunrgbd needs --dataset_dir (the layout of src/datasets/sunrgbd/prepare_dataset.py)')
    args.dataset = DATASET
    return args


def train_main(argv=None):
    args = _fix_dataset(train.parse_args(argv))
    world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
    if world > 1:
        dist.init_process_group(os.environ.get('DYNMM_DIST_BACKEND', 'nccl'))
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
    ckpt_dir = train.make_ckpt_dir(args, rank)
    model, device = build_for_args(args, n_classes=N_CLASSES)
    train_loader, valid_loader = prepare_sunrgbd(args, device, rank, world, seed=args.data_seed)
    return train.run(args, model, train_loader, valid_loader, ckpt_dir, rank, world)


def eval_main(argv=None, per_camera=None):
    args = _fix_dataset(ev.parse_args(argv))
    model, device = build_for_args(args, n_classes=N_CLASSES)
    ev.load_weights(model, args, device)
    data = sunrgbd_split(args, 'test', device)
    # --fused_labels never applies: no camera stores its labels at the network's size
    return ev.run(args, model, data, device, use_graph=not args.no_hip_graph, fused_labels=args.fused_labels,
                  per_camera=per_camera)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if not argv or argv[0] not in ('train', 'eval'):
        raise SystemExit('usage: python -m dynmm_amd.sunrgbd {train,eval} --dataset_dir DIR [flags of dynmm_amd.train / '
                         'dynmm_amd.eval]')
    return (train_main if argv[0] == 'train' else eval_main)(argv[1:])


if __name__ == '__main__':
    main()

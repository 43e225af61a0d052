"""python -m dynmm_amd.imdb_mm [--fuse 0|1] [--n-epochs N] [--eval-only] ...

Counterpart of ModalityDynMM/multimedia/imdb_mm.py (Step I): train one multi-modal MM-IMDB expert with
Supervised_Learning.train (AdamW, weight decay 0.01, BCEWithLogitsLoss, clip_grad_norm_(8), early stopping on validation
F1-macro), save it under --log-dir and test it with single_test (F1 micro / macro).
  --fuse 1 (lf): MaxOut_MLP(512, 512, 300, linear_layer=False), MaxOut_MLP(512, 1024, 4096, 512, False), Concat,
                 Linear(1024, 23), lr 8e-3 -> best_lf.pt (DynMMNet's branch3)
  --fuse 0 (ef, the reference's default): identity encoders, Concat, MaxOut_MLP(23, 512, 4396), lr 4e-2 -> best_ef.pt
--fuse 2 / 3 (LowRankTensorFusion, MultiplicativeInteractions2Modal) are refused from the command line; both models run on
the HIP path through their builders, experts.imdb_mm_lrtf() -> best_lrtf.pt and experts.imdb_mm_mim() -> best_mim.pt (lr 8e-3,
trained with experts.train like the others).  Data as dynmm_amd.imdb."""
import argparse
import os

import numpy as np
import torch

from . import experts as E
from . import imdb


def parser():
    p = argparse.ArgumentParser('imdb', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--fuse', type=int, default=0, help='fusion model')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--measure', action='store_true', help='time the test pass')
    p.add_argument('--n-epochs', type=int, default=1000, help='number of epochs')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz', help='data source')
    p.add_argument('--data-dir', type=str, default='./data/mmimdb', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/imdb', help='where the expert state_dict is written')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=1024, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


WD = 0.01


def file_name(log_dir, fuse):
    """The path imdb_mm.py writes for --fuse (best_lf.pt is what dynmm_amd.imdb.load_pretrained reads as branch3)."""
    return os.path.join(log_dir, f'best_{E.IMDB_FUSE[fuse]}.pt')


def main(argv=None):
    args = parser().parse_args(argv)
    E.imdb_mm(args.fuse)                                  # refuses --fuse 2 / 3 before any device work
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    E.ensure_dir(args.log_dir)
    filename = file_name(args.log_dir, args.fuse)
    loaders = imdb.load_data(args, device)
    adapt = lambda inputs: inputs                         # noqa: E731
    log1, log2 = [], []
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        model, lr = E.imdb_mm(args.fuse)
        model = model.to(device)
        if not args.eval_only:
            E.train(model, loaders, adapt, 'bce', lr, WD, args.n_epochs, lambda: E.save_state(model, filename))
        print(f'Testing {filename}')
        E.load_state(model, filename, device)
        with E.Timer(args.measure):
            micro, macro, _ = E.evaluate_multilabel(model, loaders[2], adapt)
        print(f'f1_micro: {micro * 100:.2f} | f1_macro: {macro * 100:.2f}')
        log1.append(micro)
        log2.append(macro)
    E.f1_summary(log1, log2)
    return np.array(log1), np.array(log2)


if __name__ == '__main__':
    main()

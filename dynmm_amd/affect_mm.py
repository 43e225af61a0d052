"""python -m dynmm_amd.affect_mm [--fusion 3] [--lr LR] [--wd WD] [--n-epochs N] [--eval-only] ...

Counterpart of ModalityDynMM/affect/affect_mm.py (Step I): train the late-fusion CMU-MOSEI expert (`--fusion 3`, lf_tran:
Transformer(35, 60), Transformer(74, 120), Transformer(300, 120), Concat, MLP(300, 128, 1)) with Supervised_Learning.train
(AdamW lr 1e-4, weight decay 1e-4, L1Loss, clip_grad_norm_(8), early stopping on the validation loss), save it as
lf_tran.pt and b2_lf_tran.pt (the name dynmm_amd.affect --model v2 reads) under --log-dir, reload it and test it on the
validation and the test split with single_test (Accuracy, Loss, Corr).  The other switches are refused: the GRU fusions
(--fusion 0, 1, 5) and the early-fusion transformer (--fusion 2, ef_tran: Transformer(409, 300) + MLP(300, 128, 1)) run on the
HIP path at the module level (experts.affect_mm_gru, affect_mm_lrtf, affect_mm_ef_tran; file_names gives their file names) but
are not wired to the command line yet, and so is MULT (--fusion 4: experts.affect_mm_mult, nn.mult.MULTModel).  Data as
dynmm_amd.affect."""
import argparse
import os

import numpy as np
import torch

from . import affect
from . import experts as E


def parser():
    p = argparse.ArgumentParser('unimodal network on mosi', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--data', type=str, default='mosei', help='dataset: mosi / mosei')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--fusion', type=int, default=3, help='0-4')
    p.add_argument('--lr', type=float, default=1e-4, help='learning rate')
    p.add_argument('--wd', type=float, default=1e-4, help='weight decay')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--measure', action='store_true', help='measure inference time')
    p.add_argument('--n-epochs', type=int, default=1000, help='number of epochs')
    p.add_argument('--graph', action='store_true', help='replay each training step as one hipGraph')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz', help='data source')
    p.add_argument('--data-dir', type=str, default='./data/mosei', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/mosei', help='where the expert state_dict is written')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=512, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


def file_names(log_dir, fusion):
    """(path affect_mm.py writes for --fusion, the b2_ copy affect_dyn.py:211 reads)."""
    name = E.AFFECT_FUSION[fusion]
    return os.path.join(log_dir, name + '.pt'), os.path.join(log_dir, 'b2_' + name + '.pt')


def main(argv=None):
    args = parser().parse_args(argv)
    E.affect_mm(args.fusion)                              # refusals before any device work
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    loaders = affect.load_data(args, device)
    adapt = lambda inputs: inputs                         # noqa: E731
    E.ensure_dir(args.log_dir)
    name = E.AFFECT_FUSION[args.fusion]
    filename, copy = file_names(args.log_dir, args.fusion)
    log = np.zeros((args.n_runs, 3))
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        model = E.affect_mm(args.fusion).to(device)
        print(f'Fusion model {name}')
        if not args.eval_only:
            E.train(model, loaders, adapt, 'l1', args.lr, args.wd, args.n_epochs, lambda: E.save_state(model, filename, copy),
                    use_graph=args.graph)
        print(f'Testing model {filename}:')
        E.load_state(model, filename, device)
        print('Val data')
        with E.Timer(args.measure):
            E.posneg_line(E.evaluate_posneg(model, loaders[1], adapt))
        print('Test data')
        with E.Timer(args.measure):
            r = E.evaluate_posneg(model, loaders[2], adapt)
        E.posneg_line(r)
        log[n] = r['Accuracy'], r['Loss'], r['Corr']
    E.posneg_summary(log, 4)
    return log


if __name__ == '__main__':
    main()

"""python -m dynmm_amd.imdb_uni [--mod 0|1] [--n-epochs N] [--eval-only] ...

Counterpart of ModalityDynMM/multimedia/imdb_uni.py (Step I): train one uni-modal MM-IMDB expert, --mod 0 text
(MLP(300, 512, 512) + MLP(512, 512, 23)) or --mod 1 image (MLP(4096, 1024, 512) + MLP(512, 512, 23)), with AdamW (lr 1e-4,
weight decay 0.01), BCEWithLogitsLoss and early stopping on validation F1-macro; save encoder_{text,image}.pt and
head_{text,image}.pt (state_dicts) under --log-dir, reload them and test (F1 micro / macro).  Data as dynmm_amd.imdb.
The protocol is dynmm_amd.experts.train with MultiBench unimodal.train's print lines (see DESIGN.md for what is assumed)."""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn

from . import experts as E
from . import imdb


def parser():
    p = argparse.ArgumentParser('imdb', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--mod', type=int, default=0, help='0: text; 1: image')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--measure', action='store_true', help='time the test pass')
    p.add_argument('--n-epochs', type=int, default=1000, help='number of epochs')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz', help='data source')
    p.add_argument('--data-dir', type=str, default='./data/mmimdb', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/imdb', help='where the expert state_dicts are written')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=1024, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


LR, WD = 1e-4, 0.01


def file_names(log_dir, mod):
    """(encoder, head) paths imdb_uni.py writes for --mod and dynmm_amd.imdb.load_pretrained reads."""
    modality = E.IMDB_MODS[mod]
    return os.path.join(log_dir, f'encoder_{modality}.pt'), os.path.join(log_dir, f'head_{modality}.pt')


def main(argv=None):
    args = parser().parse_args(argv)
    E.imdb_uni(args.mod)                                  # refuses an unknown --mod before any device work
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    E.ensure_dir(args.log_dir)
    encoderfile, headfile = file_names(args.log_dir, args.mod)
    loaders = imdb.load_data(args, device)
    adapt = lambda inputs: inputs[args.mod]               # noqa: E731 (unimodal.train's j[modalnum])
    log1, log2 = [], []
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        encoder, head = E.imdb_uni(args.mod)
        model = nn.Sequential(encoder, head).to(device)
        if not args.eval_only:
            E.train(model, loaders, adapt, 'bce', LR, WD, args.n_epochs,
                    lambda: (E.save_state(encoder, encoderfile), E.save_state(head, headfile)), protocol='uni')
        print(f'Testing model {encoderfile} and {headfile}:')
        E.load_state(encoder, encoderfile, device)
        E.load_state(head, headfile, device)
        with E.Timer(args.measure):
            micro, macro, _ = E.evaluate_multilabel(model, loaders[2], adapt)
        print(f'f1_micro: {micro * 100:.2f} | f1_macro: {macro * 100:.2f}')
        log1.append(micro)
        log2.append(macro)
    E.f1_summary(log1, log2)
    return np.array(log1), np.array(log2)


if __name__ == '__main__':
    main()

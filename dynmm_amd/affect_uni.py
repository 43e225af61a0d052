"""python -m dynmm_amd.affect_uni [--mod 0|1|2] [--hidden-dim1 H1] [--hidden-dim2 H2] [--n-epochs N] [--eval-only] ...

Counterpart of ModalityDynMM/affect/affect_uni.py (Step I): train one uni-modal CMU-MOSEI expert, Transformer(F, 120) +
MLP(120, 64, 1) on the visual (--mod 0, F = 35), audio (1, F = 74) or text (2, F = 300, the default) features, with AdamW
(lr 1e-4, weight decay 0.01), L1Loss and early stopping on the validation loss; save
reg_transformer_{encoder,head}_{visual,audio,text}.pt (state_dicts) under --log-dir — the text expert also as
b1_reg_transformer_{encoder,head}_text.pt, the names dynmm_amd.affect --model v2 reads — reload them and test them on the
validation and the test split (Accuracy, Loss, Corr).  --enc gru and --clf are refused.  Data as dynmm_amd.affect.
The protocol is dynmm_amd.experts.train (see DESIGN.md for what MultiBench's unvendored unimodal.train leaves assumed)."""
import argparse
import os

import numpy as np
import torch
import torch.nn as nn

from . import affect
from . import experts as E


def parser():
    p = argparse.ArgumentParser('unimodal network on mosi', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--mod', type=int, default=2, help='0/1/2')
    p.add_argument('--enc', type=str, default='transformer', help='encoder architecture: gru or transformer '
                   '(only transformer is implemented)')
    p.add_argument('--hidden-dim1', type=int, default=0, help='hidden dimension 1')
    p.add_argument('--hidden-dim2', type=int, default=0, help='hidden dimension 2')
    p.add_argument('--data', type=str, default='mosei', help='dataset: mosi / mosei')
    p.add_argument('--lr', type=float, default=1e-4, help='learning rate')
    p.add_argument('--clf', action='store_true', help='classification model, otherwise regression (not implemented)')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--measure', action='store_true', help='time the test passes')
    p.add_argument('--n-epochs', type=int, default=100, help='number of epochs')
    p.add_argument('--graph', action='store_true', help='replay each training step as one hipGraph')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz', help='data source')
    p.add_argument('--data-dir', type=str, default='./data/mosei', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/mosei', help='where the expert state_dicts are written')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=512, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


WD = 0.01


def file_names(log_dir, mod_name, enc='transformer'):
    """(encoder, head) paths affect_uni.py writes, and the b1_ copies affect_dyn.py:211 reads for the text expert."""
    enc_name = os.path.join(log_dir, f'reg_{enc}_encoder_{mod_name}.pt')
    head_name = os.path.join(log_dir, f'reg_{enc}_head_{mod_name}.pt')
    copies = []
    if mod_name == 'text':
        copies = [os.path.join(log_dir, 'b1_' + os.path.basename(f)) for f in (enc_name, head_name)]
    return enc_name, head_name, copies


def main(argv=None):
    args = parser().parse_args(argv)
    E.affect_uni(args.mod, args.enc, args.hidden_dim1, args.hidden_dim2, args.clf)    # refusals before any device work
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    loaders = affect.load_data(args, device)
    adapt = lambda inputs: [inputs[0][args.mod], inputs[1][args.mod]]                 # noqa: E731 (is_packed, modalnum)
    E.ensure_dir(args.log_dir)
    log = np.zeros((args.n_runs, 3))
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        encoder, head, mod_name = E.affect_uni(args.mod, args.enc, args.hidden_dim1, args.hidden_dim2, args.clf)
        model = nn.Sequential(encoder, head).to(device)
        encoder_name, head_name, copies = file_names(args.log_dir, mod_name, args.enc)
        print(f'unimodal training, modality {mod_name}, task regression')
        if not args.eval_only:
            def save():
                E.save_state(encoder, encoder_name, *copies[:1])
                E.save_state(head, head_name, *copies[1:])
            E.train(model, loaders, adapt, 'l1', args.lr, WD, args.n_epochs, save, protocol='uni', use_graph=args.graph)
        print(f'Testing model {encoder_name} | {head_name}:')
        E.load_state(encoder, encoder_name, device)
        E.load_state(head, head_name, device)
        print('Val data')
        with E.Timer(args.measure):
            E.posneg_line(E.evaluate_posneg(model, loaders[1], adapt))
        print('Test data')
        with E.Timer(args.measure):
            r = E.evaluate_posneg(model, loaders[2], adapt)
        E.posneg_line(r)
        log[n] = r['Accuracy'], r['Loss'], r['Corr']
    E.posneg_summary(log, 2)
    return log


if __name__ == '__main__':
    main()

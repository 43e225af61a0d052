"""python -m dynmm_amd.imdb [--freeze] [--hard] [--no-pretrain] [--infer-mode N] ...

Counterpart of ModalityDynMM/multimedia/imdb_dyn.py: train the MM-IMDB DynMM (Supervised_Learning.train with AdamW,
BCEWithLogitsLoss + reg * gate regulariser, clip_grad_norm_(8), early stop on validation F1-macro with patience 7), save the
best model, test it with the hard gate and print the reference's summary line (F1 micro / macro, FLOPs, branch selection
ratio).  Data: --data-dir holding {train,valid,test}.npz with `text` [N,300], `image` [N,4096], `label` [N,23] (the
reference's hdf5 needs h5py), or --dataset synthetic.  Pretrained experts: --log-dir holding the state_dicts
encoder_text.pt, head_text.pt, encoder_image.pt, head_image.pt and best_lf.pt.  run(args, model, loaders) serves a caller's
own data."""
import argparse
import copy
import os

import numpy as np
import torch

from . import ops_mlp as M
from .nn import imdb as I


def parser():
    p = argparse.ArgumentParser('imdb', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--data', type=str, default='imdb', help='dataset name')
    p.add_argument('--n-epochs', type=int, default=50, help='number of epochs')
    p.add_argument('--lr', type=float, default=1e-4, help='learning rate')
    p.add_argument('--wd', type=float, default=1e-2, help='weight decay')
    p.add_argument('--reg', type=float, default=0.1, help='reg loss weight')
    p.add_argument('--freeze', action='store_true', help='freeze branch weights')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--hard', action='store_true', help='hard labels')
    p.add_argument('--no-pretrain', action='store_true', help='train from scratch')
    p.add_argument('--infer-mode', type=int, default=0, help='infer mode')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz', help='data source')
    p.add_argument('--data-dir', type=str, default='./data/mmimdb', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/imdb', help='expert state_dicts and saved models')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=1024, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


class Loader:
    """Batches of ([text, image], label) on the device; shuffled per epoch when `shuffle`."""

    def __init__(self, text, image, label, batch_size, shuffle, device, seed=0):
        self.t = torch.as_tensor(text, dtype=torch.float32).to(device)
        self.i = torch.as_tensor(image, dtype=torch.float32).to(device)
        self.y = torch.as_tensor(label, dtype=torch.float32).to(device)
        self.bs, self.shuffle = batch_size, shuffle
        self.g = torch.Generator().manual_seed(seed)

    def __len__(self):
        return (self.t.shape[0] + self.bs - 1) // self.bs

    def __iter__(self):
        n = self.t.shape[0]
        idx = torch.randperm(n, generator=self.g).to(self.t.device) if self.shuffle else None
        for s in range(0, n, self.bs):
            if idx is None:
                yield [self.t[s:s + self.bs], self.i[s:s + self.bs]], self.y[s:s + self.bs]
            else:
                j = idx[s:s + self.bs]
                yield [self.t[j], self.i[j]], self.y[j]


def synthetic_split(n, seed):
    """Features with a learnable multilabel signal: labels are thresholded random projections of the features."""
    g = np.random.default_rng(seed)
    wt = np.random.default_rng(1234).standard_normal((I.FEATURES['text'], I.NUM_CLASSES)).astype(np.float32)
    wi = np.random.default_rng(4321).standard_normal((I.FEATURES['image'], I.NUM_CLASSES)).astype(np.float32)
    text = g.standard_normal((n, I.FEATURES['text'])).astype(np.float32)
    image = np.abs(g.standard_normal((n, I.FEATURES['image']))).astype(np.float32)
    score = text @ wt / np.sqrt(300) + (image - image.mean()) @ wi / np.sqrt(4096)
    label = (score > 0.8).astype(np.float32)
    return text, image, label


def load_data(args, device):
    if args.dataset == 'synthetic':
        n = args.synthetic_size
        splits = [synthetic_split(n, args.seed + 1), synthetic_split(max(n // 4, 2), args.seed + 2),
                  synthetic_split(max(n // 4, 2), args.seed + 3)]
    else:
        splits = []
        for name in ('train', 'valid', 'test'):
            d = np.load(os.path.join(args.data_dir, name + '.npz'))
            splits.append((d['text'], d['image'], d['label']))
    return [Loader(*s, args.batch_size, shuffle=(k == 0), device=device, seed=args.seed) for k, s in enumerate(splits)]


def load_pretrained(model, log_dir):
    """The reference's pretrained experts, as state_dicts (a pickled MultiBench module cannot be unpickled without it)."""
    parts = {'text_encoder': 'encoder_text.pt', 'text_head': 'head_text.pt', 'image_encoder': 'encoder_image.pt',
             'image_head': 'head_image.pt', 'branch3': 'best_lf.pt'}
    for attr, fname in parts.items():
        path = os.path.join(log_dir, fname)
        try:
            sd = torch.load(path, map_location='cpu', weights_only=True)
        except Exception as e:
            raise RuntimeError(f'{path}: expected a state_dict; a pickled MultiBench module cannot be loaded without '
                               f'MultiBench: export it with torch.save(torch.load(path).state_dict(), path) ({e})') from e
        getattr(model, attr).load_state_dict(sd)


def evaluate(model, loader):
    """Supervised_Learning.test for task "multilabel": (f1_micro, f1_macro, mean BCE) with one host read."""
    counts = None
    model.eval()
    with torch.no_grad():
        for inputs, y in loader:
            out, _ = model(inputs)
            if counts is None:
                counts = M.MultilabelCounts(y.shape[1], y.device)
            counts.add(out, y)
    r = counts.read()
    micro, macro = M.f1_from_counts(r['tp'], r['fp'], r['fn'])
    return micro, macro, r['loss']


def train(args, model, loaders, save=None):
    """Supervised_Learning.train (moe_model, additional_loss, multilabel, AdamW, early_stop): returns the per-epoch mean
    training objective and the best model's state_dict."""
    train_loader, valid_loader = loaders[0], loaders[1]
    step = I.ImdbTrainStep(model, lr=args.lr, weight_decay=args.wd, lossw=args.reg)
    best, patience, best_sd, history = -1.0, 0, None, []
    for epoch in range(args.n_epochs):
        model.train()
        tot, nb = torch.zeros(1, device=step.flat_g.device), 0
        for inputs, y in train_loader:
            if y.shape[0] < 2:
                continue
            last = step(inputs, y)
            tot += last['total'] * y.shape[0]
            nb += y.shape[0]
        loss = float(tot.item()) / max(nb, 1)
        history.append(loss)
        micro, macro, vloss = evaluate(model, valid_loader)
        print(f'Epoch {epoch} train loss: {loss:.4f} valid loss: {vloss:.4f} f1_micro: {micro:.4f} f1_macro: {macro:.4f}')
        if macro > best:
            patience, best = 0, macro
            best_sd = copy.deepcopy(model.state_dict())
            print('Saving Best')
            if save:
                torch.save(best_sd, save)
        else:
            patience += 1
        if patience > 7:
            break
    return history, best_sd


def run(args, model, loaders):
    """One run of imdb_dyn.py's main loop on the caller's model and loaders ([train, valid, test] iterables of
    ([text, image], label) device batches): train unless args.eval_only, restore the best model, test with the hard gate.
    Returns (branch selection ratio, f1_micro, f1_macro, FLOPs, training history)."""
    history = []
    if not args.eval_only:
        model.hard_gate = args.hard
        history, best_sd = train(args, model, loaders, getattr(args, 'save', None))
        if best_sd is not None:
            model.load_state_dict(best_sd)
    model.hard_gate = True
    model.infer_mode = args.infer_mode
    print('-' * 30 + 'Test data' + '-' * 30)
    model.reset_weight()
    micro, macro, _ = evaluate(model, loaders[2])
    print(f'f1_micro: {micro:.4f} f1_macro: {macro:.4f}')
    ratio = model.weight_stat()
    return ratio, micro, macro, model.cal_flop(), history


def main(argv=None):
    args = parser().parse_args(argv)
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    loaders = load_data(args, device)
    log1, log2 = np.zeros((args.n_runs, 1)), np.zeros((args.n_runs, 3))
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        model = I.DynMMNet(freeze=args.freeze)
        if not args.no_pretrain:
            load_pretrained(model, args.log_dir)
        model = model.to(device)
        os.makedirs(os.path.join('./log', args.data), exist_ok=True)
        args.save = os.path.join('./log', args.data, f'DynMMNet_freeze{args.freeze}_reg_{args.reg}.pt')
        if args.eval_only:
            model.load_state_dict(torch.load(args.save, map_location=device, weights_only=True))
            print(f'Testing model {args.save}:')
        ratio, micro, macro, flop, _ = run(args, model, loaders)
        log1[n] = ratio
        log2[n] = micro, macro, flop
    print(log1)
    print(log2)
    print('-' * 60)
    print(f'Finish {args.n_runs} runs')
    print(f'Test f1 micro {np.mean(log2[:, 0]) * 100:.2f} ± {np.std(log2[:, 0]) * 100:.2f} | '
          f'f1 macro {np.mean(log2[:, 1]) * 100:.2f} ± {np.std(log2[:, 0]) * 100:.2f} | '
          f'Flop saving {np.mean(log2[:, 2]):.2f} ± {np.std(log2[:, 2]):.2f}M | '
          f'Branch selection ratio {np.mean(log1):.3f} ± {np.std(log1):.3f}')
    idx = np.argmax(log2[:, 1])
    print('Best result', log2[idx, :])
    return log1, log2


if __name__ == '__main__':
    main()

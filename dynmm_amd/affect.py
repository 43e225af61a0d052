"""python -m dynmm_amd.affect [--hard-gate] [--reg R] [--freeze] [--infer-mode N] [--eval-only] [--model v2|v1] ...

Counterpart of ModalityDynMM/affect/affect_dyn.py: train the CMU-MOSEI DynMM (Supervised_Learning.train, regression branch
with moe_model: AdamW, L1Loss + reg * gate regulariser, clip_grad_norm_(8), validation loss per epoch, the best (lowest) model
saved, early stop when patience > 7), then test the best model on the validation and the test split with
Supervised_Learning.single_test's "posneg-classification" protocol (Accuracy, Loss, Corr; counts on the device) and print the
reference's per-run and summary lines with FLOPs (cal_flop) and the branch selection ratio (weight_stat).

Data: --data-dir holding {train,valid,test}.npz with `visual` [N,50,35], `audio` [N,50,74], `text` [N,50,300] and `label`
[N,1] (the reference's pickle needs MultiBench's get_dataloader), or --dataset synthetic.  Pretrained experts: --log-dir
holding state_dicts under the reference's names (affect_dyn.py:211): b1_reg_transformer_encoder_text.pt,
b1_reg_transformer_head_text.pt and b2_lf_tran.pt (--model v1: reg_transformer_{encoder,head}_{visual,audio,text}.pt).
run(args, model, loaders) serves a caller's own data."""
import argparse
import copy
import os

import numpy as np
import torch

from . import ops_seq as S
from .nn import affect as A

T_STEPS = 50
MODALITIES = ('visual', 'audio', 'text')


def parser():
    p = argparse.ArgumentParser('affect', formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('--gpu', type=int, default=0, help='which gpu to use')
    p.add_argument('--data', type=str, default='mosei', help='dataset: mosi / mosei')
    p.add_argument('--n-runs', type=int, default=1, help='number of runs')
    p.add_argument('--enc', type=str, default='transformer', help='gru / transformer (only transformer is implemented)')
    p.add_argument('--n-epochs', type=int, default=50, help='number of epochs')
    p.add_argument('--temp', type=float, default=1, help='temperature')
    p.add_argument('--hard-gate', action='store_true', help='hard gates')
    p.add_argument('--reg', type=float, default=0.0, help='reg loss weight')
    p.add_argument('--lr', type=float, default=1e-6, help='learning rate')
    p.add_argument('--wd', type=float, default=1e-4, help='weight decay')
    p.add_argument('--infer-mode', type=int, default=0, help='inference mode')
    p.add_argument('--eval-only', action='store_true', help='no training')
    p.add_argument('--freeze', action='store_true', help='freeze other parts of the model')
    p.add_argument('--model', choices=['v2', 'v1'], default='v2',
                   help='v2: DynMMNetV2 (text expert / late-fusion expert); v1: DynMMNet (three uni-modal experts)')
    p.add_argument('--no-pretrain', action='store_true', help='random experts instead of the state_dicts in --log-dir')
    p.add_argument('--dataset', choices=['npz', 'synthetic'], default='npz',
                   help='data source (synthetic: random experts when --log-dir holds none)')
    p.add_argument('--data-dir', type=str, default='./data/mosei', help='{train,valid,test}.npz')
    p.add_argument('--log-dir', type=str, default='./log/mosei', help='expert state_dicts')
    p.add_argument('--batch-size', type=int, default=128)
    p.add_argument('--synthetic-size', type=int, default=512, help='training samples of --dataset synthetic')
    p.add_argument('--seed', type=int, default=0)
    return p


class Loader:
    """Batches of ([[visual, audio, text], [lengths x 3]], label [B, 1]) — the reference's packed layout; the features and
    labels live on the device, the lengths (all T: the aligned MOSEI features) on the host.  Shuffled per epoch when
    `shuffle`."""

    def __init__(self, visual, audio, text, label, batch_size, shuffle, device, seed=0):
        self.x = [torch.as_tensor(np.ascontiguousarray(m), dtype=torch.float32).to(device) for m in (visual, audio, text)]
        self.y = torch.as_tensor(np.asarray(label), dtype=torch.float32).reshape(-1, 1).to(device)
        n = self.y.shape[0]
        if any(m.shape[0] != n or m.dim() != 3 for m in self.x):
            raise ValueError(f'expected [N, T, F] features and N labels, got {[tuple(m.shape) for m in self.x]}, {n}')
        self.lengths = torch.full((n,), self.x[0].shape[1], dtype=torch.long)
        self.bs, self.shuffle = batch_size, shuffle
        self.g = torch.Generator().manual_seed(seed)

    def __len__(self):
        return (self.y.shape[0] + self.bs - 1) // self.bs

    def __iter__(self):
        n = self.y.shape[0]
        idx = torch.randperm(n, generator=self.g) if self.shuffle else None
        for s in range(0, n, self.bs):
            if idx is None:
                j = slice(s, s + self.bs)
                yield [[m[j] for m in self.x], [self.lengths[j]] * 3], self.y[j]
            else:
                jh = idx[s:s + self.bs]
                jd = jh.to(self.y.device)
                yield [[m[jd] for m in self.x], [self.lengths[jh]] * 3], self.y[jd]


def synthetic_split(n, seed):
    """Features with a learnable sentiment signal: the label is a squashed random projection of the time-averaged text and
    audio features, in the reference's [-3, 3] range."""
    g = np.random.default_rng(seed)
    feats = [g.standard_normal((n, T_STEPS, A.FEATURES[m])).astype(np.float32) for m in MODALITIES]
    wa = np.random.default_rng(1234).standard_normal(A.FEATURES['audio']).astype(np.float32)
    wt = np.random.default_rng(4321).standard_normal(A.FEATURES['text']).astype(np.float32)
    score = feats[2].mean(1) @ wt + 0.5 * feats[1].mean(1) @ wa
    label = 3 * np.tanh(score / score.std()).astype(np.float32)
    return (*feats, label.reshape(n, 1))


def load_data(args, device):
    if args.dataset == 'synthetic':
        n = args.synthetic_size
        splits = [synthetic_split(n, args.seed + 1), synthetic_split(max(n // 4, 2), args.seed + 2),
                  synthetic_split(max(n // 4, 2), args.seed + 3)]
    else:
        splits = []
        for name in ('train', 'valid', 'test'):
            d = np.load(os.path.join(args.data_dir, name + '.npz'))
            splits.append((d['visual'], d['audio'], d['text'], d['label']))
    return [Loader(*s, args.batch_size, shuffle=(k == 0), device=device, seed=args.seed) for k, s in enumerate(splits)]


def expert_files(kind):
    """attribute path -> file name under --log-dir (affect_dyn.py:211 for v2, the commented-out list at :206-209 for v1)."""
    if kind == 'v2':
        enc = 'b1_reg_transformer_encoder_text.pt'
        return {'text_encoder': enc, 'text_head': enc.replace('encoder', 'head'), 'branch2': 'b2_lf_tran.pt'}
    files = {}
    for i, m in enumerate(MODALITIES):
        enc = f'reg_transformer_encoder_{m}.pt'
        files[f'encoders.{i}'] = enc
        files[f'heads.{i}'] = enc.replace('encoder', 'head')
    return files


def load_pretrained(model, log_dir, kind='v2'):
    """The reference's pretrained experts, as state_dicts (a pickled MultiBench module cannot be unpickled without it)."""
    for attr, fname in expert_files(kind).items():
        path = os.path.join(log_dir, fname)
        try:
            sd = torch.load(path, map_location='cpu', weights_only=True)
        except Exception as e:
            raise RuntimeError(f'{path}: expected a state_dict; a pickled MultiBench module cannot be loaded without '
                               f'MultiBench: export it with torch.save(torch.load(path).state_dict(), path) ({e})') from e
        model.get_submodule(attr).load_state_dict(sd)


def evaluate(model, loader, form='test', lossw=0.0):
    """One evaluation pass with the reference's posneg protocol, counts and loss on the device, one host read:
    {'Accuracy', 'Loss', 'Corr'}.  form 'test': single_test with L1Loss(reduction='sum'); 'valid': train's validation
    objective (mean L1 + lossw * gate regulariser) — see ops_seq.PosnegCounts."""
    counts = None
    model.eval()
    with torch.no_grad():
        for inputs, y in loader:
            out, aux = model(inputs)
            if counts is None:
                counts = S.PosnegCounts(y.device, form, lossw)
            counts.add(out, y, aux)
    return counts.metrics()


def test(model, loader):
    """single_test(..., task='posneg-classification') with its print line."""
    r = evaluate(model, loader, 'test')
    print(f"Loss: {r['Loss']:.4f} | Accuracy {r['Accuracy'] * 100:.2f} | Corr {r['Corr']:.3f}")
    return r


def train(args, model, loaders, save=None):
    """Supervised_Learning.train (moe_model, additional_loss, task "regression", AdamW, L1Loss, early_stop): returns the
    per-epoch mean training objective and the best model's state_dict."""
    train_loader, valid_loader = loaders[0], loaders[1]
    step = A.AffectTrainStep(model, lr=args.lr, weight_decay=args.wd, lossw=args.reg)
    best, patience, best_sd, history = float('inf'), 0, None, []
    for epoch in range(args.n_epochs):
        model.train()
        tot, nb = torch.zeros(1, device=step.flat_g.device), 0
        for inputs, y in train_loader:
            last = step(inputs, y)
            tot += last['total'] * y.shape[0]
            nb += y.shape[0]
        loss = float(tot.item()) / max(nb, 1)
        history.append(loss)
        model.reset_weight()
        vloss = evaluate(model, valid_loader, 'valid', args.reg)['Loss']
        model.weight_stat()
        print(f'Epoch {epoch} | train loss {loss:.3f} | valid loss {vloss:.3f}')
        if vloss < best:
            patience, best = 0, vloss
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
    """One run of affect_dyn.py's main loop on the caller's model and loaders ([train, valid, test] iterables of
    ([[visual, audio, text], lengths], label) device batches): train unless args.eval_only, restore the best model, test it on
    the validation and the test split.  Returns (Accuracy, Loss, Corr, FLOPs, branch selection ratio, training history)."""
    history = []
    model.hard_gate = args.hard_gate
    if not args.eval_only:
        history, best_sd = train(args, model, loaders, getattr(args, 'save', None))
        if best_sd is not None:
            model.load_state_dict(best_sd)
    model.infer_mode = args.infer_mode
    print('-' * 30 + 'Val data' + '-' * 30)
    test(model, loaders[1])
    model.reset_weight()
    print('-' * 30 + 'Test data' + '-' * 30)
    r = test(model, loaders[2])
    return r['Accuracy'], r['Loss'], r['Corr'], model.cal_flop(), model.weight_stat(), history


def build_model(args):
    if args.model == 'v2':
        return A.DynMMNetV2(args.temp, args.hard_gate, args.freeze)
    return A.DynMMNet(args.temp, args.hard_gate, freeze=args.freeze)


def main(argv=None):
    args = parser().parse_args(argv)
    if args.enc != 'transformer':
        raise NotImplementedError(f'--enc {args.enc}: the driver switch is not wired yet (only the transformer experts are '
                                  f'gated from the command line); the gru experts themselves run on the HIP path: '
                                  f'dynmm_amd.nn.affect.GRU, experts.affect_uni_gru / affect_mm_gru')
    torch.cuda.set_device(args.gpu)
    device = torch.device('cuda', args.gpu)
    loaders = load_data(args, device)
    log = np.zeros((args.n_runs, 5))
    for n in range(args.n_runs):
        torch.manual_seed(args.seed + n)
        model = build_model(args)
        files = [os.path.join(args.log_dir, f) for f in expert_files(args.model).values()]
        if args.dataset == 'synthetic' and not any(os.path.exists(f) for f in files):
            print(f'no expert state_dicts in {args.log_dir}: synthetic run with random experts')
        elif not args.no_pretrain:
            load_pretrained(model, args.log_dir, args.model)
        model = model.to(device)
        os.makedirs(os.path.join('./log', args.data), exist_ok=True)
        prefix = 'dyn' if args.model == 'v2' else 'dynv1'
        args.save = os.path.join('./log', args.data, f'{prefix}_enc_{args.enc}_reg_{args.reg}freeze{args.freeze}.pt')
        if args.eval_only:
            model.load_state_dict(torch.load(args.save, map_location=device, weights_only=True))
        print(f'Testing model {args.save}:')
        acc, loss, corr, flop, ratio, _ = run(args, model, loaders)
        log[n] = acc, loss, corr, flop, ratio
    for k in range(5):
        print(log[:, k])
    print('-' * 60)
    print(f'Finish {args.n_runs} runs')
    print(f'Test Accuracy {np.mean(log[:, 0]) * 100:.2f} ± {np.std(log[:, 0]) * 100:.2f}')
    print(f'Loss {np.mean(log[:, 1]):.4f} ± {np.std(log[:, 1]):.4f}')
    print(f'Corr {np.mean(log[:, 2]):.4f} ± {np.std(log[:, 2]):.4f}')
    print(f'FLOP {np.mean(log[:, 3]):.2f} ± {np.std(log[:, 3]):.2f}')
    print(f'Ratio {np.mean(log[:, 4]):.3f} ± {np.std(log[:, 4]):.2f}')
    idx = np.argmax(log[:, 1])            # (sic: the reference picks the run with the largest Loss)
    print('Best result', log[idx, :])
    return log


if __name__ == '__main__':
    main()

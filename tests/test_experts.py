"""Step I of the modality-level DynMM: the expert trainers (dynmm_amd.imdb_uni / imdb_mm / affect_uni / affect_mm, protocols
and ExpertTrainStep in dynmm_amd.experts, the single-head objective kernel of csrc/expert_loss.hip).
CPU: the CLIs' defaults against the reference scripts' argparse defaults, the refused variants, the file contract against
the Step II loaders (strict=True), the early-stop / best-model bookkeeping.  GPU: the objective kernel against torch fp64,
one train step per expert kind against the oracles with the same dropout masks, and Step I -> Step II end to end."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import imdb_oracle as IO
from tests.parity import Masks as _Masks, check_adam_params, randomize_bn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argparse defaults of ModalityDynMM/multimedia/imdb_uni.py, imdb_mm.py, affect/affect_uni.py, affect_mm.py, plus the epoch
# counts their train() calls hard-code (1000, 1000, 100, 1000)
REFERENCE_DEFAULTS = {
    'imdb_uni': {'gpu': 0, 'n_runs': 1, 'mod': 0, 'eval_only': False, 'measure': False, 'n_epochs': 1000},
    'imdb_mm': {'gpu': 0, 'n_runs': 1, 'fuse': 0, 'eval_only': False, 'measure': False, 'n_epochs': 1000},
    'affect_uni': {'gpu': 0, 'n_runs': 1, 'mod': 2, 'enc': 'transformer', 'hidden_dim1': 0, 'hidden_dim2': 0,
                   'data': 'mosei', 'lr': 1e-4, 'clf': False, 'eval_only': False, 'measure': False, 'n_epochs': 100},
    'affect_mm': {'gpu': 0, 'data': 'mosei', 'n_runs': 1, 'fusion': 3, 'lr': 1e-4, 'wd': 1e-4, 'eval_only': False,
                  'measure': False, 'n_epochs': 1000},
}
COMMON = {'dataset': 'npz', 'batch_size': 128, 'seed': 0}


def _cli(name):
    import importlib
    return importlib.import_module(f'dynmm_amd.{name}')


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(REFERENCE_DEFAULTS))
def test_parser_defaults_equal_the_reference_scripts(name):
    args = vars(_cli(name).parser().parse_args([]))
    for k, v in {**REFERENCE_DEFAULTS[name], **COMMON}.items():
        assert args[k] == v, (name, k, args[k], v)
    log_dir = './log/imdb' if name.startswith('imdb') else './log/mosei'
    assert args['log_dir'] == log_dir


@pytest.mark.parametrize('name,argv,words', [
    ('imdb_mm', ['--fuse', '2'], 'LowRankTensorFusion'),
    ('imdb_mm', ['--fuse', '3'], 'MultiplicativeInteractions2Modal'),
    ('affect_uni', ['--enc', 'gru'], 'GRU'),
    ('affect_uni', ['--clf'], 'CrossEntropyLoss'),
    ('affect_mm', ['--fusion', '0'], 'GRU'),
    ('affect_mm', ['--fusion', '1'], 'GRU'),
    ('affect_mm', ['--fusion', '5'], 'GRU'),
    ('affect_mm', ['--fusion', '4'], 'MULT'),
    ('affect_mm', ['--fusion', '2'], 'Transformer(409, 300)'),
])
def test_refused_variants_name_the_missing_piece(name, argv, words):
    with pytest.raises(NotImplementedError, match=re.escape(words)):
        _cli(name).main(argv + ['--dataset', 'synthetic'])


def _fill(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for t in module.state_dict().values():
            if t.dtype.is_floating_point:
                t.copy_(torch.randn(t.shape, generator=g))


def _step1_files(tmp):
    """Every file the four trainers write, through their own save paths; returns {path: state_dict written}."""
    from dynmm_amd import affect_mm, affect_uni, experts as E, imdb_mm, imdb_uni
    written = {}

    def save(module, *paths):
        E.save_state(module, *paths)
        for p in paths:
            written[p] = torch.load(p, weights_only=True)

    for mod in (0, 1):
        enc, head = E.imdb_uni(mod)
        _fill(enc, mod)
        _fill(head, 10 + mod)
        fe, fh = imdb_uni.file_names(tmp, mod)
        save(enc, fe)
        save(head, fh)
    for fuse in (1, 0):
        model, _ = E.imdb_mm(fuse)
        _fill(model, 20 + fuse)
        save(model, imdb_mm.file_name(tmp, fuse))
    for mod in (0, 1, 2):
        enc, head, name = E.affect_uni(mod)
        _fill(enc, 30 + mod)
        _fill(head, 40 + mod)
        fe, fh, copies = affect_uni.file_names(tmp, name)
        save(enc, fe, *copies[:1])
        save(head, fh, *copies[1:])
    model = E.affect_mm(3)
    _fill(model, 50)
    save(model, *affect_mm.file_names(tmp, 3))
    return written


def test_written_state_dicts_load_strictly_into_step2(tmp_path):
    from dynmm_amd import affect, imdb
    from dynmm_amd.nn import affect as A
    from dynmm_amd.nn import imdb as I
    tmp = str(tmp_path)
    written = _step1_files(tmp)
    names = sorted(os.path.basename(p) for p in written)
    assert names == sorted(['encoder_text.pt', 'head_text.pt', 'encoder_image.pt', 'head_image.pt', 'best_lf.pt', 'best_ef.pt',
                            'reg_transformer_encoder_visual.pt', 'reg_transformer_head_visual.pt',
                            'reg_transformer_encoder_audio.pt', 'reg_transformer_head_audio.pt',
                            'reg_transformer_encoder_text.pt', 'reg_transformer_head_text.pt',
                            'b1_reg_transformer_encoder_text.pt', 'b1_reg_transformer_head_text.pt', 'lf_tran.pt',
                            'b2_lf_tran.pt'])
    checks = []
    m = I.DynMMNet()
    imdb.load_pretrained(m, tmp)                           # load_state_dict(strict=True)
    checks += [(m.text_encoder, 'encoder_text.pt'), (m.text_head, 'head_text.pt'), (m.image_encoder, 'encoder_image.pt'),
               (m.image_head, 'head_image.pt'), (m.branch3, 'best_lf.pt')]
    for kind, model in (('v2', A.DynMMNetV2()), ('v1', A.DynMMNet())):
        affect.load_pretrained(model, tmp, kind)
        checks += [(model.get_submodule(a), f) for a, f in affect.expert_files(kind).items()]
    for module, fname in checks:
        sd_file = written[os.path.join(tmp, fname)]
        sd = module.state_dict()
        assert list(sd) == list(sd_file), fname
        for k in sd:
            assert sd[k].shape == sd_file[k].shape and torch.equal(sd[k], sd_file[k]), (fname, k)
    # the ef expert: identity encoders (no parameters) and the MaxOut_MLP head under MMDL's keys
    ef = written[os.path.join(tmp, 'best_ef.pt')]
    assert all(k.startswith('head.') for k in ef) and ef['head.op0.weight'].shape == (4396,)
    assert ef['head.hid2val.weight'].shape == (23, 512)


class _FakeStep:
    """Stands in for ExpertTrainStep: one 'step' marks the model's weight with the epoch number."""

    def __init__(self, model):
        self.model, self.epoch = model, 0
        self.loss_acc = torch.zeros(1, dtype=torch.float64)
        self.has_bn = False

        class _Opt:
            def check_finite(self):
                pass
        self.opt = _Opt()

    def __call__(self, inputs, y):
        with torch.no_grad():
            self.model.weight.fill_(float(self.epoch))
        self.loss_acc += 1.0 * y.shape[0]


def _scripted_run(monkeypatch, tmp_path, objective, metrics, n_epochs=100):
    from dynmm_amd import experts as E
    model = nn.Linear(1, 1, bias=False)
    step = _FakeStep(model)
    seq = iter(metrics)

    def fake_eval(*a, **k):
        step.epoch += 1                        # the next epoch's steps write the next number
        v = next(seq)
        return (0.0, v, 0.0) if objective == 'bce' else {'Loss': v, 'Accuracy': 0.0, 'Corr': 0.0}

    monkeypatch.setattr(E, 'evaluate_multilabel' if objective == 'bce' else 'evaluate_posneg', fake_eval)
    path = str(tmp_path / 'best.pt')
    saves = []

    def save():
        saves.append(step.epoch - 1)
        E.save_state(model, path)

    loader = [(None, torch.zeros(4, 1))]
    history, stopper, best_sd = E.train(model, [loader, None], lambda x: x, objective, 1e-3, 0.0, n_epochs, save, step=step)
    saved = torch.load(path, weights_only=True)['weight'].item()
    return history, stopper, best_sd, saves, saved


def test_early_stop_multilabel_ties_do_not_improve(monkeypatch, tmp_path):
    # F1-macro: 0 never beats the initial best (0); 0.5 at epoch 1; a tie at 0.5 is no improvement; 0.6 at epoch 3; then
    # 8 epochs without a strict improvement (ties included) end the run after the 8th
    metrics = [0.0, 0.5, 0.5, 0.6] + [0.6, 0.1, 0.6, 0.2, 0.6, 0.3, 0.6, 0.6] + [0.9] * 5
    history, stopper, best_sd, saves, saved = _scripted_run(monkeypatch, tmp_path, 'bce', metrics)
    assert saves == [1, 3]
    assert len(history) == 12                      # epochs 0..11: patience 8 > 7 after epoch 11
    assert stopper.best == 0.6 and stopper.best_epoch == 3 and stopper.patience == 8
    assert saved == 3.0 and best_sd['weight'].item() == 3.0           # the model of the best epoch


def test_early_stop_regression_lower_is_better(monkeypatch, tmp_path):
    # validation loss: strictly less improves; 10000 (the reference's initial best) does not
    metrics = [10000.0, 2.0, 2.0, 1.5, 1.7] + [1.5] * 7 + [0.1]
    history, stopper, best_sd, saves, saved = _scripted_run(monkeypatch, tmp_path, 'l1', metrics)
    assert saves == [1, 3]
    assert len(history) == 12 and stopper.patience == 8
    assert saved == 3.0 and best_sd['weight'].item() == 3.0


def test_early_stop_bookkeeping_alone():
    from dynmm_amd import experts as E
    s = E.EarlyStop('max')
    assert not s.update(0, 0.0) and s.patience == 1
    assert s.update(1, 0.1) and s.patience == 0
    for e in range(7):
        assert not s.update(2 + e, 0.1)
        assert not s.stop
    assert not s.update(9, 0.05) and s.stop and s.best_epoch == 1
    with pytest.raises(ValueError):
        E.EarlyStop('best')


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['bce', 'l1'])
@pytest.mark.parametrize('B', [1, 7, 128, 300])
@pytest.mark.parametrize('C', [1, 23])
def test_head_loss_kernel_against_fp64(kind, B, C):
    from dynmm_amd import ops_mlp as M
    g = torch.Generator().manual_seed(B * 31 + C)
    x = torch.randn(B, C, generator=g) * 4
    x.view(-1)[::5] = 80.0 * torch.sign(torch.randn(x.view(-1)[::5].shape, generator=g))   # saturated logits, |x| = 80
    y = (torch.rand(B, C, generator=g) < 0.4).float() if kind == 'bce' else torch.randn(B, C, generator=g) * 3
    if kind == 'l1':
        y.view(-1)[:1] = x.view(-1)[:1]                   # a tie: torch's sign(0) = 0 seed
    xd = x.double().requires_grad_(True)
    ref = (nn.BCEWithLogitsLoss() if kind == 'bce' else nn.L1Loss())(xd, y.double())
    ref.backward()
    gr = xd.grad
    if kind == 'bce':
        # torch's fp64 backward forms sigmoid(x) - y, which rounds to 0 at x = 80, y = 1 (the true seed is -1.8e-35 / (B C));
        # the same derivative in a form without that cancellation is the reference, and torch's agrees with it elsewhere
        xs, yd = x.double(), y.double()
        exact = ((1 - yd) * torch.sigmoid(xs) - yd * torch.sigmoid(-xs)) / x.numel()
        assert ((gr - exact).abs() <= 1e-9 * exact.abs() + 1e-30).all()
        gr = exact
    acc = torch.zeros(1, device='cuda', dtype=torch.float64)
    loss, seed = M.head_loss(x.cuda(), y.cuda(), kind, loss_acc=acc)
    loss2, seed2 = M.head_loss(x.cuda(), y.cuda(), kind, loss_acc=acc)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(seed).all()
    assert abs(loss.item() - ref.item()) <= 1e-6 * abs(ref.item()), (loss.item(), ref.item())
    # (plus an absolute 1e-40: a saturated logit's seed, ~1e-35 / (B C), is an fp32 subnormal)
    err = (seed.cpu().double() - gr).abs() - 1e-6 * gr.abs()
    assert (err <= 1e-40).all(), err.max().item()
    if kind == 'l1':
        assert seed.view(-1)[0].item() == 0.0
    assert torch.equal(loss, loss2) and torch.equal(seed, seed2)          # deterministic
    assert abs(acc.item() - 2 * loss.item() * B) <= 1e-12 * max(1.0, acc.item())
    # without a seed buffer (evaluation) the loss alone
    l3, s3 = M.head_loss(x.cuda(), y.cuda(), kind, seed=False)
    assert s3 is None and torch.equal(l3, loss)


def _imdb_pair(kind):
    """(mine, oracle fp64, input adapter) of an MM-IMDB expert kind."""
    from dynmm_amd import experts as E
    torch.manual_seed(5)
    if kind in ('text', 'image'):
        mod = 0 if kind == 'text' else 1
        mine = nn.Sequential(*E.imdb_uni(mod))
        ref = nn.Sequential(IO.MLP(300, 512, 512) if mod == 0 else IO.MLP(4096, 1024, 512), IO.MLP(512, 512, 23))
        adapt = lambda x: x[mod]                                              # noqa: E731
    elif kind == 'lf':
        mine, _ = E.imdb_mm(1)
        ref = IO.MMDL([IO.MaxOut_MLP(512, 512, 300, linear_layer=False, tag='encoders.0'),
                       IO.MaxOut_MLP(512, 1024, 4096, 512, False, tag='encoders.1')], IO.Concat(), IO.Linear(1024, 23))
        adapt = lambda x: x                                                   # noqa: E731
    else:
        mine, _ = E.imdb_mm(0)
        ref = IO.MMDL([nn.Identity(), nn.Identity()], IO.Concat(), IO.MaxOut_MLP(23, 512, 4396, tag='head'))
        adapt = lambda x: x                                                   # noqa: E731
    randomize_bn(ref, 3)
    mine.load_state_dict(ref.state_dict())
    return mine.cuda(), ref.double(), adapt


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['text', 'image', 'lf', 'ef'])
def test_imdb_expert_train_step_against_oracle(kind):
    from dynmm_amd import experts as E
    from dynmm_amd import ops_seq as S
    from dynmm_amd.nn import imdb as I
    mine, ref, adapt = _imdb_pair(kind)
    B, lr, wd = 128, 1e-3, 1e-2
    mine.train()
    ref.train()
    step = E.ExpertTrainStep(mine, 'bce', lr=lr, weight_decay=wd)
    params_r = list(ref.parameters())
    opt = torch.optim.AdamW(params_r, lr=lr, weight_decay=wd)
    names = [n for n, _ in ref.named_parameters()]
    table = {}
    prev = S.MASKS
    S.MASKS = lambda name, shape: table.get(name)
    try:
        for it in range(2):
            g = torch.Generator().manual_seed(20 + it)
            x = [torch.randn(B, 300, generator=g), torch.rand(B, 4096, generator=g)]
            y = (torch.rand(B, 23, generator=g) < 0.3).float()
            table.clear()
            IO.MASKS.clear()
            for name, m in mine.named_modules():
                if isinstance(m, I.MaxOut_MLP):
                    for site, width in (('op2', m.op2[0].num_features), ('op4', m.op4[0].num_features)):
                        k = (torch.rand(B, width, generator=g) >= 0.3).to(torch.uint8)
                        IO.MASKS[f'{name}.{site}'] = k
                        table[f'{name}.{site}'] = k.cuda()
            last = step(adapt([t.cuda() for t in x]), y.cuda())
            opt.zero_grad()
            loss_r = nn.functional.binary_cross_entropy_with_logits(ref(adapt([t.double() for t in x])), y.double())
            loss_r.backward()
            gn = torch.nn.utils.clip_grad_norm_(params_r, 8.0)
            opt.step()
            tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
            assert abs(last['loss'].item() - loss_r.item()) < tol, (kind, it, last['loss'].item(), loss_r.item())
            assert abs(last['grad_norm'].item() - gn.item()) < 1e-3 * gn.item(), (kind, it, last['grad_norm'].item(), gn.item())
    finally:
        S.MASKS = prev
        IO.MASKS.clear()
    torch.cuda.synchronize()
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, kind, names)
    sd, sd_r = mine.state_dict(), ref.state_dict()
    for k in sd:
        if 'running_' in k:
            a, b = sd[k].cpu().double(), sd_r[k].double()
            assert ((a - b).abs().max() / b.abs().max()).item() < 1e-4, k
        if 'num_batches_tracked' in k:
            assert int(sd[k]) == int(sd_r[k]) == 2, k


def _affect_pair(kind):
    from dynmm_amd import experts as E
    from oracle import affect_oracle as O
    if kind == 'lf_tran':
        ref = O.fill_(O.MMDL([O.Transformer(35, 60), O.Transformer(74, 120), O.Transformer(300, 120)], O.Concat(),
                             O.MLP(300, 128, 1)), seed=4)
        mine = E.affect_mm(3)
        adapt = lambda x: x                                                   # noqa: E731
    else:
        mod = 2 if kind == 'text' else 0
        enc, head, _ = E.affect_uni(mod)
        mine = nn.Sequential(enc, head)
        ref = O.fill_(nn.Sequential(O.Transformer((35, 74, 300)[mod], 120), O.MLP(120, 64, 1)), seed=4)
        adapt = lambda x: [x[0][mod], x[1][mod]]                              # noqa: E731
    mine.load_state_dict(ref.state_dict())
    return mine.cuda(), ref, adapt


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['text', 'visual', 'lf_tran'])
def test_affect_expert_train_step_against_oracle(kind):
    """Training mode, dropout p = 0.1 at every encoder layer's four sites with the same keep flags on both sides."""
    from dynmm_amd import experts as E
    from dynmm_amd import ops_seq as S
    from oracle import affect_oracle as O
    mine, ref, adapt = _affect_pair(kind)
    mine.train()
    ref.train()
    lr, wd = 1e-3, 1e-2
    step = E.ExpertTrainStep(mine, 'l1', lr=lr, weight_decay=wd)
    params_r = list(ref.parameters())
    opt = torch.optim.AdamW(params_r, lr=lr, weight_decay=wd)
    names = [n for n, _ in ref.named_parameters()]
    try:
        for it in range(2):
            inputs, y = O.synth_batch(6, seed=10 + it)
            mr, mh = _Masks(0.1, 40 + it), _Masks(0.1, 40 + it, 'cuda')
            O.Transformer.dropout_masks = (0.1, mr)
            S.MASKS = mh
            opt.zero_grad()
            loss_r = nn.functional.l1_loss(ref(adapt(inputs)), y)
            loss_r.backward()
            gn = torch.nn.utils.clip_grad_norm_(params_r, 8.0)
            opt.step()
            last = step(adapt([[x.cuda() for x in inputs[0]], inputs[1]]), y.cuda())
            torch.cuda.synchronize()
            assert mr.n == mh.n > 0
            tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
            assert abs(last['loss'].item() - loss_r.item()) < tol, (kind, it, last['loss'].item(), loss_r.item())
            assert abs(last['grad_norm'].item() - gn.item()) < 2e-3 * max(gn.item(), 1e-3), (kind, it, last['grad_norm'].item(),
                                                                                            gn.item())
    finally:
        O.Transformer.dropout_masks = None
        S.MASKS = None
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, kind, names)


@pytest.mark.gpu
def test_affect_expert_graph_replay_equals_eager():
    """ExpertTrainStep(use_graph=True) on a transformer expert: the same losses, norms and weights as the eager step (dropout
    off on both copies: their dropout sites differ)."""
    from dynmm_amd import experts as E
    from oracle import affect_oracle as O
    a, _, adapt = _affect_pair('text')
    b, _, _ = _affect_pair('text')
    a.eval()
    b.eval()
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = O.synth_batch(8, seed=60 + it)
        x = adapt([[t.cuda() for t in inputs[0]], inputs[1]])
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert abs(sa.loss_acc.item() - sb.loss_acc.item()) <= 1e-6 * sa.loss_acc.item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k


def _run(args, cwd, timeout=600):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, '-m'] + args, cwd=str(cwd), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, ' '.join(args) + '\n' + r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _assert_experts_hold(ckpt, log_dir, parts):
    """The Step II model saved in `ckpt` holds, under each attribute prefix, the trainable tensors of the Step I file."""
    sd = torch.load(ckpt, map_location='cpu', weights_only=True)
    for prefix, fname in parts.items():
        f = torch.load(os.path.join(log_dir, fname), map_location='cpu', weights_only=True)
        for k, v in f.items():
            if 'running_' in k or 'num_batches_tracked' in k:
                continue                           # BatchNorm statistics still move in a frozen expert's training forward
            assert torch.equal(sd[f'{prefix}.{k}'], v), (fname, k)


def _imdb_npz(d):
    """{train,valid,test}.npz in the MM-IMDB layout with mostly-positive labels: within a step or two every expert predicts
    positives, so validation F1-macro leaves 0 (the initial best) and every trainer writes its files."""
    g = np.random.default_rng(7)
    os.makedirs(d)
    for name, n in (('train', 512), ('valid', 128), ('test', 128)):
        np.savez(os.path.join(d, name + '.npz'), text=g.standard_normal((n, 300)).astype(np.float32),
                 image=np.abs(g.standard_normal((n, 4096))).astype(np.float32),
                 label=(g.random((n, 23)) < 0.8).astype(np.float32))


@pytest.mark.gpu
def test_imdb_step1_then_step2_end_to_end(tmp_path):
    log = tmp_path / 'experts'
    data = str(tmp_path / 'data')
    _imdb_npz(data)
    common = ['--data-dir', data, '--n-epochs', '2', '--log-dir', str(log)]
    for mod in ('0', '1'):
        out = _run(['dynmm_amd.imdb_uni', '--mod', mod] + common, tmp_path)
        assert re.search(r'f1 micro [0-9.]+ ± [0-9.]+\nf1 macro [0-9.]+ ± [0-9.]+', out), out
    out = _run(['dynmm_amd.imdb_mm', '--fuse', '1'] + common, tmp_path)
    assert 'Saving Best' in out and re.search(r'f1_micro: [0-9.]+ \| f1_macro: [0-9.]+', out), out
    assert sorted(os.listdir(log)) == sorted(['encoder_text.pt', 'head_text.pt', 'encoder_image.pt', 'head_image.pt',
                                              'best_lf.pt'])
    out = _run(['dynmm_amd.imdb', '--data-dir', data, '--log-dir', str(log), '--n-epochs', '1', '--freeze'], tmp_path)
    assert 'Test f1 micro' in out, out
    _assert_experts_hold(tmp_path / 'log' / 'imdb' / 'DynMMNet_freezeTrue_reg_0.1.pt', str(log),
                         {'text_encoder': 'encoder_text.pt', 'text_head': 'head_text.pt', 'image_encoder': 'encoder_image.pt',
                          'image_head': 'head_image.pt', 'branch3': 'best_lf.pt'})


@pytest.mark.gpu
def test_affect_step1_then_step2_end_to_end(tmp_path):
    from dynmm_amd import affect
    log = tmp_path / 'experts'
    common = ['--dataset', 'synthetic', '--n-epochs', '2', '--synthetic-size', '256', '--log-dir', str(log)]
    for mod in ('0', '1', '2'):
        out = _run(['dynmm_amd.affect_uni', '--mod', mod] + common, tmp_path)
        assert re.search(r'Test Accuracy [0-9.]+ ± [0-9.]+\nLoss [0-9.]+ ± [0-9.]+\nCorr', out), out
    out = _run(['dynmm_amd.affect_mm', '--graph'] + common, tmp_path)
    assert 'Saving Best' in out and re.search(r'Loss: [0-9.]+ \| Accuracy [0-9.]+ \| Corr', out), out
    for kind, prefix in (('v1', 'dynv1'), ('v2', 'dyn')):
        files = affect.expert_files(kind)
        assert all(os.path.exists(log / f) for f in files.values()), (kind, sorted(os.listdir(log)))
        out = _run(['dynmm_amd.affect', '--model', kind, '--dataset', 'synthetic', '--synthetic-size', '256', '--log-dir',
                    str(log), '--n-epochs', '1', '--freeze'], tmp_path)
        assert 'random experts' not in out and 'Test Accuracy' in out, out
        _assert_experts_hold(tmp_path / 'log' / 'mosei' / f'{prefix}_enc_transformer_reg_0.0freezeTrue.pt', str(log), files)

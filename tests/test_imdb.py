"""Modality-level DynMM on MM-IMDB features (ModalityDynMM/multimedia/imdb_dyn.py) — PARITY UNPINNED: the experts are
MultiBench modules the reference neither vendors nor pins, so the checker is tests/imdb_oracle.py, an fp64 restatement from
the torch.nn layers MultiBench wraps.  CPU: layout, freezing, FLOP bookkeeping, host F1, the oracle's own structure, the CLI's
defaults.  GPU: the kernels of csrc/mlp.hip and the whole model, forward, backward, train step and compacted eval, against
that oracle."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import imdb_oracle as O
from tests.parity import randomize_bn, rel

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 300, generator=g), torch.rand(B, 4096, generator=g)]


EXPECTED_FIRST_LAST = (('text_encoder.fc.weight', (512, 300)), ('gate.fc2.bias', (2,)))


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_state_dict_layout_matches_oracle_and_reference_list():
    from dynmm_amd.nn import imdb as I
    a, b = I.DynMMNet(freeze=False).state_dict(), O.DynMMNet(freeze=False).state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) and a[k].dtype == b[k].dtype for k in a)
    assert len(a) == 60
    keys = list(a.keys())
    assert (keys[0], tuple(a[keys[0]].shape)) == EXPECTED_FIRST_LAST[0]
    assert (keys[-1], tuple(a[keys[-1]].shape)) == EXPECTED_FIRST_LAST[1]
    assert tuple(a['branch3.encoders.1.op1.lin.weight'].shape) == (2048, 4096)
    assert tuple(a['branch3.encoders.0.op2.0.running_var'].shape) == (512,)
    assert tuple(a['branch3.encoders.0.op2.0.num_batches_tracked'].shape) == ()
    n = sum(v.numel() for k, v in a.items() if 'running_' not in k and 'num_batches' not in k)
    assert n == sum(p.numel() for p in I.DynMMNet().parameters()) == 16560159
    # a state_dict exported from the restated MultiBench modules loads strictly
    I.DynMMNet().load_state_dict(O.DynMMNet().state_dict())
    with pytest.raises(NotImplementedError):
        I.DynMMNet(pretrain=True)


def test_freeze_leaves_only_the_gate_trainable():
    from dynmm_amd.nn import imdb as I
    m = I.DynMMNet(freeze=True)
    assert all(p.requires_grad == n.startswith('gate.') for n, p in m.named_parameters())
    assert all(p.requires_grad for p in I.DynMMNet(freeze=False).parameters())


def test_cal_flop_and_weight_stat(capsys):
    from dynmm_amd.nn import imdb as I
    m = I.DynMMNet()
    m.reset_weight()
    m.weight_list = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [1.0, 0.0]])
    assert m.cal_flop() == pytest.approx(0.5 * 1.25261 + 0.5 * 10.86908, rel=1e-6)
    m.weight_list = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    assert m.weight_stat() == pytest.approx(0.75)
    assert not m.store_weight
    assert 'mean branch weight 0.2500, 0.7500' in capsys.readouterr().out


def test_host_f1_equals_sklearn():
    metrics = pytest.importorskip('sklearn.metrics')
    from dynmm_amd import ops_mlp as M
    rng = np.random.default_rng(0)
    for trial in range(5):
        y = (rng.random((97, 23)) < 0.15).astype(int)
        p = (rng.random((97, 23)) < 0.2).astype(int)
        y[:, 3] = 0                          # a class with no positives ...
        p[:, 3] = 0                          # ... and no predictions: 0/0 scores 0
        y[:, 5] = 0                          # no positives, some false positives
        p[:, 7] = 0                          # positives, never predicted
        tp = ((p == 1) & (y == 1)).sum(0)
        fp = ((p == 1) & (y == 0)).sum(0)
        fn = ((p == 0) & (y == 1)).sum(0)
        micro, macro = M.f1_from_counts(tp, fp, fn)
        assert micro == pytest.approx(metrics.f1_score(y, p, average='micro', zero_division=0), abs=1e-12)
        assert macro == pytest.approx(metrics.f1_score(y, p, average='macro', zero_division=0), abs=1e-12)
    assert M.f1_from_counts(np.zeros(3), np.zeros(3), np.zeros(3)) == (0.0, 0.0)


def test_oracle_maxout_mlp_is_multibench_composition():
    torch.manual_seed(0)
    O.MASKS.clear()
    for lin in (True, False):
        m = O.MaxOut_MLP(7, 16, 10, 12, linear_layer=lin, tag='t').double()
        randomize_bn(m, 1)
        for mode in ('train', 'eval'):
            getattr(m, mode)()
            O.MASKS['t.op2'] = (torch.rand(9, 16) >= 0.3).to(torch.uint8)
            O.MASKS['t.op4'] = (torch.rand(9, 12) >= 0.3).to(torch.uint8)
            x = torch.randn(9, 10, dtype=torch.float64)
            ref = copy.deepcopy(m)
            h = ref.op0(x)
            h = ref.op1.lin(h).view(9, 16, 2).max(-1)[0]
            h = ref.op2[0](h)
            if mode == 'train':
                h = h * O.MASKS['t.op2'] / 0.7
            h = ref.op3.lin(h).view(9, 12, 2).max(-1)[0]
            h = ref.op4[0](h)
            if mode == 'train':
                h = h * O.MASKS['t.op4'] / 0.7
            if lin:
                h = ref.hid2val(h)
            seq = nn.Sequential(m.op0, m.op1, m.op2, m.op3, m.op4, *([m.hid2val] if lin else []))
            assert torch.allclose(seq(x), h, rtol=0, atol=1e-12)
    mx = O.Maxout(5, 3, 2).double()
    x = torch.randn(4, 5, dtype=torch.float64)
    z = mx.lin(x)
    assert torch.equal(mx(x), torch.maximum(z[:, 0::2], z[:, 1::2]))


def test_cli_parses_reference_defaults():
    from dynmm_amd import imdb
    a = imdb.parser().parse_args([])
    assert (a.n_runs, a.data, a.n_epochs, a.lr, a.wd, a.reg) == (1, 'imdb', 50, 1e-4, 1e-2, 0.1)
    assert (a.freeze, a.eval_only, a.hard, a.no_pretrain, a.infer_mode) == (False, False, False, False, 0)
    a = imdb.parser().parse_args(['--freeze', '--hard', '--no-pretrain', '--infer-mode', '2', '--dataset', 'synthetic'])
    assert (a.freeze, a.hard, a.no_pretrain, a.infer_mode, a.dataset) == (True, True, True, 2, 'synthetic')


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def masks():
    """Injected keep flags on both sides: ours through ops_seq.MASKS (by site name), the oracle's through O.MASKS."""
    from dynmm_amd import ops_seq as S
    table = {}

    def make(B, seed=0, p=0.3):
        g = torch.Generator().manual_seed(seed)
        table.clear()
        O.MASKS.clear()
        for i, (m2, m4) in enumerate(((512, 512), (1024, 512))):
            for name, m in (('op2', m2), ('op4', m4)):
                key = f'branch3.encoders.{i}.{name}'
                k = (torch.rand(B, m, generator=g) >= p).to(torch.uint8)
                O.MASKS[key] = k
                table[key] = k.cuda()

    prev = S.MASKS
    S.MASKS = lambda name, shape: table.get(name)
    yield make
    S.MASKS = prev
    O.MASKS.clear()


def _bn_pair(m, eps, seed):
    torch.manual_seed(seed)
    bn = nn.BatchNorm1d(m, eps)
    randomize_bn(bn, seed)
    ref = copy.deepcopy(bn).double()
    return bn.cuda(), ref


@pytest.mark.gpu
@pytest.mark.parametrize('B', [128, 37])
@pytest.mark.parametrize('form,m', [('maxout', 512), ('maxout', 1024), ('op0', 300), ('op0', 4096)])
@pytest.mark.parametrize('train', [True, False])
def test_maxout_bn_kernel_against_fp64(B, form, m, train):
    from dynmm_amd import ops_mlp as M
    from dynmm_amd import ops_seq as S
    maxout = form == 'maxout'
    bn, bnr = _bn_pair(m, 1e-5 if maxout else 1e-4, seed=B + m)
    bn.train(train)
    bnr.train(train)
    prev = S.MASKS
    try:
        for call in range(2):
            g = torch.Generator().manual_seed(call)
            z = torch.randn(B, 2 * m if maxout else m, generator=g)
            keep = (torch.rand(B, m, generator=g) >= 0.3).to(torch.uint8)
            S.MASKS = lambda name, shape: keep.cuda() if name == 't' else None
            zd = z.cuda().requires_grad_(maxout)
            bn.zero_grad()
            y = M.maxout_bn(zd, bn, (0.3, S.new_sites(1), 't') if maxout else None, maxout=maxout)
            zr = z.double().requires_grad_(maxout)
            v = zr.view(B, m, 2).max(-1)[0] if maxout else zr
            yr = bnr(v)
            if maxout and train:
                yr = yr * keep.double() / 0.7
            assert rel(y, yr) < 2e-6, (call, rel(y, yr))
            gy = torch.randn(B, m, generator=g)
            y.backward(gy.cuda())
            yr.backward(gy.double())
            assert rel(bn.weight.grad, bnr.weight.grad) < 2e-5
            assert rel(bn.bias.grad, bnr.bias.grad) < 2e-5
            if maxout:
                assert rel(zd.grad, zr.grad) < 5e-5, rel(zd.grad, zr.grad)
                losing = (zr.grad == 0)
                assert bool((zd.grad.cpu()[losing] == 0).all())
            bnr.zero_grad()
    finally:
        S.MASKS = prev
    assert rel(bn.running_mean, bnr.running_mean) < 1e-5
    assert rel(bn.running_var, bnr.running_var) < 1e-5
    assert int(bn.num_batches_tracked.item()) == int(bnr.num_batches_tracked.item()) == (2 if train else 0)


@pytest.mark.gpu
def test_maxout_bn_batch_of_one_raises():
    from dynmm_amd import ops_mlp as M
    bn = nn.BatchNorm1d(64).cuda()
    with pytest.raises(ValueError):
        M.maxout_bn(torch.randn(1, 128, device='cuda'), bn, None)
    bn.eval()
    assert M.maxout_bn(torch.randn(1, 128, device='cuda'), bn, None).shape == (1, 64)


@pytest.mark.gpu
def test_maxout_bn_dropout_generator_keep_rate_and_new_masks():
    from dynmm_amd import ops_mlp as M
    from dynmm_amd import ops_seq as S
    bn = nn.BatchNorm1d(1024).cuda()
    z = torch.randn(128, 2048, device='cuda')
    site = S.new_sites(1)
    with torch.no_grad():
        y1 = M.maxout_bn(z, bn, (0.3, site, 'gen'))
        y1b = M.maxout_bn(z, bn, (0.3, site, 'gen'))
        S.advance_dropout_step(z.device)
        y2 = M.maxout_bn(z, bn, (0.3, site, 'gen'))
    d1, d2 = (y1 == 0), (y2 == 0)
    n = d1.numel()
    sd = (n * 0.3 * 0.7) ** 0.5
    for d in (d1, d2):
        assert abs(d.sum().item() - 0.3 * n) < 5 * sd
    assert torch.equal(d1, y1b == 0)                  # same step: the same decisions
    assert (d1 != d2).float().mean().item() > 0.3      # next step: new masks (independent: 2 p (1 - p) = 0.42 differ)


def _head_ref(logits, preds, y, temp, hard, reg):
    w = O.diff_softmax(logits, tau=temp, hard=hard)
    out = sum(w[:, k:k + 1] * p for k, p in enumerate(preds))
    aux = w[:, -1].mean()
    loss = nn.functional.binary_cross_entropy_with_logits(out, y)
    return out, aux, loss, loss + reg * aux, w


@pytest.mark.gpu
@pytest.mark.parametrize('hard', [False, True])
@pytest.mark.parametrize('temp', [1.0, 0.6])
def test_multilabel_head_against_fp64_autograd(hard, temp):
    from dynmm_amd import ops_mlp as M
    g = torch.Generator().manual_seed(int(hard) * 10 + int(temp * 10))
    B, K, Cc, reg = 37, 2, 23, 0.1
    lg = 3 * torch.randn(B, K, generator=g)
    preds = [30 * (2 * torch.rand(B, Cc, generator=g) - 1) for _ in range(K)]
    y = (torch.rand(B, Cc, generator=g) < 0.3).float()
    lr_, pr = lg.double().requires_grad_(), [p.double().requires_grad_() for p in preds]
    out_r, aux_r, loss_r, tot_r, w_r = _head_ref(lr_, pr, y.double(), temp, hard, reg)
    tot_r.backward()
    ld, pd = lg.cuda().requires_grad_(), [p.cuda().requires_grad_() for p in preds]
    r = M.ml_loss_backward(ld, pd, y.cuda(), temp, hard, reg)
    assert rel(r['out'], out_r) < 1e-6
    assert rel(r['weight'], w_r) < 1e-6
    assert abs(r['loss1'].item() - loss_r.item()) < 1e-5 * max(1, loss_r.item())
    assert abs(r['aux'].item() - aux_r.item()) < 1e-6
    assert abs(r['total'].item() - tot_r.item()) < 1e-5 * max(1, tot_r.item())
    for a, b in zip(pd, pr):
        assert rel(a.grad, b.grad) < 1e-5
    assert rel(ld.grad, lr_.grad) < 1e-4, rel(ld.grad, lr_.grad)
    # blend alone under plain autograd, arbitrary upstream gradients
    lr2, pr2 = lg.double().requires_grad_(), [p.double().requires_grad_() for p in preds]
    out_r, aux_r, _, _, _ = _head_ref(lr2, pr2, y.double(), temp, hard, reg)
    go = torch.randn(B, Cc, generator=g)
    (out_r * go.double()).sum().add(3 * aux_r).backward()
    ld2, pd2 = lg.cuda().requires_grad_(), [p.cuda().requires_grad_() for p in preds]
    out, aux, w = M.ml_blend(ld2, pd2, temp, hard)
    assert rel(out, out_r) < 1e-6 and abs(aux.item() - aux_r.item()) < 1e-6
    (out * go.cuda()).sum().add(3 * aux).backward()
    for a, b in zip(pd2, pr2):
        assert rel(a.grad, b.grad) < 1e-5
    assert rel(ld2.grad, lr2.grad) < 1e-4, rel(ld2.grad, lr2.grad)


@pytest.mark.gpu
def test_counts_kernel_against_numpy():
    from dynmm_amd import ops_mlp as M
    g = torch.Generator().manual_seed(3)
    counts = M.MultilabelCounts(23, 'cuda')
    tp = np.zeros(23, np.int64)
    fp, fn = tp.copy(), tp.copy()
    lsum = 0.0
    for B in (128, 37, 300):
        x = 4 * torch.randn(B, 23, generator=g)
        x[:, 0] = 0.0
        x[:5, 1], x[5:10, 1] = 1e-3, -1e-3
        y = (torch.rand(B, 23, generator=g) < 0.3).float()
        y[:, 2] = 0
        counts.add(x.cuda(), y.cuda())
        p = torch.sigmoid(x).round().numpy() > 0.5
        t = y.numpy() > 0.5
        tp += (p & t).sum(0)
        fp += (p & ~t).sum(0)
        fn += (~p & t).sum(0)
        lsum += nn.functional.binary_cross_entropy_with_logits(x.double(), y.double(), reduction='sum').item()
    r = counts.read()
    assert np.array_equal(r['tp'], tp) and np.array_equal(r['fp'], fp) and np.array_equal(r['fn'], fn)
    assert r['tp'][0] == 0 and r['fp'][0] == 0                 # sigmoid(0) = 0.5 rounds to 0
    assert r['n'] == 465
    assert r['loss'] == pytest.approx(lsum / (465 * 23), rel=1e-6)


def _pair(freeze=False, seed=0):
    from dynmm_amd.nn import imdb as I
    torch.manual_seed(seed)
    ref = O.DynMMNet(freeze=freeze)
    randomize_bn(ref, seed)
    mine = I.DynMMNet(freeze=freeze)
    mine.load_state_dict(ref.state_dict())
    return mine.cuda(), ref.double()


@pytest.mark.gpu
@pytest.mark.parametrize('B', [37, 128])
def test_dynmm_forward_against_oracle(masks, B):
    mine, ref = _pair()
    x = inputs(B, seed=B)
    xd, xr = [t.cuda() for t in x], [t.double() for t in x]
    for train in (True, False):
        for hard in (False, True):
            mine.train(train)
            ref.train(train)
            mine.hard_gate = ref.hard_gate = hard
            mine.temp = ref.temp = 0.8
            masks(B, seed=int(train) * 2 + int(hard))
            with torch.no_grad():
                snap = copy.deepcopy(ref.state_dict())
                mine.reset_weight()
                out, aux = mine(xd)
                out_r, aux_r, w_r = ref(xr)
                assert rel(out, out_r) < 1e-4, (train, hard, rel(out, out_r))
                assert abs(float(aux) - aux_r.item()) < 1e-5
                assert rel(mine.weight_list, w_r) < 1e-5
                for mode in (1, 2):
                    mine.infer_mode = ref.infer_mode = mode
                    ref.load_state_dict(snap)                       # (train mode: running stats moved by the last call)
                    mine.load_state_dict(snap)
                    p, zero = mine(xd)
                    p_r, _, _ = ref(xr)
                    assert zero == 0 and rel(p, p_r) < 1e-4, (mode, rel(p, p_r))
                mine.infer_mode = ref.infer_mode = 0
                for path in (1, 2, 3):
                    ref.load_state_dict(snap)
                    mine.load_state_dict(snap)
                    assert rel(mine.forward_separate_branch(xd, path, True), ref.forward_separate_branch(xr, path)) < 1e-4
                ref.load_state_dict(snap)
                mine.load_state_dict(snap)


# gradient bar per tensor, relative to the tensor's max |grad|: the largest measured on an MI355X over every parameter and
# input tensor, soft and hard gate, was 2.4e-6 (branch3.encoders.1.op4.0.weight, branch3.head.fc.weight); ~6x that
GRAD_BAR = 1.5e-5


@pytest.mark.gpu
@pytest.mark.parametrize('hard', [False, True])
def test_dynmm_gradients_against_oracle(masks, hard):
    from dynmm_amd import ops_mlp as M
    mine, ref = _pair(seed=1)
    B = 64
    x = inputs(B, seed=5)
    y = (torch.rand(B, 23, generator=torch.Generator().manual_seed(9)) < 0.3).float()
    masks(B, seed=11)
    mine.train()
    ref.train()
    mine.hard_gate = ref.hard_gate = hard
    xd = [t.cuda().requires_grad_() for t in x]
    xr = [t.double().requires_grad_() for t in x]
    logits, preds = mine.gate_and_experts(xd)
    r = M.ml_loss_backward(logits, preds, y.cuda(), mine.temp, hard, 0.1)
    torch.cuda.synchronize()
    out_r, aux_r, _ = ref(xr)
    tot = O.objective(out_r, aux_r, y.double(), 0.1)
    tot.backward()
    assert abs(r['total'].item() - tot.item()) < 1e-5 * max(1, tot.item())
    worst = {}
    named_r = dict(ref.named_parameters())
    for n, p in mine.named_parameters():
        pr = named_r[n]
        if pr.grad is None:
            assert p.grad is None or p.grad.abs().max().item() == 0, n       # image_encoder / image_head: unused
            continue
        worst[n] = rel(p.grad, pr.grad)
    worst['input.text'] = rel(xd[0].grad, xr[0].grad)
    worst['input.image'] = rel(xd[1].grad, xr[1].grad)
    print('gradient rel err max', max(worst.values()), max(worst, key=worst.get))
    bad = {k: v for k, v in worst.items() if not v < GRAD_BAR}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('freeze', [False, True])
def test_train_step_against_oracle_adamw(masks, freeze):
    from dynmm_amd.nn import imdb as I
    mine, ref = _pair(freeze=freeze, seed=2)
    B, lr, wd, reg = 128, 1e-3, 1e-2, 0.1
    mine.train()
    ref.train()
    mine.hard_gate = ref.hard_gate = False
    step = I.ImdbTrainStep(mine, lr=lr, weight_decay=wd, lossw=reg)
    params_r = [p for p in ref.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params_r, lr=lr, weight_decay=wd)
    names = [n for n, p in ref.named_parameters() if p.requires_grad]
    assert len(names) == sum(1 for p in mine.parameters() if p.requires_grad)
    for it in range(2):
        x = inputs(B, seed=20 + it)
        y = (torch.rand(B, 23, generator=torch.Generator().manual_seed(it)) < 0.3).float()
        masks(B, seed=30 + it)
        last = step([t.cuda() for t in x], y.cuda())
        opt.zero_grad()
        out_r, aux_r, _ = ref([t.double() for t in x])
        tot = O.objective(out_r, aux_r, y.double(), reg)
        tot.backward()
        gn = torch.nn.utils.clip_grad_norm_(params_r, 8.0)
        opt.step()
        tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(tot.item()))
        assert abs(last['total'].item() - tot.item()) < tol, (it, last['total'].item(), tot.item())
        assert abs(last['grad_norm'].item() - gn.item()) < 1e-3 * gn.item(), (it, last['grad_norm'].item(), gn.item())
    torch.cuda.synchronize()
    sd, sd_r = mine.state_dict(), ref.state_dict()
    for k in names:
        # Adam's first updates are lr * sign(g) whatever |g|: an element whose gradient is rounding noise can move the other
        # way (2 update sizes apart).  Almost every element must agree to a fraction of an update, none further than two.
        d = (sd[k].cpu().double() - sd_r[k]).abs()
        n_far = int((d > 0.2 * 2 * lr).sum().item())
        assert n_far <= max(1, int(2e-3 * d.numel())) and d.max().item() < 2.2 * 2 * lr, (freeze, k, n_far, d.max().item())
    for k in sd:
        if 'running_' in k:
            assert rel(sd[k], sd_r[k]) < 1e-4, k
        if 'num_batches_tracked' in k and k.startswith('branch3'):
            assert int(sd[k]) == int(sd_r[k]) == 2, k


@pytest.mark.gpu
def test_compacted_hard_gate_eval_equals_dense(monkeypatch):
    from dynmm_amd import ops_seq as S
    mine, _ = _pair(seed=3)
    mine.eval()
    mine.hard_gate = True
    B = 96
    x = [t.cuda() for t in inputs(B, seed=4)]
    rows = []
    real = S.linear_bdt

    def spy(xx, weight, *a, **k):
        if tuple(weight.shape) == (2048, 4096):           # branch3's image Maxout GEMM
            rows.append(xx.shape[0])
        return real(xx, weight, *a, **k)

    monkeypatch.setattr(S, 'linear_bdt', spy)
    b = mine.gate.fc2.bias
    base = b.detach().clone()
    for route, shift in (('all-text', (50.0, -50.0)), ('all-branch3', (-50.0, 50.0)), ('mixed', None)):
        with torch.no_grad():
            b.copy_(base if shift is None else torch.tensor(shift, device='cuda'))
            if shift is None:
                # about half the samples each way: centre the gate logits' difference on its median
                mine.compact = False
                lg = mine.gate(torch.cat(x, 1))
                d = (lg[:, 1] - lg[:, 0]).median()
                b[1] -= d + 1e-3
            mine.compact = False
            mine.reset_weight()
            rows.clear()
            dense, aux_d = mine(x)
            w_dense = mine.weight_list.clone()
            assert rows == [B]
            mine.compact = True
            mine.reset_weight()
            rows.clear()
            comp, aux_c = mine(x)
            w_comp = mine.weight_list.clone()
        n0, n1 = mine.last_counts
        assert torch.equal(w_dense, w_comp), route
        assert n1 == int(w_dense[:, 1].sum().item()) and n0 + n1 == B
        assert rows == ([n1] if n1 else []), (route, rows)
        if route == 'all-text':
            assert n1 == 0
        elif route == 'all-branch3':
            assert n0 == 0
        else:
            assert 0 < n1 < B
        assert float(aux_c) == float(aux_d)
        err = rel(comp, dense)
        assert err < 1e-5, (route, err)
        assert mine.cal_flop() == pytest.approx((mine.flop * w_dense.mean(0)).sum().item())


@pytest.mark.gpu
def test_cli_synthetic_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, '-m', 'dynmm_amd.imdb', '--dataset', 'synthetic', '--no-pretrain', '--n-epochs', '2',
                        '--synthetic-size', '768', '--lr', '1e-3'], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = [float(v) for v in re.findall(r'Epoch \d+ train loss: ([0-9.]+)', r.stdout)]
    assert len(losses) == 2 and losses[1] < losses[0], r.stdout
    assert re.search(r'Test f1 micro [0-9.]+ ± [0-9.]+ \| f1 macro [0-9.]+ ± [0-9.]+ \| Flop saving [0-9.]+ ± [0-9.]+M \| '
                     r'Branch selection ratio [0-9.]+ ± [0-9.]+', r.stdout), r.stdout
    assert os.path.exists(tmp_path / 'log' / 'imdb' / 'DynMMNet_freezeFalse_reg_0.1.pt')

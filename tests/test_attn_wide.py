"""Attention for head dimensions up to 64 (csrc/attn.hip, ops_seq.mha_wide / attention) and the early-fusion transformer
expert it unblocks (nn.affect.early_fusion_transformer, experts.affect_mm_ef_tran: affect_mm.py --fusion 2).

Kernel tests: the float64 restatement `ref_attention` of tests/test_seq_kernels.py and that file's bar rule — project bars
1e-5 (out, probs) and 2e-5 (dqkv) on `_rel` = max|a - b| / max|b|; a case that cannot sit under its project bar gets
max(project bar, 4 x the float32 error of the same restatement on the same inputs).  Every comparison prints its `FIG` line.
Whole-model tests: the plain-torch twin Sequential(oracle Transformer(409, 300), oracle MLP(300, 128, 1)) behind a
concatenation of the three modalities, with test_affect.py's whole-model bars.
"""
import gc

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from dynmm_amd import ops_seq as S
from dynmm_amd.ops_seq import attention, mha_wide
from tests.test_affect import _Masks
from tests.test_seq_kernels import LN_BWD, LN_FWD, _Figures, _FixedMasks, _attn_grads, _both, _cu, _gen, _ptr, _rel, ref_attention


@pytest.fixture(autouse=True)
def _leave_no_garbage():
    """Steps, captured graphs and 8 M-parameter models die with the test that made them, not in a later test's collector run
    (which may start inside that test's stream capture: ops.capture_scope)."""
    yield
    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
def test_ref_attention_is_torchs_sdpa_at_the_experts_head_dimension():
    B, dh, heads, T = 2, 60, 5, 50
    g = _gen(6050)
    D = dh * heads
    qkv = torch.randn(B, 3 * D, T, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(B, D, T, generator=g, dtype=torch.float64)
    out, probs = ref_attention(qkv, heads)
    got, = torch.autograd.grad(out, qkv, gy)
    q, k, v = (t.reshape(B, heads, dh, T).permute(0, 1, 3, 2) for t in qkv.split(D, dim=1))
    want_out = F.scaled_dot_product_attention(q, k, v).permute(0, 1, 3, 2).reshape(B, D, T)
    want, = torch.autograd.grad(want_out, qkv, gy)
    assert _rel(out, want_out) < 1e-12 and _rel(got, want) < 1e-12
    assert (probs.sum(-1) - 1).abs().max().item() < 1e-14


class _Twin(nn.Module):
    """MMDL([Identity] * 3, ConcatEarly, Sequential(Transformer(409, 300), MLP(300, 128, 1))) in plain torch."""

    def __init__(self):
        super().__init__()
        from oracle import affect_oracle as O
        self.head = nn.Sequential(O.Transformer(409, 300), O.MLP(300, 128, 1))

    def forward(self, inputs):
        return self.head(torch.cat(inputs[0], dim=2))


def _pair(seed, dtype=torch.float32):
    from dynmm_amd import experts as E
    from oracle import affect_oracle as O
    ref = O.fill_(_Twin(), seed=seed)
    mine = E.affect_mm_ef_tran()
    mine.load_state_dict(ref.state_dict(), strict=True)
    return mine, ref.to(dtype)


def test_ef_tran_expert_layout_files_and_switch(tmp_path):
    from dynmm_amd import affect_mm
    from dynmm_amd import experts as E
    mine, ref = _pair(1)
    a, b = mine.state_dict(), ref.state_dict()
    assert list(a.keys()) == list(b.keys())
    assert all(tuple(a[k].shape) == tuple(b[k].shape) for k in a)
    assert tuple(a['head.0.conv.weight'].shape) == (300, 409, 1)
    assert tuple(a['head.0.transformer.layers.4.self_attn.in_proj_weight'].shape) == (900, 300)
    assert tuple(a['head.0.transformer.layers.0.linear1.weight'].shape) == (2048, 300)
    assert tuple(a['head.1.fc.weight'].shape) == (128, 300) and tuple(a['head.1.fc2.weight'].shape) == (1, 128)
    assert len(mine.head[0].transformer.layers) == 5 and mine.head[0].nhead == 5
    _Twin().load_state_dict(a, strict=True)                     # and back
    path, copy = affect_mm.file_names(str(tmp_path), 2)
    assert path.endswith('ef_tran.pt') and copy.endswith('b2_ef_tran.pt')
    with pytest.raises(NotImplementedError, match=r'Transformer\(409, 300\)'):
        affect_mm.main(['--fusion', '2', '--dataset', 'synthetic'])
    with pytest.raises(NotImplementedError, match='affect_mm_ef_tran'):
        E.affect_mm(2)


def test_attention_routes_by_head_dimension(monkeypatch):
    calls = []
    monkeypatch.setattr(S._MHACore, 'apply', staticmethod(lambda qkv, heads, d: calls.append(('core', heads)) or 'core'))
    monkeypatch.setattr(S._MHAWide, 'apply', staticmethod(lambda qkv, heads, d: calls.append(('wide', heads)) or 'wide'))
    assert attention(torch.zeros(1, 3 * 24 * 5, 8), 5) == 'core'
    assert attention(torch.zeros(1, 3 * 32 * 2, 8), 2) == 'core'
    assert attention(torch.zeros(1, 3 * 33 * 2, 8), 2) == 'wide'
    assert attention(torch.zeros(1, 3 * 60 * 5, 8), 5) == 'wide'
    assert mha_wide(torch.zeros(1, 3 * 24 * 5, 8), 5) == 'wide'
    assert calls == [('core', 5), ('core', 2), ('wide', 2), ('wide', 5), ('wide', 5)]


# ---------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------
# (dh, heads, T, B): the smallest shapes at which a 16 x 16 x 4 tiling can go wrong — dh = 33 (first above the old bound), 40 (a
# k-tail of the 16-channel tiles), 48 (full tiles), 60 (the expert), 63, 64 (the bound), 1 and 24 (the 32-channel instantiation);
# T around every tile edge.
WIDE_CASES = [
    (60, 5, 50, 2), (64, 2, 64, 2),
    (33, 1, 1, 1), (33, 2, 17, 3), (33, 5, 64, 1),
    (40, 2, 2, 2), (40, 1, 33, 1),
    (48, 1, 15, 1), (48, 2, 48, 2),
    (60, 1, 16, 1), (60, 2, 63, 1),
    (63, 1, 17, 2), (63, 5, 50, 1),
    (64, 1, 1, 3), (64, 5, 15, 1), (64, 1, 63, 1),
    (1, 2, 33, 2), (24, 5, 50, 2),
]


def test_wide_case_list_covers_the_issue():
    assert {33, 40, 48, 60, 63, 64, 1, 24} <= {c[0] for c in WIDE_CASES}
    assert {1, 2, 15, 16, 17, 33, 48, 50, 63, 64} <= {c[2] for c in WIDE_CASES}
    assert {1, 2, 5} <= {c[1] for c in WIDE_CASES} and {1, 2, 3} <= {c[3] for c in WIDE_CASES}
    assert (60, 5, 50, 2) in WIDE_CASES and (64, 2, 64, 2) in WIDE_CASES


def _wide_check(fig, tag, qkv, gy, heads, keep_flags=None, p=0.0):
    keep = None if keep_flags is None else keep_flags.float() / (1 - p)
    r64, r32 = _both(lambda a, b, k: _attn_grads(a, b, heads, k), (qkv, gy, keep))
    qc = _cu(qkv).requires_grad_(True)
    if keep_flags is not None:
        S.MASKS = _FixedMasks(attn=keep_flags.to(torch.uint8).cuda())
    try:
        out = mha_wide(qc, heads, drop=None if keep_flags is None else (p, 8, 'attn'))
        probs = out.grad_fn.saved_tensors[1]
        out.backward(_cu(gy))
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    fig.check(f'{tag} out', out, r64[0], r32[0], LN_FWD)
    fig.check(f'{tag} probs', probs, r64[1], r32[1], LN_FWD)
    fig.check(f'{tag} dqkv', qc.grad, r64[2], r32[2], LN_BWD)
    rows = (probs.double().sum(-1) - 1).abs().max().item()
    print(f'FIG {tag} |rowsum - 1|={rows:.3e}')
    if not rows < 1e-5:
        fig.bad.append((tag, 'rows of probs do not sum to 1', rows))


def _inputs(dh, heads, T, B, seed):
    g = _gen(seed)
    D = dh * heads
    return torch.randn(B, 3 * D, T, generator=g), torch.randn(B, D, T, generator=g), g


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', WIDE_CASES, ids=[f'dh{c[0]}-H{c[1]}-T{c[2]}-B{c[3]}' for c in WIDE_CASES])
def test_wide_attention_matches_float64(dh, heads, T, B):
    fig = _Figures()
    qkv, gy, _ = _inputs(dh, heads, T, B, dh * 10000 + heads * 100 + T)
    _wide_check(fig, f'attn dh={dh} H={heads} T={T} B={B}', qkv, gy, heads)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', [(60, 2, 50, 4), (33, 1, 17, 4)])
def test_wide_attention_is_stable_at_large_scores(dh, heads, T, B):
    """scores of magnitude ~1e3 (q scaled): finite, and equal to the reference, which subtracts the row maximum."""
    qkv, gy, _ = _inputs(dh, heads, T, B, dh + T)
    qkv[:, :dh * heads] *= 1e3
    fig = _Figures()
    _wide_check(fig, f'attn-big dh={dh} H={heads} T={T}', qkv, gy, heads)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', [(60, 5, 50, 1), (40, 2, 13, 2), (64, 1, 63, 1)])
def test_wide_attention_with_injected_masks(dh, heads, T, B):
    """keep flags on the probabilities at T % 8 != 0 and T % 16 != 0 (partial row8 chunks, partial tiles)."""
    p = 0.25
    qkv, gy, g = _inputs(dh, heads, T, B, dh * 7 + T)
    flags = torch.rand(B * heads, T, T, generator=g) >= p
    fig = _Figures()
    _wide_check(fig, f'attn-mask dh={dh} H={heads} T={T}', qkv, gy, heads, flags, p)
    fig.done()


@pytest.fixture
def philox_state():
    """the library's Philox seed and the device's dropout step, put back after the test"""
    from dynmm_amd import ops
    seed = ops._PHILOX_SEED
    yield
    ops.manual_seed(seed)
    S.dropout_step(torch.device('cuda', torch.cuda.current_device())).zero_()


def _generator_run(fn, qkv, gy, heads, p, site, seed, step):
    from dynmm_amd import ops
    ops.manual_seed(seed)
    S.dropout_step(torch.device('cuda', torch.cuda.current_device())).fill_(step)
    qc = _cu(qkv).requires_grad_(True)
    out = fn(qc, heads, drop=(p, site, 'attn'))
    probs = out.grad_fn.saved_tensors[1]
    out.backward(_cu(gy))
    torch.cuda.synchronize()
    return out.detach(), probs.detach(), qc.grad.detach()


@pytest.mark.gpu
def test_wide_attention_draws_mha_cores_decisions(philox_state):
    """dh = 24, T = 50, p = 0.1: the same seed, site and step give mha_wide and mha_core the same keep decisions."""
    qkv, gy, _ = _inputs(24, 5, 50, 2, 2450)
    a = _generator_run(mha_wide, qkv, gy, 5, 0.1, 11, 123, 3)
    b = _generator_run(S.mha_core, qkv, gy, 5, 0.1, 11, 123, 3)
    c = _generator_run(mha_wide, qkv, gy, 5, 0.1, 11, 123, 3)
    d = _generator_run(mha_wide, qkv, gy, 5, 0.1, 11, 123, 4)
    eo, eg = _rel(a[0], b[0]), _rel(a[2], b[2])
    print(f'FIG wide-vs-core out={eo:.3e} dqkv={eg:.3e}')
    assert eo < 1e-5 and eg < 1e-5
    assert all(torch.equal(x, y) for x, y in zip(a, c))        # the same step: the same bits
    assert _rel(d[0], a[0]) > 1e-3                             # another step: other decisions


@pytest.mark.gpu
def test_wide_attention_backward_regenerates_the_forwards_decisions(philox_state):
    """(40, 2, 33, 2) with V = the identity on its first T channels: out[c][i] = P'[i][c], so the drawn flags can be read off
    out / probs; dqkv of the generator run must be the float64 gradient under exactly those flags."""
    dh, heads, T, B, p = 40, 2, 33, 2, 0.1
    D = dh * heads
    qkv, gy, _ = _inputs(dh, heads, T, B, 4033)
    v = torch.zeros(B, heads, dh, T)
    v[:, :, :T, :] = torch.eye(T)
    qkv[:, 2 * D:] = v.reshape(B, D, T)
    out, probs, dqkv = _generator_run(mha_wide, qkv, gy, heads, p, 13, 99, 5)
    pk = out.reshape(B * heads, dh, T)[:, :T, :].transpose(1, 2).cpu()            # [B*H, query, key] = P'
    flags = pk != 0
    kept = flags.float().mean().item()
    ratio = (pk / probs.cpu())[flags]
    print(f'FIG attn-gen kept={kept:.4f} expected={1 - p:.4f} ratio in [{ratio.min().item():.6f}, {ratio.max().item():.6f}]')
    assert abs(kept - (1 - p)) < 0.02
    assert (ratio - 1 / (1 - p)).abs().max().item() < 1e-5
    keep = flags.float() / (1 - p)
    r64, r32 = _both(lambda a, b, k: _attn_grads(a, b, heads, k), (qkv, gy, keep))
    fig = _Figures()
    fig.check('attn-gen out', out, r64[0], r32[0], LN_FWD)
    fig.check('attn-gen dqkv', dqkv, r64[2], r32[2], LN_BWD)
    fig.done()


@pytest.mark.gpu
def test_wide_attention_refusals_write_nothing():
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()
    for B, D, T, heads, want in [(1, 130, 8, 2, L.DYNMM_EUNSUPPORTED), (1, 8, 65, 2, L.DYNMM_EUNSUPPORTED),
                                 (2, 10, 8, 3, L.DYNMM_EINVAL)]:
        qkv = torch.randn(B, 3 * D, T, device='cuda')
        gy = torch.randn(B, D, T, device='cuda')
        out = torch.full((B, D, T), 7.0, device='cuda')
        probs = torch.full((B * heads, T, T), 7.0, device='cuda')
        dqkv = torch.full((B, 3 * D, T), 7.0, device='cuda')
        assert lib.dynmm_attn_supported(D, T, heads) == 0
        assert lib.dynmm_attn_fwd(_ptr(qkv), _ptr(out), _ptr(probs), B, D, T, heads, None, st) == want
        assert lib.dynmm_attn_bwd(_ptr(gy), _ptr(qkv), _ptr(probs), _ptr(dqkv), B, D, T, heads, None, st) == want
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (out, probs, dqkv))
        with pytest.raises(L.DynmmHipError):
            mha_wide(qkv, heads)
    assert lib.dynmm_attn_supported(300, 50, 5) == 1 and lib.dynmm_attn_supported(128, 64, 2) == 1


# ---------------------------------------------------------------------------------------------------------------
# the expert
# ---------------------------------------------------------------------------------------------------------------
def _grad_errors(mine, ref):
    gr = dict(ref.named_parameters())
    errs = {}
    for n, p in mine.named_parameters():
        if gr[n].grad is None or gr[n].grad.abs().max() < 1e-9:
            continue
        errs[n] = ((p.grad.cpu().double() - gr[n].grad.double()).norm() / gr[n].grad.double().norm()).item()
    return errs


def _model_check(tag, mine, ref, out, out_r):
    errs = _grad_errors(mine, ref)
    worst = max(errs, key=errs.get)
    eo, med = _rel(out, out_r), float(np.median(list(errs.values())))
    print(f'FIG {tag} out={eo:.3e} worst grad={errs[worst]:.3e} ({worst}) median grad={med:.3e}')
    assert eo < 2e-4
    assert errs[worst] < 2e-3, (worst, errs[worst])
    assert med < 2e-4


def _f64(inputs):
    return [[x.double() for x in inputs[0]], inputs[1]]


def _dev(inputs):
    return [[x.cuda() for x in inputs[0]], inputs[1]]


@pytest.mark.gpu
def test_ef_tran_expert_matches_the_float64_twin():
    from oracle import affect_oracle as O
    mine, ref = _pair(1, torch.float64)
    mine = mine.cuda().eval()
    inputs, y = O.synth_batch(4, seed=3)
    out_r = ref(_f64(inputs))
    (out_r - y.double()).abs().mean().backward()
    out = mine(_dev(inputs))
    (out - y.cuda()).abs().mean().backward()
    torch.cuda.synchronize()
    _model_check('ef_tran eval', mine, ref, out, out_r)


@pytest.mark.gpu
def test_ef_tran_expert_training_mode_with_injected_dropout():
    from oracle import affect_oracle as O
    mine, ref = _pair(1, torch.float64)
    mine = mine.cuda().train()
    inputs, y = O.synth_batch(4, seed=3)
    mr, mh = _Masks(0.1, 21), _Masks(0.1, 21, 'cuda')
    O.Transformer.dropout_masks = (0.1, mr)
    S.MASKS = mh
    try:
        out_r = ref(_f64(inputs))
        (out_r - y.double()).abs().mean().backward()
        out = mine(_dev(inputs))
        (out - y.cuda()).abs().mean().backward()
        torch.cuda.synchronize()
    finally:
        O.Transformer.dropout_masks = None
        S.MASKS = None
    assert mr.n == mh.n == 20 and mr.names == mh.names == ['attn', 'dropout1', 'dropout', 'dropout2'] * 5
    _model_check('ef_tran train', mine, ref, out, out_r)
    mine.eval()
    with torch.no_grad():
        out_e = mine(_dev(inputs))
    assert _rel(out_e, out_r) > 1e-3                            # dropout really acted


@pytest.mark.gpu
def test_ef_tran_train_step_matches_torch_adamw():
    from dynmm_amd import experts as E
    from oracle import affect_oracle as O
    lr, wd = 1e-3, 1e-2
    mine, ref = _pair(2)
    mine = mine.cuda().eval()                # the optimiser arithmetic is what is compared here: dropout off on both sides
    step = E.ExpertTrainStep(mine, 'l1', lr=lr, weight_decay=wd)
    opt = torch.optim.AdamW(ref.parameters(), lr=lr, weight_decay=wd)
    for it in range(2):
        inputs, y = O.synth_batch(5, seed=10 + it)
        opt.zero_grad()
        loss_r = F.l1_loss(ref(inputs), y)
        loss_r.backward()
        gn = torch.nn.utils.clip_grad_norm_(ref.parameters(), 8.0)
        opt.step()
        last = step(_dev(inputs), y.cuda())
        torch.cuda.synchronize()
        tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
        print(f'FIG ef_tran step {it} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} norm={last["grad_norm"].item():.6f} '
              f'ref={gn.item():.6f}')
        assert abs(last['loss'].item() - loss_r.item()) < tol
        assert abs(last['grad_norm'].item() - gn.item()) < 2e-3 * max(gn.item(), 1e-3)
    sd_r, sd = ref.state_dict(), mine.state_dict()
    for k in sd_r:
        d = (sd[k].cpu() - sd_r[k]).abs()
        if k.endswith('in_proj_bias'):
            third = d.numel() // 3           # the key bias of softmax attention has an analytically zero gradient
            d = torch.cat([d[:third], d[2 * third:]])
        n_far = int((d > 0.4 * lr).sum().item())
        assert n_far <= max(1, int(2e-3 * d.numel())) and d.max().item() < 4.4 * lr, (k, n_far, d.max().item())
    step.opt.check_finite()


@pytest.mark.gpu
def test_ef_tran_graph_replay(philox_state):
    from dynmm_amd import experts as E
    from dynmm_amd import ops
    from oracle import affect_oracle as O
    a, _ = _pair(2)
    b, _ = _pair(2)
    a, b = a.cuda().eval(), b.cuda().eval()
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = O.synth_batch(4, seed=60 + it)
        x = _dev(inputs)
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k
    # dropout on, weights frozen: a replay must not reuse its decisions
    c, _ = _pair(2)
    c = c.cuda().train()
    sc = E.ExpertTrainStep(c, 'l1', lr=0.0, weight_decay=0.0, use_graph=True)
    inputs, y = O.synth_batch(4, seed=70)
    x = _dev(inputs)
    ops.manual_seed(77)
    S.dropout_step(x[0][0].device).zero_()
    losses = [sc(x, y.cuda())['loss'].item() for _ in range(3)]
    assert len({round(v, 7) for v in losses}) == 3, losses
    sc.opt.check_finite()
    for st in (sb, sc):                                        # the captures are released here, with the device idle
        torch.cuda.synchronize()
        for entry in st._graphs.values():
            entry[0].reset()
        st._graphs.clear()


@pytest.mark.gpu
def test_experts_train_writes_ef_tran(tmp_path):
    from dynmm_amd import affect, affect_mm
    from dynmm_amd import experts as E
    torch.manual_seed(0)
    dev = torch.device('cuda')
    loaders = [affect.Loader(*affect.synthetic_split(n, s), 32, shuffle=(k == 0), device=dev) for k, (n, s) in
               enumerate([(64, 1), (32, 2)])]
    model = E.affect_mm_ef_tran().to(dev)
    path = affect_mm.file_names(str(tmp_path), 2)[0]
    history, stopper, best = E.train(model, loaders, lambda x: x, 'l1', 1e-4, 1e-4, 1, lambda: E.save_state(model, path),
                                     protocol='mm')
    assert len(history) == 1 and all(h == h and abs(h) < float('inf') for h in history)
    fresh = E.affect_mm_ef_tran()
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    r = E.evaluate_posneg(fresh.to(dev), loaders[1], lambda x: x)
    assert all(r[k] == r[k] and abs(r[k]) < float('inf') for k in ('Accuracy', 'Loss', 'Corr')), r

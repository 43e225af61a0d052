"""Streaming attention for sequences longer than 64 steps (csrc/attn_long.hip; ops_seq.attention_long, packed_attention_long, the
dispatchers attention / masked_attention / packed_masked_attention) and the models it unblocks: Transformer(n, d) at any T, the
ef_tran expert at T > 64, MULT with a length per modality.

Yardstick: the float64 restatement tests/mult_oracle.ref_xattn with the bar rule of tests/test_seq_kernels.py — project bars 1e-5
(out, lse) and 2e-5 (dq, dk, dv) on `_rel` = max|a - b| / max|b|; a case that cannot sit under its project bar gets
max(project bar, 4 x the float32 error of the same restatement on the same inputs).  lse is compared with the float64 logsumexp of
the masked, scaled scores.  Every comparison prints its `FIG` line.

The key tile of the kernels is 64 wide (not wider), so the case list of the issue already holds T = tile +- 1.

Hidden keys are perturbed with large FINITE values, not NaN: the products P'V, dS K run on the matrix cores, where a hidden
position is an exact zero factor — 0 x (large) is 0, 0 x NaN is not, and no matrix instruction can select per (query, key).
"""
import gc
import math

import pytest
import torch

from tests import mult_oracle as MO
from tests.test_seq_kernels import LN_BWD, LN_FWD, _Figures, _FixedMasks, _both, _cu, _gen, _ptr, _rel

# (dh, heads, Tq, Tk, B, causal)
LONG_CASES = [
    (4, 2, 65, 65, 1, 1), (4, 2, 1, 65, 1, 1), (4, 2, 65, 1, 2, 1), (12, 1, 64, 129, 1, 1), (12, 1, 129, 64, 1, 1),
    (32, 2, 127, 128, 1, 0), (60, 1, 65, 65, 1, 0), (64, 1, 130, 70, 1, 1), (5, 2, 97, 33, 2, 1), (1, 2, 200, 200, 1, 1),
    (33, 1, 80, 80, 1, 0),                                                   # the 64-step boundary and the 16-wide tile edges
    (4, 10, 50, 500, 2, 1), (4, 10, 500, 50, 2, 1), (12, 10, 500, 500, 1, 1),  # the unaligned MULT shapes
]
IDS = ['dh%d-H%d-Tq%d-Tk%d-B%d-c%d' % c for c in LONG_CASES]
NEW_NAMES = ('dynmm_attn_long_supported', 'dynmm_attn_long_fwd', 'dynmm_attn_long_bwd')


@pytest.fixture(autouse=True)
def _leave_no_garbage():
    """Steps, captured graphs and models die with the test that made them, not in a later test's collector run."""
    yield
    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_bound():
    import os
    import re

    from dynmm_amd import lib as L
    header = open(os.path.join(os.path.dirname(L.__file__), '..', 'include', 'dynmm_hip.h')).read()
    for name in NEW_NAMES:
        assert name in L.SIGNATURES, name
        assert re.search(r'^int %s\(' % name, header, re.M), name
    assert L.ABI_VERSION == 5
    assert len(L.SIGNATURES['dynmm_attn_long_fwd'][1]) == 16 and len(L.SIGNATURES['dynmm_attn_long_bwd'][1]) == 23


def test_case_list_covers_the_issue():
    want = {(4, 2, 65, 65, 1, 1), (4, 2, 1, 65, 1, 1), (4, 2, 65, 1, 2, 1), (12, 1, 64, 129, 1, 1), (12, 1, 129, 64, 1, 1),
            (32, 2, 127, 128, 1, 0), (60, 1, 65, 65, 1, 0), (64, 1, 130, 70, 1, 1), (5, 2, 97, 33, 2, 1), (1, 2, 200, 200, 1, 1),
            (33, 1, 80, 80, 1, 0), (4, 10, 50, 500, 2, 1), (4, 10, 500, 50, 2, 1), (12, 10, 500, 500, 1, 1)}
    assert want == set(LONG_CASES) and len(LONG_CASES) == len(want)


def test_dispatchers_route_by_length_and_head_dimension(monkeypatch):
    from dynmm_amd import ops_seq as S
    calls = []

    def stub(name):
        return staticmethod(lambda *a: calls.append(name) or name)
    for cls, name in ((S._MHACore, 'core'), (S._MHAWide, 'wide'), (S._CrossAttention, 'cross'), (S._PackedAttention, 'packed'),
                      (S._AttentionLong, 'long'), (S._PackedAttentionLong, 'packed_long')):
        monkeypatch.setattr(cls, 'apply', stub(name))
    z = torch.zeros
    assert S.attention(z(1, 3 * 24 * 5, 50), 5) == 'core' and S.attention(z(1, 3 * 60 * 5, 64), 5) == 'wide'
    assert S.attention(z(1, 3 * 24 * 5, 65), 5) == 'packed_long' and S.attention(z(1, 3 * 60 * 5, 65), 5) == 'packed_long'
    q = lambda dh, T: z(1, dh * 2, T)                                # noqa: E731
    assert S.masked_attention(q(4, 50), q(4, 50), q(4, 50), 2, True) == 'cross'
    assert S.masked_attention(q(32, 64), q(32, 64), q(32, 64), 2, True) == 'cross'
    assert S.masked_attention(q(4, 50), q(4, 65), q(4, 65), 2, True) == 'long'
    assert S.masked_attention(q(4, 65), q(4, 50), q(4, 50), 2, True) == 'long'
    assert S.masked_attention(q(33, 50), q(33, 50), q(33, 50), 2, True) == 'long'
    assert S.packed_masked_attention(z(1, 3 * 12 * 10, 64), 10, True) == 'packed'
    assert S.packed_masked_attention(z(1, 3 * 12 * 10, 65), 10, True) == 'packed_long'
    assert S.packed_masked_attention(z(1, 3 * 33 * 2, 8), 2, True) == 'packed_long'


# ---------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------
def _S():
    from dynmm_amd import ops_seq as S
    return S


def _ref_lse(q, k, heads, causal):
    """logsumexp over the visible keys of (q / sqrt(dh)) . k: [B*heads, Tq]"""
    B, D, Tq = q.shape
    Tk, dh = k.shape[2], D // heads
    qh, kh = (t.reshape(B * heads, dh, t.shape[2]).transpose(1, 2) for t in (q, k))
    s = (qh * dh ** -0.5) @ kh.transpose(1, 2)
    if causal:
        s = s.masked_fill(~MO.visible(Tq, Tk), float('-inf'))
    return torch.logsumexp(s, dim=-1)


def _ref(q, k, v, gy, heads, causal, keep=None):
    """(out, lse, dq, dk, dv) of the restatement"""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, _ = MO.ref_xattn(q, k, v, heads, causal, keep)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), gy)
    return out.detach(), _ref_lse(q.detach(), k.detach(), heads, causal), dq, dk, dv


def _inputs(dh, heads, Tq, Tk, B, seed):
    g = _gen(seed)
    D = dh * heads
    return (torch.randn(B, D, Tq, generator=g), torch.randn(B, D, Tk, generator=g), torch.randn(B, D, Tk, generator=g),
            torch.randn(B, D, Tq, generator=g), g)


def _run(q, k, v, gy, heads, causal, packed, drop=None):
    """(out, lse, dq, dk, dv) of the HIP path"""
    S = _S()
    D = q.shape[1]
    if packed:
        qkv = torch.cat([_cu(q), _cu(k), _cu(v)], dim=1).requires_grad_(True)
        out = S.packed_attention_long(qkv, heads, causal, drop)
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 3                                       # qkv, out, lse: no probabilities
        out.backward(_cu(gy))
        torch.cuda.synchronize()
        return out.detach(), saved[2].detach(), qkv.grad[:, :D], qkv.grad[:, D:2 * D], qkv.grad[:, 2 * D:]
    qc, kc, vc = (_cu(t).requires_grad_(True) for t in (q, k, v))
    out = S.attention_long(qc, kc, vc, heads, causal, drop)
    saved = out.grad_fn.saved_tensors
    assert len(saved) == 5                                           # q, k, v, out, lse
    out.backward(_cu(gy))
    torch.cuda.synchronize()
    return out.detach(), saved[4].detach(), qc.grad, kc.grad, vc.grad


NAMES = ('out', 'lse', 'dq', 'dk', 'dv')
BARS = (LN_FWD, LN_FWD, LN_BWD, LN_BWD, LN_BWD)


def _check(fig, tag, q, k, v, gy, heads, causal, packed=False, keep_flags=None, p=0.0, refs=None):
    S = _S()
    keep = None if keep_flags is None else keep_flags.float() / (1 - p)
    r64, r32 = refs or _both(lambda a, b, c, d, kk: _ref(a, b, c, d, heads, causal, kk), (q, k, v, gy, keep))
    if keep_flags is not None:
        S.MASKS = _FixedMasks(attn=keep_flags.to(torch.uint8).cuda())
    try:
        got = _run(q, k, v, gy, heads, causal, packed, None if keep_flags is None else (p, 8, 'attn'))
    finally:
        S.MASKS = None
    for name, gt, a, b, bar in zip(NAMES, got, r64, r32, BARS):
        fig.check(f'{tag} {name}', gt, a, b, bar)
    return r64, r32


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,Tq,Tk,B,causal', LONG_CASES, ids=IDS)
def test_attention_long_matches_float64(dh, heads, Tq, Tk, B, causal):
    """the q / k / v form, and at Tq == Tk the packed form on the same inputs (one reference serves both)"""
    fig = _Figures()
    q, k, v, gy, _ = _inputs(dh, heads, Tq, Tk, B, dh * 100000 + heads * 1000 + Tq * 70 + Tk)
    tag = 'attn_long dh=%d H=%d Tq=%d Tk=%d B=%d causal=%d' % (dh, heads, Tq, Tk, B, causal)
    refs = _check(fig, tag, q, k, v, gy, heads, causal)
    if Tq == Tk:
        _check(fig, tag + ' packed', q, k, v, gy, heads, causal, packed=True, refs=refs)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('Tq,Tk', [(97, 97), (70, 130), (130, 70)])
def test_nothing_leaks_through_the_mask(Tq, Tk):
    """(4, 2, Tq, Tk, 2), causal; k and v at one key j0 scaled by 1e4 (large and finite: module docstring).  Forward: every out and
    lse row whose visible range ends before j0 keeps its bits.  Backward: with a gradient on the first m queries only, none of
    which sees j0, EVERY bit of dq, dk and dv is what it was, and dk / dv of the keys no such query sees (j0 among them) and dq of
    the other queries are exactly 0."""
    dh, heads, B = 4, 2, 2
    q, k, v, gy, _ = _inputs(dh, heads, Tq, Tk, B, Tq * 1000 + Tk)
    off = abs(Tk - Tq)
    j0 = min(Tk - 2, off + Tq // 2)
    blind = j0 - off                                               # queries 0 .. blind-1 do not see key j0
    k2, v2 = k.clone(), v.clone()
    k2[:, :, j0] *= 1e4
    v2[:, :, j0] *= 1e4
    base = _run(q, k, v, gy, heads, True, False)
    pert = _run(q, k2, v2, gy, heads, True, False)
    assert blind > 0
    assert torch.equal(base[0][:, :, :blind], pert[0][:, :, :blind]) and torch.equal(base[1][:, :blind], pert[1][:, :blind])
    assert not torch.equal(base[0][:, :, blind:], pert[0][:, :, blind:])
    m = blind // 2
    g2 = gy.clone()
    g2[:, :, m:] = 0.0
    a = _run(q, k, v, g2, heads, True, False)
    b = _run(q, k2, v2, g2, heads, True, False)
    unseen = m + off                                               # keys unseen .. Tk-1 are hidden from queries 0 .. m-1
    assert 0 < m < blind and unseen <= j0 < Tk
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y) and bool(torch.isfinite(y).all())
    assert bool((b[3][:, :, unseen:] == 0).all()) and bool((b[4][:, :, unseen:] == 0).all())
    assert bool((b[3][:, :, :unseen] != 0).any()) and bool((b[2][:, :, m:] == 0).all()) and bool((b[2][:, :, :m] != 0).any())


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,Tq,Tk,B,causal', [(4, 2, 65, 65, 1, 1), (5, 2, 97, 33, 2, 1), (64, 1, 130, 70, 1, 1)])
def test_attention_long_with_injected_masks(dh, heads, Tq, Tk, B, causal):
    """keep flags on the probabilities at Tk % 8 != 0 (partial row8 chunks) and partial tiles in both roles"""
    p = 0.25
    q, k, v, gy, g = _inputs(dh, heads, Tq, Tk, B, dh * 7 + Tq)
    flags = torch.rand(B * heads, Tq, Tk, generator=g) >= p
    fig = _Figures()
    tag = f'attn_long-mask dh={dh} H={heads} Tq={Tq} Tk={Tk}'
    refs = _check(fig, tag, q, k, v, gy, heads, causal, keep_flags=flags, p=p)
    if Tq == Tk:
        _check(fig, tag + ' packed', q, k, v, gy, heads, causal, packed=True, keep_flags=flags, p=p, refs=refs)
    fig.done()


@pytest.mark.gpu
def test_attention_long_is_stable_at_large_scores():
    """(12, 2, 97, 97, 1, causal) with q scaled so that the scaled scores reach about +-80: finite, and under the bars against the
    reference, which subtracts the row maximum."""
    dh, heads, T = 12, 2, 97
    q, k, v, gy, _ = _inputs(dh, heads, T, T, 1, dh + T)
    s = (q.reshape(heads, dh, T).transpose(1, 2) @ k.reshape(heads, dh, T)) * dh ** -0.5
    q = q * (80.0 / s.abs().max().item())
    fig = _Figures()
    _check(fig, f'attn_long-big dh={dh} H={heads} T={T}', q, k, v, gy, heads, True)
    fig.done()


@pytest.fixture
def philox_state():
    """the library's Philox seed and the device's dropout step, put back after the test"""
    from dynmm_amd import ops
    S = _S()
    seed = ops._PHILOX_SEED
    yield
    ops.manual_seed(seed)
    S.dropout_step(torch.device('cuda', torch.cuda.current_device())).zero_()


def _seeded(seed, step):
    from dynmm_amd import ops
    ops.manual_seed(seed)
    _S().dropout_step(torch.device('cuda', torch.cuda.current_device())).fill_(step)


def _generator_run(fn, tensors, gy, seed, step):
    """fn on device copies of `tensors` with the generator at (seed, step): (out, gradients...)"""
    _seeded(seed, step)
    ts = [_cu(t).requires_grad_(True) for t in tensors]
    out = fn(*ts)
    out.backward(_cu(gy))
    torch.cuda.synchronize()
    return (out.detach(),) + tuple(t.grad.detach() for t in ts)


@pytest.mark.gpu
def test_attention_long_draws_the_existing_kernels_decisions(philox_state):
    """p = 0.1, the same seed, site and step.  (12, 5, 50, 50, 2, no mask): packed_attention_long against mha_core;
    (4, 10, 50, 50, 2, causal): attention_long against cross_attention.  Agreement within 1e-5 means equal decisions (one
    different decision moves out by ~p / T); another step gives other decisions."""
    S = _S()
    p, site = 0.1, 11
    g = _gen(1250)
    qkv, gy = torch.randn(2, 3 * 60, 50, generator=g), torch.randn(2, 60, 50, generator=g)
    mine = lambda t: S.packed_attention_long(t, 5, False, (p, site, 'attn'))        # noqa: E731
    core = lambda t: S.mha_core(t, 5, (p, site, 'attn'))                            # noqa: E731
    a, b = _generator_run(mine, [qkv], gy, 123, 3), _generator_run(core, [qkv], gy, 123, 3)
    c, d = _generator_run(mine, [qkv], gy, 123, 3), _generator_run(mine, [qkv], gy, 123, 4)
    errs = [_rel(x, y) for x, y in zip(a, b)]
    print('FIG attn_long-vs-core out=%.3e dqkv=%.3e' % tuple(errs))
    assert all(e < 1e-5 for e in errs)
    assert all(torch.equal(x, y) for x, y in zip(a, c))            # the same step: the same bits
    assert _rel(d[0], a[0]) > 1e-3                                 # another step: other decisions

    q, k, v, gy, _ = _inputs(4, 10, 50, 50, 2, 4050)
    mine = lambda *t: S.attention_long(*t, 10, True, (p, site, 'attn'))             # noqa: E731
    cross = lambda *t: S.cross_attention(*t, 10, True, (p, site, 'attn'))           # noqa: E731
    a, b = _generator_run(mine, [q, k, v], gy, 123, 3), _generator_run(cross, [q, k, v], gy, 123, 3)
    d = _generator_run(mine, [q, k, v], gy, 123, 4)
    errs = [_rel(x, y) for x, y in zip(a, b)]
    print('FIG attn_long-vs-cross out=%.3e dq=%.3e dk=%.3e dv=%.3e' % tuple(errs))
    assert all(e < 1e-5 for e in errs)
    assert _rel(d[0], a[0]) > 1e-3


@pytest.mark.gpu
def test_attention_long_backward_redraws_the_forwards_decisions(philox_state):
    """(64, 1, 70, 130, 1, no mask), p = 0.1.  The decisions do not depend on the data: with q = 0 (uniform probabilities 1 / Tk)
    and v[c][j] = 1 iff j = c + dh w, out[c][i] Tk (1 - p) is the keep flag of key c + dh w, so ceil(Tk / dh) = 3 probes at one
    (seed, step) give the whole [B*heads, Tq, Tk] flag tensor.  A forward + backward on random data at that (seed, step) must then
    be the float64 oracle's under exactly those flags."""
    S = _S()
    dh, heads, Tq, Tk, B, p = 64, 1, 70, 130, 1, 0.1
    seed, step, site = 99, 5, 13
    drop = (p, site, 'attn')
    flags = torch.zeros(B * heads, Tq, Tk)
    for w in range(math.ceil(Tk / dh)):
        n = min(dh, Tk - dh * w)
        v = torch.zeros(B, dh, Tk)
        v[:, torch.arange(n), dh * w + torch.arange(n)] = 1.0
        _seeded(seed, step)
        with torch.no_grad():
            out = S.attention_long(torch.zeros(B, dh, Tq).cuda(), torch.randn(B, dh, Tk, generator=_gen(w)).cuda(), v.cuda(),
                                   heads, False, drop)
        f = out.cpu()[:, :n, :] * Tk * (1 - p)                      # [B, key - dh w, query]
        assert bool(((f - f.round()).abs() < 1e-4).all()) and bool(((f.round() == 0) | (f.round() == 1)).all())
        flags[:, :, dh * w:dh * w + n] = f.round().transpose(1, 2)
    kept, n = flags.mean().item(), flags.numel()
    sigma = math.sqrt(p * (1 - p) / n)
    print(f'FIG attn_long-gen kept={kept:.4f} expected={1 - p:.4f} 3 sigma={3 * sigma:.4f}')
    assert abs(kept - (1 - p)) < 3 * sigma
    q, k, v, gy, _ = _inputs(dh, heads, Tq, Tk, B, 6470)
    got = _generator_run(lambda *t: S.attention_long(*t, heads, False, drop), [q, k, v], gy, seed, step)
    r64, r32 = _both(lambda a, b, c, d, kk: _ref(a, b, c, d, heads, False, kk), (q, k, v, gy, flags / (1 - p)))
    fig = _Figures()
    for name, gt, a, b, bar in zip(('out', 'dq', 'dk', 'dv'), got, r64[:1] + r64[2:], r32[:1] + r32[2:],
                                   (LN_FWD, LN_BWD, LN_BWD, LN_BWD)):
        fig.check(f'attn_long-gen {name}', gt, a, b, bar)
    fig.done()


@pytest.mark.gpu
def test_attention_long_refusals_write_nothing():
    from dynmm_amd import lib as L
    S = _S()
    lib, st = S._lib(), S._stream()
    for B, D, Tq, Tk, heads, want in [(1, 130, 8, 8, 2, L.DYNMM_EUNSUPPORTED), (2, 10, 8, 8, 3, L.DYNMM_EINVAL)]:
        q, gy = torch.randn(B, D, Tq, device='cuda'), torch.randn(B, D, Tq, device='cuda')
        k, v = torch.randn(B, D, Tk, device='cuda'), torch.randn(B, D, Tk, device='cuda')
        out, dq = torch.full((B, D, Tq), 7.0, device='cuda'), torch.full((B, D, Tq), 7.0, device='cuda')
        lse = torch.full((B * heads, Tq), 7.0, device='cuda')
        dk, dv = torch.full((B, D, Tk), 7.0, device='cuda'), torch.full((B, D, Tk), 7.0, device='cuda')
        sq, sk = D * Tq, D * Tk
        assert lib.dynmm_attn_long_supported(D, Tq, Tk, heads) == 0
        assert lib.dynmm_attn_long_fwd(_ptr(q), _ptr(k), _ptr(v), sq, sk, sk, _ptr(out), _ptr(lse), B, D, Tq, Tk, heads, 1, None,
                                       st) == want
        assert lib.dynmm_attn_long_bwd(_ptr(gy), _ptr(q), _ptr(k), _ptr(v), sq, sk, sk, _ptr(out), _ptr(lse), _ptr(dq), _ptr(dk),
                                       _ptr(dv), sq, sk, sk, B, D, Tq, Tk, heads, 1, None, st) == want
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (out, lse, dq, dk, dv))
        with pytest.raises(L.DynmmHipError):
            S.attention_long(q, k, v, heads, True)
    assert lib.dynmm_attn_long_supported(128, 8, 8, 2) == 1 and lib.dynmm_attn_long_supported(40, 50, 500, 10) == 1
    assert lib.dynmm_attn_long_supported(300, 1 << 20, 1, 5) == 1 and lib.dynmm_attn_long_supported(40, (1 << 24) + 1, 8, 10) == 0


def _fn_name(t):
    return type(t.grad_fn).__name__


@pytest.mark.gpu
def test_dispatch_keeps_the_short_kernels():
    S = _S()
    dev = dict(device='cuda', requires_grad=True)
    assert _fn_name(S.attention(torch.randn(1, 3 * 24 * 5, 50, **dev), 5)) == '_MHACoreBackward'
    assert _fn_name(S.attention(torch.randn(1, 3 * 60 * 5, 50, **dev), 5)) == '_MHAWideBackward'
    assert _fn_name(S.attention(torch.randn(1, 3 * 24 * 5, 65, **dev), 5)) == '_PackedAttentionLongBackward'
    assert _fn_name(S.attention(torch.randn(1, 3 * 60 * 5, 65, **dev), 5)) == '_PackedAttentionLongBackward'
    q = lambda T: torch.randn(1, 8, T, **dev)                        # noqa: E731
    assert _fn_name(S.masked_attention(q(50), q(50), q(50), 2, True)) == '_CrossAttentionBackward'
    assert _fn_name(S.masked_attention(q(50), q(65), q(65), 2, True)) == '_AttentionLongBackward'
    assert _fn_name(S.packed_masked_attention(torch.randn(1, 24, 50, **dev), 2, True)) == '_PackedAttentionBackward'
    assert _fn_name(S.packed_masked_attention(torch.randn(1, 24, 65, **dev), 2, True)) == '_PackedAttentionLongBackward'
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_transformer_at_70_steps_matches_the_float64_twin():
    """A.Transformer(20, 40) (dh = 8: the gate transformers' kind) at T = 70, with test_attn_wide's whole-model bars"""
    from dynmm_amd.nn import affect as A
    from oracle import affect_oracle as O
    from tests.test_attn_wide import _model_check
    ref = O.fill_(O.Transformer(20, 40), seed=4)
    mine = A.Transformer(20, 40)
    mine.load_state_dict(ref.state_dict(), strict=True)
    ref, mine = ref.double(), mine.cuda().eval()
    g = _gen(2070)
    x, gy = torch.randn(2, 70, 20, generator=g), torch.randn(2, 40, generator=g)
    out_r = ref(x.double())
    out_r.backward(gy.double())
    out = mine(x.cuda())
    out.backward(gy.cuda())
    torch.cuda.synchronize()
    _model_check('transformer(20, 40) T=70', mine, ref, out, out_r)


@pytest.mark.gpu
def test_ef_tran_expert_at_70_steps_matches_the_float64_twin():
    """Transformer(409, 300) (dh = 60), B = 2, T = 70"""
    from oracle import affect_oracle as O
    from tests.test_attn_wide import _dev, _f64, _model_check, _pair
    mine, ref = _pair(1, torch.float64)
    mine = mine.cuda().eval()
    inputs, y = O.synth_batch(2, T=70, seed=3)
    out_r = ref(_f64(inputs))
    (out_r - y.double()).abs().mean().backward()
    out = mine(_dev(inputs))
    (out - y.cuda()).abs().mean().backward()
    torch.cuda.synchronize()
    _model_check('ef_tran eval T=70', mine, ref, out, out_r)


MULT_LENGTHS = (20, 70, 97)


def _mult_batch(batch, seed, lengths=MULT_LENGTHS):
    """a MOSEI-shaped batch with a length per modality; the first steps of sample 0 are zero padding in every modality"""
    g = _gen(seed)
    xs = [torch.randn(batch, T, f, generator=g) for T, f in zip(lengths, (35, 74, 300))]
    for x in xs:
        x[0, :min(7, x.shape[1] - 1)] = 0
    return [xs, [torch.full((batch,), T, dtype=torch.long) for T in lengths]], torch.randn(batch, 1, generator=g)


@pytest.mark.gpu
def test_mult_with_a_length_per_modality_matches_the_float64_twin():
    """lengths (20, 70, 97), B = 2: cross attention at (Tq, Tk) = (20, 70), (97, 20), ... on both kernel families, the memory
    transformers at 20 (xattn.hip), 70 and 97 (attn_long.hip) steps; test_mult's whole-model bars"""
    from tests.test_mult import _hip_run, _model_check, _pair, _twin_run
    mine, ref = _pair(1)
    inputs, y = _mult_batch(2, seed=3)
    ref.eval()
    mine = mine.cuda().eval()
    out32, g32 = _twin_run(ref, inputs, y, torch.float32)
    out64, _ = _twin_run(ref, inputs, y, torch.float64)              # (ref now holds the float64 gradients)
    out, grads = _hip_run(mine, inputs, y)
    _model_check('mult eval T=(20, 70, 97)', grads, ref, out, out64, g32, out32)


@pytest.mark.gpu
def test_mult_graph_replay_with_a_length_per_modality():
    """an eager step and a captured one (use_graph=True: the first call captures, the next two replay) on lengths (20, 70, 97)
    agree to test_attn_wide's graph-replay tolerances: the streaming kernels allocate nothing and read nothing on the host"""
    from dynmm_amd import experts as E
    from tests.test_mult import _pair, _to
    a, _ = _pair(2)
    b, _ = _pair(2)
    a, b = a.cuda().eval(), b.cuda().eval()
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = _mult_batch(2, seed=60 + it)
        x = _to(inputs, lambda t: t.cuda())
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k
    sb.opt.check_finite()
    torch.cuda.synchronize()                                         # the capture is released here, with the device idle
    for entry in sb._graphs.values():
        entry[0].reset()
    sb._graphs.clear()

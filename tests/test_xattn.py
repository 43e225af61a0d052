"""Masked cross-modal attention and the embedding kernel of MULT (csrc/xattn.hip; ops_seq.cross_attention, packed_attention,
pos_embed).

Yardstick: the float64 restatement tests/mult_oracle.ref_xattn with the bar rule of tests/test_seq_kernels.py — project bars 1e-5
(out, probs) and 2e-5 (gradients) on `_rel` = max|a - b| / max|b|; a case that cannot sit under its project bar gets
max(project bar, 4 x the float32 error of the same restatement on the same inputs).  Every comparison prints its `FIG` line.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import mult_oracle as MO
from tests.test_seq_kernels import LN_BWD, LN_FWD, _Figures, _FixedMasks, _both, _cu, _gen, _ptr, _rel

# (dh, heads, Tq, Tk, B, causal)
XA_CASES = [
    (4, 10, 50, 50, 2, 1), (12, 10, 50, 50, 2, 1),                                             # the model's own shapes
    (4, 1, 1, 1, 1, 1), (4, 2, 1, 17, 1, 1), (4, 2, 17, 1, 2, 1), (4, 2, 16, 16, 1, 1), (4, 2, 17, 16, 1, 1),      # edges
    (4, 2, 15, 33, 2, 1), (4, 2, 33, 15, 2, 1), (12, 1, 63, 64, 1, 1), (12, 1, 64, 63, 1, 1), (12, 2, 64, 64, 2, 1),
    (32, 1, 64, 64, 1, 1),                                                                     # unequal lengths, the bounds
    (1, 2, 33, 33, 2, 1), (5, 2, 17, 17, 1, 1), (32, 2, 50, 50, 1, 0),                          # other head dimensions
    (4, 2, 17, 33, 1, 0), (12, 5, 50, 50, 2, 0),                                                # no mask
]
PACKED = {(12, 10, 50, 50, 2, 1), (12, 5, 50, 50, 2, 0), (1, 2, 33, 33, 2, 1)}                  # run through packed_attention


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dh,heads,Tq,Tk', [(4, 10, 50, 50), (12, 2, 33, 15)])
def test_ref_xattn_is_torchs_sdpa_with_the_boolean_mask(dh, heads, Tq, Tk):
    B, D = 2, dh * heads
    g = _gen(dh * 100 + Tq)
    q = torch.randn(B, D, Tq, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(B, D, Tk, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(B, D, Tk, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(B, D, Tq, generator=g, dtype=torch.float64)
    out, probs = MO.ref_xattn(q, k, v, heads, True)
    got = torch.autograd.grad(out, (q, k, v), gy)
    mask = torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + abs(Tk - Tq)
    assert torch.equal(mask, MO.visible(Tq, Tk))
    qh, kh, vh = (t.reshape(B, heads, dh, t.shape[2]).permute(0, 1, 3, 2) for t in (q, k, v))
    want_out = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask).permute(0, 1, 3, 2).reshape(B, D, Tq)
    want = torch.autograd.grad(want_out, (q, k, v), gy)
    assert _rel(out, want_out) < 1e-12
    assert all(_rel(a, b) < 1e-12 for a, b in zip(got, want))
    assert (probs.sum(-1) - 1).abs().max().item() < 1e-14
    assert bool((probs.reshape(B * heads, Tq, Tk)[:, ~mask] == 0).all())


def test_xattn_case_list_covers_the_issue():
    want = {(4, 10, 50, 50, 2, 1), (12, 10, 50, 50, 2, 1), (4, 1, 1, 1, 1, 1), (4, 2, 1, 17, 1, 1), (4, 2, 17, 1, 2, 1),
            (4, 2, 16, 16, 1, 1), (4, 2, 17, 16, 1, 1), (4, 2, 15, 33, 2, 1), (4, 2, 33, 15, 2, 1), (12, 1, 63, 64, 1, 1),
            (12, 1, 64, 63, 1, 1), (12, 2, 64, 64, 2, 1), (32, 1, 64, 64, 1, 1), (1, 2, 33, 33, 2, 1), (5, 2, 17, 17, 1, 1),
            (32, 2, 50, 50, 1, 0), (4, 2, 17, 33, 1, 0), (12, 5, 50, 50, 2, 0)}
    assert want == set(XA_CASES) and len(XA_CASES) == len(want)
    assert (12, 10, 50, 50, 2, 1) in PACKED and (4, 10, 50, 50, 2, 1) not in PACKED


# ---------------------------------------------------------------------------------------------------------------
# the attention kernels
# ---------------------------------------------------------------------------------------------------------------
def _S():
    from dynmm_amd import ops_seq as S
    return S


def _xa_grads(q, k, v, gy, heads, causal, keep=None):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, probs = MO.ref_xattn(q, k, v, heads, causal, keep)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), gy)
    return out.detach(), probs.detach(), dq, dk, dv


def _xa_inputs(dh, heads, Tq, Tk, B, seed):
    g = _gen(seed)
    D = dh * heads
    return (torch.randn(B, D, Tq, generator=g), torch.randn(B, D, Tk, generator=g), torch.randn(B, D, Tk, generator=g),
            torch.randn(B, D, Tq, generator=g), g)


def _xa_run(q, k, v, gy, heads, causal, packed, drop=None):
    """(out, probs, dq, dk, dv) of the HIP path"""
    S = _S()
    D = q.shape[1]
    if packed:
        qkv = torch.cat([_cu(q), _cu(k), _cu(v)], dim=1).requires_grad_(True)
        out = S.packed_attention(qkv, heads, causal, drop)
        probs = out.grad_fn.saved_tensors[1]
        out.backward(_cu(gy))
        torch.cuda.synchronize()
        return out.detach(), probs.detach(), qkv.grad[:, :D], qkv.grad[:, D:2 * D], qkv.grad[:, 2 * D:]
    qc, kc, vc = (_cu(t).requires_grad_(True) for t in (q, k, v))
    out = S.cross_attention(qc, kc, vc, heads, causal, drop)
    probs = out.grad_fn.saved_tensors[3]
    out.backward(_cu(gy))
    torch.cuda.synchronize()
    return out.detach(), probs.detach(), qc.grad, kc.grad, vc.grad


def _xa_check(fig, tag, q, k, v, gy, heads, causal, packed=False, keep_flags=None, p=0.0):
    S = _S()
    keep = None if keep_flags is None else keep_flags.float() / (1 - p)
    r64, r32 = _both(lambda a, b, c, d, kk: _xa_grads(a, b, c, d, heads, causal, kk), (q, k, v, gy, keep))
    if keep_flags is not None:
        S.MASKS = _FixedMasks(attn=keep_flags.to(torch.uint8).cuda())
    try:
        got = _xa_run(q, k, v, gy, heads, causal, packed, None if keep_flags is None else (p, 8, 'attn'))
    finally:
        S.MASKS = None
    for name, gt, a, b, bar in zip(('out', 'probs', 'dq', 'dk', 'dv'), got, r64, r32, (LN_FWD, LN_FWD, LN_BWD, LN_BWD, LN_BWD)):
        fig.check(f'{tag} {name}', gt, a, b, bar)
    probs = got[1]
    rows = (probs.double().sum(-1) - 1).abs().max().item()
    print(f'FIG {tag} |rowsum - 1|={rows:.3e}')
    if not rows < 1e-5:
        fig.bad.append((tag, 'rows of probs do not sum to 1', rows))
    if causal:
        hidden = ~MO.visible(q.shape[2], k.shape[2])
        if not bool((probs.cpu()[:, hidden] == 0).all()):
            fig.bad.append((tag, 'a masked probability is not exactly 0'))


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,Tq,Tk,B,causal', XA_CASES, ids=['dh%d-H%d-Tq%d-Tk%d-B%d-c%d' % c for c in XA_CASES])
def test_cross_attention_matches_float64(dh, heads, Tq, Tk, B, causal):
    fig = _Figures()
    q, k, v, gy, _ = _xa_inputs(dh, heads, Tq, Tk, B, dh * 100000 + heads * 1000 + Tq * 70 + Tk)
    case = (dh, heads, Tq, Tk, B, causal)
    _xa_check(fig, 'xattn dh=%d H=%d Tq=%d Tk=%d B=%d causal=%d' % case, q, k, v, gy, heads, causal, packed=case in PACKED)
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


def _generator_run(fn, qkv, gy, heads, p, site, seed, step):
    from dynmm_amd import ops
    S = _S()
    ops.manual_seed(seed)
    S.dropout_step(torch.device('cuda', torch.cuda.current_device())).fill_(step)
    qc = _cu(qkv).requires_grad_(True)
    out = fn(qc, heads, (p, site, 'attn') if p > 0 else None)
    out.backward(_cu(gy))
    torch.cuda.synchronize()
    return out.detach(), qc.grad.detach()


@pytest.mark.gpu
def test_packed_attention_agrees_with_mha_core(philox_state):
    """(12, 5, 50, 50, 2, no mask), packed: out and dqkv within 1e-5 of mha_core; with the generator on (same seed, site and step)
    both draw the same decisions."""
    S = _S()
    dh, heads, T, B = 12, 5, 50, 2
    g = _gen(1250)
    qkv, gy = torch.randn(B, 3 * dh * heads, T, generator=g), torch.randn(B, dh * heads, T, generator=g)
    mine = lambda t, h, d: S.packed_attention(t, h, False, d)       # noqa: E731
    core = lambda t, h, d: S.mha_core(t, h, d)                      # noqa: E731
    for p in (0.0, 0.1):
        a = _generator_run(mine, qkv, gy, heads, p, 11, 123, 3)
        b = _generator_run(core, qkv, gy, heads, p, 11, 123, 3)
        eo, eg = _rel(a[0], b[0]), _rel(a[1], b[1])
        print(f'FIG xattn-vs-core p={p} out={eo:.3e} dqkv={eg:.3e}')
        assert eo < 1e-5 and eg < 1e-5
    c = _generator_run(mine, qkv, gy, heads, 0.1, 11, 123, 3)
    d = _generator_run(mine, qkv, gy, heads, 0.1, 11, 123, 4)
    assert all(torch.equal(x, y) for x, y in zip(a, c))            # the same step: the same bits
    assert _rel(d[0], a[0]) > 1e-3                                 # another step: other decisions


@pytest.mark.gpu
@pytest.mark.parametrize('Tq,Tk', [(20, 20), (12, 20)])
def test_nothing_leaks_through_the_mask(Tq, Tk):
    """(4, 2, Tq, Tk), causal.  Forward: k and v at key j0 scaled by 1e3 — every out row whose visible range ends before j0 keeps
    its bits.  Backward: the last query sees every key under this mask (Tq - 1 + |Tk - Tq| >= Tk - 1), so "keys no query may see"
    are made by giving only the first m queries a gradient: dk and dv of the keys beyond their visible range are exactly 0."""
    dh, heads, B = 4, 2, 2
    q, k, v, gy, _ = _xa_inputs(dh, heads, Tq, Tk, B, Tq * 100 + Tk)
    off = abs(Tk - Tq)
    j0 = off + Tq // 2
    blind = j0 - off                                               # queries 0 .. blind-1 do not see key j0
    base = _xa_run(q, k, v, gy, heads, True, False)
    k2, v2 = k.clone(), v.clone()
    k2[:, :, j0] *= 1e3
    v2[:, :, j0] *= 1e3
    pert = _xa_run(q, k2, v2, gy, heads, True, False)
    assert blind > 0
    assert torch.equal(base[0][:, :, :blind], pert[0][:, :, :blind])
    assert torch.equal(base[1][:, :blind], pert[1][:, :blind])
    assert not torch.equal(base[0][:, :, blind:], pert[0][:, :, blind:])
    m = Tq // 3
    g2 = gy.clone()
    g2[:, :, m:] = 0.0
    part = _xa_run(q, k2, v2, g2, heads, True, False)
    unseen = m + off                                               # keys unseen .. Tk-1 are hidden from queries 0 .. m-1
    assert unseen < Tk
    assert bool((part[3][:, :, unseen:] == 0).all()) and bool((part[4][:, :, unseen:] == 0).all())
    assert bool((part[3][:, :, :unseen] != 0).any()) and bool((part[2][:, :, m:] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,Tq,Tk,B', [(4, 10, 50, 50, 2), (12, 2, 13, 33, 2)])
def test_cross_attention_with_injected_masks(dh, heads, Tq, Tk, B):
    p = 0.25
    q, k, v, gy, g = _xa_inputs(dh, heads, Tq, Tk, B, dh * 7 + Tq)
    flags = torch.rand(B * heads, Tq, Tk, generator=g) >= p
    fig = _Figures()
    _xa_check(fig, f'xattn-mask dh={dh} H={heads} Tq={Tq} Tk={Tk}', q, k, v, gy, heads, True, keep_flags=flags, p=p)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,Tq,Tk,B', [(4, 10, 50, 50, 2), (12, 2, 13, 33, 2)])
def test_cross_attention_is_stable_at_large_scores(dh, heads, Tq, Tk, B):
    """scores of magnitude ~1e3 (q scaled): finite, and equal to the reference, which subtracts the row maximum."""
    q, k, v, gy, _ = _xa_inputs(dh, heads, Tq, Tk, B, dh + Tq)
    fig = _Figures()
    _xa_check(fig, f'xattn-big dh={dh} H={heads} Tq={Tq} Tk={Tk}', q * 1e3, k, v, gy, heads, True)
    fig.done()


@pytest.mark.gpu
def test_cross_attention_refusals_write_nothing():
    from dynmm_amd import lib as L
    S = _S()
    lib, st = S._lib(), S._stream()
    for B, D, Tq, Tk, heads, want in [(1, 66, 8, 8, 2, L.DYNMM_EUNSUPPORTED), (1, 8, 65, 8, 2, L.DYNMM_EUNSUPPORTED),
                                      (1, 8, 8, 65, 2, L.DYNMM_EUNSUPPORTED), (2, 10, 8, 8, 3, L.DYNMM_EINVAL)]:
        q, gy = torch.randn(B, D, Tq, device='cuda'), torch.randn(B, D, Tq, device='cuda')
        k, v = torch.randn(B, D, Tk, device='cuda'), torch.randn(B, D, Tk, device='cuda')
        out, dq = torch.full((B, D, Tq), 7.0, device='cuda'), torch.full((B, D, Tq), 7.0, device='cuda')
        probs = torch.full((B * heads, Tq, Tk), 7.0, device='cuda')
        dk, dv = torch.full((B, D, Tk), 7.0, device='cuda'), torch.full((B, D, Tk), 7.0, device='cuda')
        sq, sk = D * Tq, D * Tk
        assert lib.dynmm_xattn_supported(D, Tq, Tk, heads) == 0
        assert lib.dynmm_xattn_fwd(_ptr(q), _ptr(k), _ptr(v), sq, sk, sk, _ptr(out), _ptr(probs), B, D, Tq, Tk, heads, 1, None,
                                   st) == want
        assert lib.dynmm_xattn_bwd(_ptr(gy), _ptr(q), _ptr(k), _ptr(v), sq, sk, sk, _ptr(probs), _ptr(dq), _ptr(dk), _ptr(dv), sq,
                                   sk, sk, B, D, Tq, Tk, heads, 1, None, st) == want
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (out, probs, dq, dk, dv))
        with pytest.raises(L.DynmmHipError):
            S.cross_attention(q, k, v, heads, True)
    assert lib.dynmm_xattn_supported(40, 50, 50, 10) == 1 and lib.dynmm_xattn_supported(64, 64, 1, 2) == 1
    assert lib.dynmm_xattn_supported(120, 50, 50, 10) == 1


# ---------------------------------------------------------------------------------------------------------------
# the embedding kernel
# ---------------------------------------------------------------------------------------------------------------
def test_sinusoid_table_is_the_closed_form():
    from dynmm_amd.nn import mult
    for E, T in [(40, 50), (120, 1), (6, 17)]:
        tab = mult.sinusoid_table(E, T)
        assert tuple(tab.shape) == (E, T)
        for c in (0, 1, E // 2 - 1):
            w = math.exp(-c * math.log(10000.0) / (E // 2 - 1))
            for t in (0, T // 2, T - 1):
                assert abs(tab[c, t].item() - math.sin((t + 1) * w)) < 1e-12
                assert abs(tab[c + E // 2, t].item() - math.cos((t + 1) * w)) < 1e-12
        assert _rel(tab, MO.position_table(E, T).t()) < 1e-14


def _embed_inputs(B, E, T, seed):
    g = _gen(seed)
    x = torch.randn(B, E, T, generator=g)
    x[0, 0, :min(3, T)] = 0.0                      # leading padded steps of sample 0 (channel 0 exactly zero)
    if B > 1:
        x[B - 1, :, :min(5, T - 1)] = 0.0          # whole padded steps of the last sample
    return x, torch.randn(B, E, T, generator=g), torch.randn(B, E, T, generator=g), g


@pytest.mark.gpu
@pytest.mark.parametrize('B,E,T', [(2, 40, 50), (1, 120, 1), (3, 6, 17)])
@pytest.mark.parametrize('masked', [False, True])
def test_pos_embed_matches_the_closed_form(B, E, T, masked):
    from dynmm_amd.nn import mult
    S = _S()
    p, scale = 0.2, math.sqrt(E)
    x, g1, g2, g = _embed_inputs(B, E, T, E * 100 + T)
    f1 = (torch.rand(B, E, T, generator=g) >= p) if masked else None
    f2 = (torch.rand(B, E, T, generator=g) >= p) if masked else None

    def ref(xx, a, b, k1, k2):
        xx = xx.clone().requires_grad_(True)
        e = MO.embed_closed_form(xx, scale)
        y1, y2 = (e if k1 is None else e * k1), (e if k2 is None else e * k2)
        dx, = torch.autograd.grad([y1, y2], xx, [a, b])
        return y1.detach(), y2.detach(), dx
    k1, k2 = (None, None) if not masked else (f1.float() / (1 - p), f2.float() / (1 - p))
    r64, r32 = _both(ref, (x, g1, g2, k1, k2))
    pad = (x[:, 0, :] == 0)[:, None, :].expand_as(x)
    assert bool(pad.any())
    pos = mult.sinusoid_table(E, T).float().cuda()
    xc = _cu(x).requires_grad_(True)
    if masked:
        S.MASKS = _FixedMasks(embed_k=f1.to(torch.uint8).cuda(), embed_v=f2.to(torch.uint8).cuda())
    try:
        if masked:
            y1, y2 = S.pos_embed(xc, pos, scale, drop=(p, 3, 'embed_k'), drop2=(p, 4, 'embed_v'))
        else:
            y1 = y2 = S.pos_embed(xc, pos, scale)
            assert not isinstance(y1, tuple)
        torch.autograd.backward([y1, y2], [_cu(g1), _cu(g2)])
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    fig = _Figures()
    tag = f'posembed B={B} E={E} T={T} masked={int(masked)}'
    fig.check(f'{tag} y1', y1, r64[0], r32[0], LN_FWD)
    fig.check(f'{tag} y2', y2, r64[1], r32[1], LN_FWD)
    fig.check(f'{tag} dx', xc.grad, r64[2], r32[2], LN_BWD)
    fig.done()
    # padded steps: sqrt(E) x (times its keep factor), no positional term
    want = scale * x * (1.0 if k1 is None else k1)
    assert _rel(y1.cpu()[pad], want[pad]) < 1e-6


@pytest.mark.gpu
def test_pos_embed_two_sites_draw_different_decisions(philox_state):
    from dynmm_amd import ops
    from dynmm_amd.nn import mult
    S = _S()
    B, E, T, p = 2, 40, 50, 0.2
    x = _cu(torch.randn(B, E, T, generator=_gen(5))) + 3.0          # no zeros: a zero output is a dropped element
    ops.manual_seed(17)
    y1, y2 = S.pos_embed(x, mult.sinusoid_table(E, T).float().cuda(), math.sqrt(E), drop=(p, 5, 'embed_k'), drop2=(p, 6, 'embed_v'))
    torch.cuda.synchronize()
    d1, d2 = (y1 == 0), (y2 == 0)
    r1, r2 = d1.float().mean().item(), d2.float().mean().item()
    print(f'FIG posembed dropped {r1:.4f} {r2:.4f} expected {p}')
    assert abs(r1 - p) < 0.03 and abs(r2 - p) < 0.03
    assert not torch.equal(d1, d2)
    kept = ~d1 & ~d2
    assert _rel(y1[kept], y2[kept]) == 0.0                           # where both keep, the same value

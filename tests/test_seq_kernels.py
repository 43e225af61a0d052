"""The sequence kernels (csrc/seq.hip, csrc/seq_ffn.hip) against float64 restatements, on every dispatch arm.

Every GPU test compares a kernel with a plain restatement of the same operation written below (torch on the CPU, no
project ops) and evaluated in float64.  The restatements themselves are checked without a GPU against torch's own
functions (F.layer_norm, scaled_dot_product_attention, clip_grad_norm_, autograd on the DiffSoftmax formula).

Bars.  `_rel` = max |a - b| / max |b|, as in test_affect.py.  The project's bars: LayerNorm and attention 1e-5 forward,
2e-5 backward; the fused feed-forward 2e-5 forward, 1e-4 data gradients.  The mixture head is held to the LayerNorm /
attention bars (per-row arithmetic over K <= 4 values and one mean over B: nothing in it is less exact than a LayerNorm
row), the plain dropout op to test_affect.py's 1e-6.  Where a case cannot sit under the project bar the yardstick is
the SAME restatement evaluated in float32 by torch on the CPU, on the same inputs, against its float64 value: the bar
of a case is max(project bar, 4 x that float32 error) — the factor 4 for the kernels' fixed summation orders (16-way
group sums, wave butterflies, hidden-unit slabs) against torch's.  Gradient-norm clipping accumulates in double and
rounds once: norm and coefficient within relative 1.2e-7 of the float64 value.

Every comparison prints `FIG <case> kernel=<err> f32=<yardstick> bar=<bar>`; cases above the project bar are marked
RAISED.  On an MI355X every other comparison of the module sat under its project bar; these 25 needed the raised one
(none needed more than 4x; the largest ratio is 2.4):

    case                                          output     kernel      float32     ratio
    large scores   dh=24 H=5 T=64 B=8             out        6.642e-05   6.642e-05   1.00
                                                  probs      7.129e-05   7.129e-05   1.00
                                                  dqkv       1.257e-04   1.257e-04   1.00
    large scores   dh=12 H=2 T=50 B=8             out        1.718e-05   1.718e-05   1.00
                                                  probs      1.565e-05   1.565e-05   1.00
                                                  dqkv       2.532e-05   2.535e-05   1.00
    large scores   dh=2  H=4 T=9  B=8             probs      1.062e-05   4.404e-06   2.41
    large scores   dh=7  H=3 T=33 B=8             out        2.680e-05   2.679e-05   1.00
                                                  probs      2.921e-05   2.921e-05   1.00
    large scores   dh=32 H=2 T=64 B=8             out        1.070e-05   1.067e-05   1.00
                                                  probs      1.308e-05   1.308e-05   1.00
                                                  dqkv       3.870e-05   3.871e-05   1.00
    moe_head  K=2 B=1 temp=1   reg=0   (soft, hard)  d_logits   2.093e-05   2.093e-05   1.00
    moe_head  K=2 B=1 temp=0.1 reg=0   (soft, hard)  d_logits   1.000e+00   1.000e+00   1.00
    moe_head  K=2 B=1 temp=0.1 reg=0.5 (soft, hard)  d_logits   9.999e-01   9.999e-01   1.00
    moe_head  K=3 B=1 temp=0.1 reg=0   (soft, hard)  d_logits   1.692e-01   1.692e-01   1.00
    moe_blend K=2 B=1 temp=0.1 soft               d_logits   3.953e-01   3.953e-01   1.00
    moe_blend K=2 B=1 temp=0.1 hard               d_logits   1.644e-02   1.644e-02   1.00
    moe_blend K=3 B=1 temp=0.1 hard               d_logits   3.465e-04   3.465e-04   1.00
    moe_blend K=4 B=1 temp=0.1 soft               d_logits   2.247e-04   1.352e-03   0.17
    moe_blend K=4 B=1 temp=0.1 hard               d_logits   3.318e-03   1.098e-02   0.30

Large scores: a score of 1e3 carries ~6e-5 of float32 rounding into the exponent, whatever the summation order; the
error sits in the few rows whose two largest scores nearly tie, and kernel and torch round them alike.  Mixture head at
B = 1 with unequal logits: d_logits = z (dw - sum z dw) / temp cancels to the last bit in float32 where one weight
saturates, while the float64 value is a number ~1e-7 of the other terms (or, at temp = 0.1, far smaller): the relative
error of the whole (tiny) vector is then the float32 format's, identical in the kernel and in torch.  With more rows the
maximum of |d_logits| is set by rows that do not cancel, and the comparison sits under the project bar.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests.parity import rel as _rel

EPS = 1e-5
LN_FWD, LN_BWD = 1e-5, 2e-5                  # test_affect.py: LayerNorm and attention
FFN_FWD, FFN_BWD = 2e-5, 1e-4                # test_affect.py: the fused feed-forward block (output, data gradient)
CLIP_REL = 1.2e-7


class _Figures:
    """Collects the comparisons of one test: each prints its figures, the test asserts once at the end."""

    def __init__(self):
        self.bad = []

    def check(self, tag, got, ref64, ref32, project):
        assert tuple(got.shape) == tuple(ref64.shape), (tag, tuple(got.shape), tuple(ref64.shape))
        err, yard = _rel(got, ref64), _rel(ref32, ref64)
        bar = max(project, 4.0 * yard)
        finite = bool(torch.isfinite(got).all())
        print(f'FIG {tag} kernel={err:.3e} f32={yard:.3e} bar={bar:.3e}' + (' RAISED' if err >= project else ''))
        if not (finite and err < bar):
            self.bad.append((tag, err, yard, bar, finite))

    def done(self):
        assert not self.bad, self.bad


# ---------------------------------------------------------------------------------------------------------------
# the restatements (any floating dtype; the tests evaluate them in float64, and in float32 for the yardstick)
# ---------------------------------------------------------------------------------------------------------------
def ref_layernorm(x, res, gamma, beta, eps, keep=None):
    """LayerNorm over D of x * keep + res for x [B, D, T] -> (y, mean [B*T], rstd [B*T]); two-pass variance."""
    v = x if keep is None else x * keep
    if res is not None:
        v = v + res
    mu = v.mean(dim=1, keepdim=True)
    d = v - mu
    rstd = ((d * d).mean(dim=1, keepdim=True) + eps).rsqrt()
    y = d * rstd * gamma[None, :, None] + beta[None, :, None]
    return y, mu.reshape(-1), rstd.reshape(-1)


def ref_attention(qkv, heads, keep=None):
    """softmax attention on the q | k | v channel split of qkv [B, 3D, T] -> (out [B, D, T], probs [B*heads, T, T] before
    dropout); keep: multiplier of the probabilities [B*heads, T, T]."""
    B, D3, T = qkv.shape
    D = D3 // 3
    dh = D // heads
    q, k, v = (t.reshape(B * heads, dh, T).transpose(1, 2) for t in qkv.split(D, dim=1))          # [B*H, T, dh]
    s = (q * dh ** -0.5) @ k.transpose(1, 2)
    e = (s - s.max(dim=-1, keepdim=True).values.detach()).exp()
    p = e / e.sum(dim=-1, keepdim=True)
    pk = p if keep is None else p * keep
    return (pk @ v).transpose(1, 2).reshape(B, D, T), p


def ref_clip(x, max_norm):
    """(norm, coef) of torch.nn.utils.clip_grad_norm_ for one flat gradient."""
    norm = (x * x).sum().sqrt()
    return norm, (max_norm / (norm + 1e-6)).clamp(max=1.0)


def ref_moe(logits, preds, target, temp, hard, reg, d_out=None, d_aux=None):
    """The mixture head in closed form: w = DiffSoftmax(logits / temp, hard), out = sum_k w_k pred_k, aux = mean w[:, K-1],
    loss1 = mean |out - target|, total = loss1 + reg * aux, and the gradients of `total` (target given) or of
    sum(out * d_out) + aux * d_aux (the blend under arbitrary upstream gradients).  The hard path is straight-through: the
    gradient of the logits runs through the soft weights."""
    B, K = logits.shape
    z = (logits / temp).softmax(dim=-1)
    if hard:
        idx = z.max(dim=-1, keepdim=True)[1]                       # first maximal index
        w = torch.zeros_like(z).scatter_(-1, idx, 1.0) - z + z
    else:
        w = z
    P = torch.stack([p.reshape(-1) for p in preds], dim=1)         # [B, K]
    out = (w * P).sum(dim=1)
    aux = w[:, K - 1].mean()
    r = {'out': out, 'weight': w, 'aux': aux}
    if target is not None:
        diff = out - target.reshape(-1)
        r['loss1'] = diff.abs().mean()
        r['total'] = r['loss1'] + reg * aux
        go = torch.sign(diff) / B                                  # sgn(0) = 0
        da = torch.as_tensor(reg, dtype=logits.dtype)
    else:
        go = d_out.reshape(-1)
        da = d_aux
    last = torch.zeros(K, dtype=logits.dtype)
    last[K - 1] = 1.0
    dw = P * go[:, None] + last[None, :] * da / B
    r['d_preds'] = [w[:, k] * go for k in range(K)]
    r['d_logits'] = z * (dw - (z * dw).sum(dim=1, keepdim=True)) / temp
    return r


def ref_ffn(x, w1, b1, w2, keep=None):
    """hidden = relu(W1 x + b1) * keep [B, F, T], out = W2 hidden [B, D, T] (the block's second bias is added by its consumer)."""
    hid = torch.relu(torch.einsum('fd,bdt->bft', w1, x) + b1[None, :, None])
    if keep is not None:
        hid = hid * keep
    return hid, torch.einsum('df,bft->bdt', w2, hid)


def ref_ffn_bwd(dout, hid, w1, w2, scale):
    """dhid = (W2^T dout) * [hid > 0] * scale, dx = W1^T dhid."""
    dhid = torch.einsum('df,bdt->bft', w2, dout) * (hid > 0).to(dout.dtype) * scale
    return dhid, torch.einsum('fd,bft->bdt', w1, dhid)


# ---------------------------------------------------------------------------------------------------------------
# CPU: the restatements against torch's own functions
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,D,T,with_res', [(2, 1, 3, True), (3, 9, 5, False), (2, 129, 7, True), (1, 1024, 4, True)])
def test_ref_layernorm_is_torchs_layer_norm(B, D, T, with_res):
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(B, D, T, generator=g, dtype=torch.float64) + 3.0).requires_grad_(True)
    res = torch.randn(B, D, T, generator=g, dtype=torch.float64).requires_grad_(True) if with_res else None
    gamma = (torch.rand(D, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(D, generator=g, dtype=torch.float64).requires_grad_(True)
    gy = torch.randn(B, D, T, generator=g, dtype=torch.float64)
    leaves = [t for t in (x, res, gamma, beta) if t is not None]
    y, mean, rstd = ref_layernorm(x, res, gamma, beta, EPS)
    got = torch.autograd.grad(y, leaves, gy)
    v = x if res is None else x + res
    want_y = F.layer_norm(v.permute(0, 2, 1), (D,), gamma, beta, EPS).permute(0, 2, 1)
    want = torch.autograd.grad(want_y, leaves, gy)
    assert _rel(y, want_y) < 1e-12
    assert _rel(mean, v.mean(1).reshape(-1)) < 1e-12
    assert _rel(rstd, (v.var(1, unbiased=False) + EPS).rsqrt().reshape(-1)) < 1e-12
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() <= 1e-11 * max(1.0, b.abs().max().item())


@pytest.mark.parametrize('B,dh,heads,T', [(2, 1, 1, 1), (2, 7, 3, 9), (1, 32, 2, 64), (2, 24, 5, 13)])
def test_ref_attention_is_torchs_sdpa(B, dh, heads, T):
    g = torch.Generator().manual_seed(dh * 100 + T)
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
    # the keep multiplier sits on the probabilities, before the product with V
    keep = (torch.rand(B * heads, T, T, generator=g) >= 0.3).double() / 0.7
    out_k, _ = ref_attention(qkv, heads, keep)
    qh, kh, vh = (t.reshape(B * heads, dh, T).transpose(1, 2) for t in qkv.split(D, dim=1))
    want_k = ((torch.softmax(qh @ kh.transpose(1, 2) / dh ** 0.5, -1) * keep) @ vh).transpose(1, 2).reshape(B, D, T)
    assert _rel(out_k, want_k) < 1e-12


@pytest.mark.parametrize('n,scale', [(1, 0.5), (255, 1.0), (4097, 0.01), (4097, 30.0)])
def test_ref_clip_is_torchs_clip_grad_norm(n, scale):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g, dtype=torch.float64) * scale
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    p.grad = x.clone()
    total = torch.nn.utils.clip_grad_norm_([p], 1.0)
    norm, coef = ref_clip(x, 1.0)
    assert abs(norm.item() - total.item()) <= 1e-14 * total.item()
    assert _rel(x * coef, p.grad) < 1e-14
    assert (coef.item() == 1.0) == (norm.item() + 1e-6 <= 1.0)


@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('hard', [False, True])
def test_ref_moe_is_autograd_on_the_reference_formula(K, hard):
    g = torch.Generator().manual_seed(K * 2 + hard)
    B, temp, reg = 37, 0.1, 0.5
    logits = (torch.randint(-16, 17, (B, K), generator=g).double() / 8).requires_grad_(True)
    preds = [torch.randn(B, 1, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(K)]
    target = torch.randn(B, 1, generator=g, dtype=torch.float64)

    def formula():                                                 # DiffSoftmax, blend, L1, reg * mean w[:, K-1]
        y_soft = (logits / temp).softmax(-1)
        if hard:
            index = y_soft.max(-1, keepdim=True)[1]
            y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
            w = y_hard - y_soft.detach() + y_soft
        else:
            w = y_soft
        out = sum(w[:, k:k + 1] * preds[k] for k in range(K))
        aux = w[:, -1].mean()
        loss1 = F.l1_loss(out, target)
        return out, w, aux, loss1, loss1 + reg * aux
    out, w, aux, loss1, total = formula()
    grads = torch.autograd.grad(total, [logits] + preds)
    r = ref_moe(logits.detach(), [p.detach() for p in preds], target, temp, hard, reg)
    assert _rel(r['out'], out.reshape(-1)) < 1e-14 and _rel(r['weight'], w) < 1e-14
    for name, want in (('aux', aux), ('loss1', loss1), ('total', total)):
        assert abs(r[name].item() - want.item()) < 1e-14
    assert _rel(r['d_logits'], grads[0]) < 1e-12
    for a, b in zip(r['d_preds'], grads[1:]):
        assert _rel(a, b.reshape(-1)) < 1e-14
    # arbitrary upstream gradients (the blend under plain autograd)
    d_out = torch.randn(B, generator=g, dtype=torch.float64)
    d_aux = torch.tensor(0.7, dtype=torch.float64)
    out, w, aux, _, _ = formula()
    grads = torch.autograd.grad((out.reshape(-1) * d_out).sum() + aux * d_aux, [logits] + preds)
    r = ref_moe(logits.detach(), [p.detach() for p in preds], None, temp, hard, 0.0, d_out, d_aux)
    assert _rel(r['d_logits'], grads[0]) < 1e-12
    for a, b in zip(r['d_preds'], grads[1:]):
        assert _rel(a, b.reshape(-1)) < 1e-14


def test_ref_moe_ties_and_sign_of_zero():
    """first maximal index on ties (Tensor.max(dim)), and no gradient through |0|."""
    logits = torch.tensor([[1., 1., 0., 1.], [0., 2., 2., 2.], [3., 3., 3., 3.], [0., 0., 1., 1.]], dtype=torch.float64)
    preds = [torch.full((4,), float(k), dtype=torch.float64) for k in range(4)]
    r = ref_moe(logits, preds, torch.tensor([0., 9., 5., 9.], dtype=torch.float64), 1.0, True, 0.0)
    assert r['weight'].argmax(-1).tolist() == [0, 1, 0, 2]
    assert _rel(r['out'], torch.tensor([0., 1., 0., 2.])) < 1e-15 and r['out'][0].item() == 0.0
    assert [d[0].item() for d in r['d_preds']] == [0.0] * 4 and abs(r['d_preds'][0][2].item() + 0.25) < 1e-15


def test_ref_ffn_is_two_linears():
    g = torch.Generator().manual_seed(0)
    B, D, T, Fh = 2, 5, 3, 32
    x = torch.randn(B, D, T, generator=g, dtype=torch.float64, requires_grad=True)
    w1, b1 = torch.randn(Fh, D, generator=g, dtype=torch.float64), torch.randn(Fh, generator=g, dtype=torch.float64)
    w2 = torch.randn(D, Fh, generator=g, dtype=torch.float64)
    keep = (torch.rand(B, Fh, T, generator=g) >= 0.25).double() / 0.75
    hid, out = ref_ffn(x, w1, b1, w2, keep)
    h = torch.relu(F.linear(x.permute(0, 2, 1), w1, b1)) * keep.permute(0, 2, 1)
    want = F.linear(h, w2).permute(0, 2, 1)
    assert _rel(out, want) < 1e-13 and _rel(hid, h.permute(0, 2, 1)) < 1e-13
    gy = torch.randn(B, D, T, generator=g, dtype=torch.float64)
    h.retain_grad()
    want.backward(gy)
    # the keep factor reaches the hidden gradient as the scale 1 / (1 - p) on the units with hid > 0
    dhid, dx = ref_ffn_bwd(gy, hid.detach(), w1, w2, 1 / 0.75)
    assert _rel(dx, x.grad) < 1e-13
    pre = torch.einsum('fd,bdt->bft', w1, x.detach()) + b1[None, :, None]
    assert _rel(dhid, torch.einsum('df,bdt->bft', w2, gy) * keep * (pre > 0)) < 1e-13


# ---------------------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------------------
def _S():
    from dynmm_amd import ops_seq as S
    return S


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cu(t):
    return None if t is None else t.detach().float().contiguous().cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _both(fn, tensors):
    """fn evaluated on float64 and on float32 copies of `tensors` (None passes through): (float64 result, float32 result)."""
    r = []
    for dt in (torch.float64, torch.float32):
        r.append(fn(*[None if t is None else t.detach().to(dt) for t in tensors]))
    return r


class _FixedMasks:
    """S.MASKS hook serving one prepared keep-flag tensor per site name."""

    def __init__(self, **by_name):
        self.by_name = by_name

    def __call__(self, name, shape):
        m = self.by_name[name]
        assert tuple(m.shape) == tuple(shape)
        return m


# ---------------------------------------------------------------------------------------------------------------
# 1. LayerNorm
# ---------------------------------------------------------------------------------------------------------------
LN_DIMS = [1, 7, 8, 9, 127, 128, 129, 255, 256, 257, 300, 512, 513, 1000, 1024]
# (B, T, residual, offset on x): fewer than kLnTok = 16 tokens; not a multiple of 16; mean >> std; 69 workgroups (the parameter
# reduction sees more than 64 rows, and 64 does not divide them)
LN_TOKENS = [(1, 3, True, 0.0), (3, 7, False, 0.0), (2, 21, True, 100.0), (22, 50, True, 0.0)]


def _ln_grads(x, res, gamma, beta, gy, keep=None):
    leaves = [t.requires_grad_(True) for t in (x, res, gamma, beta) if t is not None]
    y, mean, rstd = ref_layernorm(x, res, gamma, beta, EPS, keep)
    gr = list(torch.autograd.grad(y, leaves, gy))
    if res is None:
        gr.insert(1, None)
    return [y.detach(), mean.detach(), rstd.detach()] + gr       # y, mean, rstd, dx, dres, dgamma, dbeta


def _ln_inputs(B, D, T, with_res, offset, seed):
    g = _gen(seed)
    x = torch.randn(B, D, T, generator=g) + offset
    res = torch.randn(B, D, T, generator=g) if with_res else None
    gamma = torch.rand(D, generator=g) + 0.5
    beta = torch.randn(D, generator=g)
    gy = torch.randn(B, D, T, generator=g)
    return x, res, gamma, beta, gy


@pytest.mark.gpu
@pytest.mark.parametrize('D', LN_DIMS)
def test_layernorm_matches_float64(D):
    """ln_fwd_kernel / ln_bwd_dx_kernel on every pass count, through the autograd wrapper (workspace entry: per-workgroup
    parameter sums + ln_param_reduce_kernel) and through the library's two-pass entry (ln_bwd_param_kernel), and the
    null-dx / null-dres variants."""
    S = _S()
    lib, st = S._lib(), S._stream()
    fig = _Figures()
    for B, T, with_res, offset in LN_TOKENS:
        tag = f'ln D={D} B={B} T={T} res={int(with_res)} off={offset:g}'
        x, res, gamma, beta, gy = _ln_inputs(B, D, T, with_res, offset, D * 100 + T)
        r64, r32 = _both(_ln_grads, (x, res, gamma, beta, gy))
        xc, rc, gc, bc = (None if t is None else _cu(t).requires_grad_(True) for t in (x, res, gamma, beta))
        y = S.layernorm_bdt(xc, gc, bc, EPS, residual=rc)
        mean, rstd = y.grad_fn.saved_tensors[3:5]
        y.backward(_cu(gy))
        got = [y, mean, rstd, xc.grad, None if rc is None else rc.grad, gc.grad, bc.grad]
        names = ['y', 'mean', 'rstd', 'dx', 'dres', 'dgamma', 'dbeta']
        for i, n in enumerate(names):
            if got[i] is not None:
                fig.check(f'{tag} ws {n}', got[i], r64[i], r32[i], LN_FWD if i < 3 else LN_BWD)
        # the entry without a workspace; dx and dres both asked for
        xd, rd, gd, gyd = _cu(x), _cu(res), _cu(gamma), _cu(gy)
        mean, rstd = mean.detach(), rstd.detach()
        dx, dres = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
        dg, db = torch.full_like(gd, 7.0), torch.full_like(gd, 7.0)
        rc_ = lib.dynmm_layernorm_drop_bwd(_ptr(gyd), _ptr(xd), _ptr(rd), _ptr(gd), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dres),
                                           _ptr(dg), _ptr(db), B, D, T, None, st)
        assert rc_ == 0
        fig.check(f'{tag} 2pass dx', dx, r64[3], r32[3], LN_BWD)
        fig.check(f'{tag} 2pass dres', dres, r64[3], r32[3], LN_BWD)
        fig.check(f'{tag} 2pass dgamma', dg, r64[5], r32[5], LN_BWD)
        fig.check(f'{tag} 2pass dbeta', db, r64[6], r32[6], LN_BWD)
        # null dx (workspace entry) and null dres (two-pass entry): the other output is what it was with both present
        nb = lib.dynmm_layernorm_bwd_workspace_bytes(B, D, T)
        assert nb == -(-B * T // 16) * 2 * D * 4
        ws = torch.empty(nb // 4, device='cuda')
        dres2, dg2, db2 = torch.full_like(xd, 7.0), torch.full_like(gd, 7.0), torch.full_like(gd, 7.0)
        assert lib.dynmm_layernorm_drop_bwd_ws(_ptr(gyd), _ptr(xd), _ptr(rd), _ptr(gd), _ptr(mean), _ptr(rstd), None, _ptr(dres2),
                                               _ptr(dg2), _ptr(db2), B, D, T, None, _ptr(ws), nb, st) == 0
        dx2 = torch.full_like(xd, 7.0)
        assert lib.dynmm_layernorm_drop_bwd(_ptr(gyd), _ptr(xd), _ptr(rd), _ptr(gd), _ptr(mean), _ptr(rstd), _ptr(dx2), None,
                                            None, None, B, D, T, None, st) == 0
        assert torch.equal(dres2, dres) and torch.equal(dx2, dx), tag
        assert torch.equal(dg2, gc.grad) and torch.equal(db2, bc.grad), tag
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('D', [60, 255, 300, 1001])
def test_layernorm_with_injected_masks(D):
    """keep flags on x at one D per pass count above one, D % 8 != 0: later passes read their own block of flags, the last
    block is partial; dropped elements receive exactly zero gradient."""
    S = _S()
    B, T, p = 3, 21, 0.3
    fig = _Figures()
    x, res, gamma, beta, gy = _ln_inputs(B, D, T, True, 0.0, D)
    m = (torch.rand(B, D, T, generator=_gen(D + 1)) >= p)
    keep = m.float() / (1 - p)
    r64, r32 = _both(_ln_grads, (x, res, gamma, beta, gy, keep))
    xc, rc, gc, bc = (_cu(t).requires_grad_(True) for t in (x, res, gamma, beta))
    S.MASKS = _FixedMasks(dropout1=m.to(torch.uint8).cuda())
    try:
        y = S.layernorm_bdt(xc, gc, bc, EPS, residual=rc, drop=(p, 7, 'dropout1'))
        mean, rstd = (t.detach() for t in y.grad_fn.saved_tensors[3:5])
        y.backward(_cu(gy))
        # the two-pass entry reads the flags one element at a time (keep1)
        desc = S.Drop(p, 7, 'dropout1', (B, D, T), xc.device)
        dg, db = torch.empty(D, device='cuda'), torch.empty(D, device='cuda')
        assert S._lib().dynmm_layernorm_drop_bwd(_ptr(_cu(gy)), _ptr(xc), _ptr(rc), _ptr(gc), _ptr(mean), _ptr(rstd), None, None,
                                                 _ptr(dg), _ptr(db), B, D, T, S._drop_arg(desc), S._stream()) == 0
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    got = [y, None, None, xc.grad, rc.grad, gc.grad, bc.grad]
    for i, n in enumerate(['y', 'mean', 'rstd', 'dx', 'dres', 'dgamma', 'dbeta']):
        if got[i] is not None:
            fig.check(f'ln-mask D={D} {n}', got[i], r64[i], r32[i], LN_FWD if i < 3 else LN_BWD)
    fig.check(f'ln-mask D={D} 2pass dgamma', dg, r64[5], r32[5], LN_BWD)
    fig.check(f'ln-mask D={D} 2pass dbeta', db, r64[6], r32[6], LN_BWD)
    assert bool((xc.grad.cpu()[~m] == 0).all()) and bool((xc.grad.cpu()[m] != 0).any())
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('nparts', [1, 3, 16])
@pytest.mark.parametrize('with_bias', [False, True])
def test_layernorm_parts_matches_float64(nparts, with_bias):
    """dynmm_layernorm_parts_fwd: x arrives as `nparts` slabs (+ a per-channel bias); xsum is their sum, y its LayerNorm."""
    S = _S()
    lib, st = S._lib(), S._stream()
    fig = _Figures()
    for B, D, T in [(1, 35, 3), (3, 120, 21), (2, 300, 37), (2, 1000, 9)]:
        g = _gen(D + nparts)
        parts = torch.randn(nparts, B, D, T, generator=g)
        xbias = torch.randn(D, generator=g) if with_bias else None
        res = torch.randn(B, D, T, generator=g)
        gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)

        def run(parts, xbias, res, gamma, beta):
            xs = parts.sum(0) if xbias is None else parts.sum(0) + xbias[None, :, None]
            return (xs,) + ref_layernorm(xs, res, gamma, beta, EPS)
        r64, r32 = _both(run, (parts, xbias, res, gamma, beta))
        pc, xb, rc, gc, bc = _cu(parts), _cu(xbias), _cu(res), _cu(gamma), _cu(beta)
        xsum, y = torch.full((B, D, T), 7.0, device='cuda'), torch.full((B, D, T), 7.0, device='cuda')
        mean, rstd = torch.empty(B * T, device='cuda'), torch.empty(B * T, device='cuda')
        assert lib.dynmm_layernorm_parts_fwd(_ptr(pc), nparts, _ptr(xb), _ptr(xsum), _ptr(rc), _ptr(gc), _ptr(bc), _ptr(y),
                                             _ptr(mean), _ptr(rstd), B, D, T, EPS, None, st) == 0
        for n, a, i in (('xsum', xsum, 0), ('y', y, 1), ('mean', mean, 2), ('rstd', rstd, 3)):
            fig.check(f'ln-parts D={D} n={nparts} bias={int(with_bias)} {n}', a, r64[i], r32[i], LN_FWD)
    fig.done()


@pytest.mark.gpu
def test_layernorm_refuses_more_than_1024_channels():
    S = _S()
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()
    B, D, T = 2, 1025, 5
    x, res, gamma, beta, gy = (_cu(t) for t in _ln_inputs(B, D, T, True, 0.0, 1))
    mean, rstd = torch.zeros(B * T, device='cuda'), torch.ones(B * T, device='cuda')
    outs = [torch.full((B, D, T), 7.0, device='cuda') for _ in range(2)] + [torch.full((D,), 7.0, device='cuda') for _ in range(2)]
    a, b, c, d = outs
    nb = lib.dynmm_layernorm_bwd_workspace_bytes(B, D, T)
    ws = torch.empty(nb // 4, device='cuda')
    U = L.DYNMM_EUNSUPPORTED
    assert lib.dynmm_layernorm_drop_fwd(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(a), _ptr(mean), _ptr(rstd), B, D, T, EPS,
                                        None, st) == U
    assert lib.dynmm_layernorm_fwd(_ptr(x), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(a), _ptr(mean), _ptr(rstd), B, D, T, EPS,
                                   st) == U
    assert lib.dynmm_layernorm_parts_fwd(_ptr(x), 1, None, _ptr(b), _ptr(res), _ptr(gamma), _ptr(beta), _ptr(a), _ptr(mean),
                                         _ptr(rstd), B, D, T, EPS, None, st) == U
    assert lib.dynmm_layernorm_drop_bwd_ws(_ptr(gy), _ptr(x), _ptr(res), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(a), _ptr(b),
                                           _ptr(c), _ptr(d), B, D, T, None, _ptr(ws), nb, st) == U
    assert lib.dynmm_layernorm_drop_bwd(_ptr(gy), _ptr(x), _ptr(res), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(a), _ptr(b),
                                        _ptr(c), _ptr(d), B, D, T, None, st) == U
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
    with pytest.raises(L.DynmmHipError):
        S.layernorm_bdt(x, gamma, beta, EPS, residual=res)


# the pre-norm layer on the same kernels (dynmm_prenorm_*, ops_seq.prenorm_bdt / residual_add)
PN_DIMS = [7, 129, 300, 1001]                 # one D per pass count 1, 2, 4, 8, none a multiple of 8
PN_TOKENS = [(1, 3), (3, 21)]                 # fewer than 16 tokens; not a multiple of 16
PN_NAMES = ['sum', 'y', 'mean', 'rstd', 'dres', 'dx', 'dgamma', 'dbeta']


def _pn_grads(res, x, gamma, beta, gy, gs, keep=None):
    """(sum, y, mean, rstd, dres, dx, dgamma, dbeta) of sum = res + x * keep (x None: res), y = LayerNorm(sum); gy flows into y
    and gs (optional) into sum."""
    leaves = [t.requires_grad_(True) for t in (res, x, gamma, beta) if t is not None]
    s = res if x is None else (x if keep is None else x * keep) + res
    y, mean, rstd = ref_layernorm(s, None, gamma, beta, EPS)
    gr = list(torch.autograd.grad([y] if gs is None else [y, s], leaves, [gy] if gs is None else [gy, gs]))
    if x is None:
        gr.insert(1, None)
    return [s.detach(), y.detach(), mean.detach(), rstd.detach()] + gr


def _pn_run(S, res, x, gamma, beta, gy, gs, drop=None):
    """the same through prenorm_bdt; the leaves come back for their .grad"""
    rc, xc, gc, bc = (None if t is None else _cu(t).requires_grad_(True) for t in (res, x, gamma, beta))
    out = S.prenorm_bdt(rc, gc, bc, EPS, x=xc, drop=drop)
    s, y = out if x is not None else (None, out)
    mean, rstd = y.grad_fn.saved_tensors[2:4]
    torch.autograd.backward([y] if gs is None else [y, s], [_cu(gy)] if gs is None else [_cu(gy), _cu(gs)])
    return [s, y, mean, rstd, rc.grad, None if xc is None else xc.grad, gc.grad, bc.grad]


@pytest.mark.gpu
@pytest.mark.parametrize('D', PN_DIMS)
def test_prenorm_matches_float64(D):
    """prenorm_bdt on every pass count: without x, with x, with x and injected keep flags; gradients into both outputs and into
    y alone.  Without dropout the sum is res + x to the bit; dropped elements of x receive exactly zero gradient."""
    S = _S()
    p = 0.3
    fig = _Figures()
    for B, T in PN_TOKENS:
        x, res, gamma, beta, gy = _ln_inputs(B, D, T, True, 0.0, D * 100 + T)
        gs_ = torch.randn(B, D, T, generator=_gen(D + T))
        m = (torch.rand(B, D, T, generator=_gen(D + T + 1)) >= p)
        keep = m.float() / (1 - p)
        for form, xin, kp in (('nox', None, None), ('x', x, None), ('mask', x, keep)):
            for gs in ((None,) if xin is None else (gs_, None)):
                tag = f'pn D={D} B={B} T={T} {form} gs={int(gs is not None)}'
                r64, r32 = _both(_pn_grads, (res, xin, gamma, beta, gy, gs, kp))
                S.MASKS = _FixedMasks(res1=m.to(torch.uint8).cuda()) if kp is not None else None
                try:
                    got = _pn_run(S, res, xin, gamma, beta, gy, gs, drop=(p, 7, 'res1') if kp is not None else None)
                    torch.cuda.synchronize()
                finally:
                    S.MASKS = None
                for i, n in enumerate(PN_NAMES):
                    if got[i] is not None:
                        fig.check(f'{tag} {n}', got[i], r64[i], r32[i], LN_FWD if i < 4 else LN_BWD)
                if form == 'x':
                    assert torch.equal(got[0], _cu(res) + _cu(x)), tag
                if form == 'mask':
                    dx = got[5].cpu()
                    assert bool((dx[~m] == 0).all()) and bool((dx[m] != 0).any()), tag
    fig.done()


@pytest.mark.gpu
def test_prenorm_and_layernorm_give_the_same_bits():
    """One kernel: on the same inputs and keep flags prenorm_bdt's y, mean and rstd are layernorm_bdt's."""
    S = _S()
    B, D, T, p = 3, 300, 21, 0.3
    x, res, gamma, beta, _ = (_cu(t) for t in _ln_inputs(B, D, T, True, 0.0, 5))
    m = (torch.rand(B, D, T, generator=_gen(6)) >= p).to(torch.uint8).cuda()
    S.MASKS = _FixedMasks(res1=m)
    try:
        _, y_pn = S.prenorm_bdt(res.requires_grad_(True), gamma, beta, EPS, x=x, drop=(p, 7, 'res1'))
        y_ln = S.layernorm_bdt(x.requires_grad_(True), gamma, beta, EPS, residual=res, drop=(p, 7, 'res1'))
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    assert torch.equal(y_pn, y_ln)
    for a, b in zip(y_pn.grad_fn.saved_tensors[2:4], y_ln.grad_fn.saved_tensors[3:5]):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_prenorm_bwd_accumulates_parameter_gradients():
    """dynmm_prenorm_bwd with accumulate = 1 adds its sums to dgamma / dbeta: one float32 add per element on top of the
    accumulate = 0 result.  69 workgroups: the reduction sees more than 64 rows."""
    S = _S()
    lib, st = S._lib(), S._stream()
    B, D, T = 22, 129, 50
    _, res, gamma, beta, gy = (_cu(t) for t in _ln_inputs(B, D, T, True, 0.0, 3))
    y = torch.empty_like(res)
    mean, rstd = torch.empty(B * T, device='cuda'), torch.empty(B * T, device='cuda')
    assert lib.dynmm_prenorm_fwd(None, _ptr(res), _ptr(gamma), _ptr(beta), None, _ptr(y), _ptr(mean), _ptr(rstd), B, D, T, EPS,
                                 None, st) == 0
    nb = lib.dynmm_prenorm_bwd_workspace_bytes(B, D, T)
    assert nb == -(-B * T // 16) * 2 * D * 4
    ws = torch.empty(nb // 4, device='cuda')
    pre = [torch.randn(D, generator=_gen(4 + i)).cuda() for i in range(2)]
    out = {}
    for acc in (0, 1):
        dg, db = pre[0].clone(), pre[1].clone()
        dres = torch.empty_like(res)
        assert lib.dynmm_prenorm_bwd(_ptr(gy), None, _ptr(res), _ptr(gamma), _ptr(mean), _ptr(rstd), None, _ptr(dres), _ptr(dg),
                                     _ptr(db), B, D, T, None, acc, _ptr(ws), nb, st) == 0
        out[acc] = (dg, db, dres)
    torch.cuda.synchronize()
    assert torch.equal(out[1][0], pre[0] + out[0][0]) and torch.equal(out[1][1], pre[1] + out[0][1])
    assert torch.equal(out[1][2], out[0][2]) and not torch.equal(out[0][0], pre[0])


@pytest.mark.gpu
def test_residual_add_is_exact():
    S = _S()
    g = _gen(11)
    res, x, gy = (_cu(torch.randn(2, 1001, 9, generator=g)) for _ in range(3))
    s = S.residual_add(res.requires_grad_(True), x.requires_grad_(True))
    s.backward(gy)
    assert torch.equal(s, res + x)
    assert torch.equal(res.grad, gy) and torch.equal(x.grad, gy)


@pytest.mark.gpu
def test_prenorm_refusals_write_nothing():
    S = _S()
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()

    def call(B, D, T, beta_null=False, short=0):
        """(forward code, backward code, outputs prefilled with 7.0)"""
        x, res, gamma, beta, gy = (_cu(t) for t in _ln_inputs(B, D, T, True, 0.0, 1))
        mean, rstd = torch.full((B * T,), 7.0, device='cuda'), torch.full((B * T,), 7.0, device='cuda')
        big = [torch.full((B, D, T), 7.0, device='cuda') for _ in range(2)]
        small = [torch.full((D,), 7.0, device='cuda') for _ in range(2)]
        nb = lib.dynmm_prenorm_bwd_workspace_bytes(B, D, T)
        ws = torch.full((nb // 4,), 7.0, device='cuda')
        f = lib.dynmm_prenorm_fwd(_ptr(x), _ptr(res), _ptr(gamma), None if beta_null else _ptr(beta), _ptr(big[0]), _ptr(big[1]),
                                  _ptr(mean), _ptr(rstd), B, D, T, EPS, None, st)
        stats = [torch.zeros(B * T, device='cuda'), torch.ones(B * T, device='cuda')]
        b = lib.dynmm_prenorm_bwd(_ptr(gy), _ptr(x), _ptr(res), _ptr(gamma), _ptr(stats[0]), _ptr(stats[1]), _ptr(big[0]),
                                  _ptr(big[1]), _ptr(small[0]), _ptr(small[1]), B, D, T, None, 0, _ptr(ws), nb - short, st)
        torch.cuda.synchronize()
        return f, b, [mean, rstd, ws] + big + small

    f, b, outs = call(2, 1025, 5)
    assert f == L.DYNMM_EUNSUPPORTED and b == L.DYNMM_EUNSUPPORTED
    assert all(bool((t == 7.0).all()) for t in outs)
    f, b, outs = call(2, 129, 5, beta_null=True, short=1)
    assert f == L.DYNMM_EINVAL and b == L.DYNMM_EWORKSPACE
    assert all(bool((t == 7.0).all()) for t in outs)
    with pytest.raises(L.DynmmHipError):
        S.prenorm_bdt(torch.zeros(2, 1025, 5, device='cuda'), torch.ones(1025, device='cuda'), torch.zeros(1025, device='cuda'))


# ---------------------------------------------------------------------------------------------------------------
# 2. attention core
# ---------------------------------------------------------------------------------------------------------------
# (dh, heads, T, B).  Exact arms dh = 24 / 12 / 2, everything else runs <32, 4, EXACT=false>.  The generic arm at T = 64 is the
# one shape whose backward needs more than 64 KiB of LDS (the opt-in in launch_mha).  The opt-in is remembered per process, so
# only the first generic T = 64 backward takes the branch: here after a T = 63 launch that did not need it.  The later
# T = 64 / T = 63 cases run with the raised limit already in place.
MHA_CASES = [
    (24, 5, 64, 2), (12, 5, 64, 2), (2, 5, 64, 3),
    (24, 1, 1, 1), (24, 2, 7, 2), (24, 4, 33, 1), (24, 8, 50, 1),
    (12, 8, 8, 2), (12, 2, 9, 1), (12, 4, 16, 2), (12, 1, 63, 1),
    (2, 1, 1, 2), (2, 8, 2, 1), (2, 4, 9, 2), (2, 2, 63, 1), (2, 5, 50, 1),
    (32, 4, 63, 2), (32, 4, 64, 2), (31, 2, 64, 1), (31, 5, 63, 1),
    (1, 1, 1, 1), (1, 8, 64, 1), (1, 5, 7, 2), (3, 4, 2, 2), (3, 2, 33, 1), (3, 1, 64, 2),
    (4, 5, 8, 1), (4, 2, 50, 2), (4, 8, 63, 1), (7, 1, 9, 2), (7, 4, 16, 1), (7, 5, 64, 1),
    (8, 2, 1, 3), (8, 8, 33, 1), (8, 1, 64, 1), (16, 4, 2, 1), (16, 5, 50, 1), (16, 2, 63, 2),
    (31, 1, 8, 1), (31, 8, 16, 1), (32, 1, 7, 2), (32, 2, 9, 1), (32, 5, 33, 1), (32, 8, 64, 1),
]


def test_attention_case_list_covers_the_issue():
    assert {c[0] for c in MHA_CASES} == {1, 2, 3, 4, 7, 8, 12, 16, 24, 31, 32}
    assert {c[1] for c in MHA_CASES} == {1, 2, 4, 5, 8}
    assert {c[2] for c in MHA_CASES} == {1, 2, 7, 8, 9, 16, 33, 50, 63, 64}
    assert all(any(c[0] == dh and c[2] == 64 for c in MHA_CASES) for dh in (24, 12, 2))
    generic = [c for c in MHA_CASES if c[0] not in (24, 12, 2)]
    t = [c[2] for c in generic if c[2] in (63, 64)]
    assert t[:2] == [63, 64]
    assert any(c[0] % 4 for c in generic)


def _attn_grads(qkv, gy, heads, keep=None):
    qkv = qkv.requires_grad_(True)
    out, probs = ref_attention(qkv, heads, keep)
    dqkv, = torch.autograd.grad(out, qkv, gy)
    return out.detach(), probs.detach(), dqkv


def _attn_check(fig, tag, qkv, gy, heads, keep_flags=None, p=0.0):
    S = _S()
    keep = None if keep_flags is None else keep_flags.float() / (1 - p)
    r64, r32 = _both(lambda a, b, k: _attn_grads(a, b, heads, k), (qkv, gy, keep))
    qc = _cu(qkv).requires_grad_(True)
    if keep_flags is not None:
        S.MASKS = _FixedMasks(attn=keep_flags.to(torch.uint8).cuda())
    try:
        out = S.mha_core(qc, heads, drop=None if keep_flags is None else (p, 8, 'attn'))
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


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', MHA_CASES, ids=[f'dh{c[0]}-H{c[1]}-T{c[2]}-B{c[3]}' for c in MHA_CASES])
def test_attention_matches_float64(dh, heads, T, B):
    """mha_fwd_kernel / mha_bwd_kernel, one case of the list per test (run in list order): out, the saved probabilities
    (before dropout, rows sum to 1) and dqkv."""
    fig = _Figures()
    g = _gen(dh * 10000 + heads * 100 + T)
    D = dh * heads
    qkv, gy = torch.randn(B, 3 * D, T, generator=g), torch.randn(B, D, T, generator=g)
    _attn_check(fig, f'mha dh={dh} H={heads} T={T} B={B}', qkv, gy, heads)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', [(24, 5, 64, 8), (12, 2, 50, 8), (2, 4, 9, 8), (7, 3, 33, 8), (32, 2, 64, 8), (1, 2, 16, 8)])
def test_attention_is_stable_at_large_scores(dh, heads, T, B):
    """scores of magnitude ~1e3 (q scaled): finite, and equal to the reference, which subtracts the row maximum."""
    g = _gen(dh + T)
    D = dh * heads
    qkv, gy = torch.randn(B, 3 * D, T, generator=g), torch.randn(B, D, T, generator=g)
    qkv[:, :D] *= 1e3                                              # q . k / sqrt(dh) then has standard deviation ~1e3
    fig = _Figures()
    _attn_check(fig, f'mha-big dh={dh} H={heads} T={T}', qkv, gy, heads)
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('dh,heads,T,B', [(7, 3, 33, 2), (16, 2, 64, 1), (31, 1, 7, 2), (3, 4, 13, 1), (32, 4, 63, 1), (24, 5, 13, 1)])
def test_attention_with_injected_masks(dh, heads, T, B):
    """keep flags on the probabilities, generic arm, also at T % 8 != 0 (the last row8 chunk is partial)."""
    g = _gen(dh * 7 + T)
    D, p = dh * heads, 0.25
    qkv, gy = torch.randn(B, 3 * D, T, generator=g), torch.randn(B, D, T, generator=g)
    flags = torch.rand(B * heads, T, T, generator=g) >= p
    fig = _Figures()
    _attn_check(fig, f'mha-mask dh={dh} H={heads} T={T}', qkv, gy, heads, flags, p)
    fig.done()


@pytest.mark.gpu
def test_attention_refusals_write_nothing():
    S = _S()
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()
    for B, D, T, heads, want in [(1, 8, 65, 2, L.DYNMM_EUNSUPPORTED), (1, 66, 8, 2, L.DYNMM_EUNSUPPORTED),
                                 (2, 10, 8, 3, L.DYNMM_EINVAL)]:
        qkv = torch.randn(B, 3 * D, T, device='cuda')
        gy = torch.randn(B, D, T, device='cuda')
        out = torch.full((B, D, T), 7.0, device='cuda')
        probs = torch.full((B * heads, T, T), 7.0, device='cuda')
        dqkv = torch.full((B, 3 * D, T), 7.0, device='cuda')
        assert lib.dynmm_mha_drop_fwd(_ptr(qkv), _ptr(out), _ptr(probs), B, D, T, heads, None, st) == want
        assert lib.dynmm_mha_fwd(_ptr(qkv), _ptr(out), _ptr(probs), B, D, T, heads, st) == want
        assert lib.dynmm_mha_drop_bwd(_ptr(gy), _ptr(qkv), _ptr(probs), _ptr(dqkv), B, D, T, heads, None, st) == want
        assert lib.dynmm_mha_bwd(_ptr(gy), _ptr(qkv), _ptr(probs), _ptr(dqkv), B, D, T, heads, st) == want
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in (out, probs, dqkv))
        with pytest.raises(L.DynmmHipError):
            S.mha_core(qkv, heads)


# ---------------------------------------------------------------------------------------------------------------
# 3. mixture head
# ---------------------------------------------------------------------------------------------------------------
MOE_B = [1, 37, 256, 257, 1000]
MOE_TEMP = [1.0, 0.1, 0.001]


def _moe_inputs(B, K, seed):
    g = _gen(seed)
    logits = torch.randint(-16, 17, (B, K), generator=g).float() / 8      # multiples of 1/8: one arg-max in float32 and float64
    preds = [torch.randn(B, 1, generator=g) for _ in range(K)]
    target = torch.randn(B, 1, generator=g)
    return logits, preds, target


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 2, 3, 4])
@pytest.mark.parametrize('hard', [False, True])
def test_moe_head_matches_float64(K, hard):
    """moe_head_kernel through ops_seq.moe_loss_backward: out, weight, loss1 / aux / total, every d_pred and d_logits; experts
    with and without a gradient (null entries of d_preds: covered by the launch completing and every other output matching)."""
    S = _S()
    fig = _Figures()
    n = 0
    for B in MOE_B:
        for temp in MOE_TEMP:
            for reg in (0.0, 0.5):
                n += 1
                needs = [bool((n >> k) & 1) for k in range(K)]     # which experts ask for a gradient: every pattern over the loop
                tag = f'moe K={K} hard={int(hard)} B={B} temp={temp:g} reg={reg:g}'
                logits, preds, target = _moe_inputs(B, K, n * 10 + K)
                r64, r32 = _both(lambda lg, tg, *ps: ref_moe(lg, ps, tg, temp, hard, reg), (logits, target, *preds))
                lc = _cu(logits).requires_grad_(True)
                pc = [_cu(p).requires_grad_(nd) for p, nd in zip(preds, needs)]
                r = S.moe_loss_backward(lc, pc, _cu(target), temp, hard, reg)
                torch.cuda.synchronize()
                fig.check(f'{tag} out', r['out'].reshape(-1), r64['out'], r32['out'], LN_FWD)
                fig.check(f'{tag} weight', r['weight'], r64['weight'], r32['weight'], LN_FWD)
                for name in ('loss1', 'aux', 'total'):
                    fig.check(f'{tag} {name}', r[name].reshape(()), r64[name], r32[name], LN_FWD)
                fig.check(f'{tag} d_logits', lc.grad, r64['d_logits'], r32['d_logits'], LN_BWD)
                for k in range(K):
                    if needs[k]:
                        fig.check(f'{tag} d_pred{k}', pc[k].grad.reshape(-1), r64['d_preds'][k], r32['d_preds'][k], LN_BWD)
                if hard:                                           # the decision itself: no case left out
                    assert torch.equal(r['weight'].argmax(-1).cpu(), r64['weight'].argmax(-1)), tag
    fig.done()


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 2, 3, 4])
def test_moe_blend_matches_float64(K):
    """ops_seq.moe_blend under plain autograd with arbitrary upstream gradients (moe_head_kernel without a target +
    moe_blend_bwd_kernel)."""
    S = _S()
    fig = _Figures()
    n = 0
    for B in MOE_B:
        for temp in MOE_TEMP:
            for hard in (False, True):
                n += 1
                tag = f'blend K={K} hard={int(hard)} B={B} temp={temp:g}'
                logits, preds, _ = _moe_inputs(B, K, n * 10 + K + 5)
                g = _gen(n)
                d_out, d_aux = torch.randn(B, generator=g), torch.randn((), generator=g)
                r64, r32 = _both(lambda lg, do, da, *ps: ref_moe(lg, ps, None, temp, hard, 0.0, do, da),
                                 (logits, d_out, d_aux, *preds))
                lc = _cu(logits).requires_grad_(True)
                pc = [_cu(p).requires_grad_(True) for p in preds]
                out, aux, weight = S.moe_blend(lc, pc, temp, hard)
                ((out.reshape(-1) * _cu(d_out)).sum() + aux * _cu(d_aux)).backward()
                torch.cuda.synchronize()
                fig.check(f'{tag} out', out.reshape(-1), r64['out'], r32['out'], LN_FWD)
                fig.check(f'{tag} weight', weight, r64['weight'], r32['weight'], LN_FWD)
                fig.check(f'{tag} aux', aux.reshape(()), r64['aux'], r32['aux'], LN_FWD)
                fig.check(f'{tag} d_logits', lc.grad, r64['d_logits'], r32['d_logits'], LN_BWD)
                for k in range(K):
                    fig.check(f'{tag} d_pred{k}', pc[k].grad.reshape(-1), r64['d_preds'][k], r32['d_preds'][k], LN_BWD)
    fig.done()


@pytest.mark.gpu
def test_moe_head_ties_take_the_first_maximal_index():
    S = _S()
    rows = [[1., 1., 0., 1.], [0., 2., 2., 2.], [3., 3., 3., 3.], [0., 0., 1., 1.], [-1., -2., -1., -3.], [0., 0., 0., .125]]
    logits = torch.tensor(rows * 50)                               # 300 rows: both trips of the stride-256 loop
    B = logits.shape[0]
    preds = [torch.full((B, 1), float(k + 1)) for k in range(4)]
    want = torch.tensor([0, 1, 0, 2, 0, 3] * 50)
    for temp in MOE_TEMP:
        r = S.moe_loss_backward(_cu(logits), [_cu(p) for p in preds], _cu(torch.zeros(B, 1)), temp, True, 0.0)
        w = r['weight'].cpu()
        assert torch.equal(w.argmax(-1), want)
        assert torch.equal((w > 0.5).sum(-1), torch.ones(B, dtype=torch.long))
        assert _rel(r['out'].reshape(-1), (want + 1).double()) < 1e-6
        r64 = ref_moe(logits.double(), [p.double() for p in preds], torch.zeros(B, dtype=torch.float64), temp, True, 0.0)
        assert torch.equal(r64['weight'].argmax(-1), want)
    for K in (2, 3):                                               # the same rule with fewer experts
        r = S.moe_loss_backward(_cu(logits[:, :K]), [_cu(p) for p in preds[:K]], _cu(torch.zeros(B, 1)), 1.0, True, 0.0)
        assert r['weight'].argmax(-1).tolist() == [row[:K].index(max(row[:K])) for row in rows * 50]


@pytest.mark.gpu
def test_moe_head_sign_of_zero_is_zero():
    """rows with target == out exactly: no gradient through |0|.  Tied logits give weights of exactly 1/2 and predictions
    on a grid of 1/8 give an `out` that is exact in float32 and float64 alike."""
    S = _S()
    B, K, reg, temp = 300, 2, 0.5, 0.1
    g = _gen(3)
    logits = torch.zeros(B, K)
    logits[1::3, 1] = 0.25                                         # (some rows with unequal weights: their target is elsewhere)
    preds = [torch.randint(-16, 17, (B, 1), generator=g).float() / 8 for _ in range(K)]
    exact = (preds[0] + preds[1]) / 2
    target = torch.where((torch.arange(B) % 3 == 0)[:, None], exact, exact + 1.0)
    r64, r32 = _both(lambda lg, tg, *ps: ref_moe(lg, ps, tg, temp, False, reg), (logits, target, *preds))
    lc = _cu(logits).requires_grad_(True)
    pc = [_cu(p).requires_grad_(True) for p in preds]
    r = S.moe_loss_backward(lc, pc, _cu(target), temp, False, reg)
    zero = torch.arange(B) % 3 == 0
    fig = _Figures()
    for k in range(K):
        assert bool((pc[k].grad.cpu().reshape(-1)[zero] == 0).all()) and bool((r64['d_preds'][k][zero] == 0).all())
        fig.check(f'moe-sgn0 d_pred{k}', pc[k].grad.reshape(-1), r64['d_preds'][k], r32['d_preds'][k], LN_BWD)
    fig.check('moe-sgn0 d_logits', lc.grad, r64['d_logits'], r32['d_logits'], LN_BWD)
    fig.check('moe-sgn0 loss1', r['loss1'].reshape(()), r64['loss1'], r32['loss1'], LN_FWD)
    fig.check('moe-sgn0 total', r['total'].reshape(()), r64['total'], r32['total'], LN_FWD)
    fig.done()


# ---------------------------------------------------------------------------------------------------------------
# 4. gradient-norm clipping
# ---------------------------------------------------------------------------------------------------------------
def _clip_check(tag, x, max_norm):
    S = _S()
    max_norm = torch.tensor(max_norm, dtype=torch.float32).item()  # the kernel takes max_norm as a float
    got = S.clip_grad_norm(x.cuda(), max_norm).cpu().double()
    norm, coef = ref_clip(x.double(), torch.tensor(max_norm, dtype=torch.float64))
    en, ec = abs(got[0].item() - norm.item()) / norm.item(), abs(got[1].item() - coef.item()) / coef.item()
    print(f'FIG {tag} max_norm={max_norm:g} norm={norm.item():.9e} rel(norm)={en:.3e} rel(coef)={ec:.3e}')
    assert en <= CLIP_REL and ec <= CLIP_REL, (tag, en, ec)
    return got, norm


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 255, 4096, 4097, 4096 * 1024 + 5])
def test_clip_grad_norm_matches_float64(n):
    """sumsq_partial_kernel + clip_coef_kernel; the last n crosses the 1024-block cap (grid-stride loop)."""
    x = torch.randn(n, generator=_gen(n))
    x[-1] = 3.0                                                    # (the tail past the last full block carries weight)
    norm = x.double().norm().item()
    got, _ = _clip_check(f'clip n={n} below', x, 2.0 * norm + 1.0)
    assert got[1].item() == 1.0
    _clip_check(f'clip n={n} above', x, 0.37 * norm)
    _clip_check(f'clip n={n} far above', x, 1e-3)


@pytest.mark.gpu
def test_clip_grad_norm_mixed_magnitudes():
    """one buffer mixing magnitudes from 1e-18 to 1e15 (its squares span 66 decades but stay representable), and two buffers
    whose every square underflows (1e-30) or overflows (1e25) float32 but not the double accumulator."""
    n = 4097
    g = _gen(5)
    x = torch.randn(n, generator=g) * 10.0 ** torch.linspace(-18, 15, n)[torch.randperm(n, generator=g)]
    _clip_check('clip mixed', x, 1.0)
    tiny = torch.full((n,), 1e-30)
    assert bool((tiny * tiny == 0).all())
    got, _ = _clip_check('clip tiny', tiny, 1.0)
    assert got[1].item() == 1.0 and got[0].item() > 0
    huge = torch.randn(n, generator=g) * 1e25
    assert not bool(torch.isfinite(huge * huge).any())
    _clip_check('clip huge', huge, 1.0)


# ---------------------------------------------------------------------------------------------------------------
# 5. fused feed-forward
# ---------------------------------------------------------------------------------------------------------------
FFN_D = [1, 3, 4, 35, 60, 64, 120, 124, 128]             # (60 and 64: the two kernel instantiations the rest of the list skips)
FFN_F = [32, 64, 96, 2048]
FFN_TOK = [(3, 7), (2, 64), (5, 50)]                               # B * T = 21 (below), 128 (at), 250 (not a multiple of 128)


def _splits(Fh):
    return [s for s in range(1, 17) if (Fh // 32) % s == 0]


def test_ffn_split_lists():
    assert [_splits(f) for f in FFN_F] == [[1], [1, 2], [1, 3], [1, 2, 4, 8, 16]]


def _ffn_run(S, x, w1, b1, w2, ns, flags=None, p=0.0):
    """dynmm_ffn_fwd + the slab sum -> (hidden, out)."""
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()
    B, D, T = x.shape
    Fh = w1.shape[0]
    hid = torch.full((B, Fh, T), 7.0, device='cuda')
    parts = torch.full((ns, B, D, T), 7.0, device='cuda')
    drop = None if flags is None else C.byref(L.Dropout(_ptr(flags), None, 0, 0, p))
    assert lib.dynmm_ffn_fwd(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(hid), _ptr(parts), B, D, T, Fh, ns, drop, st) == 0
    out = torch.empty_like(x)
    assert lib.dynmm_reduce_slabs(_ptr(parts), _ptr(out), x.numel(), ns, st) == 0
    return hid, out, parts


@pytest.mark.gpu
@pytest.mark.parametrize('D', FFN_D)
@pytest.mark.parametrize('Fh', FFN_F)
def test_ffn_matches_float64_at_every_split(D, Fh):
    """ffn_kernel forward and data backward at every admissible nsplit, with and without injected hidden-layer keep flags,
    against two float64 matrix products."""
    S = _S()
    lib, st = S._lib(), S._stream()
    fig = _Figures()
    p = 0.25
    for B, T in FFN_TOK:
        g = _gen(D * 1000 + Fh + T)
        x, gy = torch.randn(B, D, T, generator=g), torch.randn(B, D, T, generator=g)
        w1, b1 = torch.randn(Fh, D, generator=g) / max(D, 1) ** 0.5, torch.randn(Fh, generator=g) * 0.5
        w2 = torch.randn(D, Fh, generator=g) / Fh ** 0.5
        flags = torch.rand(B, Fh, T, generator=g) >= p
        xc, gc, w1c, b1c, w2c = (_cu(t) for t in (x, gy, w1, b1, w2))
        assert S.ffn_fused_ok(xc, w1c, b1c, w2c, torch.zeros(D, device='cuda'))
        assert lib.dynmm_ffn_nsplit(B, D, T, Fh) in _splits(Fh)
        for masked in (False, True):
            keep = flags.float() / (1 - p) if masked else None
            scale = 1 / (1 - p) if masked else 1.0

            r64, r32 = _both(ref_ffn, (x, w1, b1, w2, keep))
            # the backward reads the sign pattern of the hidden activation it is given: one pattern for all three sides
            hid_in = r64[0].float()
            b64, b32 = _both(lambda gy, hid, w1, w2: ref_ffn_bwd(gy, hid, w1, w2, scale), (gy, hid_in, w1, w2))
            r64, r32 = r64 + b64, r32 + b32
            fc = flags.to(torch.uint8).cuda() if masked else None
            hid_in = _cu(hid_in)
            for ns in (_splits(Fh) if not masked else _splits(Fh)[-1:]):
                tag = f'ffn D={D} F={Fh} BT={B * T} ns={ns} mask={int(masked)}'
                hid, out, _ = _ffn_run(S, xc, w1c, b1c, w2c, ns, fc, p)
                fig.check(f'{tag} hidden', hid, r64[0], r32[0], FFN_FWD)
                fig.check(f'{tag} out', out, r64[1], r32[1], FFN_FWD)
                if masked:
                    assert bool((hid.cpu()[~flags] == 0).all())
                dhid = torch.full((B, Fh, T), 7.0, device='cuda')
                slabs = torch.full((ns, B, D, T), 7.0, device='cuda')
                assert lib.dynmm_ffn_bwd_data(_ptr(gc), _ptr(hid_in), _ptr(w1c), _ptr(w2c), _ptr(dhid), _ptr(slabs), B, D, T, Fh, ns,
                                              p if masked else 0.0, st) == 0
                dx = torch.empty_like(xc)
                assert lib.dynmm_reduce_slabs(_ptr(slabs), _ptr(dx), xc.numel(), ns, st) == 0
                fig.check(f'{tag} dhidden', dhid, r64[2], r32[2], FFN_BWD)
                fig.check(f'{tag} dx', dx, r64[3], r32[3], FFN_BWD)
    fig.done()


@pytest.mark.gpu
def test_ffn_refusals_agree_with_ffn_fused_ok():
    S = _S()
    from dynmm_amd import lib as L
    lib, st = S._lib(), S._stream()
    B, T = 2, 9

    def tensors(D, Fh, misalign):
        x = torch.randn(B, D, T, device='cuda')
        if misalign:                                               # contiguous [F, D] weights 4 bytes off a 16-byte boundary
            w1 = torch.randn(Fh * D + 4, device='cuda')[1:1 + Fh * D].view(Fh, D)
            assert w1.data_ptr() % 16 == 4 and w1.is_contiguous()
        else:
            w1 = torch.randn(Fh, D, device='cuda')
        return x, w1, torch.randn(Fh, device='cuda'), torch.randn(D, Fh, device='cuda'), torch.randn(D, device='cuda')

    for D, Fh, misalign, ok in [(128, 64, False, True), (129, 64, False, False), (64, 48, False, False), (64, 64, True, False)]:
        x, w1, b1, w2, b2 = tensors(D, Fh, misalign)
        assert S.ffn_fused_ok(x, w1, b1, w2, b2) == ok, (D, Fh, misalign)
        hid = torch.full((B, Fh, T), 7.0, device='cuda')
        parts = torch.full((1, B, D, T), 7.0, device='cuda')
        want = 0 if ok else L.DYNMM_EUNSUPPORTED
        assert lib.dynmm_ffn_fwd(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(hid), _ptr(parts), B, D, T, Fh, 1, None, st) == want
        dhid = torch.full((B, Fh, T), 7.0, device='cuda')
        slabs = torch.full((1, B, D, T), 7.0, device='cuda')
        assert lib.dynmm_ffn_bwd_data(_ptr(x), _ptr(hid), _ptr(w1), _ptr(w2), _ptr(dhid), _ptr(slabs), B, D, T, Fh, 1, 0.0,
                                      st) == want
        torch.cuda.synchronize()
        untouched = all(bool((t == 7.0).all()) for t in (hid, parts, dhid, slabs))
        assert untouched != ok
        assert (lib.dynmm_ffn_nsplit(B, D, T, Fh) > 0) == (lib.dynmm_ffn_supported(B, D, T, Fh) == 1)
    # a split that does not divide F / 32 is an argument error, not a geometry the kernel lacks
    x, w1, b1, w2, _ = tensors(64, 96, False)
    hid, parts = torch.empty(B, 96, T, device='cuda'), torch.empty(2, B, 64, T, device='cuda')
    assert lib.dynmm_ffn_fwd(_ptr(x), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(hid), _ptr(parts), B, 64, T, 96, 2, None,
                             st) == L.DYNMM_EINVAL


# ---------------------------------------------------------------------------------------------------------------
# 6. the plain dropout op
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 1000, 4096 * 256 + 77])
def test_dropout_apply_with_injected_mask(n):
    """dropout_kernel at n not a multiple of 256 and above 4096 * 256 elements (the grid-stride branch)."""
    S = _S()
    p = 0.3
    g = _gen(n)
    x, gy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    flags = torch.rand(n, generator=g) >= p
    keep = flags.double() / (1 - p)
    xc = _cu(x).requires_grad_(True)
    S.MASKS = _FixedMasks(dropout=flags.to(torch.uint8).cuda())
    try:
        y = S.dropout_bdt(xc, p, 9, 'dropout')
        y.backward(_cu(gy))
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    ey, eg = _rel(y, x.double() * keep), _rel(xc.grad, gy.double() * keep)
    print(f'FIG dropout n={n} y={ey:.3e} dx={eg:.3e}')
    assert ey < 1e-6 and eg < 1e-6
    assert bool((y.cpu()[~flags] == 0).all()) and bool((xc.grad.cpu()[~flags] == 0).all())

"""autograd shells for the modality-level DynMM path (ModalityDynMM/affect/affect_dyn.py, BASELINE configs[4]).

Activations are [B, D, T] fp32 (the layout the reference feeds its Conv1d after `x.permute([0, 2, 1])`); every Linear
/ Conv1d(k=1) is `linear_bdt` = the implicit-GEMM MFMA convolution of ops.conv2d with H = 1, W = T.  The kernels
added for this path live in csrc/seq.hip (with MULT's pre-norm plumbing; attention for head dimensions above 32: csrc/attn.hip;
MULT's masked cross-modal attention and embedding: csrc/xattn.hip; attention beyond 64 steps: csrc/attn_long.hip).  As everywhere
in dynmm_amd there is no CPU / eager fallback.
"""
import ctypes as C
import itertools
from collections import namedtuple

import torch
from torch.autograd import Function

from . import lib as L
from . import ops
from .ops import _chk, _grad_dst, _grads_enqueued, _lib, _operand, _p, _ptr_array, _stream


def linear_bdt(x, weight, bias=None, act=None, defer_mask=False, mask_input=False, link=None):
    """act(W x + b) over the channel axis of x [B, Ci, T] (or [B, Ci]): weight [Co, Ci] (nn.Linear,
    in_proj_weight) or [Co, Ci, 1] (nn.Conv1d).  defer_mask / mask_input: the ReLU backward of a `defer_mask` layer is
    applied in the input-gradient epilogue of its single consumer (`mask_input`), as in the conv blocks.  link: ops.GradLink
    through which x's OTHER consumer (the residual input of the layer's LayerNorm) hands its gradient to this op's
    input-gradient epilogue."""
    squeeze = x.dim() == 2
    x4 = x.reshape(x.shape[0], x.shape[1], 1, -1) if not squeeze else x.reshape(x.shape[0], x.shape[1], 1, 1)
    shape4 = (weight.shape[0], weight.shape[1], 1, 1)
    train_w = weight.requires_grad and torch.is_grad_enabled()
    # the parameter itself owns the gradient (same memory layout as its [Co, Ci, 1, 1] alias): the in-place gradient
    # protocol writes straight into weight.grad, plain autograd gets it back through _Alias
    w4 = _Alias.apply(weight, shape4) if train_w else weight.detach().view(shape4)
    fuse = torch.is_grad_enabled() and x.requires_grad
    y = ops.conv2d(x4, w4, bias, 1, 0, act, defer_mask=defer_mask and fuse, mask_input=mask_input and fuse,
                   link=link if fuse else None, w_owner=weight if train_w else None)
    return y.reshape(y.shape[0], y.shape[1]) if squeeze else y.reshape(y.shape[0], y.shape[1], -1)


# ---------------------------------------------------------------------------------------------------------------
# dropout (nn.TransformerEncoderLayer trains with p = 0.1 at four sites per layer)
# ---------------------------------------------------------------------------------------------------------------
# A site is an integer; its keep decisions are Philox(seed, (site << 32) + device step counter, element index)
# (csrc/dropout.h): nothing is stored for the backward, and a captured step draws new masks at every replay because the
# counter lives on the device (advance_dropout_step(), called once per training step).
MASKS = None            # tests: callable(site_name, shape) -> uint8 keep flags (device tensor) or None
_SITE_IDS = itertools.count(1)
_STEP = {}


def new_sites(n):
    """n consecutive site ids (one encoder layer takes 4)."""
    first = next(_SITE_IDS)
    for _ in range(n - 1):
        next(_SITE_IDS)
    return first


def dropout_step(device):
    t = _STEP.get(device)
    if t is None:
        t = _STEP[device] = torch.zeros(1, device=device, dtype=torch.int64)
    return t


def advance_dropout_step(device):
    dropout_step(device).add_(1)


class Drop:
    """One dropout site of one call: probability, site id and (tests) the injected keep flags."""

    def __init__(self, p, site, name, shape, device):
        self.p, self.site = float(p), int(site)
        self.mask = None
        if MASKS is not None and self.p > 0:
            m = MASKS(name, tuple(shape))
            if m is not None:
                if m.dtype != torch.uint8 or tuple(m.shape) != tuple(shape) or not m.is_cuda:
                    raise L.DynmmHipError(f'dropout mask for {name}: expected uint8 {tuple(shape)} on the device')
                self.mask = m.contiguous()
        self.step = dropout_step(device) if self.p > 0 else None

    def desc(self):
        return L.Dropout(_p(self.mask), _p(self.step), ops._PHILOX_SEED, self.site << 32, self.p)


def _drop_arg(d):
    return C.byref(d.desc()) if d is not None and d.p > 0 else None


def _make_drop(d, shape, device):
    """the Drop of one call from d = (p, site, name); None for d None or p == 0"""
    return Drop(d[0], d[1], d[2], shape, device) if d is not None and d[0] > 0 else None


class _DropoutBDT(Function):
    @staticmethod
    def forward(ctx, x, drop):
        x = _chk(x, 'x')
        y = torch.empty_like(x)
        L.check(_lib().dynmm_dropout_apply(_p(x), _p(y), C.c_size_t(x.numel()), _drop_arg(drop), _stream()), 'dropout')
        ctx.drop = drop
        return y

    @staticmethod
    def backward(ctx, g):
        g = _chk(g, 'grad')
        dx = torch.empty_like(g)
        L.check(_lib().dynmm_dropout_apply(_p(g), _p(dx), C.c_size_t(g.numel()), _drop_arg(ctx.drop), _stream()), 'dropout')
        return dx, None


def dropout_bdt(x, p, site, name='dropout'):
    """x * keep / (1 - p) (nn.Dropout in training mode); identity when p == 0."""
    if not p > 0:
        return x
    return _DropoutBDT.apply(x, Drop(p, site, name, x.shape, x.device))


class _Alias(Function):
    """weight viewed as [Co, Ci, 1, 1]; the gradient comes back in the same memory layout."""

    @staticmethod
    def forward(ctx, w, shape):
        ctx.shape = tuple(w.shape)
        # under the in-place gradient protocol the convolution returns no gradient for the alias: without this autograd would
        # materialise a zero tensor for it and ADD it to the parameter's .grad (round 6 census of the MOSEI step: 61 zeros + 61
        # add_ launches per step)
        ctx.set_materialize_grads(False)
        return w.view(shape)

    @staticmethod
    def backward(ctx, g):
        return (None if g is None else g.reshape(ctx.shape)), None


def _ln_ws(lib, like, B, D, T, params):
    """(workspace, bytes) of the LayerNorm backward's per-workgroup parameter sums; (None, 0) without parameter gradients."""
    if not params:
        return None, 0
    nb = lib.dynmm_layernorm_bwd_workspace_bytes(B, D, T)
    return torch.empty(nb // 4, device=like.device, dtype=torch.float32), nb


def _ln_stats(like, B, T):
    """(mean, rstd) of B * T tokens, to be filled by a LayerNorm forward"""
    return tuple(torch.empty(B * T, device=like.device, dtype=torch.float32) for _ in range(2))


def _ln_grad_bufs(like, need_x, need_res, drop, dres=None):
    """(dx, dres, gx) for the backward of dropout(x) + res: without dropout the two branches of the sum receive the same tensor
    (dres, allocated unless given; dx is None); with it x gets its keep factor on top (dx).  gx: x's gradient, if needed."""
    dropping = drop is not None and drop.p > 0
    if dres is None and (need_res or (need_x and not dropping)):
        dres = torch.empty_like(like)
    dx = torch.empty_like(like) if (need_x and dropping) else None
    return dx, dres, ((dx if dropping else dres) if need_x else None)


class _LayerNormBDT(Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, drop=None, res_link=None):
        lib = _lib()
        ctx.res_link = res_link
        x, res, gamma, beta = _chk(x, 'x'), _chk(res, 'res'), _chk(gamma, 'gamma'), _chk(beta, 'beta')
        B, D, T = x.shape
        y = torch.empty_like(x)
        mean, rstd = _ln_stats(x, B, T)
        L.check(lib.dynmm_layernorm_drop_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), B, D, T,
                                             float(eps), _drop_arg(drop), _stream()), 'layernorm_fwd')
        ctx.drop = drop
        ctx.save_for_backward(x, res, gamma, mean, rstd)
        ctx.g_param, ctx.b_param = gamma, beta
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib()
        x, res, gamma, mean, rstd = ctx.saved_tensors
        g = _chk(g, 'grad')
        B, D, T = x.shape
        need_x = ctx.needs_input_grad[0]
        need_res = res is not None and ctx.needs_input_grad[1]
        dx, dres, gx = _ln_grad_bufs(x, need_x, need_res, ctx.drop)
        dg = dg_ret = db = db_ret = None
        if ctx.needs_input_grad[2]:
            dg, dg_ret = _grad_dst(ctx.g_param)
            db, db_ret = _grad_dst(ctx.b_param)
        ws, nb = _ln_ws(lib, g, B, D, T, dg is not None)
        L.check(lib.dynmm_layernorm_drop_bwd_ws(_p(g), _p(x), _p(res), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dres), _p(dg),
                                                _p(db), B, D, T, _drop_arg(ctx.drop), _p(ws), nb, _stream()), 'layernorm_bwd')
        _grads_enqueued()
        if need_res and ctx.res_link is not None:
            # the residual input's other consumer adds this gradient in its own input-gradient epilogue (ops.GradLink): no
            # accumulation pass by autograd
            ctx.res_link.dres = dres.reshape(B, D, 1, T)
            need_res = False
        return gx, (dres if need_res else None), dg_ret, db_ret, None, None, None


def layernorm_bdt(x, gamma, beta, eps=1e-5, residual=None, drop=None, res_link=None):
    """LayerNorm over D of (dropout(x) + residual), x [B, D, T]; drop = (p, site, name) or None.  res_link: an ops.GradLink
    shared with the linear_bdt that also consumes `residual` and whose output this layer's x descends from (so its backward
    runs after this one): the residual branch's gradient is added there instead of by autograd."""
    d = _make_drop(drop, x.shape, x.device)
    if not (res_link is not None and residual is not None and torch.is_grad_enabled() and residual.requires_grad):
        res_link = None
    return _LayerNormBDT.apply(x, residual, gamma, beta, eps, d, res_link)


FFN_FUSED = True         # (module attribute: tests compare with the unfused feed-forward)


def ffn_fused_ok(x, w1, b1, w2, b2):
    """the one-launch feed-forward block (csrc/seq_ffn.hip) serves this layer"""
    if not (FFN_FUSED and x.dim() == 3 and b1 is not None and b2 is not None):
        return False
    B, D, T = x.shape
    return bool(_lib().dynmm_ffn_supported(B, D, T, w1.shape[0])) and \
        all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in (w1, b1, w2))


def _wgrad_1x1(x3, gy3, w_param, b_param):
    """weight (+ bias) gradient of a Linear over the channel axis of x3 [B, Ci, T] given gy3 [B, Co, T]: queued for a grouped
    launch under the in-place gradient protocol, launched at once otherwise.  Returns (dw, db) for autograd (None = written in
    place)."""
    lib = _lib()
    B, Ci, T = x3.shape
    Co = gy3.shape[1]
    g = L.ConvGeom(B, Ci, 1, T, Co, 1, T, 1, 1, 1, 1, 0, 0, Ci)
    if ops._wgrad_grouped(g, w_param, b_param):
        ops._queue_wgrad(g, x3, gy3, w_param, b_param)
        return None, None
    dw, dw_ret = _grad_dst(w_param)
    db, db_ret = _grad_dst(b_param)
    nbytes = lib.dynmm_conv2d_wgrad_workspace_bytes(C.byref(g))
    ws = torch.empty(max(nbytes // 4, 1), device=x3.device, dtype=torch.float32)
    L.check(lib.dynmm_conv2d_wgrad(_p(x3), None, _p(gy3), _p(dw), _p(db), _p(ws), nbytes, C.byref(g), _stream()), 'conv2d_wgrad')
    _grads_enqueued()
    return dw_ret, db_ret


class _FFNBlock(Function):
    """LayerNorm(h + dropout2(linear2(dropout(relu(linear1(h)))))): the second half of a post-norm encoder layer.  Forward =
    ffn_kernel + ln_fwd_kernel; backward = LayerNorm backward, ffn_kernel<BWD>, two (queued) weight-gradient problems and one
    ordered sum of the residual branch's gradient with the partial sums of the feed-forward branch's."""

    @staticmethod
    def forward(ctx, h, w1, b1, w2, b2, gamma, beta, eps, drop_f, drop2):
        lib = _lib()
        h = _chk(h, 'x')
        B, D, T = h.shape
        F = w1.shape[0]
        ns = lib.dynmm_ffn_nsplit(B, D, T, F)
        hidden = torch.empty((B, F, T), device=h.device, dtype=torch.float32)
        parts = torch.empty((ns, B, D, T), device=h.device, dtype=torch.float32)
        L.check(lib.dynmm_ffn_fwd(_p(h), _p(w1), _p(b1), _p(w2), _p(hidden), _p(parts), B, D, T, F, ns, _drop_arg(drop_f),
                                  _stream()), 'ffn_fwd')
        y, xsum = torch.empty_like(h), torch.empty_like(h)
        mean, rstd = _ln_stats(h, B, T)
        L.check(lib.dynmm_layernorm_parts_fwd(_p(parts), ns, _p(b2), _p(xsum), _p(h), _p(gamma), _p(beta), _p(y), _p(mean),
                                              _p(rstd), B, D, T, float(eps), _drop_arg(drop2), _stream()), 'layernorm_parts_fwd')
        ctx.drop_f, ctx.drop2, ctx.ns = drop_f, drop2, ns
        ctx.save_for_backward(h, hidden, xsum, mean, rstd, w1, w2, gamma)
        ctx.params = (w1, b1, w2, b2, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib()
        h, hidden, xsum, mean, rstd, w1, w2, gamma = ctx.saved_tensors
        pw1, pb1, pw2, pb2, pgamma, pbeta = ctx.params
        g = _chk(g, 'grad')
        B, D, T = h.shape
        F, ns = w1.shape[0], ctx.ns
        st = _stream()
        # slab ns = the residual branch's gradient, slabs 0 .. ns-1 = the feed-forward branch's partial sums
        slabs = torch.empty((ns + 1, B, D, T), device=h.device, dtype=torch.float32)
        dx, dres, dout = _ln_grad_bufs(h, True, True, ctx.drop2, dres=slabs[ns])
        dg = dg_ret = db = db_ret = None
        if ctx.needs_input_grad[5]:
            dg, dg_ret = _grad_dst(pgamma)
            db, db_ret = _grad_dst(pbeta)
        ws, nb = _ln_ws(lib, g, B, D, T, dg is not None)
        L.check(lib.dynmm_layernorm_drop_bwd_ws(_p(g), _p(xsum), _p(h), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dres), _p(dg),
                                                _p(db), B, D, T, _drop_arg(ctx.drop2), _p(ws), nb, st), 'layernorm_bwd')
        _grads_enqueued()
        dhid = torch.empty_like(hidden)
        pf = ctx.drop_f.p if ctx.drop_f is not None else 0.0
        L.check(lib.dynmm_ffn_bwd_data(_p(dout), _p(hidden), _p(w1), _p(w2), _p(dhid), _p(slabs), B, D, T, F, ns, float(pf), st),
                'ffn_bwd_data')
        # (a layer's weight and bias gradients come out of one weight-gradient problem: either of the pair asks for it)
        dw1 = db1 = dw2 = db2 = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            dw2, db2 = _wgrad_1x1(hidden, dout, pw2, pb2)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw1, db1 = _wgrad_1x1(h, dhid, pw1, pb1)
        dw1, db1, dw2, db2 = (t if need else None for t, need in zip((dw1, db1, dw2, db2), ctx.needs_input_grad[1:5]))
        dh = None
        if ctx.needs_input_grad[0]:
            dh = torch.empty_like(h)
            L.check(lib.dynmm_reduce_slabs(_p(slabs), _p(dh), h.numel(), ns + 1, st), 'reduce_slabs')
        return dh, dw1, db1, dw2, db2, dg_ret, db_ret, None, None, None


def ffn_block(h, layer, drop_f, drop2):
    """norm2(h + dropout2(linear2(dropout(relu(linear1(h)))))) of an nn.TransformerEncoderLayer; drop_* = (p, site, name)."""
    B, D, T = h.shape
    F = layer.linear1.weight.shape[0]
    df, d2 = _make_drop(drop_f, (B, F, T), h.device), _make_drop(drop2, h.shape, h.device)
    return _FFNBlock.apply(h, layer.linear1.weight, layer.linear1.bias, layer.linear2.weight, layer.linear2.bias,
                           layer.norm2.weight, layer.norm2.bias, layer.norm2.eps, df, d2)


# ---------------------------------------------------------------------------------------------------------------
# GRU (MultiBench unimodals.common_models.GRU: torch.nn.GRU, one layer, one direction, h0 = 0), csrc/gru.hip
# ---------------------------------------------------------------------------------------------------------------
GRU_ARMS = {None: 0, 0: 0, 'auto': 0, 1: 1, 'resident': 1, 2: 2, 'stepped': 2}
GRU_ARM_NAMES = {1: 'resident', 2: 'stepped'}


def gru_arm(B, H, T):
    """the dispatch arm ('resident' | 'stepped') the library picks for this shape"""
    return GRU_ARM_NAMES[_lib().dynmm_gru_arm(int(B), int(H), int(T))]


def gru_lengths(lengths, device):
    """lengths (device tensor, host tensor or list) as the device int32 [B] the kernels read.  Host lengths are uploaded per
    call; while the stream is capturing that would freeze them into the capture, so they are refused."""
    if lengths is None:
        return None
    if torch.is_tensor(lengths) and lengths.is_cuda:
        return lengths if lengths.dtype == torch.int32 and lengths.is_contiguous() else lengths.to(torch.int32).contiguous()
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise ValueError('GRU: host lengths under a stream capture would be frozen into it; pass them as a device tensor')
    return torch.as_tensor(lengths, dtype=torch.int32).to(device)


class _GRUCore(Function):
    """The recurrence over gi [T, 3H, B] (time = the convolution's batch axis): (h_n [H, B], states [T, H, B])."""

    @staticmethod
    def forward(ctx, gi, w_hh, b_hh, lengths, arm):
        lib = _lib()
        gi, w, b = _chk(gi, 'gi'), _chk(w_hh.detach(), 'weight_hh'), _chk(b_hh.detach(), 'bias_hh')
        T, H3, B = gi.shape
        H = H3 // 3
        if tuple(w.shape) != (3 * H, H) or tuple(b.shape) != (3 * H,) or H3 != 3 * H:
            raise L.DynmmHipError(f'gru: gi {tuple(gi.shape)}, weight_hh {tuple(w.shape)}, bias_hh {tuple(b.shape)} do not agree')
        if lengths is not None and (lengths.dtype != torch.int32 or not lengths.is_cuda or lengths.numel() != B):
            raise L.DynmmHipError(f'gru: lengths must be {B} int32 values on the device')
        f32 = dict(device=gi.device, dtype=torch.float32)
        st = _stream()
        packed = torch.empty(lib.dynmm_gru_packed_floats(H), **f32)
        L.check(lib.dynmm_gru_pack(_p(w), _p(packed), H, st), 'gru_pack')
        hbuf = torch.empty((T + 1, H, B), **f32)
        gates = torch.empty((T, 4 * H, B), **f32)
        hn = torch.empty((H, B), **f32)
        L.check(lib.dynmm_gru_seq_fwd(_p(gi), _p(packed), _p(b), _p(lengths), _p(hbuf), _p(gates), _p(hn), T, B, H, arm, st),
                'gru_seq_fwd')
        ctx.save_for_backward(packed, hbuf, gates)
        ctx.lengths, ctx.arm, ctx.params = lengths, arm, (w_hh, b_hh)
        ctx.set_materialize_grads(False)
        return hn, hbuf[1:]

    @staticmethod
    def backward(ctx, d_hn, d_hseq):
        lib = _lib()
        packed, hbuf, gates = ctx.saved_tensors
        T, H, B = hbuf.shape[0] - 1, hbuf.shape[1], hbuf.shape[2]
        if d_hn is None and d_hseq is None:
            return None, None, None, None, None
        d_hn, d_hseq = _chk(d_hn, 'grad'), _chk(d_hseq, 'grad')
        f32 = dict(device=hbuf.device, dtype=torch.float32)
        dgi, dgh = torch.empty((T, 3 * H, B), **f32), torch.empty((T, 3 * H, B), **f32)
        nb = lib.dynmm_gru_bwd_workspace_bytes(B, H)
        ws = torch.empty(nb // 4, **f32)
        L.check(lib.dynmm_gru_seq_bwd(_p(d_hn), _p(d_hseq), _p(packed), _p(ctx.lengths), _p(hbuf), _p(gates), _p(dgi), _p(dgh),
                                      _p(ws), nb, T, B, H, ctx.arm, _stream()), 'gru_seq_bwd')
        dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # dW_hh / db_hh: the 1x1-convolution weight gradient of (previous states, dgh), time as the batch axis
            dw, db = _wgrad_1x1(hbuf[:T], dgh, *ctx.params)
        return (dgi if ctx.needs_input_grad[0] else None), (dw if ctx.needs_input_grad[1] else None), \
            (db if ctx.needs_input_grad[2] else None), None, None


def gru_seq(x, w_ih, w_hh, b_ih, b_hh, lengths=None, arm=None):
    """torch.nn.GRU (one layer, one direction, batch_first, h0 = 0) on x [B, T, F]: (h_n [B, H], h_seq [B, T, H] or None).
    lengths (device int32 [B], host tensor or list, each in 1..T): sample b runs lengths[b] steps and h_n is its state at
    t = lengths[b] - 1 (`gru(pack_padded_sequence(x, lengths, enforce_sorted=False))[1][-1]`); no sequence is returned.
    arm: None (the library decides, `gru_arm`) | 'resident' | 'stepped'."""
    if arm not in GRU_ARMS:
        raise ValueError(f'arm must be one of None, "resident", "stepped", got {arm!r}')
    x = _chk(x, 'x')
    if x.dim() != 3:
        raise L.DynmmHipError(f'gru: x must be [B, T, F], got {tuple(x.shape)}')
    lengths = gru_lengths(lengths, x.device)
    gi = linear_bdt(x.permute(1, 2, 0).contiguous(), w_ih, b_ih)         # [T, 3H, B]: every step one contiguous slab
    train_w = torch.is_grad_enabled() and (w_hh.requires_grad or b_hh.requires_grad)
    hn, hseq = _GRUCore.apply(gi, w_hh if train_w else w_hh.detach(), b_hh if train_w else b_hh.detach(), lengths, GRU_ARMS[arm])
    return hn.t().contiguous(), (None if lengths is not None else hseq.permute(2, 0, 1).contiguous())


# ---------------------------------------------------------------------------------------------------------------
# low-rank tensor fusion (MultiBench fusions.common_fusions.LowRankTensorFusion), csrc/lrtf.hip
# ---------------------------------------------------------------------------------------------------------------
class _LRTF(Function):
    """out [B, O] of (fusion_weights [1, R], fusion_bias [1, O], z_0 .. z_{M-1}, F_0 .. F_{M-1}).  Saves its inputs only: the
    backward recomputes every P_m."""

    @staticmethod
    def forward(ctx, w, bias, M, *zf):
        lib = _lib()
        zs, fs = zf[:M], zf[M:]
        B, (R, _, O) = zs[0].shape[0], fs[0].shape
        dims = (C.c_int * M)(*[z.shape[1] for z in zs])
        st = _stream()
        out = torch.empty((B, O), device=zs[0].device, dtype=torch.float32)
        nb = lib.dynmm_lrtf_fwd_workspace_bytes(B, O, R)
        ws = torch.empty(nb // 4, device=out.device, dtype=torch.float32) if nb else None
        L.check(lib.dynmm_lrtf_fwd(_ptr_array(zs), _ptr_array(fs), dims, M, _p(w), _p(bias), _p(out), _p(ws), nb, B, O, R, st),
                'lrtf_fwd')
        ctx.M = M
        ctx.save_for_backward(w, bias, *zf)
        ctx.params = (w, bias) + tuple(fs)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib()
        M = ctx.M
        w, bias = ctx.saved_tensors[:2]
        zs, fs = ctx.saved_tensors[2:2 + M], ctx.saved_tensors[2 + M:]
        g = _chk(g, 'grad')
        B, (R, _, O) = zs[0].shape[0], fs[0].shape
        dims = (C.c_int * M)(*[z.shape[1] for z in zs])
        need = ctx.needs_input_grad
        need_z = [need[3 + m] for m in range(M)]
        need_p = need[0] or need[1] or any(need[3 + M:])
        if not (need_p or any(need_z)):
            return (None,) * (3 + 2 * M)
        dzs = [torch.empty_like(z) if n else None for z, n in zip(zs, need_z)]
        dz_arr = (C.c_void_p * M)(*[_p(t) for t in dzs])
        dw_ret = db_ret = None
        df_ret = [None] * M
        dw = db = df_arr = None
        if need_p:
            # the fused backward produces the parameter gradients together: each lands in its parameter's slice of the flat
            # gradient buffer (or in a fresh tensor under plain autograd)
            pw, pb, pf = ctx.params[0], ctx.params[1], ctx.params[2:]
            dw, dw_ret = _grad_dst(pw)
            db, db_ret = _grad_dst(pb)
            dfs = []
            for m in range(M):
                t, df_ret[m] = _grad_dst(pf[m])
                dfs.append(t)
            df_arr = _ptr_array(dfs)
        nb = lib.dynmm_lrtf_bwd_workspace_bytes(M, dims, B, O, R)
        ws = torch.empty(nb // 4, device=g.device, dtype=torch.float32)
        L.check(lib.dynmm_lrtf_bwd(_p(g), _ptr_array(zs), _ptr_array(fs), dims, M, _p(w), dz_arr, df_arr, _p(dw), _p(db), _p(ws),
                                   nb, B, O, R, _stream()), 'lrtf_bwd')
        _grads_enqueued()
        dw_ret = dw_ret if need[0] else None
        db_ret = db_ret if need[1] else None
        df_ret = [t if n else None for t, n in zip(df_ret, need[3 + M:])]
        return (dw_ret, db_ret, None, *dzs, *df_ret)


def lrtf(zs, factors, fusion_weights, fusion_bias):
    """MultiBench's LowRankTensorFusion on M = 2 or 3 inputs z_m [B, d_m]: with P_m[r] = [1 | z_m] F_m[r] ([B, O]),
    out = sum_r fusion_weights[0, r] prod_m P_m[r] + fusion_bias -> [B, O].  factors[m] [R, d_m + 1, O], fusion_weights [1, R],
    fusion_bias [1, O].  One fused kernel forward, a recomputing backward (csrc/lrtf.hip); no [R, B, O] tensor exists."""
    zs, factors = list(zs), list(factors)
    M = len(zs)
    if M not in (2, 3) or len(factors) != M:
        raise L.DynmmHipError(f'lrtf: M = {M} inputs with {len(factors)} factors: the kernels serve M = 2 or 3 modalities, one '
                              f'factor each')
    zs = [_operand('lrtf', z, f'z[{m}]') for m, z in enumerate(zs)]
    if any(z.dim() != 2 or z.shape[0] != zs[0].shape[0] for z in zs):
        raise L.DynmmHipError(f'lrtf: inputs must be [B, d_m] with one B, got {[tuple(z.shape) for z in zs]}')
    if factors[0].dim() != 3:
        raise L.DynmmHipError(f'lrtf: factors[0] must be [R, d_0 + 1, O], got {tuple(factors[0].shape)}')
    R, O = factors[0].shape[0], factors[0].shape[2]
    factors = [_operand('lrtf', f, f'factors[{m}]', (R, zs[m].shape[1] + 1, O)) for m, f in enumerate(factors)]
    w = _operand('lrtf', fusion_weights, 'fusion_weights', (1, R))
    bias = _operand('lrtf', fusion_bias, 'fusion_bias', (1, O))
    return _LRTF.apply(w, bias, M, *zs, *factors)


def _probs_shape(heads, q, k=None):
    """(B*heads, Tq, Tk): the attention probabilities of q [B, ., Tq] on k [B, ., Tk] (None: on q itself) — the shape of their
    dropout site, whether or not a tensor of them exists"""
    return (q.shape[0] * heads, q.shape[2], (q if k is None else k).shape[2])


def _mha_function(name, fwd, bwd, fwd_label, bwd_label, doc=None):
    """The autograd Function of an attention core: out [B, D, T] of (qkv [B, 3D, T], heads, drop) through the library's entry
    points `fwd` / `bwd`, which share one argument list."""

    def forward(ctx, qkv, heads, drop=None):
        qkv = _chk(qkv, 'qkv')
        B, D3, T = qkv.shape
        D = D3 // 3
        out = torch.empty((B, D, T), device=qkv.device, dtype=torch.float32)
        probs = torch.empty(_probs_shape(heads, qkv), device=qkv.device, dtype=torch.float32)
        L.check(getattr(_lib(), fwd)(_p(qkv), _p(out), _p(probs), B, D, T, heads, _drop_arg(drop), _stream()), fwd_label)
        ctx.drop = drop
        ctx.save_for_backward(qkv, probs)
        ctx.heads = heads
        return out

    def backward(ctx, g):
        qkv, probs = ctx.saved_tensors
        g = _chk(g, 'grad')
        B, D3, T = qkv.shape
        dqkv = torch.empty_like(qkv)
        L.check(getattr(_lib(), bwd)(_p(g), _p(qkv), _p(probs), _p(dqkv), B, D3 // 3, T, ctx.heads, _drop_arg(ctx.drop),
                                     _stream()), bwd_label)
        return dqkv, None, None

    return type(name, (Function,), {'forward': staticmethod(forward), 'backward': staticmethod(backward), '__doc__': doc,
                                    '__module__': __name__})


_MHACore = _mha_function('_MHACore', 'dynmm_mha_drop_fwd', 'dynmm_mha_drop_bwd', 'mha_fwd', 'mha_bwd')
_MHAWide = _mha_function('_MHAWide', 'dynmm_attn_fwd', 'dynmm_attn_bwd', 'attn_fwd', 'attn_bwd',
                         "_MHACore's contract on the matrix-core kernels of csrc/attn.hip (head dimensions up to 64).")

MHA_CORE_MAX_DH = 32     # csrc/seq.hip: kSeqMaxDh


def _probs_drop(qkv, heads, drop):
    """the Drop of the [B*heads, T, T] attention probabilities; drop = (p, site, name) or None"""
    return _make_drop(drop, _probs_shape(heads, qkv), qkv.device)


def mha_core(qkv, heads, drop=None):
    """dropout(softmax(q k^T / sqrt(dh))) v per head for qkv [B, 3D, T] (q | k | v along channels) -> [B, D, T];
    drop = (p, site, name) or None: dropout on the [B*heads, T, T] probabilities."""
    return _MHACore.apply(qkv, heads, _probs_drop(qkv, heads, drop))


def mha_wide(qkv, heads, drop=None):
    """mha_core for head dimensions up to 64 (T <= 64): the same function, arguments and dropout site (name, shape
    (B*heads, T, T), indexing, generator decisions) on 16x16 fp32 matrix-core tiles (csrc/attn.hip)."""
    return _MHAWide.apply(qkv, heads, _probs_drop(qkv, heads, drop))


MHA_MAX_T = 64           # csrc/seq.hip: kSeqMaxT, csrc/attn.hip: kAttnMaxT


def attention(qkv, heads, drop=None):
    """The attention core of an encoder layer.  Up to 64 steps: mha_core up to head dimension 32 (every model with
    d_model <= 160 at nhead = 5: the kernel and the launch they always had), mha_wide above it (Transformer(409, 300): dh = 60).
    Longer sequences: packed_attention_long without a mask (the streaming kernels of csrc/attn_long.hip; the same dropout site)."""
    if qkv.shape[2] > MHA_MAX_T:
        return packed_attention_long(qkv, heads, False, drop)
    dh = qkv.shape[1] // 3 // heads
    return mha_core(qkv, heads, drop) if dh <= MHA_CORE_MAX_DH else mha_wide(qkv, heads, drop)


# ---------------------------------------------------------------------------------------------------------------
# MULT (MultiBench fusions.mult.MULTModel): cross-modal attention and embedding (csrc/xattn.hip), pre-norm plumbing (csrc/seq.hip)
# ---------------------------------------------------------------------------------------------------------------
XATTN_MAX_DH, XATTN_MAX_T = 32, 64       # csrc/xattn.hip: kXaMaxDh, kXaMaxT


def _bdt_view(t, name):
    """t [B, D, T] fp32 on the device whose samples are contiguous [D, T] blocks (a contiguous tensor or a channel slice of
    one: the packed q | k | v of an in_proj); anything else is copied."""
    _chk(t, name)
    if t.dim() != 3:
        raise L.DynmmHipError(f'cross_attention: {name} must be [B, D, T], got {tuple(t.shape)}')
    B, D, T = t.shape
    if t.stride(2) == 1 and t.stride(1) == T and (B == 1 or t.stride(0) >= D * T):
        return t
    return t.contiguous()


def _bstride(t):
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]


# A family of kernels over separate q, k, v: `op` names it in messages, dynmm_<stem>_fwd / _bwd are its entry points (one argument
# list up to what the forward saves), extra(heads, q, k) is the shape of the one tensor the forward writes beside `out`, and
# saves_out says whether the backward reads `out` in front of it.
_QKVFamily = namedtuple('_QKVFamily', 'op stem extra saves_out')
_XATTN = _QKVFamily('cross_attention', 'xattn', _probs_shape, False)                                   # the probabilities
_ATTN_LONG = _QKVFamily('attention_long', 'attn_long', lambda heads, q, k: _probs_shape(heads, q, k)[:2], True)   # out, lse


def _qkv_fwd(fam, q, k, v, heads, causal, drop):
    """(out, what the backward needs beside the inputs) of one forward launch of the family"""
    B, D, Tq = q.shape
    Tk = k.shape[2]
    if tuple(k.shape) != (B, D, Tk) or tuple(v.shape) != (B, D, Tk):
        raise L.DynmmHipError(f'{fam.op}: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} do not agree')
    out = torch.empty((B, D, Tq), device=q.device, dtype=torch.float32)
    extra = torch.empty(fam.extra(heads, q, k), device=q.device, dtype=torch.float32)
    L.check(getattr(_lib(), f'dynmm_{fam.stem}_fwd')(_p(q), _p(k), _p(v), _bstride(q), _bstride(k), _bstride(v), _p(out), _p(extra),
                                                    B, D, Tq, Tk, heads, causal, _drop_arg(drop), _stream()), f'{fam.stem}_fwd')
    return out, ((out, extra) if fam.saves_out else (extra,))


def _qkv_bwd(fam, g, q, k, v, saved, dq, dk, dv, heads, causal, drop):
    B, D, Tq = q.shape
    L.check(getattr(_lib(), f'dynmm_{fam.stem}_bwd')(_p(g), _p(q), _p(k), _p(v), _bstride(q), _bstride(k), _bstride(v),
                                                    *map(_p, saved), _p(dq), _p(dk), _p(dv), _bstride(dq), _bstride(dk),
                                                    _bstride(dv), B, D, Tq, k.shape[2], heads, causal, _drop_arg(drop), _stream()),
            f'{fam.stem}_bwd')


def _thirds(t):
    """the channel thirds q | k | v of a packed [B, 3D, T] (views)"""
    D = t.shape[1] // 3
    return t[:, :D], t[:, D:2 * D], t[:, 2 * D:]


def _qkv_function(name, fam, packed, doc):
    """The autograd Function of a q / k / v family: out [B, D, Tq] of (q, k, v, heads, causal, drop=None), or with `packed` of
    (qkv, heads, causal, drop=None), whose gradient is then one [B, 3D, T] tensor."""
    n = 1 if packed else 3

    def forward(ctx, *args):
        inputs, (heads, causal, drop) = args[:n], (args[n:] + (None,))[:3]
        inputs = (_chk(inputs[0], 'qkv'),) if packed else tuple(_bdt_view(t, c) for t, c in zip(inputs, 'qkv'))
        ctx.drop, ctx.heads, ctx.causal = drop, heads, int(bool(causal))
        out, saved = _qkv_fwd(fam, *(_thirds(inputs[0]) if packed else inputs), heads, ctx.causal, drop)
        ctx.save_for_backward(*inputs, *saved)
        return out

    def backward(ctx, g):
        inputs, saved = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        g = _chk(g, 'grad')
        if packed:
            grads = (torch.empty_like(inputs[0]),)
            inputs, parts = _thirds(inputs[0]), _thirds(grads[0])
        else:
            grads = parts = tuple(torch.empty(t.shape, device=g.device, dtype=torch.float32) for t in inputs)
        _qkv_bwd(fam, g, *inputs, saved, *parts, ctx.heads, ctx.causal, ctx.drop)
        return (*grads, None, None, None)

    return type(name, (Function,), {'forward': staticmethod(forward), 'backward': staticmethod(backward), '__doc__': doc,
                                    '__module__': __name__})


_CrossAttention = _qkv_function(
    '_CrossAttention', _XATTN, False,
    "out [B, D, Tq] of (q [B, D, Tq], k, v [B, D, Tk]); saves its inputs and the probabilities before dropout.")
_PackedAttention = _qkv_function(
    '_PackedAttention', _XATTN, True,
    "_CrossAttention on the channel thirds q | k | v of one qkv [B, 3D, T]; the gradient is one [B, 3D, T] tensor.")


def cross_attention(q, k, v, heads, causal, drop=None):
    """dropout(softmax(q k^T / sqrt(dh) + mask)) v per head for q [B, D, Tq], k and v [B, D, Tk] -> [B, D, Tq].  causal: key j is
    visible to query i iff j <= i + |Tk - Tq| (MULT's future mask, torch.triu(-inf, 1 + |Tk - Tq|)).  q, k, v may be channel
    slices of one packed [B, 3D, T] tensor (no copy; `packed_attention` also returns their gradient as one tensor).
    drop = (p, site, name) or None: dropout on the [B*heads, Tq, Tk] probabilities.  Head dimensions up to 32, lengths up to 64
    (csrc/xattn.hip)."""
    return _CrossAttention.apply(q, k, v, heads, causal, _make_drop(drop, _probs_shape(heads, q, k), q.device))


def packed_attention(qkv, heads, causal, drop=None):
    """cross_attention on qkv [B, 3D, T] (q | k | v along channels, an in_proj's output): masked self-attention."""
    return _PackedAttention.apply(qkv, heads, causal, _probs_drop(qkv, heads, drop))


# ---------------------------------------------------------------------------------------------------------------
# streaming attention for any sequence length (csrc/attn_long.hip): the function and the dropout site of cross_attention, no
# stored probabilities
# ---------------------------------------------------------------------------------------------------------------
_AttentionLong = _qkv_function(
    '_AttentionLong', _ATTN_LONG, False,
    """out [B, D, Tq] of (q [B, D, Tq], k, v [B, D, Tk]); saves its inputs, out and the per-row log-sum-exp [B*heads, Tq] — no
    probabilities: the backward recomputes them.""")
_PackedAttentionLong = _qkv_function(
    '_PackedAttentionLong', _ATTN_LONG, True,
    "_AttentionLong on the channel thirds q | k | v of one qkv [B, 3D, T]; the gradient is one [B, 3D, T] tensor.")


def attention_long(q, k, v, heads, causal, drop=None):
    """cross_attention's function, arguments and dropout site (name, shape (B*heads, Tq, Tk), indexing, generator decisions) at
    any lengths and head dimensions up to 64, by an online softmax over 64-key tiles on the fp32 matrix cores: no
    [B*heads, Tq, Tk] tensor is written in either pass (csrc/attn_long.hip)."""
    return _AttentionLong.apply(q, k, v, heads, causal, _make_drop(drop, _probs_shape(heads, q, k), q.device))


def packed_attention_long(qkv, heads, causal, drop=None):
    """attention_long on qkv [B, 3D, T] (q | k | v along channels, an in_proj's output)."""
    return _PackedAttentionLong.apply(qkv, heads, causal, _probs_drop(qkv, heads, drop))


def _xattn_serves(dh, Tq, Tk):
    """the whole-row kernels of csrc/xattn.hip hold this shape: the path MULT always had"""
    return dh <= XATTN_MAX_DH and Tq <= XATTN_MAX_T and Tk <= XATTN_MAX_T


def masked_attention(q, k, v, heads, causal, drop=None):
    """MULT's cross-modal attention at any lengths: cross_attention where it serves (dh <= 32, both lengths <= 64), attention_long
    beyond."""
    if _xattn_serves(q.shape[1] // heads, q.shape[2], k.shape[2]):
        return cross_attention(q, k, v, heads, causal, drop)
    return attention_long(q, k, v, heads, causal, drop)


def packed_masked_attention(qkv, heads, causal, drop=None):
    """MULT's masked self-attention at any length: packed_attention where it serves, packed_attention_long beyond."""
    if _xattn_serves(qkv.shape[1] // 3 // heads, qkv.shape[2], qkv.shape[2]):
        return packed_attention(qkv, heads, causal, drop)
    return packed_attention_long(qkv, heads, causal, drop)


class _PosEmbed(Function):
    """(y1[, y2]) = dropout_s(scale x + pos) for one or two sites."""

    @staticmethod
    def forward(ctx, x, pos, scale, drop1, drop2, two):
        x = _chk(x, 'x')
        B, E, T = x.shape
        y1 = torch.empty_like(x)
        y2 = torch.empty_like(x) if two else None
        L.check(_lib().dynmm_posembed_fwd(_p(x), _p(pos), _p(y1), _p(y2), B, E, T, float(scale), _drop_arg(drop1),
                                          _drop_arg(drop2), _stream()), 'posembed_fwd')
        ctx.drops, ctx.scale, ctx.two = (drop1, drop2), float(scale), two
        ctx.set_materialize_grads(False)
        return (y1, y2) if two else y1

    @staticmethod
    def backward(ctx, g1, g2=None):
        d1, d2 = ctx.drops
        if g1 is None:
            g1, g2, d1, d2 = g2, None, d2, None
        if g1 is None:
            return None, None, None, None, None, None
        g1, g2 = _chk(g1, 'grad'), _chk(g2, 'grad')
        B, E, T = g1.shape
        dx = torch.empty_like(g1)
        L.check(_lib().dynmm_posembed_bwd(_p(g1), _p(g2), _p(dx), B, E, T, ctx.scale, _drop_arg(d1),
                                          _drop_arg(d2) if g2 is not None else None, _stream()), 'posembed_bwd')
        return dx, None, None, None, None, None


def pos_embed(x, pos, scale, drop=None, drop2=None):
    """MULT's embedding of x [B, E, T]: dropout(scale x + pos), pos [E, T] the sinusoid table of positions 1..T, left out at the
    time steps whose x[b, 0, t] is exactly 0 (padding).  drop / drop2 = (p, site, name): with drop2 the launch returns two outputs
    with dropout decisions of their own (the key and the value embedding of one source)."""
    pos = _operand('pos_embed', pos, 'pos', (x.shape[1], x.shape[2]))
    return _PosEmbed.apply(x, pos, scale, _make_drop(drop, x.shape, x.device), _make_drop(drop2, x.shape, x.device),
                           drop2 is not None)


class _PreNorm(Function):
    """(sum, y) = (res + dropout(x), LayerNorm(sum)); x None: y alone (sum = res).  direct: the parameter gradients may take the
    in-place gradient protocol (the LayerNorm is applied ONCE per step; a LayerNorm shared by several inputs returns its
    gradients to autograd, which sums them)."""

    @staticmethod
    def forward(ctx, res, x, gamma, beta, eps, drop, direct):
        lib = _lib()
        res, x, gamma, beta = _chk(res, 'res'), _chk(x, 'x'), _chk(gamma, 'gamma'), _chk(beta, 'beta')
        B, D, T = res.shape
        y = torch.empty_like(res)
        s = torch.empty_like(res) if x is not None else None
        mean, rstd = _ln_stats(res, B, T)
        L.check(lib.dynmm_prenorm_fwd(_p(x), _p(res), _p(gamma), _p(beta), _p(s), _p(y), _p(mean), _p(rstd), B, D, T, float(eps),
                                      _drop_arg(drop), _stream()), 'prenorm_fwd')
        ctx.drop, ctx.direct, ctx.has_x = drop, direct, x is not None
        ctx.save_for_backward(s if x is not None else res, gamma, mean, rstd)
        ctx.g_param, ctx.b_param = gamma, beta
        ctx.set_materialize_grads(False)
        return (s, y) if x is not None else y

    @staticmethod
    def backward(ctx, *grads):
        lib = _lib()
        s, gamma, mean, rstd = ctx.saved_tensors
        gs, gy = grads if ctx.has_x else (None, grads[0])
        B, D, T = s.shape
        if gy is None:
            if gs is None:
                return (None,) * 7
            gy = torch.zeros_like(s)               # only the sum was used downstream (no model of this project does that)
        gy, gs = _chk(gy, 'grad'), _chk(gs, 'grad')
        need_res, need_x = ctx.needs_input_grad[0], ctx.has_x and ctx.needs_input_grad[1]
        dx, dres, gx = _ln_grad_bufs(s, need_x, need_res, ctx.drop)
        dg = dg_ret = db = db_ret = None
        acc = 0
        if ctx.needs_input_grad[2]:
            if ctx.direct or (ops._direct_ok(ctx.g_param) and ops._direct_ok(ctx.b_param)):
                # in place: a LayerNorm applied once per step overwrites its gradient, a shared one ADDS to it (.grad's own
                # meaning; the step's gradient buffer starts at zero) — no accumulation pass by autograd
                dg, dg_ret = _grad_dst(ctx.g_param)
                db, db_ret = _grad_dst(ctx.b_param)
                acc = int(not ctx.direct and dg_ret is None and db_ret is None)
            else:
                dg = dg_ret = torch.empty_like(gamma)
                db = db_ret = torch.empty_like(gamma)
        ws, nb = _ln_ws(lib, s, B, D, T, dg is not None)
        L.check(lib.dynmm_prenorm_bwd(_p(gy), _p(gs), _p(s), _p(gamma), _p(mean), _p(rstd), _p(dx), _p(dres), _p(dg), _p(db), B,
                                      D, T, _drop_arg(ctx.drop), acc, _p(ws), nb, _stream()), 'prenorm_bwd')
        _grads_enqueued()
        return (dres if need_res else None), gx, dg_ret, db_ret, None, None, None


def prenorm_bdt(res, gamma, beta, eps=1e-5, x=None, drop=None, shared=False):
    """The plumbing of a pre-norm layer, one launch: with x, (res + dropout(x), LayerNorm of that sum) — both are returned, the sum
    is the next residual input and the normalisation feeds the next block; without x, LayerNorm(res) alone.  drop = (p, site,
    name) or None.  shared: this LayerNorm's parameters are applied to several inputs in one step (MULT's LN0 on query, key and
    value): inside a training step their gradients are ADDED to the parameter's gradient in place instead of overwriting it,
    otherwise they go back to autograd, which sums them."""
    d = _make_drop(drop, x.shape, x.device) if x is not None else None
    return _PreNorm.apply(res, x, gamma, beta, eps, d, not shared)


class _ResidualAdd(Function):
    """res + x, [B, D, ...] (csrc/seq.hip's LayerNorm forward without gamma: it returns after storing the sum)."""

    @staticmethod
    def forward(ctx, res, x):
        res, x = _chk(res, 'res'), _chk(x, 'x')
        B, D = res.shape[0], res.shape[1]
        s = torch.empty_like(res)
        L.check(_lib().dynmm_prenorm_fwd(_p(x), _p(res), None, None, _p(s), None, None, None, B, D, res.numel() // (B * D), 0.0,
                                         None, _stream()), 'prenorm_fwd')
        return s

    @staticmethod
    def backward(ctx, g):
        return g, g


def residual_add(res, x):
    """res + x as a HIP launch (the head of MULT: proj2(...) + z)."""
    return _ResidualAdd.apply(res, x)


class _MoEBlend(Function):
    """out[B,1] = sum_k w_k pred_k, w = DiffSoftmax(logits/temp, hard); aux = mean w[:, K-1]  (affect_dyn.py:152-165)."""

    @staticmethod
    def forward(ctx, logits, temp, hard, *preds):
        lib = _lib()
        logits = _chk(logits, 'logits')
        preds = [_chk(p.reshape(-1), 'pred') for p in preds]
        B, K = logits.shape
        f32 = dict(device=logits.device, dtype=torch.float32)
        out, weight, scal = torch.empty(B, **f32), torch.empty((B, K), **f32), torch.empty(3, **f32)
        L.check(lib.dynmm_moe_head(_p(logits), _ptr_array(preds), K, None, float(temp), int(bool(hard)), 0.0, _p(out),
                                   _p(weight), _p(scal), None, None, B, _stream()), 'moe_head')
        ctx.save_for_backward(logits, weight, *preds)
        ctx.temp = float(temp)
        ctx.mark_non_differentiable(weight)
        return out.reshape(B, 1), scal[1], weight

    @staticmethod
    def backward(ctx, d_out, d_aux, _dw):
        lib = _lib()
        logits, weight = ctx.saved_tensors[:2]
        preds = list(ctx.saved_tensors[2:])
        B, K = logits.shape
        f32 = dict(device=logits.device, dtype=torch.float32)
        d_out = None if d_out is None else _chk(d_out.reshape(-1), 'd_out')
        d_aux = None if d_aux is None else _chk(d_aux.reshape(1), 'd_aux')
        dps = [torch.empty(B, **f32) for _ in preds]
        dl = torch.empty((B, K), **f32)
        L.check(lib.dynmm_moe_blend_bwd(_p(d_out), _p(d_aux), _p(logits), _ptr_array(preds), K, _p(weight), ctx.temp,
                                        _ptr_array(dps), _p(dl), B, _stream()), 'moe_blend_bwd')
        return (dl, None, None, *[d.reshape(B, 1) for d in dps])


def moe_blend(logits, preds, temp=1.0, hard=False):
    """(out [B,1], aux scalar, weight [B,K]) — the gated mixture of the experts' predictions."""
    return _MoEBlend.apply(logits, temp, hard, *preds)


def _seed_backward(logits, preds, dps, dl):
    """The tail of a mixture's fused loss: start the backward pass from the kernel's seeds, dps[k] for every prediction that
    requires grad (None for the others) and dl for the logits."""
    roots = [p for p, d in zip(preds, dps) if d is not None]
    grads = [d.reshape(p.shape) for p, d in zip(preds, dps) if d is not None]
    if logits.requires_grad:
        roots.append(logits)
        grads.append(dl)
    if roots:
        torch.autograd.backward(roots, grads)


def moe_loss_backward(logits, preds, target, temp, hard, reg):
    """Supervised_Learning.py:120-141 for a DynMM mixture, on the device: blend, L1 loss, loss1 + reg * aux, and the
    backward pass seeded straight from the kernel (no PyTorch arithmetic kernels).  Returns
    {'out': [B,1], 'weight': [B,K], 'loss1', 'aux', 'total'}."""
    lib = _lib()
    logits = _chk(logits, 'logits')
    flat = [_chk(p.reshape(-1), 'pred') for p in preds]
    tgt = _chk(target.reshape(-1).float(), 'target')
    B, K = logits.shape
    f32 = dict(device=logits.device, dtype=torch.float32)
    out, weight, scal = torch.empty(B, **f32), torch.empty((B, K), **f32), torch.empty(3, **f32)
    dps = [torch.empty(B, **f32) if p.requires_grad else None for p in preds]
    dl = torch.empty((B, K), **f32)
    arr = (C.c_void_p * K)(*[(None if d is None else d.data_ptr()) for d in dps])
    L.check(lib.dynmm_moe_head(_p(logits.detach()), _ptr_array(flat), K, _p(tgt), float(temp), int(bool(hard)), float(reg),
                               _p(out), _p(weight), _p(scal), arr, _p(dl), B, _stream()), 'moe_head')
    _seed_backward(logits, preds, dps, dl)
    return {'out': out.reshape(B, 1), 'weight': weight, 'loss1': scal[0:1], 'aux': scal[1:2], 'total': scal[2:3]}


def clip_grad_norm(flat_grad, max_norm):
    """(norm, coef) device tensor [2]: coef = min(1, max_norm / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_."""
    lib = _lib()
    ws = torch.empty(lib.dynmm_clip_grad_norm_workspace_bytes() // 8, device=flat_grad.device, dtype=torch.float64)
    out = torch.empty(2, device=flat_grad.device, dtype=torch.float32)
    L.check(lib.dynmm_clip_grad_norm(_p(flat_grad), C.c_size_t(flat_grad.numel()), float(max_norm), ws.data_ptr(), _p(out),
                                     _stream()), 'clip_grad_norm')
    return out


# ---------------------------------------------------------------------------------------------------------------
# evaluation: Supervised_Learning.single_test, task "posneg-classification" — 2x2 counts and the loss accumulator on the
# device, Accuracy / Loss / Corr on the host from one read
# ---------------------------------------------------------------------------------------------------------------
class PosnegCounts:
    """The reference's posneg evaluation of one pass, accumulated on the device (one launch per batch, no host sync).

    form 'test' (single_test with criterion L1Loss(reduction='sum'), affect_dyn.py:228,233): each batch adds
    len(batch) * sum|out - y| — the reference multiplies the SUM by the batch size once more, so its reported Loss is
    sum_batches B_i * sum_i|out - y| / N, not the mean absolute error.  The quirk is kept: the numbers match the reference's.
    form 'valid' (train's validation, Supervised_Learning.py:160-185, objective L1Loss()): each batch adds
    (mean|out - y| + lossw * aux) * len(batch), aux = the gate regulariser the model returned with the batch."""

    FORMS = {'test': 0, 'valid': 1}

    def __init__(self, device, form='test', lossw=0.0):
        if form not in self.FORMS:
            raise ValueError(f'form must be one of {sorted(self.FORMS)}, got {form!r}')
        self.form, self.lossw = form, float(lossw)
        self.counts = torch.zeros(4, device=device, dtype=torch.int64)
        self.loss_acc = torch.zeros(1, device=device, dtype=torch.float64)
        self.n = 0

    def add(self, out, target, aux=None):
        out = _chk(out.detach(), 'out')
        tgt = _chk(target.detach().float(), 'target')
        B = out.shape[0]
        if out.dim() not in (1, 2) or out.numel() == 0 or tgt.numel() != B:
            raise L.DynmmHipError(f'posneg counts: out must be [B] or [B, C] and target hold B values, got out '
                                  f'{tuple(out.shape)}, target {tuple(tgt.shape)}')
        stride = 1 if out.dim() == 1 else out.shape[1]
        a = None
        if self.form == 'valid' and torch.is_tensor(aux):
            a = _chk(aux.detach().reshape(1).float(), 'aux')
        L.check(_lib().dynmm_posneg_counts(_p(out), stride, _p(tgt), B, _p(a), self.lossw, self.FORMS[self.form],
                                           self.counts.data_ptr(), self.loss_acc.data_ptr(), _stream()), 'posneg_counts')
        self.n += B

    def read(self):
        """{'counts': int64 numpy [n00, n01, n10, n11] (index 2 * (out >= 0) + (y >= 0)), 'loss_acc', 'n'} — the one
        device -> host transfer of a pass."""
        host = torch.cat([self.counts.double(), self.loss_acc]).cpu().numpy()
        return {'counts': host[:4].astype('int64'), 'loss_acc': float(host[4]), 'n': self.n}

    def metrics(self):
        r = self.read()
        return posneg_metrics(r['counts'], r['loss_acc'], r['n'])


def posneg_metrics(counts, loss_acc, n):
    """single_test's posneg summary from the 2x2 counts [n00, n01, n10, n11] (index 2 * pred + truth):
    {'Accuracy': (n11 + n00) / N, 'Loss': loss_acc / N, 'Corr': pearsonr(truth, pred)}.  The Pearson correlation of two 0/1
    vectors is the phi coefficient of their 2x2 table; NaN when a marginal is zero (a constant vector), as scipy gives."""
    n00, n01, n10, n11 = (int(v) for v in counts)
    N = n00 + n01 + n10 + n11
    if N != int(n):
        raise ValueError(f'the counts hold {N} samples, expected {n}')
    if N == 0:
        return {'Accuracy': float('nan'), 'Loss': float('nan'), 'Corr': float('nan')}
    den = (n10 + n11) * (n00 + n01) * (n01 + n11) * (n00 + n10)       # pred = 1, pred = 0, truth = 1, truth = 0
    corr = (n11 * n00 - n10 * n01) / den ** 0.5 if den > 0 else float('nan')
    return {'Accuracy': (n11 + n00) / N, 'Loss': float(loss_acc) / N, 'Corr': float(corr)}

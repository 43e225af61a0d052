"""autograd shells for the modality-level DynMM on MM-IMDB features (ModalityDynMM/multimedia/imdb_dyn.py).

Activations are [B, D] fp32 rows; every Linear is `ops_seq.linear_bdt` (the 1x1 MFMA convolution).  The kernels added for
this path live in csrc/mlp.hip: MultiBench's Maxout -> BatchNorm1d -> Dropout fused (and the plain BatchNorm1d of a
MaxOut_MLP's input), the multilabel mixture head, the evaluation counts and the hard-gate partition.  The multiplicative
interactions fusion of imdb_mm.py `--fuse 3` (`mim`) runs on csrc/mim.hip.  As everywhere in dynmm_amd there is no CPU / eager
fallback.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd import Function

from . import lib as L
from . import ops_seq as S
from .ops import _chk, _grad_dst, _grads_enqueued, _lib, _operand, _p, _ptr_array, _stream


def _bn_stats_ptrs(bn):
    if not bn.track_running_stats or bn.running_mean is None:
        return None, None, None
    for t in (bn.running_mean, bn.running_var):
        _chk(t, 'running stats')
    return bn.running_mean, bn.running_var, bn.num_batches_tracked


class _MaxoutBN(Function):
    @staticmethod
    def forward(ctx, z, gamma, beta, bn, maxout, drop):
        lib = _lib()
        z = _chk(z, 'z')
        B = z.shape[0]
        M = z.shape[1] // 2 if maxout else z.shape[1]
        train = bn.training or not bn.track_running_stats
        if train and B < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {tuple(z.shape)}')
        if bn.momentum is None:
            raise L.DynmmHipError('BatchNorm1d(momentum=None) (cumulative moving average) is not supported')
        rm, rv, nbt = _bn_stats_ptrs(bn)
        if not train and rm is None:
            raise L.DynmmHipError('BatchNorm1d in eval mode needs running statistics')
        if nbt is not None and not (nbt.is_cuda and nbt.dtype == torch.int64):
            raise L.DynmmHipError('num_batches_tracked must be an int64 device tensor')
        f32 = dict(device=z.device, dtype=torch.float32)
        y = torch.empty((B, M), **f32)
        mean, rstd = torch.empty(M, **f32), torch.empty(M, **f32)
        update = train and bn.training
        L.check(lib.dynmm_maxout_bn_fwd(_p(z), _p(y), _p(mean), _p(rstd), _p(rm) if update or not train else None,
                                        _p(rv) if update or not train else None, _p(nbt) if update else None,
                                        _p(_chk(gamma, 'gamma')), _p(_chk(beta, 'beta')), B, M, int(bool(maxout)),
                                        float(bn.eps), float(bn.momentum), int(train), S._drop_arg(drop), _stream()),
                'maxout_bn_fwd')
        ctx.save_for_backward(z, mean, rstd, gamma)
        ctx.params = (gamma, beta)
        ctx.maxout, ctx.train, ctx.drop = bool(maxout), bool(train), drop
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib()
        z, mean, rstd, gamma = ctx.saved_tensors
        g = _chk(g, 'grad')
        B = z.shape[0]
        M = mean.shape[0]
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        dg = dg_ret = db = db_ret = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dg, dg_ret = _grad_dst(ctx.params[0])
            db, db_ret = _grad_dst(ctx.params[1])
        L.check(lib.dynmm_maxout_bn_bwd(_p(g), _p(z), _p(mean), _p(rstd), _p(gamma), _p(dz), _p(dg), _p(db), B, M,
                                        int(ctx.maxout), int(ctx.train), S._drop_arg(ctx.drop), _stream()), 'maxout_bn_bwd')
        _grads_enqueued()
        return dz, dg_ret, db_ret, None, None, None


def maxout_bn(z, bn, drop=None, maxout=True):
    """Dropout(BatchNorm1d(Maxout(z))) with z = the Maxout's GEMM output [B, 2m] (output j = max of columns 2j, 2j + 1), as
    MultiBench's MaxOut_MLP applies op1 -> op2 / op3 -> op4; maxout=False: BatchNorm1d(z) alone (op0).  bn: the nn.BatchNorm1d
    (its mode, eps, momentum, affine parameters and running statistics); drop = (p, site, name) or None."""
    B = z.shape[0]
    M = z.shape[1] // 2 if maxout else z.shape[1]
    d = None
    if drop is not None and drop[0] > 0 and (bn.training or not bn.track_running_stats):
        d = S.Drop(drop[0], drop[1], drop[2], (B, M), z.device)
    return _MaxoutBN.apply(z, bn.weight, bn.bias, bn, bool(maxout), d)


# ---------------------------------------------------------------------------------------------------------------
# multiplicative interactions fusion (MultiBench fusions.common_fusions.MultiplicativeInteractions2Modal), csrc/mim.hip
# ---------------------------------------------------------------------------------------------------------------
class _MIM(Function):
    """out [B, D] of (m1, m2, W, U, V, b).  Saves its inputs only."""

    @staticmethod
    def forward(ctx, m1, m2, W, U, V, b):
        lib = _lib()
        (B, N), (M, D) = m1.shape, V.shape
        out = torch.empty((B, D), device=m1.device, dtype=torch.float32)
        nb = lib.dynmm_mim_fwd_workspace_bytes(B, N, M, D)
        ws = torch.empty(nb // 4, device=out.device, dtype=torch.float32)
        L.check(lib.dynmm_mim_fwd(_p(m1), _p(m2), _p(W), _p(U), _p(V), _p(b), _p(out), _p(ws), nb, B, N, M, D, _stream()),
                'mim_fwd')
        ctx.save_for_backward(m1, m2, W, U, V)
        ctx.params = (W, U, V, b)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib()
        m1, m2, W, U, V = ctx.saved_tensors
        g = _chk(g, 'grad')
        (B, N), (M, D) = m1.shape, V.shape
        need = ctx.needs_input_grad
        need_p = any(need[2:])
        if not (need_p or need[0] or need[1]):
            return (None,) * 6
        dm1 = torch.empty_like(m1) if need[0] else None
        dm2 = torch.empty_like(m2) if need[1] else None
        dst = [None] * 4
        ret = [None] * 4
        if need_p:
            # the weight pass produces the four parameter gradients together: each lands in its parameter's slice of the flat
            # gradient buffer (or in a fresh tensor under plain autograd)
            for k, prm in enumerate(ctx.params):
                dst[k], ret[k] = _grad_dst(prm)
        nb, ws = 0, None
        if need[0] or need[1]:
            nb = lib.dynmm_mim_bwd_workspace_bytes(B, N, M, D)
            ws = torch.empty(nb // 4, device=g.device, dtype=torch.float32)
        L.check(lib.dynmm_mim_bwd(_p(g), _p(m1), _p(m2), _p(W), _p(U), _p(V), _p(dm1), _p(dm2), _p(dst[0]), _p(dst[1]),
                                  _p(dst[2]), _p(dst[3]), _p(ws), nb, B, N, M, D, _stream()), 'mim_bwd')
        _grads_enqueued()
        ret = [t if n else None for t, n in zip(ret, need[2:])]
        return (dm1, dm2, *ret)


def mim(m1, m2, W, U, V, b):
    """MultiBench's MultiplicativeInteractions2Modal(output='matrix') on m1 [B, n], m2 [B, m]:
    out = einsum('bm,bmd->bd', m2, einsum('bn,nmd->bmd', m1, W) + V) + m1 @ U + b -> [B, D], with W [n, m, D], U [n, D],
    V [m, D], b [D].  One operator forward and backward (csrc/mim.hip); no [B, m, D] tensor exists."""
    m1, m2 = _operand('mim', m1, 'm1'), _operand('mim', m2, 'm2')
    if m1.dim() != 2 or m2.dim() != 2 or m1.shape[0] != m2.shape[0]:
        raise L.DynmmHipError(f'mim: m1 [B, n] and m2 [B, m] must share B, got {tuple(m1.shape)} and {tuple(m2.shape)}')
    if not torch.is_tensor(W) or W.dim() != 3:
        raise L.DynmmHipError(f'mim: W must be [n, m, D], got {tuple(W.shape) if torch.is_tensor(W) else type(W).__name__}')
    n, m, D = m1.shape[1], m2.shape[1], W.shape[2]
    W = _operand('mim', W, 'W', (n, m, D))
    U, V, b = _operand('mim', U, 'U', (n, D)), _operand('mim', V, 'V', (m, D)), _operand('mim', b, 'b', (D,))
    if 0 in (m1.shape[0], n, m, D):
        raise L.DynmmHipError(f'mim: empty operands (B, n, m, D) = {(m1.shape[0], n, m, D)}')
    return _MIM.apply(m1, m2, W, U, V, b)


# ---------------------------------------------------------------------------------------------------------------
# multilabel mixture head
# ---------------------------------------------------------------------------------------------------------------
def _flat_preds(preds):
    out = []
    for p in preds:
        p = _chk(p, 'pred')
        if p.dim() != 2:
            raise L.DynmmHipError(f'expert predictions must be [B, C], got {tuple(p.shape)}')
        out.append(p)
    return out


class _MlBlend(Function):
    """out[B,C] = sum_k w_k pred_k, w = DiffSoftmax(logits/temp, hard); aux = mean w[:, K-1]  (imdb_dyn.py:95-104)."""

    @staticmethod
    def forward(ctx, logits, temp, hard, *preds):
        lib = _lib()
        logits = _chk(logits, 'logits')
        preds = _flat_preds(preds)
        B, K = logits.shape
        Cc = preds[0].shape[1]
        f32 = dict(device=logits.device, dtype=torch.float32)
        out, weight, scal = torch.empty((B, Cc), **f32), torch.empty((B, K), **f32), torch.empty(3, **f32)
        L.check(lib.dynmm_ml_head(_p(logits), _ptr_array(preds), K, Cc, None, float(temp), int(bool(hard)), 0.0, _p(out),
                                  _p(weight), _p(scal), None, None, B, _stream()), 'ml_head')
        ctx.save_for_backward(logits, weight, *preds)
        ctx.temp = float(temp)
        ctx.mark_non_differentiable(weight)
        return out, scal[1], weight

    @staticmethod
    def backward(ctx, d_out, d_aux, _dw):
        lib = _lib()
        logits, weight = ctx.saved_tensors[:2]
        preds = list(ctx.saved_tensors[2:])
        B, K = logits.shape
        Cc = preds[0].shape[1]
        d_out = None if d_out is None else _chk(d_out, 'd_out')
        d_aux = None if d_aux is None else _chk(d_aux.reshape(1), 'd_aux')
        dps = [torch.empty_like(p) for p in preds]
        dl = torch.empty_like(logits)
        L.check(lib.dynmm_ml_blend_bwd(_p(d_out), _p(d_aux), _p(logits), _ptr_array(preds), K, Cc, _p(weight), ctx.temp,
                                       _ptr_array(dps), _p(dl), B, _stream()), 'ml_blend_bwd')
        return (dl, None, None, *dps)


def ml_blend(logits, preds, temp=1.0, hard=False):
    """(out [B,C], aux scalar, weight [B,K]): the gated mixture of the experts' [B, C] logits."""
    return _MlBlend.apply(logits, temp, hard, *preds)


def gate_weight(logits, temp=1.0, hard=False):
    """(weight [B,K], aux [1]) of DiffSoftmax(logits / temp, hard) alone (no gradient)."""
    lib = _lib()
    logits = _chk(logits.detach(), 'logits')
    B, K = logits.shape
    f32 = dict(device=logits.device, dtype=torch.float32)
    weight, scal = torch.empty((B, K), **f32), torch.empty(3, **f32)
    L.check(lib.dynmm_ml_head(_p(logits), None, K, 1, None, float(temp), int(bool(hard)), 0.0, None, _p(weight), _p(scal),
                              None, None, B, _stream()), 'ml_head')
    return weight, scal[1:2]


def ml_loss_backward(logits, preds, target, temp, hard, reg):
    """Supervised_Learning.train for a multilabel DynMM mixture, on the device: blend, BCEWithLogitsLoss, loss + reg * aux, and
    the backward pass seeded straight from the kernel.  Experts whose prediction does not require grad get no seed (and so
    no backward).  Returns {'out': [B,C], 'weight': [B,K], 'loss1', 'aux', 'total'} (device tensors [1])."""
    lib = _lib()
    logits = _chk(logits, 'logits')
    flat = _flat_preds(preds)
    tgt = _chk(target.float(), 'target')
    B, K = logits.shape
    Cc = flat[0].shape[1]
    if tuple(tgt.shape) != (B, Cc):
        raise L.DynmmHipError(f'target must be [{B}, {Cc}], got {tuple(tgt.shape)}')
    f32 = dict(device=logits.device, dtype=torch.float32)
    out, weight, scal = torch.empty((B, Cc), **f32), torch.empty((B, K), **f32), torch.empty(3, **f32)
    dps = [torch.empty((B, Cc), **f32) if p.requires_grad else None for p in preds]
    dl = torch.empty((B, K), **f32)
    arr = (C.c_void_p * K)(*[(None if d is None else d.data_ptr()) for d in dps])
    L.check(lib.dynmm_ml_head(_p(logits.detach()), _ptr_array([f.detach() for f in flat]), K, Cc, _p(tgt), float(temp),
                              int(bool(hard)), float(reg), _p(out), _p(weight), _p(scal), arr, _p(dl), B, _stream()),
            'ml_head')
    S._seed_backward(logits, preds, dps, dl)
    return {'out': out, 'weight': weight, 'loss1': scal[0:1], 'aux': scal[1:2], 'total': scal[2:3]}


# ---------------------------------------------------------------------------------------------------------------
# single-expert objective (Step I: one model, no gate)
# ---------------------------------------------------------------------------------------------------------------
HEAD_LOSSES = {'bce': L.LOSS_BCE_LOGITS, 'l1': L.LOSS_L1}


def head_loss(out, target, kind, seed=True, loss_acc=None):
    """(loss [1], d_out [B,C] or None): BCEWithLogitsLoss() ('bce') or L1Loss() ('l1') of out [B,C] (or [B]) against target of
    the same number of elements, the mean over all of them, and the backward seed dloss/dout — one launch
    (csrc/expert_loss.hip).  loss_acc: optional fp64 device [1] that receives += loss * B (an epoch's training loss)."""
    if kind not in HEAD_LOSSES:
        raise ValueError(f'head_loss: kind must be one of {sorted(HEAD_LOSSES)}, got {kind!r}')
    o = _chk(out.detach(), 'out')
    B = o.shape[0]
    Cc = o.numel() // max(B, 1)
    tgt = _chk(target.detach().float(), 'target')
    if o.dim() not in (1, 2) or o.numel() == 0 or tgt.numel() != o.numel():
        raise L.DynmmHipError(f'head_loss: out must be [B] or [B, C] and target hold as many values, got out {tuple(o.shape)}, '
                              f'target {tuple(tgt.shape)}')
    if loss_acc is not None and not (loss_acc.is_cuda and loss_acc.dtype == torch.float64 and loss_acc.numel() >= 1):
        raise L.DynmmHipError('head_loss: loss_acc must be an fp64 device tensor')
    f32 = dict(device=o.device, dtype=torch.float32)
    loss = torch.empty(1, **f32)
    d_out = torch.empty(o.shape, **f32) if seed else None
    L.check(_lib().dynmm_head_loss(_p(o), _p(tgt), B, Cc, HEAD_LOSSES[kind], _p(loss), _p(d_out),
                                   None if loss_acc is None else loss_acc.data_ptr(), _stream()), 'head_loss')
    return loss, d_out


# ---------------------------------------------------------------------------------------------------------------
# evaluation: per-class counts on the device, F1 on the host from one read
# ---------------------------------------------------------------------------------------------------------------
class MultilabelCounts:
    """TP / FP / FN per class and the BCE sum over evaluation batches, accumulated on the device (one launch per batch);
    read() is the one device -> host transfer of an evaluation pass."""

    def __init__(self, num_classes, device):
        self.C = int(num_classes)
        self.counts = torch.zeros((3, self.C), device=device, dtype=torch.int32)
        self.loss_sum = torch.zeros(1, device=device, dtype=torch.float64)
        self.n = 0

    def add(self, logits, target):
        logits = _chk(logits.detach(), 'logits')
        tgt = _chk(target.float(), 'target')
        B, Cc = logits.shape
        if Cc != self.C or tuple(tgt.shape) != (B, Cc):
            raise L.DynmmHipError(f'counts of {self.C} classes: got logits {tuple(logits.shape)}, target {tuple(tgt.shape)}')
        L.check(_lib().dynmm_ml_counts(_p(logits), _p(tgt), B, Cc, self.counts.data_ptr(), self.loss_sum.data_ptr(),
                                       _stream()), 'ml_counts')
        self.n += B

    def read(self):
        """{'tp', 'fp', 'fn': int64 [C] numpy, 'loss': mean BCE per sample and class, 'n': samples}"""
        c = self.counts.cpu().numpy().astype(np.int64)
        loss = float(self.loss_sum.item()) / max(self.n * self.C, 1)
        return {'tp': c[0], 'fp': c[1], 'fn': c[2], 'loss': loss, 'n': self.n}


def f1_from_counts(tp, fp, fn):
    """(micro, macro) F1 (sklearn.metrics.f1_score, zero_division=0: a class with 2tp + fp + fn = 0 scores 0)."""
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))
    den = 2 * tp + fp + fn
    per = np.divide(2 * tp, den, out=np.zeros_like(den), where=den > 0)
    d = 2 * tp.sum() + fp.sum() + fn.sum()
    micro = float(2 * tp.sum() / d) if d > 0 else 0.0
    return micro, float(per.mean())


# ---------------------------------------------------------------------------------------------------------------
# hard-gate compaction
# ---------------------------------------------------------------------------------------------------------------
def partition(weight):
    """(order [B], inv [B], counts [K]) device int32: the samples grouped by their gate's arg-max (ties to the lower expert),
    stable; inv is the inverse permutation."""
    weight = _chk(weight.detach(), 'weight')
    B, K = weight.shape
    i32 = dict(device=weight.device, dtype=torch.int32)
    order, inv, counts = torch.empty(B, **i32), torch.empty(B, **i32), torch.empty(K, **i32)
    L.check(_lib().dynmm_ml_partition(_p(weight), K, B, order.data_ptr(), inv.data_ptr(), counts.data_ptr(), _stream()),
            'ml_partition')
    return order, inv, counts

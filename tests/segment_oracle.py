"""float64 restatement, in plain torch, of what csrc/segment.hip computes, the seeded inputs of tests/test_segment.py and the
one comparison rule every label map is held to.

The rule: labels must be EQUAL wherever the reference's top-1 - top-2 margin exceeds tau = 1e-5 * max|logit|, and at most
0.1 % of a case's pixels may fall under tau (asserted on the reference itself, so the cap cannot hide a failure).  tau is about
50x the fp32 error of the two stencils: the torch float32 composition was within 2.1e-7 * max of float64 on these inputs (CPU),
and the reference alone leaves out at most 0.023 % of the pixels at tau."""
import functools

import torch
import torch.nn.functional as F

TAU_REL = 1e-5
UNDER_CAP = 1e-3

# (N, C, H, W) of x, the quarter-resolution map.  The kernel's tile is 8 x 32 pixels of x (csrc/segment.hip kSR x kSC):
# (17, 65) is one past TWO tiles in both directions — "tile + 1" with more than one workgroup along each axis — at the largest C.
TAIL_SHAPES = [(2, 40, 15, 20), (1, 64, 17, 65), (3, 13, 33, 31), (1, 5, 1, 1), (1, 3, 1, 7), (1, 1, 4, 4)]
BORDERS = ('zero', 'replicate')
# (H, W) -> (Ho, Wo) of argmax_resize, C = 40, N = 2
RESIZE_CASES = [((15, 20), (15, 20)), ((15, 20), (37, 53)), ((16, 24), (8, 12))]
RESIZE_N, RESIZE_C = 2, 40


def up_learned(x, w, b, border):
    """One learned 2x up-sampling (model.py:404-410): nearest x2 -> (replicate pad ->) depthwise 3x3."""
    C = x.shape[1]
    y = F.interpolate(x, scale_factor=2, mode='nearest')
    if border == 'replicate':
        return F.conv2d(F.pad(y, (1, 1, 1, 1), mode='replicate'), w.reshape(C, 1, 3, 3), b, padding=0, groups=C)
    return F.conv2d(y, w.reshape(C, 1, 3, 3), b, padding=1, groups=C)


def tail_logits(x, w1, b1, w2, b2, border):
    """up2(up1(x)) in float64."""
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    return up_learned(up_learned(x, w1, b1, border), w2, b2, border)


def resize_logits(logits, size):
    """bilinear, align_corners=False, in float64 (the identity when the size is the logits' own)."""
    x = logits.double()
    if tuple(size) == tuple(x.shape[-2:]):
        return x
    return F.interpolate(x, size=tuple(size), mode='bilinear', align_corners=False)


def labels_and_margin(logits):
    """(first-maximum arg-max [N,H,W], top-1 - top-2 margin [N,H,W], tau) of float64 logits [N,C,H,W]."""
    logits = logits.double()
    lab = logits.argmax(1)
    if logits.shape[1] == 1:
        margin = torch.full(lab.shape, float('inf'), dtype=torch.float64)
    else:
        top = logits.topk(2, dim=1).values
        margin = top[:, 0] - top[:, 1]
    return lab, margin, TAU_REL * logits.abs().max().item()


def under_share(logits):
    _, margin, tau = labels_and_margin(logits)
    return (margin <= tau).double().mean().item()


def assert_labels(pred, logits, what=''):
    """The comparison rule.  pred: integer label map (any device); logits: the float64 reference."""
    lab, margin, tau = labels_and_margin(logits.cpu())
    pred = pred.cpu().long()
    assert pred.shape == lab.shape, (what, pred.shape, lab.shape)
    under = margin <= tau
    share = under.double().mean().item()
    wrong = ((pred != lab) & ~under).sum().item()
    print(f'{what}: {under.sum().item()} of {under.numel()} pixels under tau = {tau:.3e} ({100 * share:.4f} %), '
          f'{(pred != lab).sum().item()} labels differ, {wrong} of them above tau')
    assert share <= UNDER_CAP, (what, share)
    assert wrong == 0, (what, wrong)
    return int(under.sum().item())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def tail_case(shape, seed=0):
    """(x, w1, b1, w2, b2) on the CPU, float32: weights 0.3 * randn, biases randn (a non-zero b1 matters), x = randn."""
    N, C, H, W = shape
    g = _gen(1000 + seed + 7 * C + 31 * H + 131 * W)
    x = torch.randn(N, C, H, W, generator=g)
    w1, w2 = 0.3 * torch.randn(C, 1, 3, 3, generator=g), 0.3 * torch.randn(C, 1, 3, 3, generator=g)
    b1, b2 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def tail_reference(shape, border, seed=0):
    """float64 logits of a tail case: computed once, shared, never modified."""
    return tail_logits(*tail_case(shape, seed), border)


@functools.lru_cache(maxsize=None)
def resize_case(hw, out_hw):
    """(logits [N,C,H,W] float32, label [N,Ho,Wo] uint8 with void (0) among 1..C) on the CPU."""
    g = _gen(2000 + 13 * hw[0] + 17 * out_hw[1])
    logits = torch.randn(RESIZE_N, RESIZE_C, *hw, generator=g)
    label = torch.randint(0, RESIZE_C + 1, (RESIZE_N, *out_hw), generator=g).to(torch.uint8)
    return logits, label


@functools.lru_cache(maxsize=None)
def resize_reference(hw, out_hw):
    return resize_logits(resize_case(hw, out_hw)[0], out_hw)


def constructed_case(which):
    """The two constructed cases (C = 2, 3 x 4 -> 12 x 16, margins >= 0.13): channel 1 is the constant 0.8 (w = 0, b2 = 0.8).
    A: channel 0 has x = 0, b1 = 1, w2 = 1/9 everywhere -> zero padding gives class 1 on the outermost ring and class 0 inside,
       replicate gives class 0 everywhere (b1 reaches a border logit through fewer of w2's taps).
    B: channel 0 has x = 1, w1 = 1/9 everywhere, b1 = 0, w2 = centre tap only -> zero padding gives class 1 on the outermost
       TWO rings, replicate class 0 everywhere.
    Returns (x, w1, b1, w2, b2, {border: expected labels [1,12,16]})."""
    x = torch.zeros(1, 2, 3, 4)
    w1, w2 = torch.zeros(2, 1, 3, 3), torch.zeros(2, 1, 3, 3)
    b1, b2 = torch.zeros(2), torch.tensor([0.0, 0.8])
    rings = 1
    if which == 'A':
        b1[0] = 1.0
        w2[0] = 1.0 / 9
    else:
        x[:, 0] = 1.0
        w1[0] = 1.0 / 9
        w2[0, 0, 1, 1] = 1.0
        rings = 2
    zero = torch.ones(1, 12, 16, dtype=torch.long)
    zero[:, rings:12 - rings, rings:16 - rings] = 0
    return x, w1, b1, w2, b2, {'zero': zero, 'replicate': torch.zeros(1, 12, 16, dtype=torch.long)}

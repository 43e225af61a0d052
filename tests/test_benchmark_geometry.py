"""The hot path's kernels at the geometry the benchmark runs (480x640 input, BASELINE.json configs[2]): every convolution shape
of the model against torch in float64 on the CPU at batch 4 — the C = 64 rows at 120x160 also at the benchmark's batch 32 — with
the bars of tests/test_hip_ops.py (TOL / GTOL, imported), and the other kernels at their benchmark planes.

TABLE is complete by construction: a CPU test records every convolution the oracle evaluates at 480x640 and compares the set
with the table in both directions.  Several code paths are selected by size and are live only here (8 slabs of BatchNorm
sums, weight-gradient splits, multi-round grids, tiles that straddle images at rows of 160 / 80 / 40 / 20 pixels); a case that
exists to reach such a path asserts that it did (`LIVE`, checked by the last test of the module).

Measured on an MI355X against float64 (each case prints its figures): forward 3e-7 .. 1.3e-6, gradients 3e-7 .. 1.6e-6 at batch 32,
where a weight gradient sums 614 400 products — every row meets TOL / GTOL as they stand, so no row carries a bar derived from
the fp32 CPU reference's own error."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import helpers as Hh
from tests import test_hip_ops as T
from tests.test_hip_ops import GTOL, TOL, close, rel, rnd, ops  # noqa: F401  (ops: the module-scoped fixture)

gpu = pytest.mark.gpu

# (Ci, Co, kernel, stride, padding, bias, H, W): the 42 dense convolutions on planes larger than 1x1 that configs P_se
# (NonBottleneck1D) and S_se (BasicBlock) evaluate in one training forward at 480x640
TABLE = [
    # stems
    (1, 64, (7, 7), (2, 2), (3, 3), False, 480, 640),
    (3, 64, (7, 7), (2, 2), (3, 3), False, 480, 640),
    # gate: the dual-input convolution (64 + 64 channels, never concatenated on the HIP path) and its successor
    (128, 8, (5, 5), (2, 2), (0, 0), True, 120, 160),
    (8, 8, (5, 5), (2, 2), (0, 0), True, 58, 78),
    # stage 1 (C = 64 at 120x160): NonBottleneck1D / BasicBlock
    (64, 64, (3, 1), (1, 1), (1, 0), True, 120, 160),
    (64, 64, (1, 3), (1, 1), (0, 1), True, 120, 160),
    (64, 64, (3, 3), (1, 1), (1, 1), False, 120, 160),
    # first blocks of stages 2-4 (stride 2) and their down-sampling 1x1
    (64, 128, (3, 1), (2, 1), (1, 0), True, 120, 160),
    (128, 128, (1, 3), (1, 2), (0, 1), True, 60, 160),
    (64, 128, (3, 3), (2, 2), (1, 1), False, 120, 160),
    (64, 128, (1, 1), (2, 2), (0, 0), False, 120, 160),
    (128, 256, (3, 1), (2, 1), (1, 0), True, 60, 80),
    (256, 256, (1, 3), (1, 2), (0, 1), True, 30, 80),
    (128, 256, (3, 3), (2, 2), (1, 1), False, 60, 80),
    (128, 256, (1, 1), (2, 2), (0, 0), False, 60, 80),
    (256, 512, (3, 1), (2, 1), (1, 0), True, 30, 40),
    (512, 512, (1, 3), (1, 2), (0, 1), True, 15, 40),
    (256, 512, (3, 3), (2, 2), (1, 1), False, 30, 40),
    (256, 512, (1, 1), (2, 2), (0, 0), False, 30, 40),
    # stages 2-4, decoder blocks (128 channels at 15x20 / 30x40 / 60x80) and decoder conv3x3
    (128, 128, (3, 1), (1, 1), (1, 0), True, 60, 80),
    (128, 128, (1, 3), (1, 1), (0, 1), True, 60, 80),
    (128, 128, (3, 3), (1, 1), (1, 1), False, 60, 80),
    (128, 128, (3, 1), (1, 1), (1, 0), True, 30, 40),
    (128, 128, (1, 3), (1, 1), (0, 1), True, 30, 40),
    (128, 128, (3, 3), (1, 1), (1, 1), False, 30, 40),
    (128, 128, (3, 1), (1, 1), (1, 0), True, 15, 20),
    (128, 128, (1, 3), (1, 1), (0, 1), True, 15, 20),
    (128, 128, (3, 3), (1, 1), (1, 1), False, 15, 20),
    (256, 256, (3, 1), (1, 1), (1, 0), True, 30, 40),
    (256, 256, (1, 3), (1, 1), (0, 1), True, 30, 40),
    (256, 256, (3, 3), (1, 1), (1, 1), False, 30, 40),
    (512, 512, (3, 1), (1, 1), (1, 0), True, 15, 20),
    (512, 512, (1, 3), (1, 1), (0, 1), True, 15, 20),
    (512, 512, (3, 3), (1, 1), (1, 1), False, 15, 20),
    # skip layers, pyramid pooling (5x5 bin, final convolution), side outputs, conv_out
    (64, 128, (1, 1), (1, 1), (0, 0), False, 120, 160),
    (256, 128, (1, 1), (1, 1), (0, 0), False, 30, 40),
    (512, 256, (1, 1), (1, 1), (0, 0), False, 5, 5),
    (1024, 128, (1, 1), (1, 1), (0, 0), False, 15, 20),
    (128, 40, (1, 1), (1, 1), (0, 0), True, 15, 20),
    (128, 40, (1, 1), (1, 1), (0, 0), True, 30, 40),
    (128, 40, (1, 1), (1, 1), (0, 0), True, 60, 80),
    (128, 40, (3, 3), (1, 1), (1, 1), True, 120, 160),
]

# (C, H, W) of the five depthwise 3x3 convolutions of the learned up-sampling (their OUTPUT planes): item "other kernels" below
DEPTHWISE = [(128, 30, 40), (128, 60, 80), (128, 120, 160), (40, 240, 320), (40, 480, 640)]

# dense convolutions on 1x1 planes (squeeze-and-excite MLPs, the gate head's fc, the pooled pyramid branch): deliberately left to
# their own tests (test_se_fuse_blend, test_gate_head, test_pyramid_pooling, test_model_*) — no plane, no geometry to scale
ON_1X1_PLANES = [(4, 64, True), (64, 4, True), (8, 128, True), (128, 8, True), (16, 256, True), (256, 16, True), (32, 512, True),
                 (512, 32, True), (8, 5, False), (512, 256, False)]

N_SMALL, N_BENCH = 4, 32


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def test_table_holds_every_convolution_of_the_480x640_models():
    """Every convolution of the oracle goes through F.conv2d (oracle/dynmm_oracle.py _conv): record each call's geometry in one
    training forward of P_se and S_se at 480x640 (batch 2: the training-mode BatchNorm of the 1x1 pooled branch refuses batch 1)
    and compare with the tables above in both directions.  51 + 45 distinct geometries, 57 in the union: 42 dense ones on planes
    larger than 1x1 (TABLE), 5 depthwise (DEPTHWISE), 10 on 1x1 planes (ON_1X1_PLANES)."""
    from dynmm_amd import synth
    from oracle import dynmm_oracle as O
    seen = set()
    real = O.F.conv2d

    def spy(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        assert _pair(dilation) == (1, 1)
        seen.add((int(x.shape[1]), int(w.shape[0]), tuple(w.shape[2:]), _pair(stride), _pair(padding), b is not None,
                  int(x.shape[2]), int(x.shape[3]), int(groups)))
        return real(x, w, b, stride, padding, dilation, groups)
    rgb, depth = synth.synth_inputs(2, 480, 640, seed=1)
    for cfg in ('P_se', 'S_se'):
        sd = Hh.filled_state_dict(Hh.CFGS[cfg], seed=0)
        O.F.conv2d = spy
        try:
            with torch.no_grad():
                O.forward(sd, rgb, depth, Hh.CFGS[cfg], training=True)
        finally:
            O.F.conv2d = real
    dense = {g[:8] for g in seen if g[8] == 1 and g[6:8] != (1, 1)}
    depthwise = {(g[0], g[6], g[7]) for g in seen if g[8] != 1}
    small = {(g[0], g[1], g[5]) for g in seen if g[8] == 1 and g[6:8] == (1, 1)}
    assert all(g[8] in (1, g[0]) for g in seen)
    assert all(g[2:6] == ((3, 3), (1, 1), (1, 1), True) and g[0] == g[1] for g in seen if g[8] != 1)
    assert all(g[2:5] == ((1, 1), (1, 1), (0, 0)) for g in seen if g[6:8] == (1, 1))
    assert len(TABLE) == len(set(TABLE)) == 42 and len(seen) == 57
    assert dense - set(TABLE) == set(), f'convolutions of the model without a case: {sorted(dense - set(TABLE))}'
    assert set(TABLE) - dense == set(), f'cases the model does not run: {sorted(set(TABLE) - dense)}'
    assert depthwise == set(DEPTHWISE), (sorted(depthwise), DEPTHWISE)
    assert small == set(ON_1X1_PLANES), sorted(small ^ set(ON_1X1_PLANES))


# ------------------------------------------------------------------------------------------------ row classes
def _is(row, ks, stride):
    return row[2] in ks and row[3] in stride


S1_TAPS = [r for r in TABLE if _is(r, ((1, 3), (3, 1), (3, 3)), ((1, 1),))]                    # Winograd homes / operand ring
S2_TAPS = [r for r in TABLE if _is(r, ((1, 3), (3, 1)), ((2, 1), (1, 2)))]                     # polyphase input gradient
S2_3X3 = [r for r in TABLE if _is(r, ((3, 3),), ((2, 2),))]
ONE_BY_ONE = [r for r in TABLE if r[2] == (1, 1)]
GATE = [r for r in TABLE if r[2] == (5, 5)]
STEMS = [r for r in TABLE if r[2] == (7, 7)]
assert len(S1_TAPS) + len(S2_TAPS) + len(S2_3X3) + len(ONE_BY_ONE) + len(GATE) + len(STEMS) == len(TABLE)
assert (len(S1_TAPS), len(S2_TAPS), len(S2_3X3), len(ONE_BY_ONE), len(GATE), len(STEMS)) == (19, 6, 3, 10, 2, 2)


def _batches(row):
    """Batch 4 for every row; the C = 64 rows at 120x160 also at the benchmark's batch."""
    return [N_SMALL, N_BENCH] if (row[0] == 64 and row[6:8] == (120, 160)) else [N_SMALL]


def _with_batches(rows):
    return [(n, r) for r in rows for n in _batches(r)]


def _id(v):
    if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], tuple):
        n, (ci, co, k, s, p, b, h, w) = v
        return f'n{n}-{ci}to{co}-k{k[0]}x{k[1]}-s{s[0]}x{s[1]}-{h}x{w}'
    return None


def _geom(row, n, dual=False):
    from dynmm_amd import lib as L
    ci, co, k, s, p, b, h, w = row
    ho, wo = (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1
    return L.ConvGeom(n, ci, h, w, co, ho, wo, k[0], k[1], s[0], s[1], p[0], p[1], 64 if dual else ci)


def _fwd_case(row, n):
    ci, co, k, s, p, b, h, w = row
    # conv3x1_1 of NonBottleneck1D is followed by a ReLU (resnet.py:125): the activation epilogue rides on those rows
    return (n, ci, h, w, co, k, s, p, b, 'relu' if (k == (3, 1) and b) else None)


# which selection-by-size paths the cases of this module reached; asserted by the last test
LIVE = {'variants': set(), 'ring': set(), 'splits': set(), 'rows': set(), 'slots8': set()}


def _note(ops, row, n, what, dual=False):
    lib, g = ops._lib(), _geom(row, n, dual)
    LIVE['ring'].add(int(lib.dynmm_conv2d_uses_operand_ring(C.byref(g), 0)))
    variant = int(lib.dynmm_conv2d_wgrad_variant(C.byref(g)))
    LIVE['variants'].add(variant)
    if lib.dynmm_conv2d_wgrad_workspace_bytes(C.byref(g)) > 4 * row[0] * row[1] * row[2][0] * row[2][1]:
        LIVE['splits'].add(variant)         # a workspace beyond one weight tensor: the pixel range is split into several slabs
    LIVE['rows'].add((row, what))
    return variant


# ------------------------------------------------------------------------------------------------ item 2: convolutions
# Batch 32 costs a float64 reference of 39 M elements per tensor: what would only repeat a launch another batch-32 case already
# makes is run at batch 4 alone (the suite's time budget: the new tests together cost about what tests/test_hip_model.py did).
@gpu
@pytest.mark.parametrize('case', [(n, r) for r in TABLE[2:] for n in ([N_SMALL] if r in S1_TAPS else _batches(r))], ids=_id)
def test_conv2d_at_benchmark_geometry(ops, case):
    """ops.conv2d as the model calls it (product defaults: Winograd forward where it has a home, F(4,3) / F(2,3) / 2-D input
    gradients, three-tap / vectorised / generic weight gradients), single input: forward, input, weight and bias gradient
    against float64.  (The stems and the dual-input gate convolution have tests of their own below; the gate convolution
    runs here as the single 128-channel input the oracle sees.  Batch 32 for the C = 64 rows without a Winograd home; those
    with one run the same launches, with mask and residual on top, in test_conv2d_winograd_at_benchmark_geometry.)"""
    n, row = case
    _note(ops, row, n, 'conv2d')
    print(_id(case), T.check_conv2d_fwd_bwd(ops, _fwd_case(row, n), torch.float64))


@gpu
@pytest.mark.parametrize('case', [(N_SMALL, r) for r in S1_TAPS], ids=_id)
def test_conv2d_direct_kernels_at_benchmark_geometry(ops, case):
    """The same rows with the Winograd kernels switched off (ops.WINO = '0'): the operand-ring kernels (conv_igemm_v5.hip) for
    forward and input gradient where the library says they serve the geometry; conv_out (128 -> 40: Co % 64 != 0) is refused by
    them and takes the round-2 tiles, at the same bars.  (Batch 4 only: training at batch 32 does not run these kernels.)"""
    n, row = case
    lib, g = ops._lib(), _geom(row, n)
    ring = (int(lib.dynmm_conv2d_uses_operand_ring(C.byref(g), 0)), int(lib.dynmm_conv2d_uses_operand_ring(C.byref(g), 1)))
    assert ring == ((0, 0) if row[1] % 64 else (1, 1)), (row, ring)
    calls, old = [], ops.WINO
    ops.WINO, ops.PROFILE = '0', calls
    try:
        err = T.check_conv2d_fwd_bwd(ops, _fwd_case(row, n), torch.float64)
    finally:
        ops.WINO, ops.PROFILE = old, None
    names = [c[0] for c in calls]
    assert not any('wino' in x for x in names), names
    for kind, on in zip(('fwd', 'dgrad'), ring):
        assert any(x.startswith(f'conv_igemm_v5_{kind}') for x in names) == bool(on), names
    LIVE['ring'].update(ring)
    print(_id(case), err)


def _winograd_cases():
    """All three modes at batch 4.  At batch 32 the modes that launch something the others do not: 'all' (Winograd forward;
    F(2,3) / 2-D input gradient) for every filter shape, 'dgrad43' (the F(4,3) input gradient) for 1x3 — 'dgrad' launches a
    subset of 'all', and 'dgrad43' differs from it for 1x3 filters only."""
    out = []
    for r in S1_TAPS:
        out += [(m, (N_SMALL, r)) for m in ('dgrad', 'all', 'dgrad43')]
        if N_BENCH in _batches(r):
            out += [(m, (N_BENCH, r)) for m in (('all', 'dgrad43') if r[2] == (1, 3) else ('all',))]
    return out


@gpu
@pytest.mark.parametrize('mode,case', _winograd_cases(), ids=lambda v: v if isinstance(v, str) else _id(v))
def test_conv2d_winograd_at_benchmark_geometry(ops, mode, case):
    """test_conv2d_winograd's protocol in its three modes: forward, input gradient with the producer's ReLU mask and the residual
    gradient in the epilogue, weight and bias gradient, and the ops.PROFILE check that the intended kernel ran."""
    n, row = case
    _note(ops, row, n, 'winograd ' + mode)
    print(_id(case), mode, T.check_conv2d_winograd(ops, mode, (n, row[0], row[6], row[7], row[1], row[2])))


@gpu
@pytest.mark.parametrize('case', _with_batches(S2_TAPS), ids=_id)
def test_stride2_input_gradient_at_benchmark_geometry(ops, case):
    """test_conv2d_stride2_input_gradient_on_the_pair_kernel's protocol (mask + residual in the polyphase input gradient)."""
    n, row = case
    _note(ops, row, n, 'stride-2 pair kernel')
    T.check_conv2d_stride2_input_gradient_on_the_pair_kernel(ops, (n, row[0], row[6], row[7], row[1], row[2], row[3], row[4]))


@gpu
def test_gate_convolution_at_benchmark_geometry(ops, n=N_SMALL):
    """The dual-input gate convolution 64 + 64 -> 8, 5x5, stride 2 at 120x160 (test_conv2d_dual_input's protocol, float64)."""
    assert _note(ops, GATE[0], n, 'dual input', dual=True) == 8          # conv_small.hip: weight and bias gradient on the vector ALUs
    T.check_conv2d_dual_input(ops, (n, 64, 120, 160), torch.float64)


@gpu
@pytest.mark.parametrize('row', STEMS, ids=lambda r: f'ci{r[0]}')
def test_stems_at_benchmark_geometry(ops, row):
    """Both 7x7 stems at 480x640, batch 4: without the statistics epilogue through ops.conv2d (forward, weight gradient; the
    depth stem's input gradient too), with it through test_stem_conv_epilogue_batchnorm_statistics's protocol."""
    _note(ops, row, N_SMALL, 'stem')
    print('stem', row[0], T.check_conv2d_fwd_bwd(ops, _fwd_case(row, N_SMALL), torch.float64))
    T.check_stem_conv_epilogue_batchnorm_statistics(ops, (N_SMALL, row[0], row[6], row[7]))


@gpu
@pytest.mark.parametrize('row', TABLE[2:], ids=lambda r: _id((N_SMALL, r)))
def test_grouped_weight_gradients_at_benchmark_geometry(ops, row):
    """dynmm_conv2d_wgrad_group with 3 members on every groupable row (test_grouped_weight_gradients's protocol, bit-identical
    repeats included).  What the library does not group asserts the refusal: 512 -> 256 on the 5x5 pooled plane (100 pixels: a
    single-split plan) and the gate convolution, with one input or two (its own kernel); their weight gradients are
    held to the bar by test_conv2d_at_benchmark_geometry / test_gate_convolution_at_benchmark_geometry.  (The stems have their
    own weight-gradient kernel and are not groupable either: test_stems_at_benchmark_geometry.)"""
    lib, g = ops._lib(), _geom(row, N_SMALL)
    kind = lib.dynmm_conv2d_wgrad_groupable(C.byref(g))
    if row in (GATE[0], (512, 256, (1, 1), (1, 1), (0, 0), False, 5, 5)):
        assert kind == 0 and lib.dynmm_conv2d_wgrad_groupable(C.byref(_geom(row, N_SMALL, dual=row == GATE[0]))) == 0
        return
    assert kind in (1, 2), (row, kind)
    _note(ops, row, N_SMALL, 'group')
    ci, co, k, s, p, b, h, w = row
    T.check_grouped_weight_gradients(ops, (N_SMALL, ci, h, w, co, k, p, b, s))


@gpu
@pytest.mark.parametrize('case', _with_batches([r for r in S1_TAPS if r[2] != (3, 1)]), ids=_id)
def test_statistics_epilogue_at_benchmark_geometry(ops, case):
    """test_conv_epilogue_batchnorm_statistics's protocol on the 1x3 and 3x3 rows (the convolutions that feed a training-mode
    BatchNorm).  conv_out (Co = 40) has no statistics epilogue: the refusal is asserted.  At batch 32 the C = 64 rows spread their
    4800 pixel tiles over 8 slabs."""
    n, row = case
    lib, g = ops._lib(), _geom(row, n)
    slots = lib.dynmm_conv2d_wino2d_stats_slots(C.byref(g)) if row[2] == (3, 3) else lib.dynmm_conv2d_wino_fwd_stats_slots(C.byref(g))
    if row[1] % 64:
        assert slots == 0, (row, slots)
        return
    assert slots == (8 if (n, row[0]) == (N_BENCH, 64) else 1), (row, n, slots)
    if slots == 8:
        LIVE['slots8'].add('wino2d_stats' if row[2] == (3, 3) else 'wino_fwd_stats')
    T.check_conv_epilogue_batchnorm_statistics(ops, (n, row[0], row[6], row[7], row[1], row[2]))


@gpu
@pytest.mark.parametrize('case', _with_batches([r for r in S1_TAPS if r[2] == (3, 1)]), ids=_id)
def test_fused_backward_reductions_at_benchmark_geometry(ops, case):
    """test_batchnorm_backward_reductions_from_the_consumer_dgrad's and test_bn2_backward_reductions_kernel_vs_float64's
    protocols on the 3x1 rows (conv3x1_2 consumes bn1's output; the next block's conv3x1_1 the block's own).  At batch 32 the
    C = 64 row adds into 8 slabs."""
    n, row = case
    c, h, w = row[0], row[6], row[7]
    want = 8 if (n, c) == (N_BENCH, 64) else 1
    assert T.check_batchnorm_backward_reductions_from_the_consumer_dgrad(ops, (n, c, h, w, c), True) == want
    assert T.check_bn2_backward_reductions_kernel_vs_float64(ops, (n, c, h, w)) == want
    if want == 8:
        LIVE['slots8'].add('wino_dgrad_bnred')


# ------------------------------------------------------------------------------------------------ item 4: the other kernels
@gpu
def test_maxpool_at_the_stem_plane(ops):
    T.check_maxpool_with_ties(ops, (240, 320), n=4)


@gpu
@pytest.mark.parametrize('shape', [(4, 64, 240, 320), (4, 64, 120, 160)])
def test_batchnorm_residual_relu_bits_at_benchmark_planes(ops, shape):
    T.test_batchnorm_residual_relu_decisions_as_bits(ops, shape, True)


@gpu
@pytest.mark.parametrize('use_se,col', [(True, 0), (True, None), (False, 3)])
def test_se_fuse_blend_at_the_stage1_plane(ops, use_se, col):
    T.test_se_fuse_blend(ops, use_se, col, (4, 64, 120, 160))


@gpu
@pytest.mark.parametrize('use_se', [True, False])
def test_fused_stem_tail_at_the_stem_plane(ops, use_se):
    """test_stem_bn_fuse_pool_equals_unfused_ops's protocol (stem BatchNorm + ReLU + SE fusion + both max-pools in the fused
    kernels against the unfused ops) on 4x64x240x320."""
    T.check_stem_bn_fuse_pool_equals_unfused_ops(ops, use_se, (4, 64, 240, 320))


@gpu
def test_pyramid_pooling_ops_at_the_stage4_plane(ops):
    """The context module's ops on 512 @ 15x20, batch 4: adaptive average pooling to 1x1 and 5x5, nearest and bilinear concat of
    the 256-channel branches (512 + 256 + 256 = the 1024 input channels of final_conv)."""
    from tests import test_decoder_modes as D
    for out in (1, 5):
        T.check_adaptive_avg_pool(ops, (15, 20), out, n=4, c=512)
    T.check_nearest_concat(ops, (15, 20), n=4, cs=(512, 256, 256))
    D.check_bilinear_resize_concat((5, 5), (15, 20), N=4, C0=512, C1=256)


@gpu
@pytest.mark.parametrize('c,h,w', [(c, h // 2, w // 2) for c, h, w in DEPTHWISE])
def test_upsampling_at_the_five_depthwise_geometries(ops, c, h, w):
    """All modes of test_upsample2x_modes (nearest / bilinear / learned 3x3 with replicated border) and the zero-padded learned
    one of test_upsample2x_dw3x3, with and without the skip operand, on the inputs of the five recorded depthwise convolutions
    (batch 2; the two 40-class maps, up to 480x640, at batch 1)."""
    from tests import test_decoder_modes as D
    n = 1 if c == 40 else 2
    for with_skip in (False, True):
        T.test_upsample2x_dw3x3(ops, (n, c, h, w), with_skip)
        for mode in ('nearest', 'bilinear', 'learned-3x3'):
            D.test_upsample2x_modes((n, c, h, w), mode, with_skip)


@gpu
def test_fused_loss_tail_at_benchmark_geometry(ops):
    """test_fused_upsample_cross_entropy_tail's protocol at 2x40x240x320 -> 480x640, with its run of void pixels."""
    T.check_fused_upsample_cross_entropy_tail(ops, (2, 40, 240, 320))


@gpu
def test_cross_entropy_at_benchmark_geometry(ops):
    """cross_entropy_2d on 2x40x480x640 logits with void pixels against the oracle's own loss in float64."""
    from oracle import dynmm_oracle as O
    g = torch.Generator().manual_seed(3)
    x = rnd(2, 40, 480, 640, seed=1, scale=2.0)
    t = torch.randint(0, 41, (2, 480, 640), generator=g)
    t[1, 100:140] = 0
    cw = torch.rand(40, generator=g) + 0.5
    xr = x.double().requires_grad_(True)
    l_ref = O.cross_entropy_2d([xr], [t], cw.double())[0]
    l_ref.backward()
    xg = x.cuda().requires_grad_(True)
    l = ops.cross_entropy_2d(xg, t.cuda(), cw.cuda())
    assert abs(l.item() - l_ref.item()) < 1e-5 * max(1.0, abs(l_ref.item()))
    l.backward()
    close(xg.grad, xr.grad, 1e-4, 'cross-entropy gradient')


@gpu
def test_eval_confusion_at_benchmark_geometry(ops):
    """eval_confusion on 2x40x480x640 logits and 480x640 labels (identity resize) and on 2x40x240x320 logits resized to
    480x640.  The tie allowance is COUNTED, not copied: a pixel may be classified differently from the float64 bilinear logits
    only where their two largest classes lie within 1e-5 of the plane's maximum of each other; that count is taken on the CPU
    here (with these inputs: 81 pixels of 614 400 at 480x640, 74 from 240x320), printed, and is the number of disagreements
    allowed (each moves one count out of a cell and into another: 2 per pixel)."""
    g = torch.Generator().manual_seed(5)
    for hw in ((480, 640), (240, 320)):
        x = rnd(2, 40, *hw, seed=1)
        label = torch.randint(0, 41, (2, 480, 640), generator=g)
        logits = F.interpolate(x.double(), (480, 640), mode='bilinear', align_corners=False)
        top = logits.topk(2, dim=1).values
        ties = int(((top[:, 0] - top[:, 1]) <= 1e-5 * logits.abs().max()).sum())
        print(f'eval_confusion {hw}: {ties} pixels with their two largest classes within 1e-5 of the maximum')
        pred, mask = logits.argmax(1), label > 0
        ref = torch.bincount(40 * (label[mask] - 1) + pred[mask], minlength=1600).reshape(40, 40)
        cm = torch.zeros(40, 40, dtype=torch.int64, device='cuda')
        ops.eval_confusion(x.cuda(), label.cuda(), cm)
        assert cm.sum().item() == mask.sum().item()
        diff = (cm.cpu() - ref).abs().sum().item()
        assert diff <= 2 * ties, (hw, diff, ties)


# ------------------------------------------------------------------------------------------------ liveness
@gpu
def test_every_size_selected_path_was_reached(ops):
    """The cases above exist to reach paths that only this geometry selects; this asserts they did (it runs last in the module
    and needs the tests above to have run in the same session)."""
    lib = ops._lib()
    want_variants, want_ring = set(), set()
    for row in TABLE:
        g = _geom(row, N_SMALL)
        want_variants.add(int(lib.dynmm_conv2d_wgrad_variant(C.byref(g))))
        want_ring.add(int(lib.dynmm_conv2d_uses_operand_ring(C.byref(g), 0)))
    assert want_variants == {0, 4, 6, 8} and want_ring == {0, 1}
    assert LIVE['variants'] == want_variants, LIVE['variants']
    assert LIVE['ring'] == want_ring, LIVE['ring']
    assert LIVE['splits'] >= {0, 4, 6}, LIVE['splits']          # every split-K weight-gradient variant ran with several splits
    assert LIVE['slots8'] == {'wino_fwd_stats', 'wino2d_stats', 'wino_dgrad_bnred'}, LIVE['slots8']
    assert {r for r, _ in LIVE['rows']} == set(TABLE), set(TABLE) - {r for r, _ in LIVE['rows']}
    T._WINO_REF.clear()         # (the batch-32 reference of the last Winograd case: 2 GB of float64)

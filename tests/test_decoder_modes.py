"""The decoder variants of ESANet's flags: --upsampling nearest | bilinear | learned-3x3 | learned-3x3-zeropad,
--context_module ppm | ppm-1-2-4-8 | appm | appm-1-2-4-8 | None, --encoder_decoder_fusion add | None
(FusionDynMM/src/models/model.py:311-410, context_modules.py:16-131, model_skip_mod_globalgate.py:145-207).

CPU: state_dict keys / shapes of all three networks against the reference's (tests/golden/make_decoder_modes_goldens.py),
build_model with every CLI value, the refusals that stay.
GPU: the new kernels (csrc/resample.hip) against torch fp64 on the CPU; the modules against tests/decoder_modes_oracle.py;
the networks against the reference fixture; InferStep replays and hard-gate compaction in a non-default mode."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynmm_amd import synth
from tests import decoder_modes_oracle as DO
from tests import helpers as Hh

TOL, GTOL = 2e-5, 2e-4                   # tests/test_hip_ops.py
LOGIT_TOL, TRAIN_OUT_TOL = 2e-4, 1e-3    # tests/test_hip_model.py
CLASSES = ('gate', 'skip', 'esanet')


def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'decoder_modes_96x128.npz'))


def parse(name):
    up, ctx, fusion = name.split('|')
    return dict(upsampling=up, context_module=ctx, encoder_decoder_fusion=fusion)


def make(cls, h=96, w=128, **flags):
    """The fixture's configurations (make_goldens.py build('P_se'), skip_fixture, esanet_fixture)."""
    kw = dict(height=h, width=w, num_classes=40, encoder_rgb='resnet34', encoder_depth='resnet34',
              encoder_block='NonBottleneck1D', channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3],
              pretrained_on_imagenet=False, fuse_depth_in_rgb_encoder='SE-add', **flags)
    if cls == 'gate':
        from dynmm_amd.nn.net import SkipGateESANet
        return SkipGateESANet(**kw)
    if cls == 'skip':
        from dynmm_amd.nn.net_skip import SkipESANet
        return SkipESANet(**kw)
    from dynmm_amd.nn.esanet import ESANet
    return ESANet(**kw)


def shapes(sd, keys):
    return [','.join(map(str, sd[k].shape)) for k in keys]


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('cls', CLASSES)
def test_state_dict_matches_reference_for_every_flag_value(golden_dir, cls):
    g = fixture(golden_dir)
    prefixes = ('decoder.', 'context_module.', 'skip_layer')
    for i, name in enumerate(str(c) for c in g['combos']):
        sd = make(cls, **parse(name)).state_dict()
        if i == 0:
            assert list(sd.keys()) == [str(k) for k in g[f'{cls}/full/keys']]
            assert shapes(sd, sd.keys()) == [str(s) for s in g[f'{cls}/full/shapes']]
        sub = [k for k in sd if k.startswith(prefixes)]
        assert sub == [str(k) for k in g[f'{cls}/{name}/keys']], (cls, name)
        assert shapes(sd, sub) == [str(s) for s in g[f'{cls}/{name}/shapes']], (cls, name)
        # everything else is what the default flags give
        rest = [k for k in sd if not k.startswith(prefixes)]
        full = [str(k) for k in g[f'{cls}/full/keys'] if not str(k).startswith(prefixes)]
        assert rest == full, (cls, name)


@pytest.mark.parametrize('flag,value', [('--upsampling', v) for v in ('nearest', 'bilinear', 'learned-3x3',
                                                                        'learned-3x3-zeropad')] +
                         [('--context_module', v) for v in ('ppm', 'ppm-1-2-4-8', 'appm', 'appm-1-2-4-8', 'None')] +
                         [('--encoder_decoder_fusion', v) for v in ('add', 'None')])
def test_build_model_accepts_each_cli_value(flag, value):
    from dynmm_amd.src.args import ArgumentParserRGBDSegmentation
    from dynmm_amd.src.build_model import build_model
    p = ArgumentParserRGBDSegmentation()
    p.set_common_args()
    for dyn in (['--dynamic', '--global-gate'], ['--dynamic'], []):
        args = p.parse_args(dyn + ['--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D', '--height', '96',
                                   '--width', '128', '--decoder_channels_mode', 'constant', '--nr_decoder_blocks', '1',
                                   '--no_imagenet_pretraining', flag, value])
        model, _ = build_model(args, n_classes=40)
        dec = model.decoder
        if flag == '--upsampling':
            assert dec.upsampling_mode == value and dec.decoder_module_1.upsample.mode == value
        if flag == '--encoder_decoder_fusion':
            assert dec.decoder_module_1.encoder_decoder_fusion == value
            assert isinstance(getattr(model, 'skip_layer0', None), torch.nn.Identity) == (value == 'None')
        if flag == '--context_module':
            kind = type(model.context_module).__name__
            assert kind == {'ppm': 'PyramidPoolingModule', 'ppm-1-2-4-8': 'PyramidPoolingModule',
                            'appm': 'AdaptivePyramidPoolingModule', 'appm-1-2-4-8': 'AdaptivePyramidPoolingModule',
                            'None': 'Identity'}[value]


def test_context_upsampling_follows_the_reference_rule():
    """model_skip_mod_globalgate.py:180-196: nearest for the learned modes, the decoder's mode otherwise; appm bins."""
    for up, ctx_mode in (('learned-3x3', 'nearest'), ('learned-3x3-zeropad', 'nearest'), ('nearest', 'nearest'),
                         ('bilinear', 'bilinear')):
        m = make('gate', upsampling=up, context_module='appm')
        assert m.context_module.upsampling_mode == ctx_mode
        assert m.context_module.bins == (1, 5) and m.context_module.input_size == (3, 4)
    assert make('gate', context_module='appm-1-2-4-8').context_module.bins == (1, 2, 4, 8)


def test_refusals_stay():
    from dynmm_amd.nn.net import SkipGateESANet
    with pytest.raises(NotImplementedError):
        SkipGateESANet(activation='gelu')
    for cls in CLASSES:
        with pytest.raises(NotImplementedError):
            make(cls, upsampling='bicubic')
        with pytest.raises(NotImplementedError):
            make(cls, encoder_decoder_fusion='concat')


def test_only_the_zeropad_decoder_defers_its_tail():
    for up in ('nearest', 'bilinear', 'learned-3x3'):
        assert make('gate', upsampling=up).decoder.upsampling_mode != 'learned-3x3-zeropad'
    assert make('gate').decoder.upsampling_mode == 'learned-3x3-zeropad'


# ------------------------------------------------------------------------------------------------ GPU: ops
def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).float()


UP_SHAPES = [(2, 128, 15, 20), (2, 128, 30, 40), (2, 128, 60, 80), (1, 40, 240, 320),
             (2, 3, 1, 1), (2, 5, 1, 4), (3, 4, 3, 5), (2, 6, 5, 3), (1, 7, 5, 1)]


def _ref_up(x, mode, w=None, b=None):
    size = (2 * x.shape[2], 2 * x.shape[3])
    if mode == 'bilinear':
        return F.interpolate(x, size, mode='bilinear', align_corners=False)
    y = F.interpolate(x, size, mode='nearest')
    if mode == 'nearest':
        return y
    return F.conv2d(F.pad(y, (1, 1, 1, 1), mode='replicate'), w, b, 1, 0, groups=x.shape[1])


def _run_twice(fn, inputs, gy):
    """fn on the GPU twice: outputs and every gradient, both runs (the backward must be bitwise reproducible)."""
    res = []
    for _ in range(2):
        xs = [t.cuda().requires_grad_(True) if t is not None else None for t in inputs]
        y = fn(*xs)
        y.backward(gy.cuda())
        res.append((y.detach(), [t.grad.clone() if t is not None else None for t in xs]))
    for a, b in zip(res[0][1], res[1][1]):
        if a is not None:
            assert torch.equal(a, b), 'backward is not bitwise reproducible'
    return res[0]


@pytest.mark.gpu
@pytest.mark.parametrize('shape', UP_SHAPES)
@pytest.mark.parametrize('mode', ['nearest', 'bilinear', 'learned-3x3'])
@pytest.mark.parametrize('with_skip', [False, True])
def test_upsample2x_modes(shape, mode, with_skip):
    from dynmm_amd import ops
    N, C, H, W = shape
    x = rnd(*shape, seed=1)
    w, b = rnd(C, 1, 3, 3, seed=2, scale=0.3), rnd(C, seed=3, scale=0.1)
    skip = rnd(N, C, 2 * H, 2 * W, seed=4) if with_skip else None
    learned = mode == 'learned-3x3'
    ref_in = [t.double().requires_grad_(True) if t is not None else None
              for t in (x, w if learned else None, b if learned else None, skip)]
    ref = _ref_up(ref_in[0], mode, ref_in[1], ref_in[2])
    if with_skip:
        ref = ref + ref_in[3]
    gy = rnd(*ref.shape, seed=5)
    ref.backward(gy.double())

    if learned:
        def fn(xg, wg, bg, sg):
            return ops.upsample2x_dw3x3(xg, wg, bg, sg, border='replicate')
    else:
        def fn(xg, wg, bg, sg):
            return ops.upsample2x(xg, mode, sg)
    y, grads = _run_twice(fn, [x, w if learned else None, b if learned else None, skip], gy)
    assert rel(y, ref) < TOL
    for a, r, name in zip(grads, ref_in, ('dx', 'dw', 'db', 'dskip')):
        if r is not None:
            assert rel(a, r.grad) < GTOL, name


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(2, 128, 15, 20), (1, 3, 5, 7)])
def test_learned_zeropad_is_unchanged_by_the_border_argument(shape):
    from dynmm_amd import ops
    N, C, H, W = shape
    x, w, b = rnd(*shape, seed=1).cuda(), rnd(C, 1, 3, 3, seed=2).cuda(), rnd(C, seed=3).cuda()
    assert torch.equal(ops.upsample2x_dw3x3(x, w, b), ops.upsample2x_dw3x3(x, w, b, border='zero'))


@pytest.mark.gpu
@pytest.mark.parametrize('grid,hw', [((b, b), (15, 20)) for b in (1, 2, 4, 5, 8)] +
                         [((2 * b, 2 * b), (30, 40)) for b in (1, 2, 4, 5, 8)] + [((1, 3), (5, 1)), ((3, 2), (3, 5))])
def test_bilinear_resize_concat(grid, hw):
    check_bilinear_resize_concat(grid, hw)


def check_bilinear_resize_concat(grid, hw, N=2, C0=16, C1=8):
    from dynmm_amd import ops
    (hb, wb), (H, W) = grid, hw
    x, y1, y2 = rnd(N, C0, H, W, seed=1), rnd(N, C1, hb, wb, seed=2), rnd(N, C1, 1, 1, seed=3)
    refs = [t.double().requires_grad_(True) for t in (x, y1, y2)]
    ref = torch.cat([refs[0]] + [F.interpolate(t, (H, W), mode='bilinear', align_corners=False) for t in refs[1:]], 1)
    gy = rnd(*ref.shape, seed=5)
    ref.backward(gy.double())
    out, grads = _run_twice(lambda a, b, c: ops.resize_concat(a, b, c, mode='bilinear'), [x, y1, y2], gy)
    assert rel(out, ref) < TOL
    for a, r in zip(grads, refs):
        assert rel(a, r.grad) < GTOL
    near = ops.resize_concat(x.cuda(), y1.cuda(), mode='nearest')
    assert torch.equal(near, ops.nearest_concat(x.cuda(), y1.cuda()))


# ------------------------------------------------------------------------------------------------ GPU: modules
class Wrap(torch.nn.Module):
    """m(*inputs) for a decoder (module) whose skip inputs are None with encoder_decoder_fusion 'None' (they get no
    gradient, so they are not inputs of the test)."""

    def __init__(self, m, as_list):
        super().__init__()
        self.m, self.as_list = m, as_list

    def forward(self, *xs):
        xs = list(xs) + [None] * ((4 if self.as_list else 2) - len(xs))
        return self.m(xs) if self.as_list else self.m(*xs)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['nearest', 'bilinear', 'learned-3x3'])
@pytest.mark.parametrize('fusion', ['add', 'None'])
def test_decoder_module_modes(mode, fusion):
    from tests.test_hip_blocks import rnd as brnd, run_pair
    from dynmm_amd.nn.decoder import DecoderModule
    m = DecoderModule(128, 128, 1, 40, upsampling_mode=mode, encoder_decoder_fusion=fusion)
    ins = [brnd(2, 128, 12, 16, seed=0), brnd(2, 128, 24, 32, seed=5)][:2 if fusion == 'add' else 1]
    run_pair(Wrap(m, False), lambda sd, x, *rest: DO.decoder_module(sd, 'm.m', x, rest[0] if len(rest) > 1 else None,
                                                                    rest[-1], 1, mode, fusion), ins)


@pytest.mark.gpu
@pytest.mark.parametrize('mode,fusion', [('bilinear', 'None'), ('nearest', 'add'), ('learned-3x3', 'add')])
def test_decoder_modes(mode, fusion):
    from tests.test_hip_blocks import rnd as brnd, run_pair
    from dynmm_amd.nn.decoder import Decoder
    m = Decoder(128, [128, 128, 128], [1, 1, 1], 40, upsampling_mode=mode, encoder_decoder_fusion=fusion)
    n = 2
    ins = [brnd(n, 128, 3, 4, seed=1), brnd(n, 128, 6, 8, seed=2), brnd(n, 128, 12, 16, seed=3),
           brnd(n, 128, 24, 32, seed=4)][:4 if fusion == 'add' else 1]

    def ref(sd, *args):
        xs, tr = list(args[:-1]), args[-1]
        xs = xs + [None] * (4 - len(xs))
        return DO.decoder(sd, 'm.m', xs, tr, [1, 1, 1], mode, fusion)
    run_pair(Wrap(m, True), ref, ins)


@pytest.mark.gpu
def test_pyramid_pooling_bilinear():
    from tests.test_hip_blocks import rnd as brnd, run_pair
    from dynmm_amd.nn.context import PyramidPoolingModule
    run_pair(PyramidPoolingModule(512, 128, upsampling_mode='bilinear'),
             lambda sd, x, tr: DO.pyramid_pooling(sd, 'm', x, tr, (1, 5), 'bilinear'), [brnd(3, 512, 3, 4)])


@pytest.mark.gpu
@pytest.mark.parametrize('mult', [1, 2])
@pytest.mark.parametrize('bins,mode', [((1, 5), 'bilinear'), ((1, 2, 4, 8), 'bilinear'), ((1, 5), 'nearest')])
def test_adaptive_pyramid_pooling(mult, bins, mode):
    from tests.test_hip_blocks import rnd as brnd, run_pair
    from dynmm_amd.nn.context import AdaptivePyramidPoolingModule
    size = (8, 10)
    run_pair(AdaptivePyramidPoolingModule(512, 128, size, bins, mode),
             lambda sd, x, tr: DO.adaptive_pyramid_pooling(sd, 'm', x, tr, bins, size, mode),
             [brnd(2, 512, size[0] * mult, size[1] * mult)])


# ------------------------------------------------------------------------------------------------ GPU: networks
@pytest.mark.gpu
def test_networks_match_reference_fixture(golden_dir):
    g = fixture(golden_dir)
    h, w, n, stride = [int(v) for v in g['meta']]
    rgb, depth = synth.synth_inputs(n, h, w, seed=1234, device='cuda')
    for name in (str(c) for c in g['out_combos']):
        tag = f'out/{name}'
        m = make('gate', **parse(name))
        synth.fill_state_dict(m.state_dict(), seed=0)
        m = m.cuda().eval()
        m.baseline = True
        with torch.no_grad():
            out = m(rgb, depth, test=True).cpu()
        assert Hh.rel_err(out[:, :, ::stride, ::stride], g[f'{tag}/eval_strided']) < LOGIT_TOL, name
        assert Hh.rel_err(out.sum(dim=(2, 3)), g[f'{tag}/eval_csum']) < 1e-3, name
        m = make('gate', **parse(name))
        synth.fill_state_dict(m.state_dict(), seed=0)
        m = m.cuda().train()
        m.temp, m.hard_gate = 0.8, False
        outs, lf = m(rgb, depth)
        loss = Hh.train_loss(outs, lf)
        loss.backward()
        assert Hh.rel_err(outs[0].detach().cpu()[:, :, ::stride, ::stride], g[f'{tag}/train_strided']) < TRAIN_OUT_TOL, name
        for i, o in enumerate(outs[1:]):
            assert Hh.rel_err(o.detach().cpu()[:, :, ::2, ::2], g[f'{tag}/train_side{i}']) < TRAIN_OUT_TOL, (name, i)
        ref = float(g[f'{tag}/train_loss'])
        assert abs(loss.item() - ref) < TRAIN_OUT_TOL * max(1.0, abs(ref)), name


@pytest.mark.gpu
def test_one_train_step_matches_reference(golden_dir):
    """One SGD-Nesterov step through engine.TrainStep in bilinear + appm + None: the decoder does not defer its tail, the
    losses come from the materialised logits."""
    from dynmm_amd import engine
    g = fixture(golden_dir)
    h, w, n, stride = [int(v) for v in g['meta']]
    lr, wd, mom, ratio, budget, temp = [float(v) for v in g['step/hyper']]
    m = make('gate', **parse(str(g['step/combo'])))
    synth.fill_state_dict(m.state_dict(), 0)
    m = m.cuda().train()
    m.temp, m.hard_gate = temp, False
    rgb, depth = synth.synth_inputs(n, h, w, seed=1234, device='cuda')
    labels = [synth.synth_labels(n, h // s, w // s, seed=300 + s, device='cuda') for s in (1, 8, 16, 32)]
    step = engine.TrainStep(m, g['step/cw'], lr=lr, momentum=mom, weight_decay=wd, loss_ratio=ratio,
                            flop_budget=budget)
    out = step(rgb, depth, labels)
    losses = out['losses'].cpu().numpy()
    assert np.allclose(losses, g['step/losses'], rtol=TRAIN_OUT_TOL), (losses, g['step/losses'])
    assert abs(out['loss_flop'].item() - float(g['step/loss_flop'])) < TRAIN_OUT_TOL
    assert abs(out['total'].item() - float(g['step/total'])) < TRAIN_OUT_TOL * float(g['step/total'])
    # the update itself: parameter norms at the bands of test_engine.test_two_train_steps_match_reference (one fp32 gradient
    # of an ill-conditioned batch-2 step; the SE excitation biases are the most sensitive tensors)
    sd = m.state_dict()
    names = [str(k) for k in g['step/param_names']]
    norms = np.array([sd[k].double().norm().item() for k in names])
    rel_ = np.abs(norms - g['step/param_norms']) / np.maximum(g['step/param_norms'], 1e-3)
    tol = np.array([6e-2 if 'se_layer' in k else 1e-2 for k in names])
    bad = np.nonzero(rel_ >= tol)[0]
    assert bad.size == 0, [(names[i], norms[i], g['step/param_norms'][i], rel_[i]) for i in bad[:8]]


FLAGS = dict(upsampling='bilinear', context_module='appm', encoder_decoder_fusion='None')


@pytest.mark.gpu
def test_infer_step_replay_and_compaction_in_a_non_default_mode():
    from dynmm_amd import engine
    h, w, n = 96, 128, 6
    m = make('gate', **FLAGS)
    synth.fill_state_dict(m.state_dict(), seed=2)
    m = m.cuda().eval()
    batches = [synth.synth_inputs(n, h, w, seed=900 + i, device='cuda') for i in range(3)]
    step = engine.InferStep(m, capture_after=2)
    m.baseline = True
    for rgb, depth in batches + batches[:1]:
        with torch.no_grad():
            ref = m(rgb, depth, True).clone()
        assert torch.equal(step(rgb, depth), ref)
    assert step.launch == 'hipGraph replay', step.launch
    # hard-gate compaction (as test_hard_gate_compaction_is_exact): branch-sorted depth stages == the dense forward
    m.baseline = False
    m.ini_stage = True
    m.ini_branches = [1, 4, 0, 3, 2, 4]
    rgb, depth = batches[0]
    with torch.no_grad():
        m.compact = True
        out_c = m(rgb, depth, test=True)
        assert m.last_stage_batch == [5, 4, 3, 2]
        m.compact = False
        out_d = m(rgb, depth, test=True)
    assert Hh.rel_err(out_c.cpu(), out_d.cpu()) < 1e-5

"""ESANetOneModality — the RGB-only / depth-only networks of FusionDynMM/src/models/model_one_modality.py (what
src/build_model.py:119-141 returns for --modality rgb | depth) — and the single-input squeeze-and-excitation kernels they run
on (csrc/se_scale.hip, dynmm_se1_coeff_* in csrc/gate_se.hip; ops.se_scale / ops.se_scale_pool).

CPU: the build's state_dict and the tests-side float64 oracle (tests/one_modality_oracle.py) against the fixture the REFERENCE
produced (tests/golden/make_one_modality_goldens.py); the builders and the import surface.
GPU: the operators against float64 on the CPU, the pool fusion against the composition bit by bit, determinism, the model
against the fixture, one optimisation step, hipGraph replay, the drivers."""
import functools
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynmm_amd import synth
from oracle import dynmm_oracle as O
from tests import helpers as Hh
from tests import one_modality_oracle as OM
from tests.activation_oracle import act_fn

TOL, GTOL = 2e-5, 2e-4                   # tests/test_hip_ops.py, tests/test_benchmark_geometry.py
LOGIT_TOL, TRAIN_OUT_TOL = 2e-4, 1e-3    # tests/test_hip_model.py
FULL_GRAD_NORM_TOL, FULL_GRAD_COS_TOL = 0.02, 0.999     # tests/test_hip_model.py: the equal-decisions bars

P = dict(encoder='resnet34', encoder_block='NonBottleneck1D', channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3],
         pretrained_on_imagenet=False)
CONFIGS = {          # tests/golden/make_one_modality_goldens.py
    'rgb': dict(P, input_channels=3, weighting_in_encoder='SE-add', upsampling='learned-3x3-zeropad'),
    'depth': dict(P, input_channels=1, weighting_in_encoder='SE-add', upsampling='learned-3x3-zeropad'),
    'plain': dict(P, input_channels=3, weighting_in_encoder='None', upsampling='bilinear'),
}
N_ENTRIES = {'rgb': 560, 'depth': 560, 'plain': 530}
CFG = O.Config(encoder_block='NonBottleneck1D')
FULL_GRADS = ('encoder.conv1.weight', 'se_layer0.fc.0.weight', 'se_layer3.fc.2.bias')


def make(cfg, h=96, w=128, seed=0):
    from dynmm_amd.nn.esanet import ESANetOneModality
    m = ESANetOneModality(height=h, width=w, num_classes=40, **CONFIGS[cfg])
    if seed is not None:
        synth.fill_state_dict(m.state_dict(), seed=seed)
    return m


def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'one_modality_96x128.npz'))


def inputs(g, cfg, device='cpu'):
    h, w, n, _ = [int(v) for v in g['meta']]
    rgb, depth = synth.synth_inputs(n, h, w, seed=1234, device=device)
    return rgb, depth, (rgb if CONFIGS[cfg]['input_channels'] == 3 else depth)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_state_dict_matches_reference(golden_dir, cfg):
    g = fixture(golden_dir)
    m = make(cfg, seed=None)
    sd = m.state_dict()
    assert len(sd) == N_ENTRIES[cfg]
    assert list(sd.keys()) == [str(k) for k in g[f'{cfg}/keys']]         # encoder, se_layer0..4, skip_layer1..3, context, decoder
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f'{cfg}/shapes']]
    assert [str(v.dtype) for v in sd.values()] == [str(s) for s in g[f'{cfg}/dtypes']]
    assert m.modality == ('depth' if cfg == 'depth' else 'rgb')


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_oracle_matches_reference_fixture(golden_dir, cfg):
    """the float64 restatement against the reference's fp32 run, at test_esanet_oracle_matches_reference_fixture's bars"""
    g = fixture(golden_dir)
    stride = int(g['meta'][3])
    image = inputs(g, cfg)[2].double()
    kw = dict(weighting=CONFIGS[cfg]['weighting_in_encoder'], upsampling=CONFIGS[cfg]['upsampling'])
    sd = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in make(cfg).state_dict().items()}
    with torch.no_grad():
        out = OM.forward(sd, image, CFG, **kw)
    assert Hh.rel_err(out[:, :, ::stride, ::stride], g[f'{cfg}/eval/strided']) < 2e-5
    assert Hh.rel_err(out.sum(dim=(2, 3)), g[f'{cfg}/eval/csum']) < 1e-4
    params = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and 'running_' not in k}
    outs = OM.forward(sd, image, CFG, training=True, **kw)
    assert isinstance(outs, tuple) and len(outs) == 4                           # model.py:306-308
    loss = Hh.train_loss(outs, torch.zeros(()))
    loss.backward()
    ref = float(g[f'{cfg}/train/loss'])
    assert abs(loss.item() - ref) < 1e-4 * max(1.0, abs(ref))
    assert Hh.rel_err(outs[0].detach()[:, :, ::stride, ::stride], g[f'{cfg}/train/strided']) < 2e-4
    names = [str(s) for s in g[f'{cfg}/train/grad_names']]
    norms = np.array([params[k].grad.norm().item() for k in names])
    ref = g[f'{cfg}/train/grad_norms']
    assert np.all(np.abs(norms - ref) <= 0.05 * np.maximum(ref, 1e-2 * ref.max()))


def _args(**kw):
    from dynmm_amd.src.args import ArgumentParserRGBDSegmentation
    p = ArgumentParserRGBDSegmentation()
    p.set_common_args()
    a = p.parse_args(['--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D', '--decoder_channels_mode', 'constant',
                      '--height', '96', '--width', '128'])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_builders_and_import_surface(tmp_path):
    from dynmm_amd.nn.esanet import ESANetOneModality
    from dynmm_amd.src.build_model import build_for_args, build_model, build_one_modality
    from dynmm_amd.src.models import model_one_modality
    assert model_one_modality.ESANetOneModality is ESANetOneModality
    for modality, ch in (('rgb', 3), ('depth', 1)):
        model, _ = build_one_modality(_args(pretrained_on_imagenet=False, modality=modality), 40)
        assert type(model) is ESANetOneModality and model.modality == modality and model.input_channels == ch
        assert model.encoder.conv1.weight.shape[1] == ch and len(model.state_dict()) == 560       # --fuse_depth_in_rgb_encoder SE-add
        assert type(build_for_args(_args(pretrained_on_imagenet=False, modality=modality), 40)[0]) is ESANetOneModality
    model, _ = build_one_modality(_args(pretrained_on_imagenet=False, modality='rgb', fuse_depth_in_rgb_encoder='add'), 40)
    assert len(model.state_dict()) == 560 - 5 * 4 and isinstance(model.se_layer2, torch.nn.Identity)    # no SE: 5 x (W1, b1, W2, b2)
    with pytest.raises(FileNotFoundError):                                       # ImageNet weights asked for, none on disk
        build_one_modality(_args(pretrained_on_imagenet=True, modality='depth', pretrained_dir=str(tmp_path / 'nowhere')), 40)
    with pytest.raises(NotImplementedError, match='build_one_modality'):         # build_model itself still refuses
        build_model(_args(pretrained_on_imagenet=False, modality='rgb'), 40)
    with pytest.raises(ValueError):
        build_one_modality(_args(pretrained_on_imagenet=False), 40)              # --modality rgbd
    assert type(build_for_args(_args(pretrained_on_imagenet=False), 40)[0]).__name__ == 'ESANet'


def test_squeeze_and_excitation_module_has_a_forward():
    from dynmm_amd.lib import DynmmHipError
    from dynmm_amd.nn.fusion import SqueezeAndExcitation
    m = SqueezeAndExcitation(32)
    assert 'forward' in SqueezeAndExcitation.__dict__ and [tuple(p.shape) for p in m.mlp_params()] == \
        [(2, 32, 1, 1), (2,), (32, 2, 1, 1), (32,)]
    if not torch.cuda.is_available():
        with pytest.raises(DynmmHipError):                                      # no eager fall-back
            m(torch.zeros(1, 32, 4, 4))


# ------------------------------------------------------------------------------------------------ GPU: operators
# (N, C, H, W): hidden width 1 on the vector path | the scalar path, odd pooled sizes, the pool fusion's fall-back | plane and
# pooled plane both above kChunk = 8192 (second chunk live) | several planes and hidden units
SHAPES = [(2, 16, 6, 8), (3, 32, 5, 7), (1, 16, 192, 176), (2, 64, 24, 32)]
ACTS = ['relu', 'swish', 'hswish']


def se_params(C, seed):
    r = np.random.Generator(np.random.PCG64(seed))
    hd = C // 16
    return [torch.from_numpy(r.standard_normal(s).astype(np.float32) * sc)
            for s, sc in (((hd, C, 1, 1), 0.5), ((hd,), 0.5), ((C, hd, 1, 1), 1.0), ((C,), 0.5))]


@functools.lru_cache(maxsize=None)
def case(shape, act, pool, variant=''):
    """inputs, parameters and the float64 CPU results of one operator case (computed once, shared by the tests that read it).
    variant 'zero': the second-layer bias of channel 1 at -200, so that g[:, 1] == 0 exactly; 'relu': a post-ReLU input."""
    N, C, H, W = shape
    r = np.random.Generator(np.random.PCG64([7, N, C, H, W]))
    x = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
    if variant == 'relu':
        x = x.clamp_min(0)                                       # about half the map is exactly zero: ties in most windows
    params = se_params(C, 11 + C)
    if variant == 'zero':
        params[3][1] = -200.0
    xd = x.double().requires_grad_(True)
    pd = [p.double().requires_grad_(True) for p in params]
    y = OM.squeeze_excite(pd, xd, act_fn(act))
    if pool:
        y = F.max_pool2d(y, 3, 2, 1)
    gy = torch.from_numpy(r.standard_normal(tuple(y.shape)).astype(np.float32))
    grads = torch.autograd.grad(y, [xd] + pd, gy.double())
    return x, params, gy, y.detach(), [t.detach() for t in grads]


def run_hip(x, params, gy, act, pool):
    from dynmm_amd import ops
    xh = x.cuda().requires_grad_(True)
    ph = [p.cuda().requires_grad_(True) for p in params]
    y = (ops.se_scale_pool if pool else ops.se_scale)(xh, ph, act)
    grads = torch.autograd.grad(y, [xh] + ph, gy.cuda())
    return y.detach(), list(grads)


def check_case(shape, act, pool, variant=''):
    x, params, gy, y_ref, g_ref = case(shape, act, pool, variant)
    y, grads = run_hip(x, params, gy, act, pool)
    e = Hh.rel_err(y.cpu(), y_ref)
    print(f'{shape} {act} pool={pool} {variant}: forward {e:.2e}', end='')
    errs = [Hh.rel_err(a.cpu(), b) for a, b in zip(grads, g_ref)]
    print(' gradients (x, W1, b1, W2, b2) ' + ' '.join(f'{v:.2e}' for v in errs))
    assert e < TOL
    assert max(errs) < GTOL, errs
    return y, grads


@pytest.mark.gpu
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape', SHAPES)
def test_se_scale_matches_float64(shape, act):
    check_case(shape, act, pool=False)


@pytest.mark.gpu
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape', SHAPES)
def test_se_scale_pool_matches_float64(shape, act):
    from dynmm_amd import ops
    x = torch.zeros(shape, device='cuda')
    assert ops.se_scale_pool_supported(x) == (shape[2] % 2 == 0 and shape[3] % 8 == 0)     # (3, 32, 5, 7): composed
    check_case(shape, act, pool=True)


@pytest.mark.gpu
@pytest.mark.parametrize('pool', [False, True])
def test_a_scale_of_exactly_zero(pool):
    x, params, gy, y_ref, _ = case((2, 64, 24, 32), 'relu', pool, 'zero')
    assert y_ref[:, 1].abs().max() < 1e-80                      # float64: sigmoid(-200 + ...) ~ 1e-87 ...
    y, grads = check_case((2, 64, 24, 32), 'relu', pool, 'zero')
    # ... float32: exp(200) overflows, the scale is 0 exactly — the plane is all zeros (the pool: decided by the tie rule alone)
    assert torch.all(y[:, 1] == 0) and all(torch.isfinite(t).all() for t in grads)


def _codes(y):
    """the arg-max codes an operator's node saved for its backward"""
    (idx,) = [t for t in y.grad_fn.saved_tensors if t.dtype == torch.int8]
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['', 'relu'])
@pytest.mark.parametrize('shape', [s for s in SHAPES if s[2] % 2 == 0 and s[3] % 8 == 0])
def test_pool_fusion_equals_the_composition(shape, variant):
    """se_scale_pool against max_pool_3x3_s2(se_scale(x)): values and arg-max codes bit for bit (post-ReLU input: the tie rule
    decides most windows), gradients at the operator bars."""
    from dynmm_amd import ops
    x, params, gy, _, _ = case(shape, 'relu', True, variant)
    outs = []
    for fused in (True, False):
        xh = x.cuda().requires_grad_(True)
        ph = [p.cuda().requires_grad_(True) for p in params]
        assert ops.se_scale_pool_supported(xh)
        y = ops.se_scale_pool(xh, ph) if fused else ops.max_pool_3x3_s2(ops.se_scale(xh, ph))
        outs.append((y, _codes(y), torch.autograd.grad(y, [xh] + ph, gy.cuda())))
    (y_f, c_f, g_f), (y_c, c_c, g_c) = outs
    assert type(y_f.grad_fn).__name__.startswith('_SEScalePool') and torch.equal(y_f, y_c) and torch.equal(c_f, c_c)
    if variant == 'relu':
        assert (y_f == 0).float().mean() > 0.001               # windows of zeros only: decided by the tie rule
    for a, b in zip(g_f, g_c):
        assert Hh.rel_err(a.cpu(), b.cpu()) < GTOL


@pytest.mark.gpu
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_backward_is_deterministic(shape, pool):
    x, params, gy, _, _ = case(shape, 'relu', pool)
    (y0, g0), (y1, g1) = run_hip(x, params, gy, 'relu', pool), run_hip(x, params, gy, 'relu', pool)
    assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


@pytest.mark.gpu
def test_inference_in_place_and_the_module_forward():
    from dynmm_amd import ops
    from dynmm_amd.nn.fusion import SqueezeAndExcitation
    x, params, _, y_ref, _ = case((2, 64, 24, 32), 'swish', False)
    m = SqueezeAndExcitation(64, activation='swish').cuda()
    for dst, src in zip(m.mlp_params(), params):
        dst.data.copy_(src)
    xh = x.cuda()
    y = m(xh)
    assert Hh.rel_err(y.detach().cpu(), y_ref) < TOL and y.requires_grad
    with torch.no_grad():
        z = ops.se_scale(xh, m.mlp_params(), 'swish', inplace=True)
    assert z.data_ptr() == xh.data_ptr() and torch.equal(z, y.detach())


# ------------------------------------------------------------------------------------------------ GPU: the model
@pytest.mark.gpu
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_hip_matches_reference_fixture(golden_dir, cfg):
    g = fixture(golden_dir)
    stride = int(g['meta'][3])
    rgb, depth, image = inputs(g, cfg, 'cuda')
    m = make(cfg).cuda().eval()
    with torch.no_grad():
        out = m(image).cpu()
        two = m(rgb, depth, test=True).cpu()                    # the callers' protocol: its own modality out of the two
    assert torch.equal(out, two)
    assert Hh.rel_err(out[:, :, ::stride, ::stride], g[f'{cfg}/eval/strided']) < LOGIT_TOL
    assert Hh.rel_err(out.sum(dim=(2, 3)), g[f'{cfg}/eval/csum']) < 1e-3
    m = make(cfg).cuda().train()
    outs = m(image)
    assert isinstance(outs, tuple) and len(outs) == 4
    loss = Hh.train_loss(outs, torch.zeros((), device='cuda'))
    loss.backward()
    ref = float(g[f'{cfg}/train/loss'])
    assert abs(loss.item() - ref) < TRAIN_OUT_TOL * max(1.0, abs(ref))
    assert Hh.rel_err(outs[0].detach().cpu()[:, :, ::stride, ::stride], g[f'{cfg}/train/strided']) < TRAIN_OUT_TOL
    for i, o in enumerate(outs[1:]):
        assert Hh.rel_err(o.detach().cpu(), g[f'{cfg}/train/side{i}']) < TRAIN_OUT_TOL
    params = dict(m.named_parameters())
    names = [str(s) for s in g[f'{cfg}/train/grad_names']]
    assert list(params) == names and all(p.grad is not None for p in params.values())
    norms = np.array([params[k].grad.norm().item() for k in names])
    ref = g[f'{cfg}/train/grad_norms']
    bad = np.abs(norms - ref) > 0.2 * np.maximum(ref, 1e-2 * ref.max())        # fp32 conditioning: see tests/test_hip_model.py
    assert not bad.any(), [(names[i], norms[i], ref[i]) for i in np.nonzero(bad)[0][:8]]
    # the stored full gradients: norm and direction
    for name in FULL_GRADS:
        if f'{cfg}/train/grad:{name}' not in g.files:
            assert cfg == 'plain' and name.startswith('se_layer')
            continue
        a = params[name].grad.detach().double().cpu().flatten()
        b = torch.from_numpy(g[f'{cfg}/train/grad:{name}']).double().flatten()
        dev = abs(a.norm().item() - b.norm().item()) / b.norm().item()
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()))
        print(f'{cfg} {name}: gradient norm deviation {dev:.4f}, cosine {cos:.6f}')
        assert dev < FULL_GRAD_NORM_TOL and cos > FULL_GRAD_COS_TOL, (name, dev, cos)


@pytest.mark.gpu
@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_one_train_step_matches_reference(golden_dir, cfg, use_graph):
    """One SGD-Nesterov step through engine.TrainStep (train_steps_fixture's recipe), at tests/test_decoder_modes.py's step/* bars."""
    from dynmm_amd import engine
    g = fixture(golden_dir)
    h, w, n, _ = [int(v) for v in g['meta']]
    lr, wd, mom = [float(v) for v in g['step/hyper']]
    m = make(cfg).cuda().train()
    rgb, depth, _ = inputs(g, cfg, 'cuda')
    labels = [synth.synth_labels(n, h // s, w // s, seed=300 + s, device='cuda') for s in (1, 8, 16, 32)]
    step = engine.TrainStep(m, g['step/cw'], lr=lr, momentum=mom, weight_decay=wd, use_graph=use_graph)
    out = step(rgb, depth, labels)
    losses = out['losses'].cpu().numpy()
    assert np.allclose(losses, g[f'{cfg}/step/losses'], rtol=TRAIN_OUT_TOL), (losses, g[f'{cfg}/step/losses'])
    assert out['loss_flop'].item() == 0.0
    assert abs(out['total'].item() - float(g[f'{cfg}/step/total'])) < TRAIN_OUT_TOL * float(g[f'{cfg}/step/total'])
    sd = m.state_dict()
    names = [str(k) for k in g[f'{cfg}/step/param_names']]
    norms = np.array([sd[k].double().norm().item() for k in names])
    ref = g[f'{cfg}/step/param_norms']
    rel_ = np.abs(norms - ref) / np.maximum(ref, 1e-3)
    tol = np.array([6e-2 if 'se_layer' in k else 1e-2 for k in names])
    bad = np.nonzero(rel_ >= tol)[0]
    assert bad.size == 0, [(names[i], norms[i], ref[i], rel_[i]) for i in bad[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize('cfg', ['depth', 'plain'])
def test_infer_step_replays_one_graph(cfg):
    from dynmm_amd import engine
    h, w, n = 96, 128, 2
    m = make(cfg, seed=2).cuda().eval()
    batches = [synth.synth_inputs(n, h, w, seed=900 + i, device='cuda') for i in range(2)]
    step = engine.InferStep(m)
    for rgb, depth in batches + batches[:1]:
        with torch.no_grad():
            ref = m(rgb, depth, True).clone()
        assert torch.equal(step(rgb, depth), ref)
    assert step.launch == 'hipGraph replay' and step.replays['eager'] == 0, (step.launch, step.replays)
    # engine.evaluate leaves a `hard_gate` attribute on the model: still one graph
    label = synth.synth_labels(n, h, w, seed=6, device='cuda')
    miou, cm = engine.evaluate(m, [batches[0] + (label,)], num_classes=40, infer_step=step)
    assert hasattr(m, 'hard_gate') and np.isfinite(miou) and int(cm.sum()) == int((label > 0).sum())
    rgb, depth = batches[1]
    with torch.no_grad():
        ref = m(rgb, depth, True).clone()
    assert torch.equal(step(rgb, depth), ref)
    assert step.launch == 'hipGraph replay' and step.replays['eager'] == 0, (step.launch, step.replays)


@pytest.mark.gpu
def test_evaluate_and_the_drivers(tmp_path):
    from dynmm_amd import engine, eval as E, train
    m = make('rgb').cuda().eval()
    rgb, depth = synth.synth_inputs(2, 96, 128, seed=5, device='cuda')
    label = synth.synth_labels(2, 96, 128, seed=6, device='cuda')
    miou, cm = engine.evaluate(m, [(rgb, depth, label)], num_classes=40)
    assert np.isfinite(miou) and int(cm.sum()) == int((label > 0).sum())
    common = ['--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D', '--decoder_channels_mode', 'constant',
              '--dataset', 'synthetic', '--height', '96', '--width', '128', '--batch_size', '4', '--synthetic_samples', '8',
              '--modality', 'depth']
    logs = train.train_main(common + ['--no_imagenet_pretraining', '--epochs', '1', '--debug', '--results_dir', str(tmp_path)])
    assert len(logs) == 1 and np.isfinite(logs[0]['loss_train_total']) and np.isfinite(logs[0]['mIoU_test'])
    (ckpt,) = glob.glob(str(tmp_path / 'synthetic' / 'checkpoints_*' / 'ckpt_epoch_*.pth'))
    sd = torch.load(ckpt, map_location='cpu')['state_dict']
    assert len(sd) == 560 and sd['encoder.conv1.weight'].shape[1] == 1
    results = E.main(common + ['--ckpt_path', ckpt])
    assert len(results) >= 1 and all(np.isfinite(r) for r in results)

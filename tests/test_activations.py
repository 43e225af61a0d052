"""Swish / Hswish (`--activation`) on the HIP path: the pointwise kernels, BatchNorm and the SE excitations through the
PRE-activation, the blocks, the three networks and their callers — against tests/activation_oracle.py (the reference's own
functions with the activation substituted, in float64) and against fixtures made by the reference itself
(tests/golden/make_activation_goldens.py -> activations_{swish,hswish}_96x128.npz).

Bars (the project's own): op level TOL / GTOL as rel_err against float64; block level 5e-4 on gradients (test_hip_blocks.py);
model level LOGIT_TOL / TRAIN_OUT_TOL (test_hip_model.py).

HSWISH KINK RULE.  Hswish's derivative jumps at z = +-3 (by 1/2 of the upstream gradient): an element whose float32
pre-activation falls on the other side of a kink than its float64 one moves one gradient element by order one, far above GTOL
at these sizes.  Every op- and block-level Hswish gradient case therefore ASSERTS, on the float64 pre-activations of the
restatement, that none lies within 1e-4 of +-3 (`assert_off_kinks`; the seeds were chosen so that it holds) — no element is
excluded from any comparison.  Swish is smooth and needs no such rule."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dynmm_amd import synth
from tests import activation_oracle as AO
from tests import helpers as Hh

TOL, GTOL = 2e-5, 2e-4
BLOCK_GTOL = 5e-4
LOGIT_TOL, TRAIN_OUT_TOL = 2e-4, 1e-3
SMOOTH = ('swish', 'hswish')
NETS = ('gate', 'skip', 'esanet')
GRID = [-3.0, 3.0, 0.0, 2.999999, -2.999999, 3.000001, -3.000001, -20.0, 20.0, -90.0]
H, W, N = 96, 128, 2
COMMON = dict(height=H, width=W, num_classes=40, encoder_rgb='resnet34', encoder_depth='resnet34',
              encoder_block='NonBottleneck1D', channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3],
              fuse_depth_in_rgb_encoder='SE-add', upsampling='learned-3x3-zeropad')
gpu = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def rel(a, b):
    return Hh.rel_err(a.detach().cpu(), b.detach().cpu())


def assert_off_kinks(preacts, act):
    """the Hswish kink rule of the module docstring"""
    if act != 'hswish':
        return
    d = min(((z.abs() - 3).abs().min().item() if z.numel() else 1.0) for z in preacts)
    assert d > 1e-4, f'a float64 pre-activation lies {d:.2e} from a kink of Hswish: choose another seed'


def golden(golden_dir, act):
    return np.load(os.path.join(golden_dir, f'activations_{act}_96x128.npz'))


def build_net(kind, act, **kw):
    from dynmm_amd.nn.esanet import ESANet
    from dynmm_amd.nn.net import SkipGateESANet
    from dynmm_amd.nn.net_skip import SkipESANet
    cls = {'gate': SkipGateESANet, 'skip': SkipESANet, 'esanet': ESANet}[kind]
    extra = dict(pretrained_on_imagenet=False) if kind == 'esanet' else {}
    m = cls(activation=act, **COMMON, **extra, **kw)
    synth.fill_state_dict(m.state_dict(), seed=0)
    return m


def oracle_sd(m, dtype=torch.float32):
    return {k: (v.detach().clone().cpu().to(dtype) if v.dtype.is_floating_point else v.detach().clone().cpu())
            for k, v in m.state_dict().items()}


def oracle_params(sd):
    return {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and 'running_' not in k}


CFG = Hh.CFGS['P_se']


# =================================================================================================================================
# CPU
# =================================================================================================================================
@pytest.mark.parametrize('kind', NETS)
def test_spellings(kind):
    for spelling, want in (('Swish', 'swish'), ('SiLU', 'swish'), ('HSWISH', 'hswish'), ('relu', 'relu'), ('ReLU', 'relu')):
        m = build_net(kind, spelling)
        assert m.activation == want and m.encoder_rgb.activation == want and m.decoder.decoder_module_1.conv3x3.activation == want
    with pytest.raises(NotImplementedError, match='Only relu, swish and hswish'):
        build_net(kind, 'gelu')


@pytest.mark.parametrize('act', SMOOTH)
def test_build_model_accepts_the_flag(act):
    from dynmm_amd.src.args import ArgumentParserRGBDSegmentation
    from dynmm_amd.src.build_model import build_model
    p = ArgumentParserRGBDSegmentation()
    p.set_common_args()
    for dyn in (['--dynamic', '--global-gate'], ['--dynamic'], []):
        args = p.parse_args(dyn + ['--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D', '--height', '96',
                                   '--width', '128', '--decoder_channels_mode', 'constant', '--nr_decoder_blocks', '1',
                                   '--no_imagenet_pretraining', '--activation', act])
        model, _ = build_model(args, n_classes=40)
        assert model.activation == act and model.encoder_depth.layer3[1].activation == act
        assert model.context_module.final_conv.activation == act


def test_reference_module_names_are_exported():
    from dynmm_amd.src.models import model_utils, resnet
    assert issubclass(model_utils.Swish, torch.nn.Module) and issubclass(model_utils.Hswish, torch.nn.Module)
    assert callable(model_utils.swish)
    enc = resnet.ResNet34(block='NonBottleneck1D', input_channels=1, activation=model_utils.Hswish())
    assert enc.activation == 'hswish' and enc.layer2[0].activation == 'hswish'
    assert resnet.ResNet18(activation=torch.nn.ReLU(inplace=True)).activation == 'relu'


@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('kind', NETS)
def test_state_dict_does_not_depend_on_the_activation(golden_dir, kind, act):
    g = golden(golden_dir, act)
    sd = build_net(kind, act).state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f'{kind}/keys']]
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f'{kind}/shapes']]
    assert list(sd.keys()) == list(build_net(kind, 'relu').state_dict().keys())


def _check_outputs(g, tag, out, tol=1e-6):
    stride = int(g['meta'][3])
    out = out.detach()
    assert Hh.rel_err(out[:, :, ::stride, ::stride], g[f'{tag}/strided']) < tol, tag
    assert Hh.rel_err(out.sum(dim=(2, 3)), g[f'{tag}/csum']) < 10 * tol, tag
    assert Hh.rel_err(out.abs().sum(dim=(2, 3)), g[f'{tag}/cabs']) < 10 * tol, tag


def _check_grad_norms(g, tag, params, tol=1e-5):
    names = [str(s) for s in g[f'{tag}/grad_names']]
    ref = g[f'{tag}/grad_norms']
    got = np.array([0.0 if params[nm].grad is None else params[nm].grad.norm().item() for nm in names])
    # (per entry, relative; entries below 1e-3 of the largest norm — the analytically zero gradients among them — absolutely)
    dev = np.abs(got - ref) / np.maximum(ref, 1e-3 * ref.max())
    assert dev.max() < tol, (tag, names[int(dev.argmax())], dev.max())


def oracle_run(kind, act, sd, rgb, depth, training, mode=None, noise=None, skip_cfg=None):
    """outputs (tuple in training), flop loss or None, gate weight(s) or None"""
    O = AO.oracle(act)
    if kind == 'gate':
        kw = dict(Hh.MODE_KW[mode])
        if training:
            outs, lf = O.forward(sd, rgb, depth, CFG, **kw)
            return outs, lf, None
        det = {}
        out, lf = O.forward(sd, rgb, depth, CFG, detail=det, **kw)
        return out, lf, det['weight']
    if kind == 'skip':
        _, test, hard, temp, rule = skip_cfg
        det = {}
        out = O.forward_skip(sd, rgb, depth, CFG, noise, training=training, test=test, hard_gate=hard, temp=temp,
                             block_rule=rule, detail=det)
        return out, None, det['weights']
    return O.forward_esanet(sd, rgb, depth, CFG, training=training), None, None


def net_cases(g, kind):
    """(tag, training, mode, skip_cfg) of every fixture entry of one network"""
    if kind == 'gate':
        return [(f'gate/{m}', m.startswith('train'), m, None) for m in ('eval_baseline', 'eval_soft', 'eval_hard', 'train_soft')]
    if kind == 'skip':
        out = []
        for m in ('eval_test', 'train_soft'):
            c = [int(v) for v in g[f'skip/{m}/cfg']]
            out.append((f'skip/{m}', bool(c[0]), m, (bool(c[0]), bool(c[1]), bool(c[2]), float(g[f'skip/{m}/temp']), c[3:])))
        return out
    return [('esanet/eval', False, None, None), ('esanet/train', True, None, None)]


def skip_noise(g, tag, dtype=torch.float32):
    return [torch.from_numpy(g[f'{tag}/noise{j}']).to(dtype) for j in range(4)]


@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('kind', NETS)
def test_restatement_reproduces_the_reference_fixtures(golden_dir, kind, act):
    """The float32 restatement on the CPU against every fixture entry: outputs and losses to 1e-6, gradient norms to 1e-5."""
    g = golden(golden_dir, act)
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    for tag, training, mode, scfg in net_cases(g, kind):
        sd = oracle_sd(build_net(kind, act))
        params = oracle_params(sd) if training else None
        noise = skip_noise(g, tag) if kind == 'skip' else None
        with torch.set_grad_enabled(training):
            outs, lf, wgt = oracle_run(kind, act, sd, rgb, depth, training, mode, noise, scfg)
        _check_outputs(g, tag, outs[0] if training else outs)
        if kind == 'gate':
            assert abs(lf.item() - float(g[f'{tag}/loss_flop'])) <= 1e-6 * max(1.0, abs(float(g[f'{tag}/loss_flop'])))
            if not training:
                assert Hh.rel_err(wgt, g[f'{tag}/weight']) < 1e-6
        if kind == 'skip':
            for j in range(4):
                assert Hh.rel_err(wgt[j].detach(), g[f'{tag}/weight{j}']) < 1e-6, (tag, j)
        if training:
            for i, o in enumerate(outs[1:]):
                assert Hh.rel_err(o.detach(), g[f'{tag}/side{i}']) < 1e-6, (tag, i)
            loss = Hh.train_loss(outs, lf if lf is not None else torch.zeros(()))
            loss.backward()
            assert abs(loss.item() - float(g[f'{tag}/loss'])) <= 1e-6 * max(1.0, abs(float(g[f'{tag}/loss'])))
            _check_grad_norms(g, tag, params)


@pytest.mark.parametrize('act', SMOOTH)
def test_derivative_convention_is_torch_autograd(act):
    """The closed form the kernels restate (csrc/common.h act_grad_pre) equals torch autograd in float64 on the value grid — in
    particular 1 at exactly z = 3 and 0 at exactly z = -3 for Hswish (the strict hardtanh mask)."""
    z = torch.tensor(GRID, dtype=torch.float64, requires_grad=True)
    AO.act_fn(act)(z).sum().backward()
    got = AO.act_grad(z.detach(), act)
    assert torch.allclose(got, z.grad, rtol=1e-12, atol=1e-300), (got, z.grad)
    if act == 'hswish':
        assert got[0].item() == 0.0 and got[1].item() == 1.0
        ref = F.hardswish(z.detach().clone().requires_grad_(True))
        assert torch.allclose(AO.act_fn(act)(z.detach()), ref.detach(), rtol=1e-12, atol=1e-300)
    assert torch.isfinite(AO.act_fn(act)(z.detach())).all() and AO.act_fn(act)(z.detach())[-1].abs().item() < 1e-30


# =================================================================================================================================
# GPU: 1. pointwise kernels
# =================================================================================================================================
def _pointwise_ref(x, g, act):
    z = x.double().requires_grad_(True)
    a = AO.act_fn(act)(z)
    a.backward(g.double())
    return a.detach(), z.grad


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('shape,misaligned', [((2, 5, 7, 9), False), ((2, 8, 8, 16), False), ((2, 8, 8, 16), True)])
def test_pointwise_activation(act, shape, misaligned):
    from dynmm_amd import lib as L, ops
    x = rnd(*shape, seed=3, scale=2.5)
    g = rnd(*shape, seed=4)
    assert_off_kinks([x.double()], act)
    a_ref, dz_ref = _pointwise_ref(x, g, act)

    def dev(t):                                   # (misaligned: a contiguous view 4 bytes off the 16-byte grid -> the scalar form)
        if not misaligned:
            return t.cuda()
        return torch.cat([torch.zeros(1), t.flatten()]).cuda()[1:].view(t.shape)
    xd, gd = dev(x).requires_grad_(True), dev(g)
    assert (xd.data_ptr() % 16 != 0) == misaligned
    a = ops.activation(xd, act)
    a.backward(gd)
    print(f'{act} {shape}: fwd {rel(a, a_ref):.2e} dx {rel(xd.grad, dz_ref):.2e}')
    assert rel(a, a_ref) < TOL and rel(xd.grad, dz_ref) < GTOL
    with torch.no_grad():
        assert torch.equal(ops.activation(xd.detach(), act), a.detach())
    # the bias-gradient variant through the C ABI: dz and the per-channel sum in one pass
    lib = L.load()
    n, c, hw = shape[0], shape[1], shape[2] * shape[3]
    dz, db = torch.empty_like(xd.detach()), torch.empty(c, device='cuda')
    ws = torch.empty(max(lib.dynmm_act_bwd_bias_workspace_bytes(n, c) // 4, 1), device='cuda')
    L.check(lib.dynmm_act_pre_bwd(gd.data_ptr(), xd.data_ptr(), dz.data_ptr(), db.data_ptr(), ws.data_ptr(), n, c, hw,
                                  L.ACT[act], ops._stream()), 'act_pre_bwd')
    assert torch.equal(dz, xd.grad) and rel(db, dz_ref.sum(dim=(0, 2, 3))) < GTOL
    db2 = torch.empty(c, device='cuda')
    L.check(lib.dynmm_act_pre_bwd(gd.data_ptr(), xd.data_ptr(), None, db2.data_ptr(), ws.data_ptr(), n, c, hw,
                                  L.ACT[act], ops._stream()), 'act_pre_bwd')
    assert torch.equal(db, db2)


@gpu
@pytest.mark.parametrize('act', SMOOTH)
def test_pointwise_activation_on_the_value_grid(act):
    from dynmm_amd import ops
    x = torch.tensor(GRID, dtype=torch.float32).view(1, 1, 1, -1)
    a_ref, dz_ref = _pointwise_ref(x, torch.ones_like(x), act)
    xd = x.cuda().requires_grad_(True)
    a = ops.activation(xd, act)
    a.sum().backward()
    assert rel(a, a_ref) < TOL and rel(xd.grad, dz_ref) < GTOL
    if act == 'hswish':          # the convention at the kinks, exactly
        assert xd.grad.flatten()[0].item() == 0.0 and xd.grad.flatten()[1].item() == 1.0
    last = a.flatten()[-1].item()
    assert np.isfinite(last) and last == 0.0 and torch.isfinite(xd.grad).all()       # z = -90: -0 or 0


@gpu
def test_output_form_entry_points_refuse_the_smooth_codes():
    """act' of Swish / Hswish is no function of the output: the entry points that take y answer EUNSUPPORTED, never a wrong
    gradient."""
    from dynmm_amd import lib as L, ops
    lib = L.load()
    t = torch.ones(1, 4, 4, 4, device='cuda')
    v = torch.ones(4, device='cuda')
    s = torch.zeros(8, device='cuda', dtype=torch.float64)
    for code in L.SMOOTH_ACTS:
        assert lib.dynmm_act_bwd_bias(t.data_ptr(), t.data_ptr(), t.clone().data_ptr(), None, None, 1, 4, 16, code,
                                      ops._stream()) == L.DYNMM_EUNSUPPORTED
        assert lib.dynmm_bn_bwd_reduce(t.data_ptr(), t.data_ptr(), t.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(),
                                       v.data_ptr(), s.data_ptr(), 1, 4, 16, code, 1, None, ops._stream()) == L.DYNMM_EUNSUPPORTED


# =================================================================================================================================
# GPU: 2. inference epilogues (conv + folded BN + residual + activation in one launch)
# =================================================================================================================================
EVAL_CASES = [   # n, ci, h, w, co, k, stride, padding, x2 channels, family
    (2, 64, 12, 16, 128, (1, 1), (1, 1), (0, 0), 0, 'direct'),
    (3, 128, 8, 8, 64, (3, 3), (2, 2), (1, 1), 0, 'direct'),
    (7, 64, 6, 12, 64, (3, 1), (1, 1), (1, 0), 0, 'wino'),
    (3, 128, 7, 16, 24, (1, 3), (1, 1), (0, 1), 0, 'wino'),
    (2, 64, 12, 16, 128, (3, 3), (1, 1), (1, 1), 0, 'wino2d'),
    (2, 3, 48, 64, 64, (7, 7), (2, 2), (3, 3), 0, 'direct'),
    (2, 1, 48, 64, 64, (7, 7), (2, 2), (3, 3), 0, 'direct'),
    (2, 64, 21, 37, 8, (5, 5), (2, 2), (0, 0), 64, 'direct'),
]


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('case', EVAL_CASES)
def test_fused_eval_convolution(case, act):
    from dynmm_amd import ops
    n, ci, h, w, co, k, stride, pad, c2, family = case
    x, x2 = rnd(n, ci, h, w, seed=1), (rnd(n, c2, h, w, seed=2) if c2 else None)
    wgt = torch.nn.Parameter(rnd(co, ci + c2, *k, seed=3) / ((ci + c2) * k[0] * k[1]) ** 0.5)
    bias = rnd(co, seed=4)
    bn = torch.nn.BatchNorm2d(co).eval()
    with torch.no_grad():
        bn.weight.copy_(rnd(co, seed=5).abs() + 0.5)
        bn.bias.copy_(rnd(co, seed=6))
        bn.running_mean.copy_(rnd(co, seed=7) * 0.1)
        bn.running_var.copy_(rnd(co, seed=8).abs() + 0.5)
    xin = x if x2 is None else torch.cat([x, x2], 1)
    z = F.conv2d(xin.double(), wgt.detach().double(), None, stride, pad)
    res = rnd(*z.shape, seed=9)
    g = ops._geom(x.cuda(), None if x2 is None else x2.cuda(), wgt.detach().cuda(), stride, pad)
    got_family = 'wino2d' if ops._wino2d(g, False, x2, infer=True) else ('wino' if ops._wino(g, False, x2, infer=True) else 'direct')
    assert got_family == family, (case, got_family)
    wd, bnd = torch.nn.Parameter(wgt.detach().cuda()), bn.cuda()
    fn = AO.act_fn(act)
    sc = (bn.weight.detach().double() / (bn.running_var.double() + bn.eps).sqrt()).cpu().view(1, -1, 1, 1)
    sh = (bn.bias.detach().double().cpu().view(1, -1, 1, 1) - bn.running_mean.double().cpu().view(1, -1, 1, 1) * sc)
    with torch.no_grad():
        xd, x2d = x.cuda(), (None if x2 is None else x2.cuda())
        for name, got, ref in (
                ('bias', ops.conv2d_fused_eval(xd, wd, bias.cuda(), None, act, None, stride, pad, x2d),
                 fn(z + bias.double().view(1, -1, 1, 1))),
                ('bn', ops.conv2d_fused_eval(xd, wd, None, bnd, act, None, stride, pad, x2d), fn(z * sc + sh)),
                ('bn+res', ops.conv2d_fused_eval(xd, wd, None, bnd, act, res.cuda(), stride, pad, x2d),
                 fn(z * sc + sh + res.double()))):
            print(f'{act} {case} {name}: {rel(got, ref):.2e}')
            assert rel(got, ref) < TOL, (name, case)
    # ONE launch: the activation is in the convolution's epilogue, not a pointwise pass behind it
    calls = []
    real = ops._lib().dynmm_act_pre_fwd
    try:
        ops._lib().dynmm_act_pre_fwd = lambda *a: calls.append(a) or real(*a)
        with torch.no_grad():
            ops.conv2d_fused_eval(xd, wd, None, bnd, act, None, stride, pad, x2d)
    finally:
        ops._lib().dynmm_act_pre_fwd = real
    assert not calls


# =================================================================================================================================
# GPU: 3. BatchNorm + activation, training
# =================================================================================================================================
@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('shape', [(2, 6, 5, 7), (3, 8, 8, 8)])
@pytest.mark.parametrize('eps', [1e-3, 1e-5])
@pytest.mark.parametrize('residual', [False, True])
def test_batch_norm_activation_training(act, shape, eps, residual):
    from dynmm_amd import ops
    c = shape[1]
    seed = 21
    x, r, g = rnd(*shape, seed=seed, scale=1.5), (rnd(*shape, seed=seed + 1) if residual else None), rnd(*shape, seed=seed + 2)
    gam, bet = rnd(c, seed=seed + 3).abs() + 0.5, rnd(c, seed=seed + 4)
    # float64 truth
    x64, gam64, bet64 = (t.double().requires_grad_(True) for t in (x, gam, bet))
    r64 = r.double().requires_grad_(True) if residual else None
    rm64, rv64 = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    z64 = F.batch_norm(x64, rm64, rv64, gam64, bet64, True, 0.1, eps)
    if residual:
        z64 = z64 + r64
    assert_off_kinks([z64.detach()], act)
    y64 = AO.act_fn(act)(z64)
    y64.backward(g.double())

    bn = torch.nn.BatchNorm2d(c, eps=eps)
    with torch.no_grad():
        bn.weight.copy_(gam)
        bn.bias.copy_(bet)
    bn = bn.cuda().train()
    xd = x.cuda().requires_grad_(True)
    rd = r.cuda().requires_grad_(True) if residual else None
    y = ops.batch_norm_act(xd, bn, act, rd)
    y.backward(g.cuda())
    errs = dict(y=rel(y, y64), dx=rel(xd.grad, x64.grad), dgamma=rel(bn.weight.grad, gam64.grad), dbeta=rel(bn.bias.grad, bet64.grad),
                rm=rel(bn.running_mean, rm64), rv=rel(bn.running_var, rv64))
    if residual:
        errs['dres'] = rel(rd.grad, r64.grad)
    print(act, shape, eps, residual, {k: f'{v:.2e}' for k, v in errs.items()})
    assert errs['y'] < TOL and errs['rm'] < TOL and errs['rv'] < TOL
    assert all(errs[k] < GTOL for k in errs if k.startswith('d')), errs
    assert int(bn.num_batches_tracked) == 1


@gpu
@pytest.mark.parametrize('act', SMOOTH)
def test_batch_norm_activation_with_statistics_from_the_convolution(act):
    """pre_sums: the batch statistics come out of the producing convolution's epilogue (conv2d(bn_stats=True)); same results as
    with the statistics pass, and both against float64."""
    from dynmm_amd import ops
    n, c, h, w = 2, 64, 8, 16            # (the smallest map whose 1x3 convolution leaves its statistics: W % 16 == 0)
    x, g = rnd(n, c, h, w, seed=31), rnd(n, c, h, w, seed=32)
    wgt, bias = rnd(c, c, 1, 3, seed=33) / (3 * c) ** 0.5, rnd(c, seed=34)
    gam, bet = rnd(c, seed=35).abs() + 0.5, rnd(c, seed=36)
    x64, w64, gam64, bet64 = (t.double().requires_grad_(True) for t in (x, wgt, gam, bet))
    z64 = F.batch_norm(F.conv2d(x64, w64, bias.double(), 1, (0, 1)), None, None, gam64, bet64, True, 0.1, 1e-3)
    assert_off_kinks([z64.detach()], act)
    AO.act_fn(act)(z64).backward(g.double())
    outs = []
    for stats in (True, False):
        bn = torch.nn.BatchNorm2d(c, eps=1e-3)
        with torch.no_grad():
            bn.weight.copy_(gam)
            bn.bias.copy_(bet)
        bn = bn.cuda().train()
        xd, wd, bd = x.cuda().requires_grad_(True), wgt.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        c_out = ops.conv2d(xd, wd, bd, 1, (0, 1), None, bn_stats=stats)
        if stats:
            assert getattr(c_out, '_bn_sums', None) is not None, 'this shape is expected to leave its statistics with the output'
        y = ops.batch_norm_act(c_out, bn, act)
        y.backward(g.cuda())
        outs.append(y.detach())
        errs = dict(dx=rel(xd.grad, x64.grad), dw=rel(wd.grad, w64.grad), dgamma=rel(bn.weight.grad, gam64.grad),
                    dbeta=rel(bn.bias.grad, bet64.grad))
        print(act, 'pre_sums' if stats else 'stats pass', {k: f'{v:.2e}' for k, v in errs.items()})
        assert rel(y, AO.act_fn(act)(z64)) < TOL and all(v < GTOL for v in errs.values()), errs
    assert rel(outs[0], outs[1]) < TOL


# =================================================================================================================================
# GPU: 4. conv + bias + activation, training
# =================================================================================================================================
@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('k,pad', [((3, 1), (1, 0)), ((1, 3), (0, 1))])
def test_conv_bias_activation_training(act, k, pad):
    from dynmm_amd import ops
    n, c, h, w = 2, 64, 8, 12
    x, g = rnd(n, c, h, w, seed=45), rnd(n, c, h, w, seed=42)       # (seed 41 puts a 1x3 pre-activation 1e-5 from a kink)
    wgt, bias = rnd(c, c, *k, seed=43) * (2.0 / (3 * c)) ** 0.5, rnd(c, seed=44)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wgt, bias))
    z64 = F.conv2d(x64, w64, b64, 1, pad)
    assert_off_kinks([z64.detach()], act)
    y64 = AO.act_fn(act)(z64)
    y64.backward(g.double())
    grads = []
    for hints in (False, True):         # the ReLU-decision hints are ignored by a smooth activation: same results
        xd, wd, bd = x.cuda().requires_grad_(True), wgt.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        y = ops.conv2d(xd, wd, bd, 1, pad, act, mask_input=hints, defer_mask=hints)
        y.backward(g.cuda())
        errs = dict(y=rel(y, y64), dx=rel(xd.grad, x64.grad), dw=rel(wd.grad, w64.grad), db=rel(bd.grad, b64.grad))
        print(act, k, 'hints' if hints else 'plain', {kk: f'{v:.2e}' for kk, v in errs.items()})
        assert errs['y'] < TOL and all(errs[kk] < GTOL for kk in ('dx', 'dw', 'db')), errs
        grads.append((xd.grad, wd.grad, bd.grad))
    assert all(torch.equal(a, b) for a, b in zip(*grads))


# =================================================================================================================================
# GPU: 5. SE excitation and the per-stage gate
# =================================================================================================================================
def _se_params(c, seed, double=False):
    hd = c // 16
    shapes = [(hd, c, 1, 1), (hd,), (c, hd, 1, 1), (c,)] * 2
    ps = [rnd(*s, seed=seed + i) * (0.5 if len(s) == 4 else 0.3) for i, s in enumerate(shapes)]
    return ps


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('with_wcum', [False, True])
def test_se_fuse_blend_with_a_smooth_hidden_activation(act, with_wcum):
    from dynmm_amd import ops
    n, c, h, w = 3, 64, 6, 8
    rgb, depth, g = rnd(n, c, h, w, seed=51), rnd(n, c, h, w, seed=52), rnd(n, c, h, w, seed=53)
    ps = _se_params(c, 54)
    wcum = torch.rand(n, 4, generator=torch.Generator().manual_seed(5)) if with_wcum else None
    col = 2
    t64 = [t.double().requires_grad_(True) for t in [rgb, depth] + ps]
    wc64 = wcum.double().requires_grad_(True) if with_wcum else None
    with AO.record_preacts() as pre:
        out64 = AO.se_fuse_blend(t64[2:], t64[0], t64[1], act, None if wc64 is None else wc64[:, col])
    assert_off_kinks(pre, act)
    out64.backward(g.double())
    td = [t.cuda().requires_grad_(True) for t in [rgb, depth] + ps]
    wcd = wcum.cuda().requires_grad_(True) if with_wcum else None
    out = ops.se_fuse_blend(td[0], td[1], td[2:], wcd, col, se_act=act)
    out.backward(g.cuda())
    errs = {f'd{i}': rel(a.grad, b.grad) for i, (a, b) in enumerate(zip(td, t64))}      # drgb, ddepth and the 8 parameters
    if with_wcum:
        errs['dwcum'] = rel(wcd.grad, wc64.grad)
    print(act, with_wcum, f'out {rel(out, out64):.2e}', {k: f'{v:.2e}' for k, v in errs.items()})
    assert rel(out, out64) < TOL and all(v < GTOL for v in errs.values()), errs


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('hard', [False, True])
def test_reweigh_fuse_with_a_smooth_hidden_activation(act, hard):
    from dynmm_amd import ops
    O = AO.oracle(act)
    n, c, h, w = 3, 64, 6, 8
    temp = 0.7
    rgb, depth = rnd(n, c, h, w, seed=61), rnd(n, c, h, w, seed=62)
    g, gw = rnd(n, c, h, w, seed=63), rnd(n, 2, seed=64)
    c2, hd = 2 * c, 2 * c // 16
    ps = [rnd(hd, c2, 1, 1, seed=65) * 0.5, rnd(hd, seed=66) * 0.3, rnd(c2, hd, 1, 1, seed=67) * 0.5, rnd(c2, seed=68) * 0.3]
    noise = torch.from_numpy(np.random.Generator(np.random.PCG64(7)).exponential(size=(n, 2)).astype(np.float32))
    prev = torch.rand(n, generator=torch.Generator().manual_seed(9))
    wblend = torch.softmax(rnd(n, 2, seed=69), 1)
    names = ['p.se.fc.0.weight', 'p.se.fc.0.bias', 'p.se.fc.2.weight', 'p.se.fc.2.bias']
    t64 = [t.double().requires_grad_(True) for t in [rgb, depth, wblend, prev] + ps]
    sd = dict(zip(names, t64[4:]))
    with AO.record_preacts() as pre:
        wn64 = O.reweigh_gate(sd, 'p', t64[0], t64[1], temp, noise.double(), hard, t64[3])
    assert_off_kinks(pre, act)
    wb = t64[2].view(-1, 2, 1, 1)
    out64 = wb[:, 0:1] * t64[0] + wb[:, 1:2] * (t64[0] + t64[1])
    torch.autograd.backward([out64, wn64], [g.double(), gw.double()])
    td = [t.cuda().requires_grad_(True) for t in [rgb, depth, wblend, prev] + ps]
    out, wn, _ = ops.reweigh_fuse(td[0], td[1], td[2], 2, td[4:], temp, hard, td[3], noise.cuda(), se_act=act)
    torch.autograd.backward([out, wn], [g.cuda(), gw.cuda()])
    errs = {f'd{i}': rel(a.grad, b.grad) for i, (a, b) in enumerate(zip(td, t64))}
    print(act, hard, f'out {rel(out, out64):.2e} wnext {rel(wn, wn64):.2e}', {k: f'{v:.2e}' for k, v in errs.items()})
    assert rel(out, out64) < TOL and rel(wn, wn64) < TOL and all(v < GTOL for v in errs.values()), errs


# =================================================================================================================================
# GPU: 6. blocks
# =================================================================================================================================
def run_block(module, ref_fn, inputs, act, prefix='m', seed=3):
    """train-mode forward and every gradient of a module against the restatement in float64"""
    synth.fill_state_dict(module.state_dict(), seed=seed)
    sd = {f'{prefix}.{k}': (v.detach().clone().double() if v.dtype.is_floating_point else v.detach().clone())
          for k, v in module.state_dict().items()}
    params = oracle_params(sd)
    xs_ref = [x.clone().double().requires_grad_(True) for x in inputs]
    with AO.record_preacts() as pre:
        out_ref = ref_fn(sd, *xs_ref)
    assert_off_kinks(pre, act)
    outs_ref = [o for o in (out_ref if isinstance(out_ref, tuple) else (out_ref,)) if o is not None]
    gs = [rnd(*o.shape, seed=11 + i) for i, o in enumerate(outs_ref)]
    torch.autograd.backward(outs_ref, [g.double() for g in gs])

    module = module.cuda().train()
    xs = [x.clone().cuda().requires_grad_(True) for x in inputs]
    out = module(*xs)
    outs = [o for o in (out if isinstance(out, tuple) else (out,)) if o is not None]
    torch.autograd.backward(outs, [g.cuda() for g in gs])
    worst_out = max(rel(a, b) for a, b in zip(outs, outs_ref))
    errs = {f'dinput{i}': rel(a.grad, b.grad) for i, (a, b) in enumerate(zip(xs, xs_ref))}
    gmax = max(v.grad.abs().max().item() for v in params.values())
    for name, p in module.named_parameters():
        ref = params[f'{prefix}.{name}'].grad
        if ref.abs().max() < 1e-5 * gmax:            # analytically zero (a conv bias in front of a train-mode BatchNorm)
            continue
        errs[name] = rel(p.grad, ref)
    worst = max(errs, key=errs.get)
    print(f'{type(module).__name__} {act}: outputs {worst_out:.2e}, worst gradient {worst} {errs[worst]:.2e}')
    assert worst_out < 5e-5, worst_out
    assert errs[worst] < BLOCK_GTOL, sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    new_sd = module.state_dict()
    for k, v in sd.items():
        if 'running_' in k:
            assert rel(new_sd[k[len(prefix) + 1:]], v) < 1e-4, k


def _downsample(cin, cout, stride):
    return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(cout))


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('which', ['nb1d', 'nb1d_s2', 'basic', 'bottleneck', 'chain', 'convbnact', 'ppm', 'appm', 'decoder'])
def test_blocks(which, act):
    from dynmm_amd.nn import blocks as B
    from dynmm_amd.nn.context import AdaptivePyramidPoolingModule, PyramidPoolingModule
    from dynmm_amd.nn.decoder import DecoderModule
    O = AO.oracle(act)
    x = rnd(2, 64, 12, 16, seed=7)
    if which == 'nb1d':
        run_block(B.NonBottleneck1D(64, 64, activation=act), lambda sd, x: O.non_bottleneck_1d(sd, 'm', x, True), [x], act)
    elif which == 'nb1d_s2':
        run_block(B.NonBottleneck1D(64, 128, 2, _downsample(64, 128, 2), activation=act),
                  lambda sd, x: O.non_bottleneck_1d(sd, 'm', x, True, 2), [x], act)
    elif which == 'basic':
        run_block(B.BasicBlock(64, 64, activation=act), lambda sd, x: O.basic_block(sd, 'm', x, True), [x], act)
    elif which == 'bottleneck':
        run_block(B.Bottleneck(64, 16, activation=act), lambda sd, x: O.bottleneck(sd, 'm', x, True), [x], act)
    elif which == 'chain':
        class Stage(torch.nn.Sequential):
            def forward(self, x):
                y = self[0](x)
                assert getattr(y, '_bn_out_link', None) is None, 'a smooth activation must not offer the ReLU chain'
                return self[1](y, chain=True)
        run_block(Stage(B.NonBottleneck1D(64, 64, activation=act), B.NonBottleneck1D(64, 64, activation=act)),
                  lambda sd, x: O.non_bottleneck_1d(sd, 'm.1', O.non_bottleneck_1d(sd, 'm.0', x, True), True), [x], act)
    elif which == 'convbnact':
        run_block(B.ConvBNAct(64, 128, 3, activation=act), lambda sd, x: O.conv_bn_act(sd, 'm', x, True, padding=1), [x], act)
    elif which == 'ppm':
        run_block(PyramidPoolingModule(512, 128, activation=act), lambda sd, x: O.pyramid_pooling(sd, 'm', x, True),
                  [rnd(2, 512, 3, 4, seed=8)], act)
    elif which == 'appm':
        run_block(AdaptivePyramidPoolingModule(512, 128, (3, 4), bins=(1, 5), upsampling_mode='nearest', activation=act),
                  lambda sd, x: AO.adaptive_pyramid_pooling(sd, 'm', x, True, act, (3, 4)), [rnd(2, 512, 3, 4, seed=8)], act)
    else:
        run_block(DecoderModule(64, 64, 1, 40, activation=act),
                  lambda sd, x, s: O.decoder_module(sd, 'm', x, s, True, 1), [x, rnd(2, 64, 24, 32, seed=9)], act)


# =================================================================================================================================
# GPU: 7. networks
# =================================================================================================================================
def _rl2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _hip_forward(m, kind, rgb, depth, training, test=False):
    if kind == 'gate':
        return m(rgb, depth) if training else m(rgb, depth, test=True, return_weight=True)
    if kind == 'skip':
        return m(rgb, depth, test=test)
    return m(rgb, depth)


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('kind', NETS)
def test_networks_match_the_reference_fixtures(golden_dir, kind, act):
    g = golden(golden_dir, act)
    stride = int(g['meta'][3])
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234, device='cuda')
    for tag, training, mode, scfg in net_cases(g, kind):
        kw = dict(temp=scfg[3], block_rule=scfg[4]) if kind == 'skip' else {}
        m = build_net(kind, act, **kw).cuda().train(training)
        if kind == 'gate':
            m.baseline, m.hard_gate, m.temp = mode == 'eval_baseline', mode == 'eval_hard', 1.0
        if kind == 'skip':
            m.hard_gate = scfg[2]
            m.gumbel_noise = [t.cuda() for t in skip_noise(g, tag)]
        if training:
            res = _hip_forward(m, kind, rgb, depth, True, scfg[1] if scfg else False)
            outs, lf = res if kind == 'gate' else (res, None)
            out = outs[0].detach().cpu()
            for i, o in enumerate(outs[1:]):
                assert rel(o, torch.from_numpy(g[f'{tag}/side{i}'])) < TRAIN_OUT_TOL, (tag, i)
        else:
            with torch.no_grad():
                res = _hip_forward(m, kind, rgb, depth, False, scfg[1] if scfg else False)
                out = (res[0] if kind == 'gate' else res).cpu()
                if kind == 'gate':
                    assert rel(res[1], torch.from_numpy(g[f'{tag}/weight'])) < 1e-4
                    _, lf = m(rgb, depth)
        if kind == 'gate':
            assert abs(lf.item() - float(g[f'{tag}/loss_flop'])) < 1e-4, tag
        tol = TRAIN_OUT_TOL if training else LOGIT_TOL
        e = Hh.rel_err(out[:, :, ::stride, ::stride], g[f'{tag}/strided'])
        print(f'{kind} {act} {tag}: strided outputs {e:.2e} (bar {tol})')
        assert e < tol, tag
        assert Hh.rel_err(out.sum(dim=(2, 3)), g[f'{tag}/csum']) < 1e-3 and Hh.rel_err(out.abs().sum(dim=(2, 3)), g[f'{tag}/cabs']) < 1e-3


@gpu
@pytest.mark.parametrize('act', SMOOTH)
@pytest.mark.parametrize('kind', NETS)
def test_network_gradients_against_the_float64_restatement(golden_dir, kind, act):
    """The rule of test_hip_model.test_model_vs_oracle_fwd_bwd_full_tensors: against the float64 restatement, the HIP path's median
    and maximum per-tensor relative L2 and the concatenated gradient's relative L2 stay within 3x what the SAME restatement in
    float32 on the CPU shows, plus 1e-5 / 1e-3 / 1e-5.  Analytically zero gradients are skipped as there.

    The BatchNorm + Swish / Hswish path takes its batch statistics with fp64 squares (csrc/norm.hip bn_stats_f64_kernel): with
    fp32 squares the two-values-per-channel pyramid-pooling branch lost its variance to rounding and the skip / hswish case sat at
    4.9x the restatement's error."""
    g = golden(golden_dir, act)
    tag = {'gate': 'gate/train_soft', 'skip': 'skip/train_soft', 'esanet': 'esanet/train'}[kind]
    scfg = dict((t, s) for t, _, _, s in net_cases(g, kind))[tag]
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234)
    kw = dict(temp=scfg[3], block_rule=scfg[4]) if kind == 'skip' else {}

    def restated(dtype):
        sd = oracle_sd(build_net(kind, act, **kw), dtype)
        params = oracle_params(sd)
        noise = skip_noise(g, tag, dtype) if kind == 'skip' else None
        outs, lf, _ = oracle_run(kind, act, sd, rgb.to(dtype), depth.to(dtype), True, 'train_soft', noise, scfg)
        Hh.train_loss(outs, lf if lf is not None else torch.zeros((), dtype=dtype)).backward()
        # (parameters the forward never uses — SkipESANet's se_layer*, the gates' `linear` — have no gradient: skipped below)
        return [o.detach() for o in outs], lf, {k: v.grad.detach() for k, v in params.items() if v.grad is not None}
    outs32, _, g32 = restated(torch.float32)
    outs64, lf64, g64 = restated(torch.float64)

    m = build_net(kind, act, **kw).cuda().train()
    if kind == 'skip':
        m.hard_gate = scfg[2]
        m.gumbel_noise = [t.cuda() for t in skip_noise(g, tag)]
    if kind == 'gate':
        m.temp = 1.0
    res = _hip_forward(m, kind, rgb.cuda(), depth.cuda(), True, scfg[1] if scfg else False)
    outs, lf = res if kind == 'gate' else (res, None)
    Hh.train_loss(outs, lf if lf is not None else torch.zeros((), device='cuda')).backward()
    torch.cuda.synchronize()
    for a, b32, b64 in zip(outs, outs32, outs64):
        assert rel(a, b64) < max(3 * Hh.rel_err(b32, b64), 1e-5) or rel(a, b64) < TRAIN_OUT_TOL
        assert rel(a, b64) < TRAIN_OUT_TOL
    if kind == 'gate':
        assert abs(lf.item() - lf64.item()) < 1e-4
    gmax = max(v.abs().max().item() for v in g64.values())
    params = dict(m.named_parameters())
    names = [nm for nm in params if nm in g64 and g64[nm].abs().max().item() >= 1e-5 * gmax]
    unused = [nm for nm in params if nm not in g64]
    assert all(params[nm].grad is None or not params[nm].grad.any() for nm in unused), unused[:4]
    e_hip = np.array([_rl2(params[nm].grad.cpu(), g64[nm]) for nm in names])
    e_ref = np.array([_rl2(g32[nm], g64[nm]) for nm in names])
    cat = lambda src: torch.cat([src(nm).double().flatten() for nm in names])   # noqa: E731
    c_hip, c_ref = _rl2(cat(lambda nm: params[nm].grad.cpu()), cat(lambda nm: g64[nm])), _rl2(cat(lambda nm: g32[nm]), cat(lambda nm: g64[nm]))
    print(f'{kind} {act}: per-tensor rel L2 vs float64 — HIP median {np.median(e_hip):.3e} max {e_hip.max():.3e} '
          f'({names[int(e_hip.argmax())]}) | float32 CPU restatement median {np.median(e_ref):.3e} max {e_ref.max():.3e} | '
          f'concatenated HIP {c_hip:.3e} restatement {c_ref:.3e}')
    for i in np.argsort(-e_hip)[:8]:
        print(f'    {names[int(i)]}: HIP {e_hip[i]:.3e} restatement {e_ref[i]:.3e}')
    assert np.median(e_hip) <= 3 * np.median(e_ref) + 1e-5, (np.median(e_hip), np.median(e_ref))
    assert e_hip.max() <= 3 * e_ref.max() + 1e-3, (names[int(e_hip.argmax())], e_hip.max(), e_ref.max())
    assert c_hip <= 3 * c_ref + 1e-5, (c_hip, c_ref)


# =================================================================================================================================
# GPU: 8. callers
# =================================================================================================================================
@gpu
def test_infer_step_replay_is_bit_identical_for_hswish():
    from dynmm_amd import engine
    m = build_net('gate', 'hswish').cuda().eval()
    batches = [synth.synth_inputs(N, H, W, seed=s, device='cuda') for s in (1, 2, 3)]
    step = engine.InferStep(m, capture_after=2)
    for rgb, depth in batches + batches:
        with torch.no_grad():
            ref = m(rgb, depth, True).clone()
        assert torch.equal(step(rgb, depth), ref)
    assert step.launch == 'hipGraph replay'
    auto = engine.InferStep(m, policy='auto')
    for rgb, depth in batches + batches:
        with torch.no_grad():
            ref = m(rgb, depth, True).clone()
        assert torch.equal(auto(rgb, depth), ref)


@gpu
def test_hard_gate_compaction_under_hswish_equals_the_dense_forward():
    m = build_net('gate', 'hswish').cuda().eval()
    n = 5
    rgb, depth = synth.synth_inputs(n, H, W, seed=77, device='cuda')
    m.ini_stage, m.ini_branches = True, [2, 0, 4, 1, 3]          # all five branches, unsorted
    outs = {}
    for compact in (False, True):
        m.compact = compact
        with torch.no_grad():
            outs[compact] = m(rgb, depth, test=True).clone()
    assert m.last_stage_batch == [4, 3, 2, 1]
    e = rel(outs[True], outs[False])
    print(f'hswish compaction vs dense: {e:.2e}')
    assert e < LOGIT_TOL


@gpu
def test_train_step_with_swish():
    """One engine.TrainStep SGD step: the loss equals the restatement's (float64) to 1e-4 relative, and every parameter moved —
    every one whose gradient is not analytically zero (a convolution bias in front of a train-mode BatchNorm: its float32
    gradient is rounding noise, and lr times noise need not change a float32 value; the skip rule of the gradient tests)."""
    from dynmm_amd import engine
    act = 'swish'
    O = AO.oracle(act)
    m = build_net('gate', act).cuda().train()
    m.temp, m.hard_gate = 1.0, False
    sd0 = oracle_sd(m, torch.float64)
    p0 = {k: v.detach().clone() for k, v in m.named_parameters()}
    cw = np.linspace(0.5, 2.0, 40)
    rgb, depth = synth.synth_inputs(N, H, W, seed=1234, device='cuda')
    labels = [synth.synth_labels(N, H // s, W // s, seed=300 + s, device='cuda') for s in (1, 8, 16, 32)]
    step = engine.TrainStep(m, cw, lr=0.05, momentum=0.0, weight_decay=0.0, loss_ratio=0.0)
    last = step(rgb, depth, labels)
    torch.cuda.synchronize()
    params = oracle_params(sd0)
    outs, _ = O.forward(sd0, rgb.cpu().double(), depth.cpu().double(), CFG, training=True, temp=1.0)
    ref = sum(O.cross_entropy_2d(outs, [t.cpu() for t in labels], torch.as_tensor(cw, dtype=torch.float64)))
    ref.backward()
    gmax = max(v.grad.abs().max().item() for v in params.values())
    got = float(last['total'])
    print(f'swish train step: loss {got:.6f} restatement {ref.item():.6f}')
    assert abs(got - ref.item()) <= 1e-4 * abs(ref.item())
    still = [k for k, v in m.named_parameters()
             if torch.equal(v.detach(), p0[k]) and params[k].grad.abs().max().item() >= 1e-5 * gmax]
    assert not still, still[:8]

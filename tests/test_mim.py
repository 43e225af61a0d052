"""Multiplicative interactions fusion on the HIP path: ops_mlp.mim (csrc/mim.hip), nn.imdb.MultiplicativeInteractions2Modal and the
builder experts.imdb_mm_mim.

The yardstick is `mim_ref` below: the three lines of MultiBench's fusions.common_fusions.MultiplicativeInteractions2Modal.forward
with output='matrix', in plain torch; in float64 it equals the closed form and the T_n gradient form of DESIGN.md section 7k to
1e-12 (first test).  Bars are the sequence kernels' (tests/test_seq_kernels.py, tests/test_lrtf.py): _rel = max|a - b| / max|b|
against float64, forward 1e-5, every gradient 2e-5; a case that does not sit under its bar is held to max(project bar, 4 x the
error of mim_ref in float32 on the same inputs) and marked RAISED in its FIG line.  Measured on an MI355X over every case below:
the kernels at most 1.5e-6 (`FIG 128x512-512x1024 unit out kernel=1.475e-06`, a 262144-term sum; next 1.0e-6, out at 64 x (512, 512)
x 64; every gradient under 7.6e-7), mim_ref in float32 at most 5.9e-6 (dm1 at the reference geometry, on the device; on the CPU
shapes at most 6.7e-7); no case needed a raised bar.
"""
import os

import pytest
import torch
import torch.nn as nn

from dynmm_amd import experts as E
from dynmm_amd import lib as L
from dynmm_amd import ops_mlp as M
from dynmm_amd.nn import imdb as I
from tests.parity import check_adam_params, compare_to_float64, randomize_bn, rel as _rel

FWD, BWD = 1e-5, 2e-5                         # test_seq_kernels.py: LN_FWD, LN_BWD

# (B, (n, m), D)
SHAPES = [(1, (3, 5), 4), (5, (7, 9), 20), (17, (33, 31), 40), (33, (64, 48), 72), (130, (96, 80), 136), (128, (128, 64), 256),
          (64, (512, 512), 64)]
FULL = (128, (512, 512), 1024)
INITS = ('unit', 'xavier')
NAMES = ['out', 'dm1', 'dm2', 'dW', 'dU', 'dV', 'db']


def mim_ref(m1, m2, W, U, V, b):
    """fusions.common_fusions.MultiplicativeInteractions2Modal.forward, output='matrix'."""
    Wprime = torch.einsum('bn,nmd->bmd', m1, W) + V
    bprime = torch.matmul(m1, U) + b
    return torch.einsum('bm,bmd->bd', m2, Wprime) + bprime


def closed_form(m1, m2, W, U, V, b):
    return torch.einsum('bn,bm,nmd->bd', m1, m2, W) + m2 @ V + m1 @ U + b


def _case(shape, init):
    """float64 masters of a case: unit-normal inputs and upstream gradient, parameters by `init`"""
    B, (n, m), D = shape
    g = torch.Generator().manual_seed(200 + B + 7 * D + 13 * n + m + (init == 'xavier'))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)            # noqa: E731
    m1, m2 = rn(B, n), rn(B, m)
    if init == 'unit':
        W, U, V, b = rn(n, m, D) / (n * m) ** 0.5, rn(n, D) / n ** 0.5, rn(m, D) / m ** 0.5, 0.1 * rn(D)
    else:
        torch.manual_seed(int(g.initial_seed()))
        mod = I.MultiplicativeInteractions2Modal([n, m], D, 'matrix')
        W, U, V, b = (t.detach().double() for t in (mod.W, mod.U, mod.V, mod.b))
    return {'m1': m1, 'm2': m2, 'W': W, 'U': U, 'V': V, 'b': b, 'g': rn(B, D)}


def _run(fn, c, dtype, device='cpu', need=(True,) * 6):
    ops = [c[k].to(device=device, dtype=dtype).clone().requires_grad_(r) for k, r in zip(('m1', 'm2', 'W', 'U', 'V', 'b'), need)]
    out = fn(*ops)
    (out * c['g'].to(device=device, dtype=dtype)).sum().backward()
    vals = [out] + [t.grad for t in ops]
    return {k: (None if v is None else v.detach().cpu()) for k, v in zip(NAMES, vals)}


_REF = {}


def _ref(shape, init):
    """(case, float64 results, float32 results) of mim_ref on the CPU, computed once and shared"""
    key = (shape, init)
    if key not in _REF:
        c = _case(shape, init)
        _REF[key] = (c, _run(mim_ref, c, torch.float64), _run(mim_ref, c, torch.float32))
    return _REF[key]


def _ids(s):
    return f'{s[0]}x{"-".join(map(str, s[1]))}x{s[2]}'


# ------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_closed_form_and_the_t_form_in_float64():
    for shape in SHAPES[:4]:
        c = _case(shape, 'unit')
        a, b = _run(mim_ref, c, torch.float64), _run(closed_form, c, torch.float64)
        for k in a:
            assert _rel(a[k], b[k]) < 1e-12, (shape, k)
        m1, m2, W, U, V, g = (c[k] for k in ('m1', 'm2', 'W', 'U', 'V', 'g'))
        T = torch.einsum('bd,nmd->nbm', g, W)                                    # T_n[b, m]
        hand = {'dW': torch.einsum('bn,bm,bd->nmd', m1, m2, g), 'dU': m1.t() @ g, 'dV': m2.t() @ g, 'db': g.sum(0),
                'dm1': torch.einsum('bm,nbm->bn', m2, T) + g @ U.t(), 'dm2': torch.einsum('bn,nbm->bm', m1, T) + g @ V.t()}
        for k, v in hand.items():
            assert _rel(v, a[k]) < 1e-12, (shape, k)


def test_restatement_in_float32_is_well_under_the_bars():
    for shape in SHAPES[:4]:
        for init in INITS:
            _, r64, r32 = _ref(shape, init)
            for k in r64:
                assert _rel(r32[k], r64[k]) < 0.25 * (FWD if k == 'out' else BWD), (shape, init, k)


def test_parameters_are_registered_named_shaped_and_initialised():
    torch.manual_seed(3)
    m = I.MultiplicativeInteractions2Modal([31, 17], 64, 'matrix')
    assert list(m.state_dict()) == ['W', 'U', 'V', 'b']
    assert [tuple(v.shape) for v in m.state_dict().values()] == [(31, 17, 64), (31, 64), (17, 64), (64,)]
    assert set(dict(m.named_parameters())) == set(m.state_dict()) and len(list(m.parameters())) == 4
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    for p in (m.W, m.U, m.V):
        fan_in, fan_out = nn.init._calculate_fan_in_and_fan_out(p)
        want = (2.0 / (fan_in + fan_out)) ** 0.5
        assert abs(p.std().item() - want) < 0.1 * want, tuple(p.shape)
    assert nn.init._calculate_fan_in_and_fan_out(m.W) == (17 * 64, 31 * 64)
    assert torch.count_nonzero(m.b) > 0 and 0.5 < m.b.std().item() < 1.5


def test_state_dict_loads_strictly_from_a_plain_torch_holder():
    h = _RefFusion(3, 5, 6)
    m = I.MultiplicativeInteractions2Modal([3, 5], 6, 'matrix')
    m.load_state_dict(h.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), h.parameters()))


def test_builder_has_the_reference_dimensions(tmp_path):
    from dynmm_amd import imdb_mm
    with torch.device('meta'):
        m, lr = E.imdb_mm_mim()
    assert lr == 8e-3
    assert [(e.op0.num_features, e.op1.d_out, e.op3.d_out, e.hid2val) for e in m.encoders] == \
        [(300, 512, 512, None), (4096, 1024, 512, None)]
    assert [e.tag for e in m.encoders] == ['encoders.0', 'encoders.1']
    assert isinstance(m.fuse, I.MultiplicativeInteractions2Modal) and not m.fuse.flip and not m.fuse.flatten
    assert tuple(m.fuse.W.shape) == (512, 512, 1024) and tuple(m.fuse.U.shape) == tuple(m.fuse.V.shape) == (512, 1024)
    assert tuple(m.fuse.b.shape) == (1024,)
    assert (m.head.fc.in_features, m.head.fc.out_features) == (1024, 23)
    assert imdb_mm.file_name(str(tmp_path), 3).endswith('/best_mim.pt')
    small, _ = E.imdb_mm_mim(output_dim=32)
    assert tuple(small.fuse.W.shape) == (512, 512, 32) and small.head.fc.in_features == 32
    assert list(small.fuse.state_dict()) == ['W', 'U', 'V', 'b'] and 'fuse.W' in small.state_dict()


def test_the_refused_module_options_raise():
    for kw in ({'output': 'vector'}, {'output': 'scalar'}, {'output': 'matrix', 'clip': (-1, 1)},
               {'output': 'matrix', 'grad_clip': (-1, 1)}):
        with pytest.raises(NotImplementedError):
            I.MultiplicativeInteractions2Modal([3, 5], 6, **kw)
    for dims in ([3], [3, 4, 5]):
        with pytest.raises(NotImplementedError):
            I.MultiplicativeInteractions2Modal(dims, 6, 'matrix')


def test_cpu_tensors_are_refused():
    m = I.MultiplicativeInteractions2Modal([3, 5], 6, 'matrix')
    with pytest.raises(L.DynmmHipError):
        m([torch.randn(2, 3), torch.randn(2, 5)])
    with pytest.raises(L.DynmmHipError):
        M.mim(torch.randn(2, 3), torch.randn(2, 5), m.W, m.U, m.V, m.b)


def test_the_pinned_refusal_still_raises():
    with pytest.raises(NotImplementedError, match='MultiplicativeInteractions2Modal'):
        E.imdb_mm(3)


def test_workspaces_stay_under_a_quarter_of_the_intermediate():
    """the library's size functions need no device"""
    lib = L.load()
    B, n, m, D = 128, 512, 512, 1024
    bound = B * m * D                                                            # bytes: a quarter of one [B, m, D] fp32 tensor
    fwd, bwd = lib.dynmm_mim_fwd_workspace_bytes(B, n, m, D), lib.dynmm_mim_bwd_workspace_bytes(B, n, m, D)
    assert 0 < fwd <= bound and 0 < bwd <= bound, (fwd, bwd, bound)
    assert lib.dynmm_mim_fwd_workspace_bytes(0, n, m, D) == 0 and lib.dynmm_mim_bwd_workspace_bytes(B, n, 0, D) == 0


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the op
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('init', INITS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_mim_against_float64(shape, init):
    c, r64, r32 = _ref(shape, init)
    compare_to_float64(f'{_ids(shape)} {init}', _run(M.mim, c, torch.float32, 'cuda'), r64, r32, ('out',), FWD, BWD)


@pytest.mark.gpu
def test_mim_at_the_reference_geometry():
    """float64 on the CPU would need 200 GFLOP and 6 GB here: the yardsticks run through torch on the device, after the device's
    float64 mim_ref is shown to equal the CPU's at a small shape."""
    small = SHAPES[3]
    c, r64, _ = _ref(small, 'unit')
    d64 = _run(mim_ref, c, torch.float64, 'cuda')
    for k in r64:
        assert _rel(d64[k], r64[k]) < 1e-12, k
    c = _case(FULL, 'unit')
    got = _run(M.mim, c, torch.float32, 'cuda')
    r32 = _run(mim_ref, c, torch.float32, 'cuda')
    torch.cuda.empty_cache()
    r64 = _run(mim_ref, c, torch.float64, 'cuda')
    torch.cuda.empty_cache()
    compare_to_float64(f'{_ids(FULL)} unit', got, r64, r32, ('out',), FWD, BWD)


@pytest.mark.gpu
def test_partial_requires_grad_skips_work_and_changes_no_bit():
    c = _ref(SHAPES[3], 'unit')[0]
    both = _run(M.mim, c, torch.float32, 'cuda')
    only_z = _run(M.mim, c, torch.float32, 'cuda', need=(True, True, False, False, False, False))
    only_p = _run(M.mim, c, torch.float32, 'cuda', need=(False, False, True, True, True, True))
    only_m2 = _run(M.mim, c, torch.float32, 'cuda', need=(False, True, False, False, False, False))
    for k in NAMES:
        is_z = k in ('dm1', 'dm2')
        if k == 'out':
            assert all(torch.equal(r[k], both[k]) for r in (only_z, only_p, only_m2))
            continue
        assert torch.equal(only_z[k], both[k]) if is_z else only_z[k] is None, k
        assert only_p[k] is None if is_z else torch.equal(only_p[k], both[k]), k
        assert torch.equal(only_m2[k], both[k]) if k == 'dm2' else only_m2[k] is None, k


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[6]], ids=_ids)
def test_two_calls_give_the_same_bits(shape):
    c = _ref(shape, 'unit')[0]
    a, b = _run(M.mim, c, torch.float32, 'cuda'), _run(M.mim, c, torch.float32, 'cuda')
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_operands_the_kernels_cannot_read_are_refused():
    r = lambda *s: torch.randn(*s, device='cuda')                                # noqa: E731
    m1, m2, W, U, V, b = r(4, 3), r(4, 5), r(3, 5, 6), r(3, 6), r(5, 6), r(6)
    assert tuple(M.mim(m1, m2, W, U, V, b).shape) == (4, 6)
    with pytest.raises(L.DynmmHipError, match='float32'):
        M.mim(m1.double(), m2, W, U, V, b)
    with pytest.raises(L.DynmmHipError, match='float32'):
        M.mim(m1, m2, W.double(), U, V, b)
    with pytest.raises(L.DynmmHipError, match='contiguous'):
        M.mim(r(3, 4).t(), m2, W, U, V, b)
    with pytest.raises(L.DynmmHipError, match='contiguous'):
        M.mim(m1, m2, r(3, 6, 5).transpose(1, 2), U, V, b)
    with pytest.raises(L.DynmmHipError, match='W must be'):
        M.mim(m1, m2, r(3, 4, 6), U, V, b)
    with pytest.raises(L.DynmmHipError, match='U must be'):
        M.mim(m1, m2, W, r(5, 6), V, b)
    with pytest.raises(L.DynmmHipError, match='V must be'):
        M.mim(m1, m2, W, U, r(3, 6), b)
    with pytest.raises(L.DynmmHipError, match='b must be'):
        M.mim(m1, m2, W, U, V, r(1, 6))
    with pytest.raises(L.DynmmHipError, match='share B'):
        M.mim(m1, r(3, 5), W, U, V, b)
    with pytest.raises(L.DynmmHipError):
        M.mim(m1, m2, W, U.cpu(), V, b)


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the module
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_module_flip_and_flatten_equal_the_op_bit_for_bit():
    torch.manual_seed(4)
    B, n, m, D = 9, 12, 10, 20
    x1, x2 = torch.randn(B, 2, 5, device='cuda'), torch.randn(B, 3, 4, device='cuda')        # flattened: 10 and 12
    gy = torch.randn(B, D, device='cuda')
    mod = I.MultiplicativeInteractions2Modal([n, m], D, 'matrix', flatten=True, flip=True).cuda()
    a1, a2 = x1.clone().requires_grad_(True), x2.clone().requires_grad_(True)
    out = mod([a1, a2])                                                          # flip: m1 = the second modality
    (out * gy).sum().backward()
    prm = [p.detach().clone().requires_grad_(True) for p in (mod.W, mod.U, mod.V, mod.b)]
    f1, f2 = x2.flatten(1).clone().requires_grad_(True), x1.flatten(1).clone().requires_grad_(True)
    ref = M.mim(f1, f2, *prm)
    (ref * gy).sum().backward()
    assert tuple(out.shape) == (B, D) and torch.equal(out, ref)
    assert tuple(a1.grad.shape) == (B, 2, 5) and torch.equal(a1.grad.flatten(1), f2.grad)
    assert tuple(a2.grad.shape) == (B, 3, 4) and torch.equal(a2.grad.flatten(1), f1.grad)
    for p, q in zip(mod.parameters(), prm):
        assert torch.equal(p.grad, q.grad)
    with pytest.raises(L.DynmmHipError, match='W must be'):                     # unflipped, the widths do not fit W
        I.MultiplicativeInteractions2Modal([n, m], D, 'matrix', flatten=True).cuda()([x1, x2])


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: training
# ------------------------------------------------------------------------------------------------------------------------
class _RefFusion(nn.Module):
    def __init__(self, n, m, D):
        super().__init__()
        self.W = nn.Parameter(nn.init.xavier_normal_(torch.empty(n, m, D)))
        self.U = nn.Parameter(nn.init.xavier_normal_(torch.empty(n, D)))
        self.V = nn.Parameter(nn.init.xavier_normal_(torch.empty(m, D)))
        self.b = nn.Parameter(nn.init.normal_(torch.empty(D)))

    def forward(self, zs):
        return mim_ref(zs[0], zs[1], self.W, self.U, self.V, self.b)


@pytest.mark.gpu
def test_imdb_mim_train_step_against_oracle():
    """Two steps at batch 128 with output_dim 32: BatchNorm in training mode, dropout p = 0.3 with injected keep flags."""
    from dynmm_amd import ops_seq as S
    from tests import imdb_oracle as IO
    torch.manual_seed(5)
    mine, _ = E.imdb_mm_mim(output_dim=32)
    ref = IO.MMDL([IO.MaxOut_MLP(512, 512, 300, linear_layer=False, tag='encoders.0'),
                   IO.MaxOut_MLP(512, 1024, 4096, 512, False, tag='encoders.1')], _RefFusion(512, 512, 32), IO.Linear(32, 23))
    randomize_bn(ref, 3)
    mine.load_state_dict(ref.state_dict(), strict=True)
    mine, ref = mine.cuda().train(), ref.double().train()
    B, lr, wd = 128, 1e-3, 1e-2
    step = E.ExpertTrainStep(mine, 'bce', lr=lr, weight_decay=wd)
    params_r = list(ref.parameters())
    opt = torch.optim.AdamW(params_r, lr=lr, weight_decay=wd)
    names = [n for n, _ in ref.named_parameters()]
    table = {}
    prev = S.MASKS
    S.MASKS = lambda name, shape: table.get(name)
    try:
        for it in range(2):
            g = torch.Generator().manual_seed(20 + it)
            x = [torch.randn(B, 300, generator=g), torch.rand(B, 4096, generator=g)]
            y = (torch.rand(B, 23, generator=g) < 0.3).float()
            table.clear()
            IO.MASKS.clear()
            for name, m in mine.named_modules():
                if isinstance(m, I.MaxOut_MLP):
                    for site, width in (('op2', m.op2[0].num_features), ('op4', m.op4[0].num_features)):
                        k = (torch.rand(B, width, generator=g) >= 0.3).to(torch.uint8)
                        IO.MASKS[f'{name}.{site}'] = k
                        table[f'{name}.{site}'] = k.cuda()
            assert len(table) == 4
            last = step([t.cuda() for t in x], y.cuda())
            opt.zero_grad()
            loss_r = nn.functional.binary_cross_entropy_with_logits(ref([t.double() for t in x]), y.double())
            loss_r.backward()
            gn = torch.nn.utils.clip_grad_norm_(params_r, 8.0)
            opt.step()
            print(f'FIG imdb_mim step {it} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} '
                  f'norm={last["grad_norm"].item():.6f} ref={gn.item():.6f}')
            tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
            assert abs(last['loss'].item() - loss_r.item()) < tol, (it, last['loss'].item(), loss_r.item())
            assert abs(last['grad_norm'].item() - gn.item()) < 1e-3 * gn.item(), (it, last['grad_norm'].item(), gn.item())
    finally:
        S.MASKS = prev
        IO.MASKS.clear()
    torch.cuda.synchronize()
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, 'imdb_mim', names)
    sd, sd_r = mine.state_dict(), ref.state_dict()
    for k in sd:
        if 'running_' in k:
            a, b = sd[k].cpu().double(), sd_r[k].double()
            assert ((a - b).abs().max() / b.abs().max()).item() < 1e-4, k
        if 'num_batches_tracked' in k:
            assert int(sd[k]) == int(sd_r[k]) == 2, k


@pytest.mark.gpu
def test_experts_train_writes_mim(tmp_path):
    from dynmm_amd import imdb, imdb_mm
    torch.manual_seed(0)
    dev = torch.device('cuda')
    loaders = [imdb.Loader(*imdb.synthetic_split(n, s), 32, shuffle=(k == 0), device=dev) for k, (n, s) in
               enumerate([(64, 1), (32, 2)])]
    model, lr = E.imdb_mm_mim(output_dim=32)
    model = model.to(dev)
    path = imdb_mm.file_name(str(tmp_path), 3)
    history, stopper, best = E.train(model, loaders, lambda x: x, 'bce', lr, imdb_mm.WD, 2, lambda: E.save_state(model, path))
    assert len(history) == 2 and all(h == h and abs(h) < float('inf') for h in history)
    assert path.endswith('/best_mim.pt')
    assert best is not None and os.path.exists(path)
    fresh, _ = E.imdb_mm_mim(output_dim=32)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    micro, macro, loss = E.evaluate_multilabel(fresh.to(dev), loaders[1], lambda x: x)
    assert all(v == v and abs(v) < float('inf') for v in (micro, macro, loss)), (micro, macro, loss)


@pytest.mark.gpu
def test_full_size_expert_takes_two_steps():
    """the 269 M-element flat parameter / gradient / moment buffers through clip_grad_norm and AdamW"""
    torch.manual_seed(1)
    with torch.device('cuda'):
        model, lr = E.imdb_mm_mim()              # W is initialised on the device
    model.train()
    step = E.ExpertTrainStep(model, 'bce', lr=lr, weight_decay=1e-2)
    assert step.flat_g.numel() > 268_000_000
    g = torch.Generator().manual_seed(3)
    x = [torch.randn(128, 300, generator=g).cuda(), torch.rand(128, 4096, generator=g).cuda()]
    y = (torch.rand(128, 23, generator=g) < 0.3).float().cuda()
    w0 = model.fuse.W.detach()[-1, -1].clone()
    for it in range(2):
        last = step(x, y)
        loss, norm = last['loss'].item(), last['grad_norm'].item()
        print(f'FIG imdb_mim full step {it} loss={loss:.6f} norm={norm:.6f}')
        assert loss == loss and abs(loss) < float('inf') and norm == norm and 0 < norm < float('inf')
    step.opt.check_finite()
    assert not torch.equal(model.fuse.W.detach()[-1, -1], w0)                    # the update reached the end of the largest tensor

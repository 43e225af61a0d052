"""Low-rank tensor fusion on the HIP path: ops_seq.lrtf (csrc/lrtf.hip), nn.affect.LowRankTensorFusion / GRUWithLinear and the
builders experts.affect_mm_lrtf / imdb_mm_lrtf.

The yardstick is `lrtf_ref` below: MultiBench's fusions.common_fusions.LowRankTensorFusion.forward as MultiBench writes it (cat
the ones, matmul with the factor, running product, matmul with the fusion weights, bias), in plain torch; in float64 it equals
the closed form of DESIGN.md section 7j to 1e-12 (first test).  Bars are the sequence kernels' (tests/test_seq_kernels.py,
tests/test_gru.py): _rel = max|a - b| / max|b| against float64, forward 1e-5, every gradient 2e-5; a case that does not sit under
its bar is held to max(project bar, 4 x the error of lrtf_ref in float32 on the CPU on the same inputs) and marked RAISED in
its FIG line.  Measured on an MI355X over every case below: the kernels at most 8.2e-7 (dF1 at 128 x [512, 512] x 512, R = 16),
lrtf_ref in float32 on the CPU at most 4.2e-6 (dw, same case); no case needed a raised bar.
"""
import pytest
import torch
import torch.nn as nn

from dynmm_amd import experts as E
from dynmm_amd import lib as L
from dynmm_amd import ops_seq as S
from dynmm_amd.nn import affect as A
from dynmm_amd.nn import imdb as I
from tests.parity import Masks as _Masks, check_adam_params, compare_to_float64, randomize_bn, rel as _rel
from tests.test_gru import _RefMLP, _batch, _lengths, gru_ref

FWD, BWD = 1e-5, 2e-5                         # test_seq_kernels.py: LN_FWD, LN_BWD

# (B, dims, O, R)
SHAPES = [(1, (3, 5), 4, 1), (5, (7, 3, 9), 20, 3), (17, (32, 32, 128), 128, 32), (33, (64, 48), 72, 5),
          (130, (512, 512), 512, 8), (128, (512, 512), 512, 16)]
FULL = (128, (512, 512), 512, 128)
INITS = ('unit', 'xavier')


def lrtf_ref(zs, factors, fusion_weights, fusion_bias):
    """fusions.common_fusions.LowRankTensorFusion.forward (flatten=True)."""
    B, O = zs[0].shape[0], fusion_bias.shape[1]
    fused = 1
    for z, factor in zip(zs, factors):
        ones = torch.ones(B, 1, dtype=z.dtype, device=z.device)
        with_ones = torch.cat((ones, torch.flatten(z, start_dim=1)), dim=1)
        fused = fused * torch.matmul(with_ones, factor)                         # [R, B, O]
    out = torch.matmul(fusion_weights, fused.permute(1, 0, 2)).squeeze() + fusion_bias
    return out.view(-1, O)


def closed_form(zs, factors, fusion_weights, fusion_bias):
    prod = 1
    for z, f in zip(zs, factors):
        prod = prod * (f[:, 0, :].unsqueeze(1) + torch.einsum('bk,rko->rbo', z, f[:, 1:, :]))
    return torch.einsum('r,rbo->bo', fusion_weights[0], prod) + fusion_bias


def _names(M):
    return ['out'] + [f'dz{m}' for m in range(M)] + [f'dF{m}' for m in range(M)] + ['dw', 'dbias']


def _case(shape, init):
    """float64 masters of a case: unit-normal inputs and upstream gradient, parameters by `init`"""
    B, dims, O, R = shape
    g = torch.Generator().manual_seed(100 + B + 7 * O + 13 * R + len(dims) + (init == 'xavier'))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)            # noqa: E731
    zs = [rn(B, d) for d in dims]
    if init == 'unit':
        fs = [rn(R, d + 1, O) / (d + 1) ** 0.5 for d in dims]
        w, bias = rn(1, R) / R ** 0.5, 0.1 * rn(1, O)
    else:
        torch.manual_seed(int(g.initial_seed()))
        m = A.LowRankTensorFusion(list(dims), O, R)
        fs = [f.detach().double() for f in m.factors]
        w, bias = m.fusion_weights.detach().double(), m.fusion_bias.detach().double()
    return {'zs': zs, 'fs': fs, 'w': w, 'bias': bias, 'g': rn(B, O)}


def _run(fn, c, dtype, device='cpu', need_z=True, need_p=True):
    cast = lambda t, need: t.to(device=device, dtype=dtype).clone().requires_grad_(need)       # noqa: E731
    zs = [cast(t, need_z) for t in c['zs']]
    fs = [cast(t, need_p) for t in c['fs']]
    w, bias = cast(c['w'], need_p), cast(c['bias'], need_p)
    out = fn(zs, fs, w, bias)
    (out * c['g'].to(device=device, dtype=dtype)).sum().backward()
    M = len(zs)
    vals = [out] + [z.grad for z in zs] + [f.grad for f in fs] + [w.grad, bias.grad]
    return {k: (None if v is None else v.detach().cpu()) for k, v in zip(_names(M), vals)}


_REF = {}


def _ref(shape, init):
    """(case, float64 results, float32 results) of lrtf_ref on the CPU, computed once and shared"""
    key = (shape, init)
    if key not in _REF:
        c = _case(shape, init)
        _REF[key] = (c, _run(lrtf_ref, c, torch.float64), _run(lrtf_ref, c, torch.float32))
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, (7, 3), 6, 4), (5, (7, 3, 9), 20, 3)], ids=['M2', 'M3'])
def test_restatement_equals_the_closed_form_in_float64(shape):
    c = _case(shape, 'unit')
    a, b = _run(lrtf_ref, c, torch.float64), _run(closed_form, c, torch.float64)
    for k in a:
        assert _rel(a[k], b[k]) < 1e-12, k


def test_restatement_in_float32_is_well_under_the_bars():
    for shape in SHAPES[:4]:
        for init in INITS:
            _, r64, r32 = _ref(shape, init)
            for k in r64:
                assert _rel(r32[k], r64[k]) < 0.25 * (FWD if k == 'out' else BWD), (shape, init, k)


def test_parameters_are_registered_named_shaped_and_initialised():
    torch.manual_seed(2)
    m = A.LowRankTensorFusion([31, 5, 9], 64, 8)
    assert list(m.state_dict()) == ['factors.0', 'factors.1', 'factors.2', 'fusion_weights', 'fusion_bias']
    assert isinstance(m.factors, nn.ParameterList) and len(list(m.parameters())) == 5
    assert [tuple(v.shape) for v in m.state_dict().values()] == [(8, 32, 64), (8, 6, 64), (8, 10, 64), (1, 8), (1, 64)]
    assert set(dict(m.named_parameters())) == set(m.state_dict())
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    assert torch.count_nonzero(m.fusion_bias) == 0
    for f in m.factors:
        fan_in, fan_out = nn.init._calculate_fan_in_and_fan_out(f)
        assert (fan_in, fan_out) == (f.shape[1] * 64, 8 * 64)
        want = (2.0 / (fan_in + fan_out)) ** 0.5
        assert abs(f.std().item() - want) < 0.1 * want and abs(f.mean().item()) < 0.1 * want
    assert I.LowRankTensorFusion is A.LowRankTensorFusion


def test_state_dicts_load_strictly_from_plain_torch_holders():
    class Fusion(nn.Module):
        def __init__(self):
            super().__init__()
            self.factors = nn.ParameterList([nn.Parameter(torch.randn(4, d + 1, 6)) for d in (3, 5)])
            self.fusion_weights = nn.Parameter(torch.randn(1, 4))
            self.fusion_bias = nn.Parameter(torch.randn(1, 6))

    class Encoder(nn.Module):
        def __init__(self):
            super().__init__()
            self.gru = nn.GRU(35, 64)
            self.linear = nn.Linear(64, 32)
            self.dropout_layer = nn.Dropout(0.1)

    h, m = Fusion(), A.LowRankTensorFusion([3, 5], 6, 4)
    m.load_state_dict(h.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), h.parameters()))
    h, m = Encoder(), A.GRUWithLinear(35, 64, 32, dropout=True, has_padding=True)
    assert sorted(m.state_dict()) == ['gru.bias_hh_l0', 'gru.bias_ih_l0', 'gru.weight_hh_l0', 'gru.weight_ih_l0', 'linear.bias',
                                      'linear.weight']
    m.load_state_dict(h.state_dict(), strict=True)
    assert torch.equal(m.gru.weight_hh_l0, h.gru.weight_hh_l0) and torch.equal(m.linear.weight, h.linear.weight)
    assert isinstance(m.dropout_layer, nn.Dropout) and m.dropout_layer.p == 0.1


def test_builders_have_the_reference_dimensions(tmp_path):
    from dynmm_amd import affect_mm, imdb_mm
    m = E.affect_mm_lrtf()
    assert [(e.gru.input_size, e.gru.hidden_size, e.linear.out_features) for e in m.encoders] == \
        [(35, 64, 32), (74, 128, 32), (300, 512, 128)]
    assert all(isinstance(e, A.GRUWithLinear) and e.has_padding and e.dropout and e.dropout_layer.p == 0.1 for e in m.encoders)
    assert isinstance(m.fuse, A.LowRankTensorFusion) and m.has_padding
    assert [tuple(f.shape) for f in m.fuse.factors] == [(32, 33, 128), (32, 33, 128), (32, 129, 128)]
    assert tuple(m.fuse.fusion_weights.shape) == (1, 32) and tuple(m.fuse.fusion_bias.shape) == (1, 128)
    assert (m.head.fc.in_features, m.head.fc.out_features, m.head.fc2.out_features) == (128, 512, 1)
    assert not any(isinstance(x, nn.BatchNorm1d) for x in m.modules())
    assert affect_mm.file_names(str(tmp_path), 5)[0].endswith('/lrtf.pt')
    m, lr = E.imdb_mm_lrtf()
    assert lr == 8e-3
    assert [(e.op0.num_features, e.op1.d_out, e.op3.d_out, e.hid2val) for e in m.encoders] == \
        [(300, 512, 512, None), (4096, 1024, 512, None)]
    assert [e.tag for e in m.encoders] == ['encoders.0', 'encoders.1']
    assert isinstance(m.fuse, A.LowRankTensorFusion)
    assert [tuple(f.shape) for f in m.fuse.factors] == [(128, 513, 512), (128, 513, 512)]
    assert (m.head.fc.in_features, m.head.fc.out_features) == (512, 23)
    assert imdb_mm.file_name(str(tmp_path), 2).endswith('/best_lrtf.pt')
    assert E.affect_mm_lrtf(rank=4).fuse.rank == 4 and E.imdb_mm_lrtf(rank=16)[0].fuse.rank == 16
    assert 'fuse.factors.2' in E.affect_mm_lrtf().state_dict()


def test_the_pinned_refusals_still_raise():
    with pytest.raises(NotImplementedError, match='LowRankTensorFusion'):
        E.imdb_mm(2)
    with pytest.raises(NotImplementedError, match='GRU'):
        E.affect_mm(5)
    with pytest.raises(NotImplementedError, match='LowRankTensorFusion'):
        E.affect_mm_gru(5)


def test_what_the_kernels_do_not_serve_is_refused():
    with pytest.raises(NotImplementedError):
        A.LowRankTensorFusion([3, 5], 6, 4, flatten=False)
    for dims in ([3], [3, 4, 5, 6]):
        with pytest.raises(NotImplementedError):
            A.LowRankTensorFusion(dims, 6, 4)
        zs = [torch.randn(2, d) for d in dims]
        fs = [torch.randn(4, d + 1, 6) for d in dims]
        with pytest.raises(L.DynmmHipError, match='M = '):
            S.lrtf(zs, fs, torch.randn(1, 4), torch.randn(1, 6))


def test_cpu_tensors_are_refused():
    m = A.LowRankTensorFusion([3, 5], 6, 4)
    with pytest.raises(L.DynmmHipError):
        m([torch.randn(2, 3), torch.randn(2, 5)])
    with pytest.raises(L.DynmmHipError):
        A.GRUWithLinear(3, 16, 4, has_padding=True)([torch.randn(2, 4, 3), torch.tensor([4, 1])])
    with pytest.raises(L.DynmmHipError):
        A.GRUWithLinear(3, 16, 4)(torch.randn(2, 4, 3))


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the op
# ------------------------------------------------------------------------------------------------------------------------
def _ids(s):
    return f'{s[0]}x{"-".join(map(str, s[1]))}x{s[2]}x{s[3]}'


@pytest.mark.gpu
@pytest.mark.parametrize('init', INITS)
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_lrtf_against_float64(shape, init):
    c, r64, r32 = _ref(shape, init)
    compare_to_float64(f'{_ids(shape)} {init}', _run(S.lrtf, c, torch.float32, 'cuda'), r64, r32, ('out',), FWD, BWD)


@pytest.mark.gpu
def test_lrtf_at_the_full_mm_imdb_geometry():
    c = _case(FULL, 'unit')
    r64 = _run(lrtf_ref, c, torch.float64)
    r32 = _run(lrtf_ref, c, torch.float32)
    compare_to_float64(f'{_ids(FULL)} unit', _run(S.lrtf, c, torch.float32, 'cuda'), r64, r32, ('out',), FWD, BWD)


@pytest.mark.gpu
def test_partial_requires_grad_skips_work_and_changes_no_bit():
    c = _ref(SHAPES[3], 'unit')[0]
    M = len(c['zs'])
    both = _run(S.lrtf, c, torch.float32, 'cuda')
    only_p = _run(S.lrtf, c, torch.float32, 'cuda', need_z=False)
    only_z = _run(S.lrtf, c, torch.float32, 'cuda', need_p=False)
    for k in _names(M):
        is_z = k.startswith('dz')
        if k == 'out':
            assert torch.equal(only_p[k], both[k]) and torch.equal(only_z[k], both[k])
        else:
            assert only_p[k] is None if is_z else torch.equal(only_p[k], both[k]), k
            assert torch.equal(only_z[k], both[k]) if is_z else only_z[k] is None, k
    # one input alone
    zs = [t.float().cuda().requires_grad_(m == 1) for m, t in enumerate(c['zs'])]
    out = S.lrtf(zs, [t.float().cuda() for t in c['fs']], c['w'].float().cuda(), c['bias'].float().cuda())
    (out * c['g'].float().cuda()).sum().backward()
    assert zs[0].grad is None and torch.equal(zs[1].grad.cpu(), both['dz1'])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [SHAPES[3], SHAPES[4]], ids=_ids)
def test_two_calls_give_the_same_bits(shape):
    c = _ref(shape, 'unit')[0]
    a, b = _run(S.lrtf, c, torch.float32, 'cuda'), _run(S.lrtf, c, torch.float32, 'cuda')
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_operands_the_kernels_cannot_read_are_refused():
    zs = [torch.randn(4, 3, device='cuda'), torch.randn(4, 5, device='cuda')]
    fs = [torch.randn(2, 4, 6, device='cuda'), torch.randn(2, 6, 6, device='cuda')]
    w, b = torch.randn(1, 2, device='cuda'), torch.randn(1, 6, device='cuda')
    assert tuple(S.lrtf(zs, fs, w, b).shape) == (4, 6)
    with pytest.raises(L.DynmmHipError, match='float32'):
        S.lrtf([zs[0].double(), zs[1]], fs, w, b)
    with pytest.raises(L.DynmmHipError, match='contiguous'):
        S.lrtf([torch.randn(3, 4, device='cuda').t(), zs[1]], fs, w, b)
    with pytest.raises(L.DynmmHipError, match='contiguous'):
        S.lrtf(zs, [torch.randn(2, 6, 4, device='cuda').transpose(1, 2), fs[1]], w, b)
    with pytest.raises(L.DynmmHipError, match='factors'):
        S.lrtf(zs, [fs[0], fs[0]], w, b)
    with pytest.raises(L.DynmmHipError):
        S.lrtf(zs, fs, w.cpu(), b)


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the modules
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('with_len', [True, False], ids=['lengths', 'full'])
def test_gru_with_linear_against_float64(with_len, train):
    B, T, F, H, Od, p = 5, 7, 35, 64, 32, 0.1
    torch.manual_seed(6)
    m = A.GRUWithLinear(F, H, Od, dropout=True, dropoutp=p, has_padding=with_len)
    prm = [t.detach().double().clone().requires_grad_(True) for t in
           (m.gru.weight_ih_l0, m.gru.weight_hh_l0, m.gru.bias_ih_l0, m.gru.bias_hh_l0, m.linear.weight, m.linear.bias)]
    m = m.cuda().train(train)
    x64 = torch.randn(B, T, F, dtype=torch.float64)
    ln = _lengths(B, T, 5)
    hshape = (B, H) if with_len else (B, T, H)
    keep = torch.rand(hshape, generator=torch.Generator().manual_seed(9)) >= p
    gy = torch.randn(hshape[:-1] + (Od,), dtype=torch.float64)
    calls = []

    def masks(name, shp):
        calls.append((name, shp))
        return keep.to(torch.uint8).cuda() if name == 'gru_dropout' else None

    xr = x64.clone().requires_grad_(True)
    hn, seq = gru_ref(xr, *prm[:4], ln if with_len else None)
    hidden = hn if with_len else seq
    if train:
        hidden = hidden * keep.double() / (1 - p)
    ref = hidden @ prm[4].t() + prm[5]
    (ref * gy).sum().backward()
    x = x64.float().cuda().requires_grad_(True)
    prev, S.MASKS = S.MASKS, masks
    try:
        out = m([x, ln] if with_len else x)
        (out * gy.float().cuda()).sum().backward()
    finally:
        S.MASKS = prev
    assert calls == ([('gru_dropout', hshape)] if train else [])
    assert tuple(out.shape) == tuple(ref.shape)
    tag = f'GRUWithLinear {"len" if with_len else "full"} {"train" if train else "eval"}'
    e = _rel(out, ref)
    print(f'FIG {tag} out kernel={e:.3e} bar={FWD:.3e}')
    assert e < FWD
    g = m.gru
    got = (x.grad, g.weight_ih_l0.grad, g.weight_hh_l0.grad, g.bias_ih_l0.grad, g.bias_hh_l0.grad, m.linear.weight.grad,
           m.linear.bias.grad)
    for name, a, b in zip(('dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh', 'dW_lin', 'db_lin'), got, (xr.grad, *[t.grad for t in prm])):
        e = _rel(a, b)
        print(f'FIG {tag} {name} kernel={e:.3e} bar={BWD:.3e}')
        assert e < BWD, name


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: training
# ------------------------------------------------------------------------------------------------------------------------
class _RefFusion(nn.Module):
    def __init__(self, dims, O, R):
        super().__init__()
        self.factors = nn.ParameterList([nn.Parameter(nn.init.xavier_normal_(torch.empty(R, d + 1, O))) for d in dims])
        self.fusion_weights = nn.Parameter(nn.init.xavier_normal_(torch.empty(1, R)))
        self.fusion_bias = nn.Parameter(torch.zeros(1, O))

    def forward(self, zs):
        return lrtf_ref(zs, list(self.factors), self.fusion_weights, self.fusion_bias)


class _RefGRUWithLinear(nn.Module):
    masks = None                 # callable(name, shape) -> keep flags, or None (dropout off)

    def __init__(self, F, H, Od, p=0.1):
        super().__init__()
        self.gru, self.linear, self.p = nn.GRU(F, H), nn.Linear(H, Od), p

    def forward(self, x):
        g = self.gru
        h = gru_ref(x[0], g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, x[1])[0]
        if self.training and _RefGRUWithLinear.masks is not None:
            h = h * _RefGRUWithLinear.masks('gru_dropout', tuple(h.shape)).to(h.dtype) / (1 - self.p)
        return self.linear(h)


class _RefMosei(nn.Module):
    def __init__(self, rank=32):
        super().__init__()
        self.encoders = nn.ModuleList([_RefGRUWithLinear(35, 64, 32), _RefGRUWithLinear(74, 128, 32),
                                       _RefGRUWithLinear(300, 512, 128)])
        self.fuse = _RefFusion([32, 32, 128], 128, rank)
        self.head = _RefMLP(128, 512, 1)

    def forward(self, inputs):
        return self.head(self.fuse([e([inputs[0][i], inputs[1][i]]) for i, e in enumerate(self.encoders)]))


@pytest.mark.gpu
def test_affect_lrtf_train_step_against_oracle():
    """Two steps in training mode, dropout p = 0.1 on every encoder's h_n with the same keep flags on both sides."""
    from oracle import affect_oracle as O
    torch.manual_seed(12)
    ref, mine = _RefMosei(), E.affect_mm_lrtf()
    mine.load_state_dict(ref.state_dict(), strict=True)
    ref, mine = ref.double().train(), mine.cuda().train()
    lr, wd = 1e-3, 1e-2
    step = E.ExpertTrainStep(mine, 'l1', lr=lr, weight_decay=wd)
    params_r = list(ref.parameters())
    opt = torch.optim.AdamW(params_r, lr=lr, weight_decay=wd)
    names = [n for n, _ in ref.named_parameters()]
    prev = S.MASKS
    try:
        for it in range(2):
            inputs, y = O.synth_batch(6, seed=10 + it)
            mr, mh = _Masks(0.1, 40 + it), _Masks(0.1, 40 + it, 'cuda')
            _RefGRUWithLinear.masks, S.MASKS = mr, mh
            opt.zero_grad()
            loss_r = nn.functional.l1_loss(ref([[x.double() for x in inputs[0]], inputs[1]]), y.double())
            loss_r.backward()
            gn = torch.nn.utils.clip_grad_norm_(params_r, 8.0)
            opt.step()
            last = step([[x.cuda() for x in inputs[0]], inputs[1]], y.cuda())
            torch.cuda.synchronize()
            assert mr.n == mh.n == 3
            print(f'FIG affect_lrtf step {it} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} '
                  f'norm={last["grad_norm"].item():.6f} ref={gn.item():.6f}')
            tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
            assert abs(last['loss'].item() - loss_r.item()) < tol, (it, last['loss'].item(), loss_r.item())
            assert abs(last['grad_norm'].item() - gn.item()) < 2e-3 * max(gn.item(), 1e-3), (it, last['grad_norm'].item(), gn.item())
    finally:
        _RefGRUWithLinear.masks, S.MASKS = None, prev
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, 'affect_lrtf', names)


@pytest.mark.gpu
def test_imdb_lrtf_train_step_against_oracle():
    """Two steps at batch 128 with rank 16: BatchNorm in training mode, dropout p = 0.3 with injected keep flags."""
    from tests import imdb_oracle as IO
    torch.manual_seed(5)
    mine, _ = E.imdb_mm_lrtf(rank=16)
    ref = IO.MMDL([IO.MaxOut_MLP(512, 512, 300, linear_layer=False, tag='encoders.0'),
                   IO.MaxOut_MLP(512, 1024, 4096, 512, False, tag='encoders.1')], _RefFusion([512, 512], 512, 16),
                  IO.Linear(512, 23))
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
            print(f'FIG imdb_lrtf step {it} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} '
                  f'norm={last["grad_norm"].item():.6f} ref={gn.item():.6f}')
            tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
            assert abs(last['loss'].item() - loss_r.item()) < tol, (it, last['loss'].item(), loss_r.item())
            assert abs(last['grad_norm'].item() - gn.item()) < 1e-3 * gn.item(), (it, last['grad_norm'].item(), gn.item())
    finally:
        S.MASKS = prev
        IO.MASKS.clear()
    torch.cuda.synchronize()
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, 'imdb_lrtf', names)
    sd, sd_r = mine.state_dict(), ref.state_dict()
    for k in sd:
        if 'running_' in k:
            a, b = sd[k].cpu().double(), sd_r[k].double()
            assert ((a - b).abs().max() / b.abs().max()).item() < 1e-4, k
        if 'num_batches_tracked' in k:
            assert int(sd[k]) == int(sd_r[k]) == 2, k


@pytest.mark.gpu
def test_affect_lrtf_graph_replay_equals_eager():
    """ExpertTrainStep(use_graph=True) on the MOSEI model (no BatchNorm; dropout off on both copies: their sites differ), device
    lengths that change at every step."""
    torch.manual_seed(5)
    a, b = E.affect_mm_lrtf().cuda().eval(), E.affect_mm_lrtf().cuda().eval()
    b.load_state_dict(a.state_dict())
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = _batch(8, 6, 30 + it)
        x = [[t.cuda() for t in inputs[0]], [t.cuda() for t in inputs[1]]]
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert abs(sa.loss_acc.item() - sb.loss_acc.item()) <= 1e-6 * sa.loss_acc.item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k
    inputs, y = _batch(8, 6, 40)
    sc = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    with pytest.raises(ValueError, match='lengths'):
        sc([[t.cuda() for t in inputs[0]], inputs[1]], y.cuda())
    assert not torch.cuda.is_current_stream_capturing()


@pytest.mark.gpu
def test_experts_train_writes_lrtf(tmp_path):
    from dynmm_amd import affect, affect_mm
    torch.manual_seed(0)
    dev = torch.device('cuda')
    loaders = [affect.Loader(*affect.synthetic_split(n, s), 32, shuffle=(k == 0), device=dev) for k, (n, s) in
               enumerate([(64, 1), (32, 2)])]
    model = E.affect_mm_lrtf().to(dev)
    path = affect_mm.file_names(str(tmp_path), 5)[0]
    history, stopper, best = E.train(model, loaders, lambda x: x, 'l1', 1e-3, 1e-2, 2, lambda: E.save_state(model, path),
                                     protocol='mm')
    assert len(history) == 2 and all(h == h and abs(h) < float('inf') for h in history)
    fresh = E.affect_mm_lrtf()
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    r = E.evaluate_posneg(fresh.to(dev), loaders[1], lambda x: x)
    # (Corr is NaN by definition while every prediction has one sign, which two epochs from the xavier start do not change)
    assert all(r[k] == r[k] and abs(r[k]) < float('inf') for k in ('Accuracy', 'Loss')), r

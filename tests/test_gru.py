"""The GRU experts of the modality-level DynMM (csrc/gru.hip, ops_seq.gru_seq, nn.affect.GRU, experts.affect_uni_gru /
affect_mm_gru) against a float64 restatement of torch.nn.GRU.

The yardstick is `gru_ref` below: the recurrence of torch.nn.GRU (one layer, one direction, batch_first, h0 = 0, gate order
r | z | n) with the length mask of pack_padded_sequence, in plain torch on the CPU.  Without a GPU it is compared with
torch.nn.GRU itself (packed and unpacked) in float64: h_n, the sequence and the gradients of x and the four parameters agree
to < 1e-12.  Every GPU comparison is against this restatement in float64, with torch's default initialisation and unit-normal
inputs.

Bars.  `_rel` = max |a - b| / max |b| (denominator clamped at 1e-30, so a quantity that is identically zero — dW_hh of a
one-step sequence — must come out as exact zeros).  Forward 1e-5, gradients 2e-5: the project's LayerNorm / attention bars.
Should a case not sit under them, test_seq_kernels.py's rule applies: bar = max(project bar, 4 x the error of the SAME
restatement in float32 on the CPU on the same inputs).  Every comparison prints `FIG <case> kernel=<err> f32=<yardstick>
bar=<bar>` and marks a case above the project bar RAISED.  On an MI355X no case was raised: the largest error of any quantity
on any shape and arm was 9.9e-7 (the float32 restatement: up to 6.6e-7).

Shapes (B, T, F, H), each on both dispatch arms and with / without lengths:
  (1, 1, 3, 16)      one step: dW_hh identically zero, written as zeros
  (5, 7, 35, 20)     H no tile multiple, batch smaller than a tile
  (17, 9, 74, 64)    the batch crosses a tile; W_hh resident in LDS
  (33, 6, 10, 128)   W_hh no longer fits LDS (streamed)
  (3, 4, 5, 272)     resident arm: 17 unit tiles over 16 waves (a wave owns two tiles), 68 k-steps per tile
  (18, 3, 5, 40)     stepped arm: 3 unit-tile workgroups x 2 sample tiles, 12 k-steps = 3 per wave of the 4-way K split
  (32, 50, 300, 512) the text expert's own geometry, once on the automatic arm
"""
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from dynmm_amd import experts as E
from dynmm_amd import lib as L
from dynmm_amd import ops_seq as S
from dynmm_amd.nn import affect as A
from tests.parity import check_adam_params, compare_to_float64, rel as _rel

FWD, BWD = 1e-5, 2e-5                         # test_seq_kernels.py: LN_FWD, LN_BWD
NAMES = ('h_n', 'seq', 'dx', 'dW_ih', 'dW_hh', 'db_ih', 'db_hh')

SHAPES = [(1, 1, 3, 16), (5, 7, 35, 20), (17, 9, 74, 64), (33, 6, 10, 128), (3, 4, 5, 272), (18, 3, 5, 40)]
BIG = (32, 50, 300, 512)


def gru_ref(x, w_ih, w_hh, b_ih, b_hh, lengths=None):
    """(h_n [B, H], states [B, T, H]): sample b updates while t < lengths[b] and holds its state afterwards."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(B, H)
    seq = []
    for t in range(T):
        gi = x[:, t] @ w_ih.t() + b_ih
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        new = (1 - z) * n + z * h
        if lengths is not None:
            m = (t < lengths).to(x.dtype).unsqueeze(1)
            new = m * new + (1 - m) * h
        h = new
        seq.append(h)
    return h, torch.stack(seq, 1)


def _lengths(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(1, T + 1, (B,), generator=g)
    ln[0] = T
    if B > 1:
        ln[1] = 1
    return ln


def _case(shape, with_len):
    """inputs of a case (float64 masters): x, the four parameters (torch's default initialisation), lengths, output gradients"""
    B, T, F, H = shape
    torch.manual_seed(1000 + B + 10 * T + 100 * H)
    g = nn.GRU(F, H, batch_first=True)
    p = [t.detach().double() for t in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
    x = torch.randn(B, T, F, dtype=torch.float64)
    return {'x': x, 'p': p, 'len': _lengths(B, T, 7 + B) if with_len else None,
            'gn': torch.randn(B, H, dtype=torch.float64), 'gs': torch.randn(B, T, H, dtype=torch.float64)}


def _run(fn, c, dtype, device='cpu'):
    """the 7 compared quantities of `fn` (gru_ref or S.gru_seq) on the case's inputs in `dtype` on `device`"""
    x = c['x'].to(device=device, dtype=dtype).clone().requires_grad_(True)
    w_ih, w_hh, b_ih, b_hh = (t.to(device=device, dtype=dtype).clone().requires_grad_(True) for t in c['p'])
    ln = c['len']
    hn, seq = fn(x, w_ih, w_hh, b_ih, b_hh, None if ln is None else ln.to(device))
    loss = (hn * c['gn'].to(device=device, dtype=dtype)).sum()
    if ln is None:
        loss = loss + (seq * c['gs'].to(device=device, dtype=dtype)).sum()      # a gradient into every step
    loss.backward()
    out = {'h_n': hn, 'seq': seq, 'dx': x.grad, 'dW_ih': w_ih.grad, 'dW_hh': w_hh.grad, 'db_ih': b_ih.grad, 'db_hh': b_hh.grad}
    return {k: (None if v is None else v.detach().cpu()) for k, v in out.items()}


_REF, _GPU = {}, {}


def _ref(shape, with_len):
    """(float64, float32) restatement results of a case, computed once and shared"""
    key = (shape, with_len)
    if key not in _REF:
        c = _case(shape, with_len)
        _REF[key] = (c, _run(gru_ref, c, torch.float64), _run(gru_ref, c, torch.float32))
    return _REF[key]


def _gpu(shape, with_len, arm):
    key = (shape, with_len, arm)
    if key not in _GPU:
        c = _ref(shape, with_len)[0]
        _GPU[key] = _run(lambda *a: S.gru_seq(*a[:5], lengths=a[5], arm=arm), c, torch.float32, 'cuda')
    return _GPU[key]


def _compare(tag, got, ref64, ref32, with_len):
    assert tuple(ref64) == NAMES
    compare_to_float64(tag, got, ref64, ref32, ('h_n', 'seq'), FWD, BWD, absent=('seq',) if with_len else ())


# ------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------------
def _torch_gru(c, packed):
    B, T, F = c['x'].shape
    H = c['p'][1].shape[1]
    g = nn.GRU(F, H, batch_first=True).double()
    with torch.no_grad():
        for dst, src in zip((g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0), c['p']):
            dst.copy_(src)
    x = c['x'].clone().requires_grad_(True)
    if packed:
        out, hn = g(pack_padded_sequence(x, c['len'], batch_first=True, enforce_sorted=False))
        loss = (hn[-1] * c['gn']).sum()
        seq = None
    else:
        seq, hn = g(x)
        loss = (hn[-1] * c['gn']).sum() + (seq * c['gs']).sum()
    loss.backward()
    return {'h_n': hn[-1], 'seq': seq, 'dx': x.grad, 'dW_ih': g.weight_ih_l0.grad, 'dW_hh': g.weight_hh_l0.grad,
            'db_ih': g.bias_ih_l0.grad, 'db_hh': g.bias_hh_l0.grad}


@pytest.mark.parametrize('with_len', [True, False])
@pytest.mark.parametrize('shape', [(5, 7, 35, 20), (17, 9, 74, 64), (1, 1, 3, 16)])
def test_restatement_equals_torch_gru_in_float64(shape, with_len):
    c, r64, _ = _ref(shape, with_len)
    t = _torch_gru(c, with_len)
    for k in NAMES:
        if t[k] is None:
            continue
        assert _rel(r64[k], t[k]) < 1e-12, (k, _rel(r64[k], t[k]))


def test_restatement_holds_the_state_of_finished_samples():
    c, r64, _ = _ref((5, 7, 35, 20), True)
    seq, ln = r64['seq'], c['len']
    g = nn.GRU(35, 20, batch_first=True).double()
    with torch.no_grad():
        for dst, src in zip((g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0), c['p']):
            dst.copy_(src)
    out, _ = pad_packed_sequence(g(pack_padded_sequence(c['x'], ln, batch_first=True, enforce_sorted=False))[0], batch_first=True)
    for b in range(5):
        n = int(ln[b])
        assert _rel(seq[b, :n], out[b, :n]) < 1e-12
        assert torch.equal(seq[b, n - 1:], seq[b, n - 1:n].expand(7 - n + 1, -1))


def test_state_dict_is_torchs_and_loads_strictly():
    m = A.GRU(35, 64, dropout=True, has_padding=True)
    sd = m.state_dict()
    ref = nn.GRU(35, 64, batch_first=True).state_dict()
    assert sorted(sd) == sorted('gru.' + k for k in ref)
    assert sorted(sd) == ['gru.bias_hh_l0', 'gru.bias_ih_l0', 'gru.weight_hh_l0', 'gru.weight_ih_l0']
    for k, v in ref.items():
        assert tuple(sd['gru.' + k].shape) == tuple(v.shape)

    class Holder(nn.Module):
        def __init__(self):
            super().__init__()
            self.gru = nn.GRU(35, 64, batch_first=True)
            self.dropout_layer = nn.Dropout(0.1)

    h = Holder()
    m.load_state_dict(h.state_dict(), strict=True)
    assert torch.equal(m.gru.weight_hh_l0, h.gru.weight_hh_l0)
    assert isinstance(m.dropout_layer, nn.Dropout) and m.dropout_layer.p == 0.1


def test_builders_have_the_reference_dimensions():
    for mod, (f, h1, h2) in enumerate([(35, 64, 32), (74, 128, 64), (300, 512, 256)]):
        enc, head, name = E.affect_uni_gru(mod)
        assert name == ('visual', 'audio', 'text')[mod]
        assert (enc.gru.input_size, enc.gru.hidden_size) == (f, h1) and enc.has_padding and enc.dropout
        assert (head.fc.in_features, head.fc.out_features, head.fc2.out_features) == (h1, h2, 1)
    enc, head, _ = E.affect_uni_gru(0, hidden_dim1=20, hidden_dim2=7)
    assert enc.gru.hidden_size == 20 and head.fc.out_features == 7
    lf = E.affect_mm_gru(1)
    assert [(e.gru.input_size, e.gru.hidden_size) for e in lf.encoders] == [(35, 64), (74, 128), (300, 512)]
    assert isinstance(lf.fuse, A.Concat) and (lf.head.fc.in_features, lf.head.fc.out_features, lf.head.fc2.out_features) == (704, 512, 1)
    ef = E.affect_mm_gru(0)
    assert all(isinstance(e, A.Identity) for e in ef.encoders) and isinstance(ef.fuse, A.ConcatEarly)
    assert (ef.head[0].gru.input_size, ef.head[0].gru.hidden_size) == (409, 512)
    assert (ef.head[1].fc.in_features, ef.head[1].fc.out_features, ef.head[1].fc2.out_features) == (512, 256, 1)
    assert sorted(ef.state_dict())[:2] == ['head.0.gru.bias_hh_l0', 'head.0.gru.bias_ih_l0']
    with pytest.raises(NotImplementedError, match='LowRankTensorFusion'):
        E.affect_mm_gru(5)
    with pytest.raises(ValueError):
        E.affect_uni_gru(3)


def test_concat_early_and_identity():
    xs = [torch.randn(2, 3, f) for f in (4, 5)]
    assert torch.equal(A.ConcatEarly()(xs), torch.cat(xs, dim=2))
    assert A.Identity()(xs) is xs and E.Identity is A.Identity


def test_cpu_tensors_are_refused():
    m = A.GRU(3, 16, has_padding=True)
    with pytest.raises(L.DynmmHipError):
        m([torch.randn(2, 4, 3), torch.tensor([4, 1])])
    with pytest.raises(L.DynmmHipError):
        A.GRU(3, 16)(torch.randn(2, 4, 3))
    with pytest.raises(ValueError):
        S.gru_seq(torch.randn(2, 4, 3), *[None] * 4, arm='fastest')


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the op
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('with_len', [True, False], ids=['lengths', 'full'])
@pytest.mark.parametrize('arm', ['resident', 'stepped'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gru_seq_against_float64(shape, arm, with_len):
    _, r64, r32 = _ref(shape, with_len)
    _compare(f'{shape} {arm} {"len" if with_len else "full"}', _gpu(shape, with_len, arm), r64, r32, with_len)


@pytest.mark.gpu
@pytest.mark.parametrize('with_len', [True, False], ids=['lengths', 'full'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_arms_agree(shape, with_len):
    B, T, _, H = shape
    assert S.gru_arm(B, H, T) in ('resident', 'stepped')
    auto, res, stp = (_gpu(shape, with_len, a) for a in (None, 'resident', 'stepped'))
    for k in NAMES:
        if res[k] is None:
            continue
        errs = _rel(res[k], stp[k]), _rel(auto[k], res[k]), _rel(auto[k], stp[k])
        print(f'FIG {shape} {k} resident-vs-stepped={errs[0]:.3e} auto-vs-resident={errs[1]:.3e} auto-vs-stepped={errs[2]:.3e}')
        assert max(errs) < (FWD if k in ('h_n', 'seq') else BWD), (k, errs)


@pytest.mark.gpu
@pytest.mark.parametrize('with_len', [True, False], ids=['lengths', 'full'])
def test_gru_seq_at_the_text_experts_geometry(with_len):
    _, r64, r32 = _ref(BIG, with_len)
    assert S.gru_arm(BIG[0], BIG[3], BIG[1]) in ('resident', 'stepped')
    _compare(f'{BIG} auto {"len" if with_len else "full"}', _gpu(BIG, with_len, None), r64, r32, with_len)


@pytest.mark.gpu
def test_resident_arm_refuses_what_it_cannot_hold():
    x = torch.randn(2, 2, 3, device='cuda')
    g = nn.GRU(3, 520, batch_first=True).cuda()
    w = (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
    with pytest.raises(L.DynmmHipError, match='EUNSUPPORTED'):
        S.gru_seq(x, *w, arm='resident')
    assert S.gru_arm(2, 520, 2) == 'stepped'
    hn, _ = S.gru_seq(x, *w)
    r, _ = gru_ref(x.double().cpu(), *[t.detach().double().cpu() for t in w])
    assert _rel(hn, r) < FWD


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: the module
# ------------------------------------------------------------------------------------------------------------------------
def _module_pair(F, H, seed, **kw):
    torch.manual_seed(seed)
    m = A.GRU(F, H, **kw)
    p = [t.detach().double() for t in (m.gru.weight_ih_l0, m.gru.weight_hh_l0, m.gru.bias_ih_l0, m.gru.bias_hh_l0)]
    return m.cuda(), p


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['has_padding', 'last_only', 'sequence'])
def test_module_dropout_with_injected_keep_flags(mode):
    B, T, F, H, p = 6, 5, 9, 24, 0.25
    m, prm = _module_pair(F, H, 3, dropout=True, dropoutp=p, has_padding=mode == 'has_padding', last_only=mode == 'last_only',
                          flatten=mode == 'sequence')
    x64 = torch.randn(B, T, F, dtype=torch.float64)
    ln = _lengths(B, T, 5)
    shape = (B, T, H) if mode == 'sequence' else (B, H)
    keep = (torch.rand(shape, generator=torch.Generator().manual_seed(9)) >= p)
    gy = torch.randn(shape, dtype=torch.float64)
    calls = []

    def masks(name, shp):
        calls.append((name, shp))
        return keep.to(torch.uint8).cuda() if name == 'gru_dropout' else None

    xr = x64.clone().requires_grad_(True)
    pr = [t.clone().requires_grad_(True) for t in prm]
    hn, seq = gru_ref(xr, *pr, ln if mode == 'has_padding' else None)
    base = seq if mode == 'sequence' else hn
    (base * keep.double() / (1 - p) * gy).sum().backward()
    x = x64.float().cuda().requires_grad_(True)
    arg = [x, ln] if mode == 'has_padding' else x
    prev, S.MASKS = S.MASKS, masks
    try:
        m.train()
        out = m(arg)
        (out * gy.float().cuda().reshape(out.shape)).sum().backward()
    finally:
        S.MASKS = prev
    assert calls == [('gru_dropout', shape)]
    assert tuple(out.shape) == ((B, T * H) if mode == 'sequence' else (B, H))
    assert _rel(out.reshape(shape), base * keep.double() / (1 - p)) < FWD
    g = m.gru
    for got, ref in zip((x.grad, g.weight_ih_l0.grad, g.weight_hh_l0.grad, g.bias_ih_l0.grad, g.bias_hh_l0.grad),
                        (xr.grad, *[t.grad for t in pr])):
        assert _rel(got, ref) < BWD
    m.eval()
    with torch.no_grad():
        assert _rel(m(arg).reshape(shape), base) < FWD


@pytest.mark.gpu
def test_frozen_gru_gives_the_same_dx_and_no_parameter_gradients():
    B, T, F, H = 5, 6, 7, 20
    m, _ = _module_pair(F, H, 4, has_padding=True)
    x0 = torch.randn(B, T, F, device='cuda')
    ln = _lengths(B, T, 2).cuda()
    gy = torch.randn(B, H, device='cuda')
    xa = x0.clone().requires_grad_(True)
    (m([xa, ln]) * gy).sum().backward()
    assert all(p.grad is not None for p in m.parameters())
    for p in m.parameters():
        p.requires_grad = False
        p.grad = None
    xb = x0.clone().requires_grad_(True)
    (m([xb, ln]) * gy).sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    assert all(p.grad is None for p in m.parameters())


# ------------------------------------------------------------------------------------------------------------------------
# with a GPU: training
# ------------------------------------------------------------------------------------------------------------------------
class _RefGRU(nn.Module):
    """MultiBench's GRU(has_padding=True) without dropout, from torch.nn.GRU itself."""

    def __init__(self, F, H):
        super().__init__()
        self.gru = nn.GRU(F, H, batch_first=True)

    def forward(self, x):
        return self.gru(pack_padded_sequence(x[0], x[1], batch_first=True, enforce_sorted=False))[1][-1]


class _RefMLP(nn.Module):
    def __init__(self, i, h, o):
        super().__init__()
        self.fc, self.fc2 = nn.Linear(i, h), nn.Linear(h, o)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc(x)))


class _RefLF(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoders = nn.ModuleList([_RefGRU(35, 64), _RefGRU(74, 128), _RefGRU(300, 512)])
        self.head = _RefMLP(704, 512, 1)

    def forward(self, inputs):
        return self.head(torch.cat([e([inputs[0][i], inputs[1][i]]) for i, e in enumerate(self.encoders)], dim=1))


def _batch(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, T, f, generator=g) for f in (35, 74, 300)]
    ln = _lengths(B, T, seed + 1)
    return [xs, [ln] * 3], torch.randn(B, 1, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['uni', 'lf_gru'])
def test_expert_train_step_against_torch_gru(kind):
    torch.manual_seed(11)
    if kind == 'uni':
        ref = nn.Sequential(_RefGRU(35, 64), _RefMLP(64, 32, 1))
        mine = nn.Sequential(*E.affect_uni_gru(0)[:2])
        adapt = lambda x: [x[0][0], x[1][0]]                                   # noqa: E731
    else:
        ref, mine = _RefLF(), E.affect_mm_gru(1)
        adapt = lambda x: x                                                    # noqa: E731
    mine.load_state_dict(ref.state_dict(), strict=True)
    ref = ref.double()
    mine = mine.cuda().eval()                                                  # dropout off
    lr, wd = 1e-3, 1e-2
    step = E.ExpertTrainStep(mine, 'l1', lr=lr, weight_decay=wd)
    opt = torch.optim.AdamW(ref.parameters(), lr=lr, weight_decay=wd)
    inputs, y = _batch(8, 6, 21)
    opt.zero_grad()
    loss_r = nn.functional.l1_loss(ref(adapt([[x.double() for x in inputs[0]], inputs[1]])), y.double())
    loss_r.backward()
    gn = torch.nn.utils.clip_grad_norm_(ref.parameters(), 8.0)
    opt.step()
    last = step(adapt([[x.cuda() for x in inputs[0]], inputs[1]]), y.cuda())
    torch.cuda.synchronize()
    print(f'FIG {kind} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} norm={last["grad_norm"].item():.6f} ref={gn.item():.6f}')
    assert abs(last['loss'].item() - loss_r.item()) < 1e-5
    assert abs(last['grad_norm'].item() - gn.item()) < 1e-4 * gn.item()
    step.opt.check_finite()
    check_adam_params(mine, ref, lr, kind)


@pytest.mark.gpu
def test_experts_train_writes_ef_gru(tmp_path):
    from dynmm_amd import affect, affect_mm
    torch.manual_seed(0)
    dev = torch.device('cuda')
    loaders = [affect.Loader(*affect.synthetic_split(n, s), 32, shuffle=(k == 0), device=dev) for k, (n, s) in
               enumerate([(64, 1), (32, 2)])]
    model = E.affect_mm_gru(0).to(dev)
    path = affect_mm.file_names(str(tmp_path), 0)[0]
    assert path.endswith('ef_gru.pt')
    history, stopper, best = E.train(model, loaders, lambda x: x, 'l1', 1e-3, 1e-2, 2, lambda: E.save_state(model, path),
                                     protocol='mm')
    assert len(history) == 2 and all(h == h and abs(h) < float('inf') for h in history)
    fresh = E.affect_mm_gru(0)
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    r = E.evaluate_posneg(fresh.to(dev), loaders[1], lambda x: x)
    assert all(r[k] == r[k] and abs(r[k]) < float('inf') for k in ('Accuracy', 'Loss', 'Corr')), r


@pytest.mark.gpu
def test_graph_replay_equals_eager_and_host_lengths_are_refused():
    torch.manual_seed(5)
    a = nn.Sequential(*E.affect_uni_gru(0)[:2]).cuda().eval()
    b = nn.Sequential(*E.affect_uni_gru(0)[:2]).cuda().eval()
    b.load_state_dict(a.state_dict())
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = _batch(8, 6, 30 + it)
        x = [inputs[0][0].cuda(), inputs[1][0].cuda()]                          # device lengths, different at every step
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k
    inputs, y = _batch(8, 6, 40)
    sc = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    with pytest.raises(ValueError, match='lengths'):
        sc([inputs[0][0].cuda(), inputs[1][0]], y.cuda())
    assert not torch.cuda.is_current_stream_capturing()

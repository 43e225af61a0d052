"""The MULT expert (dynmm_amd.nn.mult, experts.affect_mm_mult: affect_mm.py --fusion 4) against its plain-torch twin
tests/mult_oracle.py, with the whole-model bars of the other experts (tests/test_attn_wide._model_check: out 2e-4, worst
per-parameter gradient 2e-3, median 2e-4; a figure that depth pushes over its bar gets max(bar, 4 x the float32 twin's error
against the float64 twin) and is printed either way).
"""
import gc
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mult_oracle as MO
from tests.parity import Masks as _Masks, rel as _rel

N_PARAMS = 3080321            # 16 360 + 9 x 78 960 + 3 x 697 680 + 2 x 129 960 + 361
ACTIVE_SITES = 199            # 147 in the cross transformers, 51 in the memory transformers, 1 in the head


@pytest.fixture(autouse=True)
def _leave_no_garbage():
    """Steps, captured graphs and models die with the test that made them, not in a later test's collector run."""
    yield
    gc.collect()
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


def _pair(seed, dtype=torch.float32):
    from dynmm_amd import experts as E
    ref = MO.fill_(MO.mult_twin(), seed=seed)
    mine = E.affect_mm_mult()
    mine.load_state_dict(ref.state_dict(), strict=True)
    return mine, ref.to(dtype)


# ---------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------
def _expected_layout():
    E, shapes = 40, {}
    for i, f in enumerate((35, 74, 300)):
        shapes[f'fuse.proj.{i}.weight'] = (E, f, 1)

    def encoder(prefix, D, L):
        shapes[prefix + 'version'] = (1,)
        shapes[prefix + 'embed_positions._float_tensor'] = (1,)
        for l in range(L):
            p = f'{prefix}layers.{l}.'
            shapes[p + 'self_attn.in_proj_weight'] = (3 * D, D)
            shapes[p + 'self_attn.in_proj_bias'] = (3 * D,)
            shapes[p + 'self_attn.out_proj.weight'] = (D, D)
            shapes[p + 'self_attn.out_proj.bias'] = (D,)
            shapes[p + 'fc1.weight'], shapes[p + 'fc1.bias'] = (4 * D, D), (4 * D,)
            shapes[p + 'fc2.weight'], shapes[p + 'fc2.bias'] = (D, 4 * D), (D,)
            for n in (0, 1):
                shapes[p + f'layer_norms.{n}.weight'] = shapes[p + f'layer_norms.{n}.bias'] = (D,)
        shapes[prefix + 'layer_norm.weight'] = shapes[prefix + 'layer_norm.bias'] = (D,)
    for i in range(3):
        for j in range(3):
            encoder(f'fuse.trans.{i}.{j}.', E, 4)
    for i in range(3):
        encoder(f'fuse.trans_mems.{i}.', 3 * E, 4)
    for n, (o, c) in {'proj1': (360, 360), 'proj2': (360, 360), 'out_layer': (1, 360)}.items():
        shapes[f'fuse.{n}.weight'], shapes[f'fuse.{n}.bias'] = (o, c), (o,)
    return shapes


def test_mult_expert_layout_count_files_and_switch(tmp_path):
    from dynmm_amd import affect_mm
    from dynmm_amd import experts as E
    mine, ref = _pair(1)
    a, b = mine.state_dict(), ref.state_dict()
    want = _expected_layout()
    assert set(a) == set(want) == set(b)
    assert all(tuple(a[k].shape) == want[k] == tuple(b[k].shape) for k in want)
    assert sum(p.numel() for p in mine.parameters()) == N_PARAMS == sum(p.numel() for p in ref.parameters())
    assert N_PARAMS == 16360 + 9 * 78960 + 3 * 697680 + 2 * 129960 + 361
    MO.mult_twin().load_state_dict(a, strict=True)                   # and back
    E.affect_mm_mult().load_state_dict(b, strict=True)
    path, copy = affect_mm.file_names(str(tmp_path), 4)
    assert path.endswith('mult.pt') and not path.endswith('b2_mult.pt') and copy.endswith('b2_mult.pt')
    with pytest.raises(NotImplementedError, match='MULT'):
        affect_mm.main(['--fusion', '4', '--dataset', 'synthetic'])
    with pytest.raises(NotImplementedError, match='affect_mm_mult'):
        E.affect_mm(4)
    hp = mine.fuse
    assert (hp.num_heads, hp.layers, hp.embed_dim, hp.attn_mask) == (10, 4, 40, True)
    assert [[t.attn_dropout for t in row] for row in hp.trans] == [[0, 0, 0.1]] * 3
    assert [t.attn_dropout for t in hp.trans_mems] == [0.1] * 3 and hp.trans[0][0].dropout == 0.2


def test_oracle_positional_table_is_the_closed_form():
    for E, T in [(40, 50), (120, 17), (6, 3)]:
        tab = MO.position_table(E, T)
        for t in range(T):
            for c in range(E // 2):
                w = math.exp(-c * math.log(10000.0) / (E // 2 - 1))
                assert abs(tab[t, c].item() - math.sin((t + 1) * w)) < 1e-12
                assert abs(tab[t, c + E // 2].item() - math.cos((t + 1) * w)) < 1e-12
    x = torch.randn(2, 5, 40, dtype=torch.float64)
    x[0, :2, 0] = 0.0
    pos = MO.SinusoidalPositionalEmbedding(40)(x)
    assert bool((pos[0, :2] == 0).all()) and torch.equal(pos[1], MO.position_table(40, 5)) and not pos.requires_grad


def test_oracle_counts_the_issues_active_sites():
    """training mode on the CPU twin at a tiny batch: 199 hook calls — 147 + 51 + 1"""
    ref = MO.fill_(MO.mult_twin(), seed=3).train()
    inputs, _ = MO.padded_batch(2, seed=4, T=5)
    mk = _Masks(0.1, 7)
    MO.MULTModel.dropout_masks = mk
    try:
        with torch.no_grad():
            ref(inputs)
    finally:
        MO.MULTModel.dropout_masks = None
    assert mk.n == ACTIVE_SITES
    assert mk.names.count('attn') == 3 * 4 + 3 * 4 and mk.names.count('embed_k') == 9 and mk.names.count('embed_q') == 12
    assert mk.names[-1] == 'out' and mk.names[:3] == ['embed_q', 'embed_k', 'embed_v']
    per_target = (15 + 15 + 19) + 17
    assert mk.n == 3 * per_target + 1 and 3 * (15 + 15 + 19) == 147 and 3 * 17 == 51


# ---------------------------------------------------------------------------------------------------------------
# the expert on the GPU
# ---------------------------------------------------------------------------------------------------------------
def _grad_errors(got, ref):
    gr = dict(ref.named_parameters())
    errs = {}
    for n, g in got.items():
        r = gr[n].grad
        if r is None or r.abs().max() < 1e-9:
            continue
        errs[n] = ((g.cpu().double() - r.double()).norm() / r.double().norm()).item()
    return errs


def _model_check(tag, grads, ref64, out, out64, grads32, out32):
    """test_attn_wide._model_check with the raised-bar rule: each figure against max(bar, 4 x the float32 twin's figure)"""
    errs, yard = _grad_errors(grads, ref64), _grad_errors(grads32, ref64)
    worst, worst32 = max(errs, key=errs.get), max(yard, key=yard.get)
    eo, med = _rel(out, out64), float(np.median(list(errs.values())))
    yo, ymed = _rel(out32, out64), float(np.median(list(yard.values())))
    bars = max(2e-4, 4 * yo), max(2e-3, 4 * yard[worst32]), max(2e-4, 4 * ymed)
    print(f'FIG {tag} out={eo:.3e} (f32 twin {yo:.3e}, bar {bars[0]:.3e}) worst grad={errs[worst]:.3e} ({worst}; f32 twin '
          f'{yard[worst32]:.3e}, bar {bars[1]:.3e}) median grad={med:.3e} (f32 twin {ymed:.3e}, bar {bars[2]:.3e})')
    assert len(errs) > 590
    assert eo < bars[0]
    assert errs[worst] < bars[1], (worst, errs[worst])
    assert med < bars[2]


def _to(inputs, fn):
    return [[fn(x) for x in inputs[0]], inputs[1]]


def _twin_run(ref, inputs, y, dtype, masks=None):
    ref = ref.to(dtype)
    ref.zero_grad()
    MO.MULTModel.dropout_masks = masks
    try:
        out = ref(_to(inputs, lambda x: x.to(dtype)))
        (out - y.to(dtype)).abs().mean().backward()
    finally:
        MO.MULTModel.dropout_masks = None
    return out.detach(), {n: p.grad.detach().clone() for n, p in ref.named_parameters() if p.grad is not None}


def _hip_run(mine, inputs, y, masks=None):
    from dynmm_amd import ops_seq as S
    S.MASKS = masks
    try:
        out = mine(_to(inputs, lambda x: x.cuda()))
        (out - y.cuda()).abs().mean().backward()
        torch.cuda.synchronize()
    finally:
        S.MASKS = None
    return out.detach(), {n: p.grad.detach().clone() for n, p in mine.named_parameters() if p.grad is not None}


def _compare(tag, T, train, seed=3):
    mine, ref = _pair(1)
    inputs, y = MO.padded_batch(4, seed=seed, T=T)
    masks = (lambda dev: _Masks(0.1, 21, dev)) if train else (lambda dev: None)
    ref.train(train)
    mine = mine.cuda().train(train)
    m32, m64, mh = masks('cpu'), masks('cpu'), masks('cuda')
    out32, g32 = _twin_run(ref, inputs, y, torch.float32, m32)
    out64, _ = _twin_run(ref, inputs, y, torch.float64, m64)             # (ref now holds the float64 gradients)
    out, grads = _hip_run(mine, inputs, y, mh)
    if train:
        assert mh.n == m64.n == ACTIVE_SITES
        assert mh.names == m64.names
    _model_check(tag, grads, ref, out, out64, g32, out32)
    return mine, inputs, out64


@pytest.mark.gpu
def test_mult_expert_matches_the_float64_twin():
    _compare('mult eval T=50', 50, False)


@pytest.mark.gpu
def test_mult_expert_at_a_shorter_sequence():
    _compare('mult eval T=17', 17, False)


class _ShapeLog(_Masks):
    """Masks that also record the shape of every site served"""

    def __init__(self, *a):
        super().__init__(*a)
        self.shapes = []

    def __call__(self, name, shape):
        self.shapes.append(tuple(shape))
        return super().__call__(name, shape)


@pytest.mark.gpu
def test_mult_expert_training_mode_with_injected_dropout():
    mine, inputs, out_train = _compare('mult train T=50', 50, True)
    # the two call lists, names AND shapes
    from dynmm_amd import ops_seq as S
    ref = MO.fill_(MO.mult_twin(), seed=1).train()
    a, b = _ShapeLog(0.1, 5), _ShapeLog(0.1, 5, 'cuda')
    MO.MULTModel.dropout_masks, S.MASKS = a, b
    try:
        with torch.no_grad():
            ref(inputs)
            mine(_to(inputs, lambda x: x.cuda()))
    finally:
        MO.MULTModel.dropout_masks, S.MASKS = None, None
    assert a.n == b.n == ACTIVE_SITES and a.names == b.names and a.shapes == b.shapes
    mine.eval()
    with torch.no_grad():
        out_e = mine(_to(inputs, lambda x: x.cuda()))
    assert _rel(out_e, out_train) > 1e-3                            # dropout really acted


@pytest.mark.gpu
def test_mult_train_step_matches_torch_adamw():
    from dynmm_amd import experts as E
    lr, wd = 1e-3, 1e-2
    mine, ref = _pair(2)
    mine, ref = mine.cuda().eval(), ref.eval()      # the optimiser arithmetic is what is compared here: dropout off on both sides
    step = E.ExpertTrainStep(mine, 'l1', lr=lr, weight_decay=wd)
    opt = torch.optim.AdamW(ref.parameters(), lr=lr, weight_decay=wd)
    for it in range(2):
        inputs, y = MO.padded_batch(5, seed=10 + it)
        opt.zero_grad()
        loss_r = F.l1_loss(ref(inputs), y)
        loss_r.backward()
        gn = torch.nn.utils.clip_grad_norm_(ref.parameters(), 8.0)
        opt.step()
        last = step(_to(inputs, lambda x: x.cuda()), y.cuda())
        torch.cuda.synchronize()
        tol = 2e-5 if it == 0 else 2e-4 * max(1.0, abs(loss_r.item()))
        print(f'FIG mult step {it} loss={last["loss"].item():.7f} ref={loss_r.item():.7f} norm={last["grad_norm"].item():.6f} '
              f'ref={gn.item():.6f}')
        assert abs(last['loss'].item() - loss_r.item()) < tol
        assert abs(last['grad_norm'].item() - gn.item()) < 2e-3 * max(gn.item(), 1e-3)
    sd_r, sd = ref.state_dict(), mine.state_dict()
    for k in sd_r:
        d = (sd[k].cpu() - sd_r[k]).abs()
        if k.endswith('in_proj_bias'):
            third = d.numel() // 3           # the key bias of softmax attention has an analytically zero gradient
            d = torch.cat([d[:third], d[2 * third:]])
        n_far = int((d > 0.4 * lr).sum().item())
        assert n_far <= max(1, int(2e-3 * d.numel())) and d.max().item() < 4.4 * lr, (k, n_far, d.max().item())
    step.opt.check_finite()


@pytest.fixture
def philox_state():
    from dynmm_amd import ops
    from dynmm_amd import ops_seq as S
    seed = ops._PHILOX_SEED
    yield
    ops.manual_seed(seed)
    S.dropout_step(torch.device('cuda', torch.cuda.current_device())).zero_()


@pytest.mark.gpu
def test_mult_graph_replay(philox_state):
    from dynmm_amd import experts as E
    from dynmm_amd import ops
    from dynmm_amd import ops_seq as S
    a, _ = _pair(2)
    b, _ = _pair(2)
    a, b = a.cuda().eval(), b.cuda().eval()
    sa = E.ExpertTrainStep(a, 'l1', lr=1e-3, weight_decay=1e-2)
    sb = E.ExpertTrainStep(b, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=True)
    for it in range(3):
        inputs, y = MO.padded_batch(4, seed=60 + it)
        x = _to(inputs, lambda t: t.cuda())
        ra, rb = sa(x, y.cuda()), sb(x, y.cuda())
        assert abs(ra['loss'].item() - rb['loss'].item()) <= 1e-6 * abs(ra['loss'].item())
        assert abs(ra['grad_norm'].item() - rb['grad_norm'].item()) <= 1e-5 * ra['grad_norm'].item()
    assert len(sb._graphs) == 1
    for (k, va), vb in zip(a.state_dict().items(), b.state_dict().values()):
        assert (va - vb).abs().max().item() < 1e-5, k
    # dropout on, weights frozen: a replay must not reuse its decisions
    c, _ = _pair(2)
    c = c.cuda().train()
    sc = E.ExpertTrainStep(c, 'l1', lr=0.0, weight_decay=0.0, use_graph=True)
    inputs, y = MO.padded_batch(4, seed=70)
    x = _to(inputs, lambda t: t.cuda())
    ops.manual_seed(77)
    S.dropout_step(x[0][0].device).zero_()
    losses = [sc(x, y.cuda())['loss'].item() for _ in range(3)]
    assert len({round(v, 7) for v in losses}) == 3, losses
    sc.opt.check_finite()
    for st in (sb, sc):                                        # the captures are released here, with the device idle
        torch.cuda.synchronize()
        for entry in st._graphs.values():
            entry[0].reset()
        st._graphs.clear()


@pytest.mark.gpu
def test_experts_train_writes_mult(tmp_path):
    from dynmm_amd import affect, affect_mm
    from dynmm_amd import experts as E
    torch.manual_seed(0)
    dev = torch.device('cuda')
    loaders = [affect.Loader(*affect.synthetic_split(n, s), 32, shuffle=(k == 0), device=dev) for k, (n, s) in
               enumerate([(64, 1), (32, 2)])]
    model = E.affect_mm_mult().to(dev)
    path = affect_mm.file_names(str(tmp_path), 4)[0]
    history, stopper, best = E.train(model, loaders, lambda x: x, 'l1', 1e-4, 1e-4, 1, lambda: E.save_state(model, path),
                                     protocol='mm')
    assert path.endswith('mult.pt')
    assert len(history) == 1 and all(h == h and abs(h) < float('inf') for h in history)
    fresh = E.affect_mm_mult()
    fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    r = E.evaluate_posneg(fresh.to(dev), loaders[1], lambda x: x)
    assert all(r[k] == r[k] and abs(r[k]) < float('inf') for k in ('Accuracy', 'Loss', 'Corr')), r

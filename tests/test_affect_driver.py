"""The CMU-MOSEI DynMM driver (ModalityDynMM/affect/affect_dyn.py:177-250): `python -m dynmm_amd.affect`, the reference's
posneg evaluation protocol (Supervised_Learning.single_test, task "posneg-classification" — PINNED: the protocol is vendored in
the reference) on the device, and hard-gate compaction of DynMMNetV2 / DynMMNet (the model arithmetic stays PARITY UNPINNED,
see tests/test_affect.py).  CPU: the CLI's defaults, the host-side reduction against a numpy restatement of single_test, the
refusal of pickled experts, the kernel's static gates.  GPU: the counts kernel against numpy, compacted against dense
evaluation, the CLI end to end."""
import importlib.util
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def single_test_posneg(batches):
    """numpy restatement of Supervised_Learning.py:276-347 for criterion L1Loss(reduction='sum'): per batch
    totalloss += criterion(out, y) * len(batch); pred = out[:, 0] >= 0, truth = y >= 0; Accuracy, Loss = totalloss / N,
    Corr = pearsonr(truth, pred) (numpy's corrcoef: the same value, NaN for a constant vector)."""
    total, preds, truths = 0.0, [], []
    for out, y in batches:
        out, y = np.asarray(out, np.float64), np.asarray(y, np.float64)
        total += np.abs(out - y).sum() * len(y)
        preds.append((out[:, 0] >= 0).astype(np.int64))
        truths.append((y[:, 0] >= 0).astype(np.int64))
    pred, truth = np.concatenate(preds), np.concatenate(truths)
    with np.errstate(invalid='ignore', divide='ignore'):
        corr = np.corrcoef(truth, pred)[0, 1]
    return {'Accuracy': float((pred == truth).mean()), 'Loss': total / len(truth), 'Corr': float(corr)}, pred, truth


def table(pred, truth):
    return np.array([np.sum((pred == p) & (truth == t)) for p in (0, 1) for t in (0, 1)], np.int64)


def batches_with_zeros(sizes, seed):
    g = np.random.default_rng(seed)
    out = []
    for B in sizes:
        o = g.standard_normal((B, 1)).astype(np.float32)
        y = np.round(3 * g.uniform(-1, 1, (B, 1)), 1).astype(np.float32)
        o[::3] = 0.0
        y[::4] = 0.0
        if B > 2:
            o[1], y[2] = -0.0, -0.0
        out.append((o, y))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------------
def test_cli_parses_reference_defaults():
    from dynmm_amd import affect
    a = affect.parser().parse_args([])
    # affect_dyn.py:180-193
    assert (a.gpu, a.data, a.n_runs, a.enc, a.n_epochs, a.temp) == (0, 'mosei', 1, 'transformer', 50, 1)
    assert (a.hard_gate, a.reg, a.lr, a.wd, a.infer_mode, a.eval_only, a.freeze) == (False, 0.0, 1e-6, 1e-4, 0, False, False)
    assert (a.model, a.dataset, a.batch_size) == ('v2', 'npz', 128)
    a = affect.parser().parse_args(['--hard-gate', '--reg', '0.1', '--model', 'v1', '--dataset', 'synthetic', '--eval-only'])
    assert (a.hard_gate, a.reg, a.model, a.dataset, a.eval_only) == (True, 0.1, 'v1', 'synthetic', True)


def test_gru_encoder_is_refused():
    from dynmm_amd import affect
    with pytest.raises(NotImplementedError, match='gru'):
        affect.main(['--enc', 'gru'])


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_host_reduction_equals_single_test_restatement(seed):
    from dynmm_amd import ops_seq as S
    batches = batches_with_zeros([128, 7, 1, 300, 64], seed)
    want, pred, truth = single_test_posneg(batches)
    counts = table(pred, truth)
    acc_loss = sum(float(np.abs(o.astype(np.float64) - y).sum()) * len(y) for o, y in batches)
    got = S.posneg_metrics(counts, acc_loss, len(truth))
    assert got['Accuracy'] == want['Accuracy']
    assert got['Loss'] == pytest.approx(want['Loss'], rel=1e-12)
    assert got['Corr'] == pytest.approx(want['Corr'], rel=1e-12, abs=1e-15)


def test_host_reduction_constant_vector_gives_nan():
    from dynmm_amd import ops_seq as S
    o = np.abs(np.random.default_rng(0).standard_normal((50, 1))).astype(np.float32)      # every prediction positive
    y = np.random.default_rng(1).standard_normal((50, 1)).astype(np.float32)
    want, pred, truth = single_test_posneg([(o, y)])
    got = S.posneg_metrics(table(pred, truth), 0.0, 50)
    assert math.isnan(want['Corr']) and math.isnan(got['Corr'])
    assert got['Accuracy'] == want['Accuracy']
    # >= 0 on both sides: exact zeros count as positive
    got = S.posneg_metrics(table(np.array([1, 1, 0, 0]), np.array([1, 0, 1, 0])), 0.0, 4)
    assert got['Corr'] == 0.0 and got['Accuracy'] == 0.5
    with pytest.raises(ValueError):
        S.posneg_metrics([1, 2, 3, 4], 0.0, 11)


def test_pickled_expert_module_is_refused(tmp_path):
    from dynmm_amd import affect
    from dynmm_amd.nn import affect as A
    torch.save(A.Transformer(300, 120), tmp_path / 'b1_reg_transformer_encoder_text.pt')      # a module, not a state_dict
    model = A.DynMMNetV2()
    with pytest.raises(RuntimeError, match='state_dict'):
        affect.load_pretrained(model, str(tmp_path))


def test_expert_state_dicts_load_under_reference_names(tmp_path):
    from dynmm_amd import affect
    from dynmm_amd.nn import affect as A
    torch.manual_seed(0)
    src = A.DynMMNetV2()
    for attr, fname in affect.expert_files('v2').items():
        torch.save(src.get_submodule(attr).state_dict(), tmp_path / fname)
    assert sorted(os.listdir(tmp_path)) == ['b1_reg_transformer_encoder_text.pt', 'b1_reg_transformer_head_text.pt',
                                            'b2_lf_tran.pt']
    torch.manual_seed(1)
    dst = A.DynMMNetV2()
    affect.load_pretrained(dst, str(tmp_path))
    sd, sd_src = dst.state_dict(), src.state_dict()
    for k in sd:
        if not k.startswith('gate.'):
            assert torch.equal(sd[k], sd_src[k]), k                                 # the experts copied
    assert not torch.equal(sd['gate.1.weight'], sd_src['gate.1.weight'])             # the gate left alone


def test_v1_flop_and_weight_stat():
    from dynmm_amd.nn import affect as A
    m = A.DynMMNet()
    v2 = A.DynMMNetV2()
    assert m.flop[2].item() == v2.flop[0].item()
    assert m.flop[0].item() == pytest.approx(135.13226 - 265 * 6000 / 1e6)
    m.weight_list = torch.tensor([[1.0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0]])
    assert m.weight_stat() == 0.5
    assert m.cal_flop() == pytest.approx((m.flop * torch.tensor([0.25, 0.25, 0.5])).sum().item())


@pytest.mark.skipif(shutil.which('hipcc') is None, reason='needs hipcc (cross-compiles gfx950 without a GPU)')
def test_counts_kernel_has_no_serialised_loads():
    """The static gate of tests/test_isa_loads.py applied to csrc/affect_eval.hip."""
    spec = importlib.util.spec_from_file_location('serial_loads', os.path.join(REPO, 'scratch', 'r6', 'serial_loads.py'))
    sl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sl)
    rows = [r for r in sl.compile_and_scan(os.path.join(REPO, 'dynmm_amd', 'csrc', 'affect_eval.hip')) if 'posneg' in r[2]]
    assert rows
    for n, nl, k in rows:
        assert n == 0, f'{k}: {n} of {nl} loads wait alone'


# ------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('form', ['test', 'valid'])
def test_counts_kernel_against_numpy(form):
    from dynmm_amd import ops_seq as S
    sizes = (1, 7, 128, 300)
    batches = batches_with_zeros(sizes, seed=5)
    auxs = np.random.default_rng(6).uniform(0, 1, len(sizes)).astype(np.float32)
    lossw = 0.3
    c = S.PosnegCounts('cuda', form, lossw)
    want_loss = 0.0
    for (o, y), a in zip(batches, auxs):
        c.add(torch.from_numpy(o).cuda(), torch.from_numpy(y).cuda(), torch.tensor(a).cuda())
        d = np.abs(o.astype(np.float64) - y.astype(np.float64)).sum()
        B = len(y)
        want_loss += B * d if form == 'test' else (d / B + lossw * float(a)) * B
    r = c.read()
    want, pred, truth = single_test_posneg(batches)
    assert np.array_equal(r['counts'], table(pred, truth)), (r['counts'], table(pred, truth))
    assert r['n'] == sum(sizes)
    assert r['loss_acc'] == pytest.approx(want_loss, rel=1e-12)
    m = c.metrics()
    assert m['Accuracy'] == want['Accuracy']
    assert m['Corr'] == pytest.approx(want['Corr'], rel=1e-12)
    if form == 'test':
        assert m['Loss'] == pytest.approx(want['Loss'], rel=1e-12)
    # out[:, 0] of a wider output: the stride is honoured
    c2 = S.PosnegCounts('cuda')
    o, y = batches[2]
    wide = np.concatenate([o, -np.ones_like(o) * 7], axis=1)
    c2.add(torch.from_numpy(wide).cuda(), torch.from_numpy(y).cuda())
    assert np.array_equal(c2.read()['counts'], table((o[:, 0] >= 0).astype(np.int64), (y[:, 0] >= 0).astype(np.int64)))


def _batch(B, seed, T=50):
    from dynmm_amd.nn import affect as A
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, T, A.FEATURES[m], generator=g).cuda() for m in ('visual', 'audio', 'text')]
    return [xs, [torch.full((B,), T, dtype=torch.long)] * 3]


def _routings(m, x, K):
    """Gate biases that force (name, bias) routings: every sample to one expert, about half to two of them, and for K = 3
    the same with the middle expert empty."""
    lin = m.gate[1]
    base = lin.bias.detach().clone()
    with torch.no_grad():
        lg = m.gate_logits(x) - base
    out = []
    for k in range(K):
        b = torch.full((K,), -50.0, device='cuda')
        b[k] = 50.0
        out.append((f'all-{k}', b))
    hi = K - 1
    d = (lg[:, hi] - lg[:, 0]).median()
    b = torch.zeros(K, device='cuda')
    b[hi] = -(d + 1e-3)
    if K == 3:
        b[1] = -50.0
    out.append(('half', b))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['v2', 'v1'])
def test_compacted_hard_gate_eval_equals_dense(monkeypatch, kind):
    from dynmm_amd.nn import affect as A
    torch.manual_seed(3)
    m = (A.DynMMNetV2(1.0, True) if kind == 'v2' else A.DynMMNet(1.0, True)).cuda().eval()
    K = m.branch_num
    B = 96
    x = _batch(B, seed=4)
    calls = []
    real = A.Transformer.forward

    def spy(self, xx):
        calls.append((self.conv.weight.shape[0], self.conv.weight.shape[1], (xx[0] if isinstance(xx, list) else xx).shape[0]))
        return real(self, xx)

    monkeypatch.setattr(A.Transformer, 'forward', spy)
    with torch.no_grad():
        for name, bias in _routings(m, x, K):
            m.gate[1].bias.copy_(bias)
            m.compact = False
            m.reset_weight()
            dense, aux_d = m(x)
            w_dense = m.weight_list.clone()
            m.compact = True
            m.reset_weight()
            calls.clear()
            comp, aux_c = m(x)
            w_comp = m.weight_list.clone()
            n = m.last_counts
            assert torch.equal(w_dense, w_comp), name
            assert list(n) == [int(v) for v in w_dense.sum(0)] and sum(n) == B, (name, n)
            if name.startswith('all-'):
                assert n[int(name[-1])] == B
            else:
                assert 0 < n[0] < B and n[K - 1] == B - n[0] and (K == 2 or n[1] == 0), (name, n)
            # the gate on all samples, each expert's transformers on its own rows only, nothing for an empty expert
            want = [(10, 409, B)]
            if kind == 'v2':
                want += [(120, 300, n[0])] if n[0] else []
                want += [(60, 35, n[1]), (120, 74, n[1]), (120, 300, n[1])] if n[1] else []
            else:
                want += [(120, f, n[k]) for k, f in enumerate((35, 74, 300)) if n[k]]
            assert sorted(calls) == sorted(want), (name, calls)
            assert comp.shape == dense.shape == (B, 1)
            assert float(aux_c) == float(aux_d), name
            err = (comp - dense).abs().max().item()
            assert err <= 2e-6 * dense.abs().max().item(), (name, err)
            assert m.cal_flop() == pytest.approx((m.flop * w_dense.mean(0)).sum().item())


@pytest.mark.gpu
def test_compaction_stays_off_outside_hard_gate_eval():
    from dynmm_amd.nn import affect as A
    torch.manual_seed(0)
    m = A.DynMMNetV2(1.0, True).cuda().eval()
    x = _batch(4, seed=1)
    m.last_counts = None
    out, _ = m(x)                                        # autograd on: dense
    assert m.last_counts is None and out.requires_grad
    with torch.no_grad():
        m.hard_gate = False
        m(x)
        assert m.last_counts is None
        m.hard_gate, m.infer_mode = True, 1
        m(x)
        assert m.last_counts is None
        m.infer_mode = 0
        m(x)
        assert m.last_counts is not None and sum(m.last_counts) == 4


def _summary(stdout):
    pats = [r'Test Accuracy (\S+) ± (\S+)', r'\nLoss (\S+) ± (\S+)', r'Corr (\S+) ± (\S+)', r'FLOP (\S+) ± (\S+)',
            r'Ratio (\S+) ± (\S+)']
    vals = []
    for p in pats:
        mm = re.search(p, stdout)
        assert mm, (p, stdout[-3000:])
        vals.append(mm.group(0))
        assert all(math.isfinite(float(v)) for v in mm.groups()), (p, mm.group(0))
    return vals


@pytest.mark.gpu
def test_cli_synthetic_end_to_end(tmp_path):
    env = dict(os.environ, PYTHONPATH=REPO)
    cmd = [sys.executable, '-m', 'dynmm_amd.affect', '--dataset', 'synthetic', '--n-epochs', '2', '--hard-gate', '--reg', '0.1',
           '--synthetic-size', '256', '--lr', '1e-4']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert len(re.findall(r'Epoch \d+ \| train loss [0-9.]+ \| valid loss [0-9.]+', r.stdout)) == 2, r.stdout
    assert 'Saving Best' in r.stdout
    saved = tmp_path / 'log' / 'mosei' / 'dyn_enc_transformer_reg_0.1freezeFalse.pt'
    assert saved.exists()
    first = _summary(r.stdout)
    r2 = subprocess.run(cmd + ['--eval-only'], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert 'Epoch' not in r2.stdout
    assert _summary(r2.stdout) == first, (r.stdout[-2000:], r2.stdout[-2000:])

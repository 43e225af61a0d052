"""Timings and memory figures behind profiles/mim.md: ops_mlp.mim against the unfused composition a MultiBench user runs (the three
lines of MultiplicativeInteractions2Modal.forward with output='matrix', in float32 through torch on the same device), and
ExpertTrainStep on the multiplicative-interactions MM-IMDB expert.  Needs a HIP device; prints one JSON line per measurement.

    python profiles/mim_bench.py op         # the operator at (128, 512, 512, 1024): forward, forward + backward, each pass alone
    python profiles/mim_bench.py mem        # peak device memory above the operands, forward and forward + backward
    python profiles/mim_bench.py step       # ms and samples/s of a training step of imdb_mm_mim() at batch 128

Method (profiles/lrtf.md): every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device events, the
variants alternating window by window; the figure is the median window, min and max are reported beside it.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynmm_amd import experts as E           # noqa: E402
from dynmm_amd import ops_mlp as M           # noqa: E402

ROUNDS = 9
PEAK_TF, PEAK_TB = 157.3, 6.29               # profiles/lrtf.md: fp32 matrix peak, measured HBM copy rate
GEOMETRY = (128, 512, 512, 1024)             # B, n, m, D


def composition(m1, m2, W, U, V, b):
    """fusions.common_fusions.MultiplicativeInteractions2Modal.forward, output='matrix'"""
    Wprime = torch.einsum('bn,nmd->bmd', m1, W) + V
    bprime = torch.matmul(m1, U) + b
    return torch.einsum('bm,bmd->bd', m2, Wprime) + bprime


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def alternate(fns, iters):
    """{name: [ms per call of each window]} with the variants alternating"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def summary(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def operands(need=(True,) * 6):
    B, n, m, D = GEOMETRY
    g = torch.Generator(device='cuda').manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=g, device='cuda')                 # noqa: E731
    ops = [rn(B, n), rn(B, m), rn(n, m, D) / (n * m) ** 0.5, rn(n, D) / n ** 0.5, rn(m, D) / m ** 0.5, 0.1 * rn(D)]
    return [t.requires_grad_(r) for t, r in zip(ops, need)], rn(B, D)


def bench_op():
    B, n, m, D = GEOMETRY
    ops, gy = operands()
    ops_in = [t.detach().requires_grad_(k < 2) for k, t in enumerate(ops)]      # inputs alone need a gradient
    ops_p = [t.detach().requires_grad_(k >= 2) for k, t in enumerate(ops)]      # parameters alone

    def fwd(f):
        with torch.no_grad():
            return f(*ops)

    def fwd_bwd(f, leaves):
        for t in leaves:
            t.grad = None
        f(*leaves).backward(gy)

    t = alternate({'fused_fwd': lambda: fwd(M.mim), 'torch_fwd': lambda: fwd(composition),
                   'fused_fwd_bwd': lambda: fwd_bwd(M.mim, ops), 'torch_fwd_bwd': lambda: fwd_bwd(composition, ops),
                   'fused_fwd_bwd_inputs_only': lambda: fwd_bwd(M.mim, ops_in),
                   'fused_fwd_bwd_params_only': lambda: fwd_bwd(M.mim, ops_p)}, 10)
    gf = 2.0 * B * n * m * D / 1e9                                               # one pass over W
    w_gb = n * m * D * 4 / 1e9
    row = {'what': 'op', 'B': B, 'n': n, 'm': m, 'D': D, 'pass_gflop': gf, 'W_gb': w_gb}
    for k, ts in t.items():
        row[k] = summary(ts)
    f = row['fused_fwd']['median_ms']
    wp = row['fused_fwd_bwd_params_only']['median_ms'] - f
    ip = row['fused_fwd_bwd_inputs_only']['median_ms'] - f
    for name, ms in (('fwd', f), ('weight_pass', wp), ('input_pass', ip)):
        row[f'fused_{name}_ms'] = ms
        row[f'fused_{name}_tflops'] = gf / ms
        row[f'fused_{name}_share_of_fp32_matrix_peak'] = gf / ms / PEAK_TF
        row[f'fused_{name}_W_tb_per_s'] = w_gb / ms
    row['fwd_ratio_torch_over_fused'] = row['torch_fwd']['median_ms'] / f
    row['fwd_bwd_ratio_torch_over_fused'] = row['torch_fwd_bwd']['median_ms'] / row['fused_fwd_bwd']['median_ms']
    print(json.dumps(row), flush=True)


def bench_mem():
    """peak torch.cuda.max_memory_allocated above what is allocated before the call (operands, gradient of out)"""
    ops, gy = operands()
    for name, f in (('fused', M.mim), ('torch', composition)):
        row = {'what': 'mem', 'variant': name}
        for mode in ('fwd', 'fwd_bwd'):
            for t in ops:
                t.grad = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            if mode == 'fwd':
                with torch.no_grad():
                    out = f(*ops)
            else:
                out = f(*ops)
                out.backward(gy)
            torch.cuda.synchronize()
            row[f'{mode}_peak_above_operands_mb'] = (torch.cuda.max_memory_allocated() - base) / 1e6
            del out
        print(json.dumps(row), flush=True)
    sizes = {'W_mb': ops[2].numel() * 4 / 1e6, 'one_BmD_tensor_mb': GEOMETRY[0] * GEOMETRY[2] * GEOMETRY[3] * 4 / 1e6}
    print(json.dumps({'what': 'mem', 'variant': 'sizes', **sizes}), flush=True)


def bench_step():
    B = 128
    torch.manual_seed(0)
    with torch.device('cuda'):
        model, lr = E.imdb_mm_mim()
    model.train()
    st = E.ExpertTrainStep(model, 'bce', lr=lr, weight_decay=1e-2)
    g = torch.Generator().manual_seed(3)
    x = [torch.randn(B, 300, generator=g).cuda(), torch.rand(B, 4096, generator=g).cuda()]
    y = (torch.rand(B, 23, generator=g) < 0.3).float().cuda()
    t = alternate({'imdb_mm_mim_eager': lambda: st(x, y)}, 10)
    for k, ts in t.items():
        row = {'what': 'step', 'model': k, 'batch': B, 'parameters': sum(p.numel() for p in model.parameters()), **summary(ts)}
        row['samples_per_s'] = B / row['median_ms'] * 1e3
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/mim_bench.py measures on a HIP device; none is available')
    {'op': bench_op, 'mem': bench_mem, 'step': bench_step}[sys.argv[1]]()

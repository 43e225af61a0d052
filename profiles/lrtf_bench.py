"""Timings behind profiles/lrtf.md: ops_seq.lrtf against the unfused composition a MultiBench user runs (LowRankTensorFusion's
forward in float32 through torch on the same device), and ExpertTrainStep on the low-rank-fusion MOSEI model against the
late-fusion GRU model.  Needs a HIP device; prints one JSON line per measurement.

    python profiles/lrtf_bench.py op        # the operator at the MM-IMDB and MOSEI geometries, forward and forward+backward
    python profiles/lrtf_bench.py step      # samples/s of a training step at batch 128, eager and replayed

Method: every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device events, the variants
alternating window by window; the figure is the median window, min and max are reported beside it.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynmm_amd import experts as E           # noqa: E402
from dynmm_amd import ops_seq as S           # noqa: E402

ROUNDS = 9
PEAK_TF = 157.3                              # fp32 matrix peak of the MI355X
GEOMETRIES = {'mm-imdb': (128, (512, 512), 512, 128), 'mosei': (128, (32, 32, 128), 128, 32)}


def composition(zs, factors, fusion_weights, fusion_bias):
    """fusions.common_fusions.LowRankTensorFusion.forward (flatten=True)"""
    B, O = zs[0].shape[0], fusion_bias.shape[1]
    fused = 1
    for z, factor in zip(zs, factors):
        ones = torch.ones(B, 1, dtype=z.dtype, device=z.device)
        fused = fused * torch.matmul(torch.cat((ones, z), dim=1), factor)
    out = torch.matmul(fusion_weights, fused.permute(1, 0, 2)).squeeze() + fusion_bias
    return out.view(-1, O)


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


def flops_fwd(B, dims, O, R):
    return 2.0 * R * B * O * sum(d + 1 for d in dims) + (len(dims) + 1.0) * R * B * O


def bench_op():
    for name, (B, dims, O, R) in GEOMETRIES.items():
        g = torch.Generator().manual_seed(1)
        zs = [torch.randn(B, d, generator=g).cuda().requires_grad_(True) for d in dims]
        fs = [(torch.randn(R, d + 1, O, generator=g) / (d + 1) ** 0.5).cuda().requires_grad_(True) for d in dims]
        w = (torch.randn(1, R, generator=g) / R ** 0.5).cuda().requires_grad_(True)
        b = (0.1 * torch.randn(1, O, generator=g)).cuda().requires_grad_(True)
        gy = torch.randn(B, O, generator=g).cuda()
        leaves = zs + fs + [w, b]

        def fwd(f):
            with torch.no_grad():
                return f(zs, fs, w, b)

        def fwd_bwd(f):
            for t in leaves:
                t.grad = None
            f(zs, fs, w, b).backward(gy)

        iters = 20 if name == 'mm-imdb' else 200
        t = alternate({'fused_fwd': lambda: fwd(S.lrtf), 'torch_fwd': lambda: fwd(composition),
                       'fused_fwd_bwd': lambda: fwd_bwd(S.lrtf), 'torch_fwd_bwd': lambda: fwd_bwd(composition)}, iters)
        gf = flops_fwd(B, dims, O, R) / 1e9
        factor_mb = sum(R * (d + 1) * O * 4 for d in dims) / 1e6
        row = {'what': 'op', 'geometry': name, 'B': B, 'dims': dims, 'O': O, 'R': R, 'fwd_gflop': gf, 'factor_mb': factor_mb}
        for k, ts in t.items():
            row[k] = summary(ts)
        ms = row['fused_fwd']['median_ms']
        row['fused_fwd_tflops'] = gf / ms
        row['fused_fwd_share_of_fp32_matrix_peak'] = gf / ms / PEAK_TF
        row['fused_fwd_factor_gb_per_s'] = factor_mb / ms
        row['fwd_ratio_torch_over_fused'] = row['torch_fwd']['median_ms'] / ms
        row['fwd_bwd_ratio_torch_over_fused'] = row['torch_fwd_bwd']['median_ms'] / row['fused_fwd_bwd']['median_ms']
        print(json.dumps(row), flush=True)


def bench_step():
    B, T = 128, 50
    g = torch.Generator().manual_seed(3)
    x = [[torch.randn(B, T, f, generator=g).cuda() for f in (35, 74, 300)],
         [torch.full((B,), T, dtype=torch.int32, device='cuda')] * 3]
    y = torch.randn(B, 1, generator=g).cuda()
    steps = {}
    for name, build in (('lrtf', E.affect_mm_lrtf), ('lf_gru', lambda: E.affect_mm_gru(1))):
        for graph in (False, True):
            torch.manual_seed(0)
            model = build().cuda().train()
            st = E.ExpertTrainStep(model, 'l1', lr=1e-3, weight_decay=1e-2, use_graph=graph)
            steps[f'{name}_{"replayed" if graph else "eager"}'] = lambda st=st: st(x, y)
    t = alternate(steps, 20)
    for k, ts in t.items():
        row = {'what': 'step', 'model': k, 'batch': B, **summary(ts)}
        row['samples_per_s'] = B / row['median_ms'] * 1e3
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/lrtf_bench.py measures on a HIP device; none is available')
    {'op': bench_op, 'step': bench_step}[sys.argv[1]]()

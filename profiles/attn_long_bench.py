"""Timings behind profiles/attn_long.md: ops_seq.attention_long (csrc/attn_long.hip) against torch's attention in float32 on the
same device (F.scaled_dot_product_attention with the boolean mask where causal, and the composition that stores the
probabilities), and ExpertTrainStep on affect_mm_mult() with (50, 500, 500)-step inputs.  Needs a HIP device; prints one JSON
line per measurement.

    python profiles/attn_long_bench.py op        # the five shapes: forward, forward + backward, peak memory above the operands
    python profiles/attn_long_bench.py step      # ms per MULT training step on unaligned inputs, eager and replayed

Method (profiles/attn_wide_bench.py's): every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device
events, the variants alternating window by window; the figure is the median window, min and max are reported beside it.
"""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynmm_amd import experts as E           # noqa: E402
from dynmm_amd import ops_seq as S           # noqa: E402

ROUNDS = 7
FP32_MATRIX_PEAK_TFLOPS = 157.3              # MI355X, v_mfma_f32_* (spec): exact fp32 in, fp32 accumulate
# (B, H, dh, Tq, Tk, causal)
SHAPES = [(32, 10, 4, 50, 500, 0), (32, 10, 4, 500, 50, 0), (32, 10, 12, 500, 500, 1), (128, 5, 24, 200, 200, 0),
          (128, 5, 60, 200, 200, 0)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def alternate(fns, iters):
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


def visible_fraction(Tq, Tk, causal):
    if not causal:
        return 1.0
    off = abs(Tk - Tq)
    return sum(min(Tk, i + off + 1) for i in range(Tq)) / (Tq * Tk)


def unfused(q, k, v, mask):
    """the composition that stores the probabilities: q, k, v [B, H, T, dh]"""
    s = (q * q.shape[-1] ** -0.5) @ k.transpose(-1, -2)
    if mask is not None:
        s = s.masked_fill(~mask, float('-inf'))
    return torch.softmax(s, dim=-1) @ v


def peak_above(fn):
    """peak device memory of one call above what is allocated before it, MB"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def bench_op():
    for B, H, dh, Tq, Tk, causal in SHAPES:
        g = torch.Generator().manual_seed(1)
        D = H * dh
        q, k, v = (torch.randn(B, D, T, generator=g).cuda().requires_grad_(True) for T in (Tq, Tk, Tk))
        gy = torch.randn(B, D, Tq, generator=g).cuda()
        q4, k4, v4 = (t.detach().reshape(B, H, dh, t.shape[2]).transpose(2, 3).contiguous().requires_grad_(True) for t in (q, k, v))
        gy4 = gy.reshape(B, H, dh, Tq).transpose(2, 3).contiguous()
        mask = (torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + abs(Tk - Tq)).cuda() if causal else None

        def ours(bw):
            def run():
                if not bw:
                    with torch.no_grad():
                        S.attention_long(q, k, v, H, causal)
                else:
                    q.grad = k.grad = v.grad = None
                    S.attention_long(q, k, v, H, causal).backward(gy)
            return run

        def torchs(fn, bw):
            def run():
                if not bw:
                    with torch.no_grad():
                        fn(q4, k4, v4)
                else:
                    q4.grad = k4.grad = v4.grad = None
                    fn(q4, k4, v4).backward(gy4)
            return run
        sdpa = lambda a, b, c: F.scaled_dot_product_attention(a, b, c, attn_mask=mask)      # noqa: E731
        comp = lambda a, b, c: unfused(a, b, c, mask)                                       # noqa: E731
        fns = {}
        for bw in (False, True):
            tag = 'fwd_bwd' if bw else 'fwd'
            fns[f'long_{tag}'] = ours(bw)
            fns[f'sdpa_{tag}'] = torchs(sdpa, bw)
            fns[f'unfused_{tag}'] = torchs(comp, bw)
        mem = {k: peak_above(fn) for k, fn in fns.items() if k.endswith('fwd_bwd')}
        t = alternate(fns, 20)
        gflop = 4.0 * B * H * Tq * Tk * dh * visible_fraction(Tq, Tk, causal) / 1e9           # q k^T and P v, visible part
        row = {'what': 'op', 'B': B, 'H': H, 'dh': dh, 'Tq': Tq, 'Tk': Tk, 'causal': causal, 'fwd_gflop': gflop,
               'probs_MB': 4.0 * B * H * Tq * Tk / 1e6}
        for kk, ts in t.items():
            row[kk] = summary(ts)
        row['long_fwd_tflops'] = gflop / row['long_fwd']['median_ms']
        row['long_fwd_bwd_tflops'] = 3.5 * gflop / row['long_fwd_bwd']['median_ms']            # + 5 products of the backward
        row['fwd_share_of_fp32_matrix_peak'] = row['long_fwd_tflops'] / FP32_MATRIX_PEAK_TFLOPS
        for tag in ('fwd', 'fwd_bwd'):
            row[f'{tag}_ratio_sdpa_over_long'] = row[f'sdpa_{tag}']['median_ms'] / row[f'long_{tag}']['median_ms']
            row[f'{tag}_ratio_unfused_over_long'] = row[f'unfused_{tag}']['median_ms'] / row[f'long_{tag}']['median_ms']
        row['peak_MB_above_operands'] = mem
        print(json.dumps(row), flush=True)


def bench_step():
    g = torch.Generator().manual_seed(3)
    for batch in (32, 128):
        x = [[torch.randn(batch, T, f, generator=g).cuda() for T, f in zip((50, 500, 500), (35, 74, 300))],
             [torch.full((batch,), T, dtype=torch.int32, device='cuda') for T in (50, 500, 500)]]
        y = torch.randn(batch, 1, generator=g).cuda()
        for graph in (False, True):
            torch.manual_seed(0)
            st = E.ExpertTrainStep(E.affect_mm_mult().cuda().train(), 'l1', lr=1e-4, weight_decay=1e-4, use_graph=graph)
            torch.cuda.reset_peak_memory_stats()
            ts = alternate({'step': lambda: st(x, y)}, 3)['step']
            row = {'what': 'step', 'model': 'mult', 'lengths': [50, 500, 500], 'batch': batch,
                   'variant': 'hip_replayed' if graph else 'hip_eager', **summary(ts)}
            row['samples_per_s'] = batch / row['median_ms'] * 1e3
            row['peak_GB'] = torch.cuda.max_memory_allocated() / 1e9
            print(json.dumps(row), flush=True)
            del st
            torch.cuda.synchronize()


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/attn_long_bench.py measures on a HIP device; none is available')
    {'op': bench_op, 'step': bench_step}[sys.argv[1]]()

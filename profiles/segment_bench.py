"""Timings behind profiles/segment.md: the fused inference tail (ops.tail_argmax, csrc/segment.hip) against what it replaces
— the two upsample2x_dw3x3 launches plus torch.argmax on the same input — and InferStep.segment against InferStep.__call__ +
argmax(1).to(uint8) on the benchmark's inference model.  Needs a HIP device; prints one JSON line per measurement.

    python profiles/segment_bench.py trace   # a few calls of each tail variant: run under `rocprofv3 --kernel-trace --stats`
    python profiles/segment_bench.py op      # the two tails between device events (launch overhead included), alternating
    python profiles/segment_bench.py step    # the whole inference step at batch 16, 480x640, alternating pairs
    python profiles/segment_bench.py step_trace   # a few replays of each kind, for `rocprofv3 --kernel-trace`

Method: every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device events, the variants
alternating window by window; the figure is the median window, min and max are reported beside it.  Bytes are counted from
shapes: the fused tail reads x once and writes one byte per output pixel.
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynmm_amd import engine, ops, synth                # noqa: E402
from dynmm_amd.nn.decoder import Upsample               # noqa: E402
from dynmm_amd.nn.net import SkipGateESANet             # noqa: E402

ROUNDS = 7
HBM_PEAK = 8.0e12                                       # bytes/s, MI355X HBM3E
N, C, H, W = 16, 40, 120, 160


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters          # ms per call


def alternate(fns, iters, rounds=ROUNDS):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return times


def summary(ts):
    return {'median_ms': statistics.median(ts), 'min_ms': min(ts), 'max_ms': max(ts)}


def tail_bytes():
    """(fused, unfused) bytes from shapes"""
    x = 4 * N * C * H * W
    fused = x + N * 16 * H * W
    unfused = x + 2 * 4 * x + 16 * x + 16 * x + 8 * N * 16 * H * W      # up1 w, up2 r + w, argmax r + int64 w
    return fused, unfused


def tails():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    up1, up2 = Upsample('learned-3x3-zeropad', C).cuda(), Upsample('learned-3x3-zeropad', C).cuda()
    with torch.no_grad():
        for u in (up1, up2):
            u.conv.weight.add_(0.05 * torch.randn(C, 1, 3, 3, generator=g).cuda())
            u.conv.bias.add_(0.1 * torch.randn(C, generator=g).cuda())

    def fused():
        with torch.no_grad():
            return ops.tail_argmax(x, up1.conv, up2.conv, 'zero')

    def unfused():
        with torch.no_grad():
            return up2(up1(x)).argmax(1)
    return fused, unfused


def bench_trace():
    fused, unfused = tails()
    for _ in range(10):
        fused()
        unfused()
    torch.cuda.synchronize()
    a, b = fused().long(), unfused()
    print(json.dumps({'what': 'trace', 'labels_differ': int((a != b).sum()), 'pixels': a.numel()}), flush=True)


def bench_op():
    fused, unfused = tails()
    t = alternate({'fused': fused, 'unfused': unfused}, 50)
    fb, ub = tail_bytes()
    row = {'what': 'op', 'shape': [N, C, H, W], 'fused_bytes': fb, 'unfused_bytes': ub}
    for k, ts in t.items():
        row[k] = summary(ts)
    row['ratio_unfused_over_fused'] = row['unfused']['median_ms'] / row['fused']['median_ms']
    row['fused_bytes_per_s_events'] = fb / (row['fused']['median_ms'] * 1e-3)
    row['fused_share_of_hbm_peak_events'] = row['fused_bytes_per_s_events'] / HBM_PEAK
    print(json.dumps(row), flush=True)


def step_workload(h=480, w=640, n=16):
    m = SkipGateESANet(height=h, width=w, encoder_block='NonBottleneck1D', fuse_depth_in_rgb_encoder='SE-add')
    synth.fill_state_dict(m.state_dict(), seed=0)
    m = m.cuda().eval()
    m.baseline, m.compact, m.dual_stream = True, True, True       # bench.py's inference workload (configs[1])
    g = torch.Generator().manual_seed(1234)
    rgb, depth = torch.randn(n, 3, h, w, generator=g).cuda(), torch.randn(n, 1, h, w, generator=g).cuda()
    logits_step, labels_step = engine.InferStep(m), engine.InferStep(m)
    fns = {'logits_argmax': lambda: logits_step(rgb, depth).argmax(1).to(torch.uint8),
           'segment': lambda: labels_step.segment(rgb, depth)}
    return m, rgb, depth, fns


def bench_step_trace():
    """for `rocprofv3 --kernel-trace`: both replays captured, then 4 calls of each kind, each group between synchronisations"""
    _, _, _, fns = step_workload()
    for fn in fns.values():
        for _ in range(3):
            fn()
    for fn in fns.values():
        torch.cuda.synchronize()
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    print(json.dumps({'what': 'step_trace', 'order': list(fns)}), flush=True)


def bench_step():
    h, w, n = 480, 640, 16
    m, rgb, depth, fns = step_workload(h, w, n)
    if len(sys.argv) > 2 and sys.argv[2] == 'labels_first':       # the order of the captures and of each pair, reversed
        fns = dict(reversed(list(fns.items())))
    t = alternate(fns, 10)
    row = {'what': 'step', 'launch': 'replay', 'order': list(fns), 'batch': n, 'hw': [h, w]}
    for k, ts in t.items():
        row[k] = summary(ts)
        row[k]['img_per_s'] = n / row[k]['median_ms'] * 1e3
    row['pairs'] = [[a, b] for a, b in zip(t['logits_argmax'], t['segment'])]
    row['ratio_logits_over_segment'] = row['logits_argmax']['median_ms'] / row['segment']['median_ms']
    a, b = fns['logits_argmax'](), fns['segment']()
    row['labels_differ'] = int((a != b).sum())
    row['pixels'] = a.numel()
    print(json.dumps(row), flush=True)

    def eager_logits():
        with torch.no_grad():
            return m(rgb, depth, True).argmax(1).to(torch.uint8)
    t = alternate({'logits_argmax': eager_logits, 'segment': lambda: m.segment(rgb, depth)}, 5, rounds=5)
    row = {'what': 'step', 'launch': 'eager', 'batch': n, 'hw': [h, w]}
    for k, ts in t.items():
        row[k] = summary(ts)
    row['ratio_logits_over_segment'] = row['logits_argmax']['median_ms'] / row['segment']['median_ms']
    print(json.dumps(row), flush=True)


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/segment_bench.py measures on a HIP device; none is available')
    {'trace': bench_trace, 'op': bench_op, 'step': bench_step, 'step_trace': bench_step_trace}[sys.argv[1]]()

"""Timings behind profiles/attn_wide.md: ops_seq.mha_wide (csrc/attn.hip) against torch's attention in float32 on the same
device, against ops_seq.mha_core at a head dimension both serve, and ExpertTrainStep on the early-fusion transformer expert
against a plain-torch twin.  Needs a HIP device; prints one JSON line per measurement.

    python profiles/attn_wide_bench.py op        # (B, H, dh, T) = (128, 5, 60, 50): forward and forward+backward, p = 0 and 0.1
    python profiles/attn_wide_bench.py core      # mha_wide against mha_core at (128, 5, 24, 50)
    python profiles/attn_wide_bench.py step      # ms per training step and samples/s at batch 128: eager, replayed, torch
    python profiles/attn_wide_bench.py trace     # six eager training steps and nothing else (the program of a
                                                 #   `rocprofv3 --kernel-trace --stats -- python ... trace` run)

Method: every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device events, the variants
alternating window by window; the figure is the median window, min and max are reported beside it.
"""
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dynmm_amd import experts as E           # noqa: E402
from dynmm_amd import ops_seq as S           # noqa: E402

ROUNDS = 9


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


def attn_gflop_fwd(B, H, dh, T):
    return 2.0 * 2.0 * B * H * T * T * dh / 1e9          # q k^T and P v


def unfused(q, k, v, p):
    """the composition nn.MultiheadAttention runs without a fused kernel: q, k, v [B, H, T, dh]"""
    a = torch.softmax((q * q.shape[-1] ** -0.5) @ k.transpose(-1, -2), dim=-1)
    return F.dropout(a, p) @ v if p > 0 else a @ v


def _attention_inputs(B, H, dh, T):
    g = torch.Generator().manual_seed(1)
    D = H * dh
    qkv = torch.randn(B, 3 * D, T, generator=g).cuda().requires_grad_(True)
    gy = torch.randn(B, D, T, generator=g).cuda()
    q, k, v = (t.reshape(B, H, dh, T).transpose(2, 3).contiguous().requires_grad_(True) for t in qkv.detach().split(D, dim=1))
    return qkv, gy, (q, k, v), gy.reshape(B, H, dh, T).transpose(2, 3).contiguous()


def _ours(fn, qkv, gy, H, p, backward):
    drop = (p, 9, 'attn') if p > 0 else None
    if not backward:
        def run():
            with torch.no_grad():
                fn(qkv, H, drop=drop)
    else:
        def run():
            qkv.grad = None
            fn(qkv, H, drop=drop).backward(gy)
    return run


def _torchs(fn, qkv3, gy4, backward):
    if not backward:
        def run():
            with torch.no_grad():
                fn(*qkv3)
    else:
        def run():
            for t in qkv3:
                t.grad = None
            fn(*qkv3).backward(gy4)
    return run


def bench_op():
    B, H, dh, T = 128, 5, 60, 50
    qkv, gy, qkv3, gy4 = _attention_inputs(B, H, dh, T)
    for p in (0.0, 0.1):
        fns = {}
        for bw in (False, True):
            tag = 'fwd_bwd' if bw else 'fwd'
            fns[f'wide_{tag}'] = _ours(S.mha_wide, qkv, gy, H, p, bw)
            fns[f'sdpa_{tag}'] = _torchs(lambda q, k, v: F.scaled_dot_product_attention(q, k, v, dropout_p=p), qkv3, gy4, bw)
            fns[f'unfused_{tag}'] = _torchs(lambda q, k, v: unfused(q, k, v, p), qkv3, gy4, bw)
        t = alternate(fns, 200)
        row = {'what': 'op', 'B': B, 'H': H, 'dh': dh, 'T': T, 'p': p, 'fwd_gflop': attn_gflop_fwd(B, H, dh, T)}
        for k, ts in t.items():
            row[k] = summary(ts)
        row['wide_fwd_tflops'] = row['fwd_gflop'] / row['wide_fwd']['median_ms']
        for tag in ('fwd', 'fwd_bwd'):
            row[f'{tag}_ratio_sdpa_over_wide'] = row[f'sdpa_{tag}']['median_ms'] / row[f'wide_{tag}']['median_ms']
            row[f'{tag}_ratio_unfused_over_wide'] = row[f'unfused_{tag}']['median_ms'] / row[f'wide_{tag}']['median_ms']
        print(json.dumps(row), flush=True)


def bench_core():
    B, H, dh, T = 128, 5, 24, 50
    qkv, gy, _, _ = _attention_inputs(B, H, dh, T)
    for p in (0.0, 0.1):
        fns = {}
        for bw in (False, True):
            tag = 'fwd_bwd' if bw else 'fwd'
            fns[f'wide_{tag}'] = _ours(S.mha_wide, qkv, gy, H, p, bw)
            fns[f'core_{tag}'] = _ours(S.mha_core, qkv, gy, H, p, bw)
        t = alternate(fns, 200)
        row = {'what': 'core', 'B': B, 'H': H, 'dh': dh, 'T': T, 'p': p}
        for k, ts in t.items():
            row[k] = summary(ts)
        for tag in ('fwd', 'fwd_bwd'):
            row[f'{tag}_ratio_core_over_wide'] = row[f'core_{tag}']['median_ms'] / row[f'wide_{tag}']['median_ms']
        print(json.dumps(row), flush=True)


class TorchTwin(nn.Module):
    """Sequential(Transformer(409, 300), MLP(300, 128, 1)) behind ConcatEarly, from the torch.nn layers MultiBench wraps"""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv1d(409, 300, kernel_size=1, bias=False)
        self.transformer = nn.TransformerEncoder(nn.TransformerEncoderLayer(d_model=300, nhead=5), num_layers=5,
                                                 enable_nested_tensor=False)
        self.fc, self.fc2 = nn.Linear(300, 128), nn.Linear(128, 1)

    def forward(self, inputs):
        x = self.conv(torch.cat(inputs[0], dim=2).permute(0, 2, 1)).permute(2, 0, 1)
        return self.fc2(F.relu(self.fc(self.transformer(x)[-1])))


def _batch(B=128, T=50):
    g = torch.Generator().manual_seed(3)
    x = [[torch.randn(B, T, f, generator=g).cuda() for f in (35, 74, 300)],
         [torch.full((B,), T, dtype=torch.int32, device='cuda')] * 3]
    return x, torch.randn(B, 1, generator=g).cuda()


def _hip_step(graph):
    torch.manual_seed(0)
    model = E.affect_mm_ef_tran().cuda().train()
    return E.ExpertTrainStep(model, 'l1', lr=1e-4, weight_decay=1e-4, use_graph=graph)


def bench_step():
    x, y = _batch()
    steps = {}
    for graph in (False, True):
        st = _hip_step(graph)
        steps['hip_replayed' if graph else 'hip_eager'] = lambda st=st: st(x, y)
    torch.manual_seed(0)
    twin = TorchTwin().cuda().train()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-4, weight_decay=1e-4)

    def torch_step():
        opt.zero_grad(set_to_none=True)
        F.l1_loss(twin(x), y).backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 8.0)
        opt.step()
    steps['torch_eager'] = torch_step
    t = alternate(steps, 10)
    for k, ts in t.items():
        row = {'what': 'step', 'model': 'ef_tran', 'variant': k, 'batch': 128, **summary(ts)}
        row['samples_per_s'] = 128 / row['median_ms'] * 1e3
        print(json.dumps(row), flush=True)


def run_trace():
    x, y = _batch()
    st = _hip_step(False)
    for _ in range(6):
        st(x, y)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'trace', 'steps': 6}))


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/attn_wide_bench.py measures on a HIP device; none is available')
    {'op': bench_op, 'core': bench_core, 'step': bench_step, 'trace': run_trace}[sys.argv[1]]()

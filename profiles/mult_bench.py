"""Timings behind profiles/mult.md: the MULT expert (dynmm_amd.nn.mult, csrc/xattn.hip) against its plain-torch twin
(tests/mult_oracle.py) running in float32 on the same device — what a MultiBench user runs.  Needs a HIP device; prints one JSON
line per measurement.

    python profiles/mult_bench.py op         # cross_attention at (B, H, dh, Tq, Tk) = (32, 10, 4, 50, 50) and (32, 10, 12, 50, 50),
                                             #   forward and forward+backward, against the masked F.scaled_dot_product_attention
    python profiles/mult_bench.py encoder    # one cross-modal transformer (E = 40, 4 layers), forward and forward+backward
    python profiles/mult_bench.py step       # ms per training step and samples/s at batch 32 and 128: eager, replayed, twin
    python profiles/mult_bench.py streams    # the eager and the replayed step with three branches against one stream
    python profiles/mult_bench.py trace      # six eager training steps at batch 32 and nothing else (the program of a
                                             #   `rocprofv3 --kernel-trace --stats -- python ... trace` run)

Method: every variant is warmed up, then timed in `ROUNDS` windows of `iters` calls between device events, the variants
alternating window by window; the figure is the median window, min and max are reported beside it.
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
from dynmm_amd.nn import affect as A         # noqa: E402
from dynmm_amd.nn import mult as MU          # noqa: E402
from tests import mult_oracle as MO          # noqa: E402

ROUNDS = 7


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


def bench_op():
    for B, H, dh, Tq, Tk in [(32, 10, 4, 50, 50), (32, 10, 12, 50, 50)]:
        g = torch.Generator().manual_seed(1)
        D = H * dh
        q, k, v = (torch.randn(B, D, T, generator=g).cuda().requires_grad_(True) for T in (Tq, Tk, Tk))
        gy = torch.randn(B, D, Tq, generator=g).cuda()
        q4, k4, v4 = (t.detach().reshape(B, H, dh, t.shape[2]).transpose(2, 3).contiguous().requires_grad_(True) for t in (q, k, v))
        gy4 = gy.reshape(B, H, dh, Tq).transpose(2, 3).contiguous()
        mask = MO.visible(Tq, Tk).cuda()
        for p in (0.0, 0.1):
            drop = (p, 9, 'attn') if p > 0 else None

            def ours_f():
                with torch.no_grad():
                    S.cross_attention(q, k, v, H, True, drop)

            def ours_fb():
                q.grad = k.grad = v.grad = None
                S.cross_attention(q, k, v, H, True, drop).backward(gy)

            def sdpa_f():
                with torch.no_grad():
                    F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, dropout_p=p)

            def sdpa_fb():
                q4.grad = k4.grad = v4.grad = None
                F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask, dropout_p=p).backward(gy4)
            t = alternate({'xattn_fwd': ours_f, 'sdpa_fwd': sdpa_f, 'xattn_fwd_bwd': ours_fb, 'sdpa_fwd_bwd': sdpa_fb}, 200)
            row = {'what': 'op', 'B': B, 'H': H, 'dh': dh, 'Tq': Tq, 'Tk': Tk, 'p': p}
            for name, ts in t.items():
                row[name] = summary(ts)
            for tag in ('fwd', 'fwd_bwd'):
                row[f'{tag}_ratio_sdpa_over_xattn'] = row[f'sdpa_{tag}']['median_ms'] / row[f'xattn_{tag}']['median_ms']
            print(json.dumps(row), flush=True)


def bench_encoder():
    B, E_, T = 32, 40, 50
    hp = MU.HParams
    kw = dict(attn_dropout=0.1, relu_dropout=hp.relu_dropout, res_dropout=hp.res_dropout, embed_dropout=hp.embed_dropout,
              attn_mask=True)
    torch.manual_seed(0)
    twin = MO.TransformerEncoder(E_, hp.num_heads, hp.layers, **kw).cuda().train()
    mine = MU.TransformerEncoder(E_, hp.num_heads, hp.layers, **kw).cuda().train()
    mine.load_state_dict(twin.state_dict(), strict=True)
    g = torch.Generator().manual_seed(2)
    xq, xk = (torch.randn(B, E_, T, generator=g).cuda().requires_grad_(True) for _ in range(2))
    tq, tk = (t.detach().transpose(1, 2).contiguous().requires_grad_(True) for t in (xq, xk))
    gy = torch.randn(B, E_, T, generator=g).cuda()
    gyt = gy.transpose(1, 2).contiguous()

    def fwd(m, a, b):
        def run():
            with torch.no_grad():
                m(a, b, b)
        return run

    def fwd_bwd(m, a, b, go):
        def run():
            m.zero_grad(set_to_none=True)
            a.grad = b.grad = None
            m(a, b, b).backward(go)
        return run
    t = alternate({'hip_fwd': fwd(mine, xq, xk), 'twin_fwd': fwd(twin, tq, tk), 'hip_fwd_bwd': fwd_bwd(mine, xq, xk, gy),
                   'twin_fwd_bwd': fwd_bwd(twin, tq, tk, gyt)}, 20)
    row = {'what': 'encoder', 'B': B, 'E': E_, 'T': T, 'layers': hp.layers, 'mode': 'train'}
    for name, ts in t.items():
        row[name] = summary(ts)
    for tag in ('fwd', 'fwd_bwd'):
        row[f'{tag}_ratio_twin_over_hip'] = row[f'twin_{tag}']['median_ms'] / row[f'hip_{tag}']['median_ms']
    print(json.dumps(row), flush=True)


def _batch(B, T=50):
    g = torch.Generator().manual_seed(3)
    x = [[torch.randn(B, T, f, generator=g).cuda() for f in (35, 74, 300)],
         [torch.full((B,), T, dtype=torch.int32, device='cuda')] * 3]
    return x, torch.randn(B, 1, generator=g).cuda()


def _hip_step(graph):
    torch.manual_seed(0)
    model = E.affect_mm_mult().cuda().train()
    return E.ExpertTrainStep(model, 'l1', lr=1e-4, weight_decay=1e-4, use_graph=graph)


def _twin_step(x, y):
    torch.manual_seed(0)
    twin = MO.mult_twin().cuda().train()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-4, weight_decay=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        F.l1_loss(twin(x), y).backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), 8.0)
        opt.step()
    return step


def bench_step():
    for B in (32, 128):
        x, y = _batch(B)
        steps = {}
        for graph in (False, True):
            st = _hip_step(graph)
            steps['hip_replayed' if graph else 'hip_eager'] = lambda st=st: st(x, y)
        steps['twin_eager'] = _twin_step(x, y)
        t = alternate(steps, 5)
        for k, ts in t.items():
            row = {'what': 'step', 'model': 'mult', 'variant': k, 'batch': B, **summary(ts)}
            row['samples_per_s'] = B / row['median_ms'] * 1e3
            print(json.dumps(row), flush=True)


def bench_streams():
    B = 32
    x, y = _batch(B)
    for branches in (True, False):
        A.BRANCH_STREAMS = branches
        steps = {}
        for graph in (False, True):
            st = _hip_step(graph)
            steps['hip_replayed' if graph else 'hip_eager'] = lambda st=st: st(x, y)
        t = alternate(steps, 5)
        for k, ts in t.items():
            print(json.dumps({'what': 'streams', 'branch_streams': branches, 'variant': k, 'batch': B, **summary(ts)}), flush=True)
    A.BRANCH_STREAMS = True


def run_trace():
    x, y = _batch(32)
    st = _hip_step(False)
    for _ in range(6):
        st(x, y)
    torch.cuda.synchronize()
    print(json.dumps({'what': 'trace', 'steps': 6, 'batch': 32}))


if __name__ == '__main__':
    if not torch.cuda.is_available():
        raise SystemExit('profiles/mult_bench.py measures on a HIP device; none is available')
    {'op': bench_op, 'encoder': bench_encoder, 'step': bench_step, 'streams': bench_streams, 'trace': run_trace}[sys.argv[1]]()

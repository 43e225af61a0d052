"""GPU: the data-parallel path on the REAL model.  Two processes share GPU 0 and exchange
gradients over gloo (the driver's 8-GPU RCCL run is not ours to launch; the code path — flat buffer, buckets,
in-place gradient protocol, overlap hooks, side-stream waits, fused optimizer on the averaged buffer — is the
one `bench.py --gpus N` / train.py use over RCCL).  Checks, bit for bit:
  * every bucket's all-reduce is launched DURING backward (overlap with the in-place gradient protocol of ops.step_scope),
  * the reduced flat gradient is identical on both ranks and equals (g_rank0 + g_rank1) / 2 of the
    un-reduced per-rank gradients,
  * after the fused SGD step both replicas hold identical parameters."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from dynmm_amd import dp, engine, ops, synth
    from dynmm_amd.nn.net import SkipGateESANet
    h, w, n = 96, 128, 3
    m = SkipGateESANet(height=h, width=w, encoder_block='NonBottleneck1D', fuse_depth_in_rgb_encoder='SE-add')
    synth.fill_state_dict(m.state_dict(), seed=rank)          # de-synchronised on purpose
    m = m.cuda().train()
    dp.broadcast_parameters(m)                                  # rank 0's weights everywhere
    m.temp, m.hard_gate = 1.0, False
    rgb, depth = synth.synth_inputs(n, h, w, seed=100 + rank, device='cuda')       # per-rank shard
    labels = [synth.synth_labels(n, h // s, w // s, seed=300 + s + rank, device='cuda') for s in (1, 8, 16, 32)]
    labels = [t.to(torch.uint8) for t in labels]
    step = engine.TrainStep(m, np.linspace(0.5, 2.0, 40), lr=0.01, loss_ratio=0.1, bucket_mb=8.0, overlap=True)
    red = step.reducer
    assert red.overlap and len(red.buckets) >= 4
    # (1) un-reduced local gradient: same body with the hook detached
    red.active = False                                           # (1) un-reduced pass: hooks ignored
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    step._body(rgb, depth, labels)
    torch.cuda.synchronize()
    local = red.flat.clone()
    m.load_state_dict(sd)                                        # undo BN running-stat updates
    red.active = True
    # (2) the real step body: buckets fly during backward
    step._body(rgb, depth, labels)
    in_bwd, nb = red.launched_in_backward, len(red.buckets)
    log = list(red.launch_log)
    red.finish()
    torch.cuda.synchronize()
    reduced = red.flat.clone()
    both = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(both, local)
    want = (both[0] + both[1]) * 0.5
    step.opt.step(step._touched, step.last['total'])
    torch.cuda.synchronize()
    n_diff = int((reduced != want).sum().item())
    manual = step.flatp.flat.clone()
    # (3) the product call: the all-reduce leaves the SUM and 1/world goes into the optimizer kernel's grad_scale
    # (no pass over the flat gradient buffer) — same parameters as the averaged path above, bit for bit (x0.5 is exact),
    # and the per-step total it returns must survive the next step's zero() (train.py keeps one per step)
    m.load_state_dict(sd)
    step.opt.buf.zero_()
    step.opt.steps.zero_()
    out1 = step(rgb, depth, labels)
    total1 = out1['total']
    t1 = float(total1.item())
    folded = step.flatp.flat.clone()
    summed = red.flat.clone()
    step(rgb, depth, labels)
    fold = (int((folded != manual).sum().item()), int((summed != both[0] + both[1]).sum().item()),
            float(total1.item()) == t1, t1)
    q.put((rank, in_bwd, nb, log, (n_diff, float((reduced - want).abs().max()), float(want.abs().max())),
           reduced.cpu().numpy(), step.flatp.flat.cpu().numpy(), float((local - want).abs().max()), fold))
    dist.barrier()
    dist.destroy_process_group()


def test_real_model_two_ranks_overlap_and_exact_mean():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, in_bwd, nb, log, exact, reduced, params, spread, fold in res:
        assert in_bwd == nb, (rank, in_bwd, nb, log)           # every bucket launched from inside backward
        assert all(where == 'backward' for _, where in log), log
        assert exact[0] == 0, (rank, exact)                      # reduced == mean of the per-rank gradients, bit for bit
        assert spread > 0                                        # the two shards really had different gradients
        assert fold[0] == 0 and fold[1] == 0, fold               # 1/world folded into the optimizer == averaged buffer
        assert fold[2] and np.isfinite(fold[3]), fold            # step k's total is not aliased by step k+1
    assert res[0][8][3] == res[1][8][3]                          # ... and is the mean over ranks on both
    assert np.array_equal(res[0][5], res[1][5])                  # replicas agree on the reduced gradient
    assert np.array_equal(res[0][6], res[1][6])                  # ... and on the updated parameters


def _rccl_worker(port, q):
    """one rank over the 'nccl' (= RCCL) backend: the collective is trivial, the code path is not — communicator
    creation on the selected device, stream-ordered all-reduce of every bucket on a weight-gradient stream DURING backward,
    stream joins, division by the world size, fused optimizer."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1',
                      DYNMM_DP_FORCE_COLLECTIVES='1')
    torch.cuda.set_device(0)
    try:
        dist.init_process_group('nccl', rank=0, world_size=1)
    except Exception as e:                                       # no RCCL on this box: report, do not fail the suite
        q.put(('skip', repr(e)))
        return
    from dynmm_amd import engine, synth
    from dynmm_amd.nn.net import SkipGateESANet
    h, w, n = 96, 128, 2
    m = SkipGateESANet(height=h, width=w, encoder_block='NonBottleneck1D', fuse_depth_in_rgb_encoder='SE-add')
    synth.fill_state_dict(m.state_dict(), seed=0)
    m = m.cuda().train()
    m.temp, m.hard_gate = 1.0, False
    rgb, depth = synth.synth_inputs(n, h, w, seed=100, device='cuda')
    labels = [synth.synth_labels(n, h // s, w // s, seed=300 + s, device='cuda').to(torch.uint8) for s in (1, 8, 16, 32)]
    from dynmm_amd import ops
    out = []
    for mode in ('wgrad', 'depth', 'comm'):    # dp.GradBucketReducer(exchange=...): where the all-reduces are enqueued
        step = engine.TrainStep(m, np.linspace(0.5, 2.0, 40), lr=0.01, loss_ratio=0.1, bucket_mb=8.0, overlap=True, exchange=mode)
        red = step.reducer
        assert red.force and red.overlap       # a 1-rank reducer normally skips the collectives: forced through RCCL here
        step._body(rgb, depth, labels)
        launched = red.launched_in_backward
        red.finish()
        torch.cuda.synchronize()
        flat = red.flat.clone()
        plan = {'wgrad': ops.exchange_stream(), 'depth': ops.side_stream()}
        if mode == 'comm':                     # the classic arrangement: asynchronous work objects from a stream of its own
            assert not red._stream_ordered
            assert red._comm_stream.cuda_stream not in {s_.cuda_stream for s_ in ops.stream_plan().streams()}
        else:
            # stream-ordered on one of the step's own streams (a fifth busy stream costs the step 10 ms: dp.py), no work objects,
            # and the step stayed inside the four-stream plan
            assert red._stream_ordered and red._comm_stream.cuda_stream == plan[mode].cuda_stream and not red._works
            assert step.census['streams'] <= ops.MAX_BUSY_STREAMS, step.census
        out.append((mode, launched, len(red.buckets), bool(torch.isfinite(flat).all().item()), float(flat.abs().sum().item())))
        red.remove_hooks()
    q.put(('ok', out))
    dist.destroy_process_group()


def test_bucket_allreduce_over_rccl_single_rank():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(60)
    if res[0] == 'skip':
        pytest.skip(f'RCCL process group unavailable: {res[1]}')
    masses = []
    for mode, launched, nb, finite, mass in res[1]:
        assert launched == nb and nb >= 4, mode          # every bucket's all-reduce went out during backward, through RCCL
        assert finite and mass > 0, mode
        masses.append(mass)
    assert max(masses) - min(masses) <= 1e-5 * max(masses), masses   # the same gradients whatever stream carried the exchange


def _eval_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from dynmm_amd import dp, engine, synth
    from dynmm_amd.nn.net import SkipGateESANet
    h, w, n = 96, 128, 2
    m = SkipGateESANet(height=h, width=w, encoder_block='NonBottleneck1D', fuse_depth_in_rgb_encoder='SE-add')
    synth.fill_state_dict(m.state_dict(), seed=0)
    m = m.cuda().eval()
    dp.broadcast_parameters(m)
    with torch.no_grad():                                        # what a few training steps on different shards leave behind:
        gen = torch.Generator(device='cuda').manual_seed(10 + rank)      # replicas that disagree on the running statistics
        for name, b in m.named_buffers():
            if name.endswith('running_mean'):
                b.add_(0.05 * torch.randn(b.shape, device='cuda', generator=gen))
            elif name.endswith('running_var'):
                b.mul_(1.0 + 0.1 * torch.rand(b.shape, device='cuda', generator=gen))
    batches = []
    for i in range(4):
        rgb, depth = synth.synth_inputs(n, h, w, seed=500 + i, device='cuda')
        batches.append((rgb, depth, synth.synth_labels(n, h, w, seed=600 + i, device='cuda').to(torch.uint8)))
    own_first = engine.evaluate(m, batches, shard=False)         # this replica's own model on the whole set
    sharded = engine.evaluate(m, batches, shard=True)            # buffers from rank 0, batches rank, rank + 2, ...
    own_after = engine.evaluate(m, batches, shard=False)         # every replica now holds rank 0's buffers
    q.put((rank, own_first[0], own_first[1].numpy(), sharded[0], sharded[1].numpy(), own_after[0], own_after[1].numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_evaluation_describes_rank0_model():
    """BatchNorm running statistics differ between the replicas; the sharded evaluate() must report the mIoU of
    ONE model — rank 0's, the one train.py checkpoints — not a mixture of per-rank models."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_eval_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, m0, cm0, ms0, cms0, ma0, cma0), (_, m1, cm1, ms1, cms1, ma1, cma1) = res
    assert not np.array_equal(cm0, cm1)                          # the two replicas were different models
    assert ms0 == ms1 and np.array_equal(cms0, cms1)             # both ranks report the same sharded result ...
    assert np.array_equal(cms0, cm0) and ms0 == m0               # ... and it is rank 0's unsharded one, exactly
    assert np.array_equal(cma1, cm0) and ma1 == m0               # rank 1 now evaluates rank 0's statistics

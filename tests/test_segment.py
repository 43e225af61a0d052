"""Label maps at inference: csrc/segment.hip (tail_argmax, argmax_resize, label_confusion), Decoder.emit_labels and the networks'
`segment`, engine.InferStep.segment, engine.evaluate(fused_labels=True) and the driver `python -m dynmm_amd.predict`.

The reference is tests/segment_oracle.py (float64, plain torch) and every comparison against float64 follows its one rule:
labels equal wherever the reference's top-1 - top-2 margin exceeds tau = 1e-5 * max|logit|, at most 0.1 % of a case's pixels
under tau (asserted on the reference).  Comparisons between two device results that take the arg-max of the SAME fp32 logits
are exact."""
import argparse
import os

import numpy as np
import pytest
import torch

from dynmm_amd import synth
from tests import segment_oracle as SO

H, W = 96, 128
GATE_KW = dict(height=H, width=W, encoder_block='NonBottleneck1D', fuse_depth_in_rgb_encoder='SE-add')


@pytest.fixture(scope='module')
def ops():
    from dynmm_amd import ops as _ops
    return _ops


class _Conv:
    """what ops.tail_argmax reads of an up-sampling's depthwise conv"""

    def __init__(self, w, b):
        self.weight, self.bias = w, b


def _tail(ops, case, border):
    x, w1, b1, w2, b2 = (t.cuda() for t in case)
    pred = ops.tail_argmax(x, _Conv(w1, b1), _Conv(w2, b2), border)
    torch.cuda.synchronize()
    return pred


def _gate_model(seed=0, **kw):
    from dynmm_amd.nn.net import SkipGateESANet
    m = SkipGateESANet(**dict(GATE_KW, **kw))
    synth.fill_state_dict(m.state_dict(), seed=seed)
    return m.cuda().eval()


# ------------------------------------------------------------------------------------------------ CPU
def test_oracle_leaves_few_pixels_under_tau():
    """For every seeded input of the GPU tests the reference's share of pixels under tau stays <= 0.1 %: the cap of the
    comparison rule cannot hide a failure."""
    for shape in SO.TAIL_SHAPES:
        for border in SO.BORDERS:
            share = SO.under_share(SO.tail_reference(shape, border))
            print(f'tail {shape} {border}: {100 * share:.4f} % under tau')
            assert share <= SO.UNDER_CAP, (shape, border, share)
    for hw, out in SO.RESIZE_CASES:
        share = SO.under_share(SO.resize_reference(hw, out))
        print(f'resize {hw} -> {out}: {100 * share:.4f} % under tau')
        assert share <= SO.UNDER_CAP, (hw, out, share)


def test_oracle_constructed_cases():
    """The two constructed border cases against the float64 composition: exact, margins >= 0.13."""
    for which in 'AB':
        x, w1, b1, w2, b2, expect = SO.constructed_case(which)
        for border in SO.BORDERS:
            lab, margin, _ = SO.labels_and_margin(SO.tail_logits(x, w1, b1, w2, b2, border))
            assert torch.equal(lab, expect[border]), (which, border)
            assert margin.min().item() >= 0.13, (which, border, margin.min().item())


def test_predict_refuses_other_datasets(tmp_path):
    from dynmm_amd import predict
    small = ['--dynamic', '--global-gate', '--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D',
             '--decoder_channels_mode', 'constant', '--no_imagenet_pretraining', '--out', str(tmp_path / 'o')]
    for ds in ('sunrgbd', 'cityscapes', 'cityscapes-with-depth', 'scenenetrgbd'):
        with pytest.raises(NotImplementedError):
            predict.main(small + ['--dataset', ds, '--dataset_dir', str(tmp_path)])
    with pytest.raises(NotImplementedError):
        predict.main(small + ['--dataset', 'nyuv2'])


def test_signatures_and_header_declare_the_entry_points():
    from dynmm_amd import lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dynmm_hip.h')).read()
    for name in ('dynmm_tail_argmax', 'dynmm_argmax_resize', 'dynmm_label_confusion'):
        assert name in lib.SIGNATURES and f'int {name}(' in header
    assert lib.ABI_VERSION == 5


# ------------------------------------------------------------------------------------------------ GPU: kernels
@pytest.mark.gpu
@pytest.mark.parametrize('border', SO.BORDERS)
@pytest.mark.parametrize('shape', SO.TAIL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tail_argmax_vs_oracle(ops, shape, border):
    pred = _tail(ops, SO.tail_case(shape), border)
    N, C, h, w = shape
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (N, 4 * h, 4 * w)
    assert int(pred.max()) < C
    SO.assert_labels(pred, SO.tail_reference(shape, border), f'tail_argmax {shape} {border}')
    if C == 1:
        assert int(pred.max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['A', 'B'])
def test_tail_argmax_constructed_borders(ops, which):
    """Zero padding pads the SECOND conv with zeros in place of out-of-range up1 VALUES (not b1, not up1 evaluated outside the
    image); replicate clamps both stages.  Exact."""
    x, w1, b1, w2, b2, expect = SO.constructed_case(which)
    for border in SO.BORDERS:
        pred = _tail(ops, (x, w1, b1, w2, b2), border).cpu().long()
        assert torch.equal(pred, expect[border]), (which, border, pred[0])


@pytest.mark.gpu
def test_tail_argmax_refusals(ops):
    from dynmm_amd.lib import DynmmHipError
    x = torch.randn(1, 65, 4, 4, device='cuda')
    conv = _Conv(torch.randn(65, 1, 3, 3, device='cuda'), torch.randn(65, device='cuda'))
    with pytest.raises(DynmmHipError, match='EUNSUPPORTED'):
        ops.tail_argmax(x, conv, conv, 'zero')
    x = torch.randn(1, 3, 4, 4, device='cuda', requires_grad=True)
    conv = _Conv(torch.randn(3, 1, 3, 3, device='cuda'), torch.randn(3, device='cuda'))
    with pytest.raises(DynmmHipError, match='inference only'):
        ops.tail_argmax(x, conv, conv, 'zero')
    with pytest.raises(DynmmHipError, match='inference only'):
        ops.argmax_resize(torch.randn(1, 3, 4, 4, device='cuda', requires_grad=True))
    with torch.no_grad():
        assert ops.tail_argmax(x, conv, conv, 'zero').shape == (1, 16, 16)
    with pytest.raises(NotImplementedError):
        ops.tail_argmax(x.detach(), conv, conv, 'reflect')


@pytest.mark.gpu
@pytest.mark.parametrize('hw,out', SO.RESIZE_CASES, ids=lambda v: 'x'.join(map(str, v)))
def test_argmax_resize(ops, hw, out):
    """bincount of its labels against a label map == the cm of ops.eval_confusion on the same logits, EXACTLY (one __device__
    function serves both kernels); against float64 interpolate + arg-max the margin rule."""
    logits, label = SO.resize_case(hw, out)
    C = SO.RESIZE_C
    pred = ops.argmax_resize(logits.cuda(), None if out == hw else out)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (SO.RESIZE_N, *out)
    cm = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    ops.eval_confusion(logits.cuda(), label.cuda(), cm)
    keep = label > 0
    want = torch.bincount((label[keep].long() - 1) * C + pred.cpu()[keep].long(), minlength=C * C).reshape(C, C)
    assert torch.equal(cm.cpu(), want)
    SO.assert_labels(pred, SO.resize_reference(hw, out), f'argmax_resize {hw} -> {out}')
    if out == hw:
        assert torch.equal(pred.cpu().long(), logits.argmax(1))          # the plain arg-max of the same fp32 logits


@pytest.mark.gpu
def test_label_confusion_exact(ops):
    C = 40
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(0, C, (3, 37, 53), generator=g).to(torch.uint8)
    label = torch.randint(0, C + 4, (3, 37, 53), generator=g).to(torch.uint8)       # void (0) and labels above C
    start = torch.randint(0, 1000, (C, C), generator=g)
    cm = start.clone().cuda()
    ops.label_confusion(pred.cuda(), label.cuda(), cm)
    keep = (label >= 1) & (label <= C)
    want = start + torch.bincount((label[keep].long() - 1) * C + pred[keep].long(), minlength=C * C).reshape(C, C)
    assert torch.equal(cm.cpu(), want)
    ops.label_confusion(pred.cuda(), label.cuda(), cm)                               # accumulates
    assert torch.equal(cm.cpu(), 2 * want - start)
    # every pixel into ONE cell
    pred1 = torch.full((2, 64, 64), 7, dtype=torch.uint8, device='cuda')
    label1 = torch.full((2, 64, 64), 12, dtype=torch.uint8, device='cuda')
    cm1 = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    ops.label_confusion(pred1, label1, cm1)
    want1 = torch.zeros(C, C, dtype=torch.int64)
    want1[11, 7] = 2 * 64 * 64
    assert torch.equal(cm1.cpu(), want1)
    # a view that starts off a 16-byte boundary takes the byte path
    cm2 = torch.zeros(C, C, dtype=torch.int64, device='cuda')
    flat_p, flat_l = pred.cuda().reshape(-1), label.cuda().reshape(-1)
    ops.label_confusion(flat_p[3:], flat_l[3:], cm2)
    keep2 = keep.reshape(-1)[3:]
    want2 = torch.bincount((label.reshape(-1)[3:][keep2].long() - 1) * C + pred.reshape(-1)[3:][keep2].long(),
                           minlength=C * C).reshape(C, C)
    assert torch.equal(cm2.cpu(), want2)


# ------------------------------------------------------------------------------------------------ GPU: models
def _check_segment(m, rgb, depth, what, exact=False):
    with torch.no_grad():
        logits = m(rgb, depth, True)
    pred = m.segment(rgb, depth)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (rgb.shape[0], H, W)
    assert m.decoder.emit_labels is False                                     # restored
    if exact:
        assert torch.equal(pred.long(), logits.argmax(1)), what
    else:
        SO.assert_labels(pred, logits.double(), what)
    return pred


@pytest.mark.gpu
@pytest.mark.parametrize('hard', [False, True], ids=['soft', 'hard'])
def test_gate_model_segment(hard):
    m = _gate_model()
    m.hard_gate, m.compact = hard, True
    m.temp = 0.1 if hard else 1.0
    rgb, depth = synth.synth_inputs(4, H, W, seed=77, device='cuda')
    pred = _check_segment(m, rgb, depth, f'SkipGateESANet hard={hard}')
    with torch.no_grad():
        _, wgt_ref = m(rgb, depth, True, True)
    pred2, wgt = m.segment(rgb, depth, return_weight=True)
    assert torch.equal(pred2, pred) and torch.equal(wgt, wgt_ref)
    m.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        m.segment(rgb, depth)
    assert m.decoder.emit_labels is False


@pytest.mark.gpu
@pytest.mark.parametrize('up', ['nearest', 'bilinear', 'learned-3x3'])
def test_gate_model_segment_other_upsamplings(up):
    """'nearest' / 'bilinear' take the arg-max of the very logits the model returns: exact.  'learned-3x3' is the fused tail
    with replicated borders: the margin rule."""
    m = _gate_model(upsampling=up)
    rgb, depth = synth.synth_inputs(2, H, W, seed=78, device='cuda')
    _check_segment(m, rgb, depth, f'SkipGateESANet {up}', exact=up in ('nearest', 'bilinear'))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['esanet', 'skip', 'one_modality'])
def test_other_models_segment(kind):
    if kind == 'esanet':
        from dynmm_amd.nn.esanet import ESANet
        m = ESANet(height=H, width=W, num_classes=40, encoder_rgb='resnet34', encoder_depth='resnet34',
                   encoder_block='NonBottleneck1D', pretrained_on_imagenet=False, fuse_depth_in_rgb_encoder='SE-add',
                   upsampling='learned-3x3-zeropad')
    elif kind == 'skip':
        from dynmm_amd.nn.net_skip import SkipESANet
        m = SkipESANet(height=H, width=W, num_classes=40, encoder_rgb='resnet34', encoder_depth='resnet34',
                       encoder_block='NonBottleneck1D', nr_decoder_blocks=[3, 3, 3], fuse_depth_in_rgb_encoder='SE-add',
                       temp=1.0, block_rule=[2, 2, 2, 2])
    else:
        from dynmm_amd.nn.esanet import ESANetOneModality
        m = ESANetOneModality(height=H, width=W, num_classes=40, encoder='resnet34', encoder_block='NonBottleneck1D',
                              channels_decoder=[128, 128, 128], nr_decoder_blocks=[3, 3, 3], pretrained_on_imagenet=False,
                              input_channels=3, weighting_in_encoder='SE-add', upsampling='learned-3x3-zeropad')
    synth.fill_state_dict(m.state_dict(), seed=1)
    m = m.cuda().eval()
    if kind == 'skip':
        # the per-stage gates draw Gumbel noise per forward: pin it, so that the logits and the labels come from ONE decision
        g = torch.Generator().manual_seed(3)
        m.gumbel_noise = [torch.empty(2, 2).exponential_(generator=g).cuda() for _ in range(4)]
    rgb, depth = synth.synth_inputs(2, H, W, seed=79, device='cuda')
    pred = _check_segment(m, rgb, depth, kind)
    out = m.segment(rgb, depth, return_weight=True)
    assert torch.equal(out[0], pred)
    m.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        m.segment(rgb, depth)


# ------------------------------------------------------------------------------------------------ GPU: engine
@pytest.mark.gpu
def test_infer_step_segment_replay_equals_eager():
    """InferStep.segment replayed == segment eager, bit for bit; logits and labels alternate on ONE step, each with its own
    correct static result ("labels" is part of both graph keys)."""
    from dynmm_amd import engine
    m = _gate_model()
    m.baseline, m.hard_gate, m.temp, m.compact = False, False, 1.0, True
    batches = [synth.synth_inputs(3, H, W, seed=910 + i, device='cuda') for i in range(3)]
    step = engine.InferStep(m)
    for rgb, depth in batches:
        ref, ref_w = m.segment(rgb, depth, return_weight=True)
        ref, ref_w = ref.clone(), ref_w.clone()
        got, got_w = step.segment(rgb, depth, return_weight=True)
        assert step.launch == 'hipGraph replay'
        assert got.dtype == torch.uint8 and torch.equal(got, ref) and torch.equal(got_w, ref_w)
    assert m.decoder.emit_labels is False
    for rgb, depth in batches:                                   # alternate the two calls three times
        with torch.no_grad():
            ref_logits = m(rgb, depth, True).clone()
        ref_labels = m.segment(rgb, depth).clone()
        logits = step(rgb, depth)
        assert logits.dtype == torch.float32 and torch.equal(logits, ref_logits)
        labels = step.segment(rgb, depth)
        assert labels.dtype == torch.uint8 and torch.equal(labels, ref_labels)
    # hard data-dependent gates with compaction: back graphs per stage-count tuple
    m.hard_gate, m.temp = True, 0.1
    for rgb, depth in batches + batches:
        ref = m.segment(rgb, depth).clone()
        assert torch.equal(step.segment(rgb, depth), ref)
    # policy='auto' is honoured
    m.hard_gate, m.baseline = False, True
    auto = engine.InferStep(m, policy='auto')
    for rgb, depth in batches + batches:
        ref = m.segment(rgb, depth).clone()
        assert torch.equal(auto.segment(rgb, depth), ref)
    assert auto._choice and all('labels' in k for k in auto._choice)
    m.train()
    with pytest.raises(RuntimeError, match='eval mode'):
        step.segment(*batches[0])


@pytest.mark.gpu
def test_evaluate_fused_labels():
    from dynmm_amd import engine
    m = _gate_model()
    C = 40
    batches = []
    for i in range(2):
        rgb, depth = synth.synth_inputs(3, H, W, seed=920 + i, device='cuda')
        batches.append((rgb, depth, synth.synth_labels(3, H, W, seed=930 + i, device='cuda').to(torch.uint8)))
    miou_d, cm_default = engine.evaluate(m, batches, hard=False)
    miou_f, cm_off = engine.evaluate(m, batches, hard=False, fused_labels=False)
    assert torch.equal(cm_default, cm_off) and miou_d == miou_f          # the default path is what it was
    miou, cm = engine.evaluate(m, batches, hard=False, fused_labels=True)
    # the confusion counted on the host from segment's labels
    want = torch.zeros(C, C, dtype=torch.int64)
    under = 0
    m.hard_gate = False
    for rgb, depth, label in batches:
        pred = m.segment(rgb, depth).cpu().long()
        lab = label.cpu().long()
        keep = lab > 0
        want += torch.bincount((lab[keep] - 1) * C + pred[keep], minlength=C * C).reshape(C, C)
        with torch.no_grad():
            logits = m(rgb, depth, True).double().cpu()
        under += SO.assert_labels(pred, logits, 'evaluate batch')
    assert torch.equal(cm, want)
    assert cm.sum() == cm_default.sum()
    # a pixel whose label changes moves one count out of a cell and into another: 2 cells' worth per pixel under tau
    moved = (cm - cm_default).abs().sum().item()
    print(f'fused vs default confusion: {moved} counts moved, {under} pixels under tau, mIoU {miou:.4f} vs {miou_d:.4f}')
    assert moved <= 2 * under
    # with an InferStep, and with labels of another size (the default path serves those)
    step = engine.InferStep(m)
    assert torch.equal(engine.evaluate(m, batches, hard=False, fused_labels=True, infer_step=step)[1], cm)
    big = [(r, d, synth.synth_labels(3, 2 * H, 2 * W, seed=940, device='cuda').to(torch.uint8)) for r, d, _ in batches]
    assert torch.equal(engine.evaluate(m, big, hard=False, fused_labels=True)[1], engine.evaluate(m, big, hard=False)[1])


@pytest.mark.gpu
def test_eval_run_passes_fused_labels(monkeypatch):
    from dynmm_amd import engine
    from dynmm_amd import eval as ev
    seen = []
    real = engine.evaluate

    def spy(*a, **kw):
        seen.append(kw.get('fused_labels'))
        return real(*a, **kw)
    monkeypatch.setattr(engine, 'evaluate', spy)
    m = _gate_model()
    rgb, depth = synth.synth_inputs(2, H, W, seed=41)
    loader = [{'image': rgb, 'depth': depth, 'label_orig': synth.synth_labels(2, H, W, seed=51).to(torch.uint8)}]
    args = argparse.Namespace(hard=False, ini=False, baseline=False, num_runs=1, mode=-1, noise=0.0)
    a = ev.run(args, m, loader, fused_labels=True)
    b = ev.run(args, m, loader)
    assert seen == [True, False] and abs(a[0] - b[0]) < 1.0


@pytest.mark.gpu
def test_predict_synthetic(tmp_path):
    """python -m dynmm_amd.predict --dataset synthetic: the files exist, are 8-bit single channel with values in 1..40, and each
    equals segment + 1 (read back with the reader the data module reads labels_40 with)."""
    from dynmm_amd import predict
    from dynmm_amd.data import _png_reader
    out = tmp_path / 'pred'
    argv = ['--dynamic', '--global-gate', '--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D',
            '--decoder_channels_mode', 'constant', '--no_imagenet_pretraining', '--dataset', 'synthetic', '--height', str(H),
            '--width', str(W), '--batch_size', '2', '--synthetic_samples', '3', '--hard', '--out', str(out)]
    maps = predict.main(argv)
    assert len(maps) == 3
    read = _png_reader()
    files = sorted(os.listdir(out))
    assert files == [f'{k:06d}.png' for k in range(3)]
    for k, name in enumerate(files):
        im = read(str(out / name))
        assert im.dtype == np.uint8 and im.shape == (H, W)
        assert im.min() >= 1 and im.max() <= 40
        assert np.array_equal(im, maps[k] + 1)
    # run() on the caller's own loader returns segment's maps
    m = _gate_model()
    rgb, depth = synth.synth_inputs(2, H, W, seed=42)
    args = argparse.Namespace(hard=True, ini=False, baseline=False)
    got = predict.run(args, m, [{'image': rgb, 'depth': depth}], use_graph=False)
    ref = m.segment(rgb.cuda(), depth.cuda()).cpu().numpy()
    assert len(got) == 2 and all(np.array_equal(g, r) for g, r in zip(got, ref))

"""NYUv2 on the HIP path: the reader (dynmm_amd.data.NYUv2), the sampler of the reference's random choices, the input kernel
(csrc/rgbd_aug.hip) against tests/nyu_aug_oracle.py, and the train / eval drivers on a tiny data set written in the reference's
layout.  CPU: decoding, file lists, class weights, sampler rules, data-parallel slices, refused data sets.  GPU: the kernel with
injected parameters, loader determinism, `python -m dynmm_amd.train` / `dynmm_amd.eval` end to end."""
import argparse
import glob
import os

import numpy as np
import pytest
import torch

from dynmm_amd import data as D
from tests import nyu_aug_oracle as O

H, W = 96, 128
SMALL = ['--dynamic', '--global-gate', '--encoder', 'resnet34', '--encoder_block', 'NonBottleneck1D',
         '--decoder_channels_mode', 'constant', '--no_imagenet_pretraining']


@pytest.fixture
def fixture(tmp_path):
    root = str(tmp_path / 'nyuv2')
    return root, O.write_fixture(root)


def bincount_weights(labels, mode, c=1.02):
    """src/datasets/dataset_base.py:166-208 restated directly"""
    n_cls = 41
    per, with_ = np.zeros(n_cls), np.zeros(n_cls)
    for lab in labels:
        h, w = lab.shape
        dist = np.bincount(lab.flatten(), minlength=n_cls)
        per += dist
        with_ += (dist > 0) * h * w
    per, with_ = per[1:], with_[1:]
    if mode == 'median_frequency':
        freq = per / with_
        return np.median(freq) / freq
    return 1 / np.log(c + per / np.sum(per))


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('raw', [False, True])
def test_decoded_store_equals_written_arrays_in_file_list_order(fixture, raw):
    root, written = fixture
    for split in ('train', 'test'):
        names, rgb, depth, depth_raw, label = written[split]
        ds = D.NYUv2(root, split, 'raw' if raw else 'refined', batch_size=2, height=H, width=W, device='cpu')
        assert ds.filenames == names and names != sorted(names)
        assert ds.rgb.dtype == torch.uint8 and ds.label.dtype == torch.uint8
        np.testing.assert_array_equal(ds.rgb.numpy(), rgb)
        np.testing.assert_array_equal(ds.label.numpy(), label)
        stored = ds.depth.numpy().view(np.uint16)                          # the int16 store holds the uint16 bits
        np.testing.assert_array_equal(stored, depth_raw if raw else depth)
        assert stored.max() == 65535 and ((stored == 0).any() == raw)
        assert ds.cameras == ['kv1'] and ds.n_classes_without_void == 40
        assert (ds.depth_mean, ds.depth_std) == (2841.94941272766, 1417.2594281672277)


def test_reader_errors(tmp_path, fixture):
    root, _ = fixture
    with pytest.raises(FileNotFoundError):
        D.NYUv2(str(tmp_path / 'missing'), 'train', device='cpu')
    with pytest.raises(ValueError):
        D.NYUv2(root, 'valid', device='cpu')


@pytest.mark.parametrize('mode', ['median_frequency', 'logarithmic'])
def test_class_weights_match_bincount_restatement(fixture, mode):
    root, written = fixture
    ds = D.NYUv2(root, 'train', device='cpu')
    ref = bincount_weights(written['train'][4], mode)
    np.testing.assert_allclose(ds.compute_class_weights(mode), ref, rtol=1e-12)
    # additive over data-parallel shards: the two ranks' histograms sum to the whole split's
    parts = [D.NYUv2(root, 'train', device='cpu', rank=r, world=2).class_counts() for r in range(2)]
    whole = ds.class_counts()
    for k in range(2):
        np.testing.assert_array_equal(parts[0][k] + parts[1][k], whole[k])
    np.testing.assert_allclose(ds.weights_from_counts(parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], mode), ref,
                               rtol=1e-12)


def test_sampler_ranges_and_branch_rules():
    n, h0, w0 = 20000, 480, 640
    p, hsv = D.draw_augmentation(np.random.default_rng(3), n, h0, w0, 480, 640, 1.0, 1.4)
    th, tw, mode, ci, cj, flip = (p[:, k].astype(np.int64) for k in range(1, 7))
    assert th.min() >= 480 and th.max() <= 672 and tw.min() >= 640 and tw.max() <= 896
    np.testing.assert_array_equal(mode, (th <= 480) | (tw <= 640))
    crop = mode == 0
    assert (ci[crop] >= 0).all() and (ci[crop] < th[crop] - 480).all() and (cj[crop] < tw[crop] - 640).all()
    assert (ci[crop] == 0).any() and (ci[crop] == th[crop] - 481).any()            # both ends of randint's range are reached
    assert ((ci[~crop] == 0) & (cj[~crop] == 0)).all()
    assert 0.45 < flip.mean() < 0.55
    assert hsv[:, 0].min() >= 0.9 and hsv[:, 0].max() <= 1.1 and hsv[:, 1].min() >= 0.9 and hsv[:, 1].max() <= 1.1
    assert hsv[:, 2].min() >= -25 and hsv[:, 2].max() <= 25 and hsv[:, 2].min() < -24 and hsv[:, 2].max() > 24
    # just above 1 the rescale-instead-of-crop branch fires (e.g. 480 x 641) and keeps its stage-1 size for the second resize
    p, _ = D.draw_augmentation(np.random.default_rng(4), 4000, h0, w0, 480, 640, 1.0, 1.003)
    r = p[p[:, 3] == 1]
    assert len(r) and ((r[:, 1] == 480) | (r[:, 2] == 640)).all() and (r[:, 2] == 641).any()
    assert (p[p[:, 3] == 0][:, 1] > 480).all()
    # deterministic per seed
    a = D.draw_augmentation(np.random.default_rng(7), 50, h0, w0, 480, 640)
    b = D.draw_augmentation(np.random.default_rng(7), 50, h0, w0, 480, 640)
    c = D.draw_augmentation(np.random.default_rng(8), 50, h0, w0, 480, 640)
    assert all((x == y).all() for x, y in zip(a, b)) and not (a[1] == c[1]).all()


def test_epoch_params_shuffle_drop_last_and_seed(fixture):
    root, _ = fixture
    ds = D.NYUv2(root, 'train', batch_size=4, height=H, width=W, device='cpu', seed=5)
    assert len(ds) == 1                                                       # 6 samples, batch 4, drop_last
    p0, h0 = ds.sample_params(0)
    assert p0.shape == (1, 4, 8) and h0.shape == (1, 4, 4) and len(set(p0[0, :, 0])) == 4
    again = D.NYUv2(root, 'train', batch_size=4, height=H, width=W, device='cpu', seed=5).sample_params(0)
    assert (again[0] == p0).all() and (again[1] == h0).all()
    orders = {tuple(ds.sample_params(e)[0][0, :, 0]) for e in range(8)}
    assert len(orders) > 1                                                    # reshuffled per epoch
    test = D.NYUv2(root, 'test', batch_size=2, height=H, width=W, device='cpu')
    assert len(test) == 2
    tp, none = test.sample_params(0)
    assert none is None and (tp[:, 0] == np.arange(3)).all() and (tp[:, 1:3] == (H, W)).all() and (tp[:, 3:] == 0).all()


def test_data_parallel_slices_are_disjoint_and_cover_the_global_batches(tmp_path):
    root = str(tmp_path / 'nyu')
    O.write_fixture(root, n_train=11, n_test=1, size=(32, 64))
    ranks = [D.NYUv2(root, 'train', batch_size=2, height=32, width=64, device='cpu', seed=1, rank=r, world=2) for r in range(2)]
    one = D.NYUv2(root, 'train', batch_size=4, height=32, width=64, device='cpu', seed=1)
    for epoch in range(3):
        (p0, h0), (p1, h1) = (r.sample_params(epoch) for r in ranks)
        assert p0.shape == p1.shape == (2, 2, 8)                                   # 11 // (2 * 2) global batches
        s0, s1 = set(p0[..., 0].ravel()), set(p1[..., 0].ravel())
        assert not (s0 & s1) and len(s0 | s1) == 8
        g, gh = one.sample_params(epoch)                                           # the same global batches at world 1
        np.testing.assert_array_equal(np.concatenate([p0, p1], axis=1), g)
        np.testing.assert_array_equal(np.concatenate([h0, h1], axis=1), gh)
    assert len(ranks[0]) == 2


def test_unsupported_datasets_are_refused(tmp_path):
    from dynmm_amd import eval as ev
    from dynmm_amd import train
    for ds in ('sunrgbd', 'cityscapes', 'cityscapes-with-depth', 'scenenetrgbd'):
        with pytest.raises(NotImplementedError):
            train.train_main(SMALL + ['--dataset', ds, '--dataset_dir', str(tmp_path), '--results_dir', str(tmp_path)])
        with pytest.raises(NotImplementedError):
            ev.main(SMALL + ['--dataset', ds, '--dataset_dir', str(tmp_path)])
    with pytest.raises(NotImplementedError):
        train.train_main(SMALL + ['--dataset', 'nyuv2', '--results_dir', str(tmp_path)])
    args = argparse.Namespace(dataset='sunrgbd', dataset_dir=str(tmp_path))
    with pytest.raises(NotImplementedError):
        D.prepare_data(args, 'cpu')


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
IMG_LSB = 1 / (255 * 0.224) + 1e-5


def assert_batch(got, ref, labels_only=False):
    lab = got['label'].cpu().numpy()
    np.testing.assert_array_equal(lab, ref['label'])
    for r in (8, 16, 32):
        np.testing.assert_array_equal(got['label_down'][r].cpu().numpy(), ref['label_down'][r])
    d = np.abs(got['depth'].cpu().numpy() - ref['depth'])
    assert d.max() <= 1e-6, d.max()
    e = np.abs(got['image'].cpu().numpy() - ref['image'])
    assert e.max() <= IMG_LSB, e.max()
    assert (e <= 1e-5).mean() >= 0.999, (e <= 1e-5).mean()


def run_kernel(store, params, hsv, h=H, w=W, raw=False):
    from dynmm_amd import ops
    rgb, depth, label = store
    dev = torch.device('cuda:0')
    t = (torch.from_numpy(rgb).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(label).to(dev))
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev)
    hv = None if hsv is None else torch.from_numpy(np.ascontiguousarray(hsv, dtype=np.float32)).to(dev)
    image, dep, lab, down = ops.rgbd_aug(*t, p, h, w, O.DEPTH_MEAN, O.DEPTH_STD, raw, hsv=hv)
    torch.cuda.synchronize()
    return {'image': image, 'depth': dep, 'label': lab, 'label_down': down}


# (src, th, tw, mode, ci, cj, flip) and (h, s, v) per case, on 96 x 128 stored samples
CASES = {
    'identity': [((0, 96, 128, 1, 0, 0, 0), (1.0, 1.0, 0.0)), ((1, 96, 128, 1, 0, 0, 1), (1.0, 1.0, 0.0))],
    'double_resize': [((2, 96, 129, 1, 0, 0, 0), (1.03, 0.95, 7.5)), ((3, 97, 128, 1, 0, 0, 1), (0.93, 1.07, -3.0))],
    'scale_1.4': [((4, 134, 179, 0, 37, 50, 0), (1.0, 1.0, 0.0)), ((5, 134, 179, 0, 0, 0, 1), (1.02, 0.98, 1.5))],
    'scale_1.2_flip': [((0, 115, 154, 0, 18, 25, 1), (0.97, 1.04, -12.0)), ((1, 115, 154, 0, 1, 1, 0), (0.97, 1.04, -12.0))],
    'hue_clip_v_plus': [((2, 110, 147, 0, 5, 9, 0), (1.1, 0.9, 25.0)), ((3, 96, 128, 1, 0, 0, 1), (1.1, 1.1, 25.0))],
    'v_minus': [((4, 120, 160, 0, 23, 31, 1), (0.9, 1.1, -25.0)), ((5, 96, 128, 1, 0, 0, 0), (0.9, 0.9, -25.0))],
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('raw', [False, True])
def test_train_kernel_matches_oracle(case, raw):
    store = O.make_arrays(6, H, W, seed=11)
    params = np.array([list(p) + [0] for p, _ in CASES[case]], np.int32)
    hsv = np.array([list(h) + [0.0] for _, h in CASES[case]], np.float32)
    got = run_kernel(store, params, hsv, raw=raw)
    ref = O.batch(store, params, hsv, H, W, raw)
    assert_batch(got, ref)
    if raw:
        zero = store[1][params[:, 0]] == 0
        assert zero.any() and (got['depth'].cpu().numpy() == 0).any()
    if case == 'hue_clip_v_plus':                     # the case reaches the clips it names
        hsv0 = O.rgb_to_hsv(store[0][2])
        assert (hsv0[..., 0] * np.float32(1.1) > 1).any() and (hsv0[..., 2] + 25 > 255).any()
    if case == 'v_minus':
        assert (O.rgb_to_hsv(store[0][4])[..., 2] - 25 < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('raw', [False, True])
def test_test_split_rescale_path(tmp_path, raw):
    """stored at 120 x 160, network at 96 x 128: Rescale (linear image, nearest depth / label); label_orig untouched"""
    from dynmm_amd import ops  # noqa: F401
    root = str(tmp_path / 'nyu')
    written = O.write_fixture(root, n_train=2, n_test=3, size=(96, 128), test_size=(120, 160))
    names, rgb, depth, depth_raw, label = written['test']
    ds = D.NYUv2(root, 'test', 'raw' if raw else 'refined', batch_size=2, height=H, width=W, device='cuda:0')
    batches = list(ds)
    assert [b['image'].shape[0] for b in batches] == [2, 1]
    params, _ = ds.sample_params(0)
    assert (params[:, 3] == 1).all()
    ref = O.batch((rgb, depth_raw if raw else depth, label), params, None, H, W, raw)
    got = {'image': torch.cat([b['image'] for b in batches]), 'depth': torch.cat([b['depth'] for b in batches]),
           'label': torch.cat([b['label'] for b in batches]),
           'label_down': {r: torch.cat([b['label_down'][r] for b in batches]) for r in (8, 16, 32)}}
    assert_batch(got, ref)
    orig = torch.cat([b['label_orig'] for b in batches]).cpu().numpy()
    assert orig.dtype == np.uint8 and orig.shape == (3, 120, 160)
    np.testing.assert_array_equal(orig, label)


@pytest.mark.gpu
def test_loader_batches_match_oracle_and_are_deterministic(fixture):
    root, written = fixture
    names, rgb, depth, _, label = written['train']
    a = D.NYUv2(root, 'train', batch_size=2, height=H, width=W, device='cuda:0', seed=3)
    b = D.NYUv2(root, 'train', batch_size=2, height=H, width=W, device='cuda:0', seed=3)
    for epoch in range(2):
        params, hsv = a.sample_params(epoch)
        for k, (x, y) in enumerate(zip(a, b)):
            assert set(x) == {'image', 'depth', 'label', 'label_down'}
            for key in ('image', 'depth', 'label'):
                assert torch.equal(x[key], y[key])
            assert all(torch.equal(x['label_down'][r], y['label_down'][r]) for r in (8, 16, 32))
            assert x['image'].shape == (2, 3, H, W) and x['depth'].shape == (2, 1, H, W) and x['label'].dtype == torch.uint8
            assert_batch(x, O.batch((rgb, depth, label), params[k], hsv[k], H, W))
        assert k == 2


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the drivers end to end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_train_and_eval_drivers_on_nyuv2(fixture, tmp_path, monkeypatch):
    from dynmm_amd import engine, train
    from dynmm_amd import eval as ev
    from dynmm_amd.src.build_model import build_model
    root, written = fixture
    seen = {}
    init, call = engine.TrainStep.__init__, engine.TrainStep.__call__

    def spy_init(self, model, class_weight, *a, **k):
        seen.setdefault('cw', np.array(class_weight, dtype=np.float64))
        return init(self, model, class_weight, *a, **k)

    def spy_call(self, image, depth, targets):
        if 'batch' not in seen:
            seen['batch'] = (image.detach().cpu().numpy().copy(), depth.detach().cpu().numpy().copy(),
                             [t.detach().cpu().numpy().copy() for t in targets])
        return call(self, image, depth, targets)
    monkeypatch.setattr(engine.TrainStep, '__init__', spy_init)
    monkeypatch.setattr(engine.TrainStep, '__call__', spy_call)
    results = str(tmp_path / 'results')
    logs = train.train_main(SMALL + ['--dataset', 'nyuv2', '--dataset_dir', root, '--results_dir', results, '--height', '96',
                                     '--width', '128', '--batch_size', '2', '--epochs', '2'])
    assert len(logs) == 2 and all(np.isfinite(r['loss_train_total']) for r in logs) and 'mIoU_test' in logs[0]
    ckpts = glob.glob(os.path.join(results, 'nyuv2', 'checkpoints_*', 'ckpt_epoch_*.pth'))
    assert ckpts
    # the class weights are the fixture's
    _, rgb, depth, _, label = written['train']
    np.testing.assert_allclose(seen['cw'], bincount_weights(label, 'median_frequency'), rtol=1e-12)
    # the first step's inputs are the fixture's samples through the reference transforms (epoch 0, --data_seed 0)
    ds = D.NYUv2(root, 'train', batch_size=2, height=H, width=W, device='cpu', seed=0)
    params, hsv = ds.sample_params(0)
    ref = O.batch((rgb, depth, label), params[0], hsv[0], H, W)
    image, dep, targets = seen['batch']
    got = {'image': torch.from_numpy(image), 'depth': torch.from_numpy(dep), 'label': torch.from_numpy(targets[0]),
           'label_down': {r: torch.from_numpy(t) for r, t in zip((8, 16, 32), targets[1:])}}
    assert_batch(got, ref)

    # eval: the checkpoint on the test split equals engine.evaluate on oracle-prepared batches
    ckpt = sorted(ckpts)[-1]
    res = ev.main(SMALL + ['--dataset', 'nyuv2', '--dataset_dir', root, '--ckpt_path', ckpt, '--height', '96', '--width',
                           '128', '--batch_size', '2'])
    p = argparse.Namespace(**vars(ev_args(SMALL + ['--height', '96', '--width', '128'])))
    p.pretrained_on_imagenet = False
    model, dev = build_model(p, n_classes=40)
    model.load_state_dict(torch.load(ckpt, map_location=dev)['state_dict'])
    if hasattr(model, 'start_weight'):
        model.start_weight()
    model.hard_gate, model.ini_stage, model.baseline = False, False, False
    _, trgb, tdepth, _, tlabel = written['test']
    tp = D.NYUv2(root, 'test', batch_size=2, height=H, width=W, device='cpu').sample_params(0)[0]

    def batches():
        for b0 in range(0, 3, 2):
            ref = O.batch((trgb, tdepth, tlabel), tp[b0:b0 + 2], None, H, W)
            yield (torch.from_numpy(ref['image']).to(dev), torch.from_numpy(ref['depth']).to(dev),
                   torch.from_numpy(tlabel[b0:b0 + 2]).to(dev))
    miou, _ = engine.evaluate(model, batches(), hard=False)
    assert len(res) == 1 and abs(res[0] - miou) < 1e-9, (res, miou)


def ev_args(argv):
    from dynmm_amd.src.args import ArgumentParserRGBDSegmentation
    p = ArgumentParserRGBDSegmentation()
    p.set_common_args()
    p.set_eval_args()
    return p.parse_args(argv)

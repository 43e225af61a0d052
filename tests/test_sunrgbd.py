"""SUNRGB-D on the HIP path: the reader (dynmm_amd.data.SUNRGBD) over four cameras with four image sizes, the sampler with
per-sample sizes, the ragged input kernel (csrc/rgbd_aug.hip dynmm_rgbd_aug_ragged) against tests/sunrgbd_oracle.py, per-camera
validation with the all-cameras figure, and `python -m dynmm_amd.sunrgbd train / eval` on a tiny data set in the reference's
layout.  Geometry: network 96 x 128; stored sizes (106, 136), (106, 146), (86, 112), (88, 118) for realsense, kv2, kv1, xtion —
two cameras larger than the network in both axes, two smaller in both, as in the real set."""
import argparse
import glob
import os

import numpy as np
import pytest
import torch

from dynmm_amd import data as D
from tests import sunrgbd_oracle as O
from tests import test_nyuv2 as T

H, W = 96, 128
SMALL = T.SMALL
CAMERAS = ['realsense', 'kv2', 'kv1', 'xtion']


@pytest.fixture(scope='module')
def fixture(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('sunrgbd'))
    return root, O.write_fixture(root)                      # 2 train + 2 test images per camera; never modified


def bincount_weights(labels, mode, c=1.02):
    """src/datasets/dataset_base.py:166-208 restated directly, each image with its own h * w"""
    n_cls = 38
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


def stored_images(ds):
    """the decoded store cut back into per-image arrays (rgb, depth as uint16, label), in store order"""
    out = []
    rgb, depth, label = ds.rgb.cpu().numpy(), ds.depth.cpu().numpy().view(np.uint16), ds.label.cpu().numpy()
    for off, h, w, zero in ds.geom.cpu().numpy():
        assert zero == 0
        out.append((rgb[off:off + h * w].reshape(h, w, 3), depth[off:off + h * w].reshape(h, w),
                    label[off:off + h * w].reshape(h, w)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('raw', [False, True])
def test_decoded_stores_equal_written_arrays(fixture, raw):
    root, written = fixture
    for split in ('train', 'test'):
        rec = written[split]
        ds = D.SUNRGBD(root, split, 'raw' if raw else 'refined', batch_size=2, height=H, width=W, device='cpu')
        assert ds.cameras == CAMERAS and ds.n_classes_without_void == 37
        assert (ds.depth_mean, ds.depth_std) == (19025.14930492213, 9880.916071806689)
        assert ds.rgb_files == rec['rgb_files'] and rec['rgb_files'] != sorted(rec['rgb_files'])
        # train: file-list order; test: grouped by camera in the order of `cameras`, file-list order within a camera
        order = list(range(8)) if split == 'train' else O.grouped(rec)
        assert ds.order == order and (split == 'train' or order != sorted(order))
        assert ds.camera_of == [rec['cameras'][i] for i in order]
        assert all(c in rec['rgb_files'][i] for c, i in zip(ds.camera_of, order))
        if raw:                                              # the raw-depth path rule
            assert ds.depth_files == [p.replace('depth_bfx', 'depth') for p in rec['depth_files']] != rec['depth_files']
        assert ds.rgb.dtype == torch.uint8 and ds.depth.dtype == torch.int16 and ds.label.dtype == torch.uint8
        assert ds.rgb.dim() == 2 and ds.depth.dim() == 1 and ds.label.dim() == 1 and ds.geom.dtype == torch.int64
        images, off = stored_images(ds), 0
        assert len(images) == 8
        for k, i in enumerate(order):
            h, w = O.SIZES[rec['cameras'][i]]
            assert ds.geom[k].tolist() == [off, h, w, 0]
            off += h * w
            np.testing.assert_array_equal(images[k][0], rec['rgb'][i])
            np.testing.assert_array_equal(images[k][1], rec['depth_raw' if raw else 'depth'][i])
            np.testing.assert_array_equal(images[k][2], rec['label'][i])
            assert (images[k][1] == 0).any() == raw
        assert off == ds.label.numel()


def test_test_split_is_grouped_by_camera_and_label_orig_is_a_view(fixture):
    root, written = fixture
    rec = written['test']
    ds = D.SUNRGBD(root, 'test', batch_size=2, height=H, width=W, device='cpu')
    assert list(ds.by_camera()) == CAMERAS and len(ds) == 4 and [len(v) for v in ds.by_camera().values()] == [1] * 4
    order = O.grouped(rec)
    for c, cam in enumerate(CAMERAS):
        lo, hi = ds.camera_range[cam]
        assert (lo, hi) == (2 * c, 2 * c + 2)
        h, w = O.SIZES[cam]
        o = int(ds.offsets[lo])
        block = ds.label[o:o + 2 * h * w].view(2, h, w)                      # what a batch's label_orig is cut from
        assert block.data_ptr() == ds.label.data_ptr() + o
        for k in range(2):
            np.testing.assert_array_equal(block[k].numpy(), rec['label'][order[lo + k]])
    with pytest.raises(ValueError):
        D.SUNRGBD(root, 'train', device='cpu').by_camera()


def _copy_lists(root, dst):
    """a data directory `dst` that shares root's files; returns its file lists for the caller to alter and write"""
    os.makedirs(dst, exist_ok=True)
    os.symlink(os.path.join(root, 'SUNRGBD'), os.path.join(dst, 'SUNRGBD'))
    lists = {}
    for s in ('train', 'test'):
        for kind in ('rgb', 'depth', 'label'):
            with open(os.path.join(root, f'{s}_{kind}.txt')) as f:
                lists[s, kind] = f.read().splitlines()
    return lists


def _write_lists(dst, lists):
    for (s, kind), v in lists.items():
        with open(os.path.join(dst, f'{s}_{kind}.txt'), 'w') as f:
            f.write(''.join(f'{p}\n' for p in v))


def test_reader_errors(tmp_path, fixture):
    root, _ = fixture
    with pytest.raises(FileNotFoundError):
        D.SUNRGBD(str(tmp_path / 'missing'), 'train', device='cpu')
    with pytest.raises(ValueError):
        D.SUNRGBD(root, 'valid', device='cpu')
    # a missing file list
    dst = str(tmp_path / 'nolist')
    lists = _copy_lists(root, dst)
    del lists['train', 'depth']
    _write_lists(dst, lists)
    with pytest.raises(FileNotFoundError):
        D.SUNRGBD(dst, 'train', device='cpu')
    D.SUNRGBD(dst, 'test', device='cpu')                                     # the other split still reads
    # lists of different lengths
    dst = str(tmp_path / 'lengths')
    lists = _copy_lists(root, dst)
    lists['train', 'label'] = lists['train', 'label'][:-1]
    _write_lists(dst, lists)
    with pytest.raises(ValueError, match='list'):
        D.SUNRGBD(dst, 'train', device='cpu')
    # a label above 37
    dst = str(tmp_path / 'label38')
    lists = _copy_lists(root, dst)
    bad = np.load(os.path.join(root, lists['train', 'label'][3])).copy()
    bad[5, 7] = 38
    np.save(os.path.join(dst, 'bad.npy'), bad)
    lists['train', 'label'][3] = 'bad.npy'
    _write_lists(dst, lists)
    with pytest.raises(ValueError, match='bad.npy'):
        D.SUNRGBD(dst, 'train', device='cpu')
    # a path that names no camera
    dst = str(tmp_path / 'nocamera')
    lists = _copy_lists(root, dst)
    os.symlink(os.path.join(root, lists['train', 'rgb'][0]), os.path.join(dst, 'webcam.png'))
    lists['train', 'rgb'][0] = 'webcam.png'
    _write_lists(dst, lists)
    with pytest.raises(ValueError, match='webcam.png'):
        D.SUNRGBD(dst, 'train', device='cpu')


def test_a_test_camera_with_two_sizes_is_refused(tmp_path):
    root = str(tmp_path / 's')
    written = O.write_fixture(root, n_train=1, n_test=2, sizes={c: (32, 64) for c in CAMERAS})
    D.SUNRGBD(root, 'test', device='cpu', height=32, width=64)
    rec = written['test']
    i = [k for k, c in enumerate(rec['cameras']) if c == 'kv2'][1]
    np.save(os.path.join(root, rec['label_files'][i]), np.zeros((32, 60), np.uint8))
    with pytest.raises(ValueError, match=rec['label_files'][i].replace(os.sep, '.')):
        D.SUNRGBD(root, 'test', device='cpu', height=32, width=64)


@pytest.mark.parametrize('mode', ['median_frequency', 'logarithmic'])
def test_class_weights_match_bincount_restatement(fixture, mode):
    root, written = fixture
    ds = D.SUNRGBD(root, 'train', device='cpu')
    ref = bincount_weights(written['train']['label'], mode)
    assert ref.shape == (37,)
    np.testing.assert_allclose(ds.compute_class_weights(mode), ref, rtol=1e-12)
    # the histogram weighs each image by its own size: treating all as one size gives other median-frequency weights
    if mode == 'median_frequency':
        per, with_ = ds.class_counts()
        assert len({lab.size for lab in written['train']['label']}) == 4
        same = sum((np.bincount(lab.flatten(), minlength=38) > 0) * (106 * 136) for lab in written['train']['label'])
        assert not np.array_equal(with_, same)
    parts = [D.SUNRGBD(root, 'train', device='cpu', rank=r, world=2).class_counts() for r in range(2)]
    whole = ds.class_counts()
    for k in range(2):
        np.testing.assert_array_equal(parts[0][k] + parts[1][k], whole[k])
    np.testing.assert_allclose(ds.weights_from_counts(parts[0][0] + parts[1][0], parts[0][1] + parts[1][1], mode), ref,
                               rtol=1e-12)


def test_sample_params_use_each_samples_own_size(tmp_path):
    root = str(tmp_path / 's')
    O.write_fixture(root, n_train=13, n_test=1)                               # 52 train images
    ds = D.SUNRGBD(root, 'train', batch_size=4, height=H, width=W, device='cpu', seed=1)
    assert len(ds) == 13
    seen_rescale = {c: 0 for c in CAMERAS}
    seen = {'th<H': 0, 'tw<W': 0}
    for epoch in range(4):
        p, hsv = ds.sample_params(epoch)
        assert p.shape == (13, 4, 8) and hsv.shape == (13, 4, 4) and p.dtype == np.int32
        p = p.reshape(-1, 8).astype(np.int64)
        assert len(set(p[:, 0])) == 52
        # the same generator stream as NYUv2.sample_params: permutation first, then one draw_augmentation over the batch
        rng = np.random.default_rng((1, epoch))
        order = rng.permutation(52)
        np.testing.assert_array_equal(p[:, 0], order)
        s = rng.uniform(1.0, 1.4, 52)
        h0, w0 = ds.sizes[order, 0], ds.sizes[order, 1]
        th, tw, mode, ci, cj = p[:, 1], p[:, 2], p[:, 3], p[:, 4], p[:, 5]
        np.testing.assert_array_equal(th, np.rint(s * h0))
        np.testing.assert_array_equal(tw, np.rint(s * w0))
        np.testing.assert_array_equal(mode, (th <= H) | (tw <= W))
        crop = mode == 0
        assert (ci[crop] >= 0).all() and (ci[crop] < th[crop] - H).all()
        assert (cj[crop] >= 0).all() and (cj[crop] < tw[crop] - W).all()
        assert (ci[~crop] == 0).all() and (cj[~crop] == 0).all()
        for k in np.nonzero(~crop)[0]:
            seen_rescale[ds.camera_of[order[k]]] += 1
        seen['th<H'] += int((th < H).sum())
        seen['tw<W'] += int((tw < W).sum())
    # only the two small cameras reach the rescale-instead-of-crop branch, and it up-samples there
    assert seen_rescale['realsense'] == seen_rescale['kv2'] == 0 and seen_rescale['kv1'] > 5 and seen_rescale['xtion'] > 5
    assert seen['th<H'] > 5 and seen['tw<W'] > 5
    again = D.SUNRGBD(root, 'train', batch_size=4, height=H, width=W, device='cpu', seed=1).sample_params(2)
    mine = ds.sample_params(2)
    assert (again[0] == mine[0]).all() and (again[1] == mine[1]).all()
    assert len({tuple(ds.sample_params(e)[0][0, :, 0]) for e in range(6)}) > 1           # reshuffled per epoch
    other = D.SUNRGBD(root, 'train', batch_size=4, height=H, width=W, device='cpu', seed=2).sample_params(2)
    assert not (other[0] == mine[0]).all()
    # data parallel: two ranks' slices are disjoint and concatenate to the world-1 batches
    ranks = [D.SUNRGBD(root, 'train', batch_size=2, height=H, width=W, device='cpu', seed=1, rank=r, world=2) for r in range(2)]
    for epoch in range(2):
        (p0, h0), (p1, h1) = (r.sample_params(epoch) for r in ranks)
        assert p0.shape == p1.shape == (13, 2, 8)
        assert not set(p0[..., 0].ravel()) & set(p1[..., 0].ravel())
        g, gh = ds.sample_params(epoch)
        np.testing.assert_array_equal(np.concatenate([p0, p1], axis=1), g)
        np.testing.assert_array_equal(np.concatenate([h0, h1], axis=1), gh)
    ds.set_epoch(3)
    assert ds.epoch == 3


def test_test_split_rows_are_mode_1_with_the_cameras_size(fixture):
    root, _ = fixture
    ds = D.SUNRGBD(root, 'test', batch_size=2, height=H, width=W, device='cpu')
    p, none = ds.sample_params(0)
    assert none is None and p.shape == (8, 8) and (p[:, 0] == np.arange(8)).all()
    for cam, (lo, hi) in ds.camera_range.items():
        assert (p[lo:hi, 1:3] == O.SIZES[cam]).all() and (p[lo:hi, 3] == 1).all() and (p[lo:hi, 4:] == 0).all()


def test_ragged_entry_is_declared_and_the_abi_version_stays():
    from dynmm_amd import lib
    assert lib.ABI_VERSION == 5
    assert 'dynmm_rgbd_aug_ragged' in lib.SIGNATURES and 'dynmm_rgbd_aug' in lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dynmm_hip.h')).read()
    assert 'int dynmm_rgbd_aug_ragged(' in header
    assert len(lib.SIGNATURES['dynmm_rgbd_aug_ragged'][1]) == 21


def _miou(cm):
    cm = cm.astype(np.float64)
    return float(np.mean(np.diag(cm) / (cm.sum(1) + cm.sum(0) - np.diag(cm) + 1e-15)) * 100)


def test_validate_adds_the_all_cameras_miou_only_with_several_cameras(monkeypatch):
    """engine.validate(all_cameras=True): the figure is asked for (train.run does), because tests/test_engine.py pins the keys of
    a plain two-camera call to the cameras alone"""
    from dynmm_amd import engine
    rng = np.random.default_rng(0)
    cms = {c: rng.integers(0, 1000, (37, 37)) for c in CAMERAS}

    def stub(model, batches, num_classes=40, losses=None, **kw):
        cm = cms[next(iter(batches))[0]]
        assert num_classes == 37
        losses.update(sum_weighted=1.0, weight_sum=2.0, sum_unweighted=3.0, pixels=4.0)
        return _miou(cm), torch.from_numpy(cm)
    monkeypatch.setattr(engine, 'evaluate', stub)
    loaders = {c: [{'image': c, 'depth': None, 'label_orig': None, 'label': None}] for c in CAMERAS}
    miou, logs = engine.validate(object(), loaders, np.ones(37), dynamic=False, num_classes=37, all_cameras=True)
    assert list(miou) == CAMERAS + ['all']
    total = sum(cms.values())
    assert abs(miou['all'] - _miou(total)) < 1e-9 and logs['mIoU_test'] == miou['all']
    assert abs(miou['all'] - np.mean([miou[c] for c in CAMERAS])) > 1e-3          # not the mean of the cameras' figures
    for c in CAMERAS:
        assert abs(logs[f'mIoU_test_{c}'] - _miou(cms[c])) < 1e-9
    assert logs['loss_test'] == 4 * 1.0 / (4 * 2.0)
    one, logs1 = engine.validate(object(), {'kv1': loaders['kv1']}, np.ones(37), dynamic=False, num_classes=37, all_cameras=True)
    assert list(one) == ['kv1'] and 'mIoU_test' not in logs1 and 'mIoU_test_kv1' in logs1
    plain, logs2 = engine.validate(object(), loaders, np.ones(37), dynamic=False, num_classes=37)
    assert list(plain) == CAMERAS and 'mIoU_test' not in logs2


def test_the_other_drivers_still_refuse_sunrgbd(tmp_path):
    from dynmm_amd import train
    with pytest.raises(NotImplementedError, match='dynmm_amd.sunrgbd'):
        train.train_main(SMALL + ['--dataset', 'sunrgbd', '--dataset_dir', str(tmp_path), '--results_dir', str(tmp_path)])
    with pytest.raises(NotImplementedError, match='prepare_sunrgbd'):
        D.prepare_data(argparse.Namespace(dataset='sunrgbd', dataset_dir=str(tmp_path)), 'cpu')
    from dynmm_amd import sunrgbd
    with pytest.raises(SystemExit):
        sunrgbd.main(['predict'])
    with pytest.raises(SystemExit):
        sunrgbd.main(['train'] + SMALL)                                       # no --dataset_dir
    assert train.class_weights(argparse.Namespace(class_weighting='None'), D.SUNRGBD).shape == (37,)
    assert train.class_weights(argparse.Namespace(class_weighting='None'), D.NYUv2).shape == (40,)


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the ragged kernel against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
IMG_LSB = 1 / (255 * 0.224) + 1e-5          # the project's bars, as tests/test_nyuv2.py assert_batch holds them


def assert_batch(got, ref):
    lab = got['label'].cpu().numpy()
    np.testing.assert_array_equal(lab, ref['label'])
    for r in (8, 16, 32):
        np.testing.assert_array_equal(got['label_down'][r].cpu().numpy(), ref['label_down'][r])
    d = np.abs(got['depth'].cpu().numpy() - ref['depth'])
    e = np.abs(got['image'].cpu().numpy() - ref['image'])
    print(f'depth max |d| {d.max():.3g}  image max |d| {e.max():.3g}  within 1e-5: {(e <= 1e-5).mean():.6f}')
    assert d.max() <= 1e-6, d.max()
    assert e.max() <= IMG_LSB, e.max()
    assert (e <= 1e-5).mean() >= 0.999, (e <= 1e-5).mean()


_STORE = {}


def store():
    """two images per camera, store order realsense, kv2, kv1, xtion, realsense, ... (index % 4 = camera); built once"""
    if not _STORE:
        samples = [O.make_sample(*O.SIZES[CAMERAS[k % 4]], seed=20 + k) for k in range(8)]
        _STORE['lists'] = tuple([s[j] for s in samples] for j in range(3))
        _STORE['flat'] = O.ragged(_STORE['lists'])
    return _STORE['lists'], _STORE['flat']


def run_ragged(flat, params, hsv, raw=False, h=H, w=W):
    from dynmm_amd import ops
    rgb, depth, label, geom = flat
    dev = torch.device('cuda:0')
    t = (torch.from_numpy(rgb).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(label).to(dev),
         torch.from_numpy(geom).to(dev))
    p = torch.from_numpy(np.ascontiguousarray(params, dtype=np.int32)).to(dev)
    hv = None if hsv is None else torch.from_numpy(np.ascontiguousarray(hsv, dtype=np.float32)).to(dev)
    image, dep, lab, down = ops.rgbd_aug_ragged(*t, p, h, w, O.DEPTH_MEAN, O.DEPTH_STD, raw, hsv=hv)
    torch.cuda.synchronize()
    return {'image': image, 'depth': dep, 'label': lab, 'label_down': down}


def size_of(src):
    return O.SIZES[CAMERAS[src % 4]]


def scaled(src, s):
    h0, w0 = size_of(src)
    return int(np.rint(s * h0)), int(np.rint(s * w0))


def row(src, s, ci=0, cj=0, flip=0):
    """the sampler's row for stored image `src` at scale s: mode by its rule, crop offsets as given"""
    th, tw = scaled(src, s)
    mode = int(th <= H or tw <= W)
    return (src, th, tw, mode, 0 if mode else ci, 0 if mode else cj, flip)


def far(src, s):
    th, tw = scaled(src, s)
    return th - H - 1, tw - W - 1


PLAIN, JIT = (1.0, 1.0, 0.0), (1.03, 0.95, 7.5)
HSV_CLIP = [h for name in ('hue_clip_v_plus', 'v_minus') for _, h in T.CASES[name]]
# every launch mixes the four stored sizes with src not monotone
RAGGED_CASES = {
    # scale 1.0: the first resize is the identity; the large cameras crop, the small ones up-sample in both axes (mode 1)
    'identity': [(row(2, 1.0), PLAIN), (row(0, 1.0, 9, 7), PLAIN), (row(3, 1.0, flip=1), PLAIN), (row(1, 1.0, 0, 17, 1), PLAIN),
                 (row(4, 1.0, 3, 0), JIT), (row(7, 1.0), JIT)],
    'crop_corners_1.4': [(row(s, 1.4, *c, f), JIT) for s, f in ((6, 0), (1, 1), (3, 0), (4, 1))
                         for c in ((0, 0), far(s, 1.4))],
    'flip': [(row(5, 1.2, 11, 20, 1), JIT), (row(2, 1.3, 4, 6, 1), PLAIN), (row(0, 1.1, 2, 3, 1), JIT), (row(7, 1.0, flip=1), JIT)],
    'up_both_axes': [(row(2, 1.0), JIT), (row(6, 1.05, flip=1), JIT), (row(3, 1.0), PLAIN), (row(1, 1.2, 5, 5), PLAIN)],
    'up_one_axis': [(row(6, 1.13), JIT), (row(0, 1.25, 1, 2), PLAIN), (row(2, 1.13, flip=1), PLAIN), (row(3, 1.09), JIT)],
    'hsv_clips': [(row(5, 1.15, 5, 9), HSV_CLIP[0]), (row(2, 1.0, flip=1), HSV_CLIP[1]), (row(4, 1.25, 23, 31, 1), HSV_CLIP[2]),
                  (row(3, 1.0), HSV_CLIP[3]), (row(6, 1.3, 2, 2), HSV_CLIP[0]), (row(1, 1.0, 1, 1), HSV_CLIP[2])],
}


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(RAGGED_CASES))
@pytest.mark.parametrize('raw', [False, True])
def test_ragged_kernel_matches_oracle(case, raw):
    lists, flat = store()
    params = np.array([list(p) + [0] for p, _ in RAGGED_CASES[case]], np.int32)
    hsv = np.array([list(h) + [0.0] for _, h in RAGGED_CASES[case]], np.float32)
    src, th, tw, mode, ci, cj, flip = (params[:, k].astype(np.int64) for k in range(7))
    h0 = np.array([size_of(s)[0] for s in src])
    w0 = np.array([size_of(s)[1] for s in src])
    assert len({size_of(s) for s in src}) >= 3 and (np.diff(src) < 0).any()          # mixed sizes, src not monotone
    # each case reaches the branch it names
    if case == 'identity':
        assert (th == h0).all() and (tw == w0).all() and {s % 4 for s in src} == {0, 1, 2, 3}
        assert (mode[(src % 4) < 2] == 0).all() and (mode[(src % 4) >= 2] == 1).all()
    if case == 'crop_corners_1.4':
        assert (mode == 0).all() and {s % 4 for s in src} == {0, 1, 2, 3}
        assert ((ci == 0) & (cj == 0)).sum() == 4 and ((ci == th - H - 1) & (cj == tw - W - 1)).sum() == 4
        assert (th == np.rint(1.4 * h0)).all()
    if case == 'flip':
        assert (flip == 1).all() and (mode == 0).any() and (mode == 1).any()
    if case == 'up_both_axes':
        assert ((mode == 1) & (th < H) & (tw < W)).sum() >= 3 and ((src == 2) & (th == 86) & (tw == 112)).any()
    if case == 'up_one_axis':
        assert ((mode == 1) & (th > H) & (tw <= W)).sum() >= 2
    got = run_ragged(flat, params, hsv, raw)
    ref = O.batch(lists, params, hsv, H, W, raw)
    assert_batch(got, ref)
    if raw:
        assert any((lists[1][s] == 0).any() for s in src) and (got['depth'].cpu().numpy() == 0).any()
    if case == 'hsv_clips':                               # the clips of test_nyuv2.CASES are reached on these images
        hsv0 = O.O.rgb_to_hsv(lists[0][5])
        assert (hsv0[..., 0] * np.float32(1.1) > 1).any() and (hsv0[..., 2] + 25 > 255).any()
        assert (O.O.rgb_to_hsv(lists[0][4])[..., 2] - 25 < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize('raw', [False, True])
def test_ragged_kernel_test_transform_down_and_up_sampling(raw):
    """Rescale + Normalize from every camera's size in one launch: the large cameras down-sample, the small ones up-sample"""
    lists, flat = store()
    src = [5, 2, 7, 0, 1, 6]
    params = np.array([[s, *size_of(s), 1, 0, 0, 0, 0] for s in src], np.int32)
    assert (params[:2, 1] > H).any() and (params[:, 1] > H).sum() == 3 and (params[:, 2] < W).sum() == 3
    assert_batch(run_ragged(flat, params, None, raw), O.batch(lists, params, None, H, W, raw))


@pytest.mark.gpu
@pytest.mark.parametrize('case', sorted(T.CASES))
def test_ragged_kernel_equals_the_uniform_kernel_on_a_uniform_store(case):
    from dynmm_amd import ops
    rgb, depth, label = T.O.make_arrays(6, H, W, seed=11)
    dev = torch.device('cuda:0')
    geom = np.zeros((6, 4), np.int64)
    geom[:, 0], geom[:, 1], geom[:, 2] = np.arange(6) * H * W, H, W
    t = (torch.from_numpy(rgb).to(dev), torch.from_numpy(depth.view(np.int16)).to(dev), torch.from_numpy(label).to(dev))
    p = torch.tensor([list(p) + [0] for p, _ in T.CASES[case]], dtype=torch.int32, device=dev)
    hv = torch.tensor([list(h) + [0.0] for _, h in T.CASES[case]], dtype=torch.float32, device=dev)
    for raw in (False, True):
        for hsv in (hv, None):
            a = ops.rgbd_aug(*t, p, H, W, T.O.DEPTH_MEAN, T.O.DEPTH_STD, raw, hsv=hsv)
            b = ops.rgbd_aug_ragged(t[0].view(-1, 3), t[1].view(-1), t[2].view(-1), torch.from_numpy(geom).to(dev), p, H, W,
                                    T.O.DEPTH_MEAN, T.O.DEPTH_STD, raw, hsv=hsv)
            for x, y in zip(a[:3], b[:3]):
                assert torch.equal(x, y)
            assert all(torch.equal(a[3][r], b[3][r]) for r in (8, 16, 32))


@pytest.mark.gpu
def test_ragged_kernel_reads_an_image_past_2_31_bytes():
    """one image whose RGB byte offset exceeds 2^31 (a whole SUNRGB-D split is about 2e9 pixels): 64-bit offsets"""
    free = torch.cuda.mem_get_info()[0]
    if free < 8 * 2 ** 30:
        pytest.skip(f'the flat stores take 4.3 GB; the device reports only {free / 2 ** 30:.1f} GB free (under 8 GB)')
    from dynmm_amd import ops
    dev = torch.device('cuda:0')
    rgb0, depth0, label0 = O.make_sample(86, 112, seed=5)
    off, m = 716_000_003, 86 * 112
    assert 3 * off > 2 ** 31
    total = off + m
    rgb = torch.empty(total, 3, dtype=torch.uint8, device=dev)
    depth = torch.empty(total, dtype=torch.int16, device=dev)
    label = torch.empty(total, dtype=torch.uint8, device=dev)
    rgb[off:] = torch.from_numpy(rgb0.reshape(m, 3)).to(dev)
    depth[off:] = torch.from_numpy(depth0.view(np.int16).reshape(m)).to(dev)
    label[off:] = torch.from_numpy(label0.reshape(m)).to(dev)
    geom = torch.tensor([[0, 86, 112, 0], [off, 86, 112, 0]], dtype=torch.int64, device=dev)
    params = np.array([[1, 120, 157, 0, 11, 13, 1, 0], [1, 86, 112, 1, 0, 0, 0, 0]], np.int32)
    hsv = np.array([list(JIT) + [0.0], list(PLAIN) + [0.0]], np.float32)
    image, dep, lab, down = ops.rgbd_aug_ragged(rgb, depth, label, geom, torch.from_numpy(params).to(dev), H, W, O.DEPTH_MEAN,
                                                O.DEPTH_STD, True, hsv=torch.from_numpy(hsv).to(dev))
    torch.cuda.synchronize()
    got = {'image': image, 'depth': dep, 'label': lab, 'label_down': down}
    params[:, 0] = 0
    assert_batch(got, O.batch(([rgb0], [depth0], [label0]), params, hsv, H, W, True))


@pytest.mark.gpu
def test_ragged_operator_refuses_bad_arguments_before_launching(monkeypatch):
    from dynmm_amd import lib, ops
    _, flat = store()
    dev = torch.device('cuda:0')
    rgb, depth, label, geom = (torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev) for a in flat)
    p = torch.tensor([[0, 106, 136, 1, 0, 0, 0, 0]], dtype=torch.int32, device=dev)
    args = (O.DEPTH_MEAN, O.DEPTH_STD)
    ops.rgbd_aug_ragged(rgb, depth, label, geom, p, H, W, *args)                   # the good call
    L = ops._lib()
    real, launches = L.dynmm_rgbd_aug_ragged, []

    def counted(*a):
        launches.append(1)
        return real(*a)
    monkeypatch.setattr(L, 'dynmm_rgbd_aug_ragged', counted)
    bad = [
        dict(W=126),                                                              # width not divisible by 4
        dict(geom=geom.to(torch.int32)), dict(geom=geom[:, :3].contiguous()), dict(geom=geom.view(-1)),
        dict(geom=geom.cpu()), dict(rgb=rgb.cpu()), dict(depth=depth.cpu()), dict(label=label.cpu()), dict(p=p.cpu()),
        dict(p=p[:, :7].contiguous()), dict(rgb=rgb.view(-1)), dict(depth=depth[:-1]),
    ]
    for kw in bad:
        a = dict(rgb=rgb, depth=depth, label=label, geom=geom, p=p, W=W)
        a.update(kw)
        with pytest.raises(lib.DynmmHipError):
            ops.rgbd_aug_ragged(a['rgb'], a['depth'], a['label'], a['geom'], a['p'], H, a['W'], *args)
    with pytest.raises(lib.DynmmHipError):
        ops.rgbd_aug_ragged(rgb, depth, label, geom, p, H, W, *args, hsv=torch.zeros(1, 4))
    assert not launches                                     # refused before the library was called
    out = ops.rgbd_aug_ragged(rgb, depth, label, geom, p, H, W, *args, label_down=False)
    assert launches == [1]
    monkeypatch.undo()
    # the C entry refuses a null geom, an unaligned one and a width it cannot vectorise
    call = [rgb.data_ptr(), depth.data_ptr(), label.data_ptr(), None, label.numel(), geom.shape[0], p.data_ptr(), None, 1, H, W,
            0.0, 1.0, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None, None, None, None]
    assert L.dynmm_rgbd_aug_ragged(*call) == lib.DYNMM_EINVAL
    call[3] = geom.data_ptr() + 8
    assert L.dynmm_rgbd_aug_ragged(*call) == lib.DYNMM_EUNSUPPORTED
    call[3], call[10] = geom.data_ptr(), 126
    assert L.dynmm_rgbd_aug_ragged(*call) == lib.DYNMM_EUNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the loader
# ---------------------------------------------------------------------------------------------------------------------------
def file_order_store(rec, raw=False):
    return rec['rgb'], rec['depth_raw' if raw else 'depth'], rec['label']


@pytest.mark.gpu
def test_train_loader_batches_match_oracle_and_are_deterministic(fixture):
    root, written = fixture
    a = D.SUNRGBD(root, 'train', batch_size=2, height=H, width=W, device='cuda:0', seed=3)
    b = D.SUNRGBD(root, 'train', batch_size=2, height=H, width=W, device='cuda:0', seed=3)
    for epoch in range(2):
        params, hsv = a.sample_params(epoch)
        for k, (x, y) in enumerate(zip(a, b)):
            assert set(x) == {'image', 'depth', 'label', 'label_down'}
            for key in ('image', 'depth', 'label'):
                assert torch.equal(x[key], y[key])
            assert all(torch.equal(x['label_down'][r], y['label_down'][r]) for r in (8, 16, 32))
            assert x['image'].shape == (2, 3, H, W) and x['depth'].shape == (2, 1, H, W) and x['label'].dtype == torch.uint8
            assert_batch(x, O.batch(file_order_store(written['train']), params[k], hsv[k], H, W))
        assert k == 3


@pytest.mark.gpu
@pytest.mark.parametrize('raw', [False, True])
def test_test_split_batches_per_camera_match_oracle(tmp_path, raw):
    root = str(tmp_path / 's')
    written = O.write_fixture(root, n_train=1, n_test=3)
    rec = written['test']
    order = O.grouped(rec)
    lists = tuple([a[i] for i in order] for a in file_order_store(rec, raw))           # the oracle's store in store order
    ds = D.SUNRGBD(root, 'test', 'raw' if raw else 'refined', batch_size=2, height=H, width=W, device='cuda:0')
    params, _ = ds.sample_params(0)
    by = ds.by_camera()
    assert list(by) == CAMERAS and len(ds) == 8
    whole = list(ds)
    assert len(whole) == 8
    n = 0
    for c, cam in enumerate(CAMERAS):
        batches = list(by[cam])
        assert [b['image'].shape[0] for b in batches] == [2, 1] == [len(b['label_orig']) for b in batches]   # a last partial batch
        lo = 3 * c
        for k, bt in enumerate(batches):
            rows = params[lo + 2 * k:lo + 2 * k + bt['image'].shape[0]]
            assert_batch(bt, O.batch(lists, rows, None, H, W, raw))
            orig = bt['label_orig']
            assert orig.dtype == torch.uint8 and tuple(orig.shape[1:]) == O.SIZES[cam]
            np.testing.assert_array_equal(orig.cpu().numpy(), np.stack([lists[2][r[0]] for r in rows]))
            assert orig.data_ptr() == ds.label.data_ptr() + int(ds.offsets[rows[0][0]])              # a view of the store
            # iterating the split yields the same batches camera after camera
            assert all(torch.equal(bt[key], whole[n][key]) for key in ('image', 'depth', 'label', 'label_orig'))
            n += 1


# ---------------------------------------------------------------------------------------------------------------------------
# GPU: the drivers end to end
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sunrgbd_train_and_eval_drivers(fixture, tmp_path, monkeypatch):
    from dynmm_amd import engine, sunrgbd
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
    size = ['--height', '96', '--width', '128', '--batch_size', '2']
    logs = sunrgbd.main(['train'] + SMALL + ['--dataset_dir', root, '--results_dir', results, '--epochs', '2'] + size)
    assert len(logs) == 2 and all(np.isfinite(r['loss_train_total']) for r in logs)
    assert all(f'mIoU_test_{c}' in logs[0] for c in CAMERAS) and 'mIoU_test' in logs[0]
    ckpts = glob.glob(os.path.join(results, 'sunrgbd', 'checkpoints_*', 'ckpt_epoch_*.pth'))
    assert ckpts
    # the class weights are the fixture's, 37 of them
    train = written['train']
    assert seen['cw'].shape == (37,)
    np.testing.assert_allclose(seen['cw'], bincount_weights(train['label'], 'median_frequency'), rtol=1e-12)
    # the first step's inputs are the fixture's samples through the reference transforms (epoch 0, --data_seed 0)
    ds = D.SUNRGBD(root, 'train', batch_size=2, height=H, width=W, device='cpu', seed=0)
    params, hsv = ds.sample_params(0)
    ref = O.batch(file_order_store(train), params[0], hsv[0], H, W)
    image, dep, targets = seen['batch']
    got = {'image': torch.from_numpy(image), 'depth': torch.from_numpy(dep), 'label': torch.from_numpy(targets[0]),
           'label_down': {r: torch.from_numpy(t) for r, t in zip((8, 16, 32), targets[1:])}}
    assert_batch(got, ref)

    # eval: per camera, the checkpoint's mIoU equals engine.evaluate(num_classes=37) on oracle-prepared batches
    ckpt = sorted(ckpts)[-1]
    per_camera = []
    res = sunrgbd.eval_main(SMALL + ['--dataset_dir', root, '--ckpt_path', ckpt] + size, per_camera=per_camera)
    p = argparse.Namespace(**vars(T.ev_args(SMALL + ['--height', '96', '--width', '128'])))
    p.pretrained_on_imagenet = False
    model, dev = build_model(p, n_classes=37)
    model.load_state_dict(torch.load(ckpt, map_location=dev)['state_dict'])
    if hasattr(model, 'start_weight'):
        model.start_weight()
    model.hard_gate, model.ini_stage, model.baseline = False, False, False
    rec = written['test']
    order = O.grouped(rec)
    lists = tuple([a[i] for i in order] for a in file_order_store(rec))
    tp = D.SUNRGBD(root, 'test', batch_size=2, height=H, width=W, device='cpu').sample_params(0)[0]
    assert len(res) == 1 and len(per_camera) == 1 and list(per_camera[0]) == CAMERAS
    total = 0
    for c, cam in enumerate(CAMERAS):
        ref = O.batch(lists, tp[2 * c:2 * c + 2], None, H, W)
        batch = (torch.from_numpy(ref['image']).to(dev), torch.from_numpy(ref['depth']).to(dev),
                 torch.from_numpy(np.stack(lists[2][2 * c:2 * c + 2])).to(dev))
        miou, cm = engine.evaluate(model, [batch], num_classes=37, hard=False)
        assert cm.shape == (37, 37)
        assert abs(per_camera[0][cam] - miou) < 1e-9, (cam, per_camera[0][cam], miou)
        total = total + cm
    assert abs(res[0] - _miou(total.numpy())) < 1e-9, (res, _miou(total.numpy()))

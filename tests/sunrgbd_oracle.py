"""numpy restatement of FusionDynMM/src/preprocessing.py for SUNRGB-D (csrc/rgbd_aug.hip, the ragged entry): the transforms of
tests/nyu_aug_oracle.py by import, with SUNRGB-D's depth statistics, over samples of DIFFERENT stored sizes, plus a writer of a
tiny data set in the layout src/datasets/sunrgbd/prepare_dataset.py writes and pytorch_dataset.py reads."""
import os

import numpy as np

from tests import nyu_aug_oracle as O
from tests.nyu_aug_oracle import make_arrays, random_hsv, resize_linear_u8, resize_nearest

DEPTH_MEAN, DEPTH_STD = 19025.14930492213, 9880.916071806689
CAMERAS = ['realsense', 'kv2', 'kv1', 'xtion']
N_CLASSES = 37
# the real set's sizes scaled to a 96 x 128 network: realsense and kv2 larger than the network in both axes, kv1 and xtion
# smaller in both (real: 531x681, 530x730, 427x561, 441x591 against 480x640)
SIZES = {'realsense': (106, 136), 'kv2': (106, 146), 'kv1': (86, 112), 'xtion': (88, 118)}


def normalize(image, depth, raw):
    """ToTensor + Normalize (preprocessing.py:164-207) with SUNRGB-D's depth mean / std"""
    im = image.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    im = (im - O.IMAGENET_MEAN[:, None, None]) / O.IMAGENET_STD[:, None, None]
    d = depth.astype(np.float32)
    dn = (d - np.float32(DEPTH_MEAN)) / np.float32(DEPTH_STD)
    if raw:
        dn[d == 0] = 0
    return im.astype(np.float32), dn[None].astype(np.float32)


def train_sample(rgb, depth, label, p, hsv, height, width, raw=False):
    """get_preprocessor(phase='train') on one stored sample of any size; p = (src, th, tw, mode, ci, cj, flip, _)"""
    _, th, tw, mode, ci, cj, flip = (int(v) for v in p[:7])
    im = resize_linear_u8(rgb, th, tw)                                   # RandomRescale
    d, lab = resize_nearest(depth, th, tw), resize_nearest(label, th, tw)
    if mode:                                                             # RandomCrop: rescale instead of crop
        assert th <= height or tw <= width
        im, d, lab = resize_linear_u8(im, height, width), resize_nearest(d, height, width), resize_nearest(lab, height, width)
    else:
        assert 0 <= ci < th - height and 0 <= cj < tw - width
        im, d, lab = im[ci:ci + height, cj:cj + width], d[ci:ci + height, cj:cj + width], lab[ci:ci + height, cj:cj + width]
    im = random_hsv(im, *hsv[:3])                                        # RandomHSV
    if flip:                                                             # RandomFlip
        im, d, lab = im[:, ::-1], d[:, ::-1], lab[:, ::-1]
    image, dn = normalize(im, d, raw)
    return image, dn, np.ascontiguousarray(lab)


def valid_sample(rgb, depth, label, height, width, raw=False):
    """get_preprocessor(phase='test'): Rescale + ToTensor + Normalize"""
    im, d, lab = resize_linear_u8(rgb, height, width), resize_nearest(depth, height, width), resize_nearest(label, height, width)
    image, dn = normalize(im, d, raw)
    return image, dn, lab


def batch(store, params, hsv, height, width, raw=False):
    """the oracle's batch for params [N, 8] (+ hsv [N, 4] for train, None for test) over store = (rgb, depth, label), each a
    list of arrays of the samples' own sizes"""
    rgb, depth, label = store
    image, dn, lab = [], [], []
    for k, p in enumerate(params):
        i = int(p[0])
        if hsv is None:
            assert tuple(p[1:4]) == label[i].shape + (1,)
            out = valid_sample(rgb[i], depth[i], label[i], height, width, raw)
        else:
            out = train_sample(rgb[i], depth[i], label[i], p, hsv[k], height, width, raw)
        for dst, v in zip((image, dn, lab), out):
            dst.append(v)
    down = {r: np.stack([resize_nearest(v, height // r, width // r) for v in lab]) for r in (8, 16, 32)}   # MultiScaleLabel
    return {'image': np.stack(image), 'depth': np.stack(dn), 'label': np.stack(lab), 'label_down': down}


def make_sample(h, w, seed):
    """one random sample (tests/nyu_aug_oracle.py make_arrays) with labels 0..37"""
    rgb, depth, label = make_arrays(1, h, w, seed)
    return rgb[0], depth[0], (label[0] % (N_CLASSES + 1)).astype(np.uint8)


def ragged(store):
    """flat rgb [T,3], depth [T], label [T] and geom [S,4] {pixel offset, H0, W0, 0} of a list store"""
    rgb, depth, label = store
    geom, off = np.zeros((len(label), 4), np.int64), 0
    for k, lab in enumerate(label):
        geom[k, :3] = off, lab.shape[0], lab.shape[1]
        off += lab.size
    return (np.concatenate([a.reshape(-1, 3) for a in rgb]), np.concatenate([a.reshape(-1) for a in depth]),
            np.concatenate([a.reshape(-1) for a in label]), geom)


def write_fixture(root, n_train=2, n_test=2, sizes=None, seed=0, test_sizes=None):
    """a tiny SUNRGB-D: n_train / n_test images PER CAMERA.  Returns {split: dict(rgb_files, depth_files, label_files, cameras,
    rgb, depth, depth_raw, label)} with the arrays as lists in FILE-LIST order.  RGB is written as PNG (exact decoding); the
    paths contain the camera names; the file lists interleave the cameras and are not sorted; the raw depth (directory `depth`)
    differs from the refined one (`depth_bfx`): zeros only in raw."""
    from PIL import Image
    sizes = sizes or SIZES
    out = {}
    for split, n in (('train', n_train), ('test', n_test)):
        entries = []
        for c, cam in enumerate(CAMERAS):
            h, w = (test_sizes or sizes)[cam] if split == 'test' else sizes[cam]
            for k in range(n):
                entries.append((cam, f'{(7 * k + 3) % 100:02d}', h, w, seed + 100 * c + k + (1000 if split == 'test' else 0)))
        rng = np.random.default_rng(seed + (1 if split == 'test' else 0))
        entries = [entries[i] for i in rng.permutation(len(entries))]
        rec = dict(rgb_files=[], depth_files=[], label_files=[], cameras=[], rgb=[], depth=[], depth_raw=[], label=[])
        for cam, name, h, w, s in entries:
            rgb, depth_raw, label = make_sample(h, w, s)
            depth = np.where(depth_raw == 0, 3000, depth_raw).astype(np.uint16)
            base = os.path.join('SUNRGBD', cam, f'{split}_{name}')
            files = {'rgb': os.path.join(base, 'image', f'{name}.png'), 'depth': os.path.join(base, 'depth_bfx', f'{name}.png'),
                     'raw': os.path.join(base, 'depth', f'{name}.png'), 'label': os.path.join(base, 'label', 'label.npy')}
            for f in files.values():
                os.makedirs(os.path.dirname(os.path.join(root, f)), exist_ok=True)
            Image.fromarray(rgb, 'RGB').save(os.path.join(root, files['rgb']))
            for key, d in (('depth', depth), ('raw', depth_raw)):
                im = Image.new('I;16', (w, h))
                im.frombytes(d.astype('<u2').tobytes())
                im.save(os.path.join(root, files[key]))
            np.save(os.path.join(root, files['label']), label)
            rec['rgb_files'].append(files['rgb'])
            rec['depth_files'].append(files['depth'])
            rec['label_files'].append(files['label'])
            rec['cameras'].append(cam)
            for key, v in (('rgb', rgb), ('depth', depth), ('depth_raw', depth_raw), ('label', label)):
                rec[key].append(v)
        for kind in ('rgb', 'depth', 'label'):
            with open(os.path.join(root, f'{split}_{kind}.txt'), 'w') as f:
                f.write(''.join(f'{p}\n' for p in rec[f'{kind}_files']))
        out[split] = rec
    return out


def grouped(rec, cameras=CAMERAS):
    """positions in the file lists in the test split's store order: camera after camera, file-list order within one"""
    return [i for c in cameras for i in range(len(rec['cameras'])) if rec['cameras'][i] == c]

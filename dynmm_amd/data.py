"""Data side of the drivers.  They accept any iterable of dict batches with the reference's keys
    'image' [N,3,H,W] f32, 'depth' [N,1,H,W] f32, 'label' [N,H,W] (0 = void),
    'label_down' {8: ..., 16: ..., 32: ...}, optionally 'label_orig'
and ship three sources:
  * NYUv2: the reference's data set (FusionDynMM/src/datasets/nyuv2) read from the layout its prepare_dataset.py writes, decoded
    once and kept on the device; each batch's inputs come from one kernel (csrc/rgbd_aug.hip) that restates
    src/preprocessing.py (RandomRescale, RandomCrop, RandomHSV, RandomFlip, Normalize, MultiScaleLabel for train; Rescale +
    Normalize for test) with per-sample random choices drawn on the host.  prepare_data() builds the (train, valid) pair of
    src/prepare_data.py;
  * SUNRGBD: the reference's other indoor set (src/datasets/sunrgbd): four cameras with four image sizes, decoded once into a
    ragged store that the same kernel family reads through a per-image size table; prepare_sunrgbd() builds its pair;
  * SyntheticRGBD: a deterministic synthetic NYUv2-shaped source for smoke runs and benchmarks."""
import os

import numpy as np
import torch

from . import dp, synth

DEPTH_MEAN = 2841.94941272766           # src/datasets/nyuv2/pytorch_dataset.py:53-58: the refined-depth statistics, used for
DEPTH_STD = 1417.2594281672277          # both depth modes
# one int32 row per output sample of csrc/rgbd_aug.hip: stored index, size after RandomRescale, mode (0 = crop, 1 = the
# rescale-instead-of-crop branch), crop offsets, flip
AUG_FIELDS = ('src', 'th', 'tw', 'mode', 'ci', 'cj', 'flip', 'pad')


class SyntheticRGBD:
    n_classes_without_void = 40
    cameras = ['kv1']
    split = 'test'

    def __init__(self, n_samples, batch_size, height=480, width=640, seed=0, device='cpu', nyu_like=True):
        self.n, self.bs, self.h, self.w, self.seed, self.device = n_samples, batch_size, height, width, seed, device
        self.nyu_like = nyu_like

    def __len__(self):
        return (self.n + self.bs - 1) // self.bs

    def __iter__(self):
        for i in range(len(self)):
            n = min(self.bs, self.n - i * self.bs)
            rgb, depth = synth.synth_inputs(n, self.h, self.w, seed=self.seed + 17 * i, device=self.device,
                                            nyu_like=self.nyu_like)
            label = synth.synth_labels(n, self.h, self.w, seed=self.seed + 17 * i + 1, device=self.device)
            down = {r: synth.synth_labels(n, self.h // r, self.w // r, seed=self.seed + 17 * i + r, device=self.device)
                    for r in (8, 16, 32)}
            yield {'image': rgb, 'depth': depth, 'label': label, 'label_down': down, 'label_orig': label}

    def class_counts(self):
        """(pixels per class, pixels of the images containing the class) over this source's label maps, void included at
        index 0 — the two histograms src/datasets/dataset_base.py:160-186 accumulates.  Additive over shards: under data
        parallel the ranks SUM them before forming the weights (dynmm_amd/train.py), so every replica uses the weights of
        the whole training set, as the reference does."""
        import numpy as np
        n_cls = self.n_classes_without_void + 1
        per_class, with_class = np.zeros(n_cls), np.zeros(n_cls)
        for i in range(len(self)):
            n = min(self.bs, self.n - i * self.bs)
            label = synth.synth_labels(n, self.h, self.w, seed=self.seed + 17 * i + 1, device='cpu')
            for img in label.reshape(n, -1).to(torch.int64):
                dist = np.bincount(img.numpy(), minlength=n_cls)[:n_cls]
                per_class += dist
                with_class += (dist > 0) * img.numel()
        return per_class, with_class

    @staticmethod
    def weights_from_counts(per_class, with_class, weight_mode='median_frequency', c=1.02):
        """src/datasets/dataset_base.py:188-208 (void = class 0 removed): median_frequency = median(f) / f with
        f = pixels of the class / pixels of the images containing it; logarithmic = 1 / log(c + p); linear = counts."""
        import numpy as np
        if weight_mode not in ('median_frequency', 'logarithmic', 'linear'):
            raise ValueError(f'unknown class weighting {weight_mode!r}')
        per_class, with_class = per_class[1:], with_class[1:]
        if weight_mode == 'linear':
            w = per_class
        elif weight_mode == 'median_frequency':
            freq = per_class / with_class
            w = np.median(freq) / freq
        else:
            w = 1.0 / np.log(c + per_class / per_class.sum())
        if np.isnan(np.sum(w)):
            raise ValueError('class weighting contains NaNs')
        return w

    def compute_class_weights(self, weight_mode='median_frequency', c=1.02):
        return self.weights_from_counts(*self.class_counts(), weight_mode=weight_mode, c=c)


def _png_reader():
    """cv2.imread(IMREAD_UNCHANGED) + BGR->RGB as src/datasets/nyuv2/pytorch_dataset.py:112-120 does when cv2 is importable,
    else PIL; 16-bit grayscale PNGs come back as exact uint16 either way."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        def read(path):
            im = cv2.imread(path, cv2.IMREAD_UNCHANGED)
            if im is None:
                raise OSError(f'cannot read {path}')
            return cv2.cvtColor(im, cv2.COLOR_BGR2RGB) if im.ndim == 3 else im
        return read
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('reading NYUv2 needs cv2 or PIL (Pillow) to decode its PNG files; neither is importable') from None

    def read(path):
        with Image.open(path) as im:
            if im.mode in ('I;16', 'I;16L', 'I;16B', 'I;16N'):
                return np.array(im, dtype=np.uint16)
            if im.mode == 'I':                                  # older Pillow widens 16-bit grayscale to int32
                a = np.asarray(im)
                if a.min() < 0 or a.max() > 65535:
                    raise ValueError(f'{path}: values outside uint16')
                return a.astype(np.uint16)
            if im.mode in ('RGB', 'L', 'P'):
                return np.array(im)
            if im.mode == 'RGBA':
                return np.array(im.convert('RGB'))
            raise ValueError(f'{path}: unsupported PNG mode {im.mode}')
    return read


class NYUv2:
    """One split of NYUv2 (40 classes) in the layout of src/datasets/nyuv2/prepare_dataset.py:
        DIR/{train,test}.txt                 file lists
        DIR/{split}/rgb/NAME.png             8-bit RGB
        DIR/{split}/depth/NAME.png           16-bit depth in mm (depth_raw/ under depth_mode='raw')
        DIR/{split}/labels_40/NAME.png       8-bit labels, 0 = void
    decoded once into device tensors (rgb [S,H0,W0,3] uint8, depth [S,H0,W0] int16 holding the uint16 values, label
    [S,H0,W0] uint8).  Iterating yields the batches DataLoader(Dataset, preprocessor) yields in src/prepare_data.py: the train
    split shuffled with drop_last, each sample through the reference's random augmentation; the test split in order, resized to
    height x width when stored at another size, with 'label_orig' (the stored label).  Labels are uint8.

    Random choices (src/preprocessing.py:82-161) come from numpy.random.default_rng((seed, epoch)): the same on every rank, which
    then takes its slice [rank * batch_size, (rank + 1) * batch_size) of every global batch of batch_size * world samples."""
    n_classes_without_void = 40
    cameras = ['kv1']
    depth_mean, depth_std = DEPTH_MEAN, DEPTH_STD
    weights_from_counts = staticmethod(SyntheticRGBD.weights_from_counts)

    def __init__(self, data_dir, split='train', depth_mode='refined', batch_size=8, height=480, width=640,
                 aug_scale=(1.0, 1.4), device='cuda', seed=0, rank=0, world=1):
        if split not in ('train', 'test'):
            raise ValueError(f'NYUv2 split must be train or test, got {split!r}')
        if depth_mode not in ('refined', 'raw'):
            raise ValueError(f'depth_mode must be refined or raw, got {depth_mode!r}')
        if not os.path.isdir(data_dir):
            raise FileNotFoundError(f'NYUv2 directory {data_dir!r} does not exist')
        self.data_dir, self.split, self.depth_mode = data_dir, split, depth_mode
        self.bs, self.h, self.w = batch_size, height, width
        self.scale_low, self.scale_high = min(aug_scale), max(aug_scale)
        self.seed, self.rank, self.world, self.device = seed, rank, world, torch.device(device)
        self.epoch = 0
        with open(os.path.join(data_dir, f'{split}.txt')) as f:
            self.filenames = [ln.strip() for ln in f if ln.strip()]
        if not self.filenames:
            raise ValueError(f'{split}.txt lists no files')
        rgb, depth, label = self._decode()
        self.n = len(self.filenames)
        self.h0, self.w0 = label.shape[1:]
        lo, hi = dp.shard_batch(self.n, rank, world)
        self._counts = self._histograms(label[lo:hi])
        self.rgb = torch.from_numpy(rgb).to(self.device)
        self.depth = torch.from_numpy(depth.view(np.int16)).to(self.device)
        self.label = torch.from_numpy(label).to(self.device)
        if split == 'test':
            self._test_params = None

    def _decode(self):
        read = _png_reader()
        ddir = 'depth_raw' if self.depth_mode == 'raw' else 'depth'
        rgb = depth = label = None
        for k, name in enumerate(self.filenames):
            def path(sub):
                return os.path.join(self.data_dir, self.split, sub, f'{name}.png')
            im, d, lab = read(path('rgb')), read(path(ddir)), read(path('labels_40'))
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError(f'{path("rgb")}: expected 8-bit RGB, got {im.dtype} {im.shape}')
            if d.dtype != np.uint16 or d.ndim != 2:
                raise ValueError(f'{path(ddir)}: expected 16-bit single-channel depth, got {d.dtype} {d.shape}')
            if lab.dtype != np.uint8 or lab.ndim != 2:
                raise ValueError(f'{path("labels_40")}: expected 8-bit single-channel labels, got {lab.dtype} {lab.shape}')
            if rgb is None:
                n, (h0, w0) = len(self.filenames), lab.shape
                rgb = np.empty((n, h0, w0, 3), np.uint8)
                depth = np.empty((n, h0, w0), np.uint16)
                label = np.empty((n, h0, w0), np.uint8)
            if im.shape[:2] != label.shape[1:] or d.shape != label.shape[1:] or lab.shape != label.shape[1:]:
                raise ValueError(f'{name}: every image of the {self.split} split must have the size of the first, '
                                 f'{label.shape[1:]} (got rgb {im.shape[:2]}, depth {d.shape}, label {lab.shape})')
            if lab.max() > self.n_classes_without_void:
                raise ValueError(f'{path("labels_40")}: label {lab.max()} > {self.n_classes_without_void}')
            rgb[k], depth[k], label[k] = im, d, lab
        return rgb, depth, label

    def _histograms(self, labels):
        n_cls = self.n_classes_without_void + 1
        per_class, with_class = np.zeros(n_cls), np.zeros(n_cls)
        for lab in labels:
            dist = np.bincount(lab.reshape(-1), minlength=n_cls)
            per_class += dist
            with_class += (dist > 0) * lab.size
        return per_class, with_class

    def class_counts(self):
        """(pixels per class, pixels of the images containing the class), void at index 0, over this rank's contiguous shard
        of the stored labels (src/datasets/dataset_base.py:160-186): summed over the ranks they are the whole split's."""
        return self._counts[0].copy(), self._counts[1].copy()

    def compute_class_weights(self, weight_mode='median_frequency', c=1.02):
        return self.weights_from_counts(*self.class_counts(), weight_mode=weight_mode, c=c)

    def set_epoch(self, epoch):
        """the shuffle and the augmentation of the next iteration are those of `epoch` (resumed runs)"""
        self.epoch = epoch

    def __len__(self):
        if self.split == 'train':
            return self.n // (self.bs * self.world)
        return (self.n + self.bs - 1) // self.bs

    def sample_params(self, epoch):
        """This rank's batches of `epoch`: (params int32 [n_batches, batch_size, 8] (AUG_FIELDS), hsv float32
        [n_batches, batch_size, 4]) for train; (params [n_samples, 8], None) for test."""
        if self.split == 'test':
            mode = 0 if (self.h0, self.w0) == (self.h, self.w) else 1       # Rescale only when the size differs
            p = np.zeros((self.n, 8), np.int32)
            p[:, 0], p[:, 1], p[:, 2], p[:, 3] = np.arange(self.n), self.h0, self.w0, mode
            return p, None
        gb = self.bs * self.world
        nb = self.n // gb
        rng = np.random.default_rng((self.seed, epoch))
        order = rng.permutation(self.n)[:nb * gb]
        p, hsv = draw_augmentation(rng, len(order), self.h0, self.w0, self.h, self.w, self.scale_low, self.scale_high)
        p[:, 0] = order
        lo = self.rank * self.bs
        p = p.reshape(nb, gb, 8)[:, lo:lo + self.bs]
        hsv = hsv.reshape(nb, gb, 4)[:, lo:lo + self.bs]
        return np.ascontiguousarray(p), np.ascontiguousarray(hsv)

    def __iter__(self):
        from . import ops
        raw = self.depth_mode == 'raw'
        if self.split == 'test':
            if self._test_params is None:
                self._test_params = torch.from_numpy(self.sample_params(0)[0]).to(self.device)
            for b0 in range(0, self.n, self.bs):
                b1 = min(b0 + self.bs, self.n)
                image, depth, label, down = ops.rgbd_aug(self.rgb, self.depth, self.label, self._test_params[b0:b1], self.h,
                                                         self.w, self.depth_mean, self.depth_std, raw)
                yield {'image': image, 'depth': depth, 'label': label, 'label_down': down, 'label_orig': self.label[b0:b1]}
            return
        p, hsv = self.sample_params(self.epoch)
        self.epoch += 1
        p, hsv = torch.from_numpy(p).to(self.device), torch.from_numpy(hsv).to(self.device)   # one upload per epoch
        for b in range(p.shape[0]):
            image, depth, label, down = ops.rgbd_aug(self.rgb, self.depth, self.label, p[b], self.h, self.w, self.depth_mean,
                                                     self.depth_std, raw, hsv=hsv[b])
            yield {'image': image, 'depth': depth, 'label': label, 'label_down': down}


def draw_augmentation(rng, n, h0, w0, height, width, scale_low=1.0, scale_high=1.4):
    """n samples' random choices of src/preprocessing.py's train transforms (the stored index left at 0): params int32 [n, 8]
    (AUG_FIELDS), hsv float32 [n, 4].  RandomRescale s ~ U(low, high), th = round(s * h0), tw = round(s * w0) (:82-106);
    RandomCrop's offsets i in [0, th - height), j in [0, tw - width), or, when th <= height or tw <= width, the second resize to
    height x width (mode 1, :109-131); RandomHSV h, s ~ U(0.9, 1.1), v ~ U(-25, 25) (:134-161); RandomFlip when rand > 0.5."""
    s = rng.uniform(scale_low, scale_high, n)
    th, tw = np.rint(s * h0).astype(np.int64), np.rint(s * w0).astype(np.int64)
    rescale = (th <= height) | (tw <= width)
    ci = np.where(rescale, 0, rng.integers(0, np.maximum(th - height, 1)))
    cj = np.where(rescale, 0, rng.integers(0, np.maximum(tw - width, 1)))
    hsv = np.zeros((n, 4), np.float32)
    hsv[:, 0] = rng.uniform(0.9, 1.1, n)
    hsv[:, 1] = rng.uniform(0.9, 1.1, n)
    hsv[:, 2] = rng.uniform(-25, 25, n)
    flip = rng.random(n) > 0.5
    p = np.zeros((n, 8), np.int32)
    p[:, 1], p[:, 2], p[:, 3], p[:, 4], p[:, 5], p[:, 6] = th, tw, rescale, ci, cj, flip
    return p, hsv


def nyuv2_split(args, split, device, rank=0, world=1, seed=0):
    bs = args.batch_size if split == 'train' else (args.batch_size_valid or args.batch_size)
    return NYUv2(args.dataset_dir, split, 'raw' if args.raw_depth else 'refined', bs, args.height, args.width,
                 aug_scale=(args.aug_scale_min, args.aug_scale_max), device=device, seed=seed, rank=rank, world=world)


def prepare_data(args, device, rank=0, world=1, seed=0):
    """src/prepare_data.py:18-163 for --dataset nyuv2: (train, valid) with valid = the test split (batch_size_valid or
    batch_size, in order).  Under data parallel each rank gets its slice of every global training batch; the valid set is whole
    on every rank (engine.evaluate shards its batches)."""
    if args.dataset != 'nyuv2':
        raise NotImplementedError(f'--dataset {args.dataset}: only nyuv2 has a reader here (dynmm_amd.data.NYUv2); SUNRGB-D '
                                  'goes through dynmm_amd.data.prepare_sunrgbd / python -m dynmm_amd.sunrgbd')
    if args.dataset_dir is None:
        raise NotImplementedError('--dataset nyuv2 needs --dataset_dir (the layout of '
                                  'src/datasets/nyuv2/prepare_dataset.py)')
    return (nyuv2_split(args, 'train', device, rank, world, seed), nyuv2_split(args, 'test', device, rank, world, seed))


SUNRGBD_DEPTH_MEAN = 19025.14930492213  # src/datasets/sunrgbd/pytorch_dataset.py:43-48: the refined-depth statistics, used for
SUNRGBD_DEPTH_STD = 9880.916071806689   # both depth modes


class _CameraBatches:
    """the test batches of one camera of a SUNRGBD split (engine.validate's {camera: loader} values)"""

    def __init__(self, ds, camera):
        self.ds, self.camera = ds, camera

    def __len__(self):
        lo, hi = self.ds.camera_range[self.camera]
        return (hi - lo + self.ds.bs - 1) // self.ds.bs

    def __iter__(self):
        return self.ds._camera_batches(self.camera)


class SUNRGBD:
    """One split of SUNRGB-D (37 classes) in the layout src/datasets/sunrgbd/prepare_dataset.py writes and pytorch_dataset.py
    reads:
        DIR/{train,test}_{rgb,depth,label}.txt   one path per sample, relative to DIR, the three lists aligned
        rgb     the listed image file (JPEG in the real set)
        depth   16-bit PNG; under depth_mode='raw' the path has 'depth_bfx' replaced by 'depth'
        label   .npy, read as uint8, 0 = void
    An image belongs to the camera whose name is a substring of its RGB path.  The four cameras store four sizes, so the split
    is decoded once into a RAGGED store on the device: flat rgb [T,3] uint8, depth [T] int16 (the uint16 bits), label [T] uint8
    with the images' pixels back to back, and geom [S,4] int64 {pixel offset, H0, W0, 0} per stored image; one kernel launch per
    batch reads any mix of sizes (csrc/rgbd_aug.hip dynmm_rgbd_aug_ragged).

    train: stored in file-list order; iterating works as NYUv2's train split does (default_rng((seed, epoch)), shuffle with
    drop-last over the global batch, per-rank slices), each sample's random choices drawn for its own stored size.
    test: stored grouped by camera, in the order of `cameras`, file-list order within a camera; every camera is one dense
    [S_c, H_c, W_c] block (all its images must share a size: engine.validate keeps one confusion matrix per camera at one
    resolution), so a batch's 'label_orig' is a view.  by_camera() gives {camera: batches}; iterating the split yields the same
    batches camera after camera, the last batch of a camera partial.  The test transform is Rescale to height x width + Normalize
    (mode 1 from the camera's size)."""
    n_classes_without_void = 37
    cameras = ['realsense', 'kv2', 'kv1', 'xtion']
    depth_mean, depth_std = SUNRGBD_DEPTH_MEAN, SUNRGBD_DEPTH_STD
    weights_from_counts = staticmethod(SyntheticRGBD.weights_from_counts)

    def __init__(self, data_dir, split='train', depth_mode='refined', batch_size=8, height=480, width=640,
                 aug_scale=(1.0, 1.4), device='cuda', seed=0, rank=0, world=1):
        if split not in ('train', 'test'):
            raise ValueError(f'SUNRGBD split must be train or test, got {split!r}')
        if depth_mode not in ('refined', 'raw'):
            raise ValueError(f'depth_mode must be refined or raw, got {depth_mode!r}')
        if not os.path.isdir(data_dir):
            raise FileNotFoundError(f'SUNRGB-D directory {data_dir!r} does not exist')
        self.data_dir, self.split, self.depth_mode = data_dir, split, depth_mode
        self.bs, self.h, self.w = batch_size, height, width
        self.scale_low, self.scale_high = min(aug_scale), max(aug_scale)
        self.seed, self.rank, self.world, self.device = seed, rank, world, torch.device(device)
        self.epoch = 0
        lists = []
        for kind in ('rgb', 'depth', 'label'):
            with open(os.path.join(data_dir, f'{split}_{kind}.txt')) as f:         # FileNotFoundError when missing
                lists.append(f.read().splitlines())
        if not len(lists[0]) == len(lists[1]) == len(lists[2]):
            raise ValueError(f'{split}_rgb.txt, {split}_depth.txt and {split}_label.txt list {len(lists[0])}, {len(lists[1])} '
                             f'and {len(lists[2])} files')
        if not lists[0]:
            raise ValueError(f'{split}_rgb.txt lists no files')
        self.rgb_files, self.depth_files, self.label_files = lists
        if depth_mode == 'raw':
            self.depth_files = [p.replace('depth_bfx', 'depth') for p in self.depth_files]
        self.n = len(self.rgb_files)
        cams = []
        for p in self.rgb_files:
            hit = [c for c in self.cameras if c in p]
            if not hit:
                raise ValueError(f'{p}: the path names none of the cameras {self.cameras}')
            cams.append(hit[0])
        # order[k] = position in the file lists of stored image k
        if split == 'train':
            self.order = list(range(self.n))
        else:
            self.order = [i for c in self.cameras for i in range(self.n) if cams[i] == c]
        self.camera_of = [cams[i] for i in self.order]
        self.camera_range, k = {}, 0                      # test: [first, last + 1) stored index per camera that has images
        if split == 'test':
            for c in self.cameras:
                n_c = self.camera_of.count(c)
                if n_c:
                    self.camera_range[c] = (k, k + n_c)
                k += n_c
        rgb, depth, label = self._decode()
        lo, hi = dp.shard_batch(self.n, rank, world)
        self._counts = self._histograms(label, lo, hi)
        self.rgb = torch.from_numpy(rgb).to(self.device)
        self.depth = torch.from_numpy(depth.view(np.int16)).to(self.device)
        self.label = torch.from_numpy(label).to(self.device)
        geom = np.zeros((self.n, 4), np.int64)
        geom[:, 0], geom[:, 1], geom[:, 2] = self.offsets, self.sizes[:, 0], self.sizes[:, 1]
        self.geom = torch.from_numpy(geom).to(self.device)
        self._test_params = None

    def _decode(self):
        def full(p):
            return os.path.join(self.data_dir, p)
        # sizes first (the .npy headers), so the flat stores are allocated once
        sizes = np.empty((self.n, 2), np.int64)
        for k, i in enumerate(self.order):
            shape = np.load(full(self.label_files[i]), mmap_mode='r').shape
            if len(shape) != 2:
                raise ValueError(f'{self.label_files[i]}: expected a 2-d label map, got shape {shape}')
            sizes[k] = shape
            if self.split == 'test':
                first = self.camera_range[self.camera_of[k]][0]
                if tuple(sizes[k]) != tuple(sizes[first]):
                    raise ValueError(f'{self.label_files[i]}: every test image of camera {self.camera_of[k]} must have the '
                                     f'size of the first, {tuple(sizes[first])} (got {tuple(sizes[k])})')
        self.sizes = sizes
        pixels = sizes[:, 0] * sizes[:, 1]
        self.offsets = np.concatenate([[0], np.cumsum(pixels)[:-1]]).astype(np.int64)
        total = int(pixels.sum())
        rgb, depth, label = np.empty((total, 3), np.uint8), np.empty(total, np.uint16), np.empty(total, np.uint8)
        read = _png_reader()
        for k, i in enumerate(self.order):
            im, d = read(full(self.rgb_files[i])), read(full(self.depth_files[i]))
            lab = np.load(full(self.label_files[i])).astype(np.uint8)
            hw = tuple(sizes[k])
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError(f'{self.rgb_files[i]}: expected 8-bit RGB, got {im.dtype} {im.shape}')
            if d.dtype != np.uint16 or d.ndim != 2:
                raise ValueError(f'{self.depth_files[i]}: expected 16-bit single-channel depth, got {d.dtype} {d.shape}')
            if im.shape[:2] != hw or d.shape != hw or lab.shape != hw:
                raise ValueError(f'{self.rgb_files[i]}: rgb {im.shape[:2]}, depth {d.shape} and label {lab.shape} differ')
            if lab.max() > self.n_classes_without_void:
                raise ValueError(f'{self.label_files[i]}: label {lab.max()} > {self.n_classes_without_void}')
            o, m = int(self.offsets[k]), int(pixels[k])
            rgb[o:o + m], depth[o:o + m], label[o:o + m] = im.reshape(m, 3), d.reshape(m), lab.reshape(m)
        return rgb, depth, label

    def _histograms(self, label, lo, hi):
        """src/datasets/dataset_base.py:166-186 over stored images [lo, hi): each image counts with its own h * w"""
        n_cls = self.n_classes_without_void + 1
        per_class, with_class = np.zeros(n_cls), np.zeros(n_cls)
        for k in range(lo, hi):
            o, m = int(self.offsets[k]), int(self.sizes[k, 0] * self.sizes[k, 1])
            dist = np.bincount(label[o:o + m], minlength=n_cls)
            per_class += dist
            with_class += (dist > 0) * m
        return per_class, with_class

    class_counts = NYUv2.class_counts
    compute_class_weights = NYUv2.compute_class_weights
    set_epoch = NYUv2.set_epoch

    def __len__(self):
        if self.split == 'train':
            return self.n // (self.bs * self.world)
        return sum((hi - lo + self.bs - 1) // self.bs for lo, hi in self.camera_range.values())

    def sample_params(self, epoch):
        """As NYUv2.sample_params; params[..., 0] indexes the ragged store (geom), and every train sample's th, tw, mode and
        crop offsets come from its own stored size.  test: one mode-1 row per stored image, in store order."""
        if self.split == 'test':
            p = np.zeros((self.n, 8), np.int32)
            p[:, 0], p[:, 1], p[:, 2], p[:, 3] = np.arange(self.n), self.sizes[:, 0], self.sizes[:, 1], 1
            return p, None
        gb = self.bs * self.world
        nb = self.n // gb
        rng = np.random.default_rng((self.seed, epoch))
        order = rng.permutation(self.n)[:nb * gb]
        p, hsv = draw_augmentation(rng, len(order), self.sizes[order, 0], self.sizes[order, 1], self.h, self.w, self.scale_low,
                                   self.scale_high)
        p[:, 0] = order
        lo = self.rank * self.bs
        p = p.reshape(nb, gb, 8)[:, lo:lo + self.bs]
        hsv = hsv.reshape(nb, gb, 4)[:, lo:lo + self.bs]
        return np.ascontiguousarray(p), np.ascontiguousarray(hsv)

    def _aug(self, params, hsv=None):
        from . import ops
        return ops.rgbd_aug_ragged(self.rgb, self.depth, self.label, self.geom, params, self.h, self.w, self.depth_mean,
                                   self.depth_std, self.depth_mode == 'raw', hsv=hsv)

    def by_camera(self):
        """{camera: iterable of test batches} for the cameras that have images, in the order of `cameras`"""
        if self.split != 'test':
            raise ValueError('by_camera() is the test split\'s')
        return {c: _CameraBatches(self, c) for c in self.camera_range}

    def _camera_batches(self, camera):
        if self._test_params is None:
            self._test_params = torch.from_numpy(self.sample_params(0)[0]).to(self.device)
        lo, hi = self.camera_range[camera]
        h0, w0 = (int(v) for v in self.sizes[lo])
        o = int(self.offsets[lo])
        block = self.label[o:o + (hi - lo) * h0 * w0].view(hi - lo, h0, w0)
        for b0 in range(lo, hi, self.bs):
            b1 = min(b0 + self.bs, hi)
            image, depth, label, down = self._aug(self._test_params[b0:b1])
            yield {'image': image, 'depth': depth, 'label': label, 'label_down': down, 'label_orig': block[b0 - lo:b1 - lo]}

    def __iter__(self):
        if self.split == 'test':
            for c in self.camera_range:
                yield from self._camera_batches(c)
            return
        p, hsv = self.sample_params(self.epoch)
        self.epoch += 1
        p, hsv = torch.from_numpy(p).to(self.device), torch.from_numpy(hsv).to(self.device)   # one upload per epoch
        for b in range(p.shape[0]):
            image, depth, label, down = self._aug(p[b], hsv[b])
            yield {'image': image, 'depth': depth, 'label': label, 'label_down': down}


def sunrgbd_split(args, split, device, rank=0, world=1, seed=0):
    bs = args.batch_size if split == 'train' else (args.batch_size_valid or args.batch_size)
    return SUNRGBD(args.dataset_dir, split, 'raw' if args.raw_depth else 'refined', bs, args.height, args.width,
                   aug_scale=(args.aug_scale_min, args.aug_scale_max), device=device, seed=seed, rank=rank, world=world)


def prepare_sunrgbd(args, device, rank=0, world=1, seed=0):
    """prepare_data's counterpart for SUNRGB-D (src/prepare_data.py:20-23): (train, valid) with valid = the test split.
    python -m dynmm_amd.sunrgbd is the command line that calls it; prepare_data itself keeps refusing --dataset sunrgbd."""
    if args.dataset_dir is None:
        raise ValueError('SUNRGB-D needs --dataset_dir (the layout of src/datasets/sunrgbd/prepare_dataset.py)')
    return (sunrgbd_split(args, 'train', device, rank, world, seed), sunrgbd_split(args, 'test', device, rank, world, seed))

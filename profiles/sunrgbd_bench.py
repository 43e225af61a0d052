"""The launches behind profiles/sunrgbd.md: the input kernels at batch 32, 480x640, to be run under
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python profiles/sunrgbd_bench.py
and read with `python profiles/sunrgbd_bench.py --read OUT` (median and range per series from the kernel trace).

Series, each WARM + LAUNCHES launches, in this order (the reader cuts the trace by it):
  uniform    dynmm_rgbd_aug on a uniform 480x640 store with the parameters of a NYUv2 epoch
  ragged_a   dynmm_rgbd_aug_ragged on the same store (geom describing it) and the same parameters
  ragged_b   dynmm_rgbd_aug_ragged on a store of the four SUNRGB-D camera sizes with a SUNRGB-D epoch's parameters"""
import csv
import glob
import os
import sys

import numpy as np

WARM, LAUNCHES, BATCH, H, W = 5, 24, 32, 480, 640
SIZES = [(531, 681), (530, 730), (427, 561), (441, 591)]           # realsense, kv2, kv1, xtion
PER_SIZE = 64


def launch():
    import torch

    from dynmm_amd import data as D
    from dynmm_amd import ops
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(0)
    n_b = WARM + LAUNCHES

    def rand_store(pixels):
        return (torch.randint(0, 256, (pixels, 3), dtype=torch.uint8, device=dev, generator=g),
                torch.randint(0, 30000, (pixels,), dtype=torch.int16, device=dev, generator=g),
                torch.randint(0, 38, (pixels,), dtype=torch.uint8, device=dev, generator=g))

    def epoch(sizes, rng):
        src = rng.integers(0, len(sizes), n_b * BATCH)
        p, hsv = D.draw_augmentation(rng, len(src), sizes[src, 0], sizes[src, 1], H, W)
        p[:, 0] = src
        return (torch.from_numpy(p.reshape(n_b, BATCH, 8)).to(dev), torch.from_numpy(hsv.reshape(n_b, BATCH, 4)).to(dev))

    def geom_of(sizes):
        px = sizes[:, 0] * sizes[:, 1]
        geom = np.zeros((len(sizes), 4), np.int64)
        geom[:, 0], geom[:, 1], geom[:, 2] = np.concatenate([[0], np.cumsum(px)[:-1]]), sizes[:, 0], sizes[:, 1]
        return torch.from_numpy(geom).to(dev), int(px.sum())

    # (a) a uniform store, the parameters of a NYUv2 epoch
    S = 4 * PER_SIZE
    sizes_a = np.tile(np.array([[H, W]], np.int64), (S, 1))
    geom_a, total = geom_of(sizes_a)
    rgb, depth, label = rand_store(total)
    p, hsv = epoch(sizes_a, np.random.default_rng(1))
    for b in range(n_b):
        ops.rgbd_aug(rgb.view(S, H, W, 3), depth.view(S, H, W), label.view(S, H, W), p[b], H, W, D.DEPTH_MEAN, D.DEPTH_STD,
                     hsv=hsv[b])
    torch.cuda.synchronize()
    for b in range(n_b):
        ops.rgbd_aug_ragged(rgb, depth, label, geom_a, p[b], H, W, D.DEPTH_MEAN, D.DEPTH_STD, hsv=hsv[b])
    torch.cuda.synchronize()
    del rgb, depth, label
    # (b) the four camera sizes, interleaved in the store, the parameters of a SUNRGB-D epoch
    sizes_b = np.array(SIZES * PER_SIZE, np.int64)
    geom_b, total = geom_of(sizes_b)
    rgb, depth, label = rand_store(total)
    p, hsv = epoch(sizes_b, np.random.default_rng(2))
    mode1 = float((p[..., 3] == 1).float().mean())
    for b in range(n_b):
        ops.rgbd_aug_ragged(rgb, depth, label, geom_b, p[b], H, W, D.SUNRGBD_DEPTH_MEAN, D.SUNRGBD_DEPTH_STD, hsv=hsv[b])
    torch.cuda.synchronize()
    print(f'launched 3 x {n_b}; rescale-instead-of-crop share of (b): {mode1:.3f}')


def read(out_dir):
    rows = []
    for path in glob.glob(os.path.join(out_dir, '**', '*kernel_trace.csv'), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if 'rgbd_aug' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    us = {'uniform': [], 'ragged': []}
    for r in rows:
        us['ragged' if 'ragged' in r['Kernel_Name'] else 'uniform'].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    n_b = WARM + LAUNCHES
    assert len(us['uniform']) == n_b and len(us['ragged']) == 2 * n_b, (len(us['uniform']), len(us['ragged']))
    series = {'uniform': us['uniform'][WARM:], 'ragged_a': us['ragged'][WARM:n_b], 'ragged_b': us['ragged'][n_b + WARM:]}
    for name, v in series.items():
        print(f'{name}: {len(v)} launches, median {np.median(v):.1f} us, range {min(v):.1f}-{max(v):.1f} us')
    for key in ('VGPR_Count', 'Accum_VGPR_Count', 'SGPR_Count', 'LDS_Block_Size', 'Scratch_Size', 'Private_Segment_Size'):
        if key in rows[0]:
            print(key, {('ragged' if 'ragged' in r['Kernel_Name'] else 'uniform'): r[key] for r in rows})


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if len(sys.argv) > 2 and sys.argv[1] == '--read':
        read(sys.argv[2])
    else:
        launch()

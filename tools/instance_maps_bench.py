"""Timing of the instance ground truth: mpsr_instance_images for 8 frames of 375 x 1242 with 20
boxes each, mpsr_instance_xyz_crops for B = 32 and B = 256 at 48 x 48, the command line's frames/s end to end (PNG
reads and writes included) and the host time of build_training_sample.

    python tools/instance_maps_bench.py                 # event times per launch, CLI frames/s, sample build time
    rocprofv3 --kernel-trace --stats -d out -- python tools/instance_maps_bench.py --kernels-only

--kernels-only launches each kernel `--reps` times and nothing else (a run of its own for the profiler).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils as iu, kitti_dataset  # noqa: E402

P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
H, W = 375, 1242


def _labels(rng, n):
    rows = []
    for _ in range(n):
        z = rng.uniform(6, 40)
        x = rng.uniform(-0.4, 0.4) * z
        u = 609.6 + 721.5 * x / z
        v = 172.9 + 721.5 * 1.0 / z
        hw = 721.5 * 2.0 / z
        rows.append('Car 0.00 0 %.2f %.2f %.2f %.2f %.2f 1.50 1.62 3.88 %.2f 1.60 %.2f %.2f' % (
            rng.uniform(-3, 3), max(u - hw, 0), max(v - hw / 2, 0), min(u + hw, W - 1), min(v + hw / 2, H - 1), x, z,
            rng.uniform(-3, 3)))
    return '\n'.join(rows) + '\n'


def _frames(rng, nf):
    depth = (rng.uniform(2, 60, (nf, H, W)) * (rng.uniform(size=(nf, H, W)) > 0.1)).astype(np.float32)
    return depth


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--reps', type=int, default=50)
    a = ap.parse_args()
    from monopsr_amd.datasets.kitti import obj_utils
    rng = np.random.default_rng(0)
    depth = torch.from_numpy(_frames(rng, 8)).cuda()
    texts = [_labels(rng, 20) for _ in range(8)]
    tables = [iu.instance_box_table(obj_utils.parse_labels(t)) for t in texts]
    images = iu.instance_images_from_tables(depth, [P2] * 8, tables)
    crops = {}
    for b in (32, 256):
        fi = rng.integers(0, 8, b).astype(np.int32)
        ids = rng.integers(0, 20, b).astype(np.int32)
        y1, x1 = rng.uniform(100, 250, b), rng.uniform(0, 1000, b)
        b2 = np.stack([y1, x1, y1 + rng.uniform(20, 120, b), x1 + rng.uniform(20, 240, b)], 1).astype(np.float32)
        b3 = np.tile(np.array([[1, 1.6, 20, 3.9, 1.6, 1.5, 0.3]], np.float32), (b, 1))
        va = rng.uniform(-0.5, 0.5, b).astype(np.float32)
        crops[b] = (fi, ids, b2, b3, va)
    p2s = np.tile(P2.astype(np.float32)[None], (8, 1, 1))
    run_img = lambda: iu.instance_images_from_tables(depth, [P2] * 8, tables)
    run_crop = {b: (lambda c=c: iu.instance_xyz_crops(depth, images, p2s, *c)) for b, c in crops.items()}
    if a.kernels_only:
        for _ in range(a.reps):
            run_img()
            for b in run_crop:
                run_crop[b]()
        torch.cuda.synchronize()
        return
    print('instance images, 8 frames %dx%d, 20 boxes each: %.3f ms per launch (host wrapper included)'
          % (H, W, _timed(run_img, a.reps)))
    for b in run_crop:
        print('crops B=%d, 48x48: %.3f ms per call (host wrapper included)' % (b, _timed(run_crop[b], a.reps)))
    with tempfile.TemporaryDirectory() as tmp:
        for d in ('label_2', 'calib', 'image_2', 'depth', 'instance'):
            os.makedirs(os.path.join(tmp, d))
        names = ['%06d' % i for i in range(16)]
        for i, n in enumerate(names):
            with open(os.path.join(tmp, 'label_2', n + '.txt'), 'w') as f:
                f.write(texts[i % 8])
            with open(os.path.join(tmp, 'calib', n + '.txt'), 'w') as f:
                f.write('P2: %s\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n'
                        % ' '.join('%.12e' % v for v in P2.reshape(-1)))
            depth_map_utils.save_depth_map(os.path.join(tmp, 'depth', n + '.png'), depth[i % 8].cpu().numpy())
            Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(
                os.path.join(tmp, 'image_2', n + '.png'))
        iu.save_instance_images(tmp, os.path.join(tmp, 'depth'), os.path.join(tmp, 'instance'), names[:8])
        t0 = time.perf_counter()
        iu.save_instance_images(tmp, os.path.join(tmp, 'depth'), os.path.join(tmp, 'instance'), names)
        dt = time.perf_counter() - t0
        print('command line: %.1f frames/s end to end (%d frames, PNG I/O included)' % (len(names) / dt, len(names)))
        flt = dict(kitti_dataset.DEFAULT_OBJ_FILTER, difficulty_str='all', truncation=None, depth_range=None)
        kitti_dataset.build_training_sample(tmp, names[0], os.path.join(tmp, 'depth'), os.path.join(tmp, 'instance'),
                                            np.random.default_rng(0), obj_filter=flt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for n in names:
            kitti_dataset.build_training_sample(tmp, n, os.path.join(tmp, 'depth'), os.path.join(tmp, 'instance'),
                                                np.random.default_rng(0), obj_filter=flt)
        torch.cuda.synchronize()
        print('build_training_sample: %.1f ms per sample (32 boxes, PNG reads included)'
              % ((time.perf_counter() - t0) * 1e3 / len(names)))


if __name__ == '__main__':
    main()

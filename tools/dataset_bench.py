"""Samples per second of the two ways to build a KITTI training sample, on a synthetic split of 375 x 1242 frames:

  (a) kitti_dataset.build_training_sample in a loop: three PNG reads, host arithmetic and one crop launch per sample;
  (b) KittiDataset.next_batch at batch sizes 1 and 8 with box_jitter_type 'oversample': the split resident on the card.

Each window runs for at least --seconds after a warm-up, with a device synchronise after every batch.  Also printed:
the load time and resident_bytes.  --image-aug reference|composed turns aug_config.use_image_aug on for (b): the
frames are then gathered, noised and converted by one mpsr_image_noise launch per batch.  --kernels-only runs batches
alone, for
    rocprofv3 --kernel-trace --stats -- python tools/dataset_bench.py --kernels-only
Numbers: DESIGN.md section 7.4.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monopsr_amd.core.config_utils import ConfigObj  # noqa: E402
from monopsr_amd.datasets.kitti import kitti_dataset  # noqa: E402

H, W = 375, 1242
P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])


def make_split(top, n_frames, seed=0):
    """dataset_dir `top`: train.txt and training/ with seeded RGB, depth and instance PNGs and 1-12 cars per frame."""
    split = os.path.join(top, 'training')
    dirs = ('label_2', 'calib', 'image_2', 'depth_2_multiscale', 'instance_2_depth_2_multiscale')
    for d in dirs:
        os.makedirs(os.path.join(split, d))
    rng = np.random.default_rng(seed)
    names = ['%06d' % i for i in range(n_frames)]
    calib = 'P2: %s\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: 0 -1 0 0 0 0 -1 0 1 0 0 0\n' % \
        ' '.join('%.12e' % v for v in P2.reshape(-1))
    for name in names:
        n_cars = int(rng.integers(1, 13))
        depth = rng.uniform(3, 60, (H, W))
        inst = np.full((H, W), 255, np.uint8)
        rows = []
        for k in range(n_cars):
            z = rng.uniform(6, 44)
            bw, bh = rng.uniform(40, 300), rng.uniform(30, 150)
            x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
            x = (x1 + bw / 2 - P2[0, 2]) * z / P2[0, 0]
            rows.append('Car 0.00 0 %.2f %.2f %.2f %.2f %.2f 1.50 1.60 3.90 %.2f 1.60 %.2f %.2f'
                        % (rng.uniform(-3, 3), x1, y1, x1 + bw, y1 + bh, x, z, rng.uniform(-3, 3)))
            r0, r1, c0, c1 = int(y1), int(y1 + bh), int(x1), int(x1 + bw)
            inst[r0:r1, c0:c1] = k
            depth[r0:r1, c0:c1] = z + rng.uniform(-1, 1, (r1 - r0, c1 - c0))
        with open(os.path.join(split, 'label_2', name + '.txt'), 'w') as f:
            f.write('\n'.join(rows) + '\n')
        with open(os.path.join(split, 'calib', name + '.txt'), 'w') as f:
            f.write(calib)
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(
            os.path.join(split, 'image_2', name + '.png'), compress_level=1)
        Image.fromarray((depth * 256).astype(np.uint16)).save(os.path.join(split, dirs[3], name + '.png'),
                                                                compress_level=1)
        Image.fromarray(inst).save(os.path.join(split, dirs[4], name + '.png'), compress_level=1)
    with open(os.path.join(top, 'train.txt'), 'w') as f:
        f.write(''.join(n + '\n' for n in names))
    return names


def config(top, jitter='oversample', image_aug=None):
    return ConfigObj(dict(dataset_dir=top, data_split='train', data_split_dir='training', num_boxes=32, classes=['Car'],
                          oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0, use_mscnn_detections=True,
                          obj_filter_config=dict(kitti_dataset.DEFAULT_OBJ_FILTER),
                          aug_config=dict(use_image_aug=image_aug is not None, image_noise=image_aug,
                                          box_jitter_type=jitter), depth_version='multiscale',
                          instance_version='depth_2_multiscale'))


def window(fn, per_call, seconds, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return calls * per_call / dt, 1e3 * dt / (calls * per_call)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--frames', type=int, default=256)
    p.add_argument('--seconds', type=float, default=1.0, help='length of a timing window (default 1 s)')
    p.add_argument('--kernels-only', action='store_true', help='50 batches of 8 and nothing else (for rocprofv3)')
    p.add_argument('--image-aug', choices=('reference', 'composed'), default=None,
                   help="aug_config.use_image_aug with this image_noise (default: off)")
    a = p.parse_args(argv)
    if a.frames < 8:
        p.error('--frames must be >= 8')
    with tempfile.TemporaryDirectory() as top:
        t0 = time.perf_counter()
        names = make_split(top, 32 if a.kernels_only else a.frames)
        print('synthetic split: %d frames of %d x %d written in %.1f s' % (len(names), H, W, time.perf_counter() - t0))
        t0 = time.perf_counter()
        ds = kitti_dataset.KittiDataset(config(top, image_aug=a.image_aug), 'train', seed=0)
        torch.cuda.synchronize()
        print('KittiDataset: loaded in %.2f s, %d samples, %d skipped, resident_bytes %d (%.1f MB per frame)'
              % (time.perf_counter() - t0, ds.num_samples, ds.num_skipped, ds.resident_bytes,
                 ds.resident_bytes / ds.num_samples / 1e6))
        if a.kernels_only:
            for _ in range(50):
                ds.next_batch(8, True)
            torch.cuda.synchronize()
            ds.check_status()
            return 0
        split = os.path.join(top, 'training')
        depth_dir, inst_dir = ds.depth_dir, ds.instance_dir
        rng, k = np.random.default_rng(0), [0]

        def host():
            kitti_dataset.build_training_sample(split, names[k[0] % len(names)], depth_dir, inst_dir, rng)
            k[0] += 1
        rate, ms = window(host, 1, a.seconds)
        print('(a) build_training_sample, PNG reads included: %8.1f samples/s  %7.3f ms per sample' % (rate, ms))
        for bs in (1, 8):
            rate, ms = window(lambda: ds.next_batch(bs, True), bs, a.seconds)
            print("(b) KittiDataset.next_batch(%d), 'oversample'%s:    %8.1f samples/s  %7.3f ms per sample"
                  % (bs, ', image noise %r' % a.image_aug if a.image_aug else '', rate, ms))
        trials = torch.cat([s['jitter_trials'] for s in ds.next_batch(8, True)])
        print('jitter trials per jittered box in one batch: mean %.2f, max %d'
              % (float(trials[trials > 0].float().mean()), int(trials.max())))
        ds.check_status()
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""Times the LiDAR depth-map chain (csrc/depth_fill.hip) on batches of fixture-like synthetic frames.

    python tools/depth_fill_bench.py [--frames 64] [--batch 8] [--blur bilateral] [--cpu-frames 2] [--out DIR]

Synthetic frames: 375 x 1242 maps with ~36k valid pixels below the top fifth (the density of the KITTI fixture frames)
and ~120k-point clouds.  Reports, as one JSON line:
  * fill_ms_per_frame / project_ms_per_frame: device time of the launch chain per frame (events around repeated
    batches, after a warm-up);
  * e2e_frames_per_s: projection + completion + copy to the host + the uint16 PNG write (PIL), per frame, at --batch;
  * restatement_ms_per_frame: tests/ip_basic_restatement.py on the CPU -- a numpy restatement, NOT cv2.
Kernel times per launch come from a separate `rocprofv3 --kernel-trace --stats -- python tools/depth_fill_bench.py`
run."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
VELO_TO_CAM0 = np.array([[0.0, -1, 0, 0], [0, 0, -1, -0.08], [1, 0, 0, -0.27]])


def synthetic_cloud(seed, n=120000):
    rng = np.random.default_rng(seed)
    r = rng.uniform(2, 80, n)
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.43, 0.03, n)
    pts = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el) + 1.7,
                    rng.random(n)], 1)
    return pts.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--blur', default='bilateral')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-frames', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from monopsr_amd.datasets.kitti import depth_map_utils as dmu
    from monopsr_amd.ip_basic import ip_basic
    import ip_basic_restatement as rs
    h, w = 375, 1242
    clouds = [synthetic_cloud(s) for s in range(a.batch)]
    maps = dmu.project_depths_rows(clouds, [VELO_TO_CAM0] * a.batch, [P2] * a.batch, (h, w))
    ip_basic.fill_in_multiscale_batch(maps, blur_type=a.blur)
    torch.cuda.synchronize()

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (a.reps * a.batch)

    fill_ms = timed(lambda: ip_basic.fill_in_multiscale_batch(maps, blur_type=a.blur))
    proj_ms = timed(lambda: dmu.project_depths_rows(clouds, [VELO_TO_CAM0] * a.batch, [P2] * a.batch, (h, w)))
    valid = float((maps > 0).sum().item()) / a.batch
    out_dir = a.out or tempfile.mkdtemp(prefix='depth_bench_')
    os.makedirs(out_dir, exist_ok=True)
    n_done, t0 = 0, time.perf_counter()
    while n_done < a.frames:
        dense, _ = ip_basic.fill_in_multiscale_batch(
            dmu.project_depths_rows(clouds, [VELO_TO_CAM0] * a.batch, [P2] * a.batch, (h, w)), blur_type=a.blur)
        for k, d in enumerate(dense.cpu().numpy()):
            dmu.save_depth_map(os.path.join(out_dir, '%06d.png' % ((n_done + k) % a.batch)), d)
        n_done += a.batch
    e2e = n_done / (time.perf_counter() - t0)
    host_maps = maps.cpu().numpy()
    cpu_ms = None
    if a.cpu_frames > 0:
        t0 = time.perf_counter()
        for k in range(a.cpu_frames):
            rs.fill_in_multiscale(host_maps[k % a.batch], blur_type=a.blur)
        cpu_ms = (time.perf_counter() - t0) * 1000 / a.cpu_frames
    print(json.dumps({'image': [h, w], 'batch': a.batch, 'blur': a.blur, 'valid_pixels_per_frame': valid,
                      'fill_ms_per_frame': round(fill_ms, 4), 'project_ms_per_frame': round(proj_ms, 4),
                      'e2e_frames_per_s': round(e2e, 2), 'e2e_frames': n_done,
                      'restatement_ms_per_frame': None if cpu_ms is None else round(cpu_ms, 1),
                      'restatement_note': 'numpy restatement on the host CPU, not cv2'}))


if __name__ == '__main__':
    main()

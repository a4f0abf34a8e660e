"""Host time of render_instance_surfaces next to project_instance_points on the chunk of DESIGN.md section 7.7: 8 frames
of 375 x 1242 with 32 boxes of 48 x 48 points and 70 % of the masks set.  A host clock around --calls calls after
--warmup calls, --windows times; each call of project_instance_points ends in its copy of the frame offsets to the
host, render_instance_surfaces copies nothing, so its windows end in a synchronize.

Each box is a 48 x 48 grid back-projected into a rectangle of its frame (40 to 300 pixels wide, 30 to 150 high) on a
gently sloped surface (at most 0.5 m across the box, 2 cm of noise), so that the default max_edge_dz of 1 m drops a
triangle only where the mask has a hole.  Numbers: DESIGN.md section 7.9.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monopsr_amd.core import scene_reconstruction as sr  # noqa: E402

H, W = 375, 1242
P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
N_FRAMES, N_BOXES, ROI = 8, 32, 48


def make_chunk(seed=0):
    rng = np.random.default_rng(seed)
    box_frame = np.sort(np.arange(N_BOXES) % N_FRAMES).astype(np.int32)
    xyz = np.zeros((N_BOXES, ROI, ROI, 3), np.float32)
    i, j = np.meshgrid(np.linspace(-0.5, 0.5, ROI), np.linspace(-0.5, 0.5, ROI), indexing='ij')
    for b in range(N_BOXES):
        z = rng.uniform(6, 44)
        bw, bh = rng.uniform(40, 300), rng.uniform(30, 150)
        x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
        cols, rows = x1 + (j + 0.5) * bw, y1 + (i + 0.5) * bh
        zz = z + rng.uniform(-0.5, 0.5) * i + rng.uniform(-0.5, 0.5) * j + rng.uniform(-0.02, 0.02, (ROI, ROI))
        xyz[b] = np.stack([(cols - P2[0, 2]) * zz / P2[0, 0], (rows - P2[1, 2]) * zz / P2[1, 1], zz], -1)
    mask = (rng.random((N_BOXES, ROI, ROI)) < 0.7).astype(np.float32)
    return xyz, box_frame, mask


def windows(fn, calls, warmup, n):
    out = []
    for _ in range(n):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / calls)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--calls', type=int, default=500)
    p.add_argument('--warmup', type=int, default=30)
    p.add_argument('--windows', type=int, default=3)
    a = p.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    xyz, box_frame, mask = make_chunk()
    xyz_d, mask_d = torch.from_numpy(xyz).to(dev), torch.from_numpy(mask).to(dev)
    cam = torch.from_numpy(np.stack([P2] * N_FRAMES)).to(dev)
    shapes = [(H, W)] * N_FRAMES
    images = [torch.rand((H, W, 3), device=dev) for _ in range(N_FRAMES)]
    surfaces = lambda: sr.render_instance_surfaces(xyz_d, box_frame, cam, shapes, valid_mask=mask_d)
    points = lambda: sr.project_instance_points(xyz_d, box_frame, cam, shapes, images=images, valid_mask=mask_d)
    s, q = surfaces(), points()
    fmt = lambda ms: ', '.join('%.3f' % v for v in ms)
    print('%d frames of %d x %d, %d boxes of %d x %d points, %d of %d masks set'
          % (N_FRAMES, H, W, N_BOXES, ROI, ROI, int(mask.sum()), mask.size))
    print('surfaces: %d of %d triangles drawn, %d pixels won; points: %d kept, %d visible'
          % (int(s.tris_per_box.sum()), N_BOXES * 2 * (ROI - 1) ** 2, int(s.pixels_per_box.sum()),
             int(q.kept_per_box.sum()), int(q.visible_per_box.sum())))
    print('render_instance_surfaces  ms per call: %s' % fmt(windows(surfaces, a.calls, a.warmup, a.windows)))
    print('project_instance_points   ms per call: %s' % fmt(windows(points, a.calls, a.warmup, a.windows)))
    inf = lambda: sr.render_instance_surfaces(xyz_d, box_frame, cam, shapes, max_edge_dz=float('inf'))
    r = inf()
    print('no mask, max_edge_dz inf: %d triangles drawn, %d pixels won, ms per call: %s'
          % (int(r.tris_per_box.sum()), int(r.pixels_per_box.sum()), fmt(windows(inf, a.calls, a.warmup, a.windows))))
    return 0


if __name__ == '__main__':
    sys.exit(main())

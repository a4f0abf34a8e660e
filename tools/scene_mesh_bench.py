"""Host time of extract_instance_meshes next to render_instance_surfaces on the chunk of tools/scene_surface_bench.py: 8
frames of 375 x 1242 with 32 boxes of 48 x 48 points, once with 70 % of the masks set and once without a mask (and
max_edge_dz = inf), visible_only off and on.  A host clock around --calls calls after --warmup calls, --windows times;
each call of extract_instance_meshes ends in its copy of the frame offsets to the host, render_instance_surfaces copies
nothing, so its windows end in a synchronize.  Both versions alternate window by window in one process.

Also printed: the triangles and vertices kept, and the bytes that cross to the host when every frame's mesh is fetched
(what save_mesh_frame copies: xyz, rgb, normal 12 bytes each and box 4 per vertex, 12 per face) next to the bytes of
all 73,728 points and 141,376 triangles.  Numbers: DESIGN.md section 7.13.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scene_surface_bench as chunk  # noqa: E402
from monopsr_amd.core import scene_reconstruction as sr  # noqa: E402

VERTEX_BYTES, FACE_BYTES = 3 * 12 + 4, 12


def window(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--calls', type=int, default=500)
    p.add_argument('--warmup', type=int, default=30)
    p.add_argument('--windows', type=int, default=3)
    a = p.parse_args(argv)
    dev = torch.device('cuda', torch.cuda.current_device())
    xyz, box_frame, mask = chunk.make_chunk()
    xyz_d, mask_d = torch.from_numpy(xyz).to(dev), torch.from_numpy(mask).to(dev)
    cam = torch.from_numpy(np.stack([chunk.P2] * chunk.N_FRAMES)).to(dev)
    shapes = [(chunk.H, chunk.W)] * chunk.N_FRAMES
    images = [torch.rand((chunk.H, chunk.W, 3), device=dev) for _ in range(chunk.N_FRAMES)]
    n_points = chunk.N_BOXES * chunk.ROI * chunk.ROI
    n_tris = chunk.N_BOXES * 2 * (chunk.ROI - 1) ** 2
    print('%d frames of %d x %d, %d boxes of %d x %d points, %d of %d masks set; all points and triangles: %d bytes'
          % (chunk.N_FRAMES, chunk.H, chunk.W, chunk.N_BOXES, chunk.ROI, chunk.ROI, int(mask.sum()), mask.size,
             n_points * VERTEX_BYTES + n_tris * FACE_BYTES))
    fmt = lambda ms: ', '.join('%.3f' % v for v in ms)
    for what, options in (('masked', dict(valid_mask=mask_d)), ('no mask, max_edge_dz inf', dict(max_edge_dz=float('inf')))):
        fns = [('render_instance_surfaces', lambda: sr.render_instance_surfaces(xyz_d, box_frame, cam, shapes, **options))]
        for visible_only in (False, True):
            fns.append(('extract_instance_meshes visible_only=%s' % visible_only,
                        lambda v=visible_only: sr.extract_instance_meshes(xyz_d, box_frame, cam, shapes, images=images,
                                                                          visible_only=v, **options)))
        times = {name: [] for name, _ in fns}
        for _ in range(a.windows):  # the versions alternate
            for name, fn in fns:
                times[name].append(window(fn, a.calls, a.warmup))
        print('%s:' % what)
        for name, fn in fns:
            line = '  %-44s ms per call: %s' % (name, fmt(times[name]))
            if name.startswith('extract'):
                m = fn()
                nv, nt = len(m.xyz), len(m.faces)
                line += '; %d of %d triangles, %d of %d vertices, %d bytes to the host' % (
                    nt, n_tris, nv, n_points, nv * VERTEX_BYTES + nt * FACE_BYTES)
            print(line)
    return 0


if __name__ == '__main__':
    sys.exit(main())

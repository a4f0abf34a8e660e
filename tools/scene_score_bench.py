"""Device time of mpsr_scene_score next to the project + resolve + compact of the same call, with HIP events, on
synthetic chunks of 375 x 1242 frames with 32 boxes of 2304 points (48 x 48) in all: 8 frames, and 1 frame.

Each box is a 48 x 48 grid of points back-projected into a rectangle of its frame at the depth of the ground-truth
instance under it, so that the score kernel meets its instance, and the ground-truth instance image holds those
rectangles over a background of 255.  Each window runs for at least --seconds after a warm-up; the time of a call is
the events' span over the number of calls queued between them.  Numbers: DESIGN.md section 7.8.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monopsr_amd import _lib  # noqa: E402

H, W = 375, 1242
P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
N_BOXES, ROI = 32, 48


def make_chunk(n_frames, seed=0):
    rng = np.random.default_rng(seed)
    box_frame = np.sort(np.arange(N_BOXES) % n_frames).astype(np.int32)
    inst = np.full((n_frames, H, W), 255, np.uint8)
    depth = rng.uniform(3, 60, (n_frames, H, W)).astype(np.float32)
    depth[rng.random((n_frames, H, W)) < 0.3] = 0.0
    xyz = np.zeros((N_BOXES, ROI * ROI, 3), np.float32)
    gt_id = np.zeros(N_BOXES, np.int32)
    for b in range(N_BOXES):
        f = int(box_frame[b])
        k = b - int(np.searchsorted(box_frame, f))
        z = rng.uniform(6, 44)
        bw, bh = rng.uniform(40, 300), rng.uniform(30, 150)
        x1, y1 = rng.uniform(0, W - 1 - bw), rng.uniform(0, H - 1 - bh)
        inst[f, int(y1):int(y1 + bh), int(x1):int(x1 + bw)] = k
        gt_id[b] = k
        cols, rows = np.meshgrid(np.linspace(x1, x1 + bw, ROI), np.linspace(y1, y1 + bh, ROI))
        zz = z + rng.uniform(-1, 1, (ROI, ROI))
        xyz[b] = np.stack([(cols - P2[0, 2]) * zz / P2[0, 0], (rows - P2[1, 2]) * zz / P2[1, 1], zz], -1).reshape(-1, 3)
    return xyz, box_frame, gt_id, inst, depth


def window(fn, seconds, warmup=20, batch=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    calls, total_ms = 0, 0.0
    while total_ms < 1e3 * seconds:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(batch):
            fn()
        end.record()
        end.synchronize()
        total_ms += start.elapsed_time(end)
        calls += batch
    return 1e3 * total_ms / calls  # microseconds per call


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--seconds', type=float, default=1.0, help='length of a timing window (default 1 s)')
    a = p.parse_args(argv)
    lib = _lib.lib()
    dev = torch.device('cuda', torch.cuda.current_device())
    host = lambda arr: arr.ctypes.data_as(ctypes.c_void_p)
    for n_frames in (8, 1):
        xyz, bf, gt_id, inst, depth = make_chunk(n_frames)
        npts = ROI * ROI
        hw = np.ascontiguousarray(np.asarray([[H, W]] * n_frames, np.int32))
        offs = np.ascontiguousarray(np.arange(n_frames + 1, dtype=np.int64) * H * W)
        total = int(offs[-1])
        t = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        xyz_d, bf_d, gt_d, inst_d, depth_d, hw_d, offs_d = (t(v) for v in (xyz, bf, gt_id, inst, depth, hw, offs))
        cam = t(np.stack([P2] * n_frames))
        images = torch.rand((n_frames, H, W, 3), device=dev)
        table = lambda stack: t(np.asarray([_lib.ptr(stack[f]) for f in range(n_frames)], np.uint64).view(np.int64))
        image_table, depth_table, inst_table = table(images), table(depth_d), table(inst_d)
        ws = torch.empty(lib.mpsr_scene_workspace_bytes(n_frames, total, N_BOXES, npts), dtype=torch.uint8, device=dev)
        scratch = torch.empty(lib.mpsr_scene_score_scratch_bytes(n_frames), dtype=torch.uint8, device=dev)
        out_depth, out_inst = torch.empty(total, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
        cap = N_BOXES * npts
        o_xyz, o_rgb = torch.empty((cap, 3), device=dev), torch.empty((cap, 3), device=dev)
        o_box, o_pix = (torch.empty(cap, dtype=torch.int32, device=dev) for _ in range(2))
        kept, visible = (torch.empty(N_BOXES, dtype=torch.int32, device=dev) for _ in range(2))
        frame_offset = torch.empty(n_frames + 1, dtype=torch.int64, device=dev)
        counts = torch.empty((N_BOXES, 6), dtype=torch.int32, device=dev)
        sums = torch.empty((N_BOXES, 3), dtype=torch.float64, device=dev)
        ptr, stream = _lib.ptr, _lib.stream()

        def render():
            _lib.check(lib.mpsr_scene_project(ptr(xyz_d), None, ptr(bf_d), host(bf), None, ptr(cam), ptr(hw_d), host(hw),
                                              ptr(offs_d), host(offs), n_frames, N_BOXES, npts, ptr(ws), ws.numel(),
                                              stream))
            _lib.check(lib.mpsr_scene_resolve(ptr(bf_d), host(bf), n_frames, total, N_BOXES, npts, ptr(ws), ws.numel(),
                                              ptr(out_depth), ptr(out_inst), stream))
            _lib.check(lib.mpsr_scene_compact(ptr(xyz_d), ptr(bf_d), ptr(image_table), ptr(offs_d), n_frames, total,
                                              N_BOXES, npts, 0, ptr(ws), ws.numel(), ptr(o_xyz), ptr(o_rgb), ptr(o_box),
                                              ptr(o_pix), ptr(frame_offset), ptr(kept), ptr(visible), stream))

        def score():
            _lib.check(lib.mpsr_scene_score(ptr(xyz_d), ptr(bf_d), host(bf), ptr(gt_d), ptr(depth_table),
                                            ptr(inst_table), ptr(offs_d), n_frames, total, N_BOXES, npts, ptr(ws),
                                            ws.numel(), ptr(scratch), scratch.numel(), ptr(counts), ptr(sums), stream))
        render_us = window(render, a.seconds)
        render()
        score_us = window(score, a.seconds)
        c = counts.cpu().numpy()
        assert np.array_equal(c[:, 0], kept.cpu().numpy()) and np.array_equal(c[:, 2], visible.cpu().numpy())
        print('%d frame%s of %d x %d, %d boxes of %d points: project + resolve + compact %8.1f us, score %8.1f us  '
              '(kept %d, pred_px %d, inter_px %d, gt_px %d, depth_n %d)'
              % (n_frames, '' if n_frames == 1 else 's', H, W, N_BOXES, npts, render_us, score_us, c[:, 0].sum(),
                 c[:, 2].sum(), c[:, 3].sum(), c[:, 4].sum(), c[:, 5].sum()))
    return 0


if __name__ == '__main__':
    sys.exit(main())

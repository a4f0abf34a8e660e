"""Generates the LiDAR depth-map fixtures: tests/golden/depth_fixture.npz, depth_windows.npz, depth_velo_*.npy and
depth_<frame>.png.

Run in the build container only (reads the reference's mini KITTI tree and imports its code; the GPU box has neither):

    python tests/golden/make_depth_fixture.py

It imports the reference's UNMODIFIED ip_basic.fill_in_multiscale, depth_map_utils.project_depths and
calib_utils.read_frame_calib / lidar_to_cam_frame, with tests/cv2_standin.py installed as `cv2` and empty modules as
`tensorflow` and `png` (those functions never call them).  project_depths indexes with a list of two arrays, which
numpy >= 1.23 reads as one array index; its module's `np` is wrapped so that np.zeros returns an array that reads such a
list as the tuple the code was written for (the legacy meaning).  The cloud of a frame is built as get_lidar_point_cloud
builds it (velodyne .bin -> lidar_to_cam_frame, transposed).

Before writing anything it ASSERTS that tests/ip_basic_restatement.py equals the reference, map for map and stage for
stage, bit for bit, on every frame and both blur types.  Then it writes data only:
  * the raw velodyne xyz of frame 000000 (in two halves, to keep every file under 1 MiB);
  * for frames 000001, 000002 and 000006 only the points that land in the image, in their original order (the same map);
  * calibrations (P2, R0_rect, Tr_velo_to_cam) and image shapes;
  * the reference's projected maps, sparse (flat pixel index, value);
  * SHA-256 of the float32 bytes of every full-frame stage s1 .. s8 for both blur types;
  * the final maps of the bilateral fill as the uint16 PNGs save_depth_map writes;
  * windows cut from the sparse maps (top rows, image borders), each run through the reference with show_process=True,
    every stage kept as float32, for both blur types and with extrapolate on and off.
"""
import hashlib
import os
import sys
import types

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cv2_standin  # noqa: E402
import ip_basic_restatement as rs  # noqa: E402

sys.modules['cv2'] = cv2_standin
sys.modules['tensorflow'] = types.ModuleType('tensorflow')
sys.modules['png'] = types.ModuleType('png')
if not hasattr(np, 'bool'):
    np.bool = bool
sys.path.insert(0, '/root/reference/src')
from ip_basic import ip_basic  # noqa: E402
from monopsr.datasets.kitti import calib_utils, depth_map_utils  # noqa: E402

KITTI = '/root/reference/src/monopsr/tests/datasets/Kitti/object/training'
RAW_FRAME = '000000'
FRAMES = ('000000', '000001', '000002', '000006')
# (frame, row0, col0, height, width): the top rows, the left / right / bottom borders and an interior patch
WINDOWS = (('000001', 0, 0, 48, 64), ('000001', 150, 1178, 64, 64), ('000006', 310, 400, 64, 80),
           ('000000', 120, 600, 56, 72))


class _LegacyIndex(np.ndarray):
    def __getitem__(self, key):
        return super().__getitem__(tuple(key) if isinstance(key, list) else key)

    def __setitem__(self, key, value):
        super().__setitem__(tuple(key) if isinstance(key, list) else key, value)


class _NumpyLegacyIndex(types.ModuleType):
    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def zeros(*a, **k):
        return np.zeros(*a, **k).view(_LegacyIndex)


depth_map_utils.np = _NumpyLegacyIndex('numpy')


def ref_project(velo_xyz, calib, shape):
    cloud = calib_utils.lidar_to_cam_frame(velo_xyz, calib).T  # get_lidar_point_cloud
    return np.asarray(depth_map_utils.project_depths(cloud, calib.p2, shape))


def ref_fill(depths, **kw):
    out, proc = ip_basic.fill_in_multiscale(depths, show_process=True, **kw)
    return out, [np.asarray(proc[k], np.float32) for k in rs.STAGES]


def check_fill(depths, **kw):
    out, stages = ref_fill(depths, **kw)
    r_out, r_st = rs.fill_in_multiscale(depths, **kw)
    for k, a, b in zip(rs.STAGES, stages, [r_st[k] for k in rs.STAGES]):
        assert a.dtype == b.dtype == np.float32 and a.tobytes() == b.tobytes(), (k, kw, int((a != b).sum()))
    assert out.tobytes() == r_out.tobytes()
    return stages


def main():
    data, windows = {}, {}
    for f in FRAMES:
        calib = calib_utils.read_frame_calib(os.path.join(KITTI, 'calib', f + '.txt'))
        w, h = Image.open(os.path.join(KITTI, 'image_2', f + '.png')).size
        velo = np.fromfile(os.path.join(KITTI, 'velodyne', f + '.bin'), np.single).reshape(-1, 4)[:, :3]
        ref = ref_project(velo, calib, (h, w))
        rows = rs.velo_to_cam0(calib.r0_rect, calib.velo_to_cam)
        mine = rs.project_depths(velo, rows, calib.p2, (h, w))
        assert ref.dtype == np.float32 and ref.tobytes() == mine.tobytes(), f
        _, col, row = rs.project_points(velo, rows, calib.p2)
        with np.errstate(invalid='ignore'):
            inside = np.isfinite(col) & np.isfinite(row) & (col >= 0) & (col < w) & (row >= 0) & (row < h)
        kept = velo[inside]
        assert ref_project(kept, calib, (h, w)).tobytes() == ref.tobytes(), f
        if f == RAW_FRAME:
            half = len(velo) // 2
            np.save(os.path.join(HERE, 'depth_velo_%s_a.npy' % f), np.ascontiguousarray(velo[:half]))
            np.save(os.path.join(HERE, 'depth_velo_%s_b.npy' % f), np.ascontiguousarray(velo[half:]))
        else:
            np.save(os.path.join(HERE, 'depth_velo_%s.npy' % f), np.ascontiguousarray(kept))
        data['p2_%s' % f] = calib.p2
        data['r0_rect_%s' % f] = calib.r0_rect
        data['velo_to_cam_%s' % f] = calib.velo_to_cam
        data['shape_%s' % f] = np.array([h, w], np.int32)
        nz = np.flatnonzero(ref)
        data['proj_idx_%s' % f] = nz.astype(np.int32)
        data['proj_val_%s' % f] = ref.reshape(-1)[nz]
        for blur in ('bilateral', 'gaussian'):
            stages = check_fill(ref, blur_type=blur)
            data['sha_%s_%s' % (blur, f)] = np.array([hashlib.sha256(s.tobytes()).hexdigest() for s in stages])
            if blur == 'bilateral':
                png = (stages[-1] * 256.0).astype(np.uint16)
                Image.fromarray(png).save(os.path.join(HERE, 'depth_%s.png' % f))
        print('frame', f, (h, w), 'points', len(velo), 'in image', len(kept), 'valid pixels', len(nz))
    for n, (f, r0, c0, hh, ww) in enumerate(WINDOWS):
        h, w = data['shape_%s' % f]
        full = np.zeros(h * w, np.float32)
        full[data['proj_idx_%s' % f]] = data['proj_val_%s' % f]
        win = np.ascontiguousarray(full.reshape(h, w)[r0:r0 + hh, c0:c0 + ww])
        windows['in_%d' % n] = win
        for blur in ('bilateral', 'gaussian'):
            for ex in (False, True):
                windows['st_%d_%s_%d' % (n, blur, ex)] = np.stack(check_fill(win, blur_type=blur, extrapolate=ex))
    data['frames'] = np.array(FRAMES)
    data['windows'] = np.array(WINDOWS, dtype=object).astype(str)
    np.savez_compressed(os.path.join(HERE, 'depth_fixture.npz'), **data)
    np.savez_compressed(os.path.join(HERE, 'depth_windows.npz'), **windows)
    print('restatement == reference on %d frames and %d windows; fixtures written' % (len(FRAMES), len(WINDOWS)))


if __name__ == '__main__':
    main()

"""LiDAR depth maps of KITTI frames (monopsr/datasets/kitti/depth_map_utils.py and
demos/depth_completion/save_lidar_depth_maps.py of the reference), with the projection and the completion on the GPU.

    calib = read_calibration(calib_path)                              # P2, R0_rect, Tr_velo_to_cam
    maps = project_depths_batch([velo_points, ...], [calib, ...], (h, w))   # (F, h, w) CUDA tensor
    dense, _ = ip_basic.fill_in_multiscale_batch(maps)
    save_depth_map(path, dense[0].cpu().numpy())

Command line (what save_lidar_depth_maps.py does for a KITTI split directory with velodyne/, calib/ and image_2/):

    python -m monopsr_amd.datasets.kitti.depth_map_utils KITTI_SPLIT_DIR OUT_DIR [--frames 000001 ...] [--batch 8]
        [--blur bilateral|gaussian]

writes OUT_DIR/<name>.png, the uint16 map save_depth_map writes.  Frames are grouped by image size (read from the
image_2 PNG header) into batches of at most --batch, one launch chain per batch.

The projection reproduces the reference's project_depths of the cloud get_lidar_point_cloud builds: fp64 throughout,
no z > 0 filter, the last point of a pixel wins (include/monopsr_hip.h, mpsr_lidar_project_depths).  PNGs are read and
written with PIL on the host.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from monopsr_amd import _lib


class FrameCalib(object):
    """The calibration entries the depth maps need: p2 (3, 4), r0_rect (3, 3), velo_to_cam (3, 4), all float64."""
    __slots__ = ('p2', 'r0_rect', 'velo_to_cam')

    def __init__(self, p2, r0_rect, velo_to_cam):
        self.p2 = np.asarray(p2, np.float64).reshape(3, 4)
        self.r0_rect = np.asarray(r0_rect, np.float64).reshape(3, 3)
        self.velo_to_cam = np.asarray(velo_to_cam, np.float64).reshape(3, 4)


_CALIB_KEYS = {'P2': 12, 'R0_rect': 9, 'Tr_velo_to_cam': 12}


def parse_calibration(text):
    """KITTI object calibration text ("KEY: v v v ...") -> FrameCalib.  Values parse as Python floats, as the
    reference's read_frame_calib parses them; a missing entry or a wrong value count raises ValueError."""
    found = {}
    for line in text.splitlines():
        if ':' not in line:
            continue
        key, vals = line.split(':', 1)
        key = key.strip()
        if key in _CALIB_KEYS:
            v = [float(x) for x in vals.split()]
            if len(v) != _CALIB_KEYS[key]:
                raise ValueError('calibration %s has %d values, expected %d' % (key, len(v), _CALIB_KEYS[key]))
            found[key] = v
    missing = [k for k in _CALIB_KEYS if k not in found]
    if missing:
        raise ValueError('calibration lacks %s' % ', '.join(missing))
    return FrameCalib(found['P2'], found['R0_rect'], found['Tr_velo_to_cam'])


def read_calibration(path):
    with open(path) as f:
        return parse_calibration(f.read())


def velo_to_cam0(calib):
    """Rows 0..2 of R0_rect . Tr_velo_to_cam, padded to 4 x 4 and multiplied as calib_utils.lidar_to_cam_frame does."""
    r0 = np.pad(calib.r0_rect, ((0, 1), (0, 1)), 'constant', constant_values=0)
    r0[3, 3] = 1
    tr = np.pad(calib.velo_to_cam, ((0, 1), (0, 0)), 'constant', constant_values=0)
    tr[3, 3] = 1
    return np.dot(r0, tr)[:3]


def read_velodyne(path):
    """(N, 4) float32 x y z intensity (obj_utils.read_lidar)."""
    return np.fromfile(path, np.float32).reshape(-1, 4)


def _points4(p):
    """(N, 3 or 4) -> contiguous (N, 4) float32 (the intensity column is not used)."""
    p = np.asarray(p, np.float32)
    if p.ndim != 2 or p.shape[1] not in (3, 4):
        raise _lib.InvalidArgumentError('points must be (N, 3) or (N, 4), got %s' % (p.shape,))
    if p.shape[1] == 3:
        p = np.concatenate([p, np.zeros((len(p), 1), np.float32)], axis=1)
    return np.ascontiguousarray(p)


def project_depths_rows(points, transforms, cam_ps, image_shape, max_depth=100.0, device=None):
    """The batched projection: points, a list of F clouds (N_f, 3 or 4) float32; transforms, F (3, 4) fp64 point ->
    cam0 matrices; cam_ps, F (3, 4) P2 matrices -> (F, h, w) float32 CUDA tensor."""
    import torch
    nf = len(points)
    if not (len(transforms) == len(cam_ps) == nf):
        raise _lib.InvalidArgumentError('project_depths: %d clouds, %d transforms, %d cameras'
                                        % (nf, len(transforms), len(cam_ps)))
    h, w = int(image_shape[0]), int(image_shape[1])
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    clouds = [_points4(p) for p in points]
    offs = np.zeros(nf + 1, np.int64)
    offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.concatenate(clouds + [np.zeros((0, 4), np.float32)])
    tf = np.ascontiguousarray(np.stack([np.asarray(t, np.float64).reshape(3, 4) for t in transforms] or
                                       [np.zeros((3, 4))]))
    cp = np.ascontiguousarray(np.stack([np.asarray(c, np.float64).reshape(3, 4) for c in cam_ps] or
                                       [np.zeros((3, 4))]))
    lib = _lib.lib()
    with torch.cuda.device(dev):
        pts_d = torch.from_numpy(pts).to(dev)
        offs_d = torch.from_numpy(offs).to(dev)
        tf_d, cp_d = torch.from_numpy(tf).to(dev), torch.from_numpy(cp).to(dev)
        out = torch.empty((nf, h, w), dtype=torch.float32, device=dev)
        ws = torch.empty(max(1, lib.mpsr_lidar_project_workspace_bytes(nf, h, w)), dtype=torch.uint8, device=dev)
        _lib.check(lib.mpsr_lidar_project_depths(_lib.ptr(pts_d) if len(pts) else None, _lib.ptr(offs_d),
                                                 offs.ctypes.data_as(ctypes.c_void_p), nf, _lib.ptr(tf_d),
                                                 _lib.ptr(cp_d), h, w, float(max_depth), _lib.ptr(out), _lib.ptr(ws),
                                                 ws.numel(), _lib.stream()))
    return out


def project_depths_batch(velo_points, calibs, image_shape, max_depth=100.0, device=None):
    """Depth maps of F frames of one image size from their raw velodyne points (N_f, 4) and FrameCalibs: the map
    save_lidar_depth_maps.py projects (project_depths of get_lidar_point_cloud's cloud) -> (F, h, w) CUDA tensor."""
    return project_depths_rows(velo_points, [velo_to_cam0(c) for c in calibs], [c.p2 for c in calibs], image_shape,
                               max_depth, device)


def project_depths(point_cloud, cam_p, image_shape, max_depth=100.0):
    """The reference's signature: point_cloud (3, N) in cam0, cam_p (3, 4) -> (h, w) float32 numpy map.

    The kernels read float32 points: a float64 cloud is rounded to float32 first (the reference projects it in
    float64).  project_depths_batch from the raw velodyne points equals the reference's pipeline bit for bit."""
    pc = np.asarray(point_cloud)
    if pc.ndim != 2 or pc.shape[0] != 3:
        raise _lib.InvalidArgumentError('project_depths: point_cloud must be (3, N), got %s' % (pc.shape,))
    eye = np.eye(4)[:3]
    return project_depths_rows([pc.T], [eye], [cam_p], image_shape, max_depth)[0].cpu().numpy()


def read_depth_map(depth_map_path):
    """uint16 PNG -> float32 metres: / 256, then values < 0.1 become 0 (the reference's read_depth_map)."""
    from PIL import Image
    depth_image = np.asarray(Image.open(depth_map_path))
    depth_map = depth_image / 256.0
    depth_map[depth_map < 0.1] = 0.0
    return depth_map.astype(np.float32)


def save_depth_map(save_path, depth_map):
    """(depth_map * 256).astype(np.uint16) as a 16-bit greyscale PNG (the reference's save_depth_map)."""
    from PIL import Image
    depth_image = (np.asarray(depth_map) * 256.0).astype(np.uint16)
    Image.fromarray(depth_image).save(save_path, format='PNG')


def image_shape(path):
    """(h, w) from an image header (PIL reads no pixels for it)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def _groups(names, shapes, batch):
    by_shape = {}
    for n in names:
        by_shape.setdefault(shapes[n], []).append(n)
    for shape in sorted(by_shape):
        group = by_shape[shape]
        for i in range(0, len(group), batch):
            yield shape, group[i:i + batch]


def save_lidar_depth_maps(split_dir, out_dir, frames=None, batch=8, blur_type='bilateral', max_depth=100.0,
                          log=None):
    """Projects and completes the depth map of every frame (or `frames`) of split_dir into out_dir/<name>.png.
    Returns the names written, in the order written."""
    from monopsr_amd.ip_basic import ip_basic
    if batch < 1:
        raise ValueError('batch must be >= 1, got %d' % batch)
    velo_dir = os.path.join(split_dir, 'velodyne')
    if frames is None:
        if not os.path.isdir(velo_dir):
            raise FileNotFoundError('no velodyne directory in %s' % split_dir)
        frames = sorted(f[:-4] for f in os.listdir(velo_dir) if f.endswith('.bin'))
    shapes = {n: image_shape(os.path.join(split_dir, 'image_2', n + '.png')) for n in frames}
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for shape, names in _groups(frames, shapes, batch):
        velo = [read_velodyne(os.path.join(velo_dir, n + '.bin')) for n in names]
        calibs = [read_calibration(os.path.join(split_dir, 'calib', n + '.txt')) for n in names]
        maps = project_depths_batch(velo, calibs, shape, max_depth)
        dense, _ = ip_basic.fill_in_multiscale_batch(maps, max_depth=max_depth, blur_type=blur_type)
        dense = dense.cpu().numpy()
        for n, d in zip(names, dense):
            save_depth_map(os.path.join(out_dir, n + '.png'), d)
            written.append(n)
        if log:
            log('%d / %d frames (%d x %d)' % (len(written), len(frames), shape[0], shape[1]))
    return written


def main(argv=None):
    p = argparse.ArgumentParser(prog='python -m monopsr_amd.datasets.kitti.depth_map_utils',
                                description='Dense LiDAR depth maps (projection + IP-Basic completion) on the GPU.')
    p.add_argument('split_dir', help='KITTI split directory with velodyne/, calib/ and image_2/')
    p.add_argument('out_dir', help='directory for <name>.png')
    p.add_argument('--frames', nargs='+', help='frame names (default: every velodyne/*.bin)')
    p.add_argument('--batch', type=int, default=8, help='frames per launch chain (default 8)')
    p.add_argument('--blur', choices=sorted(('bilateral', 'gaussian')), default='bilateral')
    p.add_argument('--max-depth', type=float, default=100.0)
    a = p.parse_args(argv)
    if a.batch < 1:
        p.error('--batch must be >= 1')
    if not os.path.isdir(a.split_dir):
        p.error('no such directory: %s' % a.split_dir)
    names = save_lidar_depth_maps(a.split_dir, a.out_dir, a.frames, a.batch, a.blur, a.max_depth,
                                  log=lambda m: print(m, file=sys.stderr))
    print('wrote %d depth maps to %s' % (len(names), a.out_dir))
    return 0


if __name__ == '__main__':
    sys.exit(main())

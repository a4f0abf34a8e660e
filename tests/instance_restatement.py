"""A restatement in numpy of the two ground-truth steps the instance kernels run (monopsr_amd/csrc/instance_maps.hip).

instance_images: demos/instances/gen_instance_masks.py:86-153 of the reference for depth-map clouds, written per pixel.
  * The cloud is depth_map_utils.get_depth_point_cloud's with numpy 1's meaning of `depth_map / cam_p[0, 0]` (a
    float32 array divided by a float64 scalar stays float32: the scalar is rounded to float32 first): ratio =
    d / float32(f) in float32; x = (u - cu) * ratio + x_offset, y = (v - cv) * ratio in fp64, z = d; then float32.
    Every pixel is a point, zero depths included ((x_offset, 0, 0)).
  * points_in_box_3d: the float32 point promoted to fp64, dot products (x * a0 + y * a1) + z * a2, inclusive slabs.
  * project_pc_to_image: ((p0 x + p1 y) + p2 z) + p3 in fp64, u' = r0 / r2, v' = r1 / r2; inclusive 2-D box test
    against the label's float32 edges.
  * A later box overwrites an earlier one; 255 is background.
The per-box constants (corners, u / v / w axes, the six bounds) come from monopsr_amd's host code, which orders the
operations as obj_utils.compute_box_3d_corners / points_in_box_3d do.

instance_xyz_crops: instance_utils.tf_instance_xyz_crop_from_depth_map (instance_utils.py:395-481) and
depth_map_utils.tf_depth_patch_to_pc_map (:161-236), all float32, as TF 1.8 computes them.
"""
import math

import numpy as np

from monopsr_amd.datasets.kitti import instance_utils as iu

F32 = np.float32


def depth_cloud(depth, p2):
    """(H, W) float32 depth, (3, 4) fp64 P2 -> (H, W, 3) float32 points of get_depth_point_cloud (numpy 1 meaning)."""
    h, w = depth.shape
    p2 = np.asarray(p2, np.float64)
    ratio = (depth.astype(F32) / F32(p2[0, 0])).astype(np.float64)
    uu = np.arange(w, dtype=np.float64)[None, :] - p2[0, 2]
    vv = np.arange(h, dtype=np.float64)[:, None] - p2[1, 2]
    x_offset = -p2[0, 3] / p2[0, 0]
    x = uu * ratio + x_offset
    y = vv * ratio
    z = depth.astype(np.float64)
    return np.stack([x, y, z], -1).astype(F32)


def instance_image(depth, p2, table):
    """One frame: depth (H, W) float32, P2 (3, 4) fp64, table (n, BOX_STRIDE) fp64 from iu.instance_box_table."""
    pts = depth_cloud(depth, p2).astype(np.float64)
    x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
    p2 = np.asarray(p2, np.float64)
    r = [((p2[k, 0] * x + p2[k, 1] * y) + p2[k, 2] * z) + p2[k, 3] for k in range(3)]
    with np.errstate(divide='ignore', invalid='ignore'):
        pu, pv = r[0] / r[2], r[1] / r[2]
    out = np.full(depth.shape, 255, np.uint8)
    for k, t in enumerate(table):
        inside = np.ones(depth.shape, bool)
        for a in range(3):
            ax = t[5 * a:5 * a + 3]
            dot = (x * ax[0] + y * ax[1]) + z * ax[2]
            inside &= (dot <= t[5 * a + 3]) & (dot >= t[5 * a + 4])
        y1, x1, y2, x2 = t[15:19]
        inside &= (pu >= x1) & (pu <= x2) & (pv >= y1) & (pv <= y2)
        out[inside] = k
    return out


def round_half_even(v):
    return np.rint(F32(v)).astype(np.int64)


def nn_index(i, n_in, n_out):
    """resize_nearest_neighbor(align_corners=True), TF 1.8: float32 scale, roundf (ties away from zero)."""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(n_in) / F32(n_out)
    s = float(F32(F32(i) * scale))  # >= 0
    r = math.floor(s)
    r += 1 if s - r >= 0.5 else 0  # roundf: ties away from zero
    return min(r, n_in - 1)


def linspace_tf(start, stop, num):
    start, stop = F32(start), F32(stop)
    if num == 1:
        return np.array([start], F32)
    step = F32((stop - start) / F32(num - 1))
    return np.array([F32(start + F32(step * F32(i))) for i in range(num)], F32)


def instance_xyz_crop(depth, inst, p2, inst_id, box_2d, box_3d, view_ang, roi, centroid_type='middle',
                      rotate_view=True):
    """One box -> (local (r, r, 3), global (r, r, 3), valid (r, r, 1)), all float32."""
    p2 = np.asarray(p2, F32).reshape(3, 4)
    y1, x1, y2, x2 = [F32(v) for v in box_2d]
    r0, c0, r2, c2 = [int(round_half_even(v)) for v in (y1, x1, y2, x2)]
    masked = depth.astype(F32) * (inst == inst_id).astype(F32)
    crop = masked[r0:r2, c0:c2]
    rows = [nn_index(i, crop.shape[0], roi) for i in range(roi)]
    cols = [nn_index(j, crop.shape[1], roi) for j in range(roi)]
    d = crop[np.ix_(rows, cols)]
    pw, ph = F32((x2 - x1) / F32(roi)), F32((y2 - y1) / F32(roi))
    hw, hh = F32(pw / F32(2.0)), F32(ph / F32(2.0))
    xx = linspace_tf(x1 + hw, x2 - hw, roi)[None, :]
    yy = linspace_tf(y1 + hh, y2 - hh, roi)[:, None]
    ratio = d / p2[0, 0]
    x, y, z = (xx - p2[0, 2]) * ratio, (yy - p2[1, 2]) * ratio, d
    valid = (np.abs(d) >= F32(0.1)).astype(F32)
    glob = np.stack([x * valid, y * valid, z * valid], -1)
    b3 = np.asarray(box_3d, F32)
    x_offset = -p2[0, 3] / p2[0, 0]
    cen = np.array([b3[0] - x_offset, b3[1], b3[2]], F32)
    if centroid_type == 'middle':
        cen[1] = cen[1] - b3[5] / F32(2.0)
    t = -cen
    if rotate_view:
        a = -np.float64(F32(view_ang))
        c, s = F32(np.cos(a)), F32(np.sin(a))  # fp64, rounded once (as the kernel)
        t0, t2 = c * t[0] + s * t[2], -s * t[0] + c * t[2]
        lx, ly, lz = (c * x + s * z) + t0, y + t[1], (-s * x + c * z) + t2
    else:
        lx, ly, lz = x + t[0], y + t[1], z + t[2]
    loc = np.stack([lx * valid, ly * valid, lz * valid], -1)
    return loc.astype(F32), glob.astype(F32), valid[..., None]


def instance_xyz_crops(depths, insts, p2s, frame_index, instance_id, boxes_2d, boxes_3d, view_angs, roi,
                       centroid_type='middle', rotate_view=True):
    outs = [instance_xyz_crop(depths[f], insts[f], p2s[f], i, b2, b3, va, roi, centroid_type, rotate_view)
            for f, i, b2, b3, va in zip(frame_index, instance_id, boxes_2d, boxes_3d, view_angs)]
    if not outs:
        z = np.zeros((0, roi, roi, 3), F32)
        return z, z.copy(), np.zeros((0, roi, roi, 1), F32)
    return tuple(np.stack(o) for o in zip(*outs))


def instance_images(depths, p2s, labels_per_frame):
    return np.stack([instance_image(d, p, iu.instance_box_table(lbl))
                     for d, p, lbl in zip(depths, p2s, labels_per_frame)])

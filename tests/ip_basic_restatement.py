"""An independent numpy restatement of the LiDAR depth-map pipeline of MonoPSR's depth completion demo, built on the cv2
stand-in (tests/cv2_standin.py): the projection of a velodyne cloud into image 2 and IP-Basic's multi-scale completion.

The kernels of csrc/depth_fill.hip must equal this bit for bit; tests/golden/make_depth_fixture.py checks, in the build
container, that it equals the reference's own functions run on the stand-in.

project_depths: every point of the cloud, in fp64, through two 3x4 products (velodyne -> cam0 with R0_rect . Tr_velo_to_cam,
then cam0 -> pixel with P2), each row summed left to right without fused multiply-adds; the pixel is rint(u / w),
rint(v / w) (round half to even); a point whose pixel is not finite or lies outside the image is dropped.  There is no
z > 0 filter.  Where points share a pixel the LAST one in cloud order wins, and the stored value is
max_depth - max(0, max_depth - z) in fp64, rounded once to float32.

fill_in_multiscale: the stages s1 .. s8 of IP-Basic's multi-scale fill (every comparison against a float32 threshold,
since a float32 array compared with a Python float compares in float32).
"""
import numpy as np

import cv2_standin as cv2

FULL_KERNEL_5 = np.ones((5, 5), np.uint8)
FULL_KERNEL_9 = np.ones((9, 9), np.uint8)
CROSS_KERNEL_3 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
CROSS_KERNEL_5 = np.zeros((5, 5), np.uint8)
CROSS_KERNEL_5[2, :] = CROSS_KERNEL_5[:, 2] = 1
CROSS_KERNEL_7 = np.zeros((7, 7), np.uint8)
CROSS_KERNEL_7[3, :] = CROSS_KERNEL_7[:, 3] = 1

STAGES = ('s1_inverted_depths', 's2_dilated_depths', 's3_closed_depths', 's4_blurred_depths', 's5_combined_depths',
          's6_extended_depths', 's7_blurred_depths', 's8_inverted_depths')


def velo_to_cam0(r0_rect, velo_to_cam):
    """The 3x4 rows of R0_rect . Tr_velo_to_cam, composed in 4x4 as the reference's lidar_to_cam_frame composes them."""
    r0 = np.eye(4)
    r0[:3, :3] = np.asarray(r0_rect, np.float64).reshape(3, 3)
    tr = np.eye(4)
    tr[:3, :4] = np.asarray(velo_to_cam, np.float64).reshape(3, 4)
    return np.dot(r0, tr)[:3]


def _rows(m, x, y, z):
    """m (3, 4) applied to homogeneous points, each row summed left to right."""
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]


def project_points(velo_xyz, velo_to_cam0_rows, p2):
    """-> (cam0 z (N,) fp64, column (N,) fp64, row (N,) fp64): the pixel before the range test."""
    xyz = np.asarray(velo_xyz, np.float32)[:, :3].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):  # non-finite points are dropped later
        cx, cy, cz = _rows(np.asarray(velo_to_cam0_rows, np.float64), xyz[:, 0], xyz[:, 1], xyz[:, 2])
        u, v, w = _rows(np.asarray(p2, np.float64), cx, cy, cz)
        return cz, np.rint(u / w), np.rint(v / w)


def project_depths(velo_xyz, velo_to_cam0_rows, p2, image_shape, max_depth=100.0):
    """velodyne points (N, >= 3) float32 -> (H, W) float32 depth map."""
    h, w = int(image_shape[0]), int(image_shape[1])
    z, col, row = project_points(velo_xyz, velo_to_cam0_rows, p2)
    with np.errstate(invalid='ignore'):
        keep = np.isfinite(col) & np.isfinite(row) & (col >= 0) & (col < w) & (row >= 0) & (row < h)
    idx = np.nonzero(keep)[0]
    pix = row[idx].astype(np.int64) * w + col[idx].astype(np.int64)
    last = np.full(h * w, -1, np.int64)
    last[pix] = idx  # numpy keeps the last of duplicate indices; idx is increasing
    out = np.zeros(h * w, np.float32)
    hit = last >= 0
    inv = max_depth - z[last[hit]]
    out[hit] = (max_depth - np.where(inv > 0.0, inv, 0.0)).astype(np.float32)
    return out.reshape(h, w)


def _top_rows(img):
    """np.argmax(img > 0.1, axis=0): the first row above 0.1 of each column, 0 for a column without one."""
    return np.argmax(img > np.float32(0.1), axis=0)


def _below_top(shape, top):
    return np.arange(shape[0])[:, None] >= top[None, :]


def fill_in_multiscale(depth_map, max_depth=100.0, dilation_kernel_far=CROSS_KERNEL_3,
                       dilation_kernel_med=CROSS_KERNEL_5, dilation_kernel_near=CROSS_KERNEL_7, extrapolate=False,
                       blur_type='bilateral'):
    """-> (depths_out, {stage name: (H, W) float32})."""
    t01, t15, t30 = np.float32(0.1), np.float32(15.0), np.float32(30.0)
    md = np.float32(max_depth)
    d = np.asarray(depth_map, np.float32)
    near, med, far = (d > t01) & (d <= t15), (d > t15) & (d <= t30), d > t30
    s1 = np.where(d > t01, md - d, d)
    zero = np.float32(0)
    dil_far = cv2.dilate(np.where(far, s1, zero), dilation_kernel_far)
    dil_med = cv2.dilate(np.where(med, s1, zero), dilation_kernel_med)
    dil_near = cv2.dilate(np.where(near, s1, zero), dilation_kernel_near)
    s2 = s1.copy()
    for dil in (dil_far, dil_med, dil_near):
        sel = dil > t01
        s2[sel] = dil[sel]
    s3 = cv2.morphologyEx(s2, cv2.MORPH_CLOSE, FULL_KERNEL_5)
    s4 = np.where(s3 > t01, cv2.medianBlur(s3, 5), s3)
    hole = ~(s4 > t01) & _below_top(s4.shape, _top_rows(s4))
    s5 = np.where(hole, cv2.dilate(s4, FULL_KERNEL_9), s4)
    top = _top_rows(s5)
    cols = np.arange(s5.shape[1])
    if extrapolate:
        s6 = np.where(_below_top(s5.shape, top), s5, s5[top, cols][None, :])
        top_mask = np.ones(s5.shape, bool)
    else:
        s6 = s5.copy()
        top_mask = _below_top(s5.shape, top)
    s7 = s6.copy()
    for _ in range(6):
        s7 = np.where((s7 < t01) & top_mask, cv2.dilate(s7, FULL_KERNEL_5), s7)
    valid = (s7 > t01) & top_mask
    s7 = np.where(valid, cv2.medianBlur(s7, 5), s7)
    if blur_type == 'gaussian':
        valid = (s7 > t01) & top_mask
        s7 = np.where(valid, cv2.GaussianBlur(s7, (5, 5), 0), s7)
    elif blur_type == 'bilateral':
        s7 = np.where(valid, cv2.bilateralFilter(s7, 5, 0.5, 2.0), s7)
    s8 = np.where(s7 > t01, md - s7, s7)
    return s8, dict(zip(STAGES, (s1, s2, s3, s4, s5, s6, s7, s8)))

"""numpy fp64 restatement of csrc/object_pairs.hip, in the kernels' operation order.

object_pairs: each row's two boxes through the clipping of csrc/kitti_geometry.h, product by product (Python floats are
IEEE doubles and nothing is fused; only cos / sin may differ from the device's by an ulp).
metric_stats_binned: thread t of 256 adds its elements t, t + 256, ... in order, then the LDS tree adds lds[t + s] into
lds[t] for s = 128 .. 1: the same pairs in the same order, so the result is the kernel's bit for bit.
"""
import math

import numpy as np

HIT_THRESHOLDS = ((2, 0.7), (2, 0.5), (2, 0.25), (1, 0.7), (1, 0.5))  # (overlaps column, threshold) of table[:, 4:9]
MIN_HEIGHT, MAX_OCCLUSION = (40, 25, 25), (0, 1, 2)
# the label's truncation arrives as float32: the limits are rounded the same way, so that a label on 0.15 or 0.3 in the
# label file keeps the level the KITTI program gives it
MAX_TRUNCATION = tuple(float(np.float32(v)) for v in (0.15, 0.3, 0.5))
THREADS = 256
NAN = float('nan')


def _corners(x, z, l, w, ry):
    c, s = math.cos(ry), math.sin(ry)
    l2, w2 = l / 2, w / 2
    cx, cz = (l2, l2, -l2, -l2), (w2, -w2, -w2, w2)
    return [c * cx[i] + s * cz[i] + x for i in range(4)], [-s * cx[i] + c * cz[i] + z for i in range(4)]


def _shoelace(px, pz, n):
    a = 0.0
    for i in range(n):
        j = 0 if i + 1 == n else i + 1
        a += px[i] * pz[j] - px[j] * pz[i]
    return abs(a) / 2


def _bev_intersection(d, g):
    """d, g: (x, z, l, w, ry) -> (intersection, area_d, area_g)"""
    sx, sz = _corners(*d)
    gx, gz = _corners(*g)
    area_d, area_g = _shoelace(sx, sz, 4), _shoelace(gx, gz, 4)
    orient = 0.0
    for i in range(4):
        orient += gx[i] * gz[(i + 1) & 3] - gx[(i + 1) & 3] * gz[i]
    sgn = -1.0 if orient < 0 else 1.0
    n = 4
    for e in range(4):
        if n <= 0:
            break
        ax, az = gx[e], gz[e]
        ex, ez = gx[(e + 1) & 3] - ax, gz[(e + 1) & 3] - az
        tx, tz = [], []
        for i in range(n):
            j = 0 if i + 1 == n else i + 1
            si = sgn * (ex * (sz[i] - az) - ez * (sx[i] - ax))
            sj = sgn * (ex * (sz[j] - az) - ez * (sx[j] - ax))
            if si >= 0:
                tx.append(sx[i])
                tz.append(sz[i])
            if (si >= 0) != (sj >= 0):
                t = si / (si - sj)
                tx.append(sx[i] + t * (sx[j] - sx[i]))
                tz.append(sz[i] + t * (sz[j] - sz[i]))
        n = min(len(tx), 8)
        sx, sz = tx[:n], tz[:n]
    return (_shoelace(sx, sz, n) if n >= 3 else 0.0), area_d, area_g


def box_overlaps(p, g):
    """p, g: [x y z l w h ry] -> (iou_bev, iou_3d, centre_dist); NaN where a field is not finite."""
    p, g = [float(v) for v in p], [float(v) for v in g]
    if not all(math.isfinite(v) for v in p + g):
        return NAN, NAN, NAN
    (px, py, pz, pl, pw, ph, pry), (gx, gy, gz, gl, gw, gh, gry) = p, g
    bev_ok = pl > 0 and pw > 0 and gl > 0 and gw > 0
    box_ok = bev_ok and ph > 0 and gh > 0
    inter, area_d, area_g = 0.0, 1.0, 1.0
    if bev_ok:
        inter, area_d, area_g = _bev_intersection((px, pz, pl, pw, pry), (gx, gz, gl, gw, gry))
    iou_bev = inter / (area_d + area_g - inter) if bev_ok else 0.0
    ymax, ymin = min(py, gy), max(py - ph, gy - gh)
    inter_vol = inter * max(0.0, ymax - ymin)
    det_vol, gt_vol = ph * pl * pw, gh * gl * gw
    iou_3d = inter_vol / (det_vol + gt_vol - inter_vol) if box_ok else 0.0
    dx, dz = px - gx, pz - gz
    dy = (py - ph / 2) - (gy - gh / 2)
    return iou_bev, iou_3d, math.sqrt((dx * dx + dy * dy) + dz * dz)


def image_iou(a, b):
    """a, b: [x1, y1, x2, y2]; a is the detection (its area is added first)."""
    a, b = [float(v) for v in a], [float(v) for v in b]
    if not all(math.isfinite(v) for v in a + b):
        return NAN
    x1, y1, x2, y2 = max(a[0], b[0]), max(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def difficulty(info):
    """info: [truncation, occlusion, x1, y1, x2, y2] -> 0..3, or -1 when a value is not finite."""
    v = [float(x) for x in info]
    if not all(math.isfinite(x) for x in v):
        return -1
    height = v[5] - v[3]
    for level in range(3):
        if height > MIN_HEIGHT[level] and v[1] <= MAX_OCCLUSION[level] and v[0] <= MAX_TRUNCATION[level]:
            return level
    return 3


def bin_of(edges, x):
    return int(sum(1 for e in edges if e <= x))


def object_pairs(pred, gt, fed, info, depth_edges, box_iou_edges):
    """-> (overlaps (n,4) float64, table (n,9) float32, bins (n,3) int32) of mpsr_object_pairs."""
    n = len(pred)
    overlaps, bins = np.full((n, 4), np.nan), np.full((n, 3), -1, np.int32)
    full = np.full((n, 9), np.nan)
    for i in range(n):
        iou_bev, iou_3d, dist = box_overlaps(pred[i], gt[i])
        iou_fed = NAN
        if fed is not None and info is not None:
            y1, x1, y2, x2 = fed[i]
            iou_fed = image_iou([x1, y1, x2, y2], info[i][2:6])
        overlaps[i] = (iou_fed, iou_bev, iou_3d, dist)
        full[i, 0:4] = overlaps[i]
        for k, (col, thr) in enumerate(HIT_THRESHOLDS):
            v = overlaps[i, col]
            full[i, 4 + k] = v if v != v else float(v >= thr)
        z = float(gt[i][2])
        bins[i, 0] = bin_of(depth_edges, z) if math.isfinite(z) else -1
        bins[i, 1] = difficulty(info[i]) if info is not None else -1
        bins[i, 2] = -1 if iou_fed != iou_fed else bin_of(box_iou_edges, iou_fed)
    return overlaps, full.astype(np.float32), bins


def _block_sum(per_thread):
    lds = per_thread.copy()
    s = THREADS // 2
    while s >= 1:
        lds[:s] += lds[s:2 * s]
        s //= 2
    return lds[0]


def _thread_sums(terms):
    """terms (n_elem,) in element order -> (256,): thread t adds terms[t], terms[t + 256], ... in order, from 0.0"""
    rows = -(-len(terms) // THREADS)
    padded = np.zeros(rows * THREADS)
    padded[:len(terms)] = terms
    acc = np.zeros(THREADS)
    for row in padded.reshape(rows, THREADS):
        acc = acc + row
    return acc


def slot_stats(values, column_metric, n_metrics, in_slot):
    """(n_metrics, 6) of the rows in_slot (bool, n_rows) under the entry rule, in the kernel's order of summation."""
    out = np.zeros((n_metrics, 6))
    for m in range(n_metrics):
        cols = [c for c, k in enumerate(column_metric) if k == m]
        v = values[:, cols].astype(np.float64).reshape(-1)  # element e = (row e / k, the e % k-th column)
        there = np.repeat(np.asarray(in_slot, bool), len(cols))
        nan = np.isnan(v)
        ok = there & ~nan
        x = np.where(ok, v, 0.0)
        cnt = _block_sum(_thread_sums(ok.astype(np.float64)))
        drop = _block_sum(_thread_sums((there & nan).astype(np.float64)))
        total, total_abs = _block_sum(_thread_sums(x)), _block_sum(_thread_sums(np.abs(x)))
        if cnt > 0:
            mean, mean_abs = total / cnt, total_abs / cnt
            d, da = np.where(ok, v - mean, 0.0), np.where(ok, np.abs(v) - mean_abs, 0.0)
            sq, sq_abs = _block_sum(_thread_sums(d * d)), _block_sum(_thread_sums(da * da))
            out[m] = (cnt, mean, math.sqrt(sq / cnt), mean_abs, math.sqrt(sq_abs / cnt), drop)
        else:
            out[m] = (cnt, NAN, NAN, NAN, NAN, drop)
    return out


def slots_of(bins, axis_bins):
    """[in_slot (n_rows,) bool] for slot 0 (every row), then the bins of axis 0, of axis 1, ..."""
    bins = np.asarray(bins).reshape(-1, len(axis_bins))
    out = [np.ones(len(bins), bool)]
    for a, nb in enumerate(axis_bins):
        out += [bins[:, a] == b for b in range(nb)]
    return out


def metric_stats_binned(values, bins, column_metric, n_metrics, axis_bins):
    """-> (1 + sum(axis_bins), n_metrics, 6) of mpsr_metric_stats_binned."""
    return np.stack([slot_stats(values, column_metric, n_metrics, s) for s in slots_of(bins, axis_bins)])

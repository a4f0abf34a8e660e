"""numpy restatement of mpsr_shape_scores (include/monopsr_hip.h), written twice: vectorised (nearest_vectorised) and as a
loop over the points (nearest_loop).

A point is valid when its mask entry is > 0 (no mask: all ones; NaN is not > 0) and its three coordinates are finite.
d of a valid point = the minimum over the other cloud's valid points of the float32 squared distance, float32
differences, float32 products, (dx*dx + dy*dy) + dz*dz: numpy rounds every float32 operation, nothing is fused.  +inf
when the other cloud has no valid point (the caller turns that box into an empty side), NaN at points that are not
valid.  Counts compare (double) d <= t * t in fp64; sums are math.fsum over fp64 terms, so they carry one rounding.
"""
import math

import numpy as np

NAN32 = np.float32(np.nan)


def valid_points(points, mask):
    """points (P, 3) float32, mask (P,) float32 or None -> (P,) bool"""
    ok = np.isfinite(points).all(axis=1)
    if mask is not None:
        with np.errstate(invalid='ignore'):
            ok &= mask > 0
    return ok


def nearest_vectorised(q, q_ok, r, r_ok):
    """(P,) float32: d of the valid points of q against the valid points of r, NaN at the others."""
    out = np.full(len(q), NAN32, np.float32)
    qs, rs = q[q_ok], r[r_ok]
    if len(qs) == 0:
        return out
    if len(rs) == 0:
        out[q_ok] = np.float32(np.inf)
        return out
    with np.errstate(over='ignore'):
        dx = rs[None, :, 0] - qs[:, None, 0]
        dy = rs[None, :, 1] - qs[:, None, 1]
        dz = rs[None, :, 2] - qs[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    out[q_ok] = d.min(axis=1)
    return out


def nearest_loop(q, q_ok, r, r_ok):
    """nearest_vectorised, point by point, the mask and the finiteness tested per point."""
    out = np.full(len(q), NAN32, np.float32)
    keep = [j for j in range(len(r)) if r_ok[j]]
    rx, ry, rz = (r[keep, k] for k in range(3))
    for i in range(len(q)):
        if not q_ok[i]:
            continue
        if not keep:
            out[i] = np.float32(np.inf)
            continue
        with np.errstate(over='ignore'):
            dx, dy, dz = rx - q[i, 0], ry - q[i, 1], rz - q[i, 2]
            d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        out[i] = d.min()
    return out


def valid_points_loop(points, mask):
    ok = np.zeros(len(points), bool)
    for i in range(len(points)):
        m = 1.0 if mask is None else float(mask[i])
        ok[i] = m > 0 and all(math.isfinite(float(c)) for c in points[i])
    return ok


def table_row(counts_row, sums_row, T):
    """The float32 table row of one box from its counts (2 + 2T) and sums (6), the formulas in fp64."""
    n_a, n_b = int(counts_row[0]), int(counts_row[1])
    row = np.full(5 + 3 * T, np.nan)
    if n_a == 0 or n_b == 0:
        return row.astype(np.float32)
    s = [float(v) for v in sums_row]
    acc, comp = s[0] / n_a, s[2] / n_b
    row[0:5] = [acc, comp, (acc + comp) / 2, s[1] / n_a + s[3] / n_b, math.sqrt(max(s[4], s[5]))]
    for t in range(T):
        p, r = int(counts_row[2 + t]) / n_a, int(counts_row[2 + T + t]) / n_b
        row[5 + 3 * t:8 + 3 * t] = [p, r, 0.0 if p + r == 0 else 2 * p * r / (p + r)]
    return row.astype(np.float32)


def table(counts, sums, T):
    return np.stack([table_row(c, s, T) for c, s in zip(counts, sums)]) if len(counts) else \
        np.zeros((0, 5 + 3 * T), np.float32)


def shape_scores(a, b, mask_a, mask_b, thresholds, loop=False):
    """a (n, P, 3), b (n, Q, 3) float32; mask_a (n, P), mask_b (n, Q) float32 or None; thresholds: T floats.
    -> dict(counts (n, 2 + 2T) int32, sums (n, 6) float64, table (n, 5 + 3T) float32, dist_a (n, P), dist_b (n, Q)
    float32, terms (n, 4): the number of terms of each of the four sums, abs_sums (n, 4): the sum of their
    magnitudes)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, P, Q, T = a.shape[0], a.shape[1], b.shape[1], len(thresholds)
    limits = [float(t) * float(t) for t in thresholds]
    nearest, valid = (nearest_loop, valid_points_loop) if loop else (nearest_vectorised, valid_points)
    counts = np.zeros((n, 2 + 2 * T), np.int32)
    sums = np.full((n, 6), np.nan)
    dist_a, dist_b = np.full((n, P), NAN32, np.float32), np.full((n, Q), NAN32, np.float32)
    terms, abs_sums = np.zeros((n, 4), np.int64), np.zeros((n, 4))
    for k in range(n):
        a_ok = valid(a[k], None if mask_a is None else mask_a[k])
        b_ok = valid(b[k], None if mask_b is None else mask_b[k])
        counts[k, 0], counts[k, 1] = a_ok.sum(), b_ok.sum()
        if counts[k, 0] == 0 or counts[k, 1] == 0:
            continue  # an empty side: NaN sums, NaN dist rows, within counts 0
        dist_a[k], dist_b[k] = nearest(a[k], a_ok, b[k], b_ok), nearest(b[k], b_ok, a[k], a_ok)
        for side, (d, ok) in enumerate(((dist_a[k], a_ok), (dist_b[k], b_ok))):
            d64 = d[ok].astype(np.float64)
            roots = np.sqrt(d64)
            sums[k, 2 * side] = math.fsum(roots)
            sums[k, 2 * side + 1] = math.fsum(d64)
            sums[k, 4 + side] = float(d[ok].max())
            terms[k, 2 * side] = terms[k, 2 * side + 1] = len(d64)
            abs_sums[k, 2 * side], abs_sums[k, 2 * side + 1] = sums[k, 2 * side], sums[k, 2 * side + 1]
            for t in range(T):
                counts[k, 2 + side * T + t] = int((d64 <= limits[t]).sum())
    return dict(counts=counts, sums=sums, table=table(counts, sums, T), dist_a=dist_a, dist_b=dist_b, terms=terms,
                abs_sums=abs_sums)


def sum_bound(m, abs_sum):
    """How far a device sum of m non-negative fp64 terms may be from the restatement's: (m + 2) 2^-52 sum |term|.
    Derived, not measured: each root is within one ulp of the correctly rounded one the restatement adds (2^-52
    relative, over the whole sum 2^-52 sum |term|); adding m terms in any order is within (m - 1) 2^-53 sum |term| of
    the exact sum to first order, doubled here to cover the higher orders; math.fsum's one rounding is 2^-53 more."""
    return (m + 2) * 2.0 ** -52 * abs_sum


def same_bits(x, y):
    """Equal bit for bit, every NaN counting as one value (the device's NaN carries no agreed payload)."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.dtype.kind != 'f':
        return bool(np.array_equal(x, y))
    nan = np.isnan(x)
    ints = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    return bool(np.array_equal(nan, np.isnan(y)) and np.array_equal(x[~nan].view(ints), y[~nan].view(ints)))

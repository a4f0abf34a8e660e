"""numpy restatement of mpsr_surface_scores (include/monopsr_hip.h), written twice: vectorised over queries and
triangles (loop=False) and as a plain loop over queries and triangles on Python floats in the stated operation order
(loop=True; Python's float is the IEEE fp64 of the definition, every operation rounded once, nothing fused).

The point term is tests/shape_score_restatement.py's float32 arithmetic (nearest_vectorised / nearest_loop) and the
validity rule is its valid_points / valid_points_loop.  A triangle of the (h, w) grid is KEPT when its three corners
are valid and each float32 squared edge length, (dx*dx + dy*dy) + dz*dz in float32, converted to fp64, is
<= max_edge * max_edge.  d of a valid query = min((double) d_point, the edge and face terms of every kept triangle of
the other grid), the terms in fp64 with every dot product (x0 y0 + x1 y1) + x2 y2.

The loop costs a few microseconds per (query, triangle) pair, so it takes `queries`, an optional list of point
indices per call: the distances of the other points are then NaN and the statistics are taken by the caller over the
queries alone.  The vectorised version is the one the device is compared with, over every point.
"""
import math

import numpy as np

import shape_score_restatement as points

NAN = float('nan')
same_bits, sum_bound, table, table_row = points.same_bits, points.sum_bound, points.table, points.table_row


def triangle_ids(h, w):
    """(2 (h - 1)(w - 1), 3) point indices in id order: cell (i, j) gives k = 0: (v00, v01, v10), k = 1: (v11, v10,
    v01), t = (i (w - 1) + j) 2 + k."""
    out = []
    for i in range(h - 1):
        for j in range(w - 1):
            v00, v01, v10, v11 = i * w + j, i * w + j + 1, (i + 1) * w + j, (i + 1) * w + j + 1
            out += [(v00, v01, v10), (v11, v10, v01)]
    return np.asarray(out, np.int64).reshape(-1, 3)


def _len2_f32(u, v):
    """float32 squared length(s) of u -> v, float32 differences and products, (dx dx + dy dy) + dz dz"""
    with np.errstate(over='ignore', invalid='ignore'):
        dx, dy, dz = v[..., 0] - u[..., 0], v[..., 1] - u[..., 1], v[..., 2] - u[..., 2]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def kept_triangles(grid, ok, h, w, max_edge):
    """grid (h w, 3) float32, ok (h w,) bool -> (m, 3) point indices of the kept triangles, in id order"""
    tri = triangle_ids(h, w)
    if len(tri) == 0:
        return tri
    limit = float(max_edge) * float(max_edge)
    keep = ok[tri].all(axis=1)
    for u, v in ((0, 1), (1, 2), (2, 0)):
        with np.errstate(invalid='ignore'):
            keep &= _len2_f32(grid[tri[:, u]], grid[tri[:, v]]).astype(np.float64) <= limit
    return tri[keep]


def kept_triangles_loop(grid, ok, h, w, max_edge):
    limit = float(max_edge) * float(max_edge)
    out = []
    for t in triangle_ids(h, w):
        if not all(ok[int(i)] for i in t):
            continue
        fits = True
        for u, v in ((0, 1), (1, 2), (2, 0)):
            with np.errstate(over='ignore'):
                dx, dy, dz = (grid[t[v], k] - grid[t[u], k] for k in range(3))
                len2 = (dx * dx + dy * dy) + dz * dz
            assert isinstance(len2, np.float32)
            fits = fits and float(len2) <= limit
        if fits:
            out.append(t)
    return np.asarray(out, np.int64).reshape(-1, 3)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def surface_min_vectorised(d_point, q, q_ok, r, tri, chunk=256):
    """d_point (P,) float32 (NaN at the points that are not valid), q and r (P, 3) float32, tri (m, 3) kept triangles
    of r -> (P,) float64"""
    out = d_point.astype(np.float64)
    if len(tri) == 0:
        return out
    r64 = r.astype(np.float64)
    A, B, C = ([r64[tri[:, c], k][None, :] for k in range(3)] for c in range(3))
    sub = lambda x, y: [x[k] - y[k] for k in range(3)]
    e_ab, e_bc, e_ca = sub(B, A), sub(C, B), sub(A, C)
    e0, e1 = e_ab, sub(C, A)
    n = [e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]]
    nn, d00, d01, d11 = _dot(n, n), _dot(e0, e0), _dot(e0, e1), _dot(e1, e1)
    den = d00 * d11 - d01 * d01
    idx = np.flatnonzero(q_ok)
    for at in range(0, len(idx), chunk):
        sel = idx[at:at + chunk]
        qs = [q[sel, k].astype(np.float64)[:, None] for k in range(3)]
        best = np.full((len(sel), tri.shape[0]), np.inf)
        with np.errstate(divide='ignore', invalid='ignore'):
            for U, e in ((A, e_ab), (B, e_bc), (C, e_ca)):
                wv = sub(qs, U)
                ee, t = _dot(e, e), _dot(wv, e)
                hit = (ee > 0) & (t > 0) & (t < ee)
                s = t / ee
                rv = [wv[k] - s * e[k] for k in range(3)]
                best = np.where(hit, np.minimum(best, _dot(rv, rv)), best)
            wv = sub(qs, A)
            d20, d21 = _dot(wv, e0), _dot(wv, e1)
            v, u = d11 * d20 - d01 * d21, d00 * d21 - d01 * d20
            hit = (nn > 0) & (den > 0) & (v > 0) & (u > 0) & (v + u < den)
            hq = _dot(wv, n)
            best = np.where(hit, np.minimum(best, hq * hq / nn), best)
        out[sel] = np.minimum(out[sel], best.min(axis=1))
    return out


def surface_min_loop(d_point, q, q_ok, r, tri, queries=None):
    """surface_min_vectorised, query by query and triangle by triangle on Python floats; the points outside `queries`
    (a list of indices, None for all) get NaN."""
    out = np.full(len(q), NAN)
    corners = [[[float(c) for c in r[int(i)]] for i in t] for t in tri]
    for i in (range(len(q)) if queries is None else queries):
        if not q_ok[i]:
            continue
        d = float(d_point[i])
        qx, qy, qz = (float(c) for c in q[i])
        for A, B, C in corners:
            for U, V in ((A, B), (B, C), (C, A)):
                ex, ey, ez = V[0] - U[0], V[1] - U[1], V[2] - U[2]
                wx, wy, wz = qx - U[0], qy - U[1], qz - U[2]
                ee = (ex * ex + ey * ey) + ez * ez
                t = (wx * ex + wy * ey) + wz * ez
                if ee > 0 and t > 0 and t < ee:
                    s = t / ee
                    rx, ry, rz = wx - s * ex, wy - s * ey, wz - s * ez
                    term = (rx * rx + ry * ry) + rz * rz
                    if term < d:
                        d = term
            e0x, e0y, e0z = B[0] - A[0], B[1] - A[1], B[2] - A[2]
            e1x, e1y, e1z = C[0] - A[0], C[1] - A[1], C[2] - A[2]
            nx, ny, nz = e0y * e1z - e0z * e1y, e0z * e1x - e0x * e1z, e0x * e1y - e0y * e1x
            nn = (nx * nx + ny * ny) + nz * nz
            d00 = (e0x * e0x + e0y * e0y) + e0z * e0z
            d01 = (e0x * e1x + e0y * e1y) + e0z * e1z
            d11 = (e1x * e1x + e1y * e1y) + e1z * e1z
            den = d00 * d11 - d01 * d01
            wx, wy, wz = qx - A[0], qy - A[1], qz - A[2]
            d20 = (wx * e0x + wy * e0y) + wz * e0z
            d21 = (wx * e1x + wy * e1y) + wz * e1z
            v = d11 * d20 - d01 * d21
            u = d00 * d21 - d01 * d20
            if nn > 0 and den > 0 and v > 0 and u > 0 and v + u < den:
                hq = (wx * nx + wy * ny) + wz * nz
                term = hq * hq / nn
                if term < d:
                    d = term
        out[i] = d
    return out


def surface_scores(a, b, mask_a, mask_b, thresholds, max_edge, loop=False, queries=None):
    """a, b (n, h, w, 3) float32; mask_a, mask_b (n, h w) float32 or None; thresholds: T floats; max_edge: a float.
    -> dict(counts (n, 2 + 2T) int32, sums (n, 6) float64, table (n, 5 + 3T) float32, dist_a, dist_b (n, h w) float64,
    tri_counts (n, 2) int32, point_a, point_b (n, h w) float32: the point terms, terms (n, 4) and abs_sums (n, 4) as
    shape_score_restatement.shape_scores returns them).  With loop and `queries` (point indices) the distances
    are those of the queries alone and counts, sums and table are not computed (None)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    n, h, w = a.shape[:3]
    P, T = h * w, len(thresholds)
    a, b = a.reshape(n, P, 3), b.reshape(n, P, 3)
    limits = [float(t) * float(t) for t in thresholds]
    nearest, valid = (points.nearest_loop, points.valid_points_loop) if loop else \
        (points.nearest_vectorised, points.valid_points)
    kept = kept_triangles_loop if loop else kept_triangles
    counts = np.zeros((n, 2 + 2 * T), np.int32)
    sums = np.full((n, 6), np.nan)
    tri_counts = np.zeros((n, 2), np.int32)
    dist_a, dist_b = np.full((n, P), np.nan), np.full((n, P), np.nan)
    point_a, point_b = np.full((n, P), np.nan, np.float32), np.full((n, P), np.nan, np.float32)
    terms, abs_sums = np.zeros((n, 4), np.int64), np.zeros((n, 4))
    for k in range(n):
        a_ok = valid(a[k], None if mask_a is None else mask_a[k])
        b_ok = valid(b[k], None if mask_b is None else mask_b[k])
        tri_a, tri_b = kept(a[k], a_ok, h, w, max_edge), kept(b[k], b_ok, h, w, max_edge)
        counts[k, 0], counts[k, 1] = a_ok.sum(), b_ok.sum()
        tri_counts[k] = len(tri_a), len(tri_b)
        if counts[k, 0] == 0 or counts[k, 1] == 0:
            continue  # an empty side: NaN sums, NaN dist rows, within counts 0
        point_a[k], point_b[k] = nearest(a[k], a_ok, b[k], b_ok), nearest(b[k], b_ok, a[k], a_ok)
        if loop:
            dist_a[k] = surface_min_loop(point_a[k], a[k], a_ok, b[k], tri_b, queries)
            dist_b[k] = surface_min_loop(point_b[k], b[k], b_ok, a[k], tri_a, queries)
        else:
            dist_a[k] = surface_min_vectorised(point_a[k], a[k], a_ok, b[k], tri_b)
            dist_b[k] = surface_min_vectorised(point_b[k], b[k], b_ok, a[k], tri_a)
        if queries is not None:
            continue
        for side, (d, ok) in enumerate(((dist_a[k], a_ok), (dist_b[k], b_ok))):
            d64 = d[ok]
            roots = np.sqrt(d64)
            sums[k, 2 * side] = math.fsum(roots)
            sums[k, 2 * side + 1] = math.fsum(d64)
            sums[k, 4 + side] = float(d64.max())
            terms[k, 2 * side] = terms[k, 2 * side + 1] = len(d64)
            abs_sums[k, 2 * side], abs_sums[k, 2 * side + 1] = sums[k, 2 * side], sums[k, 2 * side + 1]
            for t in range(T):
                counts[k, 2 + side * T + t] = int((d64 <= limits[t]).sum())
    out = dict(dist_a=dist_a, dist_b=dist_b, tri_counts=tri_counts, point_a=point_a, point_b=point_b)
    if queries is None:
        out.update(counts=counts, sums=sums, table=table(counts, sums, T), terms=terms, abs_sums=abs_sums)
    return out

"""The surface rendering of csrc/scene.hip restated with Python integers and floats (IEEE
fp64, never contracted) in the stated operation order, as plain loops: one triangle at a time, one pixel at a time.  The
z-buffer is a minimum over keys; the score's sums run in the kernel's slice, tree and wave order.  Nothing here is
shared with the kernels or with monopsr_amd.core.scene_reconstruction.

A case is a dict: xyz (B,Hm,Wm,3) float32, box_frame (B,) int, cam_p (F,3,4) float64, shapes [(h,w)] * F, optionally
mask (B,Hm,Wm) float32 and keep (B,) int, and the two options max_edge_dz (default 1.0) and max_span_px (default 64).
"""
import numpy as np

EMPTY_KEY = (1 << 64) - 1
SUB = 256
COUNT_NAMES = ('tris', 'pred_px', 'inter_px', 'gt_px', 'depth_n')
METRIC_NAMES = ('surface_mask_iou', 'surface_mask_precision', 'surface_mask_recall', 'surface_depth_bias',
                'surface_depth_mae', 'surface_depth_rmse')
THREADS, WAVE = 256, 64


def vertices(case):
    """-> (valid (B,Hm,Wm) bool, X, Y (B,Hm,Wm) int64: the fixed-point screen coordinates; 0 where not valid)."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, mh, mw = xyz.shape[:3]
    bf = np.asarray(case['box_frame'], np.int64).reshape(nb)
    cam = np.asarray(case['cam_p'], np.float64).reshape(-1, 3, 4)
    if nb == 0:
        return np.zeros((0, mh, mw), bool), np.zeros((0, mh, mw), np.int64), np.zeros((0, mh, mw), np.int64)
    x, y, z = (xyz[..., k].astype(np.float64) for k in range(3))
    P = cam[bf][:, None, None]  # (B,1,1,3,4)
    with np.errstate(all='ignore'):
        u = [((P[..., k, 0] * x + P[..., k, 1] * y) + P[..., k, 2] * z) + P[..., k, 3] for k in range(3)]
        c, r = u[0] / u[2], u[1] / u[2]
        on = np.isfinite(xyz).all(-1) & (xyz[..., 2] > 0) & (u[2] > 0)
        if case.get('mask') is not None:
            on &= np.asarray(case['mask'], np.float32).reshape(nb, mh, mw) > 0
        if case.get('keep') is not None:
            on &= (np.asarray(case['keep']).reshape(nb) != 0)[:, None, None]
        on &= (np.abs(c) < 2.0 ** 20) & (np.abs(r) < 2.0 ** 20)
        X = np.where(on, np.rint(np.where(on, c, 0.0) * 256.0), 0.0).astype(np.int64)
        Y = np.where(on, np.rint(np.where(on, r, 0.0) * 256.0), 0.0).astype(np.int64)
    return on, X, Y


def floor_div(v, d):
    return v // d  # Python's // is a true floor division


def ceil_div(v, d):
    return -((-v) // d)


def _owns(dx, dy):
    return dy > 0 or (dy == 0 and dx < 0)


def triangles_of(mh, mw):
    """[(i, j, k, (row, col) of a, b, c)] in triangle-id order within a box."""
    out = []
    for i in range(mh - 1):
        for j in range(mw - 1):
            v00, v01, v10, v11 = (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
            out.append((i, j, 0, (v00, v01, v10)))
            out.append((i, j, 1, (v11, v10, v01)))
    return out


def render(case, cover=False):
    """-> dict: depth_maps [(h,w) float32], instance_maps [(h,w) uint8], tri_maps [(h,w) int32], tris (B,) int64 (drawn
    triangles), rect (B,4) int64 (min col, min row, max col, max row of the drawn triangles' clamped extents;
    min > max: none), drawn (B, n_tris_per_box) bool; with cover=True also cover [(h,w) int64]: how many drawn
    triangles cover each pixel centre."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, mh, mw = xyz.shape[:3]
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    nf = len(shapes)
    bf = [int(v) for v in np.asarray(case['box_frame']).reshape(nb)]
    max_dz = np.float32(case.get('max_edge_dz', 1.0))
    max_span = int(case.get('max_span_px', 64))
    valid, X, Y = vertices(case)
    zf32 = xyz[..., 2]
    per_box = 2 * (mh - 1) * (mw - 1)
    tri_list = triangles_of(mh, mw)
    keys = [[EMPTY_KEY] * (h * w) for h, w in shapes]  # Python ints: 64 bits without overflow
    covers = [np.zeros((h, w), np.int64) for h, w in shapes]
    tris = np.zeros(nb, np.int64)
    big = np.iinfo(np.int32)
    rect = np.tile(np.asarray([big.max, big.max, big.min, big.min], np.int64), (nb, 1))
    drawn = np.zeros((nb, per_box), bool)
    for b in range(nb):
        f = bf[b]
        h, w = shapes[f]
        for n, (i, j, k, corners) in enumerate(tri_list):
            t = b * per_box + n
            assert t == ((b * (mh - 1) + i) * (mw - 1) + j) * 2 + k
            if not all(valid[b, r, c] for r, c in corners):
                continue
            z3 = [zf32[b, r, c] for r, c in corners]
            if np.float32(max(z3)) - np.float32(min(z3)) > max_dz:  # float32 difference, strict
                continue
            (ax, ay), (bx, by), (cx, cy) = [(int(X[b, r, c]), int(Y[b, r, c])) for r, c in corners]
            A = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            if A == 0:
                continue
            c0, c1 = ceil_div(min(ax, bx, cx), SUB), floor_div(max(ax, bx, cx), SUB)
            r0, r1 = ceil_div(min(ay, by, cy), SUB), floor_div(max(ay, by, cy), SUB)
            if c1 - c0 + 1 > max_span or r1 - r0 + 1 > max_span:
                continue
            tris[b] += 1
            drawn[b, n] = True
            za, zb, zc = (float(v) for v in z3)
            if A < 0:
                (bx, by), (cx, cy) = (cx, cy), (bx, by)
                zb, zc = zc, zb
                A = -A
            c0, c1, r0, r1 = max(c0, 0), min(c1, w - 1), max(r0, 0), min(r1, h - 1)
            if c0 > c1 or r0 > r1:
                continue
            rect[b] = [min(rect[b, 0], c0), min(rect[b, 1], r0), max(rect[b, 2], c1), max(rect[b, 3], r1)]
            own0, own1, own2 = _owns(cx - bx, cy - by), _owns(ax - cx, ay - cy), _owns(bx - ax, by - ay)
            wa, wb, wc = 1.0 / za, 1.0 / zb, 1.0 / zc
            for row in range(r0, r1 + 1):
                sy = SUB * row
                for col in range(c0, c1 + 1):
                    sx = SUB * col
                    e0 = (cx - bx) * (sy - by) - (cy - by) * (sx - bx)
                    e1 = (ax - cx) * (sy - cy) - (ay - cy) * (sx - cx)
                    e2 = (bx - ax) * (sy - ay) - (by - ay) * (sx - ax)
                    assert e0 + e1 + e2 == A
                    if (e0 > 0 or (e0 == 0 and own0)) and (e1 > 0 or (e1 == 0 and own1)) and \
                            (e2 > 0 or (e2 == 0 and own2)):
                        q = (float(e0) * wa + float(e1) * wb) + float(e2) * wc
                        z = np.float32(float(A) / q)
                        key = (int(z.view(np.uint32)) << 32) | t
                        at = row * w + col
                        if key < keys[f][at]:
                            keys[f][at] = key
                        covers[f][row, col] += 1
    first_box = [min([b for b in range(nb) if bf[b] >= f] or [nb]) for f in range(nf)]
    depth_maps, instance_maps, tri_maps = [], [], []
    for f, (h, w) in enumerate(shapes):
        d, inst = np.zeros(h * w, np.uint32), np.full(h * w, 255, np.uint8)
        tri = np.full(h * w, -1, np.int64)
        for at, key in enumerate(keys[f]):
            if key != EMPTY_KEY:
                d[at] = key >> 32
                tri[at] = key & 0xffffffff
                inst[at] = (key & 0xffffffff) // per_box - first_box[f]
        depth_maps.append(d.view(np.float32).reshape(h, w))
        instance_maps.append(inst.reshape(h, w))
        tri_maps.append(tri.astype(np.uint32).view(np.int32).reshape(h, w))
    out = dict(depth_maps=depth_maps, instance_maps=instance_maps, tri_maps=tri_maps, tris=tris, rect=rect, drawn=drawn)
    if cover:
        out['cover'] = covers
    return out


def _tree(values):
    """Lane 0 of the fixed __shfl_down tree over 64 lanes: lane l += lane l + o for o = 32, 16, ..., 1 (a lane whose
    partner is beyond the wave adds its own value: it never reaches lane 0)."""
    v = list(values)
    for o in (32, 16, 8, 4, 2, 1):
        v = [v[l] + (v[l + o] if l + o < WAVE else v[l]) for l in range(WAVE)]
    return v[0]


def scores(case, gt, rendering=None):
    """-> dict: counts (B,5) int64 = tris, pred_px, inter_px, gt_px, depth_n; sums (B,3) float64 = the sums of e, |e|
    and e * e over the depth_n pixels in the kernel's order: the box's rectangle row-major in slices of 256, thread
    q % 256 adding in slice order, the tree within each wave of 64, the four waves in order."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, mh, mw = xyz.shape[:3]
    per_box = 2 * (mh - 1) * (mw - 1)
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    bf = [int(v) for v in np.asarray(case['box_frame']).reshape(nb)]
    if rendering is None:
        rendering = render(case)
    counts = np.zeros((nb, 5), np.int64)
    sums = np.zeros((nb, 3), np.float64)
    for b in range(nb):
        f = bf[b]
        g = int(np.asarray(gt['box_gt_id']).reshape(nb)[b])
        has_gt = 0 <= g <= 254
        true, d = np.asarray(gt['instance_images'][f], np.uint8), np.asarray(gt['depth_maps'][f], np.float32)
        tri, z = rendering['tri_maps'][f], rendering['depth_maps'][f]
        counts[b, 0] = rendering['tris'][b]
        counts[b, 3] = int((true == g).sum()) if has_gt else 0
        c0, r0, c1, r1 = (int(v) for v in rendering['rect'][b])
        rw = c1 - c0 + 1 if c0 <= c1 else 0
        area = rw * (r1 - r0 + 1) if r0 <= r1 else 0
        acc = [[0.0, 0.0, 0.0] for _ in range(THREADS)]
        for q in range(area):
            row, col = r0 + q // rw, c0 + q % rw
            t = int(tri[row, col])
            if t == -1:  # (an id is below 2^32 - 1)
                continue
            if (t & 0xffffffff) // per_box != b:
                continue
            counts[b, 1] += 1
            if not (has_gt and int(true[row, col]) == g):
                continue
            counts[b, 2] += 1
            depth = d[row, col]
            if np.isfinite(depth) and depth > 0:
                counts[b, 4] += 1
                e = float(z[row, col]) - float(depth)
                a = acc[q % THREADS]
                a[0] += e
                a[1] += abs(e)
                a[2] += e * e
        for k in range(3):
            total = 0.0
            for wave in range(THREADS // WAVE):
                total += _tree([acc[wave * WAVE + l][k] for l in range(WAVE)])
            sums[b, k] = total
    return dict(counts=counts, sums=sums)


def table(counts, sums, box_gt_id):
    """The (B,6) float32 metric table in METRIC_NAMES order: fp64 quotients rounded once; NaN where there is none."""
    c = np.asarray(counts, np.float64)
    s = np.asarray(sums, np.float64)
    gid = np.asarray(box_gt_id, np.int64).reshape(-1)
    out = np.full((len(c), 6), np.nan, np.float64)
    for b in range(len(c)):
        _, pred_px, inter_px, gt_px, depth_n = c[b]
        union = pred_px + gt_px - inter_px
        if 0 <= gid[b] <= 254 and union > 0:
            out[b, 0] = inter_px / union
        if pred_px > 0:
            out[b, 1] = inter_px / pred_px
        if gt_px > 0:
            out[b, 2] = inter_px / gt_px
        if depth_n > 0:
            out[b, 3] = s[b, 0] / depth_n
            out[b, 4] = s[b, 1] / depth_n
            out[b, 5] = np.sqrt(s[b, 2] / depth_n)
    return out.astype(np.float32)

"""The mesh extraction of csrc/scene.hip restated with Python integers and floats (IEEE fp64,
never contracted) in the stated operation and summation order, as plain loops: one triangle, one map point at a time.
Which triangles are drawn and which win a pixel comes from tests/surface_restatement.py; nothing here is shared with
the kernels or with monopsr_amd.core.scene_reconstruction.

A case is the dict surface_restatement takes.  images: None or one (h, w, 3) float32 array per frame.
"""
import math

import numpy as np

import surface_restatement

THREADS, WAVE = 256, 64


def selected(case, rendering, visible_only):
    """-> (B, 2 (Hm - 1)(Wm - 1)) bool: the triangles in the mesh.  Drawn and, with visible_only, the id of at least one
    pixel of the resolved z-buffer."""
    sel = np.array(rendering['drawn'], bool)
    if visible_only:
        won = np.zeros(sel.size, bool)
        for tri in rendering['tri_maps']:
            for t in tri.reshape(-1):
                if t != -1:
                    won[int(t) & 0xffffffff] = True
        sel &= won.reshape(sel.shape)
    return sel


def _sub(p, q):
    return [p[0] - q[0], p[1] - q[1], p[2] - q[2]]


def face_cross(a, b, c):
    """(c - a) x (b - a) of three points of Python floats: differences, products, then one subtraction each."""
    u, v = _sub(c, a), _sub(b, a)
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def length3(n):
    return math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])


def pixel_of(cam, x, y, z):
    """-> (row, col, u2) of a point under the (3, 4) camera: u_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3, rint(u / u2)."""
    u = [((float(cam[k, 0]) * x + float(cam[k, 1]) * y) + float(cam[k, 2]) * z) + float(cam[k, 3]) for k in range(3)]
    with np.errstate(all='ignore'):
        col, row = np.rint(np.float64(u[0]) / np.float64(u[2])), np.rint(np.float64(u[1]) / np.float64(u[2]))
    return float(row), float(col), u[2]


def mesh(case, rendering=None, visible_only=False, images=None):
    """-> dict: xyz, rgb, normal (V,3) float32, vertex_box (V,) int64, faces (T,3) int64 (frame-local, in the order
    a, c, b), face_box (T,) int64, area (B,) float64, vertex_box_offset / face_box_offset (B+1,) and
    vertex_frame_offset / face_frame_offset (F+1,) int64; and, for the tests, point (V,) = the global map-point index
    of each vertex and tri (T,) = the triangle id of each face."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, mh, mw = xyz.shape[:3]
    npts, per_box = mh * mw, 2 * (mh - 1) * (mw - 1)
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    nf = len(shapes)
    bf = [int(v) for v in np.asarray(case['box_frame']).reshape(nb)]
    cam = np.asarray(case['cam_p'], np.float64).reshape(-1, 3, 4)
    if rendering is None:
        rendering = surface_restatement.render(case)
    sel = selected(case, rendering, visible_only)
    tri_list = surface_restatement.triangles_of(mh, mw)
    # the triangles of each map point, in increasing id
    incident = [[] for _ in range(npts)]
    for n, (_, _, _, corners) in enumerate(tri_list):
        for r, c in corners:
            incident[r * mw + c].append(n)
    assert all(len(v) <= 6 and v == sorted(v) for v in incident)
    out_xyz, out_rgb, out_normal, out_vbox, out_point = [], [], [], [], []
    out_faces, out_fbox, out_tri = [], [], []
    area = np.zeros(nb, np.float64)
    v_box, t_box = np.zeros(nb + 1, np.int64), np.zeros(nb + 1, np.int64)
    v_frame, t_frame = np.zeros(nf + 1, np.int64), np.zeros(nf + 1, np.int64)
    frame_start = {}  # frame -> vertices in front of it
    for b in range(nb):
        f = bf[b]
        h, w = shapes[f]
        frame_start.setdefault(f, len(out_xyz))
        pt = lambda r, c: [float(xyz[b, r, c, k]) for k in range(3)]
        rank = {}
        for p in range(npts):
            mine = [n for n in incident[p] if sel[b, n]]
            if not mine:
                continue
            rank[p] = len(out_xyz) - frame_start[f]
            r, c = divmod(p, mw)
            total = [0.0, 0.0, 0.0]
            for n in mine:  # in increasing triangle id
                (ra, ca), (rb, cb), (rc, cc) = tri_list[n][3]
                e = face_cross(pt(ra, ca), pt(rb, cb), pt(rc, cc))
                total = [total[0] + e[0], total[1] + e[1], total[2] + e[2]]
            length = length3(total)
            if length > 0.0 and math.isfinite(length):
                normal = [np.float32(total[k] / length) for k in range(3)]
            else:
                normal = [np.float32(0.0)] * 3
            colour = np.zeros(3, np.float32)
            if images is not None:
                row, col, u2 = pixel_of(cam[f], *pt(r, c))
                if u2 > 0.0 and 0.0 <= col < w and 0.0 <= row < h:
                    colour = np.asarray(images[f], np.float32)[int(row), int(col)]
            out_xyz.append(xyz[b, r, c])
            out_rgb.append(colour)
            out_normal.append(normal)
            out_vbox.append(b)
            out_point.append(b * npts + p)
        acc = [0.0] * THREADS  # thread n % 256 adds triangle n, in increasing n
        for n, (_, _, _, corners) in enumerate(tri_list):
            if not sel[b, n]:
                continue
            (ra, ca), (rb, cb), (rc, cc) = corners
            out_faces.append([rank[ra * mw + ca], rank[rc * mw + cc], rank[rb * mw + cb]])  # (a, c, b)
            out_fbox.append(b)
            out_tri.append(b * per_box + n)
            acc[n % THREADS] += 0.5 * length3(face_cross(pt(ra, ca), pt(rb, cb), pt(rc, cc)))
        total = 0.0
        for wave in range(THREADS // WAVE):
            total += surface_restatement._tree(acc[wave * WAVE:(wave + 1) * WAVE])
        area[b] = total
        v_box[b + 1], t_box[b + 1] = len(out_xyz), len(out_faces)
    for f in range(nf + 1):
        first = min([b for b in range(nb) if bf[b] >= f] or [nb])
        v_frame[f], t_frame[f] = v_box[first], t_box[first]
    arr = lambda rows, dtype, tail: np.asarray(rows, dtype).reshape((len(rows),) + tail)
    return dict(xyz=arr(out_xyz, np.float32, (3,)), rgb=arr(out_rgb, np.float32, (3,)),
                normal=arr(out_normal, np.float32, (3,)), vertex_box=arr(out_vbox, np.int64, ()),
                faces=arr(out_faces, np.int64, (3,)), face_box=arr(out_fbox, np.int64, ()), area=area,
                vertex_box_offset=v_box, face_box_offset=t_box, vertex_frame_offset=v_frame, face_frame_offset=t_frame,
                point=arr(out_point, np.int64, ()), tri=arr(out_tri, np.int64, ()))

"""csrc/scene.hip restated in numpy float64 with the kernel's explicit operation order: the projection vectorised
(`project`) and as a plain per-point loop (`project_loop`), the z-buffer and the compaction as plain per-point loops
(`scene`).  Nothing here is shared with the kernels or with monopsr_amd.core.scene_reconstruction.

A case is a dict: xyz (B,P,3) float32, box_frame (B,) int, cam_p (F,3,4) float64, shapes [(h,w)] * F, and optionally
mask (B,P) float32, keep (B,) int, images [ (h,w,3) float32 ] * F.
"""
import numpy as np

EMPTY_KEY = (1 << 64) - 1


def project(case):
    """-> pix (B,P) int64: row * w + col of a kept point, -1 of a dropped one (vectorised)."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, npts = xyz.shape[:2]
    bf = np.asarray(case['box_frame'], np.int64).reshape(nb)
    cam = np.asarray(case['cam_p'], np.float64).reshape(-1, 3, 4)
    hw = np.asarray([s[:2] for s in case['shapes']], np.int64).reshape(-1, 2)
    if nb == 0 or npts == 0:
        return np.zeros((nb, npts), np.int64)
    x, y, z = (xyz[..., k].astype(np.float64) for k in range(3))
    P = cam[bf][:, None]  # (B,1,3,4)
    with np.errstate(all='ignore'):
        u = [((P[..., k, 0] * x + P[..., k, 1] * y) + P[..., k, 2] * z) + P[..., k, 3] for k in range(3)]
        col, row = np.rint(u[0] / u[2]), np.rint(u[1] / u[2])
        h, w = hw[bf, 0][:, None].astype(np.float64), hw[bf, 1][:, None].astype(np.float64)
        on = np.isfinite(xyz).all(-1) & (xyz[..., 2] > 0) & (u[2] > 0)
        if case.get('mask') is not None:
            on &= np.asarray(case['mask'], np.float32).reshape(nb, npts) > 0
        if case.get('keep') is not None:
            on &= (np.asarray(case['keep']).reshape(nb) != 0)[:, None]
        on &= (col >= 0) & (col < w) & (row >= 0) & (row < h)
        pix = np.where(on, np.where(on, row, 0) * w + np.where(on, col, 0), -1)
    return pix.astype(np.int64)


def project_loop(case):
    """The same, one point at a time with Python-level control flow."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, npts = xyz.shape[:2]
    cam = np.asarray(case['cam_p'], np.float64).reshape(-1, 3, 4)
    pix = np.full((nb, npts), -1, np.int64)
    for b in range(nb):
        f = int(case['box_frame'][b])
        h, w = int(case['shapes'][f][0]), int(case['shapes'][f][1])
        if case.get('keep') is not None and int(np.asarray(case['keep']).reshape(nb)[b]) == 0:
            continue
        for p in range(npts):
            if case.get('mask') is not None and not np.asarray(case['mask'], np.float32).reshape(nb, npts)[b, p] > 0:
                continue
            xf, yf, zf = xyz[b, p]
            if not (np.isfinite(xf) and np.isfinite(yf) and np.isfinite(zf)) or not zf > 0:
                continue
            x, y, z = np.float64(xf), np.float64(yf), np.float64(zf)
            with np.errstate(all='ignore'):
                u = [((cam[f, k, 0] * x + cam[f, k, 1] * y) + cam[f, k, 2] * z) + cam[f, k, 3] for k in range(3)]
                if not u[2] > 0:
                    continue
                col, row = np.rint(u[0] / u[2]), np.rint(u[1] / u[2])
            if col >= 0 and col < w and row >= 0 and row < h:
                pix[b, p] = int(row) * w + int(col)
    return pix


def scene(case, visible_only=False, pix=None):
    """-> dict: xyz (M,3) float32, rgb (M,3) float32 or None, box (M,) int32, pixel (M,) int32, frame_offset (F+1,)
    int64, depth_maps / instance_maps (lists), kept_per_box / visible_per_box (B,) int32."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, npts = xyz.shape[:2]
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    nf = len(shapes)
    bf = [int(v) for v in np.asarray(case['box_frame']).reshape(nb)]
    if pix is None:
        pix = project(case)
    zbits = xyz[..., 2].copy().view(np.uint32)
    keys = [[EMPTY_KEY] * (h * w) for h, w in shapes]  # Python ints: 64 bits without overflow
    for b in range(nb):
        for p in range(npts):
            at = int(pix[b, p])
            if at >= 0:
                key = (int(zbits[b, p]) << 32) | (b * npts + p)
                if key < keys[bf[b]][at]:
                    keys[bf[b]][at] = key
    first_box = [min([b for b in range(nb) if bf[b] >= f] or [nb]) for f in range(nf)]
    depth_maps, instance_maps = [], []
    for f, (h, w) in enumerate(shapes):
        d, inst = np.zeros(h * w, np.uint32), np.full(h * w, 255, np.uint8)
        for at, key in enumerate(keys[f]):
            if key != EMPTY_KEY:
                d[at] = key >> 32
                inst[at] = (key & 0xffffffff) // npts - first_box[f]
        depth_maps.append(d.view(np.float32).reshape(h, w))
        instance_maps.append(inst.reshape(h, w))
    images = case.get('images')
    out_xyz, out_rgb, out_box, out_pix = [], [], [], []
    kept, visible = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
    frame_count = np.zeros(nf, np.int64)
    for b in range(nb):
        for p in range(npts):
            at = int(pix[b, p])
            if at < 0:
                continue
            kept[b] += 1
            wins = (keys[bf[b]][at] & 0xffffffff) == b * npts + p
            visible[b] += int(wins)
            if visible_only and not wins:
                continue
            out_xyz.append(xyz[b, p])
            if images is not None:
                out_rgb.append(np.asarray(images[bf[b]], np.float32).reshape(-1, 3)[at])
            out_box.append(b)
            out_pix.append(at)
            frame_count[bf[b]] += 1
    frame_offset = np.zeros(nf + 1, np.int64)
    frame_offset[1:] = np.cumsum(frame_count)
    return dict(xyz=np.asarray(out_xyz, np.float32).reshape(-1, 3),
                rgb=None if images is None else np.asarray(out_rgb, np.float32).reshape(-1, 3),
                box=np.asarray(out_box, np.int32), pixel=np.asarray(out_pix, np.int32), frame_offset=frame_offset,
                depth_maps=depth_maps, instance_maps=instance_maps, kept_per_box=kept, visible_per_box=visible)

"""mpsr_scene_score restated in numpy as pure image comparisons: the rendered instance and depth maps of
tests/scene_restatement.py against ground-truth maps.  Nothing here is shared with the kernels or with
monopsr_amd.core.scene_reconstruction.  Written twice: vectorised (`scores`) and as a plain per-box loop (`scores_loop`).

A case is scene_restatement's dict; its ground truth is a dict: instance_images [(h,w) uint8] * F (255 background),
depth_maps [(h,w) float32] * F (0, inf, NaN: no depth), box_gt_id (B,) int (outside [0, 254]: no ground truth).

-> dict: counts (B,6) int64 = kept, on_points, pred_px, inter_px, gt_px, depth_n; sums (B,3) float64 = the sums of
e, |e| and e * e over the depth_n pixels, e = (double) rendered depth - (double) ground-truth depth.
"""
import numpy as np

import scene_restatement

COUNT_NAMES = ('kept', 'on_points', 'pred_px', 'inter_px', 'gt_px', 'depth_n')
METRIC_NAMES = ('scene_mask_iou', 'scene_mask_precision', 'scene_point_precision', 'scene_depth_bias',
                'scene_depth_mae', 'scene_depth_rmse')


def _first_boxes(bf, nf):
    return np.searchsorted(bf, np.arange(nf), side='left')


def scores(case, gt, scene=None, pix=None):
    """Vectorised: per frame, bincounts over the pixels a box wins; per point, one gather of the instance image."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, npts = xyz.shape[:2]
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    nf = len(shapes)
    bf = np.asarray(case['box_frame'], np.int64).reshape(nb)
    gid = np.asarray(gt['box_gt_id'], np.int64).reshape(nb)
    has_gt = (gid >= 0) & (gid <= 254)
    if scene is None:
        scene = scene_restatement.scene(case)
    if pix is None:
        pix = scene_restatement.project(case)
    first = _first_boxes(bf, nf)
    counts = np.zeros((nb, 6), np.int64)
    sums = np.zeros((nb, 3), np.float64)
    if nb == 0:
        return dict(counts=counts, sums=sums)
    # the points: kept, and kept on a pixel of the box's own instance
    offs = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])])
    flat_inst = np.concatenate([np.asarray(gt['instance_images'][f], np.uint8).reshape(-1) for f in range(nf)])
    kept = pix >= 0
    value = flat_inst[np.where(kept, pix + offs[bf][:, None], 0)].astype(np.int64)
    counts[:, 0] = kept.sum(1)
    counts[:, 1] = (kept & has_gt[:, None] & (value == gid[:, None])).sum(1)
    # the pixels: the rendered masks against the true ones
    for f, (h, w) in enumerate(shapes):
        inst = np.asarray(scene['instance_maps'][f]).reshape(-1)
        z = np.asarray(scene['depth_maps'][f], np.float32).reshape(-1)
        true = np.asarray(gt['instance_images'][f], np.uint8).reshape(-1).astype(np.int64)
        d = np.asarray(gt['depth_maps'][f], np.float32).reshape(-1)
        won = inst != 255
        box = first[f] + inst[won].astype(np.int64)
        inter = has_gt[box] & (true[won] == gid[box])
        with np.errstate(invalid='ignore'):
            measured = inter & np.isfinite(d[won]) & (d[won] > 0)
        counts[:, 2] += np.bincount(box, minlength=nb)
        counts[:, 3] += np.bincount(box[inter], minlength=nb)
        counts[:, 5] += np.bincount(box[measured], minlength=nb)
        e = z[won][measured].astype(np.float64) - d[won][measured].astype(np.float64)
        sums[:, 0] += np.bincount(box[measured], weights=e, minlength=nb)
        sums[:, 1] += np.bincount(box[measured], weights=np.abs(e), minlength=nb)
        sums[:, 2] += np.bincount(box[measured], weights=e * e, minlength=nb)
        hist = np.bincount(true, minlength=256)
        of_frame = (bf == f) & has_gt
        counts[of_frame, 4] = hist[gid[of_frame]]
    return dict(counts=counts, sums=sums)


def scores_loop(case, gt, scene=None, pix=None):
    """The same, one box, one pixel and one point at a time with Python-level control flow."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb, npts = xyz.shape[:2]
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    bf = [int(v) for v in np.asarray(case['box_frame']).reshape(nb)]
    if scene is None:
        scene = scene_restatement.scene(case)
    if pix is None:
        pix = scene_restatement.project_loop(case)
    counts = np.zeros((nb, 6), np.int64)
    sums = np.zeros((nb, 3), np.float64)
    for b in range(nb):
        f = bf[b]
        h, w = shapes[f]
        k = b - min(c for c in range(nb) if bf[c] == f)  # the box's ordinal within its frame
        g = int(np.asarray(gt['box_gt_id']).reshape(nb)[b])
        true, d = gt['instance_images'][f], gt['depth_maps'][f]
        rendered, z = scene['instance_maps'][f], scene['depth_maps'][f]
        for p in range(npts):
            at = int(pix[b, p])
            if at >= 0:
                counts[b, 0] += 1
                if 0 <= g <= 254 and int(true[at // w, at % w]) == g:
                    counts[b, 1] += 1
        for r in range(h):
            for c in range(w):
                mine = int(rendered[r, c]) == k and k != 255
                theirs = 0 <= g <= 254 and int(true[r, c]) == g
                counts[b, 2] += int(mine)
                counts[b, 4] += int(theirs)
                if mine and theirs:
                    counts[b, 3] += 1
                    depth = np.float32(d[r, c])
                    if np.isfinite(depth) and depth > 0:
                        counts[b, 5] += 1
                        e = np.float64(z[r, c]) - np.float64(depth)
                        sums[b, 0] += e
                        sums[b, 1] += abs(e)
                        sums[b, 2] += e * e
    return dict(counts=counts, sums=sums)


def sum_bounds(case, gt, scene=None, terms=2304):
    """(B,3): terms * 2^-53 * sum |term| of each of the three sums, the worst-case difference of two summation orders
    of that many fp64 terms."""
    xyz = np.asarray(case['xyz'], np.float32)
    nb = xyz.shape[0]
    got = scores(case, gt, scene)
    # sum |e| is itself the sum of the absolute terms of the first two; the squares are their own absolute values
    mag = np.stack([got['sums'][:, 1], got['sums'][:, 1], got['sums'][:, 2]], 1).reshape(nb, 3)
    return terms * 2.0 ** -53 * mag * (1.0 + terms * 2.0 ** -53)


def table(counts, sums, box_gt_id):
    """The (B,6) float32 metric table in METRIC_NAMES order: fp64 quotients rounded once; NaN where there is none."""
    c = np.asarray(counts, np.float64)
    s = np.asarray(sums, np.float64)
    gid = np.asarray(box_gt_id, np.int64).reshape(-1)
    out = np.full((len(c), 6), np.nan, np.float64)
    for b in range(len(c)):
        kept, on_points, pred_px, inter_px, gt_px, depth_n = c[b]
        union = pred_px + gt_px - inter_px
        if 0 <= gid[b] <= 254 and union > 0:
            out[b, 0] = inter_px / union
        if pred_px > 0:
            out[b, 1] = inter_px / pred_px
        if kept > 0:
            out[b, 2] = on_points / kept
        if depth_n > 0:
            out[b, 3] = s[b, 0] / depth_n
            out[b, 4] = s[b, 1] / depth_n
            out[b, 5] = np.sqrt(s[b, 2] / depth_n)
    return out.astype(np.float32)


def stats(values):
    """count, mean, np.std, mean |x|, std |x| per column of a float32 table in fp64, NaN entries left out one by one.
    -> (n_cols, 5) float64 (NaN where a column has no entry)."""
    v = np.asarray(values, np.float32).astype(np.float64)
    out = np.full((v.shape[1], 5), np.nan)
    for k in range(v.shape[1]):
        x = v[:, k][~np.isnan(v[:, k])]
        out[k, 0] = len(x)
        if len(x):
            out[k, 1:] = [x.mean(), x.std(), np.abs(x).mean(), np.abs(x).std()]
    return out

"""KITTI object evaluation on the GPU: 2D, orientation (AOS), bird's-eye-view and 3D AP at easy / moderate / hard.

Gives the numbers of the reference's native evaluator (scripts/offline_eval/kitti_native_eval/
evaluate_object_3d_offline.cpp and its _low_iou twin, which differ only in MIN_OVERLAP, :55) for the same label files.
The per-pair overlaps, the matching of detections to ground truth and the per-threshold statistics run as HIP kernels
in fp64 (csrc/kitti_eval.hip); the host parses labels, picks the score thresholds (getThresholds, :347-380) and turns
the summed statistics into the 41-point curves and the AP the program prints (:707-772).

    result = evaluate(gt_frames, det_frames)              # parsed frames (parse_label_file)
    result = evaluate_dirs(gt_label_dir, result_dir)      # like the C++ program: frames with a file in result_dir/data
    result = evaluate_predictions(predictions, classes, score_threshold, gt_label_dir)  # format_predictions output
    print(format_report(result, step))
    results = evaluate_sliced(gt_frames, det_frames, ious=('standard', 'low'), depth_edges=(10, 20, 30, 40, 50))
    print(format_sliced_report(results, step))            # {(iou, 'all' | depth bin): result}, one pass

result: {class: {'image', 'aos', 'bev', 'heading_bev', '3d', 'heading_3d': {'curve' (3,41), 'ap11' (3,),
'ap40' (3,)}}}, rows easy / moderate / hard, only the entries the reference evaluates.  ap11 is the printed number
(points 0, 4, ..., 40 added into a float32 sum, / 11 * 100); ap40 is the mean of points 1..40 of the same curve, * 100 (the
KITTI server's AP_R40).

Divergences from the C++ program, on purpose:
  * frames are taken in the order of their index; the program takes readdir order, which changes only the order in
    which the fp64 similarities of frames are summed;
  * a row that does not parse raises (ValueError); fscanf skips it;
  * a box with non-positive l or w (BEV), or l, w or h (3D), overlaps nothing; boost's result is undefined there.
  Kept from it: a threshold at which tp + fp == 0 gives the precision 0.0 / 0.0, a NaN that the report prints as
  '-nan', as glibc prints x86's default NaN.  Empty label files are frames without objects.  Not reproduced: the plots, the stats_*.txt files and the mail.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from monopsr_amd import _lib

CLASS_NAMES = ('car', 'pedestrian', 'cyclist')
CLASS_CODES = {'car': 0, 'pedestrian': 1, 'cyclist': 2, 'van': 3, 'person_sitting': 4, 'dontcare': 5}
OTHER = 6
FIELDS = 14  # MPSR_KITTI_FIELDS: x1 y1 x2 y2 alpha h w l tx ty tz ry score|truncation occlusion
X1, Y1, X2, Y2, ALPHA, H, W, L, TX, TY, TZ, RY, SCORE, OCCLUSION = range(FIELDS)
TRUNCATION = SCORE
N_POINTS = 41
N_CONFIGS = 27  # (metric * 3 + class) * 3 + difficulty
METRICS = ('image', 'bev', '3d')
MIN_OVERLAP = {'standard': (0.7, 0.5, 0.5), 'low': (0.5, 0.25, 0.25)}  # per class, the same for every metric (:55)
MAX_DETECTIONS_PER_FRAME = 8192  # MPSR_KITTI_MAX_FRAME_DETECTIONS: more in one frame is an InvalidArgumentError


class Frame(object):
    """The objects of one label file: codes (n,) int32 (CLASS_CODES, OTHER for any other name) and rows (n, FIELDS)
    float64 in the kernels' column order."""
    __slots__ = ('codes', 'rows')

    def __init__(self, codes, rows):
        self.codes = np.ascontiguousarray(codes, np.int32).reshape(-1)
        self.rows = np.ascontiguousarray(rows, np.float64).reshape(-1, FIELDS)
        if len(self.codes) != len(self.rows):
            raise ValueError('Frame: %d class codes for %d rows' % (len(self.codes), len(self.rows)))

    def __len__(self):
        return len(self.codes)


def class_code(name):
    return CLASS_CODES.get(name.lower(), OTHER)


def parse_labels(text, detections):
    """KITTI label text -> Frame.  Ground truth: 15 columns (type truncation occlusion alpha x1 y1 x2 y2 h w l x y z
    ry), detections: 16 (the same, then score).  Class names compare case-insensitively; CRLF and empty text are
    fine; a row with another column count or a value that is not a number raises ValueError."""
    width = 16 if detections else 15
    codes, rows = [], []
    for k, line in enumerate(text.splitlines()):
        tok = line.split()
        if not tok:
            continue
        if len(tok) != width:
            raise ValueError('label line %d has %d columns, expected %d: %r' % (k + 1, len(tok), width, line))
        v = [float(t) for t in tok[3:]]
        row = [v[1], v[2], v[3], v[4], v[0], v[5], v[6], v[7], v[8], v[9], v[10], v[11], 0.0, 0.0]
        if detections:
            row[SCORE] = v[12]
        else:
            row[TRUNCATION] = float(tok[1])
            row[OCCLUSION] = int(tok[2])  # %d (:191)
        codes.append(class_code(tok[0]))
        rows.append(row)
    return Frame(np.array(codes, np.int32), np.array(rows, np.float64).reshape(-1, FIELDS))


def parse_label_file(path, detections):
    with open(path, 'r', newline='') as f:
        return parse_labels(f.read(), detections)


def get_thresholds(scores, n_groundtruth):
    """getThresholds (:347-380): the scores at which recall reaches the 41 sample points."""
    v = np.sort(np.asarray(scores, np.float64))[::-1]
    n_gt = float(n_groundtruth)
    t = []
    current_recall = 0.0
    n = len(v)
    for i in range(n):
        l_recall = (i + 1) / n_gt if n_gt else np.inf
        r_recall = ((i + 2) / n_gt if n_gt else np.inf) if i < n - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < n - 1:
            continue
        t.append(v[i])
        current_recall += 1.0 / (N_POINTS - 1.0)
    return np.array(t, np.float64)


def _max_from_right(vals, n):
    """precision[i] = *max_element(precision.begin() + i, end) for i < n (:732-738), with max_element's comparisons
    (a NaN is replaced only by a later element that compares greater)."""
    out = list(vals)
    for i in range(n):
        best = out[i]
        for x in out[i + 1:]:
            if best < x:
                best = x
        out[i] = best
    return np.array(out, np.float64)


def ap11(curve):
    """printAp (:745-752), per row: `float sum; sum += vals[i]` over points 0, 4, ..., 40 -- each point is added to
    the float sum in double and the result rounded to float once -- then sum / 11 * 100 in float."""
    out = []
    for row in np.asarray(curve, np.float64).reshape(-1, N_POINTS):
        s = np.float32(0)
        for i in range(0, N_POINTS, 4):
            s = np.float32(np.float64(s) + row[i])
        out.append(float(np.float32(np.float32(s / np.float32(11)) * np.float32(100))))
    return np.array(out)


def c_printf_f(v):
    """printf("%f", v) of glibc: as Python's '%f', except that a NaN prints with its sign.  A threshold at which
    tp + fp == 0 gives precision 0.0 / 0.0, a NaN with the sign bit set on x86, which the C program prints as
    '-nan' (and numpy's division gives the same NaN)."""
    v = float(v)
    if v != v:
        return '-nan' if np.signbit(v) else 'nan'
    return '%f' % v


def ap40(curve):
    """AP_R40: the mean of points 1..40, * 100, per row."""
    return np.asarray(curve, np.float64).reshape(-1, N_POINTS)[:, 1:].mean(axis=1) * 100.0


def _eval_flags(dets):
    """loadDetections (:156-171): per class, which metrics are evaluated; compute_aos over all detections."""
    ev = np.zeros((3, 3), bool)  # [metric][class]
    compute_aos = True
    for fr in dets:
        r = fr.rows
        if len(r) and (r[:, ALPHA] == -10).any():
            compute_aos = False
        for c in range(3):
            m = fr.codes == c
            if not m.any():
                continue
            rc = r[m]
            ev[0, c] |= bool((rc[:, X1] >= 0).any())
            ground = (rc[:, TX] != -1000) & (rc[:, TZ] != -1000) & (rc[:, W] > 0) & (rc[:, L] > 0)
            ev[1, c] |= bool(ground.any())
            ev[2, c] |= bool((ground & (rc[:, TY] != -1000) & (rc[:, H] > 0)).any())
    return ev, compute_aos


def _host_offsets(frames):
    return np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)


class _Batch(object):
    """One ragged batch on the device (struct mpsr_kitti_batch) and what keeps its memory alive."""

    def __init__(self, gt, dets, device):
        import torch
        if len(gt) != len(dets):
            raise ValueError('evaluate: %d ground-truth frames, %d detection frames' % (len(gt), len(dets)))
        self.nf = len(gt)
        dof, gof = _host_offsets(dets), _host_offsets(gt)
        pof = np.concatenate([[0], np.cumsum([len(d) * len(g) for d, g in zip(dets, gt)])]).astype(np.int64)
        self.dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        det_rows = self.up(np.concatenate([d.rows for d in dets] + [np.zeros((0, FIELDS))]), torch.float64)
        det_cls = self.up(np.concatenate([d.codes for d in dets] + [np.zeros(0, np.int32)]), torch.int32)
        gt_rows = self.up(np.concatenate([g.rows for g in gt] + [np.zeros((0, FIELDS))]), torch.float64)
        gt_cls = self.up(np.concatenate([g.codes for g in gt] + [np.zeros(0, np.int32)]), torch.int32)
        dof_d, gof_d, pof_d = self.up(dof, torch.int32), self.up(gof, torch.int32), self.up(pof, torch.int64)
        self.n_det, self.n_gt, self.n_pairs = int(dof[-1]), int(gof[-1]), int(pof[-1])
        p = _lib.ptr
        with torch.cuda.device(self.dev):
            self.struct = _lib.KittiBatch(p(det_rows), p(det_cls), p(gt_rows), p(gt_cls), p(dof_d), p(gof_d), p(pof_d),
                                          dof.ctypes.data, gof.ctypes.data, pof.ctypes.data, self.n_det, self.n_gt,
                                          self.nf)
        self.keep = (det_rows, det_cls, gt_rows, gt_cls, dof_d, gof_d, pof_d, dof, gof, pof)

    def up(self, a, dt):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev, dt)


def _pick_thresholds(ev, scores, care):
    """getThresholds of the 27 configurations of one slice.  ev (3,3) bool [metric][class]; scores (27, n_gt) with NaN
    where a ground truth has no true positive; care (27, n_frames).  -> ([thresholds per configuration], thr (27,41),
    n_thr (27,))."""
    thresholds = []
    thr = np.zeros((N_CONFIGS, N_POINTS), np.float64)
    n_thr = np.zeros(N_CONFIGS, np.int32)
    for cfg in range(N_CONFIGS):
        metric, cls = cfg // 9, (cfg // 3) % 3
        t = np.zeros(0)
        if ev[metric, cls]:
            v = scores[cfg]
            t = get_thresholds(v[~np.isnan(v)], int(care[cfg].sum()))
            if len(t) > N_POINTS:
                raise RuntimeError('getThresholds gave %d thresholds (> %d)' % (len(t), N_POINTS))
        thresholds.append(t)
        thr[cfg, :len(t)] = t
        n_thr[cfg] = len(t)
    return thresholds, thr, n_thr


def _kernel_pass(gt, dets, iou, device):
    """Overlaps, matching pass, thresholds (host), statistics pass.  Returns (thresholds per configuration, counts
    (27,41,3), similarity (27,41,2), eval flags, compute_aos)."""
    import torch
    if len(gt) != len(dets):
        raise ValueError('evaluate: %d ground-truth frames, %d detection frames' % (len(gt), len(dets)))
    if iou not in MIN_OVERLAP:
        raise ValueError('iou must be one of %s' % sorted(MIN_OVERLAP))
    ev, compute_aos = _eval_flags(dets)
    b = _Batch(gt, dets, device)
    nf, dev, batch = b.nf, b.dev, b.struct
    p = _lib.ptr
    with torch.cuda.device(dev):
        mo = np.array([MIN_OVERLAP[iou]] * 3, np.float64).reshape(9)
        mo_c = mo.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        lib, s = _lib.lib(), _lib.stream()
        overlaps = torch.empty((6, b.n_pairs), dtype=torch.float64, device=dev)
        tp_scores = torch.empty((N_CONFIGS, b.n_gt), dtype=torch.float64, device=dev)
        n_care = torch.empty((N_CONFIGS, nf), dtype=torch.int32, device=dev)
        _lib.check(lib.mpsr_kitti_overlaps(ctypes.byref(batch), p(overlaps), s))
        _lib.check(lib.mpsr_kitti_match(ctypes.byref(batch), p(overlaps), mo_c, p(tp_scores), p(n_care), s))
        scores, care = tp_scores.cpu().numpy(), n_care.cpu().numpy()
        thresholds, thr, n_thr = _pick_thresholds(ev, scores, care)
        n_active = int((n_thr > 0).sum())
        ws = torch.empty(max(1, lib.mpsr_kitti_stats_workspace_bytes(nf, n_active)), dtype=torch.uint8, device=dev)
        thr_d = b.up(thr, torch.float64)
        counts = torch.empty((N_CONFIGS, N_POINTS, 3), dtype=torch.int32, device=dev)
        sims = torch.empty((N_CONFIGS, N_POINTS, 2), dtype=torch.float64, device=dev)
        _lib.check(lib.mpsr_kitti_stats(ctypes.byref(batch), p(overlaps), mo_c, p(thr_d),
                                        n_thr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), int(compute_aos),
                                        p(counts), p(sims), p(ws), ws.numel(), s))
        counts_h, sims_h = counts.cpu().numpy(), sims.cpu().numpy()
    return thresholds, counts_h, sims_h, ev, compute_aos


def _curves(n_thr, counts, sims, aos, heading):
    """eval_class :707-738 for one configuration: precision, AOS and heading curves (41 points each)."""
    tp, fp = counts[:, 0].astype(np.float64), counts[:, 1].astype(np.float64)
    prec, a, h = np.zeros(N_POINTS), np.zeros(N_POINTS), np.zeros(N_POINTS)
    with np.errstate(invalid='ignore', divide='ignore'):
        prec[:n_thr] = tp[:n_thr] / (tp[:n_thr] + fp[:n_thr])
        a[:n_thr] = sims[:n_thr, 0] / (tp[:n_thr] + fp[:n_thr])
        h[:n_thr] = sims[:n_thr, 1] / (tp[:n_thr] + fp[:n_thr])
    return (_max_from_right(prec, n_thr), _max_from_right(a, n_thr) if aos else None,
            _max_from_right(h, n_thr) if heading else None)


def _entry(rows):
    curve = np.stack(rows)
    return {'curve': curve, 'ap11': ap11(curve), 'ap40': ap40(curve)}


def _result(thresholds, counts, sims, ev, compute_aos):
    """The nested result dict of one evaluation (one slice) from its 27 configurations' summed statistics."""
    result = {}
    for metric in range(3):
        for cls in range(3):
            if not ev[metric, cls]:
                continue
            prec, aos, head = [], [], []
            for diff in range(3):
                cfg = (metric * 3 + cls) * 3 + diff
                p, a, h = _curves(len(thresholds[cfg]), counts[cfg], sims[cfg], metric == 0 and compute_aos,
                                  metric != 0)
                prec.append(p)
                aos.append(a)
                head.append(h)
            out = result.setdefault(CLASS_NAMES[cls], {})
            name = METRICS[metric]
            out[name] = _entry(prec)
            if metric == 0 and compute_aos:
                out['aos'] = _entry(aos)
            if metric != 0:
                out['heading_' + name] = _entry(head)
    return result


def evaluate(gt, detections, iou='standard', device=None):
    """gt, detections: lists of Frame (one per image, in the same order).  iou: 'standard' (MIN_OVERLAP 0.7 / 0.5 /
    0.5) or 'low' (0.5 / 0.25 / 0.25).  Returns the nested result dict described in the module docstring."""
    return _result(*_kernel_pass(gt, detections, iou, device))


MAX_SLICES = 32  # MPSR_KITTI_MAX_SLICES
MAX_EDGES = 15   # evaluator_utils.MAX_EDGES: mpsr_object_pairs' depth axis


def slice_table(ious=('standard',), depth_edges=()):
    """The slices of evaluate_sliced, in its key order: [((iou, bin label), lo, hi)], lo = hi = None for 'all'.  Raises
    ValueError for duplicate or unknown ious, edges that do not increase, are not finite or number more than MAX_EDGES,
    and for more than MAX_SLICES slices.  Touches no device."""
    from monopsr_amd.core import evaluator_utils as eu
    ious = [ious] if isinstance(ious, str) else list(ious)
    if not ious:
        raise ValueError('evaluate_sliced: no iou set given')
    for iou in ious:
        if iou not in MIN_OVERLAP:
            raise ValueError('evaluate_sliced: iou %r is not one of %s' % (iou, sorted(MIN_OVERLAP)))
    if len(set(ious)) != len(ious):
        raise ValueError('evaluate_sliced: duplicate iou sets in %r' % (ious,))
    edges = [float(e) for e in depth_edges]
    if len(edges) > MAX_EDGES:
        raise ValueError('evaluate_sliced: %d depth edges, at most %d' % (len(edges), MAX_EDGES))
    if not all(np.isfinite(e) for e in edges):
        raise ValueError('evaluate_sliced: depth edges must be finite, got %r' % (edges,))
    if any(b <= a for a, b in zip(edges[:-1], edges[1:])):
        raise ValueError('evaluate_sliced: depth edges must increase, got %r' % (edges,))
    bins = []
    if edges:
        bounds = [-np.inf] + edges + [np.inf]
        labels = eu.edge_labels(edges)
        if len(set(labels)) != len(labels):
            raise ValueError('evaluate_sliced: depth edges %r give the same bin label twice: %r' % (edges, labels))
        bins = list(zip(labels, bounds[:-1], bounds[1:]))
    n = len(ious) * (1 + len(bins))
    if n > MAX_SLICES:
        raise ValueError('evaluate_sliced: %d iou sets x (all + %d bins) = %d slices, at most %d'
                         % (len(ious), len(bins), n, MAX_SLICES))
    out = []
    for iou in ious:
        out.append(((iou, 'all'), None, None))
        out.extend(((iou, label), lo, hi) for label, lo, hi in bins)
    return out


def _in_bin(frames, lo, hi):
    """The detections of each frame whose own z lies in lo <= z < hi (a NaN z lies in no bin)."""
    out = []
    for fr in frames:
        z = fr.rows[:, TZ]
        m = (z >= lo) & (z < hi)
        out.append(Frame(fr.codes[m], fr.rows[m]))
    return out


def evaluate_sliced(gt, detections, ious=('standard',), depth_edges=(), device=None):
    """AP of every slice in one pass.  A slice is an IoU set of `ious` and either every row
    ('all': the bits of evaluate(gt, detections, iou)) or one of the len(depth_edges) + 1 depth bins that increasing
    edges cut (evaluator_utils.edge_labels; a row with lo <= z < hi is in the bin, so an edge belongs to the upper bin,
    a NaN z to none and a 2-D-only detection's z = -1000 to the first).  A bin's AP is what the C++ program prints after
    every ground truth whose z is outside the bin has got occlusion 3 and every detection whose own z is outside it the
    class Misc; the eval flags (which metrics a class has) come from the bin's own detections, compute_aos from all.
    -> {(iou, bin label): result of evaluate's form}, ordered by ious, then 'all', then the bins.
    One batch upload, one mpsr_kitti_overlaps launch, one matching launch, getThresholds per configuration on the
    host, one statistics launch and one copy back."""
    import torch
    table = slice_table(ious, depth_edges)
    if len(gt) != len(detections):
        raise ValueError('evaluate: %d ground-truth frames, %d detection frames' % (len(gt), len(detections)))
    n_slices = len(table)
    _, compute_aos = _eval_flags(detections)
    flags = {}  # per bin, shared by the IoU sets
    for (_, label), lo, hi in table:
        if label not in flags:
            flags[label] = _eval_flags(detections if lo is None else _in_bin(detections, lo, hi))[0]
    slices_h = (_lib.KittiSlice * n_slices)()
    for k, ((iou, _), lo, hi) in enumerate(table):
        slices_h[k].min_overlap[:] = list(MIN_OVERLAP[iou]) * 3
        slices_h[k].depth_tested = int(lo is not None)
        slices_h[k].lo, slices_h[k].hi = (0.0, 0.0) if lo is None else (lo, hi)
    b = _Batch(gt, detections, device)
    nf, dev, batch = b.nf, b.dev, b.struct
    n_total = n_slices * N_CONFIGS
    p = _lib.ptr
    with torch.cuda.device(dev):
        lib, s = _lib.lib(), _lib.stream()
        slices_d = b.up(np.frombuffer(slices_h, np.uint8), torch.uint8)
        overlaps = torch.empty((6, b.n_pairs), dtype=torch.float64, device=dev)
        tp_scores = torch.empty((n_total, b.n_gt), dtype=torch.float64, device=dev)
        n_care = torch.empty((n_total, nf), dtype=torch.int32, device=dev)
        _lib.check(lib.mpsr_kitti_overlaps(ctypes.byref(batch), p(overlaps), s))
        _lib.check(lib.mpsr_kitti_match_slices(ctypes.byref(batch), p(overlaps), p(slices_d), slices_h, n_slices,
                                               p(tp_scores), p(n_care), s))
        scores, care = tp_scores.cpu().numpy(), n_care.cpu().numpy()
        del tp_scores
        thresholds, thr, n_thr = [], [], []
        for k, ((_, label), _, _) in enumerate(table):
            t, a, n = _pick_thresholds(flags[label], scores[k * N_CONFIGS:(k + 1) * N_CONFIGS],
                                       care[k * N_CONFIGS:(k + 1) * N_CONFIGS])
            thresholds.append(t)
            thr.append(a)
            n_thr.append(n)
        n_thr = np.ascontiguousarray(np.concatenate(n_thr), np.int32)
        n_active = int((n_thr > 0).sum())
        ws = torch.empty(max(1, lib.mpsr_kitti_stats_slices_workspace_bytes(nf, n_active)), dtype=torch.uint8,
                         device=dev)
        thr_d, n_thr_d = b.up(np.concatenate(thr), torch.float64), b.up(n_thr, torch.int32)
        # counts and similarities in one buffer: one copy back
        out = torch.empty(n_total * N_POINTS * (3 * 4 + 2 * 8), dtype=torch.uint8, device=dev)
        sims = out[:n_total * N_POINTS * 16].view(torch.float64)
        counts = out[n_total * N_POINTS * 16:].view(torch.int32)
        _lib.check(lib.mpsr_kitti_stats_slices(ctypes.byref(batch), p(overlaps), p(slices_d), slices_h, n_slices,
                                               p(thr_d), p(n_thr_d), n_thr.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                               int(compute_aos), p(counts), p(sims), p(ws), ws.numel(), s))
        out_h = out.cpu().numpy()
    sims_h = out_h[:n_total * N_POINTS * 16].view(np.float64).reshape(n_slices, N_CONFIGS, N_POINTS, 2)
    counts_h = out_h[n_total * N_POINTS * 16:].view(np.int32).reshape(n_slices, N_CONFIGS, N_POINTS, 3)
    results = {}
    for k, (key, _, _) in enumerate(table):
        results[key] = _result(thresholds[k], counts_h[k], sims_h[k], flags[key[1]], compute_aos)
    return results


def _atoi(s):
    """C atoi: leading blanks, a sign, digits; 0 when there are none."""
    s = s.lstrip(' \t\n\v\f\r')
    k = 1 if s[:1] in ('+', '-') else 0
    e = k
    while e < len(s) and s[e].isdigit():
        e += 1
    return int(s[:e]) if e > k else 0


def frame_index(file_name):
    """getEvalIndices (:825-840): the index of a result file = atoi of its last 10 characters; names shorter than 10
    characters are skipped (None)."""
    return None if len(file_name) < 10 else _atoi(file_name[-10:])


def _frame_indices(names):
    return sorted(i for i in (frame_index(n) for n in names) if i is not None)


def _load_gt(gt_label_dir, indices):
    gt = []
    for idx in indices:
        path = os.path.join(gt_label_dir, '%06d.txt' % idx)
        if not os.path.exists(path):
            raise FileNotFoundError("ground truth of frame %06d is missing: %s" % (idx, path))
        gt.append(parse_label_file(path, detections=False))
    return gt


def _load_dirs(gt_label_dir, result_dir):
    data = os.path.join(result_dir, 'data')
    indices = _frame_indices(os.listdir(data))
    gt = _load_gt(gt_label_dir, indices)
    dets = [parse_label_file(os.path.join(data, '%06d.txt' % idx), detections=True) for idx in indices]
    return gt, dets


def evaluate_dirs(gt_label_dir, result_dir, iou='standard', device=None):
    """The C++ program's inputs: evaluates the frames with a file in result_dir/data/ (index = getEvalIndices') against
    gt_label_dir/<index %06d>.txt.  Raises FileNotFoundError if a frame's ground truth is missing."""
    gt, dets = _load_dirs(gt_label_dir, result_dir)
    return evaluate(gt, dets, iou, device)


def evaluate_dirs_sliced(gt_label_dir, result_dir, ious=('standard',), depth_edges=(), device=None):
    """evaluate_sliced of evaluate_dirs' frames.  The arguments are checked before a file is read."""
    slice_table(ious, depth_edges)
    gt, dets = _load_dirs(gt_label_dir, result_dir)
    return evaluate_sliced(gt, dets, ious, depth_edges, device)


def evaluate_predictions(predictions, classes, score_threshold, gt_label_dir, project_3d_box=False, frame_info=None,
                         iou='standard', device=None):
    """Evaluates format_predictions output {sample name: (box_3d (n,9), box_2d (n,7))} without writing label files:
    exactly the detections export_kitti_labels(predictions, classes, score_threshold, ...) would write (the same score
    filter, rounding to 3 decimals and projection option), one frame per sample name."""
    from monopsr_amd.core import evaluator_utils as eu
    if project_3d_box and frame_info is None:
        raise ValueError('project_3d_box=True needs frame_info(sample_name) -> (cam_p, (image_w, image_h))')
    score_threshold = round(score_threshold, 3)
    by_index = []
    for name in predictions:
        idx = frame_index(name + '.txt')
        if idx is not None:
            by_index.append((idx, name))
    by_index.sort(key=lambda t: t[0])
    dets = []
    for _, name in by_index:
        b3, b2 = predictions[name]
        if not len(b3):
            dets.append(Frame(np.zeros(0, np.int32), np.zeros((0, FIELDS))))
            continue
        boxes, keep = None, None
        if project_3d_box:
            cam_p, size = frame_info(name)
            boxes, keep = eu.project_boxes_3d(np.asarray(b3, np.float64).reshape(-1, 9), cam_p, size)
        cls, v = eu.kitti_label_array(b3, b2, score_threshold, boxes, keep)
        # v: alpha | x1 y1 x2 y2 | h w l | x y z | ry score
        rows = np.column_stack([v[:, 1:5], v[:, 0], v[:, 5:13], np.zeros(len(v))])
        dets.append(Frame([class_code(classes[int(k)]) for k in cls], rows))
    gt = _load_gt(gt_label_dir, [i for i, _ in by_index])
    return evaluate(gt, dets, iou, device)


_REPORT = (('image', '%s_detection'), ('aos', '%s_orientation'), ('bev', '%s_detection_BEV'),
           ('heading_bev', '%s_heading_BEV'), ('3d', '%s_detection_3D'), ('heading_3d', '%s_heading_3D'))


def format_report(result, step=None):
    """The C++ program's stdout (:898-969): the step line (when given), then per metric pass and class
    '<class>_detection AP: e m h', '<class>_orientation', ..._BEV, _heading_BEV, _3D, _heading_3D."""
    lines = [] if step is None else [str(step)]
    for group in (_REPORT[0:2], _REPORT[2:4], _REPORT[4:6]):
        for cls in CLASS_NAMES:
            for key, fmt in group:
                if key in result.get(cls, {}):
                    ap = result[cls][key]['ap11']
                    lines.append('%s AP: %s %s %s' % (fmt % cls, c_printf_f(ap[0]), c_printf_f(ap[1]),
                                                         c_printf_f(ap[2])))
    return '\n'.join(lines) + '\n'


def format_sliced_report(results, step=None):
    """format_report of every slice of evaluate_sliced's result, each under its heading line '== <iou> <bin> =='."""
    return ''.join('== %s %s ==\n%s' % (iou, label, format_report(result, step))
                   for (iou, label), result in results.items())


def build_parser():
    ap = argparse.ArgumentParser(description='KITTI object evaluation on the GPU (the output of '
                                             'evaluate_object_3d_offline)')
    ap.add_argument('gt_dir', help='ground-truth label_2 directory')
    ap.add_argument('result_dir', help='directory holding data/<index>.txt detection files')
    ap.add_argument('--low-iou', action='store_true', help='MIN_OVERLAP 0.5 / 0.25 / 0.25 (the _low_iou program)')
    ap.add_argument('--both-iou', action='store_true',
                    help='both MIN_OVERLAP sets in one pass; the report of each under a heading line')
    ap.add_argument('--depth-edges', type=float, nargs='+', default=None, metavar='M',
                    help='also AP per depth bin: the bins\' edges in metres, increasing (an edge belongs to the bin above)')
    return ap


def parse_args(argv=None):
    """The command line's arguments; --low-iou together with --both-iou and edges evaluate_sliced refuses are argument
    errors."""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.low_iou and args.both_iou:
        ap.error('--low-iou and --both-iou exclude each other')
    args.ious = ('standard', 'low') if args.both_iou else ('low',) if args.low_iou else ('standard',)
    args.sliced = args.both_iou or args.depth_edges is not None
    if args.sliced:
        try:
            slice_table(args.ious, args.depth_edges or ())
        except ValueError as e:
            ap.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)
    # the program prints the result directory's last component (:898-902)
    cut = args.result_dir.rfind('/')
    step = args.result_dir[cut + 1:] if cut >= 0 else None
    if args.sliced:
        results = evaluate_dirs_sliced(args.gt_dir, args.result_dir, args.ious, args.depth_edges or ())
        sys.stdout.write(format_sliced_report(results, step))
        return 0
    result = evaluate_dirs(args.gt_dir, args.result_dir, args.ious[0])
    sys.stdout.write(format_report(result, step))
    return 0


if __name__ == '__main__':
    sys.exit(main())

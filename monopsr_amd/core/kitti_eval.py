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


def _kernel_pass(gt, dets, iou, device):
    """Overlaps, matching pass, thresholds (host), statistics pass.  Returns (thresholds per configuration, counts
    (27,41,3), similarity (27,41,2), eval flags, compute_aos)."""
    import torch
    if len(gt) != len(dets):
        raise ValueError('evaluate: %d ground-truth frames, %d detection frames' % (len(gt), len(dets)))
    if iou not in MIN_OVERLAP:
        raise ValueError('iou must be one of %s' % sorted(MIN_OVERLAP))
    ev, compute_aos = _eval_flags(dets)
    nf = len(gt)
    dof, gof = _host_offsets(dets), _host_offsets(gt)
    pof = np.concatenate([[0], np.cumsum([len(d) * len(g) for d, g in zip(dets, gt)])]).astype(np.int64)
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)

    def up(a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)

    det_rows = up(np.concatenate([d.rows for d in dets] + [np.zeros((0, FIELDS))]), torch.float64)
    det_cls = up(np.concatenate([d.codes for d in dets] + [np.zeros(0, np.int32)]), torch.int32)
    gt_rows = up(np.concatenate([g.rows for g in gt] + [np.zeros((0, FIELDS))]), torch.float64)
    gt_cls = up(np.concatenate([g.codes for g in gt] + [np.zeros(0, np.int32)]), torch.int32)
    dof_d, gof_d, pof_d = up(dof, torch.int32), up(gof, torch.int32), up(pof, torch.int64)
    n_det, n_gt, n_pairs = int(dof[-1]), int(gof[-1]), int(pof[-1])
    p = _lib.ptr
    with torch.cuda.device(dev):
        batch = _lib.KittiBatch(p(det_rows), p(det_cls), p(gt_rows), p(gt_cls), p(dof_d), p(gof_d), p(pof_d),
                                dof.ctypes.data, gof.ctypes.data, pof.ctypes.data, n_det, n_gt, nf)
        mo = np.array([MIN_OVERLAP[iou]] * 3, np.float64).reshape(9)
        mo_c = mo.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        lib, s = _lib.lib(), _lib.stream()
        overlaps = torch.empty((6, n_pairs), dtype=torch.float64, device=dev)
        tp_scores = torch.empty((N_CONFIGS, n_gt), dtype=torch.float64, device=dev)
        n_care = torch.empty((N_CONFIGS, nf), dtype=torch.int32, device=dev)
        _lib.check(lib.mpsr_kitti_overlaps(ctypes.byref(batch), p(overlaps), s))
        _lib.check(lib.mpsr_kitti_match(ctypes.byref(batch), p(overlaps), mo_c, p(tp_scores), p(n_care), s))
        scores, care = tp_scores.cpu().numpy(), n_care.cpu().numpy()
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
        n_active = int((n_thr > 0).sum())
        ws = torch.empty(max(1, lib.mpsr_kitti_stats_workspace_bytes(nf, n_active)), dtype=torch.uint8, device=dev)
        thr_d = up(thr, torch.float64)
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


def evaluate(gt, detections, iou='standard', device=None):
    """gt, detections: lists of Frame (one per image, in the same order).  iou: 'standard' (MIN_OVERLAP 0.7 / 0.5 /
    0.5) or 'low' (0.5 / 0.25 / 0.25).  Returns the nested result dict described in the module docstring."""
    thresholds, counts, sims, ev, compute_aos = _kernel_pass(gt, detections, iou, device)
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


def evaluate_dirs(gt_label_dir, result_dir, iou='standard', device=None):
    """The C++ program's inputs: evaluates the frames with a file in result_dir/data/ (index = getEvalIndices') against
    gt_label_dir/<index %06d>.txt.  Raises FileNotFoundError if a frame's ground truth is missing."""
    data = os.path.join(result_dir, 'data')
    indices = _frame_indices(os.listdir(data))
    gt = _load_gt(gt_label_dir, indices)
    dets = [parse_label_file(os.path.join(data, '%06d.txt' % idx), detections=True) for idx in indices]
    return evaluate(gt, dets, iou, device)


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


def main(argv=None):
    ap = argparse.ArgumentParser(description='KITTI object evaluation on the GPU (the output of '
                                             'evaluate_object_3d_offline)')
    ap.add_argument('gt_dir', help='ground-truth label_2 directory')
    ap.add_argument('result_dir', help='directory holding data/<index>.txt detection files')
    ap.add_argument('--low-iou', action='store_true', help='MIN_OVERLAP 0.5 / 0.25 / 0.25 (the _low_iou program)')
    args = ap.parse_args(argv)
    result = evaluate_dirs(args.gt_dir, args.result_dir, 'low' if args.low_iou else 'standard')
    # the program prints the result directory's last component (:898-902)
    cut = args.result_dir.rfind('/')
    sys.stdout.write(format_report(result, args.result_dir[cut + 1:] if cut >= 0 else None))
    return 0


if __name__ == '__main__':
    sys.exit(main())

"""KITTI label-file export of the detections `MonoPSRModel.format_predictions` produces.

Replaces `save_predictions_box_3d_in_kitti_format` of the reference (core/evaluator_utils.py:114-277): same call
signature, same output tree (`<base>/kitti_predictions_3d/<split>/<threshold>/<step>/data/<sample>.txt`) and the same
file text (16 columns, values rounded to 3 decimals, truncation / occlusion -1, CRLF line ends, empty file for a frame
without detections).  Built differently: the conversion is a pure function over the in-memory (n,9) / (n,7) arrays
(`kitti_label_rows`), so predictions can be exported straight from `format_predictions` output with
`export_kitti_labels` -- no detour through the '%0.5f' text files -- and the file-based entry point is a thin reader
in front of it.  `project_3d_box=True` (2-D box = clipped projection of the 3-D box, box_3d_projector.py:14-95) is
vectorised over the boxes of a frame; it needs the frame's P2 matrix and image size, which the caller supplies
(`frame_info`) because this package has no dataset reader.

The native KITTI evaluator the reference compiles and runs (evaluator_utils.py:457-560) is replaced by
`monopsr_amd.core.kitti_eval`, which computes the same AP on the GPU from these label files (`evaluate_dirs`) or
straight from format_predictions output (`evaluate_predictions`, through `kitti_label_array`).

The metrics CSVs of the reference's save_metrics (evaluator_utils.py:280-403) are written by `save_metric_stats` from
the statistics `metric_stats` (one mpsr_metric_stats launch) takes of the evaluator's device-resident table.  The
TensorBoard summaries (evaluator_utils.py:376-456) are out of scope.

`object_pairs` (one mpsr_object_pairs launch) sets each predicted box against its own label, `metric_stats_binned` (one
mpsr_metric_stats_binned launch) takes the statistics of a per-object table over all rows and per bin of up to four
axes, and `save_breakdown` writes them in long format.
"""
import csv
import os

import numpy as np

# box_3d row: x y z l w h ry score class   |   box_2d row: y1 x1 y2 x2 alpha score class
_X, _L, _W, _H, _RY, _SCORE, _CLS = 0, 3, 4, 5, 6, 7, 8


def project_boxes_3d(boxes_3d, cam_p, image_size, max_fraction=0.8):
    """Image-space bounding boxes [x1, y1, x2, y2] of 3-D boxes (n,7+) [x, y, z, l, w, h, ry] (y = bottom face),
    clipped to the image; `keep` marks the boxes the reference would keep: at least partly inside the image and,
    before clipping, not wider / taller than `max_fraction` of it, with a clipped extent that is not degenerate.
    Returns (boxes (n,4), keep (n,) bool)."""
    b = np.asarray(boxes_3d, np.float64).reshape(-1, boxes_3d.shape[-1])
    n = b.shape[0]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1]) * 0.5
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1]) * 0.5
    sy = np.array([0, 0, 0, 0, -1, -1, -1, -1.0])
    cx, cy, cz = b[:, _L, None] * sx, b[:, _H, None] * sy, b[:, _W, None] * sz  # (n,8) box frame
    c, s = np.cos(b[:, _RY, None]), np.sin(b[:, _RY, None])
    pts = np.stack([c * cx + s * cz + b[:, 0, None], cy + b[:, 1, None], -s * cx + c * cz + b[:, 2, None],
                    np.ones((n, 8))], axis=1)  # (n,4,8) camera frame, homogeneous
    uvw = np.einsum('ij,njk->nik', np.asarray(cam_p, np.float64).reshape(3, 4), pts)
    u, v = uvw[:, 0] / uvw[:, 2], uvw[:, 1] / uvw[:, 2]
    raw = np.stack([u.min(1), v.min(1), u.max(1), v.max(1)], axis=1)
    w_img, h_img = float(image_size[0]), float(image_size[1])
    inside = (raw[:, 0] <= w_img) & (raw[:, 1] <= h_img) & (raw[:, 2] >= 0) & (raw[:, 3] >= 0)
    small = ((raw[:, 2] - raw[:, 0]) <= max_fraction * w_img) & ((raw[:, 3] - raw[:, 1]) <= max_fraction * h_img)
    clipped = np.stack([np.clip(raw[:, 0], 0, None), np.clip(raw[:, 1], 0, None),
                        np.clip(raw[:, 2], None, w_img), np.clip(raw[:, 3], None, h_img)], axis=1)
    return clipped, inside & small


def kitti_label_array(box_3d, box_2d, score_threshold, image_boxes=None, keep=None):
    """The numbers of the label lines `kitti_label_rows` writes, before they become text: (class index (m,) int,
    values (m,12) float64 rounded to 3 decimals: alpha | x1 y1 x2 y2 | h w l | x y z | ry score)."""
    box_3d = np.asarray(box_3d, np.float64).reshape(-1, 9)
    box_2d = np.asarray(box_2d, np.float64).reshape(-1, 7)
    sel = box_3d[:, _SCORE] >= score_threshold
    if keep is not None:
        sel &= np.asarray(keep, bool)
    b3, b2 = box_3d[sel], box_2d[sel]
    xyxy = b2[:, [1, 0, 3, 2]] if image_boxes is None else np.asarray(image_boxes, np.float64)[sel]
    numbers = np.round(np.column_stack([b2[:, 4], xyxy, b3[:, [_H, _W, _L]], b3[:, _X:_X + 3],
                                        b3[:, [_RY, _SCORE]]]), 3)
    return b3[:, _CLS].astype(np.int64), numbers


def detection_rows(box_3d, box_2d, score_threshold, frame=None, p2=None, image_wh=None, project_3d_box=False):
    """kitti_label_array (and project_boxes_3d when project_3d_box) of device-resident predictions in one
    mpsr_kitti_detection_rows launch, without a copy to the host.  box_3d (n,9), box_2d (n,7) float32 CUDA tensors as
    format_boxes leaves them; frame (n,) int32, p2 (F,12) float64 and image_wh (F,2) int32 [width, height] are needed
    for the projection only.  -> (rows (n,14) float64 in kitti_eval's column order, rounded to 3 decimals; class index
    (n,) int32; keep (n,) int32) on the device, for ALL n rows: the caller compacts with keep."""
    import torch
    from monopsr_amd import _lib
    n, dev = int(box_3d.shape[0]), box_3d.device
    if tuple(box_3d.shape) != (n, 9) or tuple(box_2d.shape) != (n, 7) or box_3d.dtype != torch.float32 \
            or box_2d.dtype != torch.float32:
        raise ValueError('detection_rows: box_3d (n,9) and box_2d (n,7) float32, got %s %s and %s %s' % (
            tuple(box_3d.shape), box_3d.dtype, tuple(box_2d.shape), box_2d.dtype))
    n_frames = 0
    if project_3d_box:
        if frame is None or p2 is None or image_wh is None:
            raise ValueError('project_3d_box=True needs frame, p2 and image_wh')
        n_frames = int(p2.shape[0])
        if frame.dtype != torch.int32 or p2.dtype != torch.float64 or image_wh.dtype != torch.int32 \
                or frame.numel() != n or p2.numel() != 12 * n_frames or image_wh.numel() != 2 * n_frames:
            raise ValueError('detection_rows: frame (n,) int32, p2 (F,12) float64, image_wh (F,2) int32')
    with torch.cuda.device(dev):
        rows = torch.empty((n, 14), dtype=torch.float64, device=dev)
        ints = torch.empty((2, n), dtype=torch.int32, device=dev)
        p = _lib.ptr
        _lib.check(_lib.lib().mpsr_kitti_detection_rows(
            p(box_3d), p(box_2d), p(frame) if project_3d_box else None, p(p2) if project_3d_box else None,
            p(image_wh) if project_3d_box else None, n, n_frames, float(score_threshold), int(bool(project_3d_box)),
            p(rows), p(ints[0]), p(ints[1]), _lib.stream()))
    return rows, ints[0], ints[1]


NAN_RULE_ENTRY, NAN_RULE_FRAME = 0, 1
STAT_NAMES = ('count', 'mean', 'std', 'mean_abs', 'std_abs', 'dropped')


def metric_stats(values, frame, column_metric, n_metrics, n_frames, nan_rule=NAN_RULE_FRAME, out=None):
    """count, mean, np.std, mean |x|, std |x| and the number of dropped values per metric, in fp64, of a device-resident
    table in one mpsr_metric_stats launch.  values (n_rows, n_cols) float32 and frame (n_rows) int32 in [0, n_frames)
    CUDA tensors; column_metric: n_cols ints, the metric each column feeds (several columns may feed one).
    nan_rule NAN_RULE_FRAME: a NaN drops its frame's values of that metric (the reference's rule); NAN_RULE_ENTRY: the
    NaN entries alone.  -> (n_metrics, 6) float64 on the device, columns STAT_NAMES; `out` is written when given."""
    import torch
    from monopsr_amd import _lib
    import ctypes
    column_metric = [int(c) for c in column_metric]
    n_rows, n_cols = (int(v) for v in values.shape) if values.dim() == 2 else (-1, -1)
    if values.dtype != torch.float32 or n_cols != len(column_metric) or frame.dtype != torch.int32 \
            or frame.numel() != n_rows:
        raise ValueError('metric_stats: values (n_rows, %d) float32 and frame (n_rows,) int32, got %s %s and %s %s' % (
            len(column_metric), tuple(values.shape), values.dtype, tuple(frame.shape), frame.dtype))
    dev = values.device
    _lib.ptr(values), _lib.ptr(frame)  # (refuses tensors that are not on the GPU)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty((int(n_metrics), 6), dtype=torch.float64, device=dev)
        elif tuple(out.shape) != (int(n_metrics), 6) or out.dtype != torch.float64:
            raise ValueError('metric_stats: out must be (%d, 6) float64' % int(n_metrics))
        flags = None
        if nan_rule == NAN_RULE_FRAME:
            flags = torch.empty((max(int(n_metrics) * int(n_frames), 1),), dtype=torch.int32, device=dev)
        p = _lib.ptr
        _lib.check(_lib.lib().mpsr_metric_stats(
            p(values), p(frame), n_rows, n_cols, (ctypes.c_int * max(n_cols, 1))(*column_metric), int(n_metrics),
            int(n_frames), int(nan_rule), p(flags), p(out), _lib.stream()))
    return out


def metric_stats_dict(names, stats):
    """{metric name: {count, mean, std, mean_abs, std_abs, dropped}} of a host copy of metric_stats' output."""
    return {name: dict(zip(STAT_NAMES, (int(row[0]), float(row[1]), float(row[2]), float(row[3]), float(row[4]),
                                        int(row[5])))) for name, row in zip(names, stats)}


# mpsr_object_pairs' table columns, the axes of its bins and the difficulty axis' labels (KITTI's levels, then the rest)
PAIR_COLUMNS = ('iou_2d_fed', 'iou_bev', 'iou_3d', 'centre_dist', 'hit3d_70', 'hit3d_50', 'hit3d_25', 'hitbev_70',
                'hitbev_50')
BREAKDOWN_AXES = ('depth', 'difficulty', 'fed_box')
DIFFICULTY_LABELS = ('easy', 'moderate', 'hard', 'beyond')
DEFAULT_DEPTH_EDGES = (10.0, 20.0, 30.0, 40.0, 50.0)
DEFAULT_BOX_IOU_EDGES = (0.7, 0.8, 0.9)
MAX_EDGES, MAX_AXES, MAX_BINS = 15, 4, 64  # MPSR_OBJECT_PAIRS_MAX_EDGES, MPSR_METRIC_STATS_MAX_AXES / _MAX_BINS


def edge_labels(edges):
    """The labels of the len(edges) + 1 bins that increasing edges cut: '<10', '10-20', ..., '>=50' ('all' for none)."""
    e = ['%g' % float(v) for v in edges]
    if not e:
        return ['all']
    return ['<' + e[0]] + ['%s-%s' % (a, b) for a, b in zip(e[:-1], e[1:])] + ['>=' + e[-1]]


def object_pairs(pred_box_3d, gt_box_3d, fed_box_2d=None, label_info=None, depth_edges=DEFAULT_DEPTH_EDGES,
                 box_iou_edges=DEFAULT_BOX_IOU_EDGES):
    """Each predicted box against its own label in one mpsr_object_pairs launch (include/monopsr_hip.h).  pred_box_3d and
    gt_box_3d (n, 7) [x y z l w h ry] float32 CUDA tensors (more columns, as format_boxes' (n, 9), are cut off);
    fed_box_2d (n, 4) [y1 x1 y2 x2] and label_info (n, 6) [truncation, occlusion, x1, y1, x2, y2] float32, or None.
    -> (table (n, 9) float32 in PAIR_COLUMNS' order, overlaps (n, 4) float64: its first four columns unrounded,
    bins (n, 3) int32 in BREAKDOWN_AXES' order) on the device."""
    import ctypes
    import torch
    from monopsr_amd import _lib
    n = int(pred_box_3d.shape[0]) if pred_box_3d.dim() == 2 else -1

    given = (('pred_box_3d', pred_box_3d, 7), ('gt_box_3d', gt_box_3d, 7), ('fed_box_2d', fed_box_2d, 4),
             ('label_info', label_info, 6))
    for name, t, width in given:
        if t is not None and (t.dim() != 2 or int(t.shape[0]) != n or t.dtype != torch.float32 or
                              (int(t.shape[1]) < width if width == 7 else int(t.shape[1]) != width)):
            raise ValueError('object_pairs: %s must be (%d, %d) float32, got %s %s' % (name, n, width, tuple(t.shape),
                                                                                      t.dtype))
    for name, t, width in given:
        _lib.ptr(None if t is None else t[0:0])  # (refuses tensors that are not on the GPU)
    pred, gt, fed, info = (None if t is None else t[:, 0:width].contiguous() for _, t, width in given)
    de, ie = [float(v) for v in depth_edges], [float(v) for v in box_iou_edges]
    dev = pred.device
    with torch.cuda.device(dev):
        table = torch.empty((n, 9), dtype=torch.float32, device=dev)
        overlaps = torch.empty((n, 4), dtype=torch.float64, device=dev)
        bins = torch.empty((n, 3), dtype=torch.int32, device=dev)
        p = _lib.ptr
        _lib.check(_lib.lib().mpsr_object_pairs(
            p(pred), p(gt), p(fed), p(info), n, (ctypes.c_double * max(len(de), 1))(*de), len(de),
            (ctypes.c_double * max(len(ie), 1))(*ie), len(ie), p(overlaps), p(table), p(bins), _lib.stream()))
    return table, overlaps, bins


def metric_stats_binned(values, bins, column_metric, n_metrics, axis_bins, out=None):
    """metric_stats under NAN_RULE_ENTRY of every row and of every bin of every axis in one mpsr_metric_stats_binned
    launch.  values (n_rows, n_cols) float32 and bins (n_rows, n_axes) int32 CUDA tensors; axis_bins: the number of
    bins per axis.  A row whose index on an axis is outside [0, axis_bins[a]) is in none of that axis' bins.
    -> (1 + sum(axis_bins), n_metrics, 6) float64 on the device, columns STAT_NAMES: slot 0 is every row (the bits of
    metric_stats(..., NAN_RULE_ENTRY)), then axis 0's bins, axis 1's, ...; `out` is written when given."""
    import ctypes
    import torch
    from monopsr_amd import _lib
    column_metric, axis_bins = [int(c) for c in column_metric], [int(b) for b in axis_bins]
    n_rows, n_cols = (int(v) for v in values.shape) if values.dim() == 2 else (-1, -1)
    if values.dtype != torch.float32 or n_cols != len(column_metric) or bins.dtype != torch.int32 \
            or tuple(bins.shape) != (n_rows, len(axis_bins)):
        raise ValueError('metric_stats_binned: values (n_rows, %d) float32 and bins (n_rows, %d) int32, got %s %s and '
                         '%s %s' % (len(column_metric), len(axis_bins), tuple(values.shape), values.dtype,
                                    tuple(bins.shape), bins.dtype))
    dev = values.device
    _lib.ptr(values), _lib.ptr(bins)  # (refuses tensors that are not on the GPU)
    shape = (1 + max(sum(axis_bins), 0), int(n_metrics), 6)
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=dev)
        elif tuple(out.shape) != shape or out.dtype != torch.float64:
            raise ValueError('metric_stats_binned: out must be %s float64' % (shape,))
        p = _lib.ptr
        _lib.check(_lib.lib().mpsr_metric_stats_binned(
            p(values), p(bins), n_rows, n_cols, (ctypes.c_int * max(n_cols, 1))(*column_metric), int(n_metrics),
            len(axis_bins), (ctypes.c_int * max(len(axis_bins), 1))(*axis_bins), p(out), _lib.stream()))
    return out


def breakdown_dict(axes, tables):
    """result['breakdown'] of host copies of metric_stats_binned's output.  axes: [(axis, [bin labels])] in the order of
    the bins' columns; tables: [(table, metric names, stats (1 + the number of labels, n_metrics, 6))].
    -> {'axes': {axis: [labels]}, 'all': {table: {metric: statistics}}, 'tables': {table: {axis: {label: {metric:
    statistics}}}}}, every statistics a dict of STAT_NAMES."""
    out = dict(axes={axis: list(labels) for axis, labels in axes}, all={}, tables={})
    for table, names, stats in tables:
        out['all'][table] = metric_stats_dict(names, stats[0])
        slot, by_axis = 1, {}
        for axis, labels in axes:
            by_axis[axis] = {label: metric_stats_dict(names, stats[slot + k]) for k, label in enumerate(labels)}
            slot += len(labels)
        out['tables'][table] = by_axis
    return out


BREAKDOWN_HEADER = ('step', 'table', 'axis', 'bin', 'metric') + STAT_NAMES


def save_breakdown(predictions_base_dir, data_split, global_step, breakdown):
    """Appends breakdown_dict's statistics to <predictions_base_dir>/metrics/<split>/breakdown_<split>.csv in long
    format: one line per (table, axis, bin, metric) -- step, table, axis, bin, metric, count, mean, std, mean_abs,
    std_abs, dropped -- the tables, axes, bins and metrics in the dict's order, and before each table's bins its line
    over every row (axis and bin 'all').  Counts as integers, the four statistics as '{:.5f}'; into an empty file
    first the header; ',' between the fields and the csv module's line ending.  Returns the path."""
    out_dir = metrics_dir(predictions_base_dir, data_split)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'breakdown_%s.csv' % data_split)

    def lines(table, axis, label, stats):
        for metric, st in stats.items():
            yield ['{}'.format(global_step), table, axis, label, metric, '{:d}'.format(int(st['count']))] + \
                ['{:.5f}'.format(st[k]) for k in ('mean', 'std', 'mean_abs', 'std_abs')] + \
                ['{:d}'.format(int(st['dropped']))]

    with open(path, 'a', newline='') as f:
        writer = csv.writer(f, delimiter=',')
        if f.tell() == 0:
            writer.writerow(BREAKDOWN_HEADER)
        for table, by_axis in breakdown['tables'].items():
            writer.writerows(lines(table, 'all', 'all', breakdown['all'][table]))
            for axis, by_bin in by_axis.items():
                for label, stats in by_bin.items():
                    writer.writerows(lines(table, axis, label, stats))
    return path


AP_SLICES_HEADER = ('step', 'iou', 'bin', 'class', 'metric', 'difficulty', 'ap11', 'ap40')
AP_DIFFICULTIES = ('easy', 'moderate', 'hard')


def save_ap_slices(predictions_base_dir, data_split, global_step, slices):
    """Appends kitti_eval.evaluate_sliced's result to <predictions_base_dir>/metrics/<split>/ap_slices_<split>.csv in
    long format: one line per (iou, bin, class, metric key, difficulty) -- step, iou, bin, class, metric, difficulty,
    ap11, ap40 -- the slices, classes and metric keys in the dict's order.  The numbers as '{:.5f}' ('nan' stays
    'nan', whatever its sign); into an empty file first the header; ',' between the fields and the csv module's line
    ending.  Returns the path."""
    out_dir = metrics_dir(predictions_base_dir, data_split)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'ap_slices_%s.csv' % data_split)

    def number(v):
        v = float(v)
        return 'nan' if v != v else '{:.5f}'.format(v)

    with open(path, 'a', newline='') as f:
        writer = csv.writer(f, delimiter=',')
        if f.tell() == 0:
            writer.writerow(AP_SLICES_HEADER)
        for (iou, label), result in slices.items():
            for cls, by_key in result.items():
                for key, entry in by_key.items():
                    for d, name in enumerate(AP_DIFFICULTIES):
                        writer.writerow(['{}'.format(global_step), iou, label, cls, key, name,
                                         number(entry['ap11'][d]), number(entry['ap40'][d])])
    return path


def metrics_dir(predictions_base_dir, data_split):
    return os.path.join(predictions_base_dir, 'metrics', data_split)


# file name stem -> the statistic it holds
METRIC_FILES = (('metrics_avg', 'mean'), ('metrics_std', 'std'), ('metrics_avg_abs', 'mean_abs'),
                ('metrics_std_abs', 'std_abs'))


def save_metric_stats(predictions_base_dir, data_split, global_step, metric_stats):
    """Appends one line per call to metrics_avg_<split>.csv, metrics_std_<split>.csv, metrics_avg_abs_<split>.csv and
    metrics_std_abs_<split>.csv under <predictions_base_dir>/metrics/<split>/, in the format of the reference's
    save_metrics (evaluator_utils.py:280-403): the metric names sorted; into an empty file first a header of 'step'
    right-justified to 8 and every name without its 'metric_' prefix right-justified to 12; then the step
    right-justified to 8 and every value as '{:.5f}' right-justified to 12; ',' between the fields and the csv
    module's line ending.  metric_stats: {name: {mean, std, mean_abs, std_abs, ...}}.  Returns the four paths."""
    out_dir = metrics_dir(predictions_base_dir, data_split)
    os.makedirs(out_dir, exist_ok=True)
    names = sorted(metric_stats)
    header = ['step'.rjust(8)] + [(n[len('metric_'):] if n.startswith('metric_') else n).rjust(12) for n in names]
    paths = []
    for stem, stat in METRIC_FILES:
        path = os.path.join(out_dir, '%s_%s.csv' % (stem, data_split))
        with open(path, 'a', newline='') as f:
            writer = csv.writer(f, delimiter=',')
            if f.tell() == 0:
                writer.writerow(header)
            writer.writerow(['{}'.format(global_step).rjust(8)] +
                            ['{:.5f}'.format(metric_stats[n][stat]).rjust(12) for n in names])
        paths.append(path)
    return paths


def _save_prefixed_stats(prefix, predictions_base_dir, data_split, global_step, names, stats):
    """save_scene_stats ('scene_'), save_surface_stats ('surface_'), save_shape_stats ('shape_'), save_placed_stats
    ('placed_'), save_shape_surface_stats ('shape_surface_') and save_placed_surface_stats ('placed_surface_'):
    <prefix>metrics_<split>.csv."""
    out_dir = metrics_dir(predictions_base_dir, data_split)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, '%smetrics_%s.csv' % (prefix, data_split))
    short = [n[len(prefix):] if n.startswith(prefix) else n for n in names]
    with open(path, 'a', newline='') as f:
        writer = csv.writer(f, delimiter=',')
        if f.tell() == 0:
            writer.writerow(['step'.rjust(8)] + [('%s_%s' % (n, stat)).rjust(22) for n in short
                                                 for stat in ('count', 'mean', 'std')])
        row = ['{}'.format(global_step).rjust(8)]
        for n in names:
            st = stats[n]
            row += ['{:d}'.format(int(st['count'])).rjust(22), '{:.5f}'.format(st['mean']).rjust(22),
                    '{:.5f}'.format(st['std']).rjust(22)]
        writer.writerow(row)
    return path


def save_scene_stats(predictions_base_dir, data_split, global_step, names, scene_stats):
    """Appends one line per call to <predictions_base_dir>/metrics/<split>/scene_metrics_<split>.csv: the step, then
    count, mean and std of every metric of `names`, in that order; into an empty file first a header ('step', then
    <name>_count, <name>_mean, <name>_std with the 'scene_' prefix left off).  The step is right-justified to 8, the
    other fields to 22; counts as integers, means and stds as '{:.5f}'.  Returns the path."""
    return _save_prefixed_stats('scene_', predictions_base_dir, data_split, global_step, names, scene_stats)


def save_surface_stats(predictions_base_dir, data_split, global_step, names, surface_stats):
    """Appends one line per call to <predictions_base_dir>/metrics/<split>/surface_metrics_<split>.csv, in the format
    of save_scene_stats: the step, then count, mean and std of every metric of `names`, in that order; into an empty
    file first a header ('step', then <name>_count, <name>_mean, <name>_std with the 'surface_' prefix left off).  The
    step is right-justified to 8, the other fields to 22; counts as integers, means and stds as '{:.5f}'.  Returns the
    path."""
    return _save_prefixed_stats('surface_', predictions_base_dir, data_split, global_step, names, surface_stats)


def save_shape_stats(predictions_base_dir, data_split, global_step, names, shape_stats):
    """Appends one line per call to <predictions_base_dir>/metrics/<split>/shape_metrics_<split>.csv, in the format of
    save_scene_stats: the step, then count, mean and std of every metric of `names` (distance_metrics.shape_metric_names
    with the prefix 'shape_', which the header leaves off).  Returns the path."""
    return _save_prefixed_stats('shape_', predictions_base_dir, data_split, global_step, names, shape_stats)


def save_placed_stats(predictions_base_dir, data_split, global_step, names, placed_stats):
    """save_shape_stats for the scores in the camera frame: placed_metrics_<split>.csv, the prefix 'placed_'."""
    return _save_prefixed_stats('placed_', predictions_base_dir, data_split, global_step, names, placed_stats)


def save_shape_surface_stats(predictions_base_dir, data_split, global_step, names, stats):
    """save_shape_stats for the scores against surfaces: shape_surface_metrics_<split>.csv,
    the prefix 'shape_surface_'; `names` ends with the two columns of kept-triangle counts."""
    return _save_prefixed_stats('shape_surface_', predictions_base_dir, data_split, global_step, names, stats)


def save_placed_surface_stats(predictions_base_dir, data_split, global_step, names, stats):
    """save_shape_surface_stats in the camera frame: placed_surface_metrics_<split>.csv, the prefix
    'placed_surface_'."""
    return _save_prefixed_stats('placed_surface_', predictions_base_dir, data_split, global_step, names, stats)


def kitti_label_rows(box_3d, box_2d, classes, score_threshold, image_boxes=None, keep=None):
    """Detections of one frame -> list of KITTI label lines (no line ends).
    box_3d (n,9), box_2d (n,7) as format_predictions returns them; `image_boxes` (n,4) [x1,y1,x2,y2] replaces the
    2-D boxes of box_2d (projection mode), `keep` (n,) drops rows on top of the score filter."""
    cls, numbers = kitti_label_array(box_3d, box_2d, score_threshold, image_boxes, keep)
    names = [classes[int(k)] for k in cls]
    return [' '.join([name, '-1', '-1'] + [repr(float(v)) for v in row]) for name, row in zip(names, numbers)]


def write_kitti_label_file(path, rows):
    with open(path, 'w', newline='') as f:
        f.write(''.join(r + '\r\n' for r in rows))


def kitti_output_dir(predictions_base_dir, data_split, score_threshold, global_step):
    return '{}/kitti_predictions_3d/{}/{}/{}/data'.format(predictions_base_dir, data_split,
                                                          round(score_threshold, 3), global_step)


def export_kitti_labels(predictions, classes, score_threshold, out_dir, sample_names=None, project_3d_box=False,
                        frame_info=None):
    """predictions: {sample name: (box_3d (n,9), box_2d (n,7))} straight from format_predictions.  One file per name
    in `sample_names` (default: the dict's keys); frames without surviving detections get an empty file.
    project_3d_box: frame_info(sample name) -> (cam_p (3,4), (image_w, image_h)).  Returns the number of frames
    with at least one detection."""
    if project_3d_box and frame_info is None:
        raise ValueError('project_3d_box=True needs frame_info(sample_name) -> (cam_p, (image_w, image_h))')
    score_threshold = round(score_threshold, 3)
    os.makedirs(out_dir, exist_ok=True)
    valid = 0
    for name in (list(predictions) if sample_names is None else sample_names):
        rows = []
        if name in predictions and len(predictions[name][0]):
            b3, b2 = predictions[name]
            boxes, keep = (None, None)
            if project_3d_box:
                cam_p, size = frame_info(name)
                boxes, keep = project_boxes_3d(np.asarray(b3, np.float64).reshape(-1, 9), cam_p, size)
            rows = kitti_label_rows(b3, b2, classes, score_threshold, boxes, keep)
        valid += bool(rows)
        write_kitti_label_file(os.path.join(out_dir, name + '.txt'), rows)
    return valid


def _read_rows(path, width):
    if not os.path.exists(path) or os.path.getsize(path) == 0:
        return np.zeros((0, width))
    return np.loadtxt(path, ndmin=2).reshape(-1, width)


def save_predictions_box_3d_in_kitti_format(score_threshold, dataset, predictions_base_dir, predictions_box_3d_dir,
                                            predictions_box_2d_dir, global_step, project_3d_box=False):
    """The reference's entry point (same arguments): converts the per-sample text files MonoPSRModel.save_predictions
    wrote.  dataset: any object with `data_split`, `num_samples`, `sample_list[i].name`, `classes`; for
    project_3d_box=True also `frame_info(sample_name) -> (cam_p, (image_w, image_h))`.  Returns the output directory."""
    names = [dataset.sample_list[i].name for i in range(dataset.num_samples)]
    predictions = {}
    for name in names:
        b3 = _read_rows(os.path.join(predictions_box_3d_dir, name + '.txt'), 9)
        if len(b3):
            predictions[name] = (b3, _read_rows(os.path.join(predictions_box_2d_dir, name + '.txt'), 7))
    out_dir = kitti_output_dir(predictions_base_dir, dataset.data_split, score_threshold, global_step)
    export_kitti_labels(predictions, dataset.classes, score_threshold, out_dir, names, project_3d_box,
                        getattr(dataset, 'frame_info', None))
    return out_dir

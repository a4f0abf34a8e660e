"""Scores a model on a split: the reference's Evaluator.run_once (core/evaluator.py) with the predictions kept on the
card until the end.

    dataset = KittiDataset(cfg.dataset_config, 'val', mscnn_label_dir=...)      # use_mscnn_detections: True
    model = MonoPSRModel(cfg.model_config, cfg.dataset_config, net, 'test')
    result = Evaluator(model, dataset, score_threshold=0.1).run_once(global_step)
    print(result['report'])

Per chunk of frames: dataset.get_sample_dict, model.build_batch, instance_utils.format_boxes; box_3d / box_2d stay on
the device.  At the end one mpsr_kitti_detection_rows launch, one compaction and one copy to the host, then
kitti_eval.evaluate.  The evaluated frames are all of dataset.split_sample_names: a frame that keeps no label has no
detection and its ground truth counts as missed, as in the reference, which writes an empty file for it.

In 'val' mode it also reports the means of the per-object EMD / Chamfer metrics and of the loss terms
(MonoPSRModel.loss on the 'val'-mode build of each frame), accumulated on the device; NaN entries are skipped.

With metric_stats=True it also keeps one row per object of the reference's eight metrics (METRIC_COLUMNS) in a device
table and takes count / mean / std / mean |x| / std |x| of each in one mpsr_metric_stats launch at the end, under the
reference's NaN rule (a NaN drops its frame's values of that metric): result['metric_stats'], and with
predictions_base_dir the four metrics CSVs of the reference's save_metrics (evaluator_utils.save_metric_stats).

Checkpoint sweeps (the reference's run_latest_checkpoints / repeated_checkpoint_run, core/evaluator.py:387-526):
run_latest_checkpoints and repeated_checkpoint_run over checkpoint_utils.list_checkpoints, with the evaluated steps kept
in <predictions_base_dir>/evaluated_<split>.txt and every report in kitti_reports/<split>/.  The order and the skipping
are sweep_checkpoints / repeated_sweep, plain functions of a checkpoint list, the evaluated set and a callable.
python -m monopsr_amd.experiments.run_evaluation is the command line of a sweep.

chunk_hook: a callable that sees every chunk's (rows, samples, outs) during the pass, so that one network pass serves
the label files and whatever else is made of the predictions (experiments/run_inference.py: the scenes of
core/scene_reconstruction.py).

scene_metrics=True ('val' mode only): every chunk is also reconstructed (core/scene_reconstruction.py, min_score None,
the sample's gt_valid_mask_maps) and scored against dataset.frame_ground_truth(rows) in one mpsr_scene_score launch; the
per-box tables of scene_reconstruction.SCENE_METRIC_NAMES stay on the card, and one mpsr_metric_stats launch at the end
takes their statistics with NAN_RULE_ENTRY (a box without overlap drops its own entry, not its frame):
result['scene_stats'], and with predictions_base_dir one line in metrics/<split>/scene_metrics_<split>.csv
(evaluator_utils.save_scene_stats).  DESIGN.md section 7.8.

centroid_fit: None, or a dict of instance_metrics.fit_centroids' options ({} for its defaults).  With it every chunk's
predicted centroids are fitted to their 2-D boxes straight after build_batch: the label files,
AP, the scene and surface metrics and the chunk_hook all see the fitted boxes, and result['centroid_fit'] holds the
numbers of boxes that converged, stopped at the cap and were not fitted, and the mean projection error at the fit's
start (the predicted centroid put on its viewing ray: not the unfitted scene's error) and at its end over the fitted
ones.  The per-object metric table and the losses come from the 'val'-mode graph and are not affected.

scene_metrics='surface' does what True does and also renders every chunk's maps as surfaces (DESIGN.md section 7.9:
scene_reconstruction.render_instance_surfaces with its default max_edge_dz and max_span_px) and scores them against the
same ground truth: result['surface_stats'] over scene_reconstruction.SURFACE_METRIC_NAMES, and with predictions_base_dir
one line in metrics/<split>/surface_metrics_<split>.csv (evaluator_utils.save_surface_stats).

breakdown: None, or a dict of options ({} for the defaults), 'val' mode only.  With it every
chunk's predicted boxes (format_boxes' output: the fitted boxes with centroid_fit) are set against their own labels in one
mpsr_object_pairs launch -- the samples' boxes_3d and boxes_2d and dataset.frame_label_info(rows) -- and the per-object
table of evaluator_utils.PAIR_COLUMNS stays on the card with each object's bins: the label's depth (depth_edges, default
10 .. 50 m), its KITTI difficulty and the IoU of the fed 2-D box with the label's own (box_iou_edges, default 0.7, 0.8,
0.9).  At the end one mpsr_metric_stats_binned launch per table kept ('object' always, 'metrics' with metric_stats,
'scene' / 'surface' with scene_metrics) and one copy: result['breakdown'] (evaluator_utils.breakdown_dict), and with
predictions_base_dir metrics/<split>/breakdown_<split>.csv (result['breakdown_csv']).  Bins use NAN_RULE_ENTRY.  The hit
columns' means are shares of the evaluated labels, not KITTI recall: frames and labels the dataset's filter drops are
not in the denominator.

ap_slices: None, or a dict of options ({} for the defaults: both IoU sets, depth edges 10 .. 50 m), wherever
result['kitti'] is computed.  With it the frames assembled for result['kitti'] also go through
one kitti_eval.evaluate_sliced call: result['kitti_slices'] = {(iou, bin label): a result of result['kitti']'s form},
'all' and every depth bin of every IoU set of 'ious'; with predictions_base_dir also
kitti_reports/<split>/<step, 8 digits>_slices.txt (kitti_eval.format_sliced_report) and, in long format,
metrics/<split>/ap_slices_<split>.csv (evaluator_utils.save_ap_slices).  result['kitti'] and result['report'] keep
coming from `iou`.

shape_metrics: None, or a dict of options ({} for the defaults), 'val' mode only: 'thresholds'
(default distance_metrics.DEFAULT_SHAPE_THRESHOLDS: 0.05, 0.1 and 0.2 m, an assumption of this package) and 'placed'
(default False).  With it every chunk's predicted instance maps are scored against the ground-truth maps over the valid
points only, after the optional centroid fit (core/distance_metrics.py chunk_shape_scores, one mpsr_shape_scores launch
per chunk): accuracy, completeness, Chamfer-L1, squared Chamfer and Hausdorff in metres, precision / recall / F-score
at every threshold, in the object's own frame.  With 'placed' the same once more in the camera frame, of the maps placed
with the predicted (or fitted) centroid and viewing angle against gt_inst_xyz_maps_global: the number that shows what
centroid_fit does in 3-D.  The per-object tables stay on the card, and one mpsr_metric_stats launch per table at the end
takes their statistics with NAN_RULE_ENTRY: result['shape_stats'] and result['placed_stats'] (the names carry the
prefixes 'shape_' and 'placed_'), with predictions_base_dir one line each in metrics/<split>/shape_metrics_<split>.csv
and placed_metrics_<split>.csv (save_scene_stats' format), and with breakdown the kinds 'shape' and 'placed'.  METRIC_EMD
and METRIC_CHAMFER, the reference's two shape numbers over all 48 x 48 points, are not changed by it.

shape_surface_metrics: None, or a dict of options ({} for the defaults), 'val' mode only,
independent of shape_metrics: 'thresholds' (default DEFAULT_SHAPE_THRESHOLDS), 'max_edge' (default
distance_metrics.DEFAULT_SHAPE_MAX_EDGE: 0.5 m, an assumption of this package) and 'placed' (default False).  The same
clouds and masks as shape_metrics, after the optional centroid fit and before chunk_hook, but the distance of a point
is taken to the other map's triangulated surface (core/distance_metrics.py chunk_surface_scores, one
mpsr_surface_scores launch per chunk): at thresholds as tight as the grid's spacing the point scores measure how the
two grids interleave.  result['shape_surface_stats'] and result['placed_surface_stats'] under NAN_RULE_ENTRY (the
prefixes 'shape_surface_' and 'placed_surface_'; after the metrics two more columns, triangles_a and triangles_b: the
kept triangles of the prediction and of the ground truth), metrics/<split>/shape_surface_metrics_<split>.csv and
placed_surface_metrics_<split>.csv, and with breakdown the kinds 'shape_surface' and 'placed_surface'.

Not built: TF summaries and metrics_to_show.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from monopsr_amd.core import constants, evaluator_utils, kitti_eval
from monopsr_amd.datasets.kitti import instance_utils

# rows of mpsr_kitti_detection_rows (kitti_eval's column order) -> the columns of a label line after the class,
# truncation and occlusion: alpha | x1 y1 x2 y2 | h w l | x y z | ry score
_LINE_COLUMNS = [4, 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12]

# the metric table's columns, in order: (metric, number of columns).  The three columns of the dimension error are one
# metric: the reference flattens them into one list.
METRIC_COLUMNS = ((constants.METRIC_EMD, 1), (constants.METRIC_CHAMFER, 1), (constants.METRIC_VIEW_ANG_ERR, 1),
                  (constants.METRIC_PROP_CEN_Z_ERR, 1), (constants.METRIC_CEN_X_ERR, 1), (constants.METRIC_CEN_Y_ERR, 1),
                  (constants.METRIC_CEN_Z_ERR, 1), (constants.METRIC_DIM_ERR, 3))
METRIC_NAMES = tuple(name for name, _ in METRIC_COLUMNS)
COLUMN_METRIC = tuple(k for k, (_, width) in enumerate(METRIC_COLUMNS) for _ in range(width))

# what Evaluator(centroid_fit={...}) may hold: instance_metrics.fit_centroids' options
_CENTROID_FIT_OPTIONS = ('fit_viewing_angle', 'use_pixel_centres', 'cam0_shift')

# what Evaluator(breakdown={...}) may hold, with the defaults
_BREAKDOWN_OPTIONS = dict(depth_edges=evaluator_utils.DEFAULT_DEPTH_EDGES,
                          box_iou_edges=evaluator_utils.DEFAULT_BOX_IOU_EDGES)

# what Evaluator(shape_metrics={...}) may hold
_SHAPE_METRICS_OPTIONS = ('thresholds', 'placed')

# what Evaluator(shape_surface_metrics={...}) may hold
_SHAPE_SURFACE_OPTIONS = ('thresholds', 'max_edge', 'placed')

# what Evaluator(ap_slices={...}) may hold, with the defaults
_AP_SLICES_OPTIONS = dict(ious=('standard', 'low'), depth_edges=evaluator_utils.DEFAULT_DEPTH_EDGES)


def sweep_checkpoints(checkpoints, evaluated, run, ckpt_indices=None):
    """The order and the skipping of a sweep.  checkpoints: [(step, prefix)]; evaluated: a set of steps, updated in
    place; run(step, prefix) evaluates one.  ckpt_indices None: every checkpoint whose step is not in `evaluated`, in
    step order; -1 (or [-1]): the latest; otherwise the listed steps, in the order given (a step that is no checkpoint
    is a KeyError naming it, raised before anything runs).  Listed steps and the latest run whether evaluated before
    or not, as in the reference.  -> [run's results]."""
    by_step = dict(checkpoints)
    if ckpt_indices is None:
        todo = [step for step in sorted(by_step) if step not in evaluated]
    else:
        wanted = [int(i) for i in np.atleast_1d(np.asarray(ckpt_indices))]
        todo = []
        for i in wanted:
            if i == -1:
                if not by_step:
                    raise KeyError('no checkpoint to take the latest of')
                i = max(by_step)
            if i not in by_step:
                raise KeyError('no checkpoint of step %d (there are: %s)' % (i, sorted(by_step)))
            todo.append(i)
    results = []
    for step in todo:
        results.append(run(step, by_step[step]))
        evaluated.add(step)
    return results


def repeated_sweep(list_checkpoints, evaluated, run, max_iterations, eval_wait_interval=30, max_idle_seconds=None,
                   sleep=time.sleep, clock=time.monotonic):
    """Lists (list_checkpoints() -> [(step, prefix)]), evaluates what is new with sweep_checkpoints, and sleeps
    eval_wait_interval seconds when nothing is.  Returns the results once a step >= max_iterations is in `evaluated`,
    or once max_idle_seconds (None: never) have passed without a new checkpoint."""
    results = []
    last_new = clock()
    while True:
        new = sweep_checkpoints(list_checkpoints(), evaluated, run)
        results.extend(new)
        if evaluated and max(evaluated) >= max_iterations:
            return results
        if new:
            last_new = clock()
            continue
        if max_idle_seconds is not None and clock() - last_new >= max_idle_seconds:
            return results
        sleep(eval_wait_interval)


class Evaluator:

    def __init__(self, model, dataset, score_threshold=0.1, predictions_base_dir=None, batch_size=8,
                 project_3d_box=False, iou='standard', compute_metrics=True, compute_losses=True, metric_stats=False,
                 skip_evaluated_checkpoints=True, scene_metrics=False, breakdown=None, ap_slices=None,
                 shape_surface_metrics=None, shape_metrics=None, centroid_fit=None, chunk_hook=None):
        if iou not in kitti_eval.MIN_OVERLAP:
            raise ValueError('iou must be one of %s' % sorted(kitti_eval.MIN_OVERLAP))
        if ap_slices is not None:
            unknown = set(ap_slices) - set(_AP_SLICES_OPTIONS)
            if unknown:
                raise ValueError('ap_slices: unknown options %s' % sorted(unknown))
            ious = ap_slices.get('ious', _AP_SLICES_OPTIONS['ious'])
            ap_slices = dict(ious=(ious,) if isinstance(ious, str) else tuple(ious),
                             depth_edges=tuple(float(v) for v in ap_slices.get('depth_edges',
                                                                               _AP_SLICES_OPTIONS['depth_edges'])))
            kitti_eval.slice_table(**ap_slices)  # ValueError for what evaluate_sliced would refuse
        # None, or {'ious': (...), 'depth_edges': (...)}: AP per IoU set and depth bin next to result['kitti']
        self.ap_slices = ap_slices
        if int(batch_size) < 1:
            raise ValueError('batch_size %r' % (batch_size,))
        if not (getattr(dataset, 'is_test', False) or getattr(dataset, 'merges_mscnn', False)):
            raise ValueError("Evaluator needs a dataset whose samples carry label_scores: 'val' with "
                             "use_mscnn_detections, or 'test' (KittiDataset(..., mscnn_label_dir=...))")
        if scene_metrics and getattr(dataset, 'train_val_test', None) != 'val':
            raise ValueError("scene_metrics scores the reconstruction against ground truth: it needs a 'val'-mode "
                             "dataset, got %r" % (getattr(dataset, 'train_val_test', None),))
        if isinstance(scene_metrics, str) and scene_metrics != 'surface':
            raise ValueError("scene_metrics must be False, True or 'surface', got %r" % (scene_metrics,))
        if centroid_fit is not None:
            unknown = set(centroid_fit) - set(_CENTROID_FIT_OPTIONS)
            if unknown:
                raise ValueError('centroid_fit: unknown options %s' % sorted(unknown))
        if breakdown is not None:
            if getattr(dataset, 'train_val_test', None) != 'val':
                raise ValueError("breakdown sets every prediction against its label: it needs a 'val'-mode dataset, "
                                 "got %r" % (getattr(dataset, 'train_val_test', None),))
            unknown = set(breakdown) - set(_BREAKDOWN_OPTIONS)
            if unknown:
                raise ValueError('breakdown: unknown options %s' % sorted(unknown))
            breakdown = {k: tuple(float(v) for v in breakdown.get(k, default))
                         for k, default in _BREAKDOWN_OPTIONS.items()}
        # None, or {'depth_edges': (...), 'box_iou_edges': (...)}: the per-object overlap table and the binned statistics
        self.breakdown = breakdown
        if shape_metrics is not None:
            from monopsr_amd.core import distance_metrics
            if getattr(dataset, 'train_val_test', None) != 'val':
                raise ValueError("shape_metrics scores the predicted maps against the ground-truth maps: it needs a "
                                 "'val'-mode dataset, got %r" % (getattr(dataset, 'train_val_test', None),))
            unknown = set(shape_metrics) - set(_SHAPE_METRICS_OPTIONS)
            if unknown:
                raise ValueError('shape_metrics: unknown options %s' % sorted(unknown))
            shape_metrics = dict(
                thresholds=distance_metrics.check_thresholds(
                    shape_metrics.get('thresholds', distance_metrics.DEFAULT_SHAPE_THRESHOLDS)),
                placed=bool(shape_metrics.get('placed', False)))
        # None, or {'thresholds': (...), 'placed': bool}: the shape scores over valid points
        self.shape_metrics = shape_metrics
        # after a run_once with shape_metrics: (table (n, 5 + 3T) float32 in distance_metrics.shape_metric_names' order,
        # counts (n, 2 + 2T) int32, sums (n,6) float64, frame (n,) int32) on the device, one row per object in the order
        # of the pass; placed_table the same in the camera frame (None without 'placed')
        self.shape_table = None
        self.placed_table = None
        if shape_surface_metrics is not None:
            from monopsr_amd.core import distance_metrics
            if getattr(dataset, 'train_val_test', None) != 'val':
                raise ValueError("shape_surface_metrics scores the predicted maps against the ground-truth maps: it "
                                 "needs a 'val'-mode dataset, got %r" % (getattr(dataset, 'train_val_test', None),))
            unknown = set(shape_surface_metrics) - set(_SHAPE_SURFACE_OPTIONS)
            if unknown:
                raise ValueError('shape_surface_metrics: unknown options %s' % sorted(unknown))
            shape_surface_metrics = dict(
                thresholds=distance_metrics.check_thresholds(
                    shape_surface_metrics.get('thresholds', distance_metrics.DEFAULT_SHAPE_THRESHOLDS)),
                max_edge=distance_metrics.check_max_edge(
                    shape_surface_metrics.get('max_edge', distance_metrics.DEFAULT_SHAPE_MAX_EDGE)),
                placed=bool(shape_surface_metrics.get('placed', False)))
        # None, or {'thresholds': (...), 'max_edge': float, 'placed': bool}: the shape scores against surfaces
        self.shape_surface_metrics = shape_surface_metrics
        # after a run_once with shape_surface_metrics: shape_table's form, the table with two more columns (the kept
        # triangles of a and of b); placed_surface_table the same in the camera frame (None without 'placed')
        self.shape_surface_table = None
        self.placed_surface_table = None
        # after a run_once with breakdown: (table (n,9) float32 in evaluator_utils.PAIR_COLUMNS' order, overlaps (n,4)
        # float64, bins (n,3) int32 in evaluator_utils.BREAKDOWN_AXES' order, frame (n,) int32) on the device
        self.pair_table = None
        self.model = model
        # None, or a dict of instance_metrics.fit_centroids' options ({} for the defaults): every chunk's centroids are
        # fitted to their 2-D boxes straight after build_batch, and everything below sees the fitted boxes
        self.centroid_fit = None if centroid_fit is None else dict(centroid_fit)
        self.scene_metrics = bool(scene_metrics)
        self.surface_metrics = scene_metrics == 'surface'
        # after a run_once with scene_metrics='surface': (table (n,6) float32 in SURFACE_METRIC_NAMES order, counts
        # (n,5) int32, sums (n,3) float64, frame (n,) int32) on the device, in the order of the pass
        self.surface_table = None
        # after a run_once with scene_metrics: (table (n,6) float32 in SCENE_METRIC_NAMES order, counts (n,6) int32,
        # sums (n,3) float64, frame (n,) int32) on the device, one row per object in the order of the pass
        self.scene_table = None
        self.compute_metrics = bool(compute_metrics)
        self.compute_losses = bool(compute_losses)
        self.metric_stats = bool(metric_stats)
        self.skip_evaluated_checkpoints = bool(skip_evaluated_checkpoints)
        # chunk_hook(rows, samples, outs), called after each build_batch of the pass: rows = the chunk's frames as rows
        # of the dataset's frame tables (sample_names), samples / outs what get_sample_dict / build_batch returned
        # (experiments/run_inference.py writes the scenes through it); None: nothing is called
        self.chunk_hook = chunk_hook
        # after a run_once with metric_stats: (values (n,10) float32, frame (n,) int32) on the device
        self.metric_table = None
        self._loss_model = None
        self.dataset = dataset
        self.score_threshold = round(float(score_threshold), 3)
        self.predictions_base_dir = predictions_base_dir
        self.batch_size = int(batch_size)
        self.project_3d_box = bool(project_3d_box)
        self.iou = iou

    # ---- the pass over the split

    def _predict(self):
        """-> (box_3d (N,9), box_2d (N,7), frame (N,) int32: rows of the dataset's frame tables; metric sums (2,2):
        [emd, chamfer] x [sum of the entries that are not NaN, their number]; loss names and their sums (n,2) in the
        same form; the metric table (N, 10) float32 in METRIC_COLUMNS' order, or None; with scene_metrics the scene
        scores (table (N,6) float32, counts (N,6) int32, sums (N,3) float64), else None; with scene_metrics='surface'
        the surface scores in the same form (counts (N,5)), else None; with breakdown the pair table (table (N,9) float32,
        overlaps (N,4) float64, bins (N,3) int32), else None; with shape_metrics the shape scores (table (N, 5 + 3T)
        float32, counts (N, 2 + 2T) int32, sums (N,6) float64), else None; with its 'placed' the same in the camera
        frame, else None; with shape_surface_metrics and its 'placed' the same two against surfaces, the tables with
        two more columns), all on the device."""
        ds, model = self.dataset, self.model
        dev = ds.device
        # the frames in split order, whatever the epoch's shuffle made of sample_list
        position = np.argsort(np.asarray(ds.sample_list), kind='stable')
        b3s, b2s, frames = [], [], []
        sums = torch.zeros((2, 2), dtype=torch.float64, device=dev)
        with_metrics = ds.train_val_test == 'val' and self.compute_metrics
        with_losses = ds.train_val_test == 'val' and self.compute_losses
        with_table = ds.train_val_test == 'val' and self.metric_stats
        loss_names, loss_sums = [], None
        table = []
        scene_parts, surface_parts, pair_parts = [], [], []
        self._fits = []
        shape_parts, placed_parts = [], []
        shape_surface_parts, placed_surface_parts = [], []
        if with_losses or with_table:
            # the 'val'-mode graph of the same net: method by method, with the ground truth and the offsets
            from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
            if self._loss_model is None:
                self._loss_model = MonoPSRModel(model.model_config, model.dataset_config, model.device_net, 'val',
                                                model.classes_name, fused_heads=False)
            self._loss_model.device_net = model.device_net
        with torch.cuda.device(dev), torch.no_grad():
            for a in range(0, ds.num_samples, self.batch_size):
                rows = np.arange(a, min(a + self.batch_size, ds.num_samples))
                samples = ds.get_sample_dict(position[rows], epoch=0)
                outs = model.build_batch(samples)
                if self.centroid_fit is not None:
                    from monopsr_amd.core.instances import instance_metrics
                    outs, fit = instance_metrics.fit_centroids(model, samples, outs, **self.centroid_fit)
                    self._fits.append(fit)
                if self.shape_metrics is not None:
                    from monopsr_amd.core import distance_metrics
                    for parts, scores in zip((shape_parts, placed_parts),
                                             distance_metrics.chunk_shape_scores(model, samples, outs,
                                                                                 **self.shape_metrics)):
                        if scores is not None:
                            parts.append((scores.table, scores.counts, scores.sums))
                if self.shape_surface_metrics is not None:
                    from monopsr_amd.core import distance_metrics
                    for parts, scores in zip((shape_surface_parts, placed_surface_parts),
                                             distance_metrics.chunk_surface_scores(model, samples, outs,
                                                                                   **self.shape_surface_metrics)):
                        if scores is not None:
                            parts.append((torch.cat([scores.table, scores.tri_counts.float()], 1), scores.counts,
                                          scores.sums))
                if self.chunk_hook is not None:
                    self.chunk_hook(rows, samples, outs)
                if self.scene_metrics:
                    from monopsr_amd.core import scene_reconstruction
                    gt = ds.frame_ground_truth(rows)
                    gt = dict(depth_maps=[g['depth_map'] for g in gt], instance_images=[g['instance_image'] for g in gt],
                              box_gt_id=torch.cat([g['instance_ids'] for g in gt]))
                    scene = scene_reconstruction.reconstruct_frames(model, samples, outs, min_score=None, ground_truth=gt,
                                                                    surfaces={} if self.surface_metrics else None)
                    scores = scene.scores
                    scene_parts.append((scores.table(), scores.counts, scores.sums))
                    if self.surface_metrics:
                        scores = scene.surfaces.scores
                        surface_parts.append((scores.table(), scores.counts, scores.sums))
                chunk_b3 = []
                for r, s, o in zip(rows, samples, outs):
                    n = int(s['num_objs'])
                    b3, b2 = instance_utils.format_boxes(
                        o[constants.KEY_LWH], o[constants.KEY_VIEW_ANG], o[constants.KEY_ALPHA_BINS],
                        o[constants.KEY_ALPHA_REGS], o[constants.KEY_CENTROIDS], s['boxes_2d'], s['label_scores'],
                        s['class_indices'], s['cam_p'], s['rgb_image'].shape, centroid_type=model.centroid_type,
                        post_process_cen_x=model.post_process_cen_x)
                    b3s.append(b3[0:n])
                    chunk_b3.append(b3[0:n])
                    b2s.append(b2[0:n])
                    frames.append(torch.full((n,), int(r), dtype=torch.int32, device=dev))
                    if with_metrics or with_table:
                        m = model.evaluate_predictions(
                            {constants.KEY_INST_XYZ_MAP_LOCAL: o[constants.KEY_INST_XYZ_MAP_LOCAL]},
                            {constants.KEY_INST_XYZ_MAP_LOCAL: s['gt_inst_xyz_maps_local'],
                             constants.KEY_VALID_MASK_MAPS: s['gt_valid_mask_maps']}, n)
                        for k, key in enumerate((constants.METRIC_EMD, constants.METRIC_CHAMFER)):
                            v = m[key].double()
                            ok = ~torch.isnan(v)  # the reference's np.nanmean
                            sums[k, 0] += torch.where(ok, v, torch.zeros_like(v)).sum()
                            sums[k, 1] += ok.sum()
                    if with_losses or with_table:
                        lm = self._loss_model
                        out, _ = lm.build(s)
                    if with_table:
                        keys = (constants.KEY_PROP_CEN_Z, constants.KEY_CENTROIDS, constants.KEY_LWH + '_offs',
                                constants.KEY_VIEW_ANG)
                        m.update(lm.evaluate_predictions({k: out[k] for k in keys if k in out}, lm.gt_dict, n))
                        # (a metric this model does not produce is a column of NaN: count 0)
                        table.append(torch.cat(
                            [m[name].float().reshape(n, width) if name in m else
                             torch.full((n, width), float('nan'), dtype=torch.float32, device=dev)
                             for name, width in METRIC_COLUMNS], 1))
                    if with_losses:
                        losses, total = lm.loss(out, lm.gt_dict, s['gt_alpha_valid_bins'])
                        losses = dict(losses, total_loss=total)
                        if loss_sums is None:
                            loss_names = sorted(losses)
                            loss_sums = torch.zeros((len(loss_names), 2), dtype=torch.float64, device=dev)
                        v = torch.stack([torch.as_tensor(losses[k]).double().sum() for k in loss_names])
                        ok = ~torch.isnan(v)
                        loss_sums[:, 0] += torch.where(ok, v, torch.zeros_like(v))
                        loss_sums[:, 1] += ok
                if self.breakdown is not None:
                    pair_parts.append(evaluator_utils.object_pairs(
                        torch.cat(chunk_b3), torch.cat([s['boxes_3d'][0:int(s['num_objs'])] for s in samples]),
                        torch.cat([s['boxes_2d'][0:int(s['num_objs'])] for s in samples]),
                        torch.cat(ds.frame_label_info(rows)), **self.breakdown))
        return (torch.cat(b3s), torch.cat(b2s), torch.cat(frames), sums, loss_names, loss_sums,
                torch.cat(table).contiguous() if with_table else None,
                tuple(torch.cat(part).contiguous() for part in zip(*scene_parts)) if self.scene_metrics else None,
                tuple(torch.cat(part).contiguous() for part in zip(*surface_parts)) if self.surface_metrics else None,
                tuple(torch.cat(part).contiguous() for part in zip(*pair_parts)) if pair_parts else None,
                tuple(torch.cat(part).contiguous() for part in zip(*shape_parts)) if shape_parts else None,
                tuple(torch.cat(part).contiguous() for part in zip(*placed_parts)) if placed_parts else None,
                tuple(torch.cat(part).contiguous() for part in zip(*shape_surface_parts))
                if shape_surface_parts else None,
                tuple(torch.cat(part).contiguous() for part in zip(*placed_surface_parts))
                if placed_surface_parts else None)

    def _rows_to_host(self, b3, b2, frame):
        """One launch, one compaction, one copy: -> (rows (m,14) float64, class index (m,), frame (m,)) of the kept
        detections, in the order of the pass."""
        ds = self.dataset
        dev = b3.device
        n = int(b3.shape[0])
        with torch.cuda.device(dev):
            p2 = wh = None
            if self.project_3d_box:
                p2_host, wh_host = ds.frame_calibrations()
                p2, wh = torch.from_numpy(p2_host).to(dev), torch.from_numpy(wh_host).to(dev)
            rows, cls, keep = evaluator_utils.detection_rows(b3.contiguous(), b2.contiguous(), self.score_threshold,
                                                             frame, p2, wh, self.project_3d_box)
            packed = torch.cat([rows, cls.double()[:, None], frame.double()[:, None], keep.double()[:, None]], 1)
            # the kept rows first, in their order (a stable sort needs no count on the host)
            order = torch.sort(1 - keep, stable=True).indices
            host = packed.index_select(0, order).cpu().numpy()
        m = int(host[:, 16].sum()) if n else 0
        return host[:m, 0:14], host[:m, 14].astype(np.int64), host[:m, 15].astype(np.int64)

    def run_once(self, global_step=None):
        ds = self.dataset
        (b3, b2, frame, sums, loss_names, loss_sums, table, scene, surface, pairs, shape, placed, shape_surface,
         placed_surface) = self._predict()
        rows, cls, frame_h = self._rows_to_host(b3, b2, frame)
        names = ds.sample_names
        per_frame = {}
        for r in np.unique(frame_h):
            sel = frame_h == r
            per_frame[names[int(r)]] = (rows[sel], cls[sel])
        result = dict(num_frames=len(ds.split_sample_names), num_frames_with_detections=len(per_frame),
                      num_detections=int(len(rows)), num_predictions=int(b3.shape[0]), global_step=global_step,
                      kitti=None, report=None, metrics={}, losses={})
        if self.centroid_fit is not None:
            from monopsr_amd.core.instances import instance_metrics
            c = instance_metrics.fit_summary(self._fits).cpu().numpy()  # reduced on the card, one copy
            self._fits = []
            fitted = c[0] + c[1]
            result['centroid_fit'] = dict(
                converged=int(c[0]), capped=int(c[1]), not_fitted=int(c[2]),
                mean_err0=float(c[3] / fitted) if fitted else float('nan'),
                mean_err=float(c[4] / fitted) if fitted else float('nan'))
        if ds.train_val_test == 'val' and (self.compute_metrics or loss_names or table is not None):
            # one copy for all tables
            names = [constants.METRIC_EMD, constants.METRIC_CHAMFER] + list(loss_names)
            parts = [sums] + ([] if loss_sums is None else [loss_sums])
            if table is not None:
                self.metric_table = (table, frame)
                stats = evaluator_utils.metric_stats(table, frame, COLUMN_METRIC, len(METRIC_NAMES), ds.num_samples,
                                                     evaluator_utils.NAN_RULE_FRAME)
                parts.append(stats)
            s = torch.cat([t.reshape(-1) for t in parts]).cpu().numpy()
            if table is not None:
                result['metric_stats'] = evaluator_utils.metric_stats_dict(
                    METRIC_NAMES, s[-6 * len(METRIC_NAMES):].reshape(len(METRIC_NAMES), 6))
            s = s[:2 * len(names)].reshape(len(names), 2)
            means = {key: float(s[k, 0] / s[k, 1]) if s[k, 1] else float('nan') for k, key in enumerate(names)}
            if self.compute_metrics:
                result['metrics'] = {key: means[key] for key in names[:2]}
            result['losses'] = {key: means[key] for key in loss_names}
        if 'metric_stats' in result and self.predictions_base_dir is not None:
            result['metrics_csv'] = evaluator_utils.save_metric_stats(self.predictions_base_dir, ds.data_split,
                                                                      global_step, result['metric_stats'])
        from monopsr_amd.core.scene_reconstruction import SCENE_METRIC_NAMES, SURFACE_METRIC_NAMES
        shape_names, placed_names = (), ()
        if self.shape_metrics is not None:
            from monopsr_amd.core import distance_metrics
            shape_names = distance_metrics.shape_metric_names(self.shape_metrics['thresholds'], 'shape_')
            placed_names = distance_metrics.shape_metric_names(self.shape_metrics['thresholds'], 'placed_')
        shape_surface_names, placed_surface_names = (), ()
        if self.shape_surface_metrics is not None:
            from monopsr_amd.core import distance_metrics
            shape_surface_names, placed_surface_names = (
                distance_metrics.shape_metric_names(self.shape_surface_metrics['thresholds'], prefix) +
                (prefix + 'triangles_a', prefix + 'triangles_b') for prefix in ('shape_surface_', 'placed_surface_'))
        for kind, metric_names, parts, save in (
                ('scene', SCENE_METRIC_NAMES, scene, evaluator_utils.save_scene_stats),
                ('surface', SURFACE_METRIC_NAMES, surface, evaluator_utils.save_surface_stats),
                ('shape', shape_names, shape, evaluator_utils.save_shape_stats),
                ('placed', placed_names, placed, evaluator_utils.save_placed_stats),
                ('shape_surface', shape_surface_names, shape_surface, evaluator_utils.save_shape_surface_stats),
                ('placed_surface', placed_surface_names, placed_surface, evaluator_utils.save_placed_surface_stats)):
            if parts is None:
                continue
            setattr(self, kind + '_table', parts + (frame,))
            stats = evaluator_utils.metric_stats(parts[0], frame, range(len(metric_names)), len(metric_names),
                                                 ds.num_samples, evaluator_utils.NAN_RULE_ENTRY)
            result[kind + '_stats'] = evaluator_utils.metric_stats_dict(metric_names, stats.cpu().numpy())
            if self.predictions_base_dir is not None:
                result[kind + '_metrics_csv'] = save(self.predictions_base_dir, ds.data_split, global_step,
                                                     metric_names, result[kind + '_stats'])
        if pairs is not None:
            self.pair_table = pairs + (frame,)
            axes = [('depth', evaluator_utils.edge_labels(self.breakdown['depth_edges'])),
                    ('difficulty', evaluator_utils.DIFFICULTY_LABELS),
                    ('fed_box', evaluator_utils.edge_labels(self.breakdown['box_iou_edges']))]
            kept = [('object', evaluator_utils.PAIR_COLUMNS, pairs[0], range(len(evaluator_utils.PAIR_COLUMNS)))]
            if table is not None:
                kept.append(('metrics', METRIC_NAMES, table, COLUMN_METRIC))
            for kind, metric_names, parts in (('scene', SCENE_METRIC_NAMES, scene),
                                              ('surface', SURFACE_METRIC_NAMES, surface),
                                              ('shape', shape_names, shape), ('placed', placed_names, placed),
                                              ('shape_surface', shape_surface_names, shape_surface),
                                              ('placed_surface', placed_surface_names, placed_surface)):
                if parts is not None:
                    kept.append((kind, metric_names, parts[0], range(len(metric_names))))
            # one launch per table, one copy for all of them
            stats = [evaluator_utils.metric_stats_binned(values, pairs[2], column_metric, len(metric_names),
                                                         [len(labels) for _, labels in axes])
                     for _, metric_names, values, column_metric in kept]
            host, at, host_stats = torch.cat([t.reshape(-1) for t in stats]).cpu().numpy(), 0, []
            for t in stats:
                host_stats.append(host[at:at + t.numel()].reshape(tuple(t.shape)))
                at += t.numel()
            result['breakdown'] = evaluator_utils.breakdown_dict(
                axes, [(kind, metric_names, st) for (kind, metric_names, _, _), st in zip(kept, host_stats)])
            if self.predictions_base_dir is not None:
                result['breakdown_csv'] = evaluator_utils.save_breakdown(self.predictions_base_dir, ds.data_split,
                                                                         global_step, result['breakdown'])
        if self.predictions_base_dir is not None:
            out_dir = evaluator_utils.kitti_output_dir(self.predictions_base_dir, ds.data_split, self.score_threshold,
                                                       global_step)
            os.makedirs(out_dir, exist_ok=True)
            for name in ds.split_sample_names:
                lines = []
                if name in per_frame:
                    r, c = per_frame[name]
                    lines = [' '.join([ds.classes[int(k)], '-1', '-1'] + [repr(float(v)) for v in row])
                             for k, row in zip(c, r[:, _LINE_COLUMNS])]
                evaluator_utils.write_kitti_label_file(os.path.join(out_dir, name + '.txt'), lines)
            result['kitti_predictions_dir'] = out_dir
        if ds.train_val_test == 'val' or ds.has_kitti_labels:
            # the frames in the order of their index, as kitti_eval.evaluate_predictions takes them
            by_index = sorted((kitti_eval.frame_index(name + '.txt'), name) for name in ds.split_sample_names
                              if kitti_eval.frame_index(name + '.txt') is not None)
            dets = []
            for _, name in by_index:
                r, c = per_frame.get(name, (np.zeros((0, kitti_eval.FIELDS)), np.zeros(0, np.int64)))
                dets.append(kitti_eval.Frame([kitti_eval.class_code(ds.classes[int(k)]) for k in c], r))
            gt = []
            for idx, _ in by_index:
                path = os.path.join(ds.kitti_label_dir, '%06d.txt' % idx)
                if not os.path.exists(path):
                    raise FileNotFoundError('ground truth of frame %06d is missing: %s' % (idx, path))
                gt.append(kitti_eval.parse_label_file(path, detections=False))
            result['kitti'] = kitti_eval.evaluate(gt, dets, self.iou, ds.device)
            result['report'] = kitti_eval.format_report(result['kitti'], global_step)
            if self.ap_slices is not None:
                result['kitti_slices'] = kitti_eval.evaluate_sliced(gt, dets, device=ds.device, **self.ap_slices)
                if self.predictions_base_dir is not None:
                    report_dir = os.path.join(self.predictions_base_dir, 'kitti_reports', ds.data_split)
                    os.makedirs(report_dir, exist_ok=True)
                    path = os.path.join(report_dir, '%08d_slices.txt' % (global_step or 0))
                    with open(path, 'w') as f:
                        f.write(kitti_eval.format_sliced_report(result['kitti_slices'], global_step))
                    result['kitti_slices_report'] = path
                    result['ap_slices_csv'] = evaluator_utils.save_ap_slices(
                        self.predictions_base_dir, ds.data_split, global_step, result['kitti_slices'])
        return result

    def restore_checkpoint(self, path, width_div=1):
        """Restores the model's weights from a checkpoint (a TensorFlow V2 prefix, its directory, or an .npz) through
        checkpoint_utils.  -> the checkpoint's global step, or None."""
        from monopsr_amd.core import checkpoint_utils, device_net
        from monopsr_amd.core import weights as W
        checkpoint = checkpoint_utils.load_checkpoint(path)
        weights = W.synthetic_weights(seed=0, width_div=width_div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE))
        restored = checkpoint_utils.restore_monopsr_weights(weights, checkpoint)
        missing = sorted(set(weights) - set(restored))
        if missing:
            raise ValueError('checkpoint %s lacks %d variables, the first: %s' % (path, len(missing), missing[0]))
        self.model.device_net = device_net.DeviceNet(weights, device=self.dataset.device, width_div=width_div,
                                                     full_trunk=True)
        step = checkpoint.get('global_step')
        return None if step is None else int(np.asarray(step))

    def run_checkpoint_once(self, path, width_div=1):
        """restore_checkpoint, then run_once at the checkpoint's global step."""
        return self.run_once(self.restore_checkpoint(path, width_div=width_div))

    # ---- sweeps over a checkpoint directory

    def _evaluated_path(self):
        return os.path.join(self.predictions_base_dir, 'evaluated_%s.txt' % self.dataset.data_split)

    def get_evaluated_ckpts(self):
        """The steps <predictions_base_dir>/evaluated_<split>.txt lists, as a set."""
        path = self._evaluated_path()
        if not os.path.exists(path):
            return set()
        with open(path) as f:
            return {int(line) for line in f.read().split()}

    def _run_and_record(self, step, prefix, width_div):
        result = self.run_checkpoint_once(prefix, width_div=width_div)
        base = self.predictions_base_dir
        if result.get('report') is not None:
            report_dir = os.path.join(base, 'kitti_reports', self.dataset.data_split)
            os.makedirs(report_dir, exist_ok=True)
            with open(os.path.join(report_dir, '%08d_%s.txt' % (step, self.iou)), 'w') as f:
                f.write(result['report'])
        os.makedirs(base, exist_ok=True)
        with open(self._evaluated_path(), 'a') as f:
            f.write('%d\n' % step)
        return result

    def _sweep_setup(self, width_div):
        if self.predictions_base_dir is None:
            raise ValueError('a checkpoint sweep needs predictions_base_dir: the evaluated steps, the reports and the '
                             'metrics CSVs are kept there')
        evaluated = self.get_evaluated_ckpts() if self.skip_evaluated_checkpoints else set()
        return evaluated, lambda step, prefix: self._run_and_record(step, prefix, width_div)

    def run_latest_checkpoints(self, checkpoint_dir, ckpt_indices=None, width_div=1):
        """Evaluates the checkpoints `<name>-<step, 8 digits>` of a directory (sweep_checkpoints): None = every one not
        yet evaluated (evaluated_<split>.txt, with skip_evaluated_checkpoints), in step order; -1 = the latest;
        otherwise the listed steps (KeyError for a step that is not there).  After each: its report into
        <predictions_base_dir>/kitti_reports/<split>/<step>_<iou>.txt and its step appended to evaluated_<split>.txt.
        -> [run_checkpoint_once's results]."""
        from monopsr_amd.core import checkpoint_utils
        evaluated, run = self._sweep_setup(width_div)
        return sweep_checkpoints(checkpoint_utils.list_checkpoints(checkpoint_dir), evaluated, run, ckpt_indices)

    def repeated_checkpoint_run(self, checkpoint_dir, max_iterations, eval_wait_interval=30, max_idle_seconds=None,
                                width_div=1):
        """run_latest_checkpoints again and again next to a running trainer (repeated_sweep): returns once a checkpoint
        of step >= max_iterations has been evaluated, or after max_idle_seconds without a new one (None: waits for
        ever, as the reference does)."""
        from monopsr_amd.core import checkpoint_utils
        evaluated, run = self._sweep_setup(width_div)
        return repeated_sweep(lambda: checkpoint_utils.list_checkpoints(checkpoint_dir), evaluated, run,
                              max_iterations, eval_wait_interval, max_idle_seconds)


def centroid_fit_options(ap, args):
    """The Evaluator's centroid_fit of a command line's --fit-centroids and --fit-viewing-angle (None without
    --fit-centroids); run_inference and run_evaluation share it."""
    if args.fit_viewing_angle and not args.fit_centroids:
        ap.error('--fit-viewing-angle requires --fit-centroids')
    return dict(fit_viewing_angle=args.fit_viewing_angle) if args.fit_centroids else None


def add_breakdown_arguments(ap):
    """run_evaluation's --breakdown, --depth-edges and --box-iou-edges."""
    ap.add_argument('--breakdown', action='store_true',
                    help='also score every predicted box against its own label and split every per-object table by '
                         'depth, KITTI difficulty and the IoU of the fed 2-D box (DESIGN.md section 7.11)')
    ap.add_argument('--depth-edges', type=float, nargs='+', default=None, metavar='M',
                    help='the depth bins\' edges in metres (default 10 20 30 40 50)')
    ap.add_argument('--box-iou-edges', type=float, nargs='+', default=None, metavar='V',
                    help='the edges of the fed box\'s IoU bins (default 0.7 0.8 0.9)')


def breakdown_options(ap, args):
    """The Evaluator's breakdown of a command line's --breakdown, --depth-edges and --box-iou-edges (None without
    --breakdown)."""
    edges = {k: v for k, v in (('depth_edges', args.depth_edges), ('box_iou_edges', args.box_iou_edges))
             if v is not None}
    if edges and not args.breakdown:
        ap.error('--depth-edges and --box-iou-edges require --breakdown')
    return edges if args.breakdown else None


def add_shape_metrics_arguments(ap):
    """run_evaluation's --shape-metrics, --shape-thresholds and --shape-placed."""
    ap.add_argument('--shape-metrics', action='store_true',
                    help='also score every predicted instance map against the ground-truth map over the valid points: '
                         'accuracy, completeness, Chamfer-L1, Hausdorff, F-score (DESIGN.md section 7.14)')
    ap.add_argument('--shape-thresholds', type=float, nargs='+', default=None, metavar='M',
                    help='the distance thresholds of precision / recall / F-score in metres (default 0.05 0.1 0.2)')
    ap.add_argument('--shape-placed', action='store_true',
                    help='--shape-metrics: also in the camera frame, the maps placed with the predicted (or fitted) '
                         'centroid')


def shape_metrics_options(ap, args):
    """The Evaluator's shape_metrics of a command line's --shape-metrics, --shape-thresholds and --shape-placed (None
    without --shape-metrics)."""
    if (args.shape_thresholds is not None or args.shape_placed) and not args.shape_metrics:
        ap.error('--shape-thresholds and --shape-placed require --shape-metrics')
    if not args.shape_metrics:
        return None
    options = dict(placed=args.shape_placed)
    if args.shape_thresholds is not None:
        from monopsr_amd.core import distance_metrics
        try:
            options['thresholds'] = distance_metrics.check_thresholds(args.shape_thresholds)
        except ValueError as e:
            ap.error('--shape-thresholds: %s' % e)
    return options


def add_shape_surface_arguments(ap):
    """run_evaluation's --shape-surface-metrics, --shape-surface-thresholds, --shape-max-edge and
    --shape-surface-placed."""
    ap.add_argument('--shape-surface-metrics', action='store_true',
                    help='also score every predicted instance map against the ground-truth map as surfaces: the '
                         'distance of a point to the other map\'s triangles, not to its nearest point (DESIGN.md '
                         'section 7.15)')
    ap.add_argument('--shape-surface-thresholds', type=float, nargs='+', default=None, metavar='M',
                    help='the distance thresholds of precision / recall / F-score in metres (default 0.05 0.1 0.2)')
    ap.add_argument('--shape-max-edge', type=float, default=None, metavar='M',
                    help='--shape-surface-metrics: the longest 3-D edge of a triangle in metres (default 0.5; inf '
                         'keeps every triangle of valid points, 0 none)')
    ap.add_argument('--shape-surface-placed', action='store_true',
                    help='--shape-surface-metrics: also in the camera frame, the maps placed with the predicted (or '
                         'fitted) centroid')


def shape_surface_options(ap, args):
    """The Evaluator's shape_surface_metrics of a command line's --shape-surface-metrics, --shape-surface-thresholds,
    --shape-max-edge and --shape-surface-placed (None without --shape-surface-metrics)."""
    if (args.shape_surface_thresholds is not None or args.shape_max_edge is not None or args.shape_surface_placed) \
            and not args.shape_surface_metrics:
        ap.error('--shape-surface-thresholds, --shape-max-edge and --shape-surface-placed require '
                 '--shape-surface-metrics')
    if not args.shape_surface_metrics:
        return None
    from monopsr_amd.core import distance_metrics
    options = dict(placed=args.shape_surface_placed)
    try:
        if args.shape_surface_thresholds is not None:
            options['thresholds'] = distance_metrics.check_thresholds(args.shape_surface_thresholds)
        if args.shape_max_edge is not None:
            options['max_edge'] = distance_metrics.check_max_edge(args.shape_max_edge)
    except ValueError as e:
        ap.error('--shape-surface-metrics: %s' % e)
    return options


def add_ap_slices_arguments(ap):
    """run_evaluation's --ap-slices, --ap-depth-edges and --ap-ious."""
    ap.add_argument('--ap-slices', action='store_true',
                    help='also KITTI AP per IoU set and depth bin in one pass (DESIGN.md section 7.12)')
    ap.add_argument('--ap-depth-edges', type=float, nargs='+', default=None, metavar='M',
                    help='the AP depth bins\' edges in metres (default 10 20 30 40 50)')
    ap.add_argument('--ap-ious', nargs='+', default=None, choices=sorted(kitti_eval.MIN_OVERLAP, reverse=True),
                    help='the IoU sets of the AP slices (default standard low)')


def ap_slices_options(ap, args):
    """The Evaluator's ap_slices of a command line's --ap-slices, --ap-depth-edges and --ap-ious (None without
    --ap-slices)."""
    given = {k: v for k, v in (('depth_edges', args.ap_depth_edges), ('ious', args.ap_ious)) if v is not None}
    if given and not args.ap_slices:
        ap.error('--ap-depth-edges and --ap-ious require --ap-slices')
    if not args.ap_slices:
        return None
    try:
        kitti_eval.slice_table(given.get('ious', _AP_SLICES_OPTIONS['ious']),
                               given.get('depth_edges', _AP_SLICES_OPTIONS['depth_edges']))
    except ValueError as e:
        ap.error(str(e))
    return given


def format_centroid_fit(c):
    """result['centroid_fit'] as one line.  The first error is the objective at the fit's start, the predicted centroid
    moved onto its viewing ray (fit_centroids' x0): not the error of the unfitted scene."""
    return '%d converged, %d at the cap, %d not fitted; mean projection error %.4f (at the start) -> %.4f px' % (
        c['converged'], c['capped'], c['not_fitted'], c['mean_err0'], c['mean_err'])


def build_parser():
    ap = argparse.ArgumentParser(description='KITTI AP of one checkpoint on a split, with MSCNN 2-D detections')
    ap.add_argument('config', help='experiment config (yaml)')
    ap.add_argument('checkpoint', help='checkpoint prefix, directory or .npz')
    ap.add_argument('--mscnn-dir', required=True, help='MSCNN detections in KITTI label format, one file per frame')
    ap.add_argument('--data-split', default='val')
    ap.add_argument('--low-iou', action='store_true', help='MIN_OVERLAP 0.5 / 0.25 / 0.25')
    ap.add_argument('--predictions-dir', default=None, help='also write the KITTI label files under this directory')
    ap.add_argument('--width-div', type=int, default=1, help='channel divisor of the net the checkpoint was saved from')
    ap.add_argument('--fit-centroids', action='store_true',
                    help='fit every predicted centroid to its 2-D box before scoring (DESIGN.md section 7.10)')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    from monopsr_amd.core import config_utils
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    from monopsr_amd.datasets.kitti.kitti_dataset import KittiDataset
    cfg = config_utils.parse_yaml_config(args.config)
    cfg.dataset_config.data_split = args.data_split
    cfg.dataset_config.use_mscnn_detections = True
    dataset = KittiDataset(cfg.dataset_config, 'val', mscnn_label_dir=args.mscnn_dir)
    model = MonoPSRModel(cfg.model_config, cfg.dataset_config, None, 'test')
    threshold = getattr(cfg.get('train_config'), 'kitti_score_threshold', 0.1)
    ev = Evaluator(model, dataset, score_threshold=threshold, predictions_base_dir=args.predictions_dir,
                   iou='low' if args.low_iou else 'standard', centroid_fit={} if args.fit_centroids else None)
    result = ev.run_checkpoint_once(args.checkpoint, width_div=args.width_div)
    sys.stdout.write(result['report'])
    for key, value in sorted(result.get('centroid_fit', {}).items()):
        sys.stdout.write('centroid_fit %s: %s\n' % (key, value))
    for key, value in sorted(result['metrics'].items()) + sorted(result['losses'].items()):
        sys.stdout.write('%s: %.6f\n' % (key, value))
    return 0


if __name__ == '__main__':
    sys.exit(main())

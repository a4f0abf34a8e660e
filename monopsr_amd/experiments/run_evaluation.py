"""Scores the checkpoints of a directory on a split with MSCNN 2-D detections: KITTI AP and the per-object error
statistics, one row per checkpoint (the reference's experiments/run_evaluation.py over Evaluator.run_latest_checkpoints /
repeated_checkpoint_run).

    python -m monopsr_amd.experiments.run_evaluation CONFIG --checkpoint-dir DIR --mscnn-dir DIR --predictions-dir DIR

Under --predictions-dir: kitti_predictions_3d/ (the label files), metrics/<split>/metrics_{avg,std,avg_abs,std_abs}_<split>.csv,
kitti_reports/<split>/<step>_<iou>.txt and evaluated_<split>.txt, which a later run reads to skip what is done.
With --scene-metrics every checkpoint's reconstructed scenes are also scored against the LiDAR depth maps and the
instance images (mask IoU, precisions, depth error: DESIGN.md section 7.8): six more lines per checkpoint and
metrics/<split>/scene_metrics_<split>.csv.  --surface-metrics implies that and also renders the instance maps as
surfaces and scores those: six more lines and metrics/<split>/surface_metrics_<split>.csv.
With --breakdown every predicted box is also set against its own label (image, BEV and 3-D IoU, centre distance, hit
rates) and every per-object table is split by the label's depth (--depth-edges), its KITTI difficulty and the IoU of the
fed 2-D box (--box-iou-edges): the overall overlap lines per checkpoint and, in long format,
metrics/<split>/breakdown_<split>.csv.
With --ap-slices KITTI AP is also computed per IoU set (--ap-ious, default both) and depth bin (--ap-depth-edges, default
10 .. 50 m) in one pass over the same frames: kitti_reports/<split>/<step>_slices.txt and, in long format,
metrics/<split>/ap_slices_<split>.csv.
With --shape-metrics every predicted instance map is also scored against the ground-truth map over the valid points
only (accuracy, completeness, Chamfer-L1, squared Chamfer and Hausdorff in metres, precision / recall / F-score at
--shape-thresholds, default 0.05 0.1 0.2 m): one line per metric and checkpoint after the report and
metrics/<split>/shape_metrics_<split>.csv; with --shape-placed the same in the camera frame, the maps placed with the
predicted (or, with --fit-centroids, fitted) centroid: placed_metrics_<split>.csv.
With --shape-surface-metrics the same scores with the distance of a point taken to the other map's triangulated surface
(triangles with a 3-D edge longer than --shape-max-edge, default 0.5 m, are left out), at --shape-surface-thresholds:
shape_surface_metrics_<split>.csv and, with --shape-surface-placed, placed_surface_metrics_<split>.csv (DESIGN.md
section 7.15).
"""
import argparse
import sys

from monopsr_amd.core import evaluator


def build_parser():
    ap = argparse.ArgumentParser(description='KITTI AP and metric statistics of the checkpoints of a directory')
    ap.add_argument('config', help='experiment config (yaml)')
    ap.add_argument('--checkpoint-dir', required=True, help='directory of <name>-<step, 8 digits> checkpoints')
    ap.add_argument('--mscnn-dir', required=True, help='MSCNN detections in KITTI label format, one file per frame')
    ap.add_argument('--predictions-dir', required=True, help='where the label files, CSVs and reports are written')
    ap.add_argument('--data-split', default='val')
    ap.add_argument('--ckpt-indices', type=int, nargs='+', default=None,
                    help='steps to evaluate (-1: the latest); default: every checkpoint not yet evaluated')
    ap.add_argument('--repeat', action='store_true', help='keep watching the directory for new checkpoints')
    ap.add_argument('--wait-interval', type=float, default=30.0, help='seconds between two looks (--repeat)')
    ap.add_argument('--max-idle', type=float, default=None,
                    help='stop after this many seconds without a new checkpoint (--repeat; default: never)')
    ap.add_argument('--width-div', type=int, default=1, help='channel divisor of the net the checkpoints were saved from')
    ap.add_argument('--low-iou', action='store_true', help='MIN_OVERLAP 0.5 / 0.25 / 0.25')
    ap.add_argument('--scene-metrics', action='store_true',
                    help='also score the reconstructed scenes against ground truth: mask IoU and depth error per box')
    ap.add_argument('--surface-metrics', action='store_true',
                    help='the scene metrics, and the same of the instance maps rendered as surfaces')
    ap.add_argument('--fit-centroids', action='store_true',
                    help='fit every predicted centroid to its 2-D box before scoring (DESIGN.md section 7.10)')
    ap.add_argument('--fit-viewing-angle', action='store_true',
                    help='--fit-centroids: fit the viewing angle as well')
    evaluator.add_breakdown_arguments(ap)
    evaluator.add_ap_slices_arguments(ap)
    evaluator.add_shape_metrics_arguments(ap)
    evaluator.add_shape_surface_arguments(ap)
    return ap


def format_result(result):
    """The report of one checkpoint and a line of its four statistics per metric (the scene metrics and then the
    surface metrics and then the shape and placed metrics, where the result has them, in their own order after the
    others)."""
    lines = [result['report'] or '']
    for name, st in sorted(result.get('metric_stats', {}).items()):
        lines.append('%-24s n %6d  mean %12.5f  std %12.5f  mean|x| %12.5f  std|x| %12.5f  dropped %d\n' % (
            name, st['count'], st['mean'], st['std'], st['mean_abs'], st['std_abs'], st['dropped']))
    for name, st in (list(result.get('scene_stats', {}).items()) + list(result.get('surface_stats', {}).items()) +
                     list(result.get('shape_stats', {}).items()) + list(result.get('placed_stats', {}).items()) +
                     list(result.get('shape_surface_stats', {}).items()) +
                     list(result.get('placed_surface_stats', {}).items())):
        lines.append('%-24s n %6d  mean %12.5f  std %12.5f  mean|x| %12.5f  std|x| %12.5f  dropped %d\n' % (
            name, st['count'], st['mean'], st['std'], st['mean_abs'], st['std_abs'], st['dropped']))
    for name, st in result.get('breakdown', {}).get('all', {}).get('object', {}).items():
        lines.append('%-24s n %6d  mean %12.5f  std %12.5f  mean|x| %12.5f  std|x| %12.5f  dropped %d\n' % (
            name, st['count'], st['mean'], st['std'], st['mean_abs'], st['std_abs'], st['dropped']))
    if 'kitti_slices' in result:
        from monopsr_amd.core import kitti_eval
        lines.append(kitti_eval.format_sliced_report(result['kitti_slices'], None))
    if 'centroid_fit' in result:
        lines.append('centroid fit: %s\n' % evaluator.format_centroid_fit(result['centroid_fit']))
    return ''.join(lines)


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    centroid_fit = evaluator.centroid_fit_options(ap, args)
    breakdown = evaluator.breakdown_options(ap, args)
    ap_slices = evaluator.ap_slices_options(ap, args)
    shape_metrics = evaluator.shape_metrics_options(ap, args)
    shape_surface_metrics = evaluator.shape_surface_options(ap, args)
    from monopsr_amd.core import config_utils
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    from monopsr_amd.datasets.kitti.kitti_dataset import KittiDataset
    cfg = config_utils.parse_yaml_config(args.config)
    cfg.dataset_config.data_split = args.data_split
    cfg.dataset_config.use_mscnn_detections = True
    dataset = KittiDataset(cfg.dataset_config, 'val', mscnn_label_dir=args.mscnn_dir)
    model = MonoPSRModel(cfg.model_config, cfg.dataset_config, None, 'test')
    train_config = cfg.get('train_config')
    threshold = getattr(train_config, 'kitti_score_threshold', 0.1)
    ev = evaluator.Evaluator(model, dataset, score_threshold=threshold, predictions_base_dir=args.predictions_dir,
                             iou='low' if args.low_iou else 'standard', metric_stats=True,
                             scene_metrics='surface' if args.surface_metrics else args.scene_metrics,
                             centroid_fit=centroid_fit, breakdown=breakdown, ap_slices=ap_slices,
                             shape_metrics=shape_metrics, shape_surface_metrics=shape_surface_metrics)
    if args.repeat:
        max_iterations = getattr(train_config, 'max_iterations', None)
        if max_iterations is None and args.max_idle is None:
            raise SystemExit('--repeat needs train_config.max_iterations in the config or --max-idle: it would never end')
        results = ev.repeated_checkpoint_run(args.checkpoint_dir, float('inf') if max_iterations is None else max_iterations,
                                             args.wait_interval, args.max_idle, width_div=args.width_div)
    else:
        indices = args.ckpt_indices
        if indices is not None and len(indices) == 1:
            indices = indices[0]
        results = ev.run_latest_checkpoints(args.checkpoint_dir, indices, width_div=args.width_div)
    for result in results:
        sys.stdout.write('step %s\n%s' % (result['global_step'], format_result(result)))
    if not results:
        sys.stdout.write('no checkpoint to evaluate in %s\n' % args.checkpoint_dir)
    return 0


if __name__ == '__main__':
    sys.exit(main())

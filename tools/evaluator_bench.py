"""Frames per second of the two ways to score a split, on a synthetic split of 375 x 1242 frames (tools/dataset_bench.py's)
with synthetic MSCNN detection files (every label's box shifted by a few pixels, one false positive per frame):

  (a) the host path: MonoPSRModel.format_predictions per frame (three blocking copies each), then
      kitti_eval.evaluate_predictions;
  (b) Evaluator.run_once: the boxes stay on the card until one mpsr_kitti_detection_rows launch and one copy;
      --no-metrics leaves out its EMD / Chamfer and loss means, which (a) does not compute: the like-for-like run.

Both run on the same resident KittiDataset in 'val' mode with the detections merged, the same random-weight net
(--width-div) and the same chunk size.  Each is run once to warm up and then timed over --repeats passes; the
device-to-host copies of one pass of each are counted with torch.profiler.  Numbers: DESIGN.md section 7.5.

--metric-stats times mpsr_metric_stats alone with device events on a synthetic table of a full val split (3769 frames
of 32 rows, the Evaluator's ten columns) and ends.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataset_bench  # noqa: E402
from monopsr_amd.core import config_utils, constants, evaluator, kitti_eval  # noqa: E402
from monopsr_amd.datasets.kitti import kitti_dataset, obj_utils  # noqa: E402


def write_detections(top, names, seed=1):
    """mscnn/<name>.txt: the frame's labels shifted by N(0, 2 px) with a score, and one far-off false positive."""
    rng = np.random.default_rng(seed)
    out = os.path.join(top, 'mscnn')
    os.makedirs(out)
    for name in names:
        rows = []
        for o in obj_utils.read_labels(os.path.join(top, 'training', 'label_2'), name):
            d = rng.normal(0, 2.0, 4)
            rows.append('Car -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10 %.4f'
                        % (o.x1 + d[0], o.y1 + d[1], o.x2 + d[2], o.y2 + d[3], rng.uniform(0.2, 1.0)))
        rows.append('Car -1 -1 -10 5.00 5.00 45.00 35.00 -1 -1 -1 -1000 -1000 -1000 -10 0.2500')
        with open(os.path.join(out, name + '.txt'), 'w') as f:
            f.write('\n'.join(rows) + '\n')
    return out


def host_path(model, ds, batch_size, threshold):
    predictions = {name: (np.zeros((0, 9), np.float32), np.zeros((0, 7), np.float32)) for name in ds.split_sample_names}
    with torch.no_grad():
        for a in range(0, ds.num_samples, batch_size):
            samples = ds.get_sample_dict(np.arange(a, min(a + batch_size, ds.num_samples)), epoch=0)
            for s, out in zip(samples, model.build_batch(samples)):
                sample_dict = {constants.SAMPLE_NUM_OBJS: s['num_objs'], constants.SAMPLE_CAM_P: s['cam_p'],
                               constants.SAMPLE_LABEL_SCORES: s['label_scores'],
                               constants.SAMPLE_LABEL_BOXES_2D: s['boxes_2d'], 'image_shape': tuple(s['rgb_image'].shape)}
                pred = model.format_predictions(model.output_types, out, sample_dict)
                predictions[s['sample_name']] = (pred[constants.KEY_BOX_3D], pred[constants.KEY_BOX_2D])
    return kitti_eval.evaluate_predictions(predictions, ds.classes, threshold, ds.kitti_label_dir)


def _is_dtoh(name):
    n = name.lower().replace(' ', '').replace('_', '')
    return 'dtoh' in n or 'devicetohost' in n or 'device->host' in n or 'device->pageable' in n or 'device->pinned' in n


def count_copies(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if _is_dtoh(e.name))


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(repeats):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / repeats


def time_metric_stats(frames=3769, rows_per_frame=32, repeats=20):
    """Mean device time of one mpsr_metric_stats launch (both NaN rules) over `repeats` launches after a warm-up."""
    from monopsr_amd.core import evaluator_utils
    g = torch.Generator(device='cuda').manual_seed(0)
    n = frames * rows_per_frame
    values = torch.randn((n, len(evaluator.COLUMN_METRIC)), device='cuda', generator=g)
    frame = torch.arange(frames, dtype=torch.int32, device='cuda').repeat_interleave(rows_per_frame)
    out = torch.empty((len(evaluator.METRIC_NAMES), 6), dtype=torch.float64, device='cuda')
    for rule, what in ((evaluator_utils.NAN_RULE_FRAME, 'frame rule'), (evaluator_utils.NAN_RULE_ENTRY, 'entry rule')):
        run = lambda: evaluator_utils.metric_stats(values, frame, evaluator.COLUMN_METRIC, len(evaluator.METRIC_NAMES),
                                                   frames, rule, out=out)
        run()
        torch.cuda.synchronize()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(repeats):
            run()
        end.record()
        torch.cuda.synchronize()
        print('mpsr_metric_stats, %d rows x %d columns, %s: %.1f us per launch (device events, mean of %d)'
              % (n, values.shape[1], what, 1e3 * start.elapsed_time(end) / repeats, repeats))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--frames', type=int, default=64)
    p.add_argument('--batch-size', type=int, default=8)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--no-metrics', action='store_true',
                   help='run_once without the EMD / Chamfer metrics and the loss terms: the same work as the host path')
    p.add_argument('--width-div', type=int, default=1, help='channel divisor of the random-weight net (1: full size)')
    p.add_argument('--metric-stats', action='store_true', help='time mpsr_metric_stats on a full-split table and end')
    a = p.parse_args(argv)
    if a.metric_stats:
        time_metric_stats()
        return 0
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    with tempfile.TemporaryDirectory() as top:
        names = dataset_bench.make_split(top, a.frames)
        os.rename(os.path.join(top, 'train.txt'), os.path.join(top, 'val.txt'))
        mscnn = write_detections(top, names)
        dcfg = dataset_bench.config(top)
        dcfg.data_split = 'val'
        cfg = config_utils.default_config()
        ds = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
        net = dn.DeviceNet(W.synthetic_weights(seed=0, width_div=a.width_div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                           width_div=a.width_div, full_trunk=True)
        model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
        ev = evaluator.Evaluator(model, ds, 0.1, batch_size=a.batch_size, compute_metrics=not a.no_metrics,
                                 compute_losses=not a.no_metrics)
        print('split: %d frames, %d kept, %d skipped; net width / %d; chunks of %d'
              % (len(names), ds.num_samples, ds.num_skipped, a.width_div, a.batch_size))
        n = len(names)
        t_host = timed(lambda: host_path(model, ds, a.batch_size, 0.1), a.repeats)
        t_dev = timed(ev.run_once, a.repeats)
        print('(a) format_predictions per frame + evaluate_predictions: %8.1f frames/s  %8.2f ms per frame, %d '
              'device-to-host copies' % (n / t_host, 1e3 * t_host / n,
                                         count_copies(lambda: host_path(model, ds, a.batch_size, 0.1))))
        what = 'boxes and AP only' if a.no_metrics else 'with metric and loss means'
        print('(b) Evaluator.run_once, %s: %8.1f frames/s  %8.2f ms per frame, %d device-to-host copies'
              % (what, n / t_dev, 1e3 * t_dev / n, count_copies(ev.run_once)))
    return 0


if __name__ == '__main__':
    sys.exit(main())

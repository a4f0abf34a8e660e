"""KITTI evaluation timing on a seeded synthetic KITTI-val-sized set (3769 frames, ground truths with DontCare regions,
20-50 detections per frame): `evaluate` end to end, its GPU kernels alone (event-timed around each mpsr_kitti_* call),
and the tests' CPU restatement of the C++ evaluator on a subset of frames.  With --slices also `evaluate_sliced` with
both IoU sets and the default depth edges (14 slices) end to end and per pass, next to `evaluate` called once per slice on
frames rewritten beforehand as DESIGN.md section 7.12 defines a bin.
    python tools/kitti_eval_bench.py [--frames 3769] [--cpu-frames 100] [--repeats 3] [--slices]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monopsr_amd import _lib  # noqa: E402
from monopsr_amd.core import kitti_eval as ke  # noqa: E402

KINDS = ["Car", "Car", "Car", "Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "Truck"]


def synthetic(n_frames, seed=0):
    """(ground-truth texts, detection texts): 2-14 objects and 0-4 DontCare regions per frame; 20-50 detections, the
    perturbed objects first, then false positives."""
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    for _ in range(n_frames):
        g, d = [], []
        for _ in range(rng.integers(2, 15)):
            kind = KINDS[rng.integers(len(KINDS))]
            x1, y1, hgt = rng.uniform(0, 1100), rng.uniform(100, 250), rng.uniform(15, 150)
            l, w, h = rng.uniform(0.5, 4.5), rng.uniform(0.5, 2), rng.uniform(1, 2)
            tx, ty, tz, ry = rng.uniform(-15, 15), rng.uniform(1, 2), rng.uniform(5, 60), rng.uniform(-3, 3)
            g.append("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                     % (kind, rng.choice([0.0, 0.1, 0.3, 0.6]), rng.integers(0, 4), rng.uniform(-3, 3), x1, y1,
                        x1 + hgt * 1.2, y1 + hgt, h, w, l, tx, ty, tz, ry))
            if rng.random() < 0.85:
                d.append("%s -1 -1 %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f"
                         % (kind, rng.uniform(-3, 3), x1 + rng.normal(0, 4), y1 + rng.normal(0, 4),
                            x1 + hgt * 1.2 + rng.normal(0, 4), y1 + hgt + rng.normal(0, 4), h * rng.uniform(0.9, 1.1),
                            w * rng.uniform(0.9, 1.1), l * rng.uniform(0.9, 1.1), tx + rng.normal(0, 0.3),
                            ty + rng.normal(0, 0.1), tz + rng.normal(0, 0.6), ry + rng.normal(0, 0.2),
                            rng.uniform(0, 1)))
        for _ in range(rng.integers(0, 5)):
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
            g.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10"
                     % (x1, y1, x1 + rng.uniform(10, 120), y1 + rng.uniform(10, 60)))
        for _ in range(int(rng.integers(20, 51)) - len(d)):
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
            d.append("%s -1 -1 %.3f %.3f %.3f %.3f %.3f 1.5 1.6 3.9 %.3f 1.7 %.3f %.3f %.3f"
                     % (["Car", "Pedestrian", "Cyclist"][rng.integers(3)], rng.uniform(-3, 3), x1, y1,
                        x1 + rng.uniform(20, 150), y1 + rng.uniform(10, 120), rng.uniform(-15, 15),
                        rng.uniform(5, 60), rng.uniform(-3, 3), rng.uniform(0, 1)))
        gts.append("\n".join(g))
        dets.append("\n".join(d))
    return gts, dets


class KernelTimer(object):
    """Wraps the mpsr_kitti_* bindings so that every call is bracketed by events on the current stream."""
    NAMES = ("mpsr_kitti_overlaps", "mpsr_kitti_match", "mpsr_kitti_stats", "mpsr_kitti_match_slices",
             "mpsr_kitti_stats_slices")

    def __init__(self):
        self.lib = _lib.lib()
        self.events = []
        self.orig = {n: getattr(self.lib, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(self.lib, n, self._wrap(n, self.orig[n]))

    def _wrap(self, name, fn):
        def call(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            st = fn(*args)
            e1.record()
            self.events.append((name, e0, e1))
            return st
        return call

    def take(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.events:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1)
        self.events = []
        return out

    def close(self):
        for n in self.NAMES:
            setattr(self.lib, n, self.orig[n])


def rewritten(gt, dets, lo, hi):
    """Parsed frames as the definition of the bin lo <= z < hi rewrites their label files: a ground truth outside it
    gets occlusion 3, a detection outside it a class nobody evaluates."""
    out_gt, out_det = [], []
    for g, d in zip(gt, dets):
        rows = g.rows.copy()
        rows[~((rows[:, ke.TZ] >= lo) & (rows[:, ke.TZ] < hi)), ke.OCCLUSION] = 3
        out_gt.append(ke.Frame(g.codes, rows))
        codes = d.codes.copy()
        codes[~((d.rows[:, ke.TZ] >= lo) & (d.rows[:, ke.TZ] < hi))] = ke.OTHER
        out_det.append(ke.Frame(codes, d.rows))
    return out_gt, out_det


def time_slices(gt, dets, repeats):
    """evaluate_sliced (both IoU sets x ('all' + the default depth bins)) against one evaluate per slice."""
    from monopsr_amd.core import evaluator_utils as eu
    ious, edges = ("standard", "low"), eu.DEFAULT_DEPTH_EDGES
    table = ke.slice_table(ious, edges)
    t0 = time.perf_counter()
    frames = {}
    for (_, label), lo, hi in table:
        if label not in frames:
            frames[label] = (gt, dets) if lo is None else rewritten(gt, dets, lo, hi)
    print("%d slices; frames rewritten per bin beforehand in %.2f s (not timed below)"
          % (len(table), time.perf_counter() - t0))
    sliced = ke.evaluate_sliced(gt, dets, ious, edges)  # warm-up
    torch.cuda.synchronize()
    timer = KernelTimer()
    try:
        ends, kernels = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            sliced = ke.evaluate_sliced(gt, dets, ious, edges)
            torch.cuda.synchronize()
            ends.append(time.perf_counter() - t0)
            kernels.append(timer.take())
        k = kernels[int(np.argsort(ends)[len(ends) // 2])]
        print("evaluate_sliced end to end: median %.1f ms of %d (min %.1f ms)"
              % (1e3 * float(np.median(ends)), len(ends), 1e3 * min(ends)))
        print("GPU kernels: overlaps %.2f ms, match %.2f ms, stats + frame-order sum %.2f ms (total %.2f ms)"
              % (k["mpsr_kitti_overlaps"], k["mpsr_kitti_match_slices"], k["mpsr_kitti_stats_slices"], sum(k.values())))
        ends, kernels = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            single = {(iou, label): ke.evaluate(*frames[label], iou=iou) for (iou, label), _, _ in table}
            torch.cuda.synchronize()
            ends.append(time.perf_counter() - t0)
            kernels.append(timer.take())
        k = kernels[int(np.argsort(ends)[len(ends) // 2])]
        print("evaluate, %d calls on rewritten frames: median %.1f ms of %d (min %.1f ms)"
              % (len(table), 1e3 * float(np.median(ends)), len(ends), 1e3 * min(ends)))
        print("GPU kernels: overlaps %.2f ms, match %.2f ms, stats + frame-order sum %.2f ms (total %.2f ms)"
              % (k["mpsr_kitti_overlaps"], k["mpsr_kitti_match"], k["mpsr_kitti_stats"], sum(k.values())))
    finally:
        timer.close()
    same = all(ke.format_report(sliced[key]) == ke.format_report(single[key]) for key in single)
    print("the %d reports of both ways are %s" % (len(single), "equal" if same else "DIFFERENT"))
    print(ke.format_sliced_report({key: sliced[key] for key in list(sliced)[:3]}), end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--cpu-frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slices", action="store_true", help="also time evaluate_sliced against one evaluate per slice")
    args = ap.parse_args()
    t0 = time.perf_counter()
    gt_texts, det_texts = synthetic(args.frames)
    gt = [ke.parse_labels(t, False) for t in gt_texts]
    dets = [ke.parse_labels(t, True) for t in det_texts]
    t_parse = time.perf_counter() - t0
    n_det, n_gt = sum(len(d) for d in dets), sum(len(g) for g in gt)
    print("synthetic set: %d frames, %d ground truths, %d detections (generated + parsed in %.2f s)"
          % (args.frames, n_gt, n_det, t_parse))
    ke.evaluate(gt, dets)  # warm-up: library load, kernels, allocator
    torch.cuda.synchronize()
    timer = KernelTimer()
    ends, kernels = [], []
    try:
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            result = ke.evaluate(gt, dets)
            torch.cuda.synchronize()
            ends.append(time.perf_counter() - t0)
            kernels.append(timer.take())
    finally:
        timer.close()
    k = kernels[int(np.argsort(ends)[len(ends) // 2])]
    print("evaluate end to end: median %.1f ms of %d (min %.1f ms)" % (1e3 * float(np.median(ends)), len(ends),
                                                                        1e3 * min(ends)))
    print("GPU kernels: overlaps %.2f ms, match %.2f ms, stats + frame-order sum %.2f ms (total %.2f ms)"
          % (k["mpsr_kitti_overlaps"], k["mpsr_kitti_match"], k["mpsr_kitti_stats"], sum(k.values())))
    print(ke.format_report(result, None), end="")
    if args.slices:
        time_slices(gt, dets, args.repeats)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_kitti_eval as restated
    n = min(args.cpu_frames, args.frames)
    t0 = time.perf_counter()
    restated.restated_evaluate(gt_texts[:n], det_texts[:n])
    t_cpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    ke.evaluate(gt[:n], dets[:n])
    torch.cuda.synchronize()
    t_gpu = time.perf_counter() - t0
    print("CPU restatement (tests/test_kitti_eval.py) on the first %d frames: %.2f s; evaluate on the same: %.1f ms"
          % (n, t_cpu, 1e3 * t_gpu))


if __name__ == "__main__":
    main()

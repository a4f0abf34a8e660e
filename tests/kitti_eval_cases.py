"""The seeded catalogue of label sets the KITTI differential tests run through the native program
(tests/kitti_program.py), the restatement (test_kitti_eval.restated_evaluate) and the GPU evaluator: real and synthetic
frames, difficulty edges, class mixes, assignment corner cases, DontCare overlaps around the thresholds, image IoUs
exactly on a threshold or one ulp from it, frame sizes across the kernels' bitset words, and rotated, nested and
touching boxes for BEV and 3D.  A test helper, not a conftest.

A case is (indices, gt_texts, det_texts): frame index and the label text of both files, one entry per frame."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import test_kitti_eval as R  # noqa: E402  (the restatement's geometry and the fixture)

CLASSES = ("Car", "Pedestrian", "Cyclist")
MIN_OVERLAP = {"standard": (0.7, 0.5, 0.5), "low": (0.5, 0.25, 0.25)}
THRESHOLDS = (0.25, 0.5, 0.7)
GUARD = 1e-9
SYNTHETIC_FRAMES = 300
SIZES = (0, 1, 31, 32, 33, 63, 64, 65, 500, 2000)
MAX_FRAME = 8192


def num(v):
    """A value as text that reads back as the same double (fscanf %lf and float() both round correctly)."""
    return repr(float(v))


def gt_line(kind, trunc, occ, alpha, box2d, h, w, l, tx, ty, tz, ry):
    return " ".join([kind, num(trunc), "%d" % occ, num(alpha)] + [num(v) for v in box2d] +
                    [num(v) for v in (h, w, l, tx, ty, tz, ry)])


def det_line(kind, alpha, box2d, h, w, l, tx, ty, tz, ry, score):
    return " ".join([kind, "-1", "-1", num(alpha)] + [num(v) for v in box2d] +
                    [num(v) for v in (h, w, l, tx, ty, tz, ry, score)])


def dontcare_line(box2d):
    return "DontCare -1 -1 -10 %s -1 -1 -1 -1000 -1000 -1000 -10" % " ".join(num(v) for v in box2d)


def _case(frames, indices=None):
    indices = list(range(len(frames))) if indices is None else list(indices)
    return indices, ["\n".join(g) for g, _ in frames], ["\n".join(d) for _, d in frames]


# ------------------------------------------------------------------------------------------------ real data

def fixture_frames(seed=1):
    """The 13 KITTI label files of tests/golden: every object as a detection of its own class, jittered in one frame
    of two, with scores drawn from a few values (ties inside and across frames)."""
    rng = np.random.default_rng(seed)
    texts = [str(t) for t in R.golden()["label_texts"]]
    dets = []
    for f, text in enumerate(texts):
        out = []
        for line in text.splitlines():
            t = line.split()
            if not t or t[0] == "DontCare":
                continue
            v = [float(x) for x in t[3:15]]
            if f % 2:
                v = [x + rng.normal(0, 0.02 * (1 + abs(x) / 50)) for x in v]
            out.append(det_line(t[0], v[0], v[1:5], v[5], v[6], v[7], v[8], v[9], v[10], v[11],
                                rng.choice([0.3, 0.5, 0.75, 0.9, rng.uniform(0, 1)])))
        dets.append("\n".join(out))
    return list(range(len(texts))), texts, dets


def synthetic_frames(n=SYNTHETIC_FRAMES, seed=7):
    """tools/kitti_eval_bench.py's synthetic set (DontCare regions, 20-50 detections per frame), non-contiguous
    frame numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kitti_eval_bench import synthetic
    gts, dets = synthetic(n, seed)
    return [3 * i + 1 for i in range(n)], gts, dets


# ------------------------------------------------------------------------------------------------ difficulty and classes

def difficulty_edges():
    """Ground-truth heights of exactly 40 and 25 px, one px either side, and fractional ones just either side (the
    double difference y2 - y1 lands on either side of the integer); detection heights that truncate to 40 / 25 or one
    less; occlusion 0-3; truncation 0.15, 0.30, 0.50 and the next double either side."""
    frames = []
    heights = [40.0, 25.0, 41.0, 39.0, 26.0, 24.0, 40.3 - 0.3, 39.9999999, 40.0000001, 24.9999999, 25.0000001]
    truncs = [0.0]
    for t in (0.15, 0.3, 0.5):
        truncs += [np.nextafter(t, 0.0), t, np.nextafter(t, 1.0)]
    k = 0
    for cls in CLASSES:
        g, d = [], []
        for hgt in heights:
            for occ in range(4):
                for tr in truncs[::3] if occ else truncs:
                    x1, y1 = 20.0 + 70 * (k % 16), 100.3 + 130 * (k // 16)
                    k += 1
                    box = (x1, y1, x1 + 50.5, y1 + hgt)
                    g.append(gt_line(cls, tr, occ, 0.3, box, 1.5, 1.6, 3.9, x1 / 10, 1.7, 30 + y1 / 20, 0.2))
                    dh = [40.0, 39.999, 40.9, 25.0, 24.999, 25.7][k % 6]
                    d.append(det_line(cls, 0.35, (x1 + 0.5, y1, x1 + 50.5, y1 + dh), 1.5, 1.6, 3.9, x1 / 10 + 0.05,
                                      1.7, 30 + y1 / 20, 0.25, 0.05 + 0.9 * ((k * 37) % 101) / 101))
        frames.append((g, d))
    return _case(frames, [5, 6, 7])


def class_mix(alpha_off):
    """Car, Pedestrian and Cyclist with Van, Person_sitting, Truck, Tram, Misc and DontCare rows; Cyclist detections
    without any Cyclist ground truth; Tram ground truth with a Tram detection (never evaluated); a Pedestrian
    ground truth class with no detections in one frame.  alpha_off: one detection with alpha = -10, which turns AOS
    off for the whole run."""
    rng = np.random.default_rng(11)
    kinds = ["Car", "Van", "Pedestrian", "Person_sitting", "Truck", "Tram", "Misc", "car", "PEDESTRIAN"]
    frames = []
    for f in range(12):
        g, d = [], []
        for k in range(8):
            kind = kinds[(f + k) % len(kinds)]
            x1, y1, hgt = 30.0 + 140 * k + rng.uniform(0, 20), 120 + rng.uniform(0, 60), rng.uniform(20, 90)
            box = (x1, y1, x1 + hgt * 1.3, y1 + hgt)
            l, w, h = rng.uniform(1, 4.5), rng.uniform(0.6, 2), rng.uniform(1.2, 2)
            tx, tz, ry = -20 + 5 * k + rng.uniform(0, 1), rng.uniform(10, 50), rng.uniform(-3, 3)
            g.append(gt_line(kind, rng.choice([0.0, 0.2, 0.4]), int(rng.integers(0, 3)), rng.uniform(-3, 3), box,
                             h, w, l, tx, 1.7, tz, ry))
            dkind = {"Van": "Car", "Person_sitting": "Pedestrian", "Misc": "Car"}.get(kind, kind)
            if f == 3 and dkind.lower() == "pedestrian":
                continue  # ground truth of a class, no detection of it in this frame
            jit = rng.normal(0, 3, 4)
            d.append(det_line(dkind, rng.uniform(-3, 3), np.add(box, jit), h * 1.02, w * 0.98, l, tx + 0.2, 1.7,
                              tz + 0.3, ry + rng.normal(0, 0.2), rng.uniform(0, 1)))
        g.append(dontcare_line((900.0, 150.0, 1000.0, 220.0)))
        d.append(det_line("Cyclist", 0.5, (500.0 + f, 150.0, 560.0, 230.0), 1.7, 0.6, 1.8, 3.0, 1.7, 20.0, 0.1,
                          0.2 + 0.05 * f))
        frames.append((g, d))
    if alpha_off:
        t = frames[7][1][2].split()
        t[3] = "-10"
        frames[7][1][2] = " ".join(t)
    return _case(frames, [10, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47])


# ------------------------------------------------------------------------------------------------ assignment

def assignment():
    """Score ties inside a frame and across frames; two detections with exactly equal image IoU to one ground truth
    (the first wins the matching pass, the higher score the threshold pass); a detection overlapping an ignored and
    a valid ground truth; a too-small detection that overlaps a ground truth more than a valid one; DontCare regions
    covering exactly, just under and just over each threshold of a detection (criterion 0)."""
    frames = []
    for cls in CLASSES:
        g, d = [], []
        # equal IoU: two detections shifted by 10 px either way (both 9000 / 11000)
        g.append(gt_line(cls, 0.0, 0, 0.1, (100.0, 100.0, 200.0, 200.0), 1.5, 1.6, 3.9, 1.0, 1.7, 20.0, 0.1))
        d.append(det_line(cls, 0.2, (90.0, 100.0, 190.0, 200.0), 1.5, 1.6, 3.9, 1.0, 1.7, 20.0, 0.1, 0.4))
        d.append(det_line(cls, -0.4, (110.0, 100.0, 210.0, 200.0), 1.5, 1.6, 3.9, 1.2, 1.7, 20.0, 0.1, 0.6))
        # ignored (occluded) and valid ground truth, one detection overlapping both
        g.append(gt_line(cls, 0.0, 3, 0.1, (300.0, 100.0, 400.0, 200.0), 1.5, 1.6, 3.9, 5.0, 1.7, 20.0, 0.1))
        g.append(gt_line(cls, 0.0, 0, 0.1, (305.0, 100.0, 405.0, 200.0), 1.5, 1.6, 3.9, 5.2, 1.7, 20.0, 0.1))
        d.append(det_line(cls, 0.1, (302.0, 100.0, 402.0, 200.0), 1.5, 1.6, 3.9, 5.1, 1.7, 20.0, 0.1, 0.5))
        # ties: the same score four times in this frame (and in every frame)
        for k in range(4):
            x = 500.0 + 60 * k
            g.append(gt_line(cls, 0.0, 0, 0.0, (x, 100.0, x + 50, 160.0), 1.5, 1.6, 3.9, 9.0 + 2 * k, 1.7, 25.0, 0.0))
            d.append(det_line(cls, 0.5, (x + 1, 100.0, x + 50, 161.0), 1.5, 1.6, 3.9, 9.0 + 2 * k, 1.7, 25.2, 0.1,
                              0.5))
        # a too-small detection (height 20 < 25) with the larger overlap, then a valid one
        g.append(gt_line(cls, 0.0, 0, 0.0, (800.0, 100.0, 860.0, 121.0), 1.5, 1.6, 3.9, 20.0, 1.7, 30.0, 0.0))
        d.append(det_line(cls, 0.0, (800.0, 100.0, 860.0, 120.0), 1.5, 1.6, 3.9, 20.0, 1.7, 30.0, 0.0, 0.7))
        d.append(det_line(cls, 0.0, (802.0, 100.0, 860.0, 121.0), 1.5, 1.6, 3.9, 20.1, 1.7, 30.0, 0.0, 0.3))
        # DontCare: a 100 x 50 detection covered 0.25 / 0.5 / 0.7 of its area exactly, and 1 px less and more
        for k, cover in enumerate((25.0, 50.0, 70.0)):
            for j, extra in enumerate((-1.0, 0.0, 1.0)):
                x, y = 1000.0 + 120 * j, 300.0 + 80 * k
                g.append(dontcare_line((x, y, x + cover + extra, y + 50)))
                d.append(det_line(cls, 0.0, (x, y, x + 100, y + 50), 1.5, 1.6, 3.9, -10.0 - 3 * j, 1.7, 40.0 + 3 * k,
                                  0.0, 0.8 + 0.05 * j + 0.01 * k))  # above every threshold: never ignored
        frames.append((g, d))
    return _case(frames, [2, 4, 8])


# ------------------------------------------------------------------------------------------------ strict 2D thresholds

def image_iou(a, b):
    """imageBoxOverlap(a = detection, b = ground truth, -1) in the program's operation order, in fp64 (no
    contraction)."""
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(a[2], b[2]), min(a[3], b[3])
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    a_area = (a[2] - a[0]) * (a[3] - a[1])
    b_area = (b[2] - b[0]) * (b[3] - b[1])
    return inter / (a_area + b_area - inter)


def _threshold_pair(rng, target):
    """A (detection, ground truth) pair of 2D boxes with non-integer corners whose image IoU is exactly `target`, or
    None.  Bisection on the detection's x2, then a walk over the neighbouring doubles."""
    gx1, gy1 = rng.uniform(0.5, 3.5), rng.uniform(100, 200)
    g = (gx1, gy1, gx1 + rng.uniform(40, 200), gy1 + rng.uniform(45, 150))
    dy1, dy2 = g[1] + rng.uniform(-3, 3), g[3] + rng.uniform(-3, 3)
    dx1 = g[0] + rng.uniform(-0.4, 0.4)

    def f(x2):
        return image_iou((dx1, dy1, x2, dy2), g)
    lo, hi = dx1 + 1e-3, g[2]
    if not (f(lo) < target < f(hi)):
        return None
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if f(mid) < target:
            lo = mid
        else:
            hi = mid
    x = lo
    for _ in range(64):
        if f(x) == target:
            return (dx1, dy1, x, dy2), g
        x = np.nextafter(x, np.inf)
    return None


def strict_image_thresholds(iou, per_kind=8, seed=3):
    """Per class, detection / ground-truth pairs whose image IoU in fp64 is min_overlap exactly, one ulp above it (true
    positives) and one ulp below (false positives), as the program computes it.  One pair per 2D slot; the 3D boxes of
    each pair are far apart (BEV and 3D overlap 0)."""
    rng = np.random.default_rng(seed)
    frames = []
    for c, cls in enumerate(CLASSES):
        mo = MIN_OVERLAP[iou][c]
        g, d = [], []
        for target in (mo, np.nextafter(mo, 1.0), np.nextafter(mo, 0.0)):
            found = 0
            while found < per_kind:
                pair = _threshold_pair(rng, float(target))
                if pair is None:
                    continue
                db, gb = pair
                assert image_iou(db, gb) == target
                off = 300.0 * len(g)
                db, gb = (db[0] + 0, db[1] + off, db[2], db[3] + off), (gb[0], gb[1] + off, gb[2], gb[3] + off)
                if image_iou(db, gb) != target:  # the vertical shift moved the rounding: draw again
                    continue
                g.append(gt_line(cls, 0.0, 0, 0.5, gb, 1.5, 1.6, 3.9, 2.0 * len(g), 1.7, 20.0, 0.0))
                d.append(det_line(cls, 0.4, db, 1.5, 1.6, 3.9, 2.0 * len(g) - 1, 1.7, 60.0, 0.0,
                                  rng.uniform(0.05, 0.95)))
                found += 1
        frames.append((g, d))
    return _case(frames, [100, 200, 300])


# ------------------------------------------------------------------------------------------------ sizes

def _crowd(rng, n_det, n_gt, dontcare=1):
    g, d = [], []
    objs = []
    for k in range(n_gt):
        cls = CLASSES[k % 3]
        x1, y1, hgt = rng.uniform(0, 1100), rng.uniform(100, 250), rng.uniform(30, 120)
        box = (x1, y1, x1 + hgt * 1.2, y1 + hgt)
        l, w, h = rng.uniform(1, 4.5), rng.uniform(0.5, 2), rng.uniform(1, 2)
        tx, tz, ry = rng.uniform(-15, 15), rng.uniform(5, 60), rng.uniform(-3, 3)
        g.append(gt_line(cls, rng.choice([0.0, 0.2, 0.4]), int(rng.integers(0, 3)), rng.uniform(-3, 3), box,
                         h, w, l, tx, 1.7, tz, ry))
        objs.append((cls, box, h, w, l, tx, tz, ry))
    for k in range(dontcare):
        x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
        g.append(dontcare_line((x1, y1, x1 + rng.uniform(20, 200), y1 + rng.uniform(20, 100))))
    for k in range(n_det):
        if objs and k % 4 == 0:
            cls, box, h, w, l, tx, tz, ry = objs[(k // 4) % len(objs)]
            d.append(det_line(cls, rng.uniform(-3, 3), np.add(box, rng.normal(0, 4, 4)), h, w, l,
                              tx + rng.normal(0, 0.3), 1.7, tz + rng.normal(0, 0.5), ry + rng.normal(0, 0.2),
                              round(rng.uniform(0, 1), 3)))
        else:
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
            d.append(det_line(CLASSES[int(rng.integers(3))], rng.uniform(-3, 3),
                              (x1, y1, x1 + rng.uniform(10, 150), y1 + rng.uniform(10, 120)), 1.5, 1.6, 3.9,
                              rng.uniform(-15, 15), 1.7, rng.uniform(5, 60), rng.uniform(-3, 3),
                              round(rng.uniform(0, 1), 3)))
    return g, d


def sizes(seed=5):
    """Frames of 0, 1, 31, 32, 33, 63, 64, 65, 500 and 2000 detections (the assignment bitsets' word boundaries and
    the LDS layout), frames without ground truth, without detections, with DontCare only; non-contiguous numbers."""
    rng = np.random.default_rng(seed)
    frames = [_crowd(rng, n, 6) for n in SIZES]
    frames.append(_crowd(rng, 40, 0, dontcare=0))  # no ground truth
    frames.append(_crowd(rng, 0, 9))  # no detections
    g, d = _crowd(rng, 20, 0, dontcare=3)  # DontCare only
    frames.append((g, d))
    return _case(frames, [0, 2, 5, 9, 14, 20, 27, 35, 44, 54, 999, 1000, 123456])


def max_frame(seed=9):
    """One frame at the limit of MAX_FRAME detections, next to an ordinary one."""
    rng = np.random.default_rng(seed)
    return _case([_crowd(rng, MAX_FRAME, 12, dontcare=2), _crowd(rng, 30, 5)], [1, 8])


# ------------------------------------------------------------------------------------------------ BEV / 3D rotations

def rotations():
    """Pairs in bird's-eye view: ry of 0, +-pi/2, +-pi and 1e-7 from them; coincident centres rotated by 90 degrees;
    nested boxes; boxes touching along an edge or at a corner; collinear edges; long thin boxes; height ranges that
    touch exactly (3D height term 0).  Every size strictly positive.  Each pair sits 30 m from the next; the 2D boxes
    of a pair match (so the image pass sees true positives as well)."""
    pi = math.pi
    angles = [0.0, pi / 2, -pi / 2, pi, -pi]
    angles += [a + s for a in angles for s in (1e-7, -1e-7)]
    # (gt l w h ty ry, det dl dw dh dx dty dz dry): the detection relative to its ground truth
    pairs = []
    for a in angles:
        pairs.append(((4.0, 1.7, 1.5, 1.7, a), (4.0, 1.7, 1.5, 0.0, 0.0, 0.0, pi / 2)))  # coincident, 90 degrees
        pairs.append(((3.9, 1.6, 1.5, 1.7, a), (3.8, 1.6, 1.45, 0.3, 0.05, 0.2, 0.03)))  # a near match
        pairs.append(((3.9, 1.6, 1.5, 1.7, a), (3.9, 1.6, 1.5, 0.0, 0.0, 0.0, 1e-7)))  # almost identical
    pairs += [
        ((4.0, 2.0, 1.5, 1.7, 0.3), (3.0, 1.5, 1.5, 0.0, 0.0, 0.0, 0.3)),  # nested, area ratio 0.5625
        ((4.0, 2.0, 1.5, 1.7, 0.0), (3.2, 1.7, 1.2, 0.2, -0.1, 0.1, 0.0)),  # nested, shifted
        ((4.0, 2.0, 1.5, 1.7, 0.0), (4.0, 2.0, 1.5, 4.0, 0.0, 0.0, 0.0)),  # touching along an edge
        ((4.0, 2.0, 1.5, 1.7, 0.0), (4.0, 2.0, 1.5, 4.0, 0.0, 2.0, 0.0)),  # touching at a corner
        ((4.0, 2.0, 1.5, 1.7, pi / 2), (4.0, 2.0, 1.5, 0.0, 0.0, 4.0, pi / 2)),  # touching, rotated
        ((4.0, 2.0, 1.5, 1.7, 0.0), (4.0, 2.0, 1.5, 1.3, 0.0, 0.0, 0.0)),  # collinear long edges, shifted along them
        ((4.0, 2.0, 1.5, 1.7, 0.0), (2.2, 2.0, 1.5, 0.9, 0.0, 0.0, 0.0)),  # collinear long edges, nested end
        ((12.0, 0.3, 1.5, 1.7, 0.0), (12.0, 0.3, 1.5, 0.0, 0.0, 0.12, 0.0)),  # long and thin, side by side
        ((12.0, 0.3, 1.5, 1.7, 0.4), (11.0, 0.28, 1.5, 0.1, 0.0, 0.02, 0.41)),  # long and thin, rotated
        ((4.0, 2.0, 1.5, 1.7, 0.0), (4.0, 2.0, 1.5, 0.1, -1.5, 0.0, 0.0)),  # height ranges touch: 3D term 0
        ((4.0, 2.0, 1.5, 1.7, 0.7), (4.0, 2.0, 1.5, 0.1, 1.5, 0.0, 0.7)),  # touching from below
    ]
    frames = []
    for cls in CLASSES:
        g, d = [], []
        for k, ((l, w, h, ty, ry), (dl, dw, dh, dx, dty, dz, dry)) in enumerate(pairs):
            tx, tz = -40.0 + 30.0 * (k % 4), 10.0 + 30.0 * (k // 4)
            x1 = 40.0 * (k % 25)
            box = (x1, 100.0 + 3 * k, x1 + 35.0, 160.0 + 3 * k)
            g.append(gt_line(cls, 0.0, 0, 0.1, box, h, w, l, tx, ty, tz, ry))
            d.append(det_line(cls, 0.1 + dry, box, dh, dw, dl, tx + dx, ty + dty, tz + dz, ry + dry,
                              0.2 + 0.7 * ((k * 13) % len(pairs)) / len(pairs)))
        frames.append((g, d))
    return _case(frames, [3, 33, 333])


# ------------------------------------------------------------------------------------------------ the BEV / 3D guard

def _box(text, det):
    return R.RBox(text, det)


def guard(case):
    """Drops every detection whose fp64 BEV or 3D overlap (restatement; union and criterion 0) with a row of its
    frame lies within GUARD of 0.25, 0.5 or 0.7: the program computes those through the shim, not boost, so a near
    tie there would prove nothing.  Image overlaps are not guarded (the program's own code computes them).  Returns
    (case, number of detections dropped)."""
    indices, gts, dets = case
    out, dropped = [], 0
    for gt_text, det_text in zip(gts, dets):
        gt = [_box(t, False) for t in gt_text.splitlines() if t.split()]
        keep = []
        for line in det_text.splitlines():
            if not line.split():
                continue
            d = _box(line, True)
            rd = 0.5 * math.hypot(d.l, d.w)
            bad = False
            for g in gt:
                if math.hypot(d.t1 - g.t1, d.t3 - g.t3) > rd + 0.5 * math.hypot(g.l, g.w) + 1e-6:
                    continue  # footprints cannot meet
                for fn in (R.r_ground_overlap, R.r_box3d_overlap):
                    for crit in (-1, 0):
                        o = fn(d, g, crit)
                        if any(abs(o - t) <= GUARD for t in THRESHOLDS):
                            bad = True
            if bad:
                dropped += 1
            else:
                keep.append(line)
        out.append("\n".join(keep))
    return (indices, gts, out), dropped


NAMES = ("fixture", "synthetic", "difficulty", "classes", "classes_alpha_off", "assignment", "strict_2d", "sizes",
         "max_frame", "rotations")

_CACHE = {}


def case(name, iou):
    """The named case for an IoU set ('standard' / 'low'), guarded; (indices, gt_texts, det_texts, dropped)."""
    key = (name, iou if name == "strict_2d" else None)
    if key not in _CACHE:
        make = {"fixture": fixture_frames, "synthetic": synthetic_frames, "difficulty": difficulty_edges,
                "classes": lambda: class_mix(False), "classes_alpha_off": lambda: class_mix(True),
                "assignment": assignment, "strict_2d": lambda: strict_image_thresholds(iou), "sizes": sizes,
                "max_frame": max_frame, "rotations": rotations}[name]
        c, dropped = guard(make())
        _CACHE[key] = c + (dropped,)
    return _CACHE[key]

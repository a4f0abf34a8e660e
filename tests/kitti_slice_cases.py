"""What the AP-by-slice tests share: the two text rewrites that define a depth bin's AP for the
unmodified KITTI program, the test edges, the hand-made case "on the edges" and the list of catalogue cases the
comparison runs.  A test helper, not a conftest.

The AP of the bin lo <= z < hi is what the program prints for the same frames after
  * every ground-truth row whose z (token 13) is outside the bin has got occlusion 3 (token 2), and
  * every detection row whose own z is outside the bin has got the class Misc (token 0)."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kitti_eval_cases as C  # noqa: E402

EDGES = (20.0, 35.0)
LABELS = ("<20", "20-35", ">=35")
BOUNDS = ((-math.inf, 20.0), (20.0, 35.0), (35.0, math.inf))
IOUS = ("standard", "low")
SYNTHETIC_CUT = 60

# the catalogue's cases of the comparison (kitti_eval_cases.NAMES without max_frame), then the two of this file
CATALOGUE = ("fixture", "difficulty", "classes", "classes_alpha_off", "assignment", "strict_2d", "sizes", "rotations")
NAMES = CATALOGUE + ("on_the_edges", "synthetic_cut")


def in_bin(z, lo, hi):
    return lo <= z < hi  # False for a NaN


def rewrite_text(text, lo, hi, detections):
    out = []
    for line in text.splitlines():
        tok = line.split()
        if not tok:
            continue
        if not in_bin(float(tok[13]), lo, hi):
            if detections:
                tok[0] = "Misc"
            else:
                tok[2] = "3"
        out.append(" ".join(tok))
    return "\n".join(out)


def rewrite(gt_text, det_text, lo, hi):
    """One frame's label texts as the definition rewrites them for the bin lo <= z < hi."""
    return rewrite_text(gt_text, lo, hi, False), rewrite_text(det_text, lo, hi, True)


def rewrite_case(case, lo, hi):
    indices, gts, dets = case[:3]
    pairs = [rewrite(g, d, lo, hi) for g, d in zip(gts, dets)]
    return indices, [g for g, _ in pairs], [d for _, d in pairs]


def in_bin_counts(case, lo, hi, kind="car"):
    """(ground truths, detections) of a class whose z is in the bin, over the case's frames."""
    _, gts, dets = case[:3]
    count = lambda texts: sum(1 for t in texts for line in t.splitlines()
                              if line.split() and line.split()[0].lower() == kind
                              and in_bin(float(line.split()[13]), lo, hi))
    return count(gts), count(dets)


# ------------------------------------------------------------------------------------------------ on the edges

# Frame 1, the Car ground truths in order: z one double below 20, exactly 20, one above; one below 35, exactly 35, one
# above; their detections a few centimetres away -- (ground truth z, detection z).
EDGE_PAIRS = ((float(np.nextafter(20.0, 0.0)), 20.03), (20.0, 19.97), (float(np.nextafter(20.0, 100.0)), 20.02),
              (float(np.nextafter(35.0, 0.0)), 35.04), (35.0, 34.95), (float(np.nextafter(35.0, 100.0)), 35.03))

# Written out by hand from the rows below: per bin, the in-bin Car ground truths that pass the easy level (n_gt of
# (image, car, easy)) and the in-bin Car detections, over the three frames.
#   <20   : gt 19.99..; det 19.97
#   20-35 : gt 20, 20.0..01, 34.99..; det 20.03, 20.02, 34.95, and the 20 px detection at 34.9
#   >=35  : gt 35, 35.0..01, and the 35.3 one of the small detection; det 35.04, 35.03
# The NaN rows are in no bin; the 20 px detection is below the easy level's 40 px and every level's 25 px.
EDGE_CAR_COUNTS = {"<20": (1, 1), "20-35": (3, 4), ">=35": (3, 2)}


def on_the_edges():
    half_pi = math.pi / 2
    g, d = [], []
    for k, (gz, dz) in enumerate(EDGE_PAIRS):
        x1 = 30.0 + 150.0 * k
        box = (x1, 150.0, x1 + 90.0, 210.0)  # 60 px
        g.append(C.gt_line("Car", 0.0, 0, 0.1, box, 1.5, 1.6, 3.9, -18.0 + 7.0 * k, 1.7, gz, half_pi))
        d.append(C.det_line("Car", 0.12, (x1 + 1.0, 150.5, x1 + 90.0, 210.0), 1.5, 1.6, 3.9, -18.0 + 7.0 * k, 1.7, dz,
                            half_pi + 0.01, 0.3 + 0.1 * k))
    # a Car in the last bin whose only overlapping detection is 20 px high and 40 cm on the other side of the edge:
    # in the last bin that row is a Misc below every level's minimum height -- ignored_det 1, not -1
    g.append(C.gt_line("Car", 0.0, 0, 0.1, (950.0, 150.0, 1040.0, 210.0), 1.5, 1.6, 3.9, 26.0, 1.7, 35.3, half_pi))
    d.append(C.det_line("Car", 0.1, (950.0, 170.0, 1040.0, 190.0), 1.5, 1.6, 3.9, 26.0, 1.7, 34.9, half_pi, 0.85))
    frame1 = (g, d)
    # frame 2: a NaN z in one ground truth and one detection (in no bin); a Pedestrian in the first bin with a
    # 2-D-only detection (z = -1000: the first bin) and one with a full detection
    g = [C.gt_line("Car", 0.0, 0, 0.1, (100.0, 150.0, 190.0, 210.0), 1.5, 1.6, 3.9, -5.0, 1.7, float("nan"), 0.1),
         C.gt_line("Pedestrian", 0.0, 0, 0.2, (400.0, 140.0, 440.0, 230.0), 1.8, 0.6, 0.8, 1.0, 1.7, 15.0, 0.3),
         C.gt_line("Pedestrian", 0.0, 1, 0.2, (600.0, 140.0, 640.0, 230.0), 1.8, 0.6, 0.8, 5.0, 1.7, 16.0, 0.3)]
    d = [C.det_line("Car", 0.1, (300.0, 150.0, 390.0, 210.0), 1.5, 1.6, 3.9, 8.0, 1.7, float("nan"), 0.1, 0.6),
         " ".join(["Pedestrian", "-1", "-1", C.num(0.25)] + [C.num(v) for v in (401.0, 140.0, 440.0, 229.0)] +
                  ["-1", "-1", "-1", "-1000", "-1000", "-1000", "-10", C.num(0.7)]),
         C.det_line("Pedestrian", 0.2, (600.0, 141.0, 640.0, 230.0), 1.8, 0.6, 0.8, 5.05, 1.7, 16.1, 0.3, 0.4)]
    frame2 = (g, d)
    # frame 3: every row in the middle bin
    g, d = [], []
    for k, z in enumerate((25.0, 30.0)):
        x1 = 200.0 + 300.0 * k
        box = (x1, 150.0, x1 + 50.0, 215.0)
        g.append(C.gt_line("Cyclist", 0.0, 0, 0.3, box, 1.7, 0.6, 1.8, -3.0 + 6.0 * k, 1.7, z, 0.2))
        d.append(C.det_line("Cyclist", 0.3, (x1 + 1.0, 150.0, x1 + 50.0, 214.0), 1.7, 0.6, 1.8, -3.0 + 6.0 * k, 1.7,
                            z + 0.1, 0.25, 0.5 + 0.2 * k))
    frames = [frame1, frame2, (g, d)]
    return [4, 9, 12], ["\n".join(g) for g, _ in frames], ["\n".join(d) for _, d in frames]


_CACHE = {}


def case(name, iou):
    """(indices, gt_texts, det_texts, dropped) of a case of NAMES, guarded as the catalogue's are.  Only strict_2d
    depends on `iou`."""
    if name in CATALOGUE:
        return C.case(name, iou)
    if name not in _CACHE:
        if name == "synthetic_cut":
            indices, gts, dets = C.case("synthetic", iou)[:3]
            made = (indices[:SYNTHETIC_CUT], gts[:SYNTHETIC_CUT], dets[:SYNTHETIC_CUT])
        else:
            made = on_the_edges()
        c, dropped = C.guard(made)
        _CACHE[name] = c + (dropped,)
    return _CACHE[name]


def by_index(case_):
    """The case's frames in the order of their index, as the evaluator takes them: (gt_texts, det_texts)."""
    indices, gts, dets = case_[:3]
    order = sorted(range(len(indices)), key=lambda k: indices[k])
    return [gts[k] for k in order], [dets[k] for k in order]

"""KITTI evaluation on the GPU (csrc/kitti_eval.hip through monopsr_amd.core.kitti_eval) against the fp64 restatement
of evaluate_object_3d_offline.cpp in test_kitti_eval.py and against the reference's own Python IoU pins
(tests/golden/kitti_eval.npz)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_kitti_eval as R  # noqa: E402  (the restatement)

pytestmark = pytest.mark.gpu

# three_d_iou rasterises both bases at 1 cm (PIL polygons, outline included): on the fixture's 174 pins it differs
# from the exact overlap by at most 0.0168 (measured with the restatement); the bound below leaves a little room.
RASTER_BOUND_3D = 0.02


def _ke():
    from monopsr_amd.core import kitti_eval as ke
    return ke


def _rows(boxes):
    """[(l, w, h, tx, ty, tz, ry, x1, y1, x2, y2)] -> detection Frame rows of class car."""
    ke = _ke()
    out = np.zeros((len(boxes), ke.FIELDS))
    for k, (l, w, h, tx, ty, tz, ry, x1, y1, x2, y2) in enumerate(boxes):
        out[k, [ke.L, ke.W, ke.H, ke.TX, ke.TY, ke.TZ, ke.RY, ke.X1, ke.Y1, ke.X2, ke.Y2]] = \
            [l, w, h, tx, ty, tz, ry, x1, y1, x2, y2]
    return out


def _overlaps(gt_rows, det_rows):
    """The overlap kernel on one frame: (6, n_det, n_gt)."""
    import ctypes
    import torch
    from monopsr_amd import _lib
    ke = _ke()
    dev = torch.device("cuda", 0)
    nd, ng = len(det_rows), len(gt_rows)
    d = torch.from_numpy(np.ascontiguousarray(det_rows, np.float64)).to(dev)
    g = torch.from_numpy(np.ascontiguousarray(gt_rows, np.float64)).to(dev)
    dc = torch.zeros(nd, dtype=torch.int32, device=dev)
    gc = torch.zeros(ng, dtype=torch.int32, device=dev)
    dof, gof, pof = np.array([0, nd], np.int32), np.array([0, ng], np.int32), np.array([0, nd * ng], np.int64)
    dofd, gofd, pofd = [torch.from_numpy(a).to(dev) for a in (dof, gof, pof)]
    b = _lib.KittiBatch(d.data_ptr(), dc.data_ptr(), g.data_ptr(), gc.data_ptr(), dofd.data_ptr(), gofd.data_ptr(),
                        pofd.data_ptr(), dof.ctypes.data, gof.ctypes.data, pof.ctypes.data, nd, ng, 1)
    out = torch.empty((6, nd * ng), dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().mpsr_kitti_overlaps(ctypes.byref(b), out.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    assert ke.FIELDS == 14
    return out.cpu().numpy().reshape(6, nd, ng)


class _Box(object):
    def __init__(self, row):
        ke = _ke()
        self.x1, self.y1, self.x2, self.y2 = row[ke.X1], row[ke.Y1], row[ke.X2], row[ke.Y2]
        self.h, self.w, self.l = row[ke.H], row[ke.W], row[ke.L]
        self.t1, self.t2, self.t3, self.ry = row[ke.TX], row[ke.TY], row[ke.TZ], row[ke.RY]


def _restated_overlaps(gt_rows, det_rows):
    out = np.zeros((6, len(det_rows), len(gt_rows)))
    for j, dr in enumerate(det_rows):
        for i, gr in enumerate(gt_rows):
            d, g = _Box(dr), _Box(gr)
            for m, fn in enumerate(R.R_OVERLAPS):
                out[m, j, i] = fn(d, g, -1)
                out[m + 3, j, i] = fn(d, g, 0)
    return out


def _random_boxes(rng, n):
    boxes = []
    for _ in range(n):
        x1, y1 = rng.uniform(0, 500), rng.uniform(0, 300)
        boxes.append([rng.uniform(0.3, 6), rng.uniform(0.3, 3), rng.uniform(0.5, 3), rng.uniform(-3, 3),
                      rng.uniform(0, 3), rng.uniform(-3, 3), rng.uniform(-4, 4), x1, y1, x1 + rng.uniform(1, 200),
                      y1 + rng.uniform(1, 150)])
    return boxes


def test_overlap_kernel_matches_the_restatement():
    rng = np.random.default_rng(7)
    special = [
        [2, 1, 1.5, 0, 1, 0, 0.3, 10, 10, 50, 60],            # identical to the next
        [2, 1, 1.5, 0, 1, 0, 0.3, 10, 10, 50, 60],
        [4, 3, 2, 0, 1, 0, 1.1, 0, 0, 100, 100],               # contains the first
        [1, 1, 1, 10, 1, 10, 0, 200, 200, 210, 210],           # disjoint
        [1, 1, 1, 11, 1, 11, 0, 210, 210, 220, 220],           # corner-touching the previous (BEV and image)
        [40, 20, 5, 0, 2, 0, 0.7, 0, 0, 1000, 370],            # very different sizes
        [0.05, 0.04, 0.1, 0.1, 1, 0.1, 2.0, 20, 20, 21, 21],
        [2, 1, 1.5, 0, 1, 0, 0.3 + math.pi / 2, 10, 10, 50, 60],  # rotated by 90 degrees
    ]
    boxes = special + _random_boxes(rng, 40)
    rows = _rows(boxes)
    got = _overlaps(rows, rows)
    want = _restated_overlaps(rows, rows)
    assert np.abs(got - want).max() <= 1e-12
    assert (got[:3, 0, 1] == got[:3, 0, 1]).all() and abs(got[1, 0, 1] - 1) < 1e-12 and abs(got[2, 0, 1] - 1) < 1e-12
    assert got[1, 3, 4] == 0 and got[0, 3, 4] == 0  # corner touching


def test_overlap_known_answers():
    rows = _rows([[1, 1, 1, 0, 1, 0, 0, 0, 0, 10, 10], [1, 1, 1, 0, 1, 0, 0, 0, 0, 10, 10],
                  [1, 1, 1, 0.5, 1, 0, 0, 5, 0, 15, 10], [1, 1, 1, 0, 1, 0, math.pi / 4, 0, 0, 10, 10]])
    o = _overlaps(rows[:1], rows)
    assert np.allclose(o[:3, 1, 0], 1, atol=1e-12, rtol=0)                  # identical boxes
    assert np.allclose(o[:3, 2, 0], 1 / 3, atol=1e-12, rtol=0)              # shifted by half their length
    assert abs(o[1, 3, 0] - 1 / math.sqrt(2)) < 1e-12                       # unit square vs itself rotated 45 deg
    assert abs(o[4, 2, 0] - 0.5) < 1e-12                                    # criterion 0: over the detection's area
    # non-positive dimensions (DontCare rows: -1 -1 -1 at -1000): no BEV / 3D overlap
    dc = _rows([[-1, -1, -1, -1000, -1000, -1000, -10, 0, 0, 10, 10]])
    o = _overlaps(dc, rows[:1])
    assert (o[[1, 2, 4, 5]] == 0).all() and o[3, 0, 0] == 1


def test_reference_pins():
    g = R.golden()
    ke = _ke()
    a, b = g["pin2d_a"], g["pin2d_b"]
    ra = np.zeros((len(a), ke.FIELDS))
    rb = np.zeros((len(b), ke.FIELDS))
    ra[:, [ke.X1, ke.Y1, ke.X2, ke.Y2]] = a
    rb[:, [ke.X1, ke.Y1, ke.X2, ke.Y2]] = b
    got = np.array([_overlaps(ra[k:k + 1], rb[k:k + 1])[0, 0, 0] for k in range(len(a))])
    assert np.abs(got - g["pin2d_iou"]).max() <= 1e-12
    a3, b3 = g["pin3d_a"], g["pin3d_b"]  # [ry, l, h, w, tx, ty, tz]

    def rows3(x):
        r = np.zeros((len(x), ke.FIELDS))
        r[:, [ke.RY, ke.L, ke.H, ke.W, ke.TX, ke.TY, ke.TZ]] = x
        return r
    ra3, rb3 = rows3(a3), rows3(b3)
    got3 = np.array([_overlaps(ra3[k:k + 1], rb3[k:k + 1])[2, 0, 0] for k in range(len(a3))])
    assert np.abs(got3 - g["pin3d_iou"]).max() <= RASTER_BOUND_3D
    assert (got3 > 0).sum() >= 150


# ------------------------------------------------------------------------------------------------ full evaluation

def _det_line(cls, alpha, x1, y1, x2, y2, h, w, l, tx, ty, tz, ry, score):
    return " ".join([cls, "-1", "-1"] + ["%.6f" % v for v in (alpha, x1, y1, x2, y2, h, w, l, tx, ty, tz, ry, score)])


def _gt_as_detections(texts, rng=None, perturb=False):
    out = []
    for text in texts:
        lines = []
        for line in str(text).splitlines():
            t = line.split()
            if not t or t[0] == "DontCare":
                continue
            v = [float(x) for x in t[3:15]]
            score = 1.0 if rng is None else float(rng.uniform(0.05, 1))
            if perturb:
                v[1:5] = list(np.array(v[1:5]) + rng.normal(0, 3, 4))
                v[8] += rng.normal(0, 0.3)
                v[10] += rng.normal(0, 0.5)
                v[11] += rng.normal(0, 0.2)
                v[0] += rng.normal(0, 0.3)
            lines.append(_det_line(t[0], *v, score))
        out.append("\r\n".join(lines) + ("\r\n" if lines else ""))
    return out


def _perturbed_detections(texts, seed):
    rng = np.random.default_rng(seed)
    dets = _gt_as_detections(texts, rng, perturb=True)
    out = []
    for k, (text, det) in enumerate(zip(texts, dets)):
        lines = [x for x in det.splitlines() if x]
        for line in str(text).splitlines():
            t = line.split()
            if not t:
                continue
            v = [float(x) for x in t[3:15]]
            if t[0] == "DontCare":  # a car detection inside a DontCare region
                lines.append(_det_line("Car", 0.1, v[1] + 1, v[2] + 1, v[3] - 1, v[4] - 1, 1.5, 1.6, 3.9,
                                       rng.uniform(-5, 5), 1.7, rng.uniform(10, 40), 0.1, rng.uniform(0.1, 1)))
            if t[0] == "Van":  # a Van labelled as a car
                lines.append(_det_line("Car", *v, float(rng.uniform(0.1, 1))))
        for _ in range(3):  # false positives of every class, some below the minimum height
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 300)
            hgt = rng.choice([10.0, 24.9, 30.0, 39.5, 60.0])
            lines.append(_det_line(rng.choice(["Car", "Pedestrian", "Cyclist", "car", "Van"]), rng.uniform(-3, 3),
                                   x1, y1, x1 + rng.uniform(20, 120), y1 + hgt, 1.5, 1.6, 3.9, rng.uniform(-10, 10),
                                   1.7, rng.uniform(5, 60), rng.uniform(-3, 3), rng.uniform(0, 1)))
        if k == 5:  # one file with an invalid orientation: AOS is not evaluated
            t = lines[0].split()
            t[3] = "-10"
            lines[0] = " ".join(t)
        out.append("\n".join(lines) + "\n")
    return out


def _synthetic(n_frames, seed):
    rng = np.random.default_rng(seed)
    gts, dets = [], []
    kinds = ["Car", "Car", "Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare", "Truck"]
    for _ in range(n_frames):
        g, d = [], []
        for _ in range(rng.integers(0, 6)):
            kind = rng.choice(kinds)
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
            hgt = rng.uniform(15, 120)
            l, w, h = rng.uniform(0.5, 4.5), rng.uniform(0.5, 2), rng.uniform(1, 2)
            tx, ty, tz, ry = rng.uniform(-15, 15), rng.uniform(1, 2), rng.uniform(5, 50), rng.uniform(-3, 3)
            if kind == "DontCare":
                g.append("DontCare -1 -1 -10 %.2f %.2f %.2f %.2f -1 -1 -1 -1000 -1000 -1000 -10"
                         % (x1, y1, x1 + 60, y1 + hgt))
                continue
            g.append("%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f"
                     % (kind, rng.choice([0.0, 0.2, 0.4, 0.8]), rng.integers(0, 4), rng.uniform(-3, 3), x1, y1,
                        x1 + hgt * 1.5, y1 + hgt, h, w, l, tx, ty, tz, ry))
            if rng.random() < 0.8:
                d.append(_det_line(kind if rng.random() < 0.9 else "Car", rng.uniform(-3, 3),
                                   x1 + rng.normal(0, 4), y1 + rng.normal(0, 4), x1 + hgt * 1.5 + rng.normal(0, 4),
                                   y1 + hgt + rng.normal(0, 4), h * rng.uniform(0.9, 1.1), w * rng.uniform(0.9, 1.1),
                                   l * rng.uniform(0.9, 1.1), tx + rng.normal(0, 0.3), ty + rng.normal(0, 0.1),
                                   tz + rng.normal(0, 0.5), ry + rng.normal(0, 0.2), rng.uniform(0, 1)))
        for _ in range(rng.integers(0, 3)):
            x1, y1 = rng.uniform(0, 1100), rng.uniform(100, 250)
            d.append(_det_line(rng.choice(["Car", "Pedestrian", "Cyclist"]), rng.uniform(-3, 3), x1, y1,
                               x1 + 50, y1 + rng.uniform(20, 80), 1.5, 1.6, 3.9, rng.uniform(-15, 15), 1.7,
                               rng.uniform(5, 50), rng.uniform(-3, 3), rng.uniform(0, 1)))
        gts.append("\n".join(g))
        dets.append("\n".join(d))
    return gts, dets


def _check_against_restatement(gt_texts, det_texts, iou):
    ke = _ke()
    result = ke.evaluate([ke.parse_labels(str(t), False) for t in gt_texts],
                         [ke.parse_labels(str(t), True) for t in det_texts], iou=iou)
    curves, lines = R.restated_evaluate([str(t) for t in gt_texts], [str(t) for t in det_texts], iou)
    got = {(c, k): v["curve"] for c, d in result.items() for k, v in d.items()}
    assert sorted(got) == sorted(curves)
    for key in curves:
        assert np.allclose(got[key], curves[key], rtol=0, atol=1e-9, equal_nan=True), key
    assert ke.format_report(result, None).splitlines() == lines
    return result, lines


@pytest.mark.parametrize("iou", ["standard", "low"])
def test_fixture_ground_truth_as_its_own_detections(iou):
    g = R.golden()
    texts = list(g["label_texts"])
    result, lines = _check_against_restatement(texts, _gt_as_detections(texts, np.random.default_rng(1)), iou)
    assert set(result) == {"car", "pedestrian", "cyclist"} and "aos" in result["car"]
    assert "car_detection_3D AP" in "\n".join(lines)


@pytest.mark.parametrize("iou", ["standard", "low"])
def test_fixture_perturbed_detections(iou):
    g = R.golden()
    texts = list(g["label_texts"])
    result, _ = _check_against_restatement(texts, _perturbed_detections(texts, 11), iou)
    assert "aos" not in result["car"]  # one file has alpha -10


@pytest.mark.parametrize("iou", ["standard", "low"])
def test_synthetic_frames(iou):
    gts, dets = _synthetic(300, 5)
    result, _ = _check_against_restatement(gts, dets, iou)
    assert "aos" in result["car"] and "heading_3d" in result["pedestrian"]


def test_three_perfect_cars_give_9_09():
    ke = _ke()
    gt = "\n".join("Car 0.00 0 0.1 100 100 200 200 1.5 1.6 3.9 %d 1.7 20 0.2" % x for x in (-6, 0, 6))
    det = "\n".join(_det_line("Car", 0.1, 100, 100, 200, 200, 1.5, 1.6, 3.9, x, 1.7, 20, 0.2, 0.9) for x in (-6, 0, 6))
    result = ke.evaluate([ke.parse_labels(gt, False)], [ke.parse_labels(det, True)])
    for key in ("image", "aos", "bev", "heading_bev", "3d", "heading_3d"):
        assert "%f" % result["car"][key]["ap11"][0] == "9.090909", key


def test_threshold_without_tp_or_fp_prints_minus_nan():
    """The only threshold (0.5, the score of the car's true positive in the first pass) finds, in the second pass,
    the 0.5 detection taken by the Van (larger overlap, neighbouring class: ignored) and the 0.9 detection inside the
    DontCare region: tp = fp = 0, precision 0.0 / 0.0, printed '-nan' by the C program."""
    gt = "\n".join(["Van 0.00 0 0.1 100 100 200 200 1.5 1.6 3.9 0 1.7 20 0.2",
                    "Car 0.00 0 0.1 100 100 200 210 1.5 1.6 3.9 0 1.7 20 0.2",
                    "DontCare -1 -1 -10 90 80 210 190 -1 -1 -1 -1000 -1000 -1000 -10"])
    det = "\n".join(["Car -1 -1 0.1 100 85 200 185 1.5 1.6 3.9 -1000 -1000 -1000 0.2 0.9",
                     "Car -1 -1 0.1 100 100 200 202 1.5 1.6 3.9 -1000 -1000 -1000 0.2 0.5"])
    result, lines = _check_against_restatement([gt], [det], "standard")
    assert lines == ["car_detection AP: -nan -nan -nan", "car_orientation AP: -nan -nan -nan"]


def test_round_trip_predictions_equal_exported_label_files(tmp_path):
    from monopsr_amd.core import evaluator_utils as eu
    ke = _ke()
    g = R.golden()
    gt_dir = tmp_path / "label_2"
    gt_dir.mkdir()
    rng = np.random.default_rng(2)
    classes = ["Car", "Pedestrian", "Cyclist"]
    predictions = {}
    for name, text in zip(g["label_names"], g["label_texts"]):
        (gt_dir / str(name)).write_bytes(str(text).encode())
        b3, b2 = [], []
        for line in str(text).splitlines():
            t = line.split()
            if not t or t[0] not in classes:
                continue
            v = [float(x) for x in t[3:15]]
            score = rng.uniform(0, 1)
            k = classes.index(t[0])
            b3.append([v[8] + rng.normal(0, 0.2), v[9], v[10] + rng.normal(0, 0.4), v[7], v[6], v[5],
                       v[11] + rng.normal(0, 0.1), score, k])
            b2.append([v[2] + rng.normal(0, 2), v[1] + rng.normal(0, 2), v[4] + rng.normal(0, 2),
                       v[3] + rng.normal(0, 2), v[0] + rng.normal(0, 0.2), score, k])
        predictions[str(name)[:-4]] = (np.array(b3).reshape(-1, 9), np.array(b2).reshape(-1, 7))
    out_dir = tmp_path / "120000"
    eu.export_kitti_labels(predictions, classes, 0.3, str(out_dir / "data"))
    a = ke.evaluate_predictions(predictions, classes, 0.3, str(gt_dir))
    b = ke.evaluate_dirs(str(gt_dir), str(out_dir))
    assert ke.format_report(a, "120000") == ke.format_report(b, "120000")
    for c in b:
        for k in b[c]:
            assert np.array_equal(a[c][k]["curve"], b[c][k]["curve"])
    # the command line prints the same report, the step line being the result directory's name
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output([sys.executable, "-m", "monopsr_amd.core.kitti_eval", str(gt_dir), str(out_dir)],
                                  cwd=root, env=dict(os.environ, PYTHONPATH=root)).decode()
    assert out == ke.format_report(b, "120000")
    # a frame whose ground truth is missing
    eu.write_kitti_label_file(str(out_dir / "data" / "000999.txt"), [])
    with pytest.raises(FileNotFoundError):
        ke.evaluate_dirs(str(gt_dir), str(out_dir))


def test_errors_and_empty_detections():
    from monopsr_amd import _lib
    ke = _ke()
    g = R.golden()
    gt = [ke.parse_labels(str(t), False) for t in g["label_texts"]]
    empty = [ke.Frame(np.zeros(0, np.int32), np.zeros((0, ke.FIELDS))) for _ in gt]
    assert ke.evaluate(gt, empty) == {}
    assert ke.format_report(ke.evaluate(gt, empty), "0") == "0\n"
    n = ke.MAX_DETECTIONS_PER_FRAME + 1
    rows = np.tile(_rows([[1.6, 3.9, 1.5, 0, 1.7, 20, 0, 100, 100, 200, 200]]), (n, 1))
    rows[:, ke.SCORE] = np.linspace(0, 1, n)
    big = [ke.Frame(np.zeros(n, np.int32), rows)]
    with pytest.raises(_lib.InvalidArgumentError, match="8192"):
        ke.evaluate(gt[:1], big)

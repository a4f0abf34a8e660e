"""KITTI evaluation, CPU side: the label parser, getThresholds, AP11 / AP40, the report format and the host-side
argument checks of the mpsr_kitti_* entry points (they load without a GPU).

This module also holds the checker the GPU tests (test_kitti_eval_gpu.py) compare against: `restated_evaluate`, an
independent fp64 numpy restatement of evaluate_object_3d_offline.cpp -- a straight loop port of cleanData /
computeStatistics / eval_class with half-plane clipping for the bird's-eye-view overlap.  It takes frames as
(class names, rows) straight from the label text, so it shares nothing with monopsr_amd.core.kitti_eval."""
import ctypes
import math
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz")

# ---------------------------------------------------------------------------------------------------- restatement

R_CLASSES = ("car", "pedestrian", "cyclist")
R_MIN_HEIGHT = (40, 25, 25)
R_MAX_OCCLUSION = (0, 1, 2)
R_MAX_TRUNCATION = (0.15, 0.3, 0.5)
R_MIN_OVERLAP = {"standard": (0.7, 0.5, 0.5), "low": (0.5, 0.25, 0.25)}


class RBox(object):
    """One label line, field names as in tBox / tGroundtruth / tDetection."""

    def __init__(self, line, det):
        t = line.split()
        self.type = t[0]
        v = [float(x) for x in t[1:]]
        self.truncation, self.occlusion = v[0], int(t[2])
        self.alpha, self.x1, self.y1, self.x2, self.y2 = v[2:7]
        self.h, self.w, self.l, self.t1, self.t2, self.t3, self.ry = v[7:14]
        self.thresh = v[14] if det else -1000


def r_parse(text, det):
    return [RBox(line, det) for line in text.splitlines() if line.split()]


def r_image_overlap(a, b, criterion=-1):
    x1, y1, x2, y2 = max(a.x1, b.x1), max(a.y1, b.y1), min(a.x2, b.x2), min(a.y2, b.y2)
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    a_area = (a.x2 - a.x1) * (a.y2 - a.y1)
    b_area = (b.x2 - b.x1) * (b.y2 - b.y1)
    return inter / (a_area + b_area - inter) if criterion == -1 else inter / a_area


def r_polygon(g):
    c, s = math.cos(g.ry), math.sin(g.ry)
    xs = (g.l / 2, g.l / 2, -g.l / 2, -g.l / 2)
    zs = (g.w / 2, -g.w / 2, -g.w / 2, g.w / 2)
    return [(c * x + s * z + g.t1, -s * x + c * z + g.t3) for x, z in zip(xs, zs)]


def r_area(poly):
    a = 0.0
    for i in range(len(poly)):
        (x0, z0), (x1, z1) = poly[i], poly[(i + 1) % len(poly)]
        a += x0 * z1 - x1 * z0
    return abs(a) / 2


def r_clip(subject, clip):
    """Sutherland-Hodgman: `subject` clipped by every edge's half-plane of the convex polygon `clip`."""
    turn = 0.0
    for i in range(len(clip)):
        (x0, z0), (x1, z1) = clip[i], clip[(i + 1) % len(clip)]
        turn += x0 * z1 - x1 * z0
    sign = -1.0 if turn < 0 else 1.0
    out = list(subject)
    for e in range(len(clip)):
        (ax, az), (bx, bz) = clip[e], clip[(e + 1) % len(clip)]
        ex, ez = bx - ax, bz - az
        pts, out = out, []
        for i in range(len(pts)):
            (px, pz), (qx, qz) = pts[i], pts[(i + 1) % len(pts)]
            sp = sign * (ex * (pz - az) - ez * (px - ax))
            sq = sign * (ex * (qz - az) - ez * (qx - ax))
            if sp >= 0:
                out.append((px, pz))
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                out.append((px + t * (qx - px), pz + t * (qz - pz)))
        if not out:
            break
    return out


def r_bev_inter(d, g):
    dp, gp = r_polygon(d), r_polygon(g)
    inter = r_clip(dp, gp)
    return (r_area(inter) if len(inter) >= 3 else 0.0), r_area(dp), r_area(gp)


def r_ground_overlap(d, g, criterion=-1):
    if not (d.l > 0 and d.w > 0 and g.l > 0 and g.w > 0):
        return 0.0
    inter, ad, ag = r_bev_inter(d, g)
    return inter / (ad + ag - inter) if criterion == -1 else inter / ad


def r_box3d_overlap(d, g, criterion=-1):
    if not (d.l > 0 and d.w > 0 and d.h > 0 and g.l > 0 and g.w > 0 and g.h > 0):
        return 0.0
    inter, _, _ = r_bev_inter(d, g)
    ymax, ymin = min(d.t2, g.t2), max(d.t2 - d.h, g.t2 - g.h)
    iv = inter * max(0.0, ymax - ymin)
    dv, gv = d.h * d.l * d.w, g.h * g.l * g.w
    return iv / (dv + gv - iv) if criterion == -1 else iv / dv


R_OVERLAPS = (r_image_overlap, r_ground_overlap, r_box3d_overlap)


def r_get_thresholds(v, n_gt):
    v = sorted(v, reverse=True)
    t, current = [], 0.0
    for i in range(len(v)):
        l_recall = (i + 1) / n_gt
        r_recall = (i + 2) / n_gt if i < len(v) - 1 else l_recall
        if (r_recall - current) < (current - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current += 1.0 / 40.0
    return t


def r_clean_data(cls, gt, det, diff):
    name = R_CLASSES[cls]
    ign_gt, dc, ign_det, n_gt = [], [], [], 0
    for g in gt:
        height = g.y2 - g.y1
        gtype = g.type.lower()
        if gtype == name:
            valid = 1
        elif (name == "pedestrian" and gtype == "person_sitting") or (name == "car" and gtype == "van"):
            valid = 0
        else:
            valid = -1
        ignore = g.occlusion > R_MAX_OCCLUSION[diff] or g.truncation > R_MAX_TRUNCATION[diff] or \
            height <= R_MIN_HEIGHT[diff]
        if valid == 1 and not ignore:
            ign_gt.append(0)
            n_gt += 1
        elif valid == 0 or (ignore and valid == 1):
            ign_gt.append(1)
        else:
            ign_gt.append(-1)
    dc = [g for g in gt if g.type.lower() == "dontcare"]
    for d in det:
        valid = 1 if d.type.lower() == name else -1
        height = int(abs(d.y1 - d.y2))
        ign_det.append(1 if height < R_MIN_HEIGHT[diff] else (0 if valid == 1 else -1))
    return ign_gt, dc, ign_det, n_gt


def r_compute_statistics(metric, cls, gt, det, dc, ign_gt, ign_det, compute_fp, min_ov, ov, ov_dc, aos, aos3d,
                         thresh=0.0):
    NO_DET = -10000000.0
    tp = fp = fn = 0
    v, delta, delta_g = [], [], []
    assigned = [False] * len(det)
    ign_thr = [compute_fp and d.thresh < thresh for d in det]
    for i in range(len(gt)):
        if ign_gt[i] == -1:
            continue
        det_idx, valid, max_ov, assigned_ign = -1, NO_DET, 0.0, False
        for j in range(len(det)):
            if ign_det[j] == -1 or assigned[j] or ign_thr[j]:
                continue
            o = ov[j][i]
            if not compute_fp and o > min_ov and det[j].thresh > valid:
                det_idx, valid = j, det[j].thresh
            elif compute_fp and o > min_ov and (o > max_ov or assigned_ign) and ign_det[j] == 0:
                max_ov, det_idx, valid, assigned_ign = o, j, 1, False
            elif compute_fp and o > min_ov and valid == NO_DET and ign_det[j] == 1:
                det_idx, valid, assigned_ign = j, 1, True
        if valid == NO_DET and ign_gt[i] == 0:
            fn += 1
        elif valid != NO_DET and (ign_gt[i] == 1 or ign_det[det_idx] == 1):
            assigned[det_idx] = True
        elif valid != NO_DET:
            tp += 1
            v.append(det[det_idx].thresh)
            if aos:
                delta.append(gt[i].alpha - det[det_idx].alpha)
            if aos3d:
                delta_g.append(abs(gt[i].ry - det[det_idx].ry))
            assigned[det_idx] = True
    sim = sim_g = 0.0
    if compute_fp:
        for j in range(len(det)):
            if not (assigned[j] or ign_det[j] == -1 or ign_det[j] == 1 or ign_thr[j]):
                fp += 1
        nstuff = 0
        for i in range(len(dc)):
            for j in range(len(det)):
                if assigned[j] or ign_det[j] in (-1, 1) or ign_thr[j]:
                    continue
                if ov_dc[j][i] > min_ov:
                    assigned[j] = True
                    nstuff += 1
        fp -= nstuff
        if aos:
            sim = -1.0
            if tp > 0 or fp > 0:
                sim = 0.0
                for x in [0.0] * fp + [(1.0 + math.cos(d)) / 2.0 for d in delta]:
                    sim += x
        if aos3d:
            sim_g = -1.0
            if tp > 0 or fp > 0:
                sim_g = 0.0
                for x in [0.0] * fp + [(1.0 + math.cos(d)) / 2.0 for d in delta_g]:
                    sim_g += x
    return tp, fp, fn, sim, sim_g, v


def r_max_from_right(vals, n):
    for i in range(n):
        best = vals[i]
        for x in vals[i + 1:]:
            if best < x:
                best = x
        vals[i] = best
    return vals


def r_eval_class(metric, cls, diff, gts, dets, ovs, compute_aos, compute_aos_ground, min_ov):
    n_gt, v, frames = 0, [], []
    for f, (gt, det) in enumerate(zip(gts, dets)):
        ign_gt, dc, ign_det, n = r_clean_data(cls, gt, det, diff)
        n_gt += n
        ov = ovs[f]
        dci = [k for k, g in enumerate(gt) if g.type.lower() == "dontcare"]
        ov_dc = [[ov[1][j][k] for k in dci] for j in range(len(det))]
        frames.append((gt, det, dc, ign_gt, ign_det, ov[0], ov_dc))
        v += r_compute_statistics(metric, cls, gt, det, dc, ign_gt, ign_det, False, min_ov, ov[0], ov_dc, False,
                                  False)[5]
    thresholds = r_get_thresholds(v, n_gt)
    pr = [[0, 0, 0, 0.0, 0.0] for _ in thresholds]
    for gt, det, dc, ign_gt, ign_det, ov, ov_dc in frames:
        memo = {}
        for t, th in enumerate(thresholds):
            key = tuple(d.thresh < th for d in det)  # the statistics depend on the threshold through this set only
            if key not in memo:
                memo[key] = r_compute_statistics(metric, cls, gt, det, dc, ign_gt, ign_det, True, min_ov, ov, ov_dc,
                                                 compute_aos, compute_aos_ground, th)
            tp, fp, fn, sim, sim_g, _ = memo[key]
            pr[t][0] += tp
            pr[t][1] += fp
            pr[t][2] += fn
            if sim != -1:
                pr[t][3] += sim
            if sim_g != -1:
                pr[t][4] += sim_g
    precision, aos, aos_g = [0.0] * 41, [0.0] * 41, [0.0] * 41
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, (tp, fp, fn, s, sg) in enumerate(pr):
            den = np.float64(tp + fp)
            precision[i] = float(np.float64(tp) / den)
            aos[i] = float(np.float64(s) / den)
            aos_g[i] = float(np.float64(sg) / den)
    n = len(thresholds)
    return r_max_from_right(precision, n), r_max_from_right(aos, n), r_max_from_right(aos_g, n)


def r_ap11(vals):
    """`float sum = 0; sum += vals[i]` in C: the point is added in double, the sum rounded to float once."""
    s = np.float32(0)
    for i in range(0, 41, 4):
        s = np.float32(float(s) + vals[i])
    return float(np.float32(np.float32(s / np.float32(11)) * np.float32(100)))


def r_printf_f(v):
    """glibc's %f: NaNs print with their sign ('-nan' for x86's default NaN of 0.0 / 0.0)."""
    if math.isnan(v):
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%f" % v


def restated_evaluate(gt_texts, det_texts, iou="standard"):
    """The C++ program on label texts (frames in the given order).  Returns ({(class, key): (3,41) curve}, report
    lines without the step line)."""
    gts = [r_parse(t, False) for t in gt_texts]
    dets = [r_parse(t, True) for t in det_texts]
    compute_aos = True
    ev = [[False] * 3 for _ in range(3)]
    for det in dets:
        for d in det:
            if d.alpha == -10:
                compute_aos = False
            for c in range(3):
                if d.type.lower() == R_CLASSES[c]:
                    ev[0][c] |= d.x1 >= 0
                    ev[1][c] |= d.t1 != -1000 and d.t3 != -1000 and d.w > 0 and d.l > 0
                    ev[2][c] |= d.t1 != -1000 and d.t2 != -1000 and d.t3 != -1000 and d.h > 0 and d.w > 0 and d.l > 0
                    break
    curves, lines = {}, []
    for metric in range(3):
        fn = R_OVERLAPS[metric]
        ovs = [([[fn(d, g, -1) for g in gt] for d in det], [[fn(d, g, 0) for g in gt] for d in det])
               for gt, det in zip(gts, dets)]
        for c in range(3):
            if not ev[metric][c]:
                continue
            res = [r_eval_class(metric, c, diff, gts, dets, ovs, compute_aos and metric == 0, metric != 0,
                                R_MIN_OVERLAP[iou][c]) for diff in range(3)]
            name = R_CLASSES[c]
            keys = [(0, ("image", "%s_detection")), (1, ("aos", "%s_orientation"))] if metric == 0 else \
                [(0, (("bev", "3d")[metric - 1], "%s_detection_" + ("BEV", "3D")[metric - 1])),
                 (2, (("heading_bev", "heading_3d")[metric - 1], "%s_heading_" + ("BEV", "3D")[metric - 1]))]
            for k, (key, fmt) in keys:
                if key == "aos" and not compute_aos:
                    continue
                curve = np.array([r[k] for r in res])
                curves[(name, key)] = curve
                lines.append("%s AP: %s %s %s" % ((fmt % name,) + tuple(r_printf_f(r_ap11(row)) for row in curve)))
    return curves, lines


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------------- CPU tests


def test_parser_reads_the_fixture_and_handles_crlf_case_and_empty_files():
    from monopsr_amd.core import kitti_eval as ke
    g = golden()
    counts = {}
    for text in g["label_texts"]:
        fr = ke.parse_labels(str(text), detections=False)
        for c in fr.codes:
            counts[int(c)] = counts.get(int(c), 0) + 1
    assert counts[0] == 35 and counts[1] == 14 and counts[2] == 6 and counts[3] == 1 and counts[5] == 26
    assert counts[6] == 2  # Truck, Misc
    line = "Car 0.00 0 1.85 387.63 181.54 423.81 203.12 1.67 1.87 3.69 -16.53 2.39 58.49 1.57"
    fr = ke.parse_labels(line + "\r\n" + line.replace("Car", "cAR").replace(" 0 1.85", " 2 1.85") + "\r\n", False)
    assert list(fr.codes) == [0, 0]
    r = fr.rows[1]
    assert (r[ke.X1], r[ke.Y1], r[ke.X2], r[ke.Y2], r[ke.ALPHA]) == (387.63, 181.54, 423.81, 203.12, 1.85)
    assert (r[ke.H], r[ke.W], r[ke.L], r[ke.TX], r[ke.TY], r[ke.TZ], r[ke.RY]) == (1.67, 1.87, 3.69, -16.53, 2.39,
                                                                                  58.49, 1.57)
    assert r[ke.TRUNCATION] == 0.0 and r[ke.OCCLUSION] == 2
    det = ke.parse_labels("Person_sitting -1 -1 0.5 1 2 3 4 1.5 0.6 0.8 1 2 3 0.1 0.875\n", True)
    assert list(det.codes) == [4] and det.rows[0, ke.SCORE] == 0.875
    assert len(ke.parse_labels("", True)) == 0 and len(ke.parse_labels("\r\n", False)) == 0
    assert ke.class_code("DontCare") == 5 and ke.class_code("van") == 3 and ke.class_code("Tram") == 6
    with pytest.raises(ValueError):
        ke.parse_labels(line, True)  # 15 columns where a detection has 16
    with pytest.raises(ValueError):
        ke.parse_labels(line.replace("1.67", "x"), False)


def test_parse_label_file_and_frame_index(tmp_path):
    from monopsr_amd.core import kitti_eval as ke
    p = tmp_path / "000007.txt"
    p.write_bytes(b"Car -1 -1 0.1 10 20 110 90 1.5 1.6 3.9 1 1.7 20 0.2 0.9\r\n")
    fr = ke.parse_label_file(str(p), True)
    assert len(fr) == 1 and fr.rows[0, ke.SCORE] == 0.9
    assert ke.frame_index("000007.txt") == 7 and ke.frame_index("a.txt") is None
    assert ke.frame_index("run_000123.txt") == 123 and ke.frame_index("readme.txt") == 0


def test_get_thresholds_known_answers():
    from monopsr_amd.core import kitti_eval as ke
    # three ground truths, three true positives: one threshold per recall step reached -> 3 thresholds, not 41
    t = ke.get_thresholds([0.9, 0.8, 0.7], 3)
    assert list(t) == [0.9, 0.8, 0.7]
    # 80 ground truths, 80 TPs: every other score is skipped (recall steps of 1/40), the last one always kept
    s = np.linspace(1, 0.01, 80)
    t = ke.get_thresholds(s, 80)
    assert len(t) == 41 and t[0] == s[0] and t[-1] == s[-1]
    assert list(t) == r_get_thresholds(list(s), 80)
    # fewer TPs than ground truths: recall never reaches 1
    rng = np.random.default_rng(3)
    for n_tp, n_gt in ((5, 40), (17, 17), (100, 250), (0, 10)):
        sc = list(rng.random(n_tp))
        assert list(ke.get_thresholds(sc, n_gt)) == r_get_thresholds(sc, n_gt)


def test_three_perfect_detections_of_three_cars_cap_ap_at_9_09():
    """The reference's number: 3 thresholds -> precision 1 at points 0..2, 0 elsewhere -> AP11 = 1/11 * 100."""
    from monopsr_amd.core import kitti_eval as ke
    curve = np.zeros((3, 41))
    curve[:, :3] = 1.0
    assert np.allclose(ke.ap11(curve), 100.0 / 11, atol=1e-5)
    assert "%f" % ke.ap11(curve)[0] == "9.090909"
    assert np.allclose(ke.ap40(curve), 2 / 40 * 100)


# A curve of precisions tp / (tp + fp) whose printed AP11 the C loop of printAp (`float sum[3]; sum[v] +=
# vals[v][i]`, then printf("%f", sum[v] / 11 * 100)), compiled with g++ 11 on x86-64, gives as 78.347092.  Rounding
# every point to float before a float addition (two roundings) would give 78.347115.
C_AP11_CURVE = [1.0] * 5 + [6 / 7] * 2 + [0.8] * 3 + [0.75] * 2 + [8 / 11] * 29
C_AP11_PRINTED = "78.347092"


def test_ap11_adds_each_point_into_the_float_sum_in_double_and_ap40_is_the_mean_of_points_1_to_40():
    from monopsr_amd.core import kitti_eval as ke
    curve = np.array([C_AP11_CURVE] * 3)
    assert ["%f" % v for v in ke.ap11(curve)] == [C_AP11_PRINTED] * 3
    twice = np.float32(0)
    for i in range(0, 41, 4):
        twice = np.float32(twice + np.float32(C_AP11_CURVE[i]))
    assert "%f" % (twice / np.float32(11) * np.float32(100)) != C_AP11_PRINTED  # the two forms do differ here
    rng = np.random.default_rng(1)
    curve = np.sort(rng.random((3, 41)), axis=1)[:, ::-1]
    got = ke.ap11(curve)
    for k in range(3):
        assert got[k] == r_ap11(curve[k])
    assert np.allclose(ke.ap40(curve), curve[:, 1:].sum(axis=1) / 40 * 100, rtol=1e-14)


def test_a_threshold_without_tp_or_fp_prints_minus_nan_as_the_c_program():
    """tp + fp == 0 at a threshold: precision 0.0 / 0.0 is x86's default NaN (sign bit set), which stays in the
    float sum and which glibc's printf prints as '-nan'."""
    from monopsr_amd.core import kitti_eval as ke
    with np.errstate(invalid="ignore"):
        nan = np.array([0.0]) / np.array([0.0])
    curve = np.ones((3, 41))
    curve[1, 0] = nan[0]
    ap = ke.ap11(curve)
    assert [ke.c_printf_f(v) for v in ap] == ["100.000000", "-nan", "100.000000"]
    assert ke.c_printf_f(float("nan")) == "nan" and ke.c_printf_f(-0.0) == "-0.000000"
    e = {"curve": curve, "ap11": ap, "ap40": ke.ap40(curve)}
    assert ke.format_report({"car": {"image": e}}).splitlines() == ["car_detection AP: 100.000000 -nan 100.000000"]


def test_running_max_keeps_max_element_semantics():
    from monopsr_amd.core import kitti_eval as ke
    v = np.array([0.5, 0.9, np.nan, 0.7] + [0.0] * 37)
    out = ke._max_from_right(v, 4)
    assert out[0] == 0.9 and out[1] == 0.9 and np.isnan(out[2]) and out[3] == 0.7  # NaN < x is false


def test_report_format_order_and_step_line():
    from monopsr_amd.core import kitti_eval as ke
    e = {"curve": np.ones((3, 41)), "ap11": np.array([100.0, 50.0, 9.090909004]), "ap40": np.ones(3)}
    result = {"cyclist": {"image": e, "bev": e, "heading_bev": e},
              "car": {k: e for k in ("image", "aos", "bev", "heading_bev", "3d", "heading_3d")}}
    text = ke.format_report(result, "120000")
    assert text.splitlines() == [
        "120000",
        "car_detection AP: 100.000000 50.000000 9.090909", "car_orientation AP: 100.000000 50.000000 9.090909",
        "cyclist_detection AP: 100.000000 50.000000 9.090909",
        "car_detection_BEV AP: 100.000000 50.000000 9.090909", "car_heading_BEV AP: 100.000000 50.000000 9.090909",
        "cyclist_detection_BEV AP: 100.000000 50.000000 9.090909",
        "cyclist_heading_BEV AP: 100.000000 50.000000 9.090909",
        "car_detection_3D AP: 100.000000 50.000000 9.090909", "car_heading_3D AP: 100.000000 50.000000 9.090909"]
    assert ke.format_report({}, None) == "\n"


def test_restatement_geometry_known_answers():
    """A self-check of the checker, not of the feature (it passes without it): the restatement's own geometry, which
    the GPU results are held to."""
    class B(object):
        pass

    def box(l, w, tx, tz, ry, h=1.0, ty=0.0):
        b = B()
        b.l, b.w, b.h, b.t1, b.t2, b.t3, b.ry = l, w, h, tx, ty, tz, ry
        return b
    assert abs(r_ground_overlap(box(2, 1, 0, 0, 0.3), box(2, 1, 0, 0, 0.3)) - 1) < 1e-12
    assert abs(r_ground_overlap(box(1, 1, 0, 0, 0), box(1, 1, 0.5, 0, 0)) - 1 / 3) < 1e-12
    assert abs(r_ground_overlap(box(1, 1, 0, 0, 0), box(1, 1, 0, 0, math.pi / 4)) - 1 / math.sqrt(2)) < 1e-12
    assert r_ground_overlap(box(1, 1, 0, 0, 0), box(1, 1, 1, 1, 0)) == 0.0  # corner touching
    assert abs(r_box3d_overlap(box(1, 1, 0, 0, 0), box(1, 1, 0, 0, 0, ty=0.5)) - 1 / 3) < 1e-12


def test_restatement_three_perfect_cars():
    """A self-check of the checker, not of the feature (it passes without it): the reference's AP cap with few
    ground truths."""
    gt = ["Car 0.00 0 0.1 100 100 200 200 1.5 1.6 3.9 %d 1.7 20 0.2" % x for x in (-6, 0, 6)]
    det = [g.replace("0.00 0", "-1 -1") + " 0.9" for g in gt]
    curves, lines = restated_evaluate(["\n".join(gt)], ["\n".join(det)])
    assert lines[0] == "car_detection AP: 9.090909 9.090909 9.090909"
    assert len(lines) == 6


# ---------------------------------------------------------------------------------------------------- C ABI checks


def _batch(lib_mod, n_frames, dof, gof, pof, n_det=None, n_gt=None):
    dof = np.asarray(dof, np.int32)
    gof = np.asarray(gof, np.int32)
    pof = np.asarray(pof, np.int64)
    fake = 0x1000  # never dereferenced: every failing call below stops on the host
    b = lib_mod.KittiBatch(fake, fake, fake, fake, fake, fake, fake, dof.ctypes.data, gof.ctypes.data,
                           pof.ctypes.data, int(dof[-1]) if n_det is None else n_det,
                           int(gof[-1]) if n_gt is None else n_gt, n_frames)
    return b, (dof, gof, pof)


def test_entry_points_check_arguments_on_the_host():
    from monopsr_amd import _lib
    lib = _lib.lib()
    mo = (ctypes.c_double * 9)(*([0.7, 0.5, 0.5] * 3))
    nthr = (ctypes.c_int * 27)()
    fake = 0x1000

    def status(b):
        return lib.mpsr_kitti_overlaps(ctypes.byref(b), fake, None)
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6])
    b.n_det = -1
    assert status(b) == 1 and b"negative" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 2, [0, 2, 1], [0, 3, 3], [0, 6, 6])
    assert status(b) == 1 and b"decrease" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 5])
    assert status(b) == 1 and b"pairs" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6], n_det=4)
    assert status(b) == 1 and b"row counts" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6])
    b.det = None
    assert status(b) == 1 and b"null" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6])
    b.gt_off_host = None
    assert status(b) == 1 and b"null" in lib.mpsr_last_error()
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6])
    assert lib.mpsr_kitti_overlaps(ctypes.byref(b), None, None) == 1 and b"null" in lib.mpsr_last_error()
    assert lib.mpsr_kitti_overlaps(None, fake, None) == 1
    # a frame beyond the statistics kernels' bitset: a clean error, before any launch
    big = 8193
    b, keep = _batch(_lib, 1, [0, big], [0, 1], [0, big])
    assert lib.mpsr_kitti_match(ctypes.byref(b), fake, mo, fake, fake, None) == 1
    assert b"8192" in lib.mpsr_last_error()
    assert lib.mpsr_kitti_stats(ctypes.byref(b), fake, mo, fake, nthr, 1, fake, fake, fake, 1 << 30, None) == 1
    b, keep = _batch(_lib, 1, [0, 2], [0, 3], [0, 6])
    nthr[4] = 42
    assert lib.mpsr_kitti_stats(ctypes.byref(b), fake, mo, fake, nthr, 1, fake, fake, fake, 1 << 30, None) == 1
    assert b"thresholds" in lib.mpsr_last_error()
    nthr[4] = 10
    assert lib.mpsr_kitti_stats(ctypes.byref(b), fake, mo, fake, nthr, 1, fake, fake, fake, 16, None) == 3  # workspace
    assert lib.mpsr_kitti_match(ctypes.byref(b), fake, None, fake, fake, None) == 1  # min_overlap
    # empty batch: nothing to do
    b, keep = _batch(_lib, 0, [0], [0], [0])
    assert lib.mpsr_kitti_overlaps(ctypes.byref(b), None, None) == 0
    assert lib.mpsr_kitti_match(ctypes.byref(b), None, mo, None, None, None) == 0
    assert lib.mpsr_kitti_stats_workspace_bytes(0, 27) == 0
    assert lib.mpsr_kitti_stats_workspace_bytes(10, 2) >= 10 * 2 * 41 * 28

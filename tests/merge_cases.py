"""The seeded catalogue of MSCNN-merge cases shared by tests/test_mscnn_merge.py (CPU, against the recorded reference)
and tests/test_mscnn_merge_gpu.py (the kernel).  A case: name, label_boxes (L,4) and det_boxes (D,4) float32
[y1, x1, y2, x2], label_z (L,) float32, det_scores (D,) float64, min_iou, score_type.  EXACT names the cases whose best
IoU sits on the threshold on purpose; in every other case no pair's IoU lies within 1e-5 of min_iou (checked here)."""
import numpy as np

import merge_restatement as mr

EXACT = ('seventy_of_100', 'exact_half')  # 'just_under' is 1e-3 away


def _case(name, lb, lz, db, ds, min_iou=0.7, score_type='distance'):
    return dict(name=name, label_boxes=np.asarray(lb, np.float32).reshape(-1, 4),
                label_z=np.asarray(lz, np.float32).reshape(-1), det_boxes=np.asarray(db, np.float32).reshape(-1, 4),
                det_scores=np.asarray(ds, np.float64).reshape(-1), min_iou=float(min_iou), score_type=score_type)


def _random_boxes(rng, n):
    y1, x1 = rng.uniform(0, 300, n), rng.uniform(0, 1100, n)
    h, w = rng.uniform(12, 70, n), rng.uniform(12, 120, n)
    return np.round(np.stack([y1, x1, y1 + h, x1 + w], 1), 2).astype(np.float32)


def _random_case(rng, name, n_labels, n_dets, min_iou, score_type):
    """Labels, then detections that are shifted labels (some twice: the later wins), far-off false positives and a
    few zero scores; pairs whose IoU comes within 1e-5 of min_iou are redrawn."""
    lb = _random_boxes(rng, n_labels)
    db = np.zeros((n_dets, 4), np.float32)
    for d in range(n_dets):
        while True:
            if n_labels and rng.uniform() < 0.8:
                box = lb[rng.integers(n_labels)] + np.round(rng.normal(0, 3.0, 4), 2).astype(np.float32)
            else:
                box = _random_boxes(rng, 1)[0]
            box = box.astype(np.float32)
            if not n_labels or (np.abs(mr.two_d_iou(box, lb) - min_iou) > 1e-4).all():
                break
        db[d] = box
    ds = np.round(rng.uniform(0.2, 1.0, n_dets), 4)
    ds[rng.uniform(size=n_dets) < 0.05] = 0.0
    return _case(name, lb, np.round(rng.uniform(2, 70, n_labels), 2), db, ds, min_iou, score_type)


def catalogue():
    rng = np.random.default_rng(20240611)
    unit = [0, 0, 10, 10]
    cases = [
        _case('no_labels', [], [], [[0, 0, 10, 10]], [0.9]),
        _case('no_detections', [unit, [20, 20, 50, 60]], [10, 50], [], []),
        _case('nothing', [], [], [], []),
        _case('one_by_one', [[100, 200, 150, 300]], [20], [[101, 202, 151, 299]], [0.83]),
        _case('one_by_one_miss', [[100, 200, 150, 300]], [20], [[300, 800, 340, 900]], [0.83]),
        # two labels at equal IoU with the detection: the lower index wins
        _case('tie_lower_index', [[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]], [10, 20, 30],
              [[0, 0, 10, 9]], [0.6]),
        _case('tie_mirrored', [[0, 20, 10, 30], [0, 0, 10, 10]], [10, 20], [[0, 0, 10, 30]], [0.6], min_iou=0.3),
        # two detections accepted by one label: the later wins
        _case('later_wins', [[0, 0, 100, 100]], [10], [[0, 0, 100, 95], [0, 0, 100, 90]], [0.9, 0.4]),
        # the first detection moves label 0 far away; the second still matches label 0's ORIGINAL box
        _case('original_box', [[0, 0, 100, 100], [0, 300, 100, 400]], [10, 20],
              [[0, 0, 100, 75], [0, 24, 100, 100]], [0.9, 0.5]),
        # a detection score of exactly 0 is accepted and then refilled
        _case('zero_score', [[0, 0, 100, 100]], [22.5], [[0, 0, 100, 99]], [0.0]),
        _case('zero_score_max', [[0, 0, 100, 100]], [22.5], [[0, 0, 100, 99]], [0.0], score_type='max'),
        _case('zero_score_min', [[0, 0, 100, 100]], [22.5], [[0, 0, 100, 99]], [0.0], score_type='min'),
        # 70 / 100: the float32 quotient widened is 0.69999998..., < 0.7; the reference rounds it to 3 decimals, 0.7: accepted
        _case('seventy_of_100', [unit], [10], [[0, 0, 10, 7]], [0.8], min_iou=0.7),
        _case('exact_half', [unit], [10], [[0, 0, 10, 5]], [0.8], min_iou=0.5),
        # 699 / 1000 = 0.699 after rounding (0.6990000009...): refused; 6995 / 10000 rounds half to even, 0.7 (x1000 = 699.5)
        _case('just_under', [[0, 0, 10, 100]], [10], [[0, 0, 10, 69.9]], [0.8], min_iou=0.7),
        # the clip of the distance score: 1, just above 0.1 (1 - 0.9 in float32), 0.1 twice
        _case('clip_z', [[0, 0, 10, 10], [0, 20, 10, 30], [0, 40, 10, 50], [0, 60, 10, 70]], [0, 40.5, 45, 60], [], []),
        _case('clip_z_max', [[0, 0, 10, 10], [0, 20, 10, 30]], [0, 60], [], [], score_type='max'),
        _case('clip_z_min', [[0, 0, 10, 10], [0, 20, 10, 30]], [0, 60], [], [], score_type='min'),
    ]
    cases.append(_random_case(rng, 'wide_65x70', 65, 70, 0.7, 'distance'))
    cases.append(_random_case(rng, 'wide_130x9_ped', 130, 9, 0.5, 'max'))
    for k, (nl, nd) in enumerate(((3, 5), (7, 7), (64, 3), (1, 12), (12, 1))):
        cases.append(_random_case(rng, 'random_%d' % k, nl, nd, (0.7, 0.5)[k % 2], ('distance', 'max', 'min')[k % 3]))
    # the clustered labels of a crowded frame: many near ties
    base = np.array([100, 500, 160, 600], np.float32)
    lb = np.stack([base + np.float32(2 * k) for k in range(6)])
    cases.append(_case('crowded', lb, [10, 12, 14, 16, 18, 20], lb[::-1] + np.float32(0.5),
                       [0.9, 0.8, 0.7, 0.6, 0.5, 0.4]))
    _check(cases)
    return cases


def _check(cases):
    names = [c['name'] for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        if c['name'] in EXACT or not len(c['label_boxes']):
            continue
        for d in c['det_boxes']:
            iou = mr.two_d_iou(d, c['label_boxes'])
            assert (np.abs(iou - c['min_iou']) > 1e-5).all(), (c['name'], iou)

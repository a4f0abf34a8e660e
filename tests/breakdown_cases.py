"""The rows mpsr_object_pairs is tried on (tests/test_breakdown.py on the restatement, tests/test_breakdown_gpu.py on
the device) and the tables of the binned statistics.

catalogue() -> float32 arrays pred, gt (n,7) [x y z l w h ry], fed (n,4) [y1 x1 y2 x2], info (n,6) [truncation,
occlusion, x1, y1, x2, y2], and `rows`: name -> index of the rows with a known answer.  257 rows: the known answers,
rotations, containment, far coordinates, a NaN or an infinity in each field in turn, z on the depth edges, the
difficulty levels' limits, then 200 seeded random pairs around a shared centre.
"""
import math

import numpy as np

DEPTH_EDGES = (10.0, 20.0, 30.0, 40.0, 50.0)
BOX_IOU_EDGES = (0.7, 0.8, 0.9)
SIZES = (0, 1, 63, 64, 65, 257)
MARGIN = 1e-9  # no restated IoU of the catalogue may be this close to a hit threshold or a box_iou_edges entry

# (name, pred, gt) with float64 values: what the CPU test asks the restatement, and (rounded) the catalogue's first rows
UNIT = [0.0, 1.0, 20.0, 1.0, 1.0, 1.0, 0.0]


def _moved(box, **kw):
    out = list(box)
    for k, v in kw.items():
        out['xyzlwhr'.index(k)] = v
    return out


KNOWN = [
    ('identical', [1.0, 1.5, 20.0, 4.0, 2.0, 1.5, 0.3], [1.0, 1.5, 20.0, 4.0, 2.0, 1.5, 0.3]),
    ('half_length', _moved(UNIT, x=0.5), UNIT),
    ('rotated_45', _moved(UNIT, r=math.pi / 4), UNIT),
    ('corner_touching', _moved(UNIT, x=1.0, z=21.0), UNIT),
    ('edge_touching', _moved(UNIT, x=1.0), UNIT),
    ('stacked', _moved(UNIT, y=2.0), UNIT),
    ('zero_length', _moved(UNIT, l=0.0), UNIT),
    ('negative_width', UNIT, _moved(UNIT, w=-1.0)),
    ('zero_height', _moved(UNIT, h=0.0), UNIT),
]

# (truncation, occlusion, height of the label's box) -> the level
DIFFICULTY = [
    ((0.0, 0, 40.0), 1), ((0.0, 0, 40.5), 0), ((0.0, 0, 25.0), 3), ((0.0, 0, 25.5), 1), ((0.15, 0, 60.0), 0),
    ((0.16, 0, 60.0), 1), ((0.3, 1, 60.0), 1), ((0.31, 1, 60.0), 2), ((0.5, 2, 60.0), 2), ((0.51, 2, 60.0), 3),
    ((0.0, 3, 60.0), 3), ((0.0, 1, 60.0), 1), ((0.0, 2, 60.0), 2),
]

_LABEL_BOX = [100.0, 120.0, 220.0, 200.0]  # x1 y1 x2 y2
_FED_BOX = [118.0, 104.0, 203.0, 226.0]    # y1 x1 y2 x2: a detection a few pixels off the label's box


def difficulty_info(trunc, occ, height):
    return [trunc, float(occ), 100.0, 120.0, 220.0, 120.0 + height]


def catalogue(seed=0):
    rng = np.random.default_rng(seed)
    pred, gt, fed, info, rows = [], [], [], [], {}
    car_p, car_g = [1.2, 1.6, 24.5, 3.9, 1.6, 1.5, 0.4], [1.0, 1.65, 25.0, 4.1, 1.7, 1.55, 0.3]

    def add(p, g, f=None, i=None, name=None):
        if name is not None:
            rows[name] = len(pred)
        pred.append(list(p))
        gt.append(list(g))
        fed.append(list(_FED_BOX if f is None else f))
        info.append(list([0.0, 0.0] + _LABEL_BOX if i is None else i))

    for name, p, g in KNOWN:
        add(p, g, name=name)
    for k, turn in enumerate((0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi)):
        add(_moved(car_g, r=car_g[6] + turn), car_g, name='turn_%d' % k)
    add([1.0, 1.6, 25.0, 1.0, 0.5, 1.0, 0.3], car_g, name='contained')
    add(_moved(car_p, x=1001.2, z=1024.5), _moved(car_g, x=1001.0, z=1025.0), name='far')
    add(_moved(car_p, x=-998.8, z=24.5), _moved(car_g, x=-999.0, z=25.0))
    bad = (float('nan'), float('inf'), float('-inf'))
    rows['non_finite'] = len(pred)
    for k in range(24):  # pred's seven fields, gt's seven, fed's four, info's six
        p, g, f, i = list(car_p), list(car_g), list(_FED_BOX), [0.1, 1.0] + _LABEL_BOX
        target, at = ((p, k), (g, k - 7), (f, k - 14), (i, k - 18))[(k >= 7) + (k >= 14) + (k >= 18)]
        target[at] = bad[k % 3]
        add(p, g, f, i)
    rows['on_depth_edge'] = len(pred)
    for z in (10.0, 20.0, 50.0):
        add(_moved(car_p, z=z - 0.5), _moved(car_g, z=z))
    rows['difficulty'] = len(pred)
    for (trunc, occ, height), _ in DIFFICULTY:
        add(car_p, car_g, i=difficulty_info(trunc, occ, height))
    rows['random'] = len(pred)
    for _ in range(200):
        centre = np.array([rng.uniform(-20, 20), rng.uniform(1, 2), rng.uniform(3, 65)])
        dims, ry = np.array([rng.uniform(3, 5), rng.uniform(1.4, 2), rng.uniform(1.3, 1.8)]), rng.uniform(-math.pi, math.pi)
        g = list(centre) + list(dims) + [ry]
        p = list(centre + rng.normal(0, [0.4, 0.1, 0.8])) + list(dims * rng.uniform(0.85, 1.15, 3)) + \
            [ry + rng.normal(0, 0.25)]
        x1, y1 = rng.uniform(0, 1000), rng.uniform(100, 250)
        w, h = rng.uniform(20, 200), rng.uniform(15, 120)
        lab = [x1, y1, x1 + w, y1 + h]
        d = rng.normal(0, 0.05, 4) * [w, h, w, h]
        add(p, g, [lab[1] + d[1], lab[0] + d[0], lab[3] + d[3], lab[2] + d[2]],
            [rng.choice([0.0, 0.1, 0.2, 0.4, 0.8]), float(rng.integers(0, 4))] + lab)
    f32 = lambda a, w: np.asarray(a, np.float32).reshape(-1, w)
    return dict(pred=f32(pred, 7), gt=f32(gt, 7), fed=f32(fed, 4), info=f32(info, 6), rows=rows)


def margin_of(overlaps):
    """The least distance of the restated IoUs (overlaps (n,4): iou_2d_fed, iou_bev, iou_3d, ...) from a value that
    decides a hit or a fed-box bin, NaNs left out."""
    out = np.inf
    for col, marks in ((0, BOX_IOU_EDGES), (1, (0.7, 0.5)), (2, (0.7, 0.5, 0.25))):
        v = overlaps[:, col]
        v = v[~np.isnan(v)]
        for m in marks:
            if v.size:
                out = min(out, float(np.abs(v - m).min()))
    return out


# ---- tables of the binned statistics

N_ROWS = (0, 1, 255, 256, 257, 5000)
COLUMN_METRIC = (0, 1, 2, 3, 4, 5, 6, 7, 7, 7)  # evaluator.COLUMN_METRIC: the last three columns feed one metric
N_METRICS = 8
AXES = ((3,), (4, 2), (6, 4, 4))  # axis_bins of the 1-, 2- and 3-axis cases
NAN_PLACEMENTS = ('none', 'entry', 'column')


def stats_table(n_rows, seed):
    """tests/test_metric_stats_gpu.py's _table: unit normals times per-column scales of 0.01 .. 100 plus offsets of the
    same order."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2, 2, len(COLUMN_METRIC))
    offset = scale * rng.uniform(-2, 2, len(COLUMN_METRIC))
    return (rng.standard_normal((n_rows, len(COLUMN_METRIC))) * scale + offset).astype(np.float32)


def place_nans(values, placement):
    v = values.copy()
    if placement == 'entry' and len(v):
        v[len(v) // 2, 8] = np.nan
    elif placement == 'column':
        v[:, 2] = np.nan
    return v


def stats_bins(n_rows, axis_bins, seed):
    """(n_rows, n_axes) int32: indices in [-1, axis_bins[a]] (-1 and axis_bins[a] itself are in no bin), and the last
    bin of every axis with two or more bins left empty."""
    rng = np.random.default_rng(seed)
    cols = []
    for nb in axis_bins:
        b = rng.integers(-1, nb + 1, n_rows)
        if nb >= 2:
            b[b == nb - 1] = 0
        cols.append(b)
    return np.stack(cols, 1).astype(np.int32).reshape(n_rows, len(axis_bins))


STATS_CASES = [(n, axes, p) for k, n in enumerate(N_ROWS) for axes in (AXES[k % 3],) for p in NAN_PLACEMENTS
               if n or p == 'none']

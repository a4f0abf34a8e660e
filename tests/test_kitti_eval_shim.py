"""The boost-free shim the native KITTI evaluator is compiled against (oracle/ref_eval/shim): its bird's-eye-view and
3D IoU through a probe built by the same recipe (oracle/_ref/shim_probe), against known answers, the restatement's
exact geometry and the reference's own Python IoU pins (tests/golden/kitti_eval.npz).  CPU only."""
import math
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kitti_program as P  # noqa: E402
import test_kitti_eval as R  # noqa: E402

# The pins' three_d_iou rasterises both bases at 1 cm (see test_kitti_eval_gpu.RASTER_BOUND_3D).
RASTER_BOUND_3D = 0.02


def probe(pairs):
    """pairs: [((l, w, h, tx, ty, tz, ry), (same))] -> (n, 2) array of (BEV IoU, 3D IoU) from the shim."""
    text = "".join(" ".join(repr(float(v)) for v in tuple(a) + tuple(b)) + "\n" for a, b in pairs)
    proc = subprocess.run([P.binary("shim_probe")], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          universal_newlines=True, timeout=60)
    assert proc.returncode == 0, proc.stderr
    out = np.array([[float(x) for x in line.split()] for line in proc.stdout.splitlines()]).reshape(-1, 2)
    assert len(out) == len(pairs)
    return out


class _B(object):
    def __init__(self, l, w, h, tx, ty, tz, ry):
        self.l, self.w, self.h, self.t1, self.t2, self.t3, self.ry = l, w, h, tx, ty, tz, ry


def test_shim_known_answers():
    s2 = math.sqrt(2.0)
    inter45 = 2 * (s2 - 1)  # unit square and the same square turned 45 degrees about its centre
    cases = [
        (((3.9, 1.6, 1.5, 2.0, 1.7, 20.0, 0.3), (3.9, 1.6, 1.5, 2.0, 1.7, 20.0, 0.3)), (1.0, 1.0)),
        (((1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, math.pi / 4)),
         (inter45 / (2 - inter45), inter45 / (2 - inter45))),
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0), (2.0, 1.0, 1.0, 0.5, 0.0, 0.2, 0.0)), (0.25, 0.25)),  # nested
        (((4.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.7), (2.0, 1.0, 1.0, 0.0, -0.5, 0.0, 0.7)), (0.25, 0.125)),  # nested in 3D
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0), (4.0, 2.0, 1.0, 4.0, 0.0, 0.0, 0.0)), (0.0, 0.0)),  # shared edge
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0), (4.0, 2.0, 1.0, 4.0, 0.0, 2.0, 0.0)), (0.0, 0.0)),  # shared corner
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, math.pi / 2), (4.0, 2.0, 1.0, 0.0, 0.0, 4.0, math.pi / 2)), (0.0, 0.0)),
        (((1.0, 1.0, 1.0, 0.0, 0.0, 0.0, math.pi / 4), (1.0, 1.0, 1.0, s2, 0.0, 0.0, math.pi / 4)), (0.0, 0.0)),
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0), (4.0, 2.0, 1.0, 0.0, 1.0, 0.0, 0.0)), (1.0, 0.0)),  # heights touch
        (((4.0, 2.0, 1.0, 0.0, 0.0, 0.0, 0.0), (4.0, 2.0, 1.0, 10.0, 0.0, 0.0, 0.0)), (0.0, 0.0)),  # apart
    ]
    got = probe([c for c, _ in cases])
    for k, (_, want) in enumerate(cases):
        assert np.allclose(got[k], want, rtol=0, atol=1e-14), (k, got[k], want)
    for k in (4, 5, 6, 7, 9):
        assert got[k, 0] == 0.0 and got[k, 1] == 0.0, (k, got[k])  # no sliver of area from rounding


def test_shim_matches_the_exact_restatement_and_the_reference_pins():
    g = R.golden()
    a3, b3 = g["pin3d_a"], g["pin3d_b"]  # [ry, l, h, w, tx, ty, tz]

    def box(x):
        ry, l, h, w, tx, ty, tz = x
        return (l, w, h, tx, ty, tz, ry)
    pairs = [(box(a), box(b)) for a, b in zip(a3, b3)]
    rng = np.random.default_rng(2)
    for _ in range(300):  # random pairs at all angles, sizes and offsets
        a = (rng.uniform(0.2, 6), rng.uniform(0.2, 3), rng.uniform(0.5, 2), rng.uniform(-3, 3), rng.uniform(1, 2),
             rng.uniform(-3, 3), rng.uniform(-4, 4))
        b = (rng.uniform(0.2, 6), rng.uniform(0.2, 3), rng.uniform(0.5, 2), a[3] + rng.normal(0, 1),
             a[4] + rng.normal(0, 0.3), a[5] + rng.normal(0, 1), rng.uniform(-4, 4))
        pairs.append((a, b))
    got = probe(pairs)
    exact = np.array([[R.r_ground_overlap(_B(*a), _B(*b)), R.r_box3d_overlap(_B(*a), _B(*b))] for a, b in pairs])
    assert np.abs(got - exact).max() <= 1e-12
    assert (exact[:, 0] > 0).sum() > 300
    pins = g["pin3d_iou"]
    assert np.abs(got[:len(pins), 1] - pins).max() <= RASTER_BOUND_3D
    assert (got[:len(pins), 1] > 0).sum() >= 150


def test_shim_aborts_on_a_counter_clockwise_polygon():
    """A box with one negative size makes a counter-clockwise footprint: outside what the shim reproduces."""
    proc = subprocess.run([P.binary("shim_probe")], input="4 -2 1 0 0 0 0 4 2 1 0 0 0 0\n", stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert proc.returncode != 0 and "counter-clockwise" in proc.stderr

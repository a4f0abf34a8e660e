"""mpsr_kitti_detection_rows against evaluator_utils.kitti_label_array / project_boxes_3d: 0, 1, 65 and 300 rows over
4 frames."""
import numpy as np
import pytest
import torch

from monopsr_amd.core import evaluator_utils as eu

pytestmark = pytest.mark.gpu

P2 = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
P2_B = np.array([[707.0912, 0, 601.8873, 0], [0, 707.0912, 183.1104, 0], [0, 0, 1, 0]])
FRAMES = [(P2, (1242, 375)), (P2_B, (1224, 370)), (P2, (1238, 374)), (P2_B, (1241, 376))]
THRESHOLD = 0.1
# kitti_label_array's columns (alpha | x1 y1 x2 y2 | h w l | x y z | ry score) in the kernel's (kitti_eval's) order
TO_EVAL = [1, 2, 3, 4, 0, 5, 6, 7, 8, 9, 10, 11, 12]


def _inputs(n, seed):
    rng = np.random.default_rng(seed)
    b3 = np.zeros((n, 9), np.float32)
    b3[:, 0] = rng.uniform(-25, 25, n)
    b3[:, 1] = rng.uniform(0.8, 2.5, n)
    b3[:, 2] = rng.uniform(4.0, 70, n)   # some boxes straddle the image border or are too large in it
    b3[:, 3:6] = rng.uniform(1.2, 4.5, (n, 3))
    b3[:, 6] = rng.uniform(-np.pi, np.pi, n)
    b3[:, 7] = rng.uniform(0.0, 1.0, n)
    b2 = np.zeros((n, 7), np.float32)
    b2[:, 0:2] = rng.uniform(0, 300, (n, 2))
    b2[:, 2:4] = b2[:, 0:2] + rng.uniform(5, 200, (n, 2)).astype(np.float32)
    b2[:, 4] = rng.uniform(-np.pi, np.pi, n)
    b2[:, 5] = b3[:, 7]
    if n > 2:
        b3[1, 7] = b2[1, 5] = np.float32(THRESHOLD)  # float32(0.1) > 0.1: kept
        b3[2, 7] = b2[2, 5] = 0.5                    # exactly representable ...
    frame = rng.integers(0, len(FRAMES), n).astype(np.int32)
    return b3, b2, frame


def _device(b3, b2, frame, threshold, project):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p2 = dev(np.stack([f[0] for f in FRAMES]).reshape(-1, 12).astype(np.float64))
    wh = dev(np.asarray([f[1] for f in FRAMES], np.int32))
    rows, cls, keep = eu.detection_rows(dev(b3), dev(b2), threshold, dev(frame), p2, wh, project)
    assert rows.dtype == torch.float64 and cls.dtype == torch.int32 and keep.dtype == torch.int32
    return rows.cpu().numpy(), cls.cpu().numpy(), keep.cpu().numpy().astype(bool)


@pytest.mark.parametrize('n', [0, 1, 65, 300])
def test_rows_without_projection_are_bit_equal(n):
    b3, b2, frame = _inputs(n, 7 + n)
    rows, cls, keep = _device(b3, b2, frame, THRESHOLD, False)
    assert rows.shape == (n, 14) and cls.shape == (n,) and keep.shape == (n,)
    assert np.array_equal(keep, b3[:, 7].astype(np.float64) >= THRESHOLD)
    want_cls, want = eu.kitti_label_array(b3, b2, THRESHOLD)
    assert rows[keep][:, :13].tobytes() == np.ascontiguousarray(want[:, TO_EVAL]).tobytes()
    assert (rows[:, 13] == 0).all() and np.array_equal(cls[keep], want_cls)
    if n:
        # every row is formed, kept or not
        _, every = eu.kitti_label_array(b3, b2, -1.0)
        assert rows[:, :13].tobytes() == np.ascontiguousarray(every[:, TO_EVAL]).tobytes()


def test_a_score_on_the_threshold_is_kept():
    b3, b2, frame = _inputs(8, 3)
    b3[:, 7] = [0.5, 0.25, 0.125, 0.75, 0.4999, 0.5001, 0.0, 1.0]
    _, _, keep = _device(b3, b2, frame, 0.5, False)
    assert list(keep) == [True, False, False, True, False, True, False, True]


def _raw_extents(b3, p2):
    """The unclipped [u_min, v_min, u_max, v_max] of project_boxes_3d: the image moved by 1e6 px so that no clip acts."""
    shifted = p2.copy()
    shifted[0] += 1e6 * p2[2]
    shifted[1] += 1e6 * p2[2]
    return eu.project_boxes_3d(b3, shifted, (1e12, 1e12))[0] - 1e6


@pytest.mark.parametrize('n', [1, 65, 300])
def test_rows_with_projection_equal_after_rounding(n):
    """cos / sin and the sums of the projection differ from numpy's in the last bits, so a row is compared only when,
    on the CPU, no unrounded box value lies within 1e-6 of a rounding boundary (half a unit of the third decimal) and
    no keep test lies within 1e-6 of its bound.  At most 1 % of the rows may be left out."""
    b3, b2, frame = _inputs(n, 11 + n)
    rows, cls, keep = _device(b3, b2, frame, THRESHOLD, True)
    boxes, want_keep, safe = np.zeros((n, 4)), np.zeros(n, bool), np.ones(n, bool)
    for f, (p2, size) in enumerate(FRAMES):
        sel = frame == f
        if not sel.any():
            continue
        b = b3[sel].astype(np.float64)
        boxes[sel], want_keep[sel] = eu.project_boxes_3d(b, p2, size)
        raw = _raw_extents(b, p2)
        w, h = float(size[0]), float(size[1])
        bounds = np.stack([raw[:, 0] - w, raw[:, 1] - h, raw[:, 2], raw[:, 3], raw[:, 2] - w, raw[:, 3] - h,
                           raw[:, 0], raw[:, 1], (raw[:, 2] - raw[:, 0]) - 0.8 * w, (raw[:, 3] - raw[:, 1]) - 0.8 * h], 1)
        scaled = boxes[sel] * 1000
        on_half = np.abs(scaled - np.floor(scaled) - 0.5) * 1e-3
        safe[sel] = (np.abs(bounds) > 2e-6).all(1) & (on_half > 1e-6).all(1)
    assert (~safe).sum() <= 0.01 * n, (~safe).sum()
    want_keep &= b3[:, 7].astype(np.float64) >= THRESHOLD
    assert np.array_equal(keep[safe], want_keep[safe])
    _, want = eu.kitti_label_array(b3, b2, -1.0, boxes)
    assert np.array_equal(rows[safe][:, :13], want[safe][:, TO_EVAL])
    assert np.array_equal(cls, b3[:, 8].astype(np.int32))
    if n >= 65:
        assert keep.any() and (~keep).any() and (boxes[:, 0] == 0).any()

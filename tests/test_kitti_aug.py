"""The jitter's random numbers and arithmetic on the host: Philox4x32-10 known answers, the restatement against an
independently written scalar loop on one np.random state, and the choice of seeds for the GPU comparison.  No GPU."""
import numpy as np
import pytest

import jitter_restatement as jr

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize('counter,key,want', KNOWN)
def test_philox4x32_10_known_answers(counter, key, want):
    assert tuple(int(w) for w in jr.philox4x32_10(counter, key)) == want
    # vectorised over a counter word: every lane is the scalar answer
    got = jr.philox4x32_10((np.array([counter[0], 5, 7]), counter[1], counter[2], counter[3]), key)
    assert tuple(int(w[0]) for w in got) == want
    assert tuple(int(w[1]) for w in got) == tuple(int(w) for w in jr.philox4x32_10((5,) + counter[1:], key))


def test_uniform_and_normal_pair():
    assert jr.uniform53(np.uint64(0), np.uint64(0)) == 0.0
    assert jr.uniform53(np.uint64(0xffffffff), np.uint64(0xffffffff)) == 1.0 - 2.0 ** -53
    assert jr.uniform53(np.uint64(1 << 5), np.uint64(0)) == 2.0 ** -27
    assert jr.seed_key(0x1234567890abcdef) == (0x90abcdef, 0x12345678)
    j = np.arange(200000)
    z0, z1 = jr.normal_pair(j, 3, 11, 2, jr.STREAM_JITTER, seed=5)
    for z in (z0, z1):
        assert np.isfinite(z).all()
        assert abs(z.mean()) < 4 / np.sqrt(len(z)) and abs(z.std() - 1) < 4 / np.sqrt(2 * len(z))
    assert abs(np.corrcoef(z0, z1)[0, 1]) < 4 / np.sqrt(len(j))
    # a draw depends on its coordinates only
    a, _ = jr.normal_pair(7, 3, 11, 2, jr.STREAM_JITTER, seed=5)
    assert a == z0[7]
    for other in ((7, 4, 11, 2, 1, 5), (7, 3, 12, 2, 1, 5), (7, 3, 11, 3, 1, 5), (7, 3, 11, 2, 0, 5),
                  (7, 3, 11, 2, 1, 6), (7, 3, 11, 2, 1, 5 + (1 << 32))):
        assert jr.normal_pair(*other)[0] != a


def test_oversample_indices_keep_the_labels_first():
    idx = jr.oversample_indices(3, 32, frame_index=9, epoch=1, seed=2)
    assert list(idx[:3]) == [0, 1, 2] and idx.min() >= 0 and idx.max() <= 2 and len(set(idx[3:])) == 3
    assert np.array_equal(idx, jr.oversample_indices(3, 32, 9, 1, 2))
    assert not np.array_equal(idx, jr.oversample_indices(3, 32, 9, 2, 2))
    assert np.array_equal(jr.oversample_indices(1, 8, 0, 0, 0), np.zeros(8))
    counts = np.bincount(jr.oversample_indices(4, 40004, 1, 0, 3)[4:], minlength=4)
    assert (np.abs(counts - 10000) < 4 * np.sqrt(10000 * 0.75)).all()


def _boxes(rng, n, h, w):
    bw, bh = rng.uniform(2, 600, n), rng.uniform(2, 370, n)
    x1, y1 = rng.uniform(0, w - 1 - np.minimum(bw, w - 1)), rng.uniform(0, h - 1 - np.minimum(bh, h - 1))
    b = np.stack([x1, y1, np.minimum(x1 + bw, w - 1), np.minimum(y1 + bh, h - 1)], 1)
    return b.astype(np.float32).astype(np.float64)  # label values are float32


@pytest.mark.parametrize('thr', [0.5, 0.7])
def test_restatement_equals_the_scalar_loop_on_one_random_state(thr):
    """The vectorised restatement fed np.random's normals equals the scalar oracle (Python floats, np.random.normal
    called as the reference calls it: centre x, centre y, half width, half height) box for box in fp64: the arithmetic,
    the order of the four draws, loc + scale * z, the clip and the accept rule."""
    rng = np.random.default_rng(int(thr * 10))
    h, w = 375, 1242
    boxes = _boxes(rng, 300, h, w)
    boxes[::7, 0], boxes[1::7, 1] = 0.0, 0.0  # touching the left / top border
    boxes[2::7, 2], boxes[3::7, 3] = w - 1, h - 1

    np.random.seed(1234)
    want, ref_trials = jr.scalar_jitter(boxes, thr, (h, w))

    np.random.seed(1234)
    hook = lambda t, active: tuple(np.array([np.random.normal()]) for _ in range(4))
    got, trials = [], []
    for b in boxes:  # one box at a time: the oracle finishes a box before it starts the next
        o, t, _ = jr.jitter_boxes(b[None], [1], [(h, w)], [0], [0], 0, 0, thr, max_trials=10 ** 6, normals=hook)
        got.append(o[0])
        trials.append(int(t[0]))
    got = np.array(got)
    assert trials == ref_trials
    assert got.tobytes() == want.tobytes()
    small = (boxes[:, 2] - boxes[:, 0] < 10) | (boxes[:, 3] - boxes[:, 1] < 10)
    assert small.any() and (np.array(trials)[small] == 0).all() and (got[small] == boxes[small]).all()
    assert (np.array(trials)[~small] >= 1).all() and (got[~small] != boxes[~small]).any(1).all()


def test_scalar_loop_by_hand():
    """The oracle itself on draws given by hand: z = (0.3, -0.6, 0.6, -1.2) moves a 200 x 100 box at (100..300, 50..150)
    to centre (200 + 100/3 * 0.3, 100 - 50/3 * 0.6) = (210, 90) and half sizes (100 + 100/6 * 0.6, 50 - 50/6 * 1.2) =
    (110, 40): the box (100, 50, 320, 130), whose IoU with the label is 16000 / (17600 + 20000 - 16000)."""
    z = iter([0.3, -0.6, 0.6, -1.2])
    calls = []

    def normal(mean, sd):
        calls.append((mean, sd))
        return mean + sd * next(z)
    out, trials = jr.scalar_jitter([[100.0, 50.0, 300.0, 150.0]], 0.7, (375, 1242), normal=normal)
    assert trials == [1] and np.allclose(out[0], [100, 50, 320, 130], atol=1e-12)
    assert calls == [(200.0, 100 / 3), (100.0, 50 / 3), (100.0, 100 / 6), (50.0, 50 / 6)]
    assert abs(jr._overlap_ratio((100.0, 50.0, 320.0, 130.0), (100.0, 50.0, 300.0, 150.0)) - 16000 / 21600) < 1e-15
    assert jr._overlap_ratio((0.0, 0.0, 10.0, 10.0), (10.0, 0.0, 20.0, 10.0)) == 0.0
    # the clip: a trial past the right and bottom borders ends at w - 1, h - 1
    z = iter([0.0, 0.0, 6.0, 6.0] + [0.0] * 4)
    # (IoU 9800 / 22999 = 0.426)
    out, trials = jr.scalar_jitter([[1100.0, 300.0, 1240.0, 370.0]], 0.4, (375, 1242), normal=lambda m, s: m + s * next(z))
    assert trials == [1] and list(out[0]) == [1030.0, 265.0, 1241.0, 374.0]
    # below the threshold is rejected, the next trial is taken; under 10 px nothing is drawn
    z = iter([3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    out, trials = jr.scalar_jitter([[100.0, 50.0, 300.0, 150.0], [5.0, 5.0, 14.0, 90.0]], 0.7, (375, 1242),
                                   normal=lambda m, s: m + s * next(z))
    assert trials == [2, 0] and list(out[0]) == [100.0, 50.0, 300.0, 150.0] and list(out[1]) == [5.0, 5.0, 14.0, 90.0]


def test_restatement_properties_and_cap():
    rng = np.random.default_rng(3)
    h, w = 370, 1224
    boxes = _boxes(rng, 2000, h, w)
    n = len(boxes)
    flags = (np.arange(n) % 5 != 0).astype(np.int32)
    out, trials, near = jr.jitter_boxes(boxes, flags, [(h, w)] * n, np.arange(n) % 17, np.arange(n), 9, 1, 0.7)
    assert not near.any() and trials.max() <= 4096
    small = (boxes[:, 2] - boxes[:, 0] < 10) | (boxes[:, 3] - boxes[:, 1] < 10)
    left = small | (flags == 0)
    assert (out[left] == boxes[left]).all() and (trials[left] == 0).all() and (trials[~left] >= 1).all()
    assert (jr.two_d_iou_pairs(out, boxes) >= 0.7).all()
    assert out[:, 0].min() >= 0 and out[:, 1].min() >= 0 and out[:, 2].max() <= w - 1 and out[:, 3].max() <= h - 1
    # the cap: at IoU 1 nothing is accepted; the box is kept and max_trials + 1 reported
    out, trials, _ = jr.jitter_boxes(boxes[~small][:5], [1] * 5, [(h, w)] * 5, [0] * 5, range(5), 0, 0, 1.0,
                                     max_trials=8)
    assert (trials == 9).all() and (out == boxes[~small][:5]).all()
    # a slot's result does not depend on its neighbours
    one, t1, _ = jr.jitter_boxes(boxes[7:8], flags[7:8], [(h, w)], [7 % 17], [7], 9, 1, 0.7)
    full, tf, _ = jr.jitter_boxes(boxes, flags, [(h, w)] * n, np.arange(n) % 17, np.arange(n), 9, 1, 0.7)
    assert one[0].tobytes() == full[7].tobytes() and t1[0] == tf[7]


def test_gpu_comparison_cases_have_no_trial_at_the_threshold():
    """The seeds of tests/test_kitti_aug_gpu.py are chosen so that the restatement alone leaves no slot out."""
    import jitter_cases
    total = 0
    for case in jitter_cases.cases():
        _, trials, near = jr.jitter_boxes(case['boxes'], case['flags'], case['hw'], case['frame_index'], case['slot'],
                                          case['seed'], case['epoch'], case['thr'])
        assert not near.any(), (case['seed'], case['epoch'], case['thr'], int(near.sum()))
        assert trials.max() <= 4096
        total += len(trials)
    assert total >= 20000

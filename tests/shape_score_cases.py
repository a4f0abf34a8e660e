"""The clouds mpsr_shape_scores is tried on (tests/test_shape_score.py on the restatement, tests/test_shape_score_gpu.py
on the device).  case(name) -> dict(a (n,P,3), b (n,Q,3) float32, mask_a (n,P), mask_b (n,Q) float32 or None,
thresholds); restated(name) is its restatement, computed once.

The kernel's sizes: a workgroup takes a slab of 1024 queries (256 threads x 4) and stages the searched cloud in LDS
tiles of 1024 points, padded to runs of 8.  So the shapes: one point; fewer points than a run; 255 / 257 (a thread
short of and past one pass of the staging loop); 256 against one whole tile; 1025 against 1023 (a second slab and a
second tile of one point; a tile one short); 2304 = 48 x 48, three slabs and three tiles, against itself and against
500.  n = 1, 3, 4 and 33: one box past the 32 of the frame the kernel is sized for.
"""
import functools

import numpy as np

import shape_score_restatement as restatement

TILE = SLAB = 1024


def _cloud(rng, n, points, scale=2.0):
    return (rng.standard_normal((n, points, 3)) * scale).astype(np.float32)


def _random_mask(rng, n, points, share=0.25):
    return (rng.uniform(size=(n, points)) < share).astype(np.float32)


def _grid(rng, n, points, cells=8, step=2.0 ** -4):
    """points on a dyadic grid: every difference, product and sum of the distance is exact, ties are frequent"""
    return (rng.integers(0, cells, size=(n, points, 3)) * step).astype(np.float32)


def _one_point():
    rng = np.random.default_rng(1)
    return dict(a=_cloud(rng, 1, 1), b=_cloud(rng, 1, 1), mask_a=None, mask_b=None, thresholds=())


def _short():
    rng = np.random.default_rng(2)
    return dict(a=_cloud(rng, 3, 7), b=_cloud(rng, 3, 3), mask_a=_random_mask(rng, 3, 7, 0.5),
                mask_b=_random_mask(rng, 3, 3, 0.7), thresholds=(1.5,))


def _many_boxes():
    rng = np.random.default_rng(3)
    return dict(a=_cloud(rng, 33, 255), b=_cloud(rng, 33, 257), mask_a=_random_mask(rng, 33, 255),
                mask_b=_random_mask(rng, 33, 257), thresholds=(0.25, 0.5, 1.0))


def _null_masks():
    rng = np.random.default_rng(4)
    return dict(a=_cloud(rng, 3, 256), b=_cloud(rng, 3, 1024), mask_a=None, mask_b=None,
                thresholds=(0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 3.2, 6.4))


def _hostile():
    """NaN and +-inf coordinates and NaN mask entries on both sides, under a random mask and outside it"""
    rng = np.random.default_rng(5)
    a, b = _cloud(rng, 3, 1025), _cloud(rng, 3, 1023)
    ma, mb = _random_mask(rng, 3, 1025), _random_mask(rng, 3, 1023)
    for cloud, mask in ((a, ma), (b, mb)):
        n, points = mask.shape
        for value in (np.nan, np.inf, -np.inf):
            for _ in range(12):
                cloud[rng.integers(n), rng.integers(points), rng.integers(3)] = value
        for _ in range(12):
            mask[rng.integers(n), rng.integers(points)] = np.nan
        mask[:, -1] = 1.0  # the last tile's only point
    a[1, -1, 0] = np.nan
    return dict(a=a, b=b, mask_a=ma, mask_b=mb, thresholds=(0.25, 0.5, 1.0))


def _empty_tile_and_slab():
    """mask_a empties a's second thousand: one whole LDS tile where a is searched, one whole slab where it asks;
    mask_b the same of b's first thousand"""
    rng = np.random.default_rng(6)
    ma, mb = _random_mask(rng, 3, 2304), _random_mask(rng, 3, 2304)
    ma[:, TILE:2 * TILE] = 0.0
    mb[:, 0:SLAB] = 0.0
    return dict(a=_cloud(rng, 3, 2304), b=_cloud(rng, 3, 2304), mask_a=ma, mask_b=mb, thresholds=(0.25, 0.5, 1.0))


def _frame():
    """one box more than the 32 of a frame, the map's 2304 points against 500"""
    rng = np.random.default_rng(7)
    return dict(a=_cloud(rng, 33, 2304), b=_cloud(rng, 33, 500), mask_a=_random_mask(rng, 33, 2304),
                mask_b=_random_mask(rng, 33, 500), thresholds=(0.25, 0.5, 1.0))


def _empty_sides():
    """box 0: no valid a; box 1: no valid b; box 2: one valid point on each side; box 3: neither side"""
    rng = np.random.default_rng(8)
    ma, mb = _random_mask(rng, 4, 255), _random_mask(rng, 4, 257)
    ma[0] = 0.0
    mb[1] = 0.0
    ma[2], mb[2] = 0.0, 0.0
    ma[2, 200], mb[2, 256] = 1.0, 0.5
    ma[3], mb[3] = 0.0, -1.0
    return dict(a=_cloud(rng, 4, 255), b=_cloud(rng, 4, 257), mask_a=ma, mask_b=mb, thresholds=(0.25, 0.5, 1.0))


def _ties():
    """duplicates and exact ties on a dyadic grid; the thresholds are one, two and three of the grid's steps of 2^-4,
    so many d are exactly their squares: `<=` is hit on the boundary"""
    rng = np.random.default_rng(9)
    a, b = _grid(rng, 3, 256), _grid(rng, 3, 1024, cells=5)
    a[:, 10:20] = a[:, 0:10]
    return dict(a=a, b=b, mask_a=None, mask_b=None, thresholds=(2.0 ** -4, 2.0 ** -3, 3 * 2.0 ** -4))


def _overflow():
    """coordinates of 1e20: the squares overflow, d = +inf, and so are the sums and the Hausdorff distance"""
    rng = np.random.default_rng(10)
    a, b = _cloud(rng, 1, 7), _cloud(rng, 1, 3)
    a[0, 2] = (1e20, 0.0, 0.0)
    return dict(a=a, b=b, mask_a=None, mask_b=None, thresholds=(1.0,))


def _constructed():
    """a = the 48 x 48 grid of spacing 2^-4 (below 8 m) at z = 1; b = a shifted by (3, 4, 0) 2^-8.  Every point's
    nearest neighbour is its own copy: every d = 25 2^-16, every root 5 2^-8, every sum exact in any order.  (With a
    shift of (3, 4, 0) 2^-6 -- a whole spacing in y -- the nearest point would be a neighbour's copy at 2^-6 and the
    edge rows' roots would not be exact; the shift is 2^-8 so that the property holds.)  The second threshold is
    the root itself."""
    k = np.arange(48, dtype=np.float64) * 2.0 ** -4
    a = np.stack(list(np.meshgrid(k, k, indexing='ij')) + [np.ones((48, 48))], -1).reshape(1, 2304, 3)
    b = a + np.array([3, 4, 0]) * 2.0 ** -8
    assert np.array_equal(a.astype(np.float32), a) and np.array_equal(b.astype(np.float32), b)
    return dict(a=a.astype(np.float32), b=b.astype(np.float32), mask_a=None, mask_b=None,
                thresholds=(4 * 2.0 ** -8, 5 * 2.0 ** -8))


def _clone():
    """b is a copy of a with the same mask: every d is 0, precision = recall = fscore = 1, hausdorff 0"""
    rng = np.random.default_rng(12)
    a, mask = _cloud(rng, 3, 2304), _random_mask(rng, 3, 2304)
    a[0, 5, 1], a[1, 7, 2] = np.nan, np.inf
    return dict(a=a, b=a.copy(), mask_a=mask, mask_b=mask.copy(), thresholds=(0.05, 0.1, 0.2))


_CASES = dict(one_point=_one_point, short=_short, many_boxes=_many_boxes, null_masks=_null_masks, hostile=_hostile,
              empty_tile_and_slab=_empty_tile_and_slab, frame=_frame, empty_sides=_empty_sides, ties=_ties,
              overflow=_overflow, constructed=_constructed, clone=_clone)
NAMES = tuple(_CASES)
# null masks and finite clouds: d is mpsr_nn_distance_fwd's
NN_DISTANCE_NAMES = ('one_point', 'null_masks', 'ties', 'overflow', 'constructed')
# every term and every partial sum is exact: the sums are bit for bit
EXACT_SUM_NAMES = ('constructed', 'clone')


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def restated(name):
    c = case(name)
    r = restatement.shape_scores(c['a'], c['b'], c['mask_a'], c['mask_b'], c['thresholds'])
    for v in r.values():
        v.setflags(write=False)
    return r

"""The grids mpsr_surface_scores is tried on (tests/test_surface_score.py on the restatement,
tests/test_surface_score_gpu.py on the device).  case(name) -> dict(a, b (n, h, w, 3) float32, mask_a, mask_b (n, h w)
float32 or None, thresholds, max_edge); restated(name) is its vectorised restatement, computed once;
loop_queries(name) the point indices the plain-loop restatement is run on (None: every point).

The kernel's sizes: a workgroup takes a slab of 512 queries (256 threads x 2), stages the searched grid's points in
LDS tiles of 1024 and its triangles 256 ids to a pass.  So the grids: (1, 1), (1, 5) (no cell); (2, 2), (2, 3), (3, 2)
(two and four triangles); (5, 7) (48 triangles, one pass); (17, 16) (272 points, 480 triangles: a second pass, threads
without a triangle in it); (48, 48) (five slabs, three point tiles, eighteen passes).  n = 1, 3, 4 and 33.
"""
import functools

import numpy as np

import surface_score_restatement as restatement

S = 2.0 ** -4   # the dyadic grids' spacing
U = 2.0 ** -8   # and their unit of height
INF = float('inf')


def _plane(h, w, z=0.0, di=0.0, dj=0.0):
    """(h, w, 3) float64: point (i, j) at ((i + di) S, (j + dj) S, z)"""
    i, j = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing='ij')
    return np.stack([(i + di) * S, (j + dj) * S, np.full((h, w), z)], -1)


def _f32(x):
    y = np.asarray(x, np.float32)
    assert np.array_equal(y.astype(np.float64), np.asarray(x, np.float64), equal_nan=True)
    return y


def _surface(rng, n, h, w, noise=0.02):
    """a bumpy sheet over a grid of about 8 cm: (n, h, w, 3) float32"""
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    base = np.stack([0.08 * i, 0.08 * j, 0.3 * np.sin(0.4 * i) * np.cos(0.3 * j)], -1)
    return (base[None] + rng.standard_normal((n, h, w, 3)) * noise).astype(np.float32)


def _random_mask(rng, n, points, share):
    return (rng.uniform(size=(n, points)) < share).astype(np.float32)


def _one_point():
    rng = np.random.default_rng(1)
    return dict(a=_surface(rng, 1, 1, 1), b=_surface(rng, 1, 1, 1), mask_a=None, mask_b=None, thresholds=(),
                max_edge=0.5)


def _row():
    """(1, 5): points and no cell"""
    rng = np.random.default_rng(2)
    return dict(a=_surface(rng, 3, 1, 5), b=_surface(rng, 3, 1, 5), mask_a=_random_mask(rng, 3, 5, 0.7),
                mask_b=_random_mask(rng, 3, 5, 0.7), thresholds=(0.05,), max_edge=0.5)


def _quad():
    """(2, 2): b is one dyadic cell in z = 0; a's four points sit exactly above the vertex v00, above the middle of the
    diagonal that the two triangles share, above the middle of the boundary edge v00 - v01, and half a cell beyond that
    edge; box 1 the same mirrored in z, box 2 with a's last point masked"""
    b = _plane(2, 2)
    a = np.array([[[0, 0, 3 * U], [S / 2, S / 2, 3 * U]], [[0, S / 2, 3 * U], [-S / 2, S / 2, 3 * U]]])
    a = np.stack([a, a * [1, 1, -1], a])
    mask_a = np.ones((3, 4), np.float32)
    mask_a[2, 3] = 0
    return dict(a=_f32(a), b=_f32(np.stack([b] * 3)), mask_a=mask_a, mask_b=None, thresholds=(2 * U, 3 * U, S),
                max_edge=INF)


def _above_and_beyond():
    """(5, 7): b the dyadic plane; a's points, row by row: exactly above vertices; above the middles of the edges along
    j (interior from row 1 on, row 0 on the boundary); above the middles of the edges along i; above the middles of
    the diagonals; and a last row half a cell beyond the boundary."""
    b = _plane(5, 7)
    a = np.stack([_plane(1, 7, 3 * U, 2, 0)[0], _plane(1, 7, 3 * U, 1, 0.5)[0], _plane(1, 7, 3 * U, 0.5, 0)[0],
                  _plane(1, 7, 3 * U, 1.5, 0.5)[0], _plane(1, 7, 3 * U, -0.5, 0.25)[0]])
    a[1, 6], a[3, 6] = (0, 2.5 * S, 3 * U), (4 * S, 5.5 * S, 3 * U)  # (j + 0.5 would leave the grid: boundary edges)
    return dict(a=_f32(a[None]), b=_f32(b[None]), mask_a=None, mask_b=None,
                thresholds=tuple(k * U for k in (1, 2, 3, 4, 5, 8, 16, 32)), max_edge=0.5)


def _dyadic_plane():
    """(17, 16), three boxes: b is the grid of spacing 2^-4 in z = 0, a's point (i, j) sits a quarter cell inside
    cell (i, j) at height 3 2^-8, and a's last row and column, which have no cell, are masked.  Every d_a is the face
    term 9 2^-16 where the nearest point is at 41 2^-16 (two quarter cells of 2^-6 and the height: 16 + 16 + 9); every
    root and every sum of side a is exact in any order.  Side b: every d_b is dyadic, so sum d_b is exact; its points
    inside a's sheet are at 9 2^-16 and those on the near boundary at 25 2^-16, but the far boundary is three quarters
    of a cell from a's last valid row, 153 2^-16, whose root is not exact: sum sqrt d_b is held to the bound only.
    Boxes 1 and 2 are box 0 moved by whole cells, which changes no difference.  The thresholds sit below, on and above
    the height."""
    h, w = 17, 16
    b, a = _plane(h, w), _plane(h, w, 3 * U, 0.25, 0.25)
    mask_a = np.ones((h, w), np.float32)
    mask_a[-1, :], mask_a[:, -1] = 0, 0
    shift = np.array([[0, 0, 0], [3 * S, -2 * S, S], [-5 * S, 7 * S, 0]])[:, None, None, :]
    return dict(a=_f32(a[None] + shift), b=_f32(b[None] + shift), mask_a=np.stack([mask_a.reshape(-1)] * 3),
                mask_b=None, thresholds=(2 * U, 3 * U, S), max_edge=0.5)


def _max_edge_zero():
    rng = np.random.default_rng(5)
    return dict(a=_surface(rng, 3, 5, 7), b=_surface(rng, 3, 5, 7), mask_a=_random_mask(rng, 3, 35, 0.8),
                mask_b=_random_mask(rng, 3, 35, 0.8), thresholds=(0.05, 0.1, 0.2), max_edge=0.0)


def _max_edge_inf():
    """every triangle of valid points is kept, those across a jump of 50 m included"""
    rng = np.random.default_rng(6)
    b = _surface(rng, 3, 5, 7)
    b[:, 2:, :, 2] += 50.0
    return dict(a=_surface(rng, 3, 5, 7), b=b, mask_a=None, mask_b=_random_mask(rng, 3, 35, 0.9), thresholds=(0.05,),
                max_edge=INF)


def _edge_on_the_limit():
    """(2, 3) with max_edge 0.5: the float32 squared length of b's edge v(0,0) - v(0,1) is exactly 0.25 = max_edge^2
    (kept), that of v(0,1) - v(0,2) is the next float32 above 0.25 (dropped)."""
    dy = np.float32(2.0 ** -12.5)
    b = np.array([[[0, 0, 0], [0.5, 0, 0], [1.0, dy, 0]], [[0.25, 0.25, 0], [0.75, 0.25, 0], [1.25, 0.25, 0]]],
                 np.float32)
    over = restatement._len2_f32(b[0, 1], b[0, 2])
    assert restatement._len2_f32(b[0, 0], b[0, 1]) == np.float32(0.25)
    assert over == np.nextafter(np.float32(0.25), np.float32(1)), over
    rng = np.random.default_rng(7)
    a = (b + rng.standard_normal(b.shape) * 0.05).astype(np.float32)
    return dict(a=a[None], b=b[None], mask_a=None, mask_b=None, thresholds=(0.05,), max_edge=0.5)


def _holes():
    """(17, 16): rectangular holes in both masks; b's point (8, 8) is valid with its eight neighbours masked, so all
    six triangles it is a corner of are dropped: it stays part of the surface as a point"""
    rng = np.random.default_rng(8)
    ma, mb = np.ones((3, 17, 16), np.float32), np.ones((3, 17, 16), np.float32)
    ma[:, 2:6, 3:9], ma[:, 10:, :2], mb[:, 12:15, 5:14] = 0, 0, 0
    mb[:, 7:10, 7:10] = 0
    mb[:, 8, 8] = 1
    return dict(a=_surface(rng, 3, 17, 16), b=_surface(rng, 3, 17, 16), mask_a=ma.reshape(3, -1),
                mask_b=mb.reshape(3, -1), thresholds=(0.05, 0.1, 0.2), max_edge=0.5)


def _no_triangle():
    """b's mask is a checkerboard: every triangle has two neighbours along j among its corners, so none is kept; the
    side is a cloud, not an empty side"""
    rng = np.random.default_rng(9)
    i, j = np.meshgrid(np.arange(5), np.arange(7), indexing='ij')
    mb = ((i + j) % 2 == 0).astype(np.float32).reshape(1, -1)
    return dict(a=_surface(rng, 3, 5, 7), b=_surface(rng, 3, 5, 7), mask_a=None, mask_b=np.repeat(mb, 3, 0),
                thresholds=(0.05, 0.1, 0.2), max_edge=0.5)


def _random_masks():
    """one box more than the 32 of a frame, ~25 % masks"""
    rng = np.random.default_rng(10)
    a = _surface(rng, 33, 17, 16)
    b = (a + rng.standard_normal(a.shape) * 0.03).astype(np.float32)
    return dict(a=a, b=b, mask_a=_random_mask(rng, 33, 272, 0.75), mask_b=_random_mask(rng, 33, 272, 0.75),
                thresholds=(0.05, 0.1, 0.2), max_edge=0.5)


def _degenerate():
    """(3, 2): box 0 has duplicate vertices (b's first row is one point twice), box 1's b is collinear, box 2's b is
    one point six times; every triangle is kept and adds no face term, none or some edge terms, and no division by 0"""
    rng = np.random.default_rng(11)
    b = _surface(rng, 3, 3, 2)
    b[0, 0, 1] = b[0, 0, 0]
    b[1] = np.array([0.25, -0.5, 0.125])[None, None, :] * np.arange(6).reshape(3, 2, 1)
    b[2] = b[2, 0, 0]
    return dict(a=_surface(rng, 3, 3, 2), b=b, mask_a=None, mask_b=None, thresholds=(0.1,), max_edge=INF)


def _clone():
    """b is a copy of a with the same mask: every d is 0, precision = recall = fscore = 1, hausdorff 0"""
    rng = np.random.default_rng(12)
    a, mask = _surface(rng, 3, 17, 16), _random_mask(rng, 3, 272, 0.6)
    a[0, 5, 1, 1], a[1, 7, 2, 2] = np.nan, np.inf
    return dict(a=a, b=a.copy(), mask_a=mask, mask_b=mask.copy(), thresholds=(0.05, 0.1, 0.2), max_edge=0.5)


def _hostile():
    """NaN and +-inf coordinates and NaN mask entries on both sides, under a random mask and outside it"""
    rng = np.random.default_rng(13)
    a, b = _surface(rng, 3, 5, 7), _surface(rng, 3, 5, 7)
    ma, mb = _random_mask(rng, 3, 35, 0.8), _random_mask(rng, 3, 35, 0.8)
    for grid, mask in ((a, ma), (b, mb)):
        for value in (np.nan, np.inf, -np.inf):
            for _ in range(3):
                grid[rng.integers(3), rng.integers(5), rng.integers(7), rng.integers(3)] = value
        for _ in range(4):
            mask[rng.integers(3), rng.integers(35)] = np.nan
    a[1, 0, 0, 0], ma[1, 0] = np.nan, 1.0
    return dict(a=a, b=b, mask_a=ma, mask_b=mb, thresholds=(0.05, 0.1, 0.2), max_edge=0.5)


def _overflow():
    """coordinates of 1e20 with max_edge +inf: float32 squares overflow (len2 = +inf is kept, d_point = +inf), the
    fp64 terms do not, so a query out there, beside the edge from b's far vertex, gets a finite d from that edge"""
    rng = np.random.default_rng(14)
    a, b = _surface(rng, 1, 2, 3), _surface(rng, 1, 2, 3)
    a[0, 0, 1] = (1e15, 5e19, 5e19)
    b[0, 1, 2] = (0.0, 1e20, 1e20)
    return dict(a=a, b=b, mask_a=None, mask_b=None, thresholds=(1.0,), max_edge=INF)


def _empty_sides():
    """box 0: no valid a; box 1: no valid b; box 2: one valid point on each side; box 3: neither side"""
    rng = np.random.default_rng(15)
    ma, mb = np.ones((4, 6), np.float32), np.ones((4, 6), np.float32)
    ma[0] = 0.0
    mb[1] = 0.0
    ma[2], mb[2] = 0.0, 0.0
    ma[2, 4], mb[2, 5] = 1.0, 0.5
    ma[3], mb[3] = 0.0, -1.0
    return dict(a=_surface(rng, 4, 2, 3), b=_surface(rng, 4, 2, 3), mask_a=ma, mask_b=mb, thresholds=(0.05, 0.1, 0.2),
                max_edge=0.5)


def _half_cylinder():
    """One half-cylinder, 4 m long with radius 0.9 m, sampled twice on 48 x 48 grids half a cell apart: both maps are
    the same surface, and the point scores see the sampling."""
    def sample(offset):
        i, j = np.meshgrid(np.arange(48) + offset, np.arange(48) + offset, indexing='ij')
        theta = np.pi * j / 48
        return np.stack([4.0 * i / 48, 0.9 * np.cos(theta), 0.9 * np.sin(theta)], -1).astype(np.float32)
    return dict(a=sample(0.25)[None], b=sample(0.75)[None], mask_a=None, mask_b=None, thresholds=(0.05, 0.1, 0.2),
                max_edge=0.5)


_CASES = dict(one_point=_one_point, row=_row, quad=_quad, above_and_beyond=_above_and_beyond,
              dyadic_plane=_dyadic_plane, max_edge_zero=_max_edge_zero, max_edge_inf=_max_edge_inf,
              edge_on_the_limit=_edge_on_the_limit, holes=_holes, no_triangle=_no_triangle,
              random_masks=_random_masks, degenerate=_degenerate, clone=_clone, hostile=_hostile, overflow=_overflow,
              empty_sides=_empty_sides, half_cylinder=_half_cylinder)
NAMES = tuple(_CASES)
# the sums (of sums[:, 0:4]) whose every term and partial sum is exact: bit for bit
EXACT_SUMS = dict(dyadic_plane=(0, 1, 3), clone=(0, 1, 2, 3))
# the plain loop costs microseconds per (query, triangle) pair: on the larger grids it runs on every STEP-th point
_LOOP_STEP = dict(holes=3, random_masks=7, clone=3, dyadic_plane=3, half_cylinder=23)


def loop_queries(name):
    if name not in _LOOP_STEP:
        return None
    c = case(name)
    return list(range(0, c['a'].shape[1] * c['a'].shape[2], _LOOP_STEP[name]))


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
    r = restatement.surface_scores(c['a'], c['b'], c['mask_a'], c['mask_b'], c['thresholds'], c['max_edge'])
    for v in r.values():
        v.setflags(write=False)
    return r

"""The catalogue of surface-rendering cases shared by tests/test_scene_surface.py (properties of the restatement) and
tests/test_scene_surface_gpu.py (the kernels against the restatement).  A case is the dict tests/surface_restatement.py
takes; `expected(name)` renders it once, `ground_truth(name)` is its seeded ground truth and `expected_scores(name)`
the restatement's scores against it.

The shapes are the smallest at which each rule can go wrong: maps of 2 x 2 (one cell) to 48 x 48, frames of 5 x 7 to
100 x 104 pixels.  Under pow2_camera(4, 0, 0) a point (col z / 4, row z / 4, z) with z a power of two projects to
(col, row) exactly.
"""
import functools

import numpy as np

import scene_cases
import scene_score_cases
import surface_restatement

SHAPES = scene_cases.SHAPES  # (5, 7), (8, 8), (6, 13)
F = 4.0
INF = float('inf')


def at_pixels(cols, rows, z, f=F, cx=0.0, cy=0.0):
    """(Hm,Wm,3) float32: the points that project to (cols, rows) at depth z under pow2_camera(f, cx, cy)."""
    cols, rows, z = np.broadcast_arrays(np.asarray(cols, np.float64), np.asarray(rows, np.float64),
                                        np.asarray(z, np.float64))
    return np.stack([(cols - cx) * z / f, (rows - cy) * z / f, z], -1).astype(np.float32)


def plane(col0, row0, dcol, drow, mh, mw, z=4.0):
    """A fronto-parallel (mh, mw) grid: vertex (i, j) on pixel (col0 + j dcol, row0 + i drow)."""
    rows, cols = np.meshgrid(row0 + drow * np.arange(mh), col0 + dcol * np.arange(mw), indexing='ij')
    return at_pixels(cols, rows, z)


def _case(maps, box_frame, shapes, cams=None, **options):
    cams = [scene_cases.pow2_camera(F, 0.0, 0.0)] * len(shapes) if cams is None else cams
    return dict(xyz=np.stack(maps).astype(np.float32), box_frame=np.asarray(box_frame, np.int64),
                cam_p=np.stack(cams).astype(np.float64), shapes=list(shapes), **options)


def _one_frame_each(maps, shape, **options):
    return _case(maps, np.arange(len(maps)), [shape] * len(maps), **options)


def cell_case():
    return _case([plane(1, 1, 3, 2, 2, 2)], [0], [SHAPES[0]])


def fractional_2x3_case():
    cols = [[0.3, 3.7, 6.2], [1.1, 4.4, 7.9]]
    rows = [[0.6, 0.2, 1.3], [5.5, 6.1, 4.7]]
    z = [[2.0, 2.5, 3.0], [2.25, 2.75, 2.5]]
    return _case([at_pixels(cols, rows, z)], [0], [SHAPES[1]])


def on_centres_case():
    """4 x 5 vertices two pixels apart, all on pixel centres: every shared edge and every cell diagonal runs through
    pixel centres.  Spans columns [2, 10] and rows [1, 7]."""
    return _case([plane(2, 1, 2, 2, 4, 5)], [0], [(9, 12)])


ON_CENTRES_SPAN = (2, 10, 1, 7)  # c0, c1, r0, r1


def mirrored_case():
    """on_centres with the map's columns reversed: the same surface, every triangle facing the other way."""
    return _case([plane(2, 1, 2, 2, 4, 5)[:, ::-1]], [0], [(9, 12)])


def snap_halfway_case():
    """One 2 x 2 box per frame whose first vertex has u 256 = k + 0.5 exactly (k even and odd), or is one float32 ulp
    to either side, on one axis at a time.  pow2_camera(1, 0, 0): u0 / u2 = x / z, exact with z = 2.  The depths differ
    from vertex to vertex, so that a vertex one fixed-point unit off changes the interpolated depths."""
    maps = []
    z = np.asarray([[2.0, 3.0], [2.5, 3.5]])
    for axis in (0, 1):
        for k in (0, 1, 2, 3):
            half = np.float32((1.0 + (k + 0.5) / 256.0) * 2.0)  # x = col z, exact
            for v in (np.nextafter(half, np.float32(-np.inf)), half, np.nextafter(half, np.float32(np.inf))):
                m = at_pixels([[1.0, 4.0], [1.0, 4.0]], [[1.0, 1.0], [3.0, 3.0]], z, f=1.0)
                m[0, 0, axis] = v
                maps.append(m)
    return _one_frame_each(maps, (5, 6), cams=[scene_cases.pow2_camera(1.0, 0.0, 0.0)] * len(maps), max_edge_dz=INF)


INVALID_KINDS = ('control', 'mask_zero', 'nan_x', 'inf_y', 'minus_inf_z', 'z_zero', 'z_negative', 'u2_not_positive',
                 'u_2_to_20', 'u_below_2_to_20', 'keep_zero')


def invalid_case():
    """One 3 x 3 box per frame, vertices on pixels 1, 3, 5; the CENTRE vertex is invalid in one way per box: only the
    six triangles that touch it disappear.  u2_not_positive: a camera whose third row is (0.5, 0, 1, 0) and a centre
    vertex at x = -10, z = 4: u2 = -1.  u_2_to_20: u0 / u2 = 2^20 exactly (invalid); u_below_2_to_20: one ulp less (a
    valid vertex; its triangles fall to the span limit).  keep_zero: the whole box is out."""
    maps, cams = [], []
    mask = np.ones((len(INVALID_KINDS), 3, 3), np.float32)
    keep = np.ones(len(INVALID_KINDS), np.int32)
    for n, kind in enumerate(INVALID_KINDS):
        m = plane(1, 1, 2, 2, 3, 3)
        cam = scene_cases.pow2_camera(F, 0.0, 0.0)
        if kind == 'mask_zero':
            mask[n, 1, 1] = 0.0
        elif kind == 'nan_x':
            m[1, 1, 0] = np.nan
        elif kind == 'inf_y':
            m[1, 1, 1] = np.inf
        elif kind == 'minus_inf_z':
            m[1, 1, 2] = -np.inf
        elif kind == 'z_zero':
            m[1, 1, 2] = 0.0
        elif kind == 'z_negative':
            m[1, 1, 2] = -4.0
        elif kind == 'u2_not_positive':
            cam[2] = [0.5, 0.0, 1.0, 0.0]
            m[1, 1, 0] = -10.0
        elif kind == 'u_2_to_20':
            m[1, 1, 0] = 2.0 ** 20
        elif kind == 'u_below_2_to_20':
            m[1, 1, 0] = np.nextafter(np.float32(2.0 ** 20), np.float32(0.0))
        elif kind == 'keep_zero':
            keep[n] = 0
        maps.append(m)
        cams.append(cam)
    return _one_frame_each(maps, (7, 7), cams=cams, mask=mask, keep=keep)


EDGE_DZ_KINDS = ('met_at_v00', 'exceeded_at_v00', 'met_at_v11', 'exceeded_at_v11', 'met_below', 'exceeded_below')


def edge_dz_case():
    """max_edge_dz = 0.5, one 2 x 2 box per frame: one vertex 0.5 m behind (kept: the comparison is strict) or one
    float32 ulp more (dropped) -- or in front of -- the other three at 4 m."""
    maps = []
    above = np.nextafter(np.float32(4.5), np.float32(np.inf))
    below = np.nextafter(np.float32(3.5), np.float32(-np.inf))
    for kind, (i, j, z) in zip(EDGE_DZ_KINDS, ((0, 0, 4.5), (0, 0, above), (1, 1, 4.5), (1, 1, above), (0, 0, 3.5),
                                               (0, 0, below))):
        zz = np.full((2, 2), 4.0)
        zz[i, j] = np.float64(z)
        maps.append(at_pixels([[1.0, 5.0], [1.0, 5.0]], [[1.0, 1.0], [3.0, 3.0]], zz))
    return _one_frame_each(maps, SHAPES[0], max_edge_dz=0.5)


SPAN_KINDS = (('cols_1_4', 1.0, 4.0, 1.0, 2.0, True), ('cols_1_5', 1.0, 5.0, 1.0, 2.0, False),
              ('cols_half', 0.5, 4.5, 1.0, 2.0, True), ('cols_wider_half', 0.5, 5.0, 1.0, 2.0, False),
              ('rows_1_5', 1.0, 2.0, 1.0, 5.0, False), ('rows_2_5', 1.0, 2.0, 2.0, 5.0, True),
              ('negative_4', -2.0, 1.0, 1.0, 2.0, True), ('negative_half_4', -2.5, 1.5, 1.0, 2.0, True),
              ('negative_5', -3.0, 1.0, 1.0, 2.0, False), ('negative_rows_5', 1.0, 2.0, -3.5, 1.25, False),
              ('negative_rows_4', 1.0, 2.0, -2.75, 1.25, True))


def span_case():
    """max_span_px = 4, one 2 x 2 box per frame from (c0, r0) to (c1, r1): an extent of exactly 4 (drawn) and of 5
    (dropped), with fractional and negative bounds: floor(max) - ceil(min) + 1."""
    maps = [at_pixels([[c0, c1], [c0, c1]], [[r0, r0], [r1, r1]], 4.0) for _, c0, c1, r0, r1, _ in SPAN_KINDS]
    return _one_frame_each(maps, SHAPES[1], max_span_px=4)


def degenerate_case():
    """Box 0: every vertex on one line (all areas 0).  Box 1: a 3 x 4 map folded over itself (columns 1, 5, 3, 7: the
    middle cells face the other way and overlap their neighbours).  Box 2: the first two columns coincide (the
    triangles between them have no area)."""
    line = at_pixels([[1, 2, 3], [2, 3, 4], [3, 4, 5]], [[1, 2, 3], [2, 3, 4], [3, 4, 5]], 4.0)
    line = np.concatenate([line, line[:, -1:]], 1)  # (3, 4)
    rows = np.repeat(np.asarray([[1.0], [3.0], [6.0]]), 4, 1)
    fold = at_pixels(np.tile(np.asarray([1.0, 5.0, 3.0, 7.0]), (3, 1)), rows,
                     np.tile(np.asarray([4.0, 4.25, 4.5, 4.75]), (3, 1)))
    twice = at_pixels(np.tile(np.asarray([2.0, 2.0, 4.0, 6.5]), (3, 1)), rows, 2.0)
    return _one_frame_each([line, fold, twice], (8, 9))


def identical_case():
    """Two boxes with the same map in one frame (the lower id wins every pixel), a third one nearer over a corner."""
    m = plane(1, 1, 2, 2, 3, 3)
    near = plane(4, 3, 1, 1, 3, 3, z=2.0)
    return _case([m, m.copy(), near], [0, 0, 0], [SHAPES[1]])


def boxes_255_case():
    """255 boxes of one cell in ONE frame, box b over the pixel (1 + b % 7, 1 + (b // 7) % 7), nearer on every round
    over the image."""
    maps = []
    for b in range(255):
        c, r = b % 7, (b // 7) % 7
        maps.append(plane(c, r, 1, 1, 2, 2, z=4.0 * 2.0 ** -(b // 49)))
    return _case(maps, np.zeros(255, np.int64), [SHAPES[1]])


def off_image_case():
    """Boxes partly and wholly outside a 5 x 7 image, on all sides, with negative coordinates."""
    maps = [plane(-3, -2, 2, 2, 3, 4, z=8.0),      # columns -3 .. 3, rows -2 .. 2
            plane(-9, 1, 2, 1, 3, 4, z=4.0),       # wholly to the left: columns -9 .. -3
            plane(1, 6, 2, 2, 3, 4, z=4.0),        # wholly below
            plane(4, 2, 2, 2, 3, 4, z=4.0),        # over the right and the lower border
            plane(-2.5, -2.5, 4, 5, 3, 4, z=16.0),  # behind everything, over the whole image
            plane(-10.25, -7, 3.25, 3.25, 3, 4, z=2.0)]  # ends at (-0.5, -0.5): off by half a pixel
    return _case(maps, [0] * len(maps), [SHAPES[0]])


def random_case(n_boxes, mh, mw, seed):
    """Three frames of different sizes, the middle one without a box.  Smooth maps with noise, over the image and a
    margin around it; a few invalid vertices of every kind, masks and keep flags; cameras off the powers of two."""
    rng = np.random.default_rng(seed)
    shapes = list(SHAPES)
    first = max(1, (3 * n_boxes) // 7)
    box_frame = np.where(np.arange(n_boxes) < first, 0, 2)
    cams = [scene_cases.pow2_camera(4.0, 3.0 + f, 2.0 + f) + rng.uniform(-1.0, 1.0, (3, 4)) * (rng.random((3, 4)) < 0.5) *
            np.asarray([[0.05], [0.05], [0.002]]) for f in range(3)]
    maps = []
    i, j = np.meshgrid(np.arange(mh), np.arange(mw), indexing='ij')
    for b in range(n_boxes):
        f = int(box_frame[b])
        h, w = shapes[f]
        tc, tr = rng.uniform(-0.2, 1.2) * w, rng.uniform(-0.2, 1.2) * h
        sw, sh = rng.uniform(0.3, 1.2) * w, rng.uniform(0.3, 1.2) * h
        cols = tc + (j / (mw - 1.0) - 0.5) * sw + rng.uniform(-0.3, 0.3, (mh, mw))
        rows = tr + (i / (mh - 1.0) - 0.5) * sh + rng.uniform(-0.3, 0.3, (mh, mw))
        z = rng.choice([2.0, 4.0, 8.0]) + rng.uniform(-0.3, 0.3) * j + rng.uniform(-0.3, 0.3) * i + \
            rng.uniform(-0.05, 0.05, (mh, mw))
        z = np.maximum(z, 0.5)
        maps.append(at_pixels(cols, rows, z, 4.0, 3.0 + f, 2.0 + f))
    xyz = np.stack(maps)
    bad = rng.random((n_boxes, mh, mw)) < 0.03
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.asarray([np.nan, np.inf, -np.inf, 0.0, -1.0], np.float32),
                                                              int(bad.sum()))
    mask = (rng.random((n_boxes, mh, mw)) < 0.9).astype(np.float32) * rng.uniform(0.1, 2.0, (n_boxes, mh, mw))
    mask[rng.random((n_boxes, mh, mw)) < 0.03] = -1.0
    keep = (rng.random(n_boxes) < 0.85).astype(np.int32)
    keep[-1], keep[1] = 0, 1
    mask[1] = 1.0
    return _case(list(xyz), box_frame, shapes, cams=cams, mask=mask.astype(np.float32), keep=keep)


def big_case():
    """48 x 48 maps on a frame of 96 x 128 pixels: a wavy surface over most of the image and past its right border, a
    nearer one in front of its middle; a second, small frame with one 48 x 48 box squeezed into 5 x 7 pixels (most
    triangles cover no pixel centre)."""
    i, j = np.meshgrid(np.arange(48), np.arange(48), indexing='ij')
    rng = np.random.default_rng(48)
    wavy = at_pixels(8.3 + 2.7 * j + 0.4 * np.sin(i / 3.0), 4.6 + 1.85 * i + 0.4 * np.cos(j / 4.0),
                     8.0 + 0.5 * np.sin(i / 5.0) * np.cos(j / 7.0) + rng.uniform(-0.01, 0.01, (48, 48)))
    near = at_pixels(40.2 + 0.9 * j, 30.7 + 0.6 * i, 4.0 + 0.02 * j + rng.uniform(-0.01, 0.01, (48, 48)))
    tiny = at_pixels(0.5 + 0.12 * j, 0.25 + 0.09 * i, 2.0 + 0.001 * i)
    mask = (rng.random((3, 48, 48)) < 0.97).astype(np.float32)
    return _case([wavy, near, tiny], [0, 0, 1], [(96, 128), SHAPES[0]], mask=mask)


FEATURE_SHAPE = (100, 104)
FEATURE_ORIGIN = (3, 2)  # column and row of vertex (0, 0); vertices two pixels apart


def feature_case():
    """The point of the feature: ONE box whose 48 x 48 map is a fronto-parallel plane with vertices two pixels apart,
    94 x 94 pixels between its first and its last vertex."""
    return _case([plane(FEATURE_ORIGIN[0], FEATURE_ORIGIN[1], 2, 2, 48, 48, z=8.0)], [0], [FEATURE_SHAPE])


def feature_ground_truth():
    """The instance image is exactly the rectangle the surface covers: the pixel centres in (c0, c1] x (r0, r1] (an
    edge owns its boundary when it runs downwards, or leftwards when level: the lower and the right border of the
    rectangle are in, the upper and the left one out); every pixel has a LiDAR depth of 8.25 m."""
    c0, r0 = FEATURE_ORIGIN
    image = np.full(FEATURE_SHAPE, 255, np.uint8)
    image[r0 + 1:r0 + 95, c0 + 1:c0 + 95] = 7
    return dict(instance_images=[image], depth_maps=[np.full(FEATURE_SHAPE, 8.25, np.float32)],
                box_gt_id=np.asarray([7], np.int64))


_BUILDERS = {
    'cell_2x2': cell_case,
    'fractional_2x3': fractional_2x3_case,
    'on_centres_4x5': on_centres_case,
    'mirrored_4x5': mirrored_case,
    'snap_halfway': snap_halfway_case,
    'invalid_vertices': invalid_case,
    'edge_dz': edge_dz_case,
    'span_limit': span_case,
    'degenerate': degenerate_case,
    'identical_boxes': identical_case,
    'boxes_255': boxes_255_case,
    'off_image': off_image_case,
    'random_b12_5x4': lambda: random_case(12, 5, 4, 1254),
    'random_b3_2x3': lambda: random_case(3, 2, 3, 323),
    'big_48x48': big_case,
    'feature_94': feature_case,
}
NAMES = tuple(_BUILDERS)
DETERMINISM_CASES = ('random_b12_5x4', 'big_48x48')


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    return surface_restatement.render(case(name), cover=True)


def _big_ground_truth():
    """The rendered instance map moved three pixels to the right as the true one (ids 10 + ordinal), LiDAR depths on
    the 1/256 m grid with holes."""
    c, want = case('big_48x48'), expected('big_48x48')
    rng = np.random.default_rng(4848)
    images, depths = [], []
    for inst in want['instance_maps']:
        moved = np.roll(inst, 3, axis=1)
        images.append(np.where(moved == 255, 255, moved + 10).astype(np.uint8))
        depths.append(scene_score_cases._depths(rng, *inst.shape))
    ordinal = np.asarray([0, 1, 0])
    return dict(instance_images=images, depth_maps=depths, box_gt_id=(ordinal + 10).astype(np.int64))


@functools.lru_cache(maxsize=None)
def ground_truth(name):
    """Seeded instance images and LiDAR depth maps (zeros, negative, inf and NaN entries among them) as
    tests/scene_score_cases.py makes them: with eight boxes or more one box has the id -1, one 300, one an id that no
    pixel carries and two boxes of a frame share an id."""
    if name == 'feature_94':
        return feature_ground_truth()
    if name == 'big_48x48':
        return _big_ground_truth()
    return scene_score_cases.seeded_ground_truth(case(name), 7000 + NAMES.index(name), expected(name))


@functools.lru_cache(maxsize=None)
def expected_scores(name):
    return surface_restatement.scores(case(name), ground_truth(name), expected(name))

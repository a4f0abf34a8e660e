"""The catalogue of scene-reconstruction cases shared by tests/test_scene_reconstruction.py (the restatement against its
own per-point loop) and tests/test_scene_reconstruction_gpu.py (the kernels against the restatement).  A case is the dict
tests/scene_restatement.py takes; `expected(name, visible_only)` computes a case's reference once.
"""
import functools

import numpy as np

import scene_restatement

SHAPES = ((5, 7), (8, 8), (6, 13))


def pow2_camera(f, cx, cy, t=0.0):
    return np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, t]], np.float64)


def encoded_image(frame, h, w):
    """value = ((frame * 64 + row) * 64 + col) * 4 + channel: exact in float32, different at every place."""
    r, c, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
    return (((frame * 64 + r) * 64 + c) * 4 + k).astype(np.float32)


def images_for(shapes):
    return [encoded_image(f, h, w) for f, (h, w) in enumerate(shapes)]


def _ulp_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def _at(t_col, t_row, z, f, cx, cy):
    """the float32 point whose pixel coordinates are exactly (t_col, t_row) under pow2_camera(f, cx, cy)"""
    return [np.float32((t_col - cx) * z / f), np.float32((t_row - cy) * z / f), np.float32(z)]


def rounding_case(shape, f, z, cx, cy):
    """Points at k + 0.5 (k even and odd), -0.5, w - 0.5 and h - 0.5 and one ulp on either side of each, on one axis
    at a time.  f and z are powers of two: u0 / u2 is exact, and half to even decides."""
    h, w = shape
    pts = []
    for t in [-0.5, 0.5, 1.5, 2.5, 3.5, w - 1.5, w - 0.5]:
        x0 = np.float32((t - cx) * z / f)
        for x in _ulp_neighbours(x0):
            pts.append([x, np.float32((1.0 - cy) * z / f), np.float32(z)])
    for t in [-0.5, 0.5, 1.5, 2.5, 3.5, h - 1.5, h - 0.5]:
        y0 = np.float32((t - cy) * z / f)
        for y in _ulp_neighbours(y0):
            pts.append([np.float32((2.0 - cx) * z / f), y, np.float32(z)])
    xyz = np.asarray(pts, np.float32)[None]
    return dict(xyz=xyz, box_frame=[0], cam_p=pow2_camera(f, cx, cy)[None], shapes=[shape], images=images_for([shape]))


def dropped_case():
    """Frame 0: a pinhole camera; frame 1: the same with P[2][3] = -5, so that u2 <= 0 for 0 < z <= 5."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    f, cx, cy = 2.0, 0.0, 0.0
    ok = _at(2.0, 1.0, 2.0, f, cx, cy)
    box0 = [ok, _at(3.0, 1.0, 0.0, f, cx, cy), [1.0, 1.0, -1.0], [nan, 1.0, 2.0], [1.0, nan, 2.0], [1.0, 1.0, nan],
            [inf, 1.0, 2.0], [1.0, -inf, 2.0], [1.0, 1.0, inf], [1.0, 1.0, -inf], ok, ok, ok, ok,
            _at(7.0, 1.0, 2.0, f, cx, cy), _at(-1.0, 1.0, 2.0, f, cx, cy), _at(2.0, 5.0, 2.0, f, cx, cy),
            _at(2.0, -1.0, 2.0, f, cx, cy), [1e30, 1.0, 2.0], [3e38, 3e38, 1e-30]]
    n = len(box0)
    mask0 = np.ones(n, np.float32)
    mask0[10], mask0[11], mask0[12] = 0.0, -1.0, nan
    # frame 1: z = 2 and 5 have u2 = -3 and 0 (dropped, z > 0); z = 8 has u2 = 3 (kept when its pixel is inside)
    box1 = [[1.0, 1.0, 2.0], [1.0, 1.0, 5.0], [3.0, 3.0, 8.0]] + [[0.0, 0.0, 8.0]] * (n - 3)
    box2 = [ok] * n  # keep = 0
    xyz = np.asarray([box0, box1, box2], np.float32)
    return dict(xyz=xyz, box_frame=[0, 1, 1], cam_p=np.stack([pow2_camera(f, cx, cy), pow2_camera(f, cx, cy, -5.0)]),
                shapes=[SHAPES[0], SHAPES[1]], mask=np.stack([mask0, np.ones(n, np.float32), np.ones(n, np.float32)]),
                keep=[1, 1, 0], images=images_for([SHAPES[0], SHAPES[1]]))


def zbuffer_case(equal):
    """Three boxes on pixel (row 2, col 3) at depths 8, 4, 2 (or all 4), two boxes on (1, 1), and box 0 hitting
    (4, 6) twice: farther first, then nearer (or twice at one depth)."""
    f, cx, cy = 4.0, 1.0, 0.0
    z = (4.0, 4.0, 4.0) if equal else (8.0, 4.0, 2.0)
    far = (z[0], z[0]) if equal else (16.0, 1.0)
    box0 = [_at(3.0, 2.0, z[0], f, cx, cy), _at(6.0, 4.0, far[0], f, cx, cy), _at(6.0, 4.0, far[1], f, cx, cy),
            _at(1.0, 1.0, z[0], f, cx, cy), _at(0.0, 0.0, 32.0, f, cx, cy)]
    box1 = [_at(5.0, 0.0, 2.0, f, cx, cy), _at(3.0, 2.0, z[1], f, cx, cy), _at(3.2, 2.2, z[1], f, cx, cy),
            _at(2.0, 2.0, 1.0, f, cx, cy), _at(2.0, 3.0, 1.0, f, cx, cy)]
    box2 = [_at(1.0, 1.0, z[2], f, cx, cy), _at(3.0, 2.0, z[2], f, cx, cy), _at(4.0, 4.0, 0.5, f, cx, cy),
            _at(4.0, 3.0, 0.5, f, cx, cy), _at(0.0, 4.0, 0.25, f, cx, cy)]
    shape = SHAPES[0]
    return dict(xyz=np.asarray([box0, box1, box2], np.float32), box_frame=[0, 0, 0],
                cam_p=pow2_camera(f, cx, cy)[None], shapes=[shape], images=images_for([shape]))


def two_box_case():
    case = zbuffer_case(False)
    return dict(case, xyz=case['xyz'][:2], box_frame=[0, 0])


def random_case(n_boxes, n_points, seed, with_images=True, with_mask=True, with_keep=True):
    """1 to 3 frames of different sizes; with 3 frames the middle one has no box.  With 3 boxes or more: the first and
    the last box keep no point (behind the camera / keep = 0) and box 1 keeps every point.  Depths come from a few
    values, so that float32 depths tie."""
    rng = np.random.default_rng(seed)
    nf = 1 if n_boxes == 1 else 3
    shapes = list(SHAPES[:nf])
    if nf == 1:
        box_frame = np.zeros(n_boxes, np.int64)
    else:
        first = max(1, (3 * n_boxes) // 7)
        box_frame = np.where(np.arange(n_boxes) < first, 0, 2)
    # off the powers of two: rows 0 and 1 by up to 0.05, row 2 by up to 0.002 (a pixel moves by less than 0.5)
    cams = np.stack([pow2_camera(4.0, 3.0 + f, 2.0 + f) + rng.uniform(-1.0, 1.0, (3, 4)) * (rng.random((3, 4)) < 0.5) *
                     np.asarray([[0.05], [0.05], [0.002]]) for f in range(nf)])
    h = np.asarray([shapes[f][0] for f in box_frame], np.float64)[:, None]
    w = np.asarray([shapes[f][1] for f in box_frame], np.float64)[:, None]
    z = rng.choice(np.asarray([1.0, 2.0, 2.0, 4.0, 8.0]), (n_boxes, n_points)) * \
        np.where(rng.random((n_boxes, n_points)) < 0.3, rng.uniform(0.5, 1.5, (n_boxes, n_points)), 1.0)
    # pixel targets over the image and a margin of 30 % around it
    tc = rng.uniform(-0.3, 1.3, (n_boxes, n_points)) * w
    tr = rng.uniform(-0.3, 1.3, (n_boxes, n_points)) * h
    cx = np.asarray([3.0 + f for f in box_frame])[:, None]
    cy = np.asarray([2.0 + f for f in box_frame])[:, None]
    xyz = np.stack([(tc - cx) * z / 4.0, (tr - cy) * z / 4.0, z], -1).astype(np.float32)
    bad = rng.random((n_boxes, n_points)) < 0.03
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.asarray([np.nan, np.inf, -np.inf, 0.0, -1.0],
                                                                         np.float32), int(bad.sum()))
    mask = (rng.random((n_boxes, n_points)) < 0.8).astype(np.float32) * rng.uniform(0.1, 2.0, (n_boxes, n_points))
    mask[rng.random((n_boxes, n_points)) < 0.05] = -1.0
    keep = (rng.random(n_boxes) < 0.85).astype(np.int32)
    if n_boxes >= 3:
        xyz[0, :, 2] = -np.abs(xyz[0, :, 2])         # the first box: behind the camera
        keep[-1] = 0                                 # the last box: not kept
        keep[1] = 1                                  # box 1: every point inside, valid and kept
        f1 = int(box_frame[1])
        z1 = rng.choice(np.asarray([1.0, 2.0, 4.0]), n_points)
        c1 = rng.uniform(1.0, shapes[f1][1] - 2.0, n_points)
        r1 = rng.uniform(1.0, shapes[f1][0] - 2.0, n_points)
        xyz[1] = np.stack([(c1 - (3.0 + f1)) * z1 / 4.0, (r1 - (2.0 + f1)) * z1 / 4.0, z1], -1).astype(np.float32)
        mask[1] = 1.0
    case = dict(xyz=xyz, box_frame=box_frame, cam_p=cams, shapes=shapes)
    if with_mask:
        case['mask'] = mask.astype(np.float32)
    if with_keep:
        case['keep'] = keep
    if with_images:
        case['images'] = images_for(shapes)
    return case


def many_boxes_case(n_boxes):
    """n_boxes boxes of one point in ONE frame, box b on pixel b % (h * w), nearer boxes later."""
    h, w = SHAPES[1]
    b = np.arange(n_boxes)
    z = (2.0 ** -(b // (h * w))).astype(np.float64)  # 1, then 0.5 on the second round over the image, ...
    col, row = (b % (h * w)) % w, (b % (h * w)) // w
    xyz = np.stack([col * z / 2.0, row * z / 2.0, z], -1).astype(np.float32)[:, None]
    return dict(xyz=xyz, box_frame=np.zeros(n_boxes, np.int64), cam_p=pow2_camera(2.0, 0.0, 0.0)[None], shapes=[(h, w)])


def distinct_pixels_case():
    """One cloud whose kept points fall on distinct pixels with 0 < z < 100 (the cross-check against
    depth_map_utils.project_depths); every point has z > 0 and is finite."""
    rng = np.random.default_rng(11)
    h, w = SHAPES[2]
    cam = pow2_camera(4.0, 3.0, 2.0) + rng.uniform(-0.02, 0.02, (3, 4))
    cam[2] = [0, 0, 1, 0.001]
    order = rng.permutation(h * w)[:40]
    z = rng.uniform(1.0, 90.0, 40)
    tc, tr = (order % w) + rng.uniform(-0.3, 0.3, 40), (order // w) + rng.uniform(-0.3, 0.3, 40)
    # u = P . [x y z 1]: solve the pinhole part for x, y (the small perturbations move a target by far less than 0.2)
    x, y = (tc - 3.0) * z / 4.0, (tr - 2.0) * z / 4.0
    out = np.stack([rng.uniform(50, 80, 6), rng.uniform(-5, 5, 6), rng.uniform(1.0, 3.0, 6)], -1)  # far off the image
    xyz = np.concatenate([np.stack([x, y, z], -1), out]).astype(np.float32)[None]
    return dict(xyz=xyz, box_frame=[0], cam_p=cam[None], shapes=[(h, w)])


RANDOM_SIZES = ((1, 1), (1, 35), (1, 64), (1, 65), (1, 300), (1, 2304), (3, 65), (3, 300), (3, 2304), (70, 1),
                (70, 35), (70, 64), (70, 300))
DETERMINISM_CASE = 'random_b70_p300'

_BUILDERS = {
    'rounding_5x7': lambda: rounding_case(SHAPES[0], 2.0, 2.0, 0.0, 0.0),
    'rounding_8x8_offset': lambda: rounding_case(SHAPES[1], 4.0, 0.5, 2.0, 1.0),
    'rounding_6x13': lambda: rounding_case(SHAPES[2], 8.0, 4.0, 1.0, 3.0),
    'dropped': dropped_case,
    'zbuffer_three_boxes': lambda: zbuffer_case(False),
    'zbuffer_equal_depth': lambda: zbuffer_case(True),
    'zbuffer_two_boxes': two_box_case,
    'boxes_255': lambda: many_boxes_case(255),
    'no_mask_no_keep': lambda: random_case(3, 35, 5, with_mask=False, with_keep=False),
    'no_images': lambda: random_case(3, 65, 6, with_images=False),
}
for _b, _p in RANDOM_SIZES:
    _BUILDERS['random_b%d_p%d' % (_b, _p)] = functools.partial(random_case, _b, _p, 100 * _b + _p)

NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def expected(name, visible_only=False):
    return scene_restatement.scene(case(name), visible_only)

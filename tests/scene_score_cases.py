"""The cases of tests/scene_cases.py with ground truth (seeded instance images and LiDAR depth maps) for
mpsr_scene_score, shared by tests/test_scene_score.py and tests/test_scene_score_gpu.py.  `case(name)` is the scene case,
`ground_truth(name)` its dict for tests/scene_score_restatement.py, `expected(name)` the restatement's result, computed
once.

Instance images: ids 0..254 in rectangular blobs over a background of 255.  Depth maps: multiples of 1/256 m (the grid
of the PNG format) below 128 m, with zeros ("no depth") and a few inf / NaN entries.  box_gt_id: mostly the id under one
of the box's own points; in the larger cases one box has no ground truth (-1), one has an id above 254 (300: none
either), one an id that no pixel carries and two boxes of one frame share an id.

EXACT cases (bit-for-bit sums): every z is a multiple of 2^-10 below 128 m and every depth a multiple of 2^-8 below
128 m, so e is a multiple of 2^-10 with |e| < 2^7 and e * e a multiple of 2^-20 below 2^14: a sum of at most 2304 such
terms is below 2^26 in units of 2^-20, 46 bits, and fits the 53 bits of fp64 in any order.  The `grid_*` cases are
scene_cases.random_case with z rounded to that grid; `identity` and `scaled` are constructed on pow2_camera, `identity_2304` and
`scaled_2304` likewise with a whole box of 48 x 48 points, so that a sum has 2304 terms from nine slices.  The
`random_*` cases keep their arbitrary float32 z and are compared within scene_score_restatement.sum_bounds.
"""
import functools

import numpy as np

import scene_cases
import scene_restatement
import scene_score_restatement

Z_GRID, DEPTH_GRID, LIMIT = 2.0 ** -10, 2.0 ** -8, 128.0


def _grid_case(n_boxes, n_points, seed):
    case = dict(scene_cases.random_case(n_boxes, n_points, seed))
    xyz = np.array(case['xyz'], np.float32)
    z = xyz[..., 2].astype(np.float64)
    with np.errstate(invalid='ignore'):
        xyz[..., 2] = np.where(np.isfinite(z), np.rint(z / Z_GRID) * Z_GRID, z).astype(np.float32)
    case['xyz'] = xyz
    return case


def _blobs(rng, h, w, ids):
    image = np.full((h, w), 255, np.uint8)
    for v in ids:
        r0, c0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        r1, c1 = int(rng.integers(r0 + 1, min(h, r0 + 5) + 1)), int(rng.integers(c0 + 1, min(w, c0 + 7) + 1))
        image[r0:r1, c0:c1] = v
    return image


def _depths(rng, h, w):
    d = (rng.integers(1, int(12.0 / DEPTH_GRID), (h, w)) * DEPTH_GRID).astype(np.float32)
    d[rng.random((h, w)) < 0.2] = 0.0
    d[rng.random((h, w)) < 0.04] = np.inf
    d[rng.random((h, w)) < 0.04] = np.nan
    d[rng.random((h, w)) < 0.02] = -1.0
    return d


def seeded_ground_truth(case, seed, scene=None):
    """Ground truth for any scene case: blobs of a few ids per frame (0 and 254 among them), box ids mostly from under
    the pixels the box wins (`scene`: the case's rendering, computed when not given)."""
    rng = np.random.default_rng(seed)
    shapes = [(int(s[0]), int(s[1])) for s in case['shapes']]
    nb = np.asarray(case['xyz']).shape[0]
    bf = np.asarray(case['box_frame'], np.int64).reshape(nb)
    images, depths, present = [], [], []
    for h, w in shapes:
        ids = [0, 254] + [int(v) for v in rng.choice(np.arange(1, 254), 5, replace=False)]
        images.append(_blobs(rng, h, w, [ids[k] for k in rng.permutation(len(ids))]))
        depths.append(_depths(rng, h, w))
        present.append(sorted(set(np.unique(images[-1]).tolist()) - {255}))
    if scene is None:
        scene = scene_restatement.scene(case)
    gid = np.zeros(nb, np.int64)
    for b in range(nb):
        f = int(bf[b])
        won = scene['instance_maps'][f] == b - int(np.searchsorted(bf, f))
        under = [int(v) for v in images[f][won] if v != 255]
        if under and rng.random() < 0.8:
            gid[b] = under[int(rng.integers(0, len(under)))]
        else:
            gid[b] = present[f][int(rng.integers(0, len(present[f])))]
    if nb >= 3 and bf[1] == bf[2]:
        gid[2] = gid[1]                                   # two boxes of one frame share an id
    if nb >= 8:
        f = int(bf[5])
        gid[3], gid[4] = -1, 300                          # no ground truth, below and above the range
        gid[5] = min(set(range(1, 254)) - set(present[f]))  # an id that no pixel of the frame carries
        gid[7] = gid[6]
    return dict(instance_images=images, depth_maps=depths, box_gt_id=gid)


# ---- the two constructed cases on pow2_camera

_CAMERA = (4.0, 3.0, 2.0)  # f, cx, cy
_SHAPE = scene_cases.SHAPES[2]
_BLOBS = ((7, 1, 5, 1, 7), (0, 0, 4, 8, 13))  # id, rows [r0, r1), columns [c0, c1): 24 and 20 pixels, apart
# a whole 48 x 48 box on a frame of 50 x 61 pixels (3050 bytes: no multiple of 16), and a box of 400 points next to it
_BIG_SHAPE = (50, 61)
_BIG_BLOBS = ((254, 1, 49, 2, 50), (3, 0, 50, 52, 60))


def _constructed(scale, _SHAPE=_SHAPE, _BLOBS=_BLOBS):
    """Two boxes whose points are the pixel centres of one ground-truth instance each, back-projected at the LiDAR
    depth and moved along their rays by `scale` (a box's points beyond its blob's are dropped: z = -1)."""
    f, cx, cy = _CAMERA
    h, w = _SHAPE
    rng = np.random.default_rng(77)
    depth = (rng.integers(256, 40 * 256, (h, w)) * DEPTH_GRID).astype(np.float32)  # 1 .. 40 m, every pixel measured
    image = np.full((h, w), 255, np.uint8)
    boxes = []
    for v, r0, r1, c0, c1 in _BLOBS:
        image[r0:r1, c0:c1] = v
        rows, cols = np.meshgrid(np.arange(r0, r1), np.arange(c0, c1), indexing='ij')
        d = depth[rows, cols].astype(np.float64).reshape(-1)
        boxes.append(np.stack([(cols.reshape(-1) - cx) * d / f, (rows.reshape(-1) - cy) * d / f, d], -1) * scale)
    npts = max(len(b) for b in boxes)
    xyz = np.full((len(boxes), npts, 3), -1.0, np.float64)
    for b, pts in enumerate(boxes):
        xyz[b, :len(pts)] = pts
    assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)  # exact in float32
    case = dict(xyz=xyz.astype(np.float32), box_frame=[0, 0], cam_p=scene_cases.pow2_camera(f, cx, cy)[None],
                shapes=[_SHAPE])
    gt = dict(instance_images=[image], depth_maps=[depth], box_gt_id=np.asarray([v[0] for v in _BLOBS], np.int64))
    return case, gt


GRID_SIZES = scene_cases.RANDOM_SIZES
RANDOM_NAMES = tuple('random_b%d_p%d' % s for s in scene_cases.RANDOM_SIZES)
OTHER_SCENE_NAMES = ('boxes_255', 'zbuffer_three_boxes', 'zbuffer_equal_depth', 'dropped')

_BUILDERS = {'identity': lambda: _constructed(1.0), 'scaled': lambda: _constructed(1.25),
             'identity_2304': lambda: _constructed(1.0, _BIG_SHAPE, _BIG_BLOBS),
             'scaled_2304': lambda: _constructed(1.25, _BIG_SHAPE, _BIG_BLOBS)}
for _k, (_b, _p) in enumerate(GRID_SIZES):
    def _build(b=_b, p=_p, k=_k):
        c = _grid_case(b, p, 100 * b + p)
        return c, seeded_ground_truth(c, 1000 + k)
    _BUILDERS['grid_b%d_p%d' % (_b, _p)] = _build
for _k, _name in enumerate(OTHER_SCENE_NAMES):
    _BUILDERS[_name] = lambda name=_name, k=_k: (scene_cases.case(name), seeded_ground_truth(
        scene_cases.case(name), 2000 + k, scene_cases.expected(name)))
EXACT_NAMES = tuple(_BUILDERS)
for _k, _name in enumerate(RANDOM_NAMES):
    _BUILDERS[_name] = lambda name=_name, k=_k: (scene_cases.case(name), seeded_ground_truth(
        scene_cases.case(name), 3000 + k, scene_cases.expected(name)))
NAMES = tuple(_BUILDERS)
DETERMINISM_CASE = scene_cases.DETERMINISM_CASE


@functools.lru_cache(maxsize=None)
def _built(name):
    return _BUILDERS[name]()


def case(name):
    return _built(name)[0]


def ground_truth(name):
    return _built(name)[1]


@functools.lru_cache(maxsize=None)
def scene(name):
    """The restatement's rendering of the case (the existing catalogue's own cache where the case is its)."""
    if name in scene_cases.NAMES and case(name) is scene_cases.case(name):
        return scene_cases.expected(name)
    return scene_restatement.scene(case(name))


@functools.lru_cache(maxsize=None)
def expected(name):
    return scene_score_restatement.scores(case(name), ground_truth(name), scene(name))

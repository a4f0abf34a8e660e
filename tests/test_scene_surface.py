"""Instance maps rendered as surfaces without a GPU: the four entry points' declarations and
host-side argument checks, the properties the restatement of tests/surface_restatement.py must have by itself, the metric
table's arithmetic, the command lines' flags, the Evaluator's argument and the CSV writer."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import surface_cases as cases
import surface_restatement as restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('mpsr_scene_surface_workspace_bytes', 'mpsr_scene_surface_render', 'mpsr_scene_surface_resolve',
             'mpsr_scene_surface_score')


def test_new_names_are_declared_bound_and_exported():
    import subprocess
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    lib = _lib.lib()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert re.search(r' T %s\b' % name, exported), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.ABI_VERSION == 13 and lib.mpsr_abi_version() == 13
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^[^\n#]*\bscene\.o\b[^\n]*:[^\n]*\n\t[^\n]*\$\(NOFMA\)', mk, re.M)


def _render(lib, nf, nb, mh, mw, dz=1.0, span=64, ptr=None, host_bf=None, host_hw=None, host_offs=None, ws=(None, 0),
            **null):
    """mpsr_scene_surface_render with `ptr` for every device pointer (never dereferenced: each call fails or returns on
    the host) and the host tables where given."""
    a = dict(xyz=ptr, mask=None, box_frame=ptr, box_frame_host=host_bf, keep=None, cam=ptr, hw=ptr, hw_host=host_hw,
             offs=ptr, offs_host=host_offs)
    a.update(null)
    return lib.mpsr_scene_surface_render(a['xyz'], a['mask'], a['box_frame'], a['box_frame_host'], a['keep'], a['cam'],
                                         a['hw'], a['hw_host'], a['offs'], a['offs_host'], nf, nb, mh, mw, dz, span,
                                         ws[0], ws[1], None)


def test_host_checks_of_the_entry_points_need_no_gpu():
    from monopsr_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(256)
    as_ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    bf = np.ascontiguousarray(np.asarray([0, 1, 1], np.int32))
    hw = np.ascontiguousarray(np.asarray([[5, 7], [8, 8]], np.int32))
    offs = np.ascontiguousarray(np.asarray([0, 35, 99], np.int64))
    tables = dict(ptr=fake, host_bf=as_ptr(bf), host_hw=as_ptr(hw), host_offs=as_ptr(offs))
    wsb = lib.mpsr_scene_surface_workspace_bytes
    # the workspace size: keys, vertices, first boxes, triangle counts and rectangles, each aligned to 256 bytes
    assert wsb(2, 99, 3, 48, 48) == 1024 + 3 * 48 * 48 * 8 + 256 + 256 + 256
    assert wsb(0, 99, 3, 4, 4) == 0 and wsb(2, 0, 3, 4, 4) == 0 and wsb(2, 99, 0, 4, 4) == 0
    assert wsb(2, 99, 3, 1, 4) == 0 and wsb(2, 99, 3, 4, 1) == 0 and wsb(2, 99, 1 << 30, 3, 3) == 0
    # the map: 2 x 2 or more, before anything else (even with empty sizes)
    for mh, mw in ((1, 4), (4, 1), (0, 0), (-3, 4)):
        assert _render(lib, 2, 3, mh, mw, **tables) == 1 and b'map_h and map_w must be 2 or more' in lib.mpsr_last_error()
        assert _render(lib, 0, 0, mh, mw) == 1
    # max_span_px in 1 .. 1024
    for span in (0, 1025, -1):
        assert _render(lib, 2, 3, 4, 4, span=span, **tables) == 1 and b'max_span_px' in lib.mpsr_last_error()
    # max_edge_dz > 0; +inf is allowed (the call goes on to the workspace check)
    for dz in (0.0, -1.0, float('nan'), -float('inf')):
        assert _render(lib, 2, 3, 4, 4, dz=dz, **tables) == 1 and b'max_edge_dz' in lib.mpsr_last_error()
    assert _render(lib, 2, 3, 4, 4, dz=float('inf'), span=1, **tables) == 3 and b'workspace' in lib.mpsr_last_error()
    assert _render(lib, 2, 3, 4, 4, dz=1e-30, span=1024, **tables) == 3
    # the triangle id must fit 32 bits: n_boxes (map_h - 1) (map_w - 1) 2 >= 2^32 is refused, one cell less is not
    assert _render(lib, 1, 1 << 15, 257, 257, **tables) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert _render(lib, 1, 1 << 30, 3, 2) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert _render(lib, 1, (1 << 15) - 1, 257, 257) == 1 and b'null' in lib.mpsr_last_error()  # past that check
    # empty sizes are no-ops; negative ones are not
    assert _render(lib, 0, 3, 4, 4) == 0 and _render(lib, 2, 0, 4, 4) == 0
    assert _render(lib, -1, 3, 4, 4) == 1 and b'negative' in lib.mpsr_last_error()
    # null pointers with non-empty sizes
    for key in ('xyz', 'box_frame', 'box_frame_host', 'cam', 'hw', 'hw_host', 'offs', 'offs_host'):
        assert _render(lib, 2, 3, 4, 4, **dict(tables, **{key: None})) == 1, key
        assert b'null' in lib.mpsr_last_error(), key
    # the frame tables
    bad = np.ascontiguousarray(np.asarray([0, 35, 98], np.int64))
    assert _render(lib, 2, 3, 4, 4, **dict(tables, host_offs=as_ptr(bad))) == 1 and b'spans' in lib.mpsr_last_error()
    for frames, what in (([0, 2, 1], b'of frame 2'), ([1, 0, 1], b'decreases')):
        b = np.ascontiguousarray(np.asarray(frames, np.int32))
        assert _render(lib, 2, 3, 4, 4, **dict(tables, host_bf=as_ptr(b))) == 1 and what in lib.mpsr_last_error()
    # a missing or short workspace: status 3, still before any launch
    need = wsb(2, 99, 3, 4, 4)
    assert _render(lib, 2, 3, 4, 4, **tables) == 3 and b'workspace' in lib.mpsr_last_error()
    assert _render(lib, 2, 3, 4, 4, ws=(fake, need - 1), **tables) == 3 and b'workspace' in lib.mpsr_last_error()

    # resolve: more than 255 boxes in a frame are refused; the workspace
    resolve = lambda nf, tp, nb, mh, mw, b, ws=(None, 0), tri=None: lib.mpsr_scene_surface_resolve(
        fake, as_ptr(b), nf, tp, nb, mh, mw, ws[0], ws[1], fake, fake, tri, None)
    many = np.zeros(256, np.int32)
    assert resolve(1, 64, 256, 2, 2, many) == 1 and b'more than 255 boxes' in lib.mpsr_last_error()
    assert resolve(1, 64, 255, 2, 2, many[:255].copy()) == 3 and b'workspace' in lib.mpsr_last_error()
    assert resolve(1, 64, 255, 1, 2, many) == 1 and b'2 or more' in lib.mpsr_last_error()
    assert resolve(1, 0, 255, 2, 2, many) == 0 and resolve(0, 64, 255, 2, 2, many) == 0
    assert lib.mpsr_scene_surface_resolve(fake, as_ptr(many), 1, 64, 3, 2, 2, fake, 1 << 20, None, fake, None, None) == 1
    assert b'null' in lib.mpsr_last_error()

    # score: the ground truth goes together, the workspace, then the scratch
    def score(nf, tp, nb, mh, mw, ws=(None, 0), scratch=(None, 0), **null):
        a = dict(box_frame=fake, box_frame_host=as_ptr(bf), gt_id=fake, depth=fake, inst=fake, hw=fake, offs=fake,
                 counts=fake, sums=fake)
        a.update(null)
        return lib.mpsr_scene_surface_score(a['box_frame'], a['box_frame_host'], a['gt_id'], a['depth'], a['inst'],
                                            a['hw'], a['offs'], nf, tp, nb, mh, mw, ws[0], ws[1], scratch[0], scratch[1],
                                            a['counts'], a['sums'], None)
    for key in ('box_frame', 'box_frame_host', 'gt_id', 'depth', 'inst', 'hw', 'offs', 'counts', 'sums'):
        assert score(2, 99, 3, 4, 4, **{key: None}) == 1 and b'null' in lib.mpsr_last_error(), key
    assert score(2, 99, 3, 4, 1) == 1 and b'2 or more' in lib.mpsr_last_error()
    assert score(2, 99, 3, 4, 4) == 3 and b'workspace' in lib.mpsr_last_error()
    assert score(2, 99, 3, 4, 4, ws=(fake, need)) == 3 and b'scratch' in lib.mpsr_last_error()
    assert score(2, 99, 3, 4, 4, ws=(fake, need), scratch=(fake, 2 * 1024 - 1)) == 3 and b'scratch' in lib.mpsr_last_error()
    assert score(0, 99, 3, 4, 4) == 0 and score(2, 0, 3, 4, 4) == 0


# ---- properties of the restatement itself


def test_fronto_parallel_grid_covers_every_pixel_of_its_span_once():
    """Vertices on integer pixels spanning [c0, c1] x [r0, r1]: exactly (c1 - c0)(r1 - r0) pixel centres are covered,
    each by ONE triangle, although every shared edge and every cell diagonal runs through pixel centres."""
    for name, (c0, c1, r0, r1) in (('on_centres_4x5', cases.ON_CENTRES_SPAN), ('mirrored_4x5', cases.ON_CENTRES_SPAN),
                                   ('feature_94', (3, 97, 2, 96)), ('cell_2x2', (1, 4, 1, 3))):
        got = cases.expected(name)
        cover = got['cover'][0]
        assert int(cover.sum()) == (c1 - c0) * (r1 - r0) and int(cover.max()) == 1, name
        inside = np.zeros_like(cover)
        inside[r0 + 1:r1 + 1, c0 + 1:c1 + 1] = 1  # the lower and the right border belong to the surface
        assert np.array_equal(cover, inside), name
        assert int(got['tris'][0]) == got['drawn'].shape[1] and got['rect'][0].tolist() == [c0, r0, c1, r1]
        assert np.array_equal(got['instance_maps'][0] == 0, inside == 1) and np.array_equal(got['tri_maps'][0] >= 0, inside == 1)


def test_mirrored_map_gives_the_same_depth_map():
    a, b = cases.expected('on_centres_4x5'), cases.expected('mirrored_4x5')
    assert a['depth_maps'][0].tobytes() == b['depth_maps'][0].tobytes() and bool((a['depth_maps'][0] == 4.0).any())
    assert np.array_equal(a['instance_maps'][0], b['instance_maps'][0])
    assert not np.array_equal(a['tri_maps'][0], b['tri_maps'][0])
    # the facing: every doubled area of the mirrored map is negative before the swap
    _, X, Y = restatement.vertices(cases.case('mirrored_4x5'))
    for i, j, k, (pa, pb, pc) in restatement.triangles_of(4, 5):
        area = (X[0][pb] - X[0][pa]) * (Y[0][pc] - Y[0][pa]) - (Y[0][pb] - Y[0][pa]) * (X[0][pc] - X[0][pa])
        assert area < 0


def test_tilted_plane_renders_its_analytic_depth():
    """Vertices anywhere on the plane z = z0 + a x + b y, seen through pow2_camera(f, 0, 0): 1 / z is affine in the
    pixel, 1 / z = (1 - (a col + b row) / f) / z0, and perspective-correct interpolation reproduces an affine 1 / z
    exactly.  What is left is (i) the snapping: every vertex moves by at most 1/512 pixel in each direction, which
    moves the interpolated 1 / z by at most (|a| + |b|) / (f z0) / 512; (ii) the float32 rounding of the vertices'
    x, y and z: a relative 2^-24 each, which moves a vertex's pixel by at most 3 * 2^-24 of its coordinate (below
    2^7 here) and its 1 / z by 2^-24 of itself; (iii) the float32 rounding of the result, 2^-24 relative, and fp64
    arithmetic, far below.  |dz| <= z^2 |d(1/z)|."""
    f, z0, a, b = 4.0, 6.0, 0.05, -0.03
    rng = np.random.default_rng(79)
    i, j = np.meshgrid(np.arange(7), np.arange(6), indexing='ij')
    cols = 1.0 + 3.1 * j + rng.uniform(-0.4, 0.4, j.shape)
    rows = 0.5 + 2.7 * i + rng.uniform(-0.4, 0.4, i.shape)
    z = z0 / (1.0 - (a * cols + b * rows) / f)
    assert float(z.min()) > 0
    case = dict(xyz=cases.at_pixels(cols, rows, z)[None], box_frame=[0], cam_p=cases.scene_cases.pow2_camera(f, 0, 0)[None],
                shapes=[(20, 22)], max_edge_dz=cases.INF)
    got = restatement.render(case)
    depth = got['depth_maps'][0].astype(np.float64)
    hit = got['instance_maps'][0] == 0
    assert int(hit.sum()) > 200 and int(got['tris'][0]) == 2 * 6 * 5
    rr, cc = np.nonzero(hit)
    inv = (1.0 - (a * cc + b * rr) / f) / z0
    slope = (abs(a) + abs(b)) / (f * z0)
    d_inv = slope * (1.0 / 512.0 + 3.0 * 2.0 ** -24 * 2.0 ** 7) + 2.0 ** -24 * inv
    zmax = float(z.max())
    bound = zmax * zmax * d_inv * (1.0 + zmax * d_inv) + 2.0 ** -24 * zmax
    err = np.abs(depth[rr, cc] - 1.0 / inv)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(err.max()) > 0.0  # (the plane is tilted: the snapping is visible)


def test_only_the_triangles_at_an_invalid_vertex_disappear():
    got = cases.expected('invalid_vertices')
    full = np.ones(8, bool)
    # the centre vertex (1, 1) of a 3 x 3 map is a corner of six of the eight triangles: all but triangle 0 of cell
    # (0, 0) and triangle 1 of cell (1, 1)
    around = np.asarray([True, False, False, False, False, False, False, True])
    for n, kind in enumerate(cases.INVALID_KINDS):
        want = full if kind == 'control' else ~full if kind == 'keep_zero' else around
        assert np.array_equal(got['drawn'][n], want), kind
    valid, X, _ = restatement.vertices(cases.case('invalid_vertices'))
    for n, kind in enumerate(cases.INVALID_KINDS):
        if kind == 'u_below_2_to_20':  # a valid vertex at 2^20 - 1/16 pixels: its triangles fall to the span limit
            assert bool(valid[n].all()) and int(X[n, 1, 1]) == 2 ** 28 - 16
        elif kind not in ('control', 'keep_zero'):
            assert not valid[n, 1, 1] and int(valid[n].sum()) == 8, kind


def test_edge_and_span_limits_are_met_exactly():
    got = cases.expected('edge_dz')
    for n, kind in enumerate(cases.EDGE_DZ_KINDS):
        # vertex (0, 0) is a corner of triangle 0 only, vertex (1, 1) of triangle 1 only
        want = [True, True] if kind.startswith('met') else [False, True] if 'v00' in kind or 'below' in kind else [True, False]
        assert got['drawn'][n].tolist() == want, kind
    got = cases.expected('span_limit')
    for n, kind in enumerate(cases.SPAN_KINDS):
        assert got['drawn'][n].tolist() == [kind[-1]] * 2, kind[0]
    assert restatement.floor_div(-1, 256) == -1 and restatement.ceil_div(-1, 256) == 0
    assert restatement.floor_div(-256, 256) == -1 == restatement.ceil_div(-256, 256)
    assert restatement.ceil_div(1, 256) == 1 and restatement.floor_div(255, 256) == 0


def test_the_catalogue_holds_what_it_is_meant_to_hold():
    shapes = {tuple(np.asarray(cases.case(n)['xyz']).shape[1:3]) for n in cases.NAMES}
    assert shapes >= {(2, 2), (2, 3), (5, 4), (48, 48)}
    frames = {tuple(s) for n in cases.NAMES for s in cases.case(n)['shapes']}
    assert (5, 7) in frames and (96, 128) in frames
    assert len(cases.case('random_b12_5x4')['shapes']) == 3 and 1 not in cases.case('random_b12_5x4')['box_frame']
    got = cases.expected('identical_boxes')
    s = cases.expected_scores('identical_boxes')['counts']
    assert s[0, 1] > 0 and s[1, 1] == 0 and s[1, 0] == s[0, 0] == 8 and not (got['instance_maps'][0] == 1).any()
    got = cases.expected('degenerate')
    assert got['tris'].tolist() == [0, 12, 8] and int(got['cover'][1].max()) >= 2
    assert cases.expected('boxes_255')['tris'].tolist() == [2] * 255
    # (the last round over the image hides the earlier ones: ordinals 206 .. 254, and the background)
    assert np.unique(cases.expected('boxes_255')['instance_maps'][0]).tolist() == list(range(206, 256))
    got = cases.expected('off_image')
    assert got['tris'].tolist() == [12] * 6 and (got['rect'][1] == got['rect'][2]).all() and got['rect'][1, 0] > got['rect'][1, 2]
    assert got['rect'][0].tolist() == [0, 0, 3, 2] and bool((got['instance_maps'][0] != 255).all())
    snap = cases.expected('snap_halfway')
    _, X, Y = restatement.vertices(cases.case('snap_halfway'))
    # half to even: 256 + k + 0.5 -> 256, 258, 258, 260; one ulp below and above go down and up
    assert X[0:12, 0, 0].tolist() == [256, 256, 257, 257, 258, 258, 258, 258, 259, 259, 260, 260]
    assert Y[12:24, 0, 0].tolist() == X[0:12, 0, 0].tolist()
    # a vertex one fixed-point unit off renders other depths; two vertices that snap alike render the same
    assert len({snap['depth_maps'][n].tobytes() for n in (0, 2, 6, 9, 11)}) == 5
    assert snap['depth_maps'][2].tobytes() == snap['depth_maps'][3].tobytes()
    for name in ('random_b12_5x4', 'big_48x48', 'invalid_vertices'):
        gt, c = cases.ground_truth(name), cases.expected_scores(name)['counts']
        assert int(c[:, 2].sum()) > 0 and int(c[:, 4].sum()) > 0 and int((c[:, 4] < c[:, 2]).sum()) > 0, name
        d = np.concatenate([d.reshape(-1) for d in gt['depth_maps']])
        assert bool((d == 0).any() and (d < 0).any() and np.isinf(d).any() and np.isnan(d).any())
    gid = cases.ground_truth('random_b12_5x4')['box_gt_id']
    c = cases.expected_scores('random_b12_5x4')['counts']
    assert gid[3] == -1 and gid[4] == 300 and c[3, 3] == c[4, 3] == c[5, 3] == 0 and 0 <= gid[5] <= 254
    c = cases.expected_scores('feature_94')
    assert c['counts'].tolist() == [[4418, 8836, 8836, 8836, 8836]] and c['sums'].tolist() == [[-2209.0, 2209.0, 552.25]]
    assert restatement.table(c['counts'], c['sums'], [7]).tolist() == [[1.0, 1.0, 1.0, -0.25, 0.25, 0.25]]


def test_score_sums_run_in_slice_tree_and_wave_order():
    """The restated reduction on values whose sum depends on the order: lane 0 of the tree is ((l0 + l32) + (l16 + l48))
    + ..., not the sum from left to right."""
    v = [0.0] * 64
    v[0], v[32], v[16] = 1.0, 2.0 ** -53, 2.0 ** -53
    assert restatement._tree(v) == 1.0 and sum(v) == 1.0
    v[48] = 2.0 ** -53
    assert restatement._tree(v) == 1.0 + 2.0 ** -52  # (l16 + l48) is added as one term
    assert ((1.0 + v[16]) + v[32]) + v[48] == 1.0


# ---- the Python layer


def test_table_arithmetic_and_nan_rules():
    import torch
    from monopsr_amd.core import scene_reconstruction as sr
    assert sr.SURFACE_METRIC_NAMES == restatement.METRIC_NAMES and sr.SURFACE_COUNT_NAMES == restatement.COUNT_NAMES
    assert sr.SURFACE_METRIC_NAMES == ('surface_mask_iou', 'surface_mask_precision', 'surface_mask_recall',
                                       'surface_depth_bias', 'surface_depth_mae', 'surface_depth_rmse')
    assert sr.SURFACE_SUM_NAMES == ('sum_e', 'sum_abs_e', 'sum_e2')
    #          tris pred inter gt depth_n
    counts = [[10, 8, 4, 12, 3],       # everything defined: IoU 4 / 16, recall 4 / 12
              [10, 8, 0, 0, 0],        # no ground truth (-1): IoU and recall NaN although pred > 0
              [0, 0, 0, 5, 0],         # nothing drawn: IoU 0 / 5 = 0, recall 0, precision NaN
              [7, 0, 0, 0, 0],         # an id no pixel has, nothing won: union 0 -> NaN everywhere
              [3, 3, 3, 3, 0],         # a perfect mask without a measured depth
              [4418, 1, 1, 100000, 1],
              [9, 9, 9, 9, 9]]         # id 300: no ground truth (gt_px is 0 from the kernel; 9 here: recall 1)
    sums = [[0.75, 1.5, 3.0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [-0.1, 0.1, 0.1 * 0.1], [9.0, 9.0, 9.0]]
    gid = [0, -1, 254, 17, 3, 9, 300]
    got = sr.surface_score_table(torch.tensor(counts, dtype=torch.int32), torch.tensor(sums, dtype=torch.float64),
                                 torch.tensor(gid, dtype=torch.int32))
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 6)
    got = got.numpy()
    nan = np.nan
    want = np.asarray([[4 / 16, 4 / 8, 4 / 12, 0.25, 0.5, 1.0],
                       [nan, 0.0, nan, nan, nan, nan],
                       [0.0, nan, 0.0, nan, nan, nan],
                       [nan, nan, nan, nan, nan, nan],
                       [1.0, 1.0, 1.0, nan, nan, nan],
                       [1 / 100000, 1.0, 1 / 100000, -0.1, 0.1, np.sqrt(0.1 * 0.1)],
                       [nan, 1.0, 1.0, 1.0, 1.0, 1.0]], np.float64).astype(np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))
    assert np.array_equal(np.nan_to_num(restatement.table(counts, sums, gid)), np.nan_to_num(want))
    scores = sr.SurfaceScores(torch.tensor(counts, dtype=torch.int32), torch.tensor(sums, dtype=torch.float64),
                              torch.tensor(gid, dtype=torch.int32))
    assert np.array_equal(np.nan_to_num(scores.table().numpy()), np.nan_to_num(want))


def test_public_names_and_what_stays_as_it_was():
    from monopsr_amd.core import evaluator
    from monopsr_amd.core import scene_reconstruction as sr
    assert sr.SURFACE_DIRS == ('depth_surface', 'instances_surface') and sr.SCENE_DIRS == ('points', 'depth', 'instances')
    sig = inspect.signature(sr.render_instance_surfaces)
    assert list(sig.parameters) == ['xyz_global_maps', 'box_frame', 'cam_p', 'frame_shapes', 'valid_mask', 'keep',
                                    'max_edge_dz', 'max_span_px', 'ground_truth', 'want_tri', 'device']
    assert sig.parameters['max_edge_dz'].default == 1.0 and sig.parameters['max_span_px'].default == 64
    assert sig.parameters['want_tri'].default is False and sig.parameters['ground_truth'].default is None
    sig = inspect.signature(sr.reconstruct_frames)
    assert list(sig.parameters)[-1] == 'surfaces' and sig.parameters['surfaces'].default is None
    assert list(sig.parameters)[:-1] == ['model', 'samples', 'outs', 'min_score', 'visible_only', 'ground_truth']
    assert 'surfaces' in sr.SceneResult.__slots__
    assert set(sr.SurfaceResult.__slots__) == {'depth_maps', 'instance_maps', 'tri_maps', 'tris_per_box',
                                               'pixels_per_box', 'scores'}
    sig = inspect.signature(evaluator.Evaluator.__init__)
    assert sig.parameters['scene_metrics'].default is False and list(sig.parameters)[-1] == 'chunk_hook'


def test_surface_files(tmp_path):
    from monopsr_amd.core import scene_reconstruction as sr
    from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils
    dirs = sr.surface_output_dirs(str(tmp_path))
    assert sorted(os.listdir(str(tmp_path))) == sorted(sr.SURFACE_DIRS) and sorted(dirs) == sorted(sr.SURFACE_DIRS)
    paths = sr.save_empty_surface_frame(dirs, '000007', (5, 7, 3))
    assert paths == (os.path.join(dirs['depth_surface'], '000007.png'), os.path.join(dirs['instances_surface'], '000007.png'))
    assert depth_map_utils.read_depth_map(paths[0]).shape == (5, 7) and not depth_map_utils.read_depth_map(paths[0]).any()
    assert bool((instance_utils.read_instance_image(paths[1]) == 255).all())


def test_run_inference_accepts_surfaces():
    from monopsr_amd.experiments import run_inference
    need = ['cfg.yaml', 'ckpt', '--mscnn-dir', 'm', '--output-dir', 'o']
    ap = run_inference.build_parser()
    plain = ap.parse_args(need)
    assert plain.surfaces is False and plain.max_edge_dz == 1.0 and plain.max_span_px == 64
    # the old defaults
    assert (plain.data_split, plain.width_div, plain.no_scenes, plain.min_score, plain.visible_only) == \
        ('val', 1, False, None, False)
    args = ap.parse_args(need + ['--surfaces', '--max-edge-dz', '0.5', '--max-span-px', '128'])
    assert args.surfaces is True and args.max_edge_dz == 0.5 and args.max_span_px == 128
    sig = inspect.signature(run_inference.SceneWriter.__init__)
    assert list(sig.parameters) == ['self', 'model', 'base', 'min_score', 'visible_only', 'surfaces']
    assert sig.parameters['surfaces'].default is None


def test_run_evaluation_accepts_surface_metrics():
    from monopsr_amd.experiments import run_evaluation
    need = ['cfg.yaml', '--checkpoint-dir', 'c', '--mscnn-dir', 'm', '--predictions-dir', 'p']
    ap = run_evaluation.build_parser()
    plain = ap.parse_args(need)
    assert plain.surface_metrics is False and plain.scene_metrics is False
    assert (plain.data_split, plain.ckpt_indices, plain.repeat, plain.wait_interval, plain.max_idle, plain.width_div,
            plain.low_iou) == ('val', None, False, 30.0, None, 1, False)
    args = ap.parse_args(need + ['--surface-metrics'])
    assert args.surface_metrics is True and args.scene_metrics is False
    assert ap.parse_args(need + ['--scene-metrics']).surface_metrics is False
    stats = lambda names: {n: dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1) for n in names}
    scene_names = ('scene_mask_iou', 'scene_depth_rmse')
    text = run_evaluation.format_result(dict(report='R\n', scene_stats=stats(scene_names),
                                             surface_stats=stats(restatement.METRIC_NAMES)))
    lines = text.splitlines()
    assert lines[0] == 'R' and [l.split()[0] for l in lines[1:]] == list(scene_names + restatement.METRIC_NAMES)


def test_surface_stats_csv(tmp_path):
    from monopsr_amd.core import evaluator_utils
    names = restatement.METRIC_NAMES
    stats = {n: dict(count=k, mean=k + 0.5, std=0.125 * k, mean_abs=1.0, std_abs=0.0, dropped=0)
             for k, n in enumerate(names)}
    path = evaluator_utils.save_surface_stats(str(tmp_path), 'val', 40, names, stats)
    assert path == os.path.join(str(tmp_path), 'metrics', 'val', 'surface_metrics_val.csv')
    assert evaluator_utils.save_surface_stats(str(tmp_path), 'val', 80, names, stats) == path
    rows = [[c.strip() for c in line.split(',')] for line in open(path).read().splitlines()]
    assert len(rows) == 3 and all(len(r) == 1 + 3 * len(names) for r in rows)
    assert rows[0][:4] == ['step', 'mask_iou_count', 'mask_iou_mean', 'mask_iou_std'] and rows[0][-1] == 'depth_rmse_std'
    assert rows[0][7:10] == ['mask_recall_count', 'mask_recall_mean', 'mask_recall_std']
    assert rows[1][0] == '40' and rows[2][0] == '80' and rows[1][1:] == rows[2][1:]
    assert rows[1][4:7] == ['1', '1.50000', '0.12500']
    # the same layout as the scene metrics' file: fields of 8 and 22 characters
    line = open(path).read().splitlines()[1]
    assert [len(c) for c in line.split(',')] == [8] + [22] * 18

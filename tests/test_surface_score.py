"""mpsr_surface_scores without a GPU: the restatement against itself and against hand-worked numbers, the catalogue's
properties, the entry point's argument checks and the Python surface (the device: tests/test_surface_score_gpu.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import shape_score_restatement as point_restatement
import surface_score_cases as cases
import surface_score_restatement as restatement
from monopsr_amd.core import evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', cases.NAMES)
def test_the_two_restatements_agree(name):
    """The plain loop over queries and triangles against the vectorised version, bit for bit: on every point of the
    small grids, on every STEP-th point (cases.loop_queries) of the larger ones."""
    c, want = cases.case(name), cases.restated(name)
    queries = cases.loop_queries(name)
    got = restatement.surface_scores(c['a'], c['b'], c['mask_a'], c['mask_b'], c['thresholds'], c['max_edge'],
                                     loop=True, queries=queries)
    assert restatement.same_bits(got['tri_counts'], want['tri_counts']), name
    for key in ('point_a', 'point_b'):
        assert restatement.same_bits(got[key], want[key]), (name, key)
    if queries is None:
        for key in ('counts', 'sums', 'table', 'dist_a', 'dist_b'):
            assert restatement.same_bits(got[key], want[key]), (name, key)
    else:
        for key in ('dist_a', 'dist_b'):
            assert restatement.same_bits(got[key][:, queries], want[key][:, queries]), (name, key)
            assert np.isfinite(got[key][:, queries]).sum() >= 10, (name, key)


def test_hand_worked_grids():
    """b is the unit cell v00 = (0,0,0), v01 = (0,1,0), v10 = (1,0,0), v11 = (1,1,0): triangles (v00, v01, v10) and
    (v11, v10, v01), the longest squared edge 2 (the diagonal).  a's four points:
        (0.25, 0.25, 0.5)  inside the first triangle: the face term 0.5^2 = 0.25; the nearest point v00 is at
                           0.0625 + 0.0625 + 0.25 = 0.375
        (0, 0, 2)          exactly above v00: t = 0 on both edges from v00 and v = u = 0 on the face: no term; d is
                           the point's 4
        (0.5, 0.5, 1)      above the middle of the shared diagonal: the edge term 1 (v + u = den: no face term); the
                           nearest points are at 0.25 + 0.25 + 1 = 1.5
        (-1, 0.5, 0)       beyond the boundary edge v00 - v01: its edge term 1, the nearest points at 1.25
    a's own triangles have squared edges 2.375 and 3.25.  With max_edge 1.5 (2.25) b keeps both triangles and a none:
    d_a = 0.25, 4, 1, 1 and d_b = the point distances 0.375, 0.875, 0.875, 1.375.
    sum sqrt d_a = 0.5 + 2 + 1 + 1 = 4.5, sum d_a = 6.25, sum d_b = 3.5, the maxima 4 and 1.375.
    accuracy = 4.5 / 4 = 1.125, chamfer_sq = 6.25 / 4 + 3.5 / 4 = 2.4375, hausdorff = 2.
    At 1: d_a <= 1 three times (two on the boundary), d_b <= 1 three times: precision = recall = fscore = 0.75.
    At 2: everything.  With max_edge 0 no triangle is kept and d_a = the point distances 0.375, 4, 1.5, 1.25."""
    f = np.float32
    b = f([[[[0, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0]]]])
    a = f([[[[0.25, 0.25, 0.5], [0, 0, 2]], [[0.5, 0.5, 1], [-1, 0.5, 0]]]])
    for loop in (False, True):
        r = restatement.surface_scores(a, b, None, None, (1.0, 2.0), 1.5, loop=loop)
        assert r['tri_counts'].tolist() == [[0, 2]]
        assert r['dist_a'].tolist() == [[0.25, 4.0, 1.0, 1.0]] and r['dist_b'].tolist() == [[0.375, 0.875, 0.875, 1.375]]
        assert r['point_a'].tolist() == [[0.375, 4.0, 1.5, 1.25]]
        assert r['counts'].tolist() == [[4, 4, 3, 4, 3, 4]]
        s = r['sums'][0]
        assert [s[0], s[1], s[3], s[4], s[5]] == [4.5, 6.25, 3.5, 4.0, 1.375]
        root_b = np.sqrt([0.375, 0.875, 0.875, 1.375]).sum()
        assert abs(s[2] - root_b) < 1e-15
        t = r['table'][0]
        assert t[0] == 1.125 and t[1] == f(s[2] / 4) and t[3] == 2.4375 and t[4] == 2.0
        assert t[5:].tolist() == [0.75, 0.75, 0.75, 1.0, 1.0, 1.0]
        r = restatement.surface_scores(a, b, None, None, (1.0, 2.0), 0.0, loop=loop)
        assert r['tri_counts'].tolist() == [[0, 0]] and r['dist_a'].tolist() == [[0.375, 4.0, 1.5, 1.25]]
        # an empty side: NaN rows, the counts of valid points and of kept triangles still reported
        r = restatement.surface_scores(a, b, f([[0, 0, 0, 0]]), None, (1.0,), 1.5, loop=loop)
        assert r['counts'].tolist() == [[0, 4, 0, 0]] and r['tri_counts'].tolist() == [[0, 2]]
        assert np.isnan(r['sums']).all() and np.isnan(r['table']).all() and r['table'].shape == (1, 8)
        assert np.isnan(r['dist_a']).all() and np.isnan(r['dist_b']).all()


def _point_scores(name):
    c = cases.case(name)
    n, h, w = c['a'].shape[:3]
    return point_restatement.shape_scores(c['a'].reshape(n, h * w, 3), c['b'].reshape(n, h * w, 3), c['mask_a'],
                                          c['mask_b'], c['thresholds'])


def test_the_catalogue_holds_what_it_is_meant_to_hold():
    shapes = {cases.case(n)['a'].shape[1:3] for n in cases.NAMES}
    assert {(1, 1), (1, 5), (2, 2), (2, 3), (3, 2), (5, 7), (17, 16), (48, 48)} <= shapes
    assert {1, 3, 33} <= {cases.case(n)['a'].shape[0] for n in cases.NAMES}
    assert {0, 1, 3, 8} <= {len(cases.case(n)['thresholds']) for n in cases.NAMES}
    assert {0.0, 0.5, float('inf')} <= {cases.case(n)['max_edge'] for n in cases.NAMES}
    unit = 2.0 ** -16
    # d <= (double) d_point everywhere, NaN in the same places
    for name in cases.NAMES:
        r = cases.restated(name)
        for side in 'ab':
            d, p = r['dist_' + side], r['point_' + side].astype(np.float64)
            live = ~np.isnan(d)
            assert np.array_equal(np.isnan(p) | np.isnan(r['sums'][:, :1]), ~live), name
            assert (d[live] <= p[live]).all() and (d[live] >= 0).all(), name
    # the dyadic plane: every d_a = 9 2^-16 where the point is at 41 2^-16; side a's sums exact; side b dyadic
    c, r = cases.case('dyadic_plane'), cases.restated('dyadic_plane')
    ok = c['mask_a'] > 0
    assert ok.sum() == 3 * 16 * 15 and (r['dist_a'][ok] == 9 * unit).all() and (r['point_a'][ok] == 41 * unit).all()
    assert (r['sums'][:, 0] == 240 * 3 * 2.0 ** -8).all() and (r['sums'][:, 1] == 240 * 9 * unit).all()
    assert set(np.unique(r['dist_b'] / unit)) == {9.0, 25.0, 41.0, 153.0, 169.0, 297.0}
    assert r['counts'][0].tolist() == [240, 272, 0, 240, 240] + r['counts'][0, 5:].tolist()
    assert r['tri_counts'].tolist() == [[2 * 15 * 14, 480]] * 3
    assert (r['table'][:, 5] == 0).all() and (r['table'][:, 8] == 1).all()  # precision below and on the height
    # queries above a vertex, an interior edge, a boundary edge: the height squared; beyond the boundary: the edge term
    r = cases.restated('above_and_beyond')
    d = r['dist_a'].reshape(5, 7) / unit
    assert (d[:4] == 9).all() and (d[4, :6] == 9 + 64).all() and d[4, 6] == 9 + 64 + 16  # (the last: past the corner)
    assert (r['point_a'].reshape(5, 7)[0] == 9 * unit).all() and (r['point_a'].reshape(5, 7)[1:] > 9 * unit).all()
    r = cases.restated('quad')
    assert (r['dist_a'][:2] / unit == [9, 9, 9, 9 + 64]).all() and (r['dist_a'][2, :3] / unit == 9).all()
    assert np.isnan(r['dist_a'][2, 3]) and r['tri_counts'].tolist() == [[2, 2], [2, 2], [1, 2]]
    # max_edge 0: the point distances, bit for bit, and no triangle; +inf: every triangle of valid points
    r, p = cases.restated('max_edge_zero'), _point_scores('max_edge_zero')
    assert (r['tri_counts'] == 0).all() and restatement.same_bits(r['counts'], p['counts'])
    for side in 'ab':
        assert restatement.same_bits(r['dist_' + side], p['dist_' + side].astype(np.float64))
    c, r = cases.case('max_edge_inf'), cases.restated('max_edge_inf')
    assert (r['tri_counts'][:, 0] == 48).all() and (r['tri_counts'][:, 1] > 20).all()
    finite = cases.restated('max_edge_inf')['tri_counts'][:, 1]
    half = restatement.surface_scores(c['a'], c['b'], c['mask_a'], c['mask_b'], (), 0.5)['tri_counts'][:, 1]
    assert (half < finite).all()  # the triangles across the jump
    # the limit itself is kept, one ulp over is not: of b's four triangles the one with the longer edge is dropped
    # (a is b with noise: its edges of about 0.5 fall on either side)
    assert cases.restated('edge_on_the_limit')['tri_counts'][0, 1] == 3
    # the orphan: valid, in no kept triangle, and a nearest point of a's queries
    c, r = cases.case('holes'), cases.restated('holes')
    tri = restatement.kept_triangles(c['b'][0].reshape(-1, 3), c['mask_b'][0] > 0, 17, 16, 0.5)
    orphan = 8 * 16 + 8
    assert c['mask_b'][0, orphan] == 1 and orphan not in tri and 0 < len(tri) < 480
    assert not np.isnan(r['dist_b'][0, orphan])
    # points and no triangle: not an empty side
    r = cases.restated('no_triangle')
    assert (r['tri_counts'][:, 1] == 0).all() and (r['tri_counts'][:, 0] == 48).all()
    assert (r['counts'][:, 1] == 18).all() and not np.isnan(r['table']).any()
    assert (r['dist_b'][~np.isnan(r['dist_b'])] < r['point_b'][~np.isnan(r['dist_b'])]).any()
    # the clone: zeros and ones
    r = cases.restated('clone')
    ok = ~np.isnan(r['dist_a'])
    assert (r['dist_a'][ok] == 0).all() and 0 < ok.sum() < ok.size and (r['sums'] == 0).all()
    assert (r['table'][:, :5] == 0).all() and (r['table'][:, 5:] == 1).all() and (r['tri_counts'] > 0).all()
    # degenerate triangles are kept and give finite numbers
    r = cases.restated('degenerate')
    assert (r['tri_counts'] == 4).all() and np.isfinite(r['sums']).all()
    # overflow: the float32 point distance is +inf, the surface distance finite
    r = cases.restated('overflow')
    assert np.isinf(r['point_a'][0, 1]) and np.isfinite(r['dist_a'][0, 1]) and r['dist_a'][0, 1] > 1e20
    assert r['tri_counts'].tolist() == [[4, 4]]
    # the empty sides
    r = cases.restated('empty_sides')
    assert r['counts'][:, :2].tolist() == [[0, 6], [6, 0], [1, 1], [0, 0]] and np.isnan(r['table'][[0, 1, 3]]).all()
    assert not np.isnan(r['table'][2]).any() and (r['counts'][[0, 1, 3], 2:] == 0).all()
    assert r['tri_counts'].tolist() == [[0, 4], [4, 0], [0, 0], [0, 0]]
    # hostile values on both sides, some under the mask
    c = cases.case('hostile')
    for grid, mask in ((c['a'], c['mask_a']), (c['b'], c['mask_b'])):
        bad = ~np.isfinite(grid.reshape(3, 35, 3)).all(-1)
        assert np.isnan(grid).any() and np.isinf(grid).any() and np.isnan(mask).any() and (bad & (mask > 0)).any()
    # the half-cylinder: one surface sampled twice.  To the nearest point the accuracy is half a grid spacing and
    # nothing is within 5 cm; to the surface it is the chord error and everything but the rim is
    r, p = cases.restated('half_cylinder'), _point_scores('half_cylinder')
    print('half-cylinder: point accuracy %.4f precision@0.05 %.3f; surface accuracy %.4f precision@0.05 %.3f' % (
        p['table'][0, 0], p['table'][0, 5], r['table'][0, 0], r['table'][0, 5]))
    assert p['table'][0, 0] > 0.04 and p['table'][0, 5] < 0.05
    assert r['table'][0, 0] < 0.004 and r['table'][0, 5] > 0.97 and r['tri_counts'].tolist() == [[4418, 4418]]


# ---- the library and the Python surface, on the host


def test_symbols_are_declared_and_bound():
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    assert re.search(r'\bint mpsr_surface_scores\s*\(', header)
    assert re.search(r'\bsize_t mpsr_surface_scores_workspace_bytes\s*\(', header)
    for name in ('mpsr_surface_scores', 'mpsr_surface_scores_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 13 and _lib.lib().mpsr_abi_version() == 13
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bsurface_score\.hip', mk, re.M)
    assert re.search(r'^[^\n]*\bsurface_score\.o[^\n]*:[^\n]*\n\t\$\(HIPCC\) \$\(FLAGS\) \$\(NOFMA\)', mk, re.M)
    src = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'surface_score.hip')).read()
    assert '#pragma clang fp contract(off)' in src and not re.search(r'\batomic\w*\s*\(', src)
    # what it shares with mpsr_shape_scores lives in the core header, under the same rule
    assert '#include "shape_score_core.h"' in src
    assert re.search(r'^[^\n]*\bsurface_score\.o[^\n]*:[^\n]*\bshape_score_core\.h\b', mk, re.M)
    core = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'shape_score_core.h')).read()
    assert '#pragma clang fp contract(off)' in core and not re.search(r'\batomic\w*\s*\(', core)
    assert '#include "common.h"' in src and not re.search(r'^\s*extern\s+(?!"C")', src, re.M)


def test_workspace_bytes():
    from monopsr_amd import _lib
    f = _lib.lib().mpsr_surface_scores_workspace_bytes
    # per (box, direction, slab of 512 queries): three doubles and 2 + T counts; the total rounded up to 8 bytes
    assert f(32, 48, 48, 3) == 32 * 2 * 5 * (24 + 4 * 5)
    assert f(1, 1, 1, 0) == 2 * (24 + 8) and f(2, 1, 5, 8) == 2 * 2 * (24 + 40)
    assert f(5, 17, 31, 1) == 5 * 2 * 2 * (24 + 12) and f(1, 2, 2, 1) == 2 * (24 + 12)
    assert f(0, 4, 4, 3) == 0 and f(-1, 4, 4, 3) == 0 and f(3, 4, 4, 9) == 0 and f(3, 0, 4, 1) == 0
    assert f(1 << 20, 2048, 1, 0) == 0 and f(1, 1 << 15, 1 << 15, 0) > 0 and f(1, 1 << 16, 1 << 15, 0) == 0


def _refused(f, *args):
    from monopsr_amd import _lib
    assert f(*args) == 1, args
    msg = _lib.lib().mpsr_last_error()
    assert msg, args
    return msg


def test_argument_errors_need_no_gpu():
    """Status 1 (3 for the workspace) with a message before anything touches the device: the pointers below are
    never dereferenced."""
    from monopsr_amd import _lib
    f = _lib.lib().mpsr_surface_scores
    fake = 4096
    dbl = lambda *v: (ctypes.c_double * max(len(v), 1))(*v)
    #     a     A     b     B     n  h  w  t               T  e    W     S        c     s     o     d     f     r
    ok = (fake, fake, fake, fake, 3, 5, 7, dbl(0.1, 0.2), 2, 0.5, fake, 1 << 20, fake, fake, fake, fake, fake, fake,
          None)
    call = lambda **kw: [kw.get(k, v) for k, v in zip('aAbBnhwtTeWScsodfr_', ok)]
    assert b'negative' in _refused(f, *call(n=-1))
    for k in 'hw':
        for bad in (0, -1):
            assert b'has no point' in _refused(f, *call(**{k: bad}))
    for k in 'ab':
        assert b'grid pointer is null' in _refused(f, *call(**{k: None}))
    for k in 'csor':
        assert b'output pointer is null' in _refused(f, *call(**{k: None}))
    assert b'workspace is null' in _refused(f, *call(W=None))
    assert b'aligned' in _refused(f, *call(W=fake + 4))
    for T in (-1, 9):
        assert b'outside 0..8' in _refused(f, *call(T=T, t=dbl(*range(1, 10))))
    assert b'thresholds is null' in _refused(f, *call(t=None))
    for bad in (float('nan'), float('inf'), 0.0, -1.0):
        assert b'not a finite distance > 0' in _refused(f, *call(t=dbl(bad, 1.0)))
    assert b'not increasing' in _refused(f, *call(t=dbl(0.2, 0.2)))
    for bad in (float('nan'), -1.0, -0.001, float('-inf')):
        assert b'not a length >= 0' in _refused(f, *call(e=bad))
    assert b'31 bits' in _refused(f, *call(n=1 << 20, h=2048))
    assert b'31 bits' in _refused(f, *call(n=1, h=1 << 16, w=1 << 15))
    assert b'not a length' in _refused(f, *call(n=0, e=-1.0))  # checked whatever n is
    need = _lib.lib().mpsr_surface_scores_workspace_bytes(3, 5, 7, 2)
    assert f(*call(S=need - 1)) == 3 and b'workspace' in _lib.lib().mpsr_last_error()
    # n == 0: a no-op, whatever the pointers
    assert f(None, None, None, None, 0, 5, 7, None, 0, float('inf'), None, 0, None, None, None, None, None, None,
             None) == 0


def test_wrapper_refusals_and_names():
    from monopsr_amd import _lib
    from monopsr_amd.core import distance_metrics as dm
    z = torch.zeros
    with pytest.raises(_lib.InvalidArgumentError, match='GPU'):
        dm.surface_scores(z((2, 3, 4, 3)), z((2, 3, 4, 3)))
    for a, b in ((z((2, 12, 3)), z((2, 12, 3))), (z((2, 3, 4, 2)), z((2, 3, 4, 2))),
                 (z((2, 3, 4, 3), dtype=torch.float64), z((2, 3, 4, 3))),
                 (np.zeros((2, 3, 4, 3), np.float32), z((2, 3, 4, 3)))):
        with pytest.raises(_lib.InvalidArgumentError, match='float32'):
            dm.surface_scores(a, b)
    assert dm.DEFAULT_SHAPE_MAX_EDGE == 0.5 and dm.DEFAULT_SHAPE_THRESHOLDS == (0.05, 0.1, 0.2)
    assert dm.check_max_edge(0) == 0.0 and dm.check_max_edge(float('inf')) == float('inf')
    for bad in (-1, float('nan'), -0.5):
        with pytest.raises(ValueError, match='max_edge'):
            dm.check_max_edge(bad)
    assert dm.SurfaceScores._fields == ('counts', 'sums', 'table', 'dist_a', 'dist_b', 'tri_counts', 'names')
    names = list(inspect.signature(dm.surface_scores).parameters)
    assert names == ['points_a', 'points_b', 'mask_a', 'mask_b', 'thresholds', 'max_edge', 'want_dists']
    names = list(inspect.signature(dm.chunk_surface_scores).parameters)
    assert names == ['model', 'samples', 'outs', 'thresholds', 'max_edge', 'placed']
    assert 'DEFAULT_SHAPE_MAX_EDGE' in dm.__doc__ and 'assumption' in dm.__doc__


class _Dataset(object):
    merges_mscnn, is_test = True, False

    def __init__(self, mode):
        self.train_val_test = mode


def test_evaluator_option_validation_and_signature():
    with pytest.raises(ValueError, match="'val'-mode"):
        evaluator.Evaluator(None, _Dataset('test'), shape_surface_metrics={})
    with pytest.raises(ValueError, match="unknown options \\['edge'\\]"):
        evaluator.Evaluator(None, _Dataset('val'), shape_surface_metrics=dict(edge=1))
    with pytest.raises(ValueError, match='not increasing'):
        evaluator.Evaluator(None, _Dataset('val'), shape_surface_metrics=dict(thresholds=(2, 1)))
    with pytest.raises(ValueError, match='max_edge'):
        evaluator.Evaluator(None, _Dataset('val'), shape_surface_metrics=dict(max_edge=-1))
    ev = evaluator.Evaluator(None, _Dataset('val'), shape_surface_metrics={})
    assert ev.shape_surface_metrics == dict(thresholds=(0.05, 0.1, 0.2), max_edge=0.5, placed=False)
    assert ev.shape_surface_table is None and ev.placed_surface_table is None and ev.shape_metrics is None
    ev = evaluator.Evaluator(None, _Dataset('val'), shape_surface_metrics=dict(thresholds=[1], placed=1,
                                                                               max_edge=float('inf')), shape_metrics={})
    assert ev.shape_surface_metrics == dict(thresholds=(1.0,), max_edge=float('inf'), placed=True)
    # independent of shape_metrics, whose normalised dict keeps its two keys
    assert ev.shape_metrics == dict(thresholds=(0.05, 0.1, 0.2), placed=False)
    assert evaluator.Evaluator(None, _Dataset('val')).shape_surface_metrics is None
    names = list(inspect.signature(evaluator.Evaluator.__init__).parameters)
    assert names[-5:] == ['ap_slices', 'shape_surface_metrics', 'shape_metrics', 'centroid_fit', 'chunk_hook']
    assert inspect.signature(evaluator.Evaluator.__init__).parameters['shape_surface_metrics'].default is None


def test_command_line_options():
    from monopsr_amd.experiments import run_evaluation
    ap = run_evaluation.build_parser()
    base = ['cfg.yaml', '--checkpoint-dir', 'c', '--mscnn-dir', 'm', '--predictions-dir', 'p']
    opts = lambda extra: evaluator.shape_surface_options(ap, ap.parse_args(base + extra))
    assert opts([]) is None and opts(['--shape-metrics']) is None
    assert opts(['--shape-surface-metrics']) == dict(placed=False)
    assert evaluator.shape_metrics_options(ap, ap.parse_args(base + ['--shape-surface-metrics'])) is None
    assert opts(['--shape-surface-metrics', '--shape-surface-thresholds', '0.1', '0.3', '--shape-max-edge', 'inf',
                 '--shape-surface-placed']) == dict(placed=True, thresholds=(0.1, 0.3), max_edge=float('inf'))
    assert opts(['--shape-surface-metrics', '--shape-max-edge', '0']) == dict(placed=False, max_edge=0.0)
    for bad in (['--shape-surface-placed'], ['--shape-surface-thresholds', '0.1'], ['--shape-max-edge', '0.5'],
                ['--shape-surface-metrics', '--shape-surface-thresholds', '0.3', '0.1'],
                ['--shape-surface-metrics', '--shape-max-edge', '-1'],
                ['--shape-surface-metrics', '--shape-max-edge', 'nan']):
        with pytest.raises(SystemExit):
            opts(bad)
    stats = dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1)
    text = run_evaluation.format_result(dict(report='r\n', shape_stats={'shape_accuracy': stats},
                                             shape_surface_stats={'shape_surface_accuracy': stats},
                                             placed_surface_stats={'placed_surface_accuracy': stats}))
    assert [l.split()[0] for l in text.splitlines()] == ['r', 'shape_accuracy', 'shape_surface_accuracy',
                                                         'placed_surface_accuracy']


def test_csv_writers(tmp_path):
    from monopsr_amd.core import distance_metrics as dm
    from monopsr_amd.core import evaluator_utils
    stats = dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1)
    for prefix, save in (('shape_surface_', evaluator_utils.save_shape_surface_stats),
                         ('placed_surface_', evaluator_utils.save_placed_surface_stats)):
        names = dm.shape_metric_names((0.05,), prefix) + (prefix + 'triangles_a', prefix + 'triangles_b')
        path = save(str(tmp_path), 'val', 7, names, {n: stats for n in names})
        assert path == os.path.join(str(tmp_path), 'metrics', 'val', '%smetrics_val.csv' % prefix)
        save(str(tmp_path), 'val', 8, names, {n: stats for n in names})
        lines = open(path).read().splitlines()
        assert len(lines) == 3 and [l.split(',')[0].strip() for l in lines] == ['step', '7', '8']
        header = [c.strip() for c in lines[0].split(',')]
        assert header[1:4] == ['accuracy_count', 'accuracy_mean', 'accuracy_std'] and len(header) == 1 + 3 * 10
        assert header[-6:] == ['triangles_a_count', 'triangles_a_mean', 'triangles_a_std', 'triangles_b_count',
                               'triangles_b_mean', 'triangles_b_std']
        assert [c.strip() for c in lines[1].split(',')][1:4] == ['3', '0.50000', '0.25000']

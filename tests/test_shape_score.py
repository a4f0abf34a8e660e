"""mpsr_shape_scores without a GPU: the restatement against itself and against hand-worked numbers, the catalogue's
properties, the entry point's argument checks and the Python surface (the device: tests/test_shape_score_gpu.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shape_score_cases as cases
import shape_score_restatement as restatement
from monopsr_amd.core import evaluator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('name', cases.NAMES)
def test_the_two_restatements_agree(name):
    c, want = cases.case(name), cases.restated(name)
    got = restatement.shape_scores(c['a'], c['b'], c['mask_a'], c['mask_b'], c['thresholds'], loop=True)
    for key in ('counts', 'sums', 'table', 'dist_a', 'dist_b'):
        assert restatement.same_bits(got[key], want[key]), (name, key)


def test_hand_worked_clouds():
    """Three clouds worked by hand.

    1. a = (0,0,0), (1,0,0); b = (0,0,0); no masks; thresholds 0.5 and 1.
       d_a = 0, 1; d_b = 0.  accuracy = (0 + 1) / 2 = 0.5; completeness = 0; chamfer_l1 = 0.25;
       chamfer_sq = (0 + 1) / 2 + 0 = 0.5; hausdorff = 1.
       At 0.5: precision 1/2, recall 1, fscore 2 (1/2) 1 / (3/2) = 2/3.  At 1: the point at distance 1 is on the
       boundary and counts: precision 1, recall 1, fscore 1.
    2. a = (0,0,0), (3,4,0), (100,100,100) with mask 1, 1, 0; b = (0,0,0), (3,4,0), (NaN,0,0) with mask 2, 0, 1:
       b's only valid point is the origin (mask 0 and a NaN coordinate leave the others out).  thresholds 4 and 5.
       d_a = 0, 25, NaN; d_b = 0, NaN, NaN; n_a = 2, n_b = 1.  accuracy = (0 + 5) / 2 = 2.5; completeness = 0;
       chamfer_l1 = 1.25; chamfer_sq = 25 / 2 = 12.5; hausdorff = 5.
       At 4: precision 1/2, recall 1, fscore 2/3.  At 5: precision 1 (boundary), recall 1, fscore 1.
    3. a = two points, both with mask 0; b = two valid points: an empty side.  n_a = 0, n_b = 2, the within counts 0,
       the six sums, the table row and both dist rows NaN.
    """
    f = np.float32
    r = restatement.shape_scores(f([[[0, 0, 0], [1, 0, 0]]]), f([[[0, 0, 0]]]), None, None, (0.5, 1.0))
    assert r['counts'].tolist() == [[2, 1, 1, 2, 1, 1]]
    assert r['sums'].tolist() == [[1.0, 1.0, 0.0, 0.0, 1.0, 0.0]]
    assert r['dist_a'].tolist() == [[0.0, 1.0]] and r['dist_b'].tolist() == [[0.0]]
    assert r['table'].tolist() == [[0.5, 0.0, 0.25, 0.5, 1.0, 0.5, 1.0, float(f(2 / 3)), 1.0, 1.0, 1.0]]

    a = f([[[0, 0, 0], [3, 4, 0], [100, 100, 100]]])
    b = f([[[0, 0, 0], [3, 4, 0], [np.nan, 0, 0]]])
    r = restatement.shape_scores(a, b, f([[1, 1, 0]]), f([[2, 0, 1]]), (4.0, 5.0))
    assert r['counts'].tolist() == [[2, 1, 1, 2, 1, 1]]
    assert r['sums'].tolist() == [[5.0, 25.0, 0.0, 0.0, 25.0, 0.0]]
    assert r['dist_a'][0, :2].tolist() == [0.0, 25.0] and np.isnan(r['dist_a'][0, 2])
    assert r['dist_b'][0, 0] == 0.0 and np.isnan(r['dist_b'][0, 1:]).all()
    assert r['table'].tolist() == [[2.5, 0.0, 1.25, 12.5, 5.0, 0.5, 1.0, float(f(2 / 3)), 1.0, 1.0, 1.0]]

    r = restatement.shape_scores(f([[[0, 0, 0], [1, 1, 1]]]), f([[[0, 0, 0], [2, 2, 2]]]), f([[0, 0]]), None, (1.0,))
    assert r['counts'].tolist() == [[0, 2, 0, 0]]
    assert np.isnan(r['sums']).all() and np.isnan(r['table']).all() and r['table'].shape == (1, 8)
    assert np.isnan(r['dist_a']).all() and np.isnan(r['dist_b']).all()


def test_the_catalogue_holds_what_it_is_meant_to_hold():
    shapes = {(cases.case(n)['a'].shape[1], cases.case(n)['b'].shape[1]) for n in cases.NAMES}
    assert {(1, 1), (7, 3), (255, 257), (256, 1024), (1025, 1023), (2304, 2304), (2304, 500)} <= shapes
    assert {1, 3, 33} <= {cases.case(n)['a'].shape[0] for n in cases.NAMES}
    assert {0, 1, 3, 8} <= {len(cases.case(n)['thresholds']) for n in cases.NAMES}
    # the constructed case: every d = 25 2^-16, on the second threshold
    r = cases.restated('constructed')
    assert (r['dist_a'] == 25 * 2.0 ** -16).all() and (r['dist_b'] == 25 * 2.0 ** -16).all()
    assert r['sums'][0].tolist() == [2304 * 5 * 2.0 ** -8, 2304 * 25 * 2.0 ** -16] * 2 + [25 * 2.0 ** -16] * 2
    assert r['counts'][0].tolist() == [2304, 2304, 0, 2304, 0, 2304]
    assert r['table'][0, 5:].tolist() == [0, 0, 0, 1, 1, 1]
    # the clone: zeros and ones
    r = cases.restated('clone')
    ok = ~np.isnan(r['dist_a'])
    assert (r['dist_a'][ok] == 0).all() and 0 < ok.sum() < ok.size and (r['sums'] == 0).all()
    assert (r['table'][:, :5] == 0).all() and (r['table'][:, 5:] == 1).all()
    # ties: distances exactly on a threshold, and duplicates
    c, r = cases.case('ties'), cases.restated('ties')
    for t in c['thresholds']:
        assert (r['dist_a'].astype(np.float64) == t * t).sum() > 10
    assert (r['dist_b'].astype(np.float64) == c['thresholds'][0] ** 2).sum() > 10
    # overflow
    r = cases.restated('overflow')
    assert np.isinf(r['dist_a'][0, 2]) and np.isinf(r['sums'][0, [0, 1, 4]]).all() and np.isinf(r['table'][0, 4])
    assert np.isfinite(r['sums'][0, [2, 3, 5]]).all()
    # the empty sides
    r = cases.restated('empty_sides')
    assert r['counts'][:, :2].tolist()[0][0] == 0 and r['counts'][1, 1] == 0 and r['counts'][2, :2].tolist() == [1, 1]
    assert r['counts'][3, :2].tolist() == [0, 0] and np.isnan(r['table'][[0, 1, 3]]).all()
    assert not np.isnan(r['table'][2]).any() and (r['counts'][[0, 1, 3], 2:] == 0).all()
    # one whole tile and one whole slab without a valid point; hostile values on both sides, some under the mask
    c = cases.case('empty_tile_and_slab')
    assert (c['mask_a'][:, 1024:2048] == 0).all() and (c['mask_b'][:, :1024] == 0).all()
    c, r = cases.case('hostile'), cases.restated('hostile')
    for cloud, mask in ((c['a'], c['mask_a']), (c['b'], c['mask_b'])):
        bad = ~np.isfinite(cloud).all(-1)
        assert np.isnan(cloud).any() and np.isinf(cloud).any() and np.isnan(mask).any()
        assert (bad & (mask > 0)).any()
    assert (r['counts'][:, :2] > 0).all()


def test_sum_bound_is_what_the_docstring_derives():
    """The device adds m fp64 terms in its own order, each root within one ulp: (m + 2) 2^-52 sum |term|."""
    assert restatement.sum_bound(10, 3.0) == 12 * 2.0 ** -52 * 3.0


# ---- the library and the Python surface, on the host


def test_symbols_are_declared_and_bound():
    from monopsr_amd import _lib
    from monopsr_amd.core import distance_metrics
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    assert re.search(r'\bint mpsr_shape_scores\s*\(', header)
    assert re.search(r'\bsize_t mpsr_shape_scores_workspace_bytes\s*\(', header)
    for name in ('mpsr_shape_scores', 'mpsr_shape_scores_workspace_bytes'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 13 and _lib.lib().mpsr_abi_version() == 13
    assert 'MPSR_SHAPE_MAX_THRESHOLDS %d' % distance_metrics.MAX_THRESHOLDS in header
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bshape_score\.hip', mk, re.M)
    assert re.search(r'^[^\n]*\bshape_score\.o[^\n]*:[^\n]*\n\t\$\(HIPCC\) \$\(FLAGS\) \$\(NOFMA\)', mk, re.M)
    src = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'shape_score.hip')).read()
    assert '#pragma clang fp contract(off)' in src and not re.search(r'\batomic\w*\s*\(', src)
    # what it shares with mpsr_surface_scores lives in the core header, under the same rule
    assert '#include "shape_score_core.h"' in src
    assert re.search(r'^[^\n]*\bshape_score\.o[^\n]*:[^\n]*\bshape_score_core\.h\b', mk, re.M)
    core = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'shape_score_core.h')).read()
    assert '#pragma clang fp contract(off)' in core and not re.search(r'\batomic\w*\s*\(', core)


def test_workspace_bytes():
    from monopsr_amd import _lib
    f = _lib.lib().mpsr_shape_scores_workspace_bytes
    # per (box, direction, slab of 1024 queries): two fp64 sums, a float maximum, 1 + T counts
    assert f(32, 2304, 2304, 3) == 32 * 2 * 3 * (16 + 4 + 4 * 4)
    assert f(1, 1, 1, 0) == 2 * (16 + 4 + 4) and f(2, 0, 0, 8) == 2 * 2 * (16 + 4 + 36)
    assert f(5, 1025, 7, 1) == 5 * 2 * 2 * (16 + 4 + 8)
    assert f(0, 10, 10, 3) == 0 and f(-1, 10, 10, 3) == 0 and f(3, 10, 10, 9) == 0 and f(1 << 20, 2048, 1, 0) == 0


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
    f = _lib.lib().mpsr_shape_scores
    fake = 4096
    dbl = lambda *v: (ctypes.c_double * max(len(v), 1))(*v)
    #     a     A     P  b     B     Q  n  t               T  w     W        c     s     o     d     e     stream
    ok = (fake, fake, 5, fake, fake, 7, 3, dbl(0.1, 0.2), 2, fake, 1 << 20, fake, fake, fake, fake, fake, None)
    call = lambda **kw: [kw.get(k, v) for k, v in zip('aAPbBQntTwWcsode_', ok)]
    for k in 'PQn':
        assert b'negative' in _refused(f, *call(**{k: -1}))
    for k in 'ab':
        assert b'cloud pointer is null' in _refused(f, *call(**{k: None}))
    for k in 'cso':
        assert b'output pointer is null' in _refused(f, *call(**{k: None}))
    assert b'workspace is null' in _refused(f, *call(w=None))
    assert b'aligned' in _refused(f, *call(w=fake + 4))
    for T in (-1, 9):
        assert b'outside 0..8' in _refused(f, *call(T=T, t=dbl(*range(1, 10))))
    assert b'thresholds is null' in _refused(f, *call(t=None))
    for bad in (float('nan'), float('inf'), 0.0, -1.0):
        assert b'not a finite distance > 0' in _refused(f, *call(t=dbl(bad, 1.0)))
    assert b'not increasing' in _refused(f, *call(t=dbl(0.2, 0.2)))
    assert b'not increasing' in _refused(f, *call(t=dbl(0.2, 0.1)))
    assert b'31 bits' in _refused(f, *call(n=1 << 20, P=2048))
    assert b'31 bits' in _refused(f, *call(n=1 << 20, Q=2048))
    assert b'not increasing' in _refused(f, *call(n=0, t=dbl(2, 1)))  # the thresholds are checked whatever n is
    need = _lib.lib().mpsr_shape_scores_workspace_bytes(3, 5, 7, 2)
    assert f(*call(W=need - 1)) == 3 and b'workspace' in _lib.lib().mpsr_last_error()
    # n == 0: a no-op, whatever the pointers; null masks and null dist pointers are no errors (P == Q == 0 reaches
    # no cloud either, but launches: the device test)
    assert f(None, None, 5, None, None, 7, 0, None, 0, None, 0, None, None, None, None, None, None) == 0


def test_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from monopsr_amd import _lib
    from monopsr_amd.core import distance_metrics as dm
    z = torch.zeros
    with pytest.raises(_lib.InvalidArgumentError, match='GPU'):
        dm.shape_scores(z((2, 5, 3)), z((2, 7, 3)))
    for a, b in ((z((2, 5, 2)), z((2, 7, 3))), (z((2, 5, 3)), z((7, 3))), (z((2, 5, 3), dtype=torch.float64), z((2, 7, 3))),
                 (np.zeros((2, 5, 3), np.float32), z((2, 7, 3)))):
        with pytest.raises(_lib.InvalidArgumentError, match='float32'):
            dm.shape_scores(a, b)
    assert issubclass(_lib.InvalidArgumentError, ValueError)


def test_shape_metric_names_and_thresholds():
    from monopsr_amd.core import distance_metrics as dm
    assert dm.DEFAULT_SHAPE_THRESHOLDS == (0.05, 0.1, 0.2)
    assert dm.shape_metric_names((), '') == ('accuracy', 'completeness', 'chamfer_l1', 'chamfer_sq', 'hausdorff')
    assert dm.shape_metric_names((0.05, 0.1, 2), 'shape_') == (
        'shape_accuracy', 'shape_completeness', 'shape_chamfer_l1', 'shape_chamfer_sq', 'shape_hausdorff',
        'shape_precision_0.05', 'shape_recall_0.05', 'shape_fscore_0.05', 'shape_precision_0.1', 'shape_recall_0.1',
        'shape_fscore_0.1', 'shape_precision_2', 'shape_recall_2', 'shape_fscore_2')
    assert len(dm.shape_metric_names(range(1, 9), 'placed_')) == 5 + 3 * 8
    assert dm.check_thresholds([1, 2]) == (1.0, 2.0) and dm.check_thresholds(()) == ()
    for bad in ((0.0,), (-1.0,), (float('nan'),), (float('inf'),), (0.2, 0.2), (0.2, 0.1), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            dm.check_thresholds(bad)
    assert dm.ShapeScores._fields == ('counts', 'sums', 'table', 'dist_a', 'dist_b', 'names')


class _Dataset(object):
    merges_mscnn, is_test = True, False

    def __init__(self, mode):
        self.train_val_test = mode


def test_evaluator_refuses_shape_metrics_outside_val_and_unknown_options():
    with pytest.raises(ValueError, match="'val'-mode"):
        evaluator.Evaluator(None, _Dataset('test'), shape_metrics={})
    with pytest.raises(ValueError, match="unknown options \\['threshold'\\]"):
        evaluator.Evaluator(None, _Dataset('val'), shape_metrics=dict(threshold=(1, 2)))
    with pytest.raises(ValueError, match='not increasing'):
        evaluator.Evaluator(None, _Dataset('val'), shape_metrics=dict(thresholds=(2, 1)))
    ev = evaluator.Evaluator(None, _Dataset('val'), shape_metrics={})
    assert ev.shape_metrics == dict(thresholds=(0.05, 0.1, 0.2), placed=False)
    assert ev.shape_table is None and ev.placed_table is None
    ev = evaluator.Evaluator(None, _Dataset('val'), shape_metrics=dict(thresholds=[1], placed=1), chunk_hook=print)
    assert ev.shape_metrics == dict(thresholds=(1.0,), placed=True) and ev.chunk_hook is print
    assert evaluator.Evaluator(None, _Dataset('val')).shape_metrics is None
    # shape_metrics stands in front of chunk_hook, which stays last (and centroid_fit next to last:
    # tests/test_proj_fit.py); it is a new name at the end of the options that came before the two
    import inspect
    names = list(inspect.signature(evaluator.Evaluator.__init__).parameters)
    assert names[-3:] == ['shape_metrics', 'centroid_fit', 'chunk_hook']
    assert inspect.signature(evaluator.Evaluator.__init__).parameters['shape_metrics'].default is None


def test_command_line_options():
    from monopsr_amd.experiments import run_evaluation
    ap = run_evaluation.build_parser()
    base = ['cfg.yaml', '--checkpoint-dir', 'c', '--mscnn-dir', 'm', '--predictions-dir', 'p']
    assert evaluator.shape_metrics_options(ap, ap.parse_args(base)) is None
    assert evaluator.shape_metrics_options(ap, ap.parse_args(base + ['--shape-metrics'])) == dict(placed=False)
    args = ap.parse_args(base + ['--shape-metrics', '--shape-thresholds', '0.1', '0.3', '--shape-placed'])
    assert evaluator.shape_metrics_options(ap, args) == dict(placed=True, thresholds=(0.1, 0.3))
    for bad in (['--shape-placed'], ['--shape-thresholds', '0.1'], ['--shape-metrics', '--shape-thresholds', '0.3', '0.1']):
        with pytest.raises(SystemExit):
            evaluator.shape_metrics_options(ap, ap.parse_args(base + bad))
    stats = dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1)
    text = run_evaluation.format_result(dict(report='r\n', shape_stats={'shape_accuracy': stats},
                                             placed_stats={'placed_accuracy': stats}))
    assert [l.split()[0] for l in text.splitlines()] == ['r', 'shape_accuracy', 'placed_accuracy']


def test_csv_writers(tmp_path):
    from monopsr_amd.core import distance_metrics as dm
    from monopsr_amd.core import evaluator_utils
    stats = dict(count=3, mean=0.5, std=0.25, mean_abs=0.5, std_abs=0.25, dropped=1)
    for prefix, save in (('shape_', evaluator_utils.save_shape_stats), ('placed_', evaluator_utils.save_placed_stats)):
        names = dm.shape_metric_names((0.05,), prefix)
        path = save(str(tmp_path), 'val', 7, names, {n: stats for n in names})
        assert path == os.path.join(str(tmp_path), 'metrics', 'val', '%smetrics_val.csv' % prefix)
        save(str(tmp_path), 'val', 8, names, {n: stats for n in names})
        lines = open(path).read().splitlines()
        assert len(lines) == 3 and [l.split(',')[0].strip() for l in lines] == ['step', '7', '8']
        header = [c.strip() for c in lines[0].split(',')]
        assert header[1:4] == ['accuracy_count', 'accuracy_mean', 'accuracy_std'] and len(header) == 1 + 3 * 8
        assert header[-1] == 'fscore_0.05_std'
        assert [c.strip() for c in lines[1].split(',')][1:4] == ['3', '0.50000', '0.25000']

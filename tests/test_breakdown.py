"""The per-object overlap table and the binned statistics without a device: the restatement the GPU tests compare
against (tests/breakdown_restatement.py) is itself checked against an independently written scalar loop, the
reference's recorded IoUs and known answers; then the two symbols, their host-side argument checks, the CSV writer and
the options of the Evaluator and the command line."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakdown_cases as C  # noqa: E402
import breakdown_restatement as BR  # noqa: E402
import test_kitti_eval as R  # noqa: E402  (Sutherland-Hodgman on Python floats, written for the AP tests)

from monopsr_amd.core import evaluator, evaluator_utils  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RASTER_BOUND_3D = 0.02  # tests/test_kitti_eval_gpu.py: the reference's 1 cm raster against the exact overlap
MEAN_TOL, STD_RTOL = 1e-10, 1e-9  # tests/test_metric_stats_gpu.py


@pytest.fixture(scope='module')
def cat():
    c = C.catalogue()
    c['restated'] = BR.object_pairs(c['pred'], c['gt'], c['fed'], c['info'], C.DEPTH_EDGES, C.BOX_IOU_EDGES)
    return c


class _Obj(object):
    def __init__(self, box7=None, box4=None):
        if box7 is not None:
            self.t1, self.t2, self.t3, self.l, self.w, self.h, self.ry = (float(v) for v in box7)
        if box4 is not None:
            self.x1, self.y1, self.x2, self.y2 = (float(v) for v in box4)


def test_catalogue_shape_and_margin(cat):
    assert len(cat['pred']) == max(C.SIZES) == 257 and cat['rows']['random'] == 57
    assert C.margin_of(cat['restated'][0]) > C.MARGIN


def test_restatement_against_an_independent_scalar_loop(cat):
    overlaps, table, bins = cat['restated']
    for i in range(len(cat['pred'])):
        p, g, f, info = (cat[k][i].astype(np.float64) for k in ('pred', 'gt', 'fed', 'info'))
        if np.isfinite(np.r_[p, g]).all():
            want_bev, want_3d = R.r_ground_overlap(_Obj(p), _Obj(g)), R.r_box3d_overlap(_Obj(p), _Obj(g))
            centre = lambda b: np.array([b[0], b[1] - b[5] / 2, b[2]])
            assert abs(overlaps[i, 1] - want_bev) <= 1e-12 and abs(overlaps[i, 2] - want_3d) <= 1e-12, i
            assert abs(overlaps[i, 3] - np.linalg.norm(centre(p) - centre(g))) <= 1e-12 * max(overlaps[i, 3], 1), i
        else:
            assert np.isnan(overlaps[i, 1:4]).all() and np.isnan(table[i, 4:9]).all(), i
        if np.isfinite(np.r_[f, info[2:]]).all():
            want = R.r_image_overlap(_Obj(box4=f[[1, 0, 3, 2]]), _Obj(box4=info[2:]))
            assert abs(overlaps[i, 0] - want) <= 1e-12, i
            assert bins[i, 2] == np.searchsorted(C.BOX_IOU_EDGES, overlaps[i, 0], side='right'), i
        else:
            assert np.isnan(overlaps[i, 0]) and bins[i, 2] == -1, i
        z = g[2]
        assert bins[i, 0] == (np.searchsorted(C.DEPTH_EDGES, z, side='right') if np.isfinite(z) else -1), i
    assert np.array_equal(table[:, 0:4], overlaps.astype(np.float32), equal_nan=True)
    ok = ~np.isnan(overlaps[:, 2])
    assert np.array_equal(table[ok, 4], (overlaps[ok, 2] >= 0.7).astype(np.float32))
    assert np.array_equal(table[ok, 6], (overlaps[ok, 2] >= 0.25).astype(np.float32))
    assert np.array_equal(table[ok, 8], (overlaps[ok, 1] >= 0.5).astype(np.float32))
    assert 0 < table[ok, 4].sum() < table[ok, 6].sum() < ok.sum()  # the thresholds separate the random pairs


def test_non_finite_rows(cat):
    overlaps, table, bins = cat['restated']
    a = cat['rows']['non_finite']
    for k in range(24):
        i = a + k
        assert np.isnan(overlaps[i, 1:4]).all() == (k < 14), k      # a field of the two 3-D boxes
        assert np.isnan(overlaps[i, 0]) == (14 <= k < 18 or k >= 20), k  # the fed box, or the label's own box
        assert (bins[i, 1] == -1) == (k >= 18), k                   # any of label_info's six values
        assert (bins[i, 0] == -1) == (k == 9), k                    # the label's z
        assert (bins[i, 2] == -1) == bool(np.isnan(overlaps[i, 0])), k


def test_reference_pins():
    g = R.golden()
    got = np.array([BR.image_iou(a, b) for a, b in zip(g['pin2d_a'], g['pin2d_b'])])
    assert np.abs(got - g['pin2d_iou']).max() <= 1e-12
    order = [4, 5, 6, 1, 3, 2, 0]  # [ry, l, h, w, tx, ty, tz] -> [x y z l w h ry]
    got3 = np.array([BR.box_overlaps(a[order], b[order])[1] for a, b in zip(g['pin3d_a'], g['pin3d_b'])])
    assert len(got3) == 174
    print('restated 3-D IoU against the 174 pins: largest difference %.4f' % np.abs(got3 - g['pin3d_iou']).max())
    assert np.abs(got3 - g['pin3d_iou']).max() <= RASTER_BOUND_3D


def test_known_answers():
    got = {name: BR.box_overlaps(p, g) for name, p, g in C.KNOWN}
    assert all(abs(v - 1) <= 1e-12 for v in got['identical'][0:2]) and got['identical'][2] == 0
    assert all(abs(v - 1 / 3) <= 1e-12 for v in got['half_length'][0:2]) and got['half_length'][2] == 0.5
    assert abs(got['rotated_45'][0] - 1 / math.sqrt(2)) <= 1e-12
    assert got['corner_touching'][0:2] == (0.0, 0.0) and got['edge_touching'][0:2] == (0.0, 0.0)
    assert got['stacked'][1] == 0 and abs(got['stacked'][0] - 1) <= 1e-12 and got['stacked'][2] == 1.0
    assert got['zero_length'][0:2] == (0.0, 0.0) and got['negative_width'][0:2] == (0.0, 0.0)
    assert got['zero_height'][1] == 0 and abs(got['zero_height'][0] - 1) <= 1e-12
    assert BR.image_iou([0, 0, 10, 10], [5, 0, 15, 10]) == 1 / 3 and BR.image_iou([0, 0, 10, 10], [10, 10, 20, 20]) == 0


def test_difficulty_levels(cat):
    for (trunc, occ, height), want in C.DIFFICULTY:
        assert BR.difficulty(np.asarray(C.difficulty_info(trunc, occ, height), np.float32)) == want, (trunc, occ, height)
    a = cat['rows']['difficulty']
    assert cat['restated'][2][a:a + len(C.DIFFICULTY), 1].tolist() == [want for _, want in C.DIFFICULTY]
    assert {0, 1, 2, 3} <= set(cat['restated'][2][:, 1].tolist())


def test_depth_edges_take_their_value_into_the_upper_bin(cat):
    a = cat['rows']['on_depth_edge']
    assert cat['restated'][2][a:a + 3, 0].tolist() == [1, 2, 5]
    assert BR.bin_of(C.DEPTH_EDGES, 9.999) == 0 and BR.bin_of(C.DEPTH_EDGES, 1e9) == 5 and BR.bin_of((), 3.0) == 0


@pytest.mark.parametrize('n_rows,axis_bins,placement', C.STATS_CASES)
def test_binned_restatement_against_numpy(n_rows, axis_bins, placement):
    values = C.place_nans(C.stats_table(n_rows, 2000 + n_rows), placement)
    bins = C.stats_bins(n_rows, axis_bins, 3000 + n_rows)
    got = BR.metric_stats_binned(values, bins, C.COLUMN_METRIC, C.N_METRICS, axis_bins)
    assert got.shape == (1 + sum(axis_bins), C.N_METRICS, 6)
    slot, slots = 1, [np.ones(n_rows, bool)]
    for a, nb in enumerate(axis_bins):  # plain per-row binning
        for b in range(nb):
            slots.append(np.array([int(row[a]) == b for row in bins], bool).reshape(n_rows))
    for s, rows in enumerate(slots):
        for m in range(C.N_METRICS):
            x = values[rows][:, [c for c, k in enumerate(C.COLUMN_METRIC) if k == m]].astype(np.float64).reshape(-1)
            kept = x[~np.isnan(x)]
            assert got[s, m, 0] == kept.size and got[s, m, 5] == x.size - kept.size, (s, m)
            if not kept.size:
                assert np.isnan(got[s, m, 1:5]).all(), (s, m)
                continue
            mean_abs = np.abs(kept).mean()
            assert abs(got[s, m, 1] - kept.mean()) <= MEAN_TOL * mean_abs and \
                abs(got[s, m, 3] - mean_abs) <= MEAN_TOL * mean_abs, (s, m)
            np.testing.assert_allclose(got[s, m, [2, 4]], [kept.std(), np.abs(kept).std()], rtol=STD_RTOL, atol=1e-300)
    for a, nb in enumerate(axis_bins):
        first = 1 + sum(axis_bins[:a])
        outside = int(((bins[:, a] < 0) | (bins[:, a] >= nb)).sum()) if n_rows else 0
        assert got[first:first + nb, 0, 0].sum() + outside == got[0, 0, 0] == n_rows
        if nb >= 2 and n_rows:
            assert got[first + nb - 1, 0, 0] == 0 and (n_rows < 50 or outside > 0)  # the empty bin; rows in no bin


# ---- the library and the Python surface, on the host

def test_symbols_are_declared_and_bound():
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    for name in ('mpsr_object_pairs', 'mpsr_metric_stats_binned'):
        assert name in _lib.SIGNATURES and re.search(r'\bint %s\s*\(' % name, header), name
        assert hasattr(_lib.lib(), name)
    assert _lib.ABI_VERSION == 13 and _lib.lib().mpsr_abi_version() == 13
    for macro, value in (('MPSR_OBJECT_PAIRS_MAX_EDGES', evaluator_utils.MAX_EDGES),
                         ('MPSR_METRIC_STATS_MAX_AXES', evaluator_utils.MAX_AXES),
                         ('MPSR_METRIC_STATS_MAX_BINS', evaluator_utils.MAX_BINS)):
        assert '%s %d' % (macro, value) in header
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bobject_pairs\.hip', mk, re.M)
    assert re.search(r'^[^\n]*\bobject_pairs\.o[^\n]*:[^\n]*\n\t\$\(HIPCC\) \$\(FLAGS\) \$\(NOFMA\)', mk, re.M)


def _refused(f, *args):
    from monopsr_amd import _lib
    assert f(*args) == 1, args
    msg = _lib.lib().mpsr_last_error()
    assert msg, args
    return msg


def test_object_pairs_argument_errors_need_no_gpu():
    """Status 1 with a message before anything touches the device: the pointers below are never dereferenced."""
    from monopsr_amd import _lib
    f = _lib.lib().mpsr_object_pairs
    fake = 4096
    dbl = lambda *v: (ctypes.c_double * max(len(v), 1))(*v)
    de, ie = dbl(10, 20, 30), dbl(0.7, 0.9)
    ok = (fake, fake, fake, fake, 5, de, 3, ie, 2, fake, fake, fake, None)
    call = lambda **kw: [kw.get(k, v) for k, v in zip('abcdnEeIiotzs', ok)]
    assert b'negative' in _refused(f, *call(n=-1))
    for k in 'ab':
        assert b'box pointer is null' in _refused(f, *call(**{k: None}))
    for k in 'otz':
        assert b'output pointer is null' in _refused(f, *call(**{k: None}))
    assert b'not increasing' in _refused(f, *call(E=dbl(10, 10, 30)))
    assert b'not increasing' in _refused(f, *call(I=dbl(0.9, 0.7)))
    assert b'not finite' in _refused(f, *call(E=dbl(10, float('nan'), 30)))
    assert b'not finite' in _refused(f, *call(I=dbl(0.7, float('inf'))))
    assert b'too many' in _refused(f, *call(E=dbl(*range(16)), e=16))
    assert b'too many' in _refused(f, *call(i=-1))
    assert b'null' in _refused(f, *call(E=None))
    assert b'not increasing' in _refused(f, *call(n=0, E=dbl(3, 2, 1)))  # the edges are checked whatever n is
    assert f(None, None, None, None, 0, None, 0, None, 0, None, None, None, None) == 0  # n == 0: a no-op
    assert f(None, None, None, None, 0, dbl(*range(15)), 15, ie, 2, None, None, None, None) == 0


def test_metric_stats_binned_argument_errors_need_no_gpu():
    from monopsr_amd import _lib
    f = _lib.lib().mpsr_metric_stats_binned
    fake = 4096
    ints = lambda *v: (ctypes.c_int * max(len(v), 1))(*v)
    cm = ints(*C.COLUMN_METRIC)
    ok = (fake, fake, 5, 10, cm, 8, 2, ints(6, 4), fake, None)
    call = lambda **kw: [kw.get(k, v) for k, v in zip('vbrcmMaAos', ok)]
    for k in 'rcMa':
        assert b'negative' in _refused(f, *call(**{k: -1}))
    assert b'limit' in _refused(f, *call(c=33, m=ints(*([0] * 33))))
    assert b'n_metrics' in _refused(f, *call(M=11))
    assert b'n_axes 5' in _refused(f, *call(a=5, A=ints(1, 1, 1, 1, 1)))
    assert b'65 bins' in _refused(f, *call(a=3, A=ints(30, 30, 5)))
    assert b'axis_bins[1]' in _refused(f, *call(A=ints(6, -1)))
    assert b'axis_bins is null' in _refused(f, *call(A=None))
    for bad in (8, -1):
        assert b'column_metric[9]' in _refused(f, *call(m=ints(*(C.COLUMN_METRIC[:9] + (bad,)))))
    assert b'column_metric is null' in _refused(f, *call(m=None))
    assert b'stats is null' in _refused(f, *call(o=None))
    assert b'table pointer is null' in _refused(f, *call(v=None))
    assert b'table pointer is null' in _refused(f, *call(b=None))
    assert f(None, None, 0, 0, None, 0, 0, None, None, None) == 0  # nothing to write


def test_wrappers_refuse_cpu_tensors():
    from monopsr_amd import _lib
    from monopsr_amd.core import evaluation
    z = torch.zeros
    with pytest.raises(_lib.MpsrError, match='GPU'):
        evaluator_utils.object_pairs(z((3, 7)), z((3, 7)))
    with pytest.raises(ValueError, match='gt_box_3d'):
        evaluator_utils.object_pairs(z((3, 7)), z((2, 7)))
    with pytest.raises(ValueError, match='fed_box_2d'):
        evaluator_utils.object_pairs(z((3, 7)), z((3, 7)), z((3, 5)))
    with pytest.raises(_lib.MpsrError, match='GPU'):
        evaluator_utils.metric_stats_binned(z((3, 10)), z((3, 2), dtype=torch.int32), C.COLUMN_METRIC, 8, (6, 4))
    with pytest.raises(ValueError, match='int32'):
        evaluator_utils.metric_stats_binned(z((3, 10)), z((3, 2)), C.COLUMN_METRIC, 8, (6, 4))
    for fn, width in ((evaluation.two_d_iou, 4), (evaluation.three_d_iou, 7), (evaluation.bev_iou, 7)):
        with pytest.raises(_lib.MpsrError, match='GPU'):
            fn(z(width), z((2, width)))
    with pytest.raises(_lib.MpsrError, match='GPU'):
        evaluation.paired_overlaps(z((3, 7)), z((3, 7)))
    with pytest.raises(_lib.MpsrError, match='GPU'):
        evaluation.mask_iou(z((4, 4)), z((4, 4)))


def test_labels():
    assert evaluator_utils.edge_labels((10, 20, 30, 40, 50)) == ['<10', '10-20', '20-30', '30-40', '40-50', '>=50']
    assert evaluator_utils.edge_labels((0.7, 0.8, 0.9)) == ['<0.7', '0.7-0.8', '0.8-0.9', '>=0.9']
    assert evaluator_utils.edge_labels(()) == ['all']
    assert len(evaluator_utils.PAIR_COLUMNS) == 9 and evaluator_utils.BREAKDOWN_AXES == ('depth', 'difficulty', 'fed_box')


def _breakdown(scale):
    nan = float('nan')
    st = lambda n, mean: dict(count=n, mean=mean * scale, std=0.5, mean_abs=abs(mean), std_abs=0.25, dropped=1)
    empty = dict(count=0, mean=nan, std=nan, mean_abs=nan, std_abs=nan, dropped=0)
    stats = np.array([[list(st(5, 0.123456789).values()), list(st(5, -2.0).values())],
                      [list(st(3, 0.5).values()), list(st(3, -1.0).values())],
                      [list(empty.values())] * 2,
                      [list(st(2, 0.25).values()), list(st(2, -4.0).values())]])
    return evaluator_utils.breakdown_dict([('depth', ['<10', '>=10']), ('difficulty', ['easy'])],
                                          [('object', ('iou_3d', 'centre_dist'), stats)])


def test_breakdown_dict_and_csv_byte_for_byte(tmp_path):
    b = _breakdown(1.0)
    assert b['axes'] == {'depth': ['<10', '>=10'], 'difficulty': ['easy']}
    assert b['all']['object']['iou_3d'] == dict(count=5, mean=0.123456789, std=0.5, mean_abs=0.123456789, std_abs=0.25,
                                                dropped=1)
    assert b['tables']['object']['depth']['>=10']['centre_dist']['count'] == 0
    assert b['tables']['object']['difficulty']['easy']['centre_dist']['mean'] == -4.0
    path = evaluator_utils.save_breakdown(str(tmp_path), 'val', 120000, b)
    assert path == os.path.join(str(tmp_path), 'metrics', 'val', 'breakdown_val.csv')
    first = (b'step,table,axis,bin,metric,count,mean,std,mean_abs,std_abs,dropped\r\n'
             b'120000,object,all,all,iou_3d,5,0.12346,0.50000,0.12346,0.25000,1\r\n'
             b'120000,object,all,all,centre_dist,5,-2.00000,0.50000,2.00000,0.25000,1\r\n'
             b'120000,object,depth,<10,iou_3d,3,0.50000,0.50000,0.50000,0.25000,1\r\n'
             b'120000,object,depth,<10,centre_dist,3,-1.00000,0.50000,1.00000,0.25000,1\r\n'
             b'120000,object,depth,>=10,iou_3d,0,nan,nan,nan,nan,0\r\n'
             b'120000,object,depth,>=10,centre_dist,0,nan,nan,nan,nan,0\r\n'
             b'120000,object,difficulty,easy,iou_3d,2,0.25000,0.50000,0.25000,0.25000,1\r\n'
             b'120000,object,difficulty,easy,centre_dist,2,-4.00000,0.50000,4.00000,0.25000,1\r\n')
    with open(path, 'rb') as f:
        assert f.read() == first
    # a second call appends its lines and no header
    evaluator_utils.save_breakdown(str(tmp_path), 'val', 130000, _breakdown(2.0))
    with open(path, 'rb') as f:
        text = f.read()
    assert text.startswith(first) and text.count(b'step,') == 1 and text.count(b'\r\n') == 17
    assert b'130000,object,depth,<10,centre_dist,3,-2.00000,0.50000,1.00000,0.25000,1\r\n' in text


def test_run_evaluation_parser_accepts_the_flags():
    from monopsr_amd.experiments import run_evaluation
    ap = run_evaluation.build_parser()
    need = ['c.yaml', '--checkpoint-dir', 'k', '--mscnn-dir', 'd', '--predictions-dir', 'p']
    plain = ap.parse_args(need)
    assert plain.breakdown is False and evaluator.breakdown_options(ap, plain) is None
    assert evaluator.breakdown_options(ap, ap.parse_args(need + ['--breakdown'])) == {}
    args = ap.parse_args(need + ['--breakdown', '--depth-edges', '15', '30.5', '--box-iou-edges', '0.5'])
    assert evaluator.breakdown_options(ap, args) == dict(depth_edges=[15.0, 30.5], box_iou_edges=[0.5])
    with pytest.raises(SystemExit):
        evaluator.breakdown_options(ap, ap.parse_args(need + ['--depth-edges', '15']))


class _Dataset(object):
    merges_mscnn, is_test = True, False

    def __init__(self, mode):
        self.train_val_test = mode


def test_evaluator_refuses_breakdown_outside_val_and_unknown_options():
    with pytest.raises(ValueError, match="'val'-mode"):
        evaluator.Evaluator(None, _Dataset('test'), breakdown={})
    with pytest.raises(ValueError, match="unknown options \\['depth_edge'\\]"):
        evaluator.Evaluator(None, _Dataset('val'), breakdown=dict(depth_edge=(1, 2)))
    ev = evaluator.Evaluator(None, _Dataset('val'), breakdown=dict(depth_edges=(15, 30)))
    assert ev.breakdown == dict(depth_edges=(15.0, 30.0), box_iou_edges=(0.7, 0.8, 0.9)) and ev.pair_table is None
    assert evaluator.Evaluator(None, _Dataset('val')).breakdown is None

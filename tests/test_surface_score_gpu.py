"""mpsr_surface_scores on the device against tests/surface_score_restatement.py over tests/surface_score_cases.py and
against mpsr_shape_scores on the same inputs, then the evaluator's shape_surface_metrics end to end on the fixture split
(the host side: tests/test_surface_score.py).

The device is compared with the VECTORISED restatement, which covers every point; tests/test_surface_score.py holds
that one to the plain loop over queries and triangles bit for bit, on every point of the small grids and on a fixed
subset of the larger ones (the loop costs microseconds a pair)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mscnn_split
import scene_score_restatement
import shape_score_calls as calls
import surface_score_cases as cases
import surface_score_restatement as restatement
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import distance_metrics as dm
from monopsr_amd.datasets.kitti import instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
OUTPUTS = ('counts', 'sums', 'table', 'dist_a', 'dist_b', 'tri_counts')


def _call(c, poison=False, offset=0, thresholds=None, workspace_short=0, max_edge=None):
    """One mpsr_surface_scores call through the C entry point.  Every output sits `offset` elements into an allocation
    with a guard element behind it; poison fills outputs and workspace with NaN / 0xFF first (else with zeros).
    -> (status, {name: numpy array}, the buffers' values before)."""
    n, h, w = c['a'].shape[:3]
    P = h * w
    thr = tuple(c['thresholds'] if thresholds is None else thresholds)
    T = len(thr)
    shapes = dict(counts=((n, 2 + 2 * T), torch.int32), sums=((n, 6), torch.float64),
                  table=((n, 5 + 3 * T), torch.float32), dist_a=((n, P), torch.float64), dist_b=((n, P), torch.float64),
                  tri_counts=((n, 2), torch.int32))
    lib = _lib.lib()
    need = int(lib.mpsr_surface_scores_workspace_bytes(n, h, w, T))
    assert need % 8 == 0 and (need > 0) == (n > 0 and T <= dm.MAX_THRESHOLDS)

    def launch(inputs, out, ws):
        a, ma, b, mb = inputs
        return lib.mpsr_surface_scores(
            a, ma, b, mb, n, h, w, (ctypes.c_double * max(T, 1))(*thr), T,
            float(c['max_edge'] if max_edge is None else max_edge), ws, need - workspace_short, out['counts'],
            out['sums'], out['table'], out['dist_a'], out['dist_b'], out['tri_counts'], _lib.stream())
    return calls.guarded_call([c[k] for k in ('a', 'mask_a', 'b', 'mask_b')], shapes, need, launch, poison, offset)


@pytest.fixture(scope='module')
def device_results():
    return {}


def _result(device_results, name):
    if name not in device_results:
        status, out, _ = _call(cases.case(name), poison=True)
        assert status == 0, _lib.lib().mpsr_last_error()
        device_results[name] = out
    return device_results[name]


@pytest.mark.parametrize('name', cases.NAMES)
def test_catalogue_equals_the_restatement(device_results, name):
    """counts, tri_counts, dist_a, dist_b and the two maxima bit for bit (every operation is an IEEE float32 or fp64
    operation in a stated order without contraction, and a minimum has no order); the four sums within (m + 2) 2^-52
    sum |term|, bit for bit where every term is exact; the table from the device's own counts and sums, to a float32
    neighbour; NaN exactly where defined."""
    c, want, got = cases.case(name), cases.restated(name), _result(device_results, name)
    T = len(c['thresholds'])
    for key in ('counts', 'tri_counts', 'dist_a', 'dist_b'):
        assert restatement.same_bits(got[key], want[key]), (name, key)
    assert restatement.same_bits(got['sums'][:, 4:6], want['sums'][:, 4:6]), name
    calls.assert_sums_within_the_bound(name, got['sums'], want, cases.EXACT_SUMS.get(name, ()))
    own = restatement.table(got['counts'], got['sums'], T)
    assert calls.neighbours(got['table'], own), name
    empty = (want['counts'][:, 0] == 0) | (want['counts'][:, 1] == 0)
    assert np.array_equal(np.isnan(got['table']).all(1), empty) and np.array_equal(np.isnan(got['table']).any(1), empty)
    assert np.array_equal(np.isnan(got['sums']).all(1), empty) and np.array_equal(np.isnan(got['sums']).any(1), empty)
    assert (got['counts'][empty, 2:] == 0).all()
    assert np.isnan(got['dist_a'][empty]).all() and np.isnan(got['dist_b'][empty]).all()
    n, h, w = c['a'].shape[:3]
    for side in 'ab':
        ok = np.stack([restatement.points.valid_points(c[side][k].reshape(-1, 3),
                                                       None if c['mask_' + side] is None else c['mask_' + side][k])
                       for k in range(n)])
        assert np.array_equal(np.isnan(got['dist_' + side]), ~ok | empty[:, None]), (name, side)


def _point_call(c):
    """mpsr_shape_scores on the same inputs: -> ShapeScores with the dist rows"""
    n, h, w = c['a'].shape[:3]
    up = lambda k: None if c[k] is None else torch.from_numpy(np.array(c[k])).cuda()
    return dm.shape_scores(up('a').reshape(n, h * w, 3), up('b').reshape(n, h * w, 3), up('mask_a'), up('mask_b'),
                           c['thresholds'], want_dists=True)


@pytest.mark.parametrize('name', cases.NAMES)
def test_never_farther_than_the_nearest_point(device_results, name):
    """dist <= (double) mpsr_shape_scores' dist elementwise, exactly, NaN in the same places."""
    got, point = _result(device_results, name), _point_call(cases.case(name))
    for side, p in (('a', point.dist_a), ('b', point.dist_b)):
        d, p = got['dist_' + side], p.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(d), np.isnan(p)), (name, side)
        live = ~np.isnan(d)
        assert bool((d[live] <= p[live]).all()), (name, side)
    assert np.array_equal(got['counts'][:, :2], point.counts[:, :2].cpu().numpy())


@pytest.mark.parametrize('name', ('max_edge_zero', 'holes', 'hostile', 'overflow', 'empty_sides', 'half_cylinder'))
def test_max_edge_zero_is_mpsr_shape_scores(name):
    """At max_edge = 0 no triangle adds a term: counts, dist and the maxima equal mpsr_shape_scores' bit for bit, the
    sums within the bound (the two kernels add in different orders)."""
    c = cases.case(name)
    status, got, _ = _call(c, poison=True, max_edge=0.0)
    assert status == 0, _lib.lib().mpsr_last_error()
    point = _point_call(c)
    assert np.array_equal(got['counts'], point.counts.cpu().numpy()) and (got['tri_counts'] == 0).all()
    for side, p in (('a', point.dist_a), ('b', point.dist_b)):
        assert restatement.same_bits(got['dist_' + side], p.cpu().numpy().astype(np.float64)), (name, side)
    ps = point.sums.cpu().numpy()
    assert restatement.same_bits(got['sums'][:, 4:6], ps[:, 4:6])
    gs, ws = got['sums'][:, 0:4], ps[:, 0:4]
    special = ~np.isfinite(ws)
    assert restatement.same_bits(np.where(special, gs, 0.0), np.where(special, ws, 0.0)), name
    m = np.repeat(got['counts'][:, :2], 2, axis=1)
    err = np.abs(np.where(special, 0.0, gs) - np.where(special, 0.0, ws))
    assert bool((err <= restatement.sum_bound(m, np.where(special, 0.0, ws))).all()), name


@pytest.mark.parametrize('name', ('hostile', 'random_masks', 'empty_sides', 'holes'))
def test_two_runs_poison_and_odd_offsets_return_the_same_bytes(device_results, name):
    """The same bytes from a second run, from zeroed instead of NaN / 0xFF-filled outputs and workspace, and from
    pointers one and three elements into larger allocations; the elements around every buffer keep their values."""
    first = calls.output_bytes(_result(device_results, name), OUTPUTS)
    for kw in (dict(poison=True), dict(poison=False), dict(poison=True, offset=1), dict(poison=False, offset=3)):
        status, out, _ = _call(cases.case(name), **kw)
        assert status == 0 and calls.output_bytes(out, OUTPUTS) == first, (name, kw)


def test_wrapper_null_dist_pointers_and_refusals():
    c, want = cases.case('random_masks'), cases.restated('random_masks')
    up = lambda k: None if c[k] is None else torch.from_numpy(np.array(c[k])).cuda()
    s = dm.surface_scores(up('a'), up('b'), up('mask_a'), up('mask_b'), c['thresholds'], c['max_edge'])
    assert s.dist_a is None and s.dist_b is None and s.names == dm.shape_metric_names(c['thresholds'])
    assert restatement.same_bits(s.counts.cpu().numpy(), want['counts'])
    assert restatement.same_bits(s.tri_counts.cpu().numpy(), want['tri_counts'])
    assert s.sums.dtype == torch.float64 and s.table.dtype == torch.float32 and s.tri_counts.dtype == torch.int32
    # (n, h, w, 1) masks, the dist rows in fp64; the default max_edge is the case's 0.5
    s4 = dm.surface_scores(up('a'), up('b'), up('mask_a').reshape(33, 17, 16, 1), up('mask_b'), c['thresholds'],
                           want_dists=True)
    assert torch.equal(s4.counts, s.counts) and torch.equal(s4.sums.view(torch.int64), s.sums.view(torch.int64))
    assert s4.dist_a.dtype == torch.float64 and restatement.same_bits(s4.dist_a.cpu().numpy(), want['dist_a'])
    z = dm.surface_scores(up('a')[:0], up('b')[:0], thresholds=())
    assert tuple(z.counts.shape) == (0, 2) and tuple(z.table.shape) == (0, 5) and tuple(z.tri_counts.shape) == (0, 2)
    with pytest.raises(_lib.InvalidArgumentError, match='one float32 entry per point'):
        dm.surface_scores(up('a'), up('b'), up('mask_a')[:, :5])
    with pytest.raises(_lib.InvalidArgumentError, match='points_b'):
        dm.surface_scores(up('a'), up('b')[:5])
    with pytest.raises(_lib.InvalidArgumentError, match='points_b'):
        dm.surface_scores(up('a'), up('b').reshape(33, 16, 17, 3))
    with pytest.raises(_lib.InvalidArgumentError, match='not increasing'):
        dm.surface_scores(up('a'), up('b'), thresholds=(0.2, 0.1))
    with pytest.raises(_lib.InvalidArgumentError, match='max_edge'):
        dm.surface_scores(up('a'), up('b'), max_edge=-1.0)
    with pytest.raises(_lib.InvalidArgumentError, match='no point'):
        dm.surface_scores(up('a')[:, :0], up('b')[:, :0])


def test_more_work_items_than_the_grid_has_workgroups():
    """2^19 + 3 boxes of a (1, 1) grid are 2^20 + 6 work items, more than the 2^20 workgroups the search kernel is
    launched with at most: the last six are reached by the grid's stride, and the step past them must end the loop.
    One point a side and no triangle make the restatement a line of numpy."""
    n = (1 << 19) + 3
    rng = np.random.default_rng(21)
    a, b = (rng.standard_normal((n, 1, 1, 3)).astype(np.float32) for _ in range(2))
    ma, mb = ((rng.uniform(size=(n, 1)) < 0.9).astype(np.float32) for _ in range(2))
    ma[-1], mb[-1], ma[-2], mb[-2], ma[-3] = 1.0, 1.0, 1.0, 1.0, 0.0  # the strided items: two whole boxes, an empty side
    t = 1.5
    status, got, _ = _call(dict(a=a, b=b, mask_a=ma, mask_b=mb, thresholds=(t,), max_edge=0.5), poison=True)
    assert status == 0, _lib.lib().mpsr_last_error()
    both = (ma[:, 0] > 0) & (mb[:, 0] > 0)
    delta = b[:, 0, 0] - a[:, 0, 0]
    d = (delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2]
    assert d.dtype == np.float32 and 0 < both.sum() < n
    d64 = np.where(both, d.astype(np.float64), np.nan)
    assert restatement.same_bits(got['dist_a'][:, 0], d64) and restatement.same_bits(got['dist_b'][:, 0], d64)
    within = (both & (d.astype(np.float64) <= t * t)).astype(np.int32)
    want_counts = np.stack([(ma[:, 0] > 0).astype(np.int32), (mb[:, 0] > 0).astype(np.int32), within, within], 1)
    assert np.array_equal(got['counts'], want_counts) and (got['tri_counts'] == 0).all()
    root = np.sqrt(d64)
    assert restatement.same_bits(got['sums'][:, [1, 3, 4, 5]], np.stack([d64] * 4, 1))
    for k in (0, 2):  # a sum of one term: the root itself, within the bound's three ulps
        err = np.abs(np.where(both, got['sums'][:, k] - root, 0.0))
        assert np.array_equal(np.isnan(got['sums'][:, k]), ~both)
        assert bool((err <= restatement.sum_bound(1, np.where(both, root, 0.0))).all())
    own = restatement.table(got['counts'], got['sums'], 1)
    assert calls.neighbours(got['table'], own)


def test_argument_errors_leave_the_outputs_untouched():
    c = cases.case('row')
    for kw, status, text in ((dict(thresholds=(0.5, 0.25)), 1, b'not increasing'),
                             (dict(thresholds=(float('nan'),)), 1, b'finite'),
                             (dict(thresholds=tuple(range(1, 10))), 1, b'outside'),
                             (dict(max_edge=-1.0), 1, b'max_edge'), (dict(max_edge=float('nan')), 1, b'max_edge'),
                             (dict(workspace_short=8), 3, b'workspace')):
        got, out, before = _call(c, poison=True, offset=1, **kw)
        assert got == status and text in _lib.lib().mpsr_last_error(), kw
        for k in OUTPUTS:
            assert np.isnan(out[k]).all() if out[k].dtype.kind == 'f' else (out[k] == -1).all(), (kw, k)


# ---- end to end: the fixture split, a small random-weight net (built as tests/test_shape_score_gpu.py's setup)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_surface_score')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    val = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    test = kitti_dataset.KittiDataset(mscnn_split.config(root, has_kitti_labels=True), 'test', mscnn_label_dir=mscnn)
    return root, mscnn, model, val, test


def _clouds_of_chunk(model, samples, outs):
    counts = [int(s['num_objs']) for s in samples]
    roi, total = tuple(model.map_roi_size), sum(counts)
    host = lambda ts, width: torch.cat(ts).reshape((total,) + roi + (3,)).cpu().numpy() if width else \
        torch.cat(ts).reshape(total, -1).cpu().numpy()
    return dict(
        local=host([o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n] for o, n in zip(outs, counts)], 3),
        placed=host([instance_utils.tf_inst_xyz_map_local_to_global(
            o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n], roi, o[constants.KEY_VIEW_ANG][0:n],
            o[constants.KEY_CENTROIDS][0:n]) for o, n in zip(outs, counts)], 3),
        gt_local=host([s['gt_inst_xyz_maps_local'][0:n] for s, n in zip(samples, counts)], 3),
        gt_global=host([s['gt_inst_xyz_maps_global'][0:n] for s, n in zip(samples, counts)], 3),
        mask=host([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)], 0))


@pytest.fixture(scope='module')
def restated_chunks():
    """The restatement of a chunk's clouds, computed once per (clouds, thresholds, max_edge)."""
    cache = {}

    def restate(chunks, a, b, thresholds, max_edge):
        parts = []
        for c in chunks:
            key = (c[a].tobytes(), c[b].tobytes(), c['mask'].tobytes(), tuple(thresholds), max_edge)
            if key not in cache:
                cache[key] = restatement.surface_scores(c[a], c[b], c['mask'], c['mask'], thresholds, max_edge)
            parts.append(cache[key])
        return {k: np.concatenate([p[k] for p in parts])
                for k in ('counts', 'sums', 'table', 'terms', 'abs_sums', 'tri_counts')}
    return restate


def _assert_table_and_stats(kept, want, stats, names):
    """The evaluator's table (table with the two triangle columns, counts, sums, frame) against the restated chunks, and
    the statistics against mpsr_metric_stats' restatement (scene_score_restatement.stats) of the evaluator's own table
    (only fp64 summation order separates the two: 8 n 2^-53 (mean |x| + std |x|), as tests/test_shape_score_gpu.py)
    and of the restated table (every entry on a float32 neighbour: 2^-22 (mean |x| + std |x|))."""
    table, counts, sums, frame = kept
    assert np.array_equal(counts.cpu().numpy(), want['counts']) and frame.numel() == len(want['counts'])
    assert restatement.same_bits(sums[:, 4:6].cpu().numpy(), want['sums'][:, 4:6])
    live = np.isfinite(want['sums'][:, 0:4])
    err = np.abs(np.where(live, sums[:, 0:4].cpu().numpy(), 0.0) - np.where(live, want['sums'][:, 0:4], 0.0))
    assert bool((err <= restatement.sum_bound(want['terms'], np.where(live, want['abs_sums'], 0.0))).all())
    host = table.cpu().numpy()
    assert calls.neighbours(host[:, :-2], want['table'])
    assert np.array_equal(host[:, -2:], want['tri_counts'].astype(np.float32))
    want_table = np.concatenate([want['table'], want['tri_counts'].astype(np.float32)], 1)
    assert list(stats) == list(names) and len(names) == want_table.shape[1]
    assert names[-2].endswith('triangles_a') and names[-1].endswith('triangles_b')
    own_stats, want_stats = scene_score_restatement.stats(host), scene_score_restatement.stats(want_table)
    for k, name in enumerate(names):
        st = stats[name]
        assert st['count'] == int(own_stats[k, 0]) == int(want_stats[k, 0]), name
        assert st['dropped'] == len(want['counts']) - st['count'], name
        tight = 8 * max(int(own_stats[k, 0]), 1) * 2.0 ** -53 * (own_stats[k, 3] + own_stats[k, 4])
        tol = 2.0 ** -22 * (want_stats[k, 3] + want_stats[k, 4])
        for j, key in enumerate(('mean', 'std', 'mean_abs', 'std_abs')):
            for w, bound in ((own_stats[k, 1 + j], tight), (want_stats[k, 1 + j], tol)):
                assert np.isnan(st[key]) if np.isnan(w) else abs(st[key] - w) <= bound, (name, key, st[key], w)


def _names(thr, prefix):
    return dm.shape_metric_names(thr, prefix) + (prefix + 'triangles_a', prefix + 'triangles_b')


@pytest.fixture(scope='module')
def unfitted(setup, tmp_path_factory):
    """Evaluator(shape_surface_metrics={'placed': True}) next to a plain run: (plain result, scored result, the
    evaluator, the chunks' clouds, the directory)."""
    _, _, model, val, _ = setup
    base = tmp_path_factory.mktemp('surface_runs')
    plain = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(base / 'plain'), batch_size=2,
                                metric_stats=True).run_once(5)
    chunks = []
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(base / 'scored'), batch_size=2,
                             metric_stats=True, shape_surface_metrics={'placed': True},
                             chunk_hook=lambda rows, samples, outs: chunks.append(_clouds_of_chunk(model, samples, outs)))
    scored = ev.run_once(5)
    return plain, scored, ev, chunks, base


def test_evaluator_surface_stats_equal_the_restatement(setup, unfitted, restated_chunks):
    _, _, model, val, test = setup
    plain, scored, ev, chunks, base = unfitted
    assert len(chunks) == (val.num_samples + 1) // 2 >= 2
    thr, edge = dm.DEFAULT_SHAPE_THRESHOLDS, dm.DEFAULT_SHAPE_MAX_EDGE
    shape = restated_chunks(chunks, 'local', 'gt_local', thr, edge)
    placed = restated_chunks(chunks, 'placed', 'gt_global', thr, edge)
    assert len(shape['counts']) == scored['num_predictions'] and int((shape['counts'][:, :2] > 0).all(1).sum()) >= 4
    assert (shape['tri_counts'] > 0).any()  # the fixture's maps have triangles within half a metre: not vacuous
    _assert_table_and_stats(ev.shape_surface_table, shape, scored['shape_surface_stats'], _names(thr, 'shape_surface_'))
    _assert_table_and_stats(ev.placed_surface_table, placed, scored['placed_surface_stats'],
                            _names(thr, 'placed_surface_'))
    # both CSVs: a header and one line
    for kind in ('shape_surface', 'placed_surface'):
        stats = scored[kind + '_stats']
        path = os.path.join(str(base / 'scored'), 'metrics', val.data_split, '%s_metrics_%s.csv' % (kind, val.data_split))
        assert scored[kind + '_metrics_csv'] == path
        lines = open(path).read().splitlines()
        assert len(lines) == 2 and lines[0].split(',')[0].strip() == 'step' and lines[1].split(',')[0].strip() == '5'
        fields = [c.strip() for c in lines[1].split(',')]
        assert len(fields) == 1 + 3 * 16 and fields[1] == '%d' % stats[kind + '_accuracy']['count']
        assert float(fields[2]) == float('%.5f' % stats[kind + '_accuracy']['mean'])
        assert [c.strip() for c in lines[0].split(',')][-3] == 'triangles_b_count'
        assert not os.path.exists(path.replace(str(base / 'scored'), str(base / 'plain')))
    # everything else is what it is without shape_surface_metrics
    calls.same_elsewhere(plain, scored, {'shape_surface_stats', 'placed_surface_stats', 'shape_surface_metrics_csv',
                                    'placed_surface_metrics_csv'}, val)
    assert 'shape_surface_stats' not in plain and 'shape_stats' not in scored
    with pytest.raises(ValueError):
        evaluator.Evaluator(model, test, THRESHOLD, shape_surface_metrics={})


def test_evaluator_fitted_centroids_breakdown_and_shape_metrics(setup, unfitted, restated_chunks, tmp_path):
    """With centroid_fit the shape_surface_* table keeps its bits and the placed_surface_* table comes from the fitted
    centroids; with breakdown the kinds 'shape_surface' and 'placed_surface' appear; shape_metrics next to it gives
    its own tables, never farther from the surface than from the points."""
    _, _, model, val, _ = setup
    _, _, ev0, chunks0, _ = unfitted
    chunks = []
    thr = (0.1, 0.5)
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path), batch_size=2,
                             shape_surface_metrics={'placed': True, 'thresholds': thr, 'max_edge': 0.5},
                             shape_metrics={'placed': True, 'thresholds': thr}, centroid_fit={}, breakdown={},
                             chunk_hook=lambda rows, samples, outs: chunks.append(_clouds_of_chunk(model, samples, outs)))
    result = ev.run_once(6)
    for k in range(len(chunks)):
        assert np.array_equal(chunks[k]['local'], chunks0[k]['local'])
    # the object's own frame: the first five columns, the triangle columns, the valid counts and the sums
    for cols in (slice(0, 5), slice(-2, None)):
        assert torch.equal(ev.shape_surface_table[0][:, cols].view(torch.int32),
                           ev0.shape_surface_table[0][:, cols].view(torch.int32))
    assert torch.equal(ev.shape_surface_table[1][:, :2], ev0.shape_surface_table[1][:, :2])
    assert torch.equal(ev.shape_surface_table[2].view(torch.int64), ev0.shape_surface_table[2].view(torch.int64))
    # placed: from the fitted centroids, which the hook saw
    placed = restated_chunks(chunks, 'placed', 'gt_global', thr, 0.5)
    _assert_table_and_stats(ev.placed_surface_table, placed, result['placed_surface_stats'],
                            _names(thr, 'placed_surface_'))
    fit = result['centroid_fit']
    assert fit['converged'] + fit['capped'] > 0
    moved = any(not np.array_equal(c['placed'], c0['placed']) for c, c0 in zip(chunks, chunks0))
    assert moved and not torch.equal(ev.placed_surface_table[2].view(torch.int64),
                                     ev0.placed_surface_table[2].view(torch.int64))
    # the point scores of the same run: the same valid counts, sums that are no smaller
    for surface, point in ((ev.shape_surface_table, ev.shape_table), (ev.placed_surface_table, ev.placed_table)):
        assert torch.equal(surface[1][:, :2], point[1][:, :2])
        s, p = surface[2].cpu().numpy(), point[2].cpu().numpy()
        live = ~np.isnan(p[:, 0])
        assert np.array_equal(np.isnan(s[:, 0]), ~live) and bool((s[live][:, 4:6] <= p[live][:, 4:6]).all())
        assert bool((surface[1][:, 2:] >= point[1][:, 2:]).all())
    # the breakdown's kinds, and slot 0
    bd = result['breakdown']
    kinds = {'shape_surface', 'placed_surface', 'shape', 'placed'}
    assert {'object'} | kinds <= set(bd['all']) and kinds <= set(bd['tables'])
    for kind in ('shape_surface', 'placed_surface'):
        assert repr(bd['all'][kind]) == repr(result[kind + '_stats']), kind
        assert set(bd['tables'][kind]) == {'depth', 'difficulty', 'fed_box'}
    text = open(result['breakdown_csv']).read()
    assert ',shape_surface,all,all,shape_surface_accuracy,' in text and ',placed_surface,depth,' in text


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


def test_run_evaluation_command_line(setup, tmp_path, capsys):
    """--shape-surface-metrics --shape-surface-placed on the fixture split and one saved checkpoint: the lines after
    the report, in the tables' order, and one line in each CSV."""
    import yaml
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    from monopsr_amd.experiments import run_evaluation
    root, mscnn, _, _, _ = setup
    ckpts = str(tmp_path / 'ckpts')
    os.makedirs(ckpts)
    checkpoint_utils.save_checkpoint(os.path.join(ckpts, 'monopsr'),
                                     W.synthetic_weights(seed=92, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)), 40)
    with open(os.path.join(os.path.dirname(config_utils.__file__), '..', 'configs', 'monopsr_model_000.yaml')) as f:
        cfg = yaml.safe_load(f)
    cfg['dataset_config'] = _plain(mscnn_split.config(root))
    config_path = str(tmp_path / 'config.yaml')
    with open(config_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    capsys.readouterr()
    assert run_evaluation.main([config_path, '--checkpoint-dir', ckpts, '--mscnn-dir', mscnn, '--width-div', '8',
                                '--predictions-dir', str(tmp_path / 'scored'), '--shape-surface-metrics',
                                '--shape-surface-placed', '--shape-surface-thresholds', '0.1', '0.4',
                                '--shape-max-edge', '0.3']) == 0
    printed = capsys.readouterr().out
    assert printed.startswith('step 40\n')
    lines = [l for l in printed.splitlines() if l.startswith(('shape_', 'placed_'))]
    assert [l.split()[0] for l in lines] == list(_names((0.1, 0.4), 'shape_surface_') +
                                                 _names((0.1, 0.4), 'placed_surface_'))
    for kind, first in (('shape_surface', lines[0]), ('placed_surface', lines[13])):
        rows = open(os.path.join(str(tmp_path / 'scored'), 'metrics', 'val',
                                 '%s_metrics_val.csv' % kind)).read().splitlines()
        assert len(rows) == 2 and rows[1].split(',')[0].strip() == '40'
        assert int(rows[1].split(',')[1]) == int(first.split()[2])

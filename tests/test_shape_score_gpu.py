"""mpsr_shape_scores on the device against tests/shape_score_restatement.py over tests/shape_score_cases.py, then the
evaluator's shape_metrics end to end on the fixture split (the host side: tests/test_shape_score.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mscnn_split
import scene_score_restatement
import shape_score_calls as calls
import shape_score_cases as cases
import shape_score_restatement as restatement
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import distance_metrics as dm
from monopsr_amd.datasets.kitti import instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
OUTPUTS = ('counts', 'sums', 'table', 'dist_a', 'dist_b')


def _call(c, poison=False, offset=0, thresholds=None, workspace_short=0):
    """One mpsr_shape_scores call through the C entry point.  Every output sits `offset` elements into an allocation
    with a guard element behind it; poison fills outputs and workspace with NaN / 0xFF first (else with zeros).
    -> (status, {name: numpy array}, the guards' values afterwards)."""
    n, P, Q = c['a'].shape[0], c['a'].shape[1], c['b'].shape[1]
    thr = tuple(c['thresholds'] if thresholds is None else thresholds)
    T = len(thr)
    shapes = dict(counts=((n, 2 + 2 * T), torch.int32), sums=((n, 6), torch.float64),
                  table=((n, 5 + 3 * T), torch.float32), dist_a=((n, P), torch.float32), dist_b=((n, Q), torch.float32))
    lib = _lib.lib()
    need = int(lib.mpsr_shape_scores_workspace_bytes(n, P, Q, T))
    assert need % 8 == 0 and (need > 0) == (n > 0 and T <= dm.MAX_THRESHOLDS)

    def launch(inputs, out, ws):
        a, ma, b, mb = inputs
        return lib.mpsr_shape_scores(a, ma, P, b, mb, Q, n, (ctypes.c_double * max(T, 1))(*thr), T, ws,
                                     need - workspace_short, out['counts'], out['sums'], out['table'], out['dist_a'],
                                     out['dist_b'], _lib.stream())
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
    """counts, dist_a, dist_b and the two maxima bit for bit; the four sums within (m + 2) 2^-52 sum |term| (one ulp per
    root plus any summation order: restatement.sum_bound), bit for bit where every term is exact; the table from the
    device's own counts and sums, to a float32 neighbour."""
    c, want, got = cases.case(name), cases.restated(name), _result(device_results, name)
    T = len(c['thresholds'])
    for key in ('counts', 'dist_a', 'dist_b'):
        assert restatement.same_bits(got[key], want[key]), (name, key)
    assert restatement.same_bits(got['sums'][:, 4:6], want['sums'][:, 4:6]), name
    calls.assert_sums_within_the_bound(name, got['sums'], want, (0, 1, 2, 3) if name in cases.EXACT_SUM_NAMES else ())
    own = restatement.table(got['counts'], got['sums'], T)
    assert calls.neighbours(got['table'], own), name
    # NaN exactly where defined: the rows of an empty side, the points that are not valid
    empty = (want['counts'][:, 0] == 0) | (want['counts'][:, 1] == 0)
    assert np.array_equal(np.isnan(got['table']).all(1), empty) and np.array_equal(np.isnan(got['table']).any(1), empty)
    assert np.array_equal(np.isnan(got['sums']).all(1), empty) and np.array_equal(np.isnan(got['sums']).any(1), empty)
    assert (got['counts'][empty, 2:] == 0).all()
    assert np.isnan(got['dist_a'][empty]).all() and np.isnan(got['dist_b'][empty]).all()


@pytest.mark.parametrize('name', cases.NN_DISTANCE_NAMES)
def test_null_masks_give_nn_distance(device_results, name):
    from monopsr_amd.tf_ops.nn_distance import tf_nndistance
    c, got = cases.case(name), _result(device_results, name)
    assert c['mask_a'] is None and c['mask_b'] is None and np.isfinite(c['a']).all() and np.isfinite(c['b']).all()
    d1, _, d2, _ = tf_nndistance.nn_distance(torch.from_numpy(np.array(c['a'])).cuda(),
                                             torch.from_numpy(np.array(c['b'])).cuda())
    assert restatement.same_bits(got['dist_a'], d1.cpu().numpy()), name
    assert restatement.same_bits(got['dist_b'], d2.cpu().numpy()), name


@pytest.mark.parametrize('name', ('hostile', 'frame', 'empty_sides'))
def test_two_runs_poison_and_odd_offsets_return_the_same_bytes(device_results, name):
    """The same bytes from a second run, from zeroed instead of NaN / 0xFF-filled outputs and workspace, and from
    pointers one and three elements into larger allocations; the elements around every buffer keep their values."""
    first = calls.output_bytes(_result(device_results, name), OUTPUTS)
    for kw in (dict(poison=True), dict(poison=False), dict(poison=True, offset=1), dict(poison=False, offset=3)):
        status, out, _ = _call(cases.case(name), **kw)
        assert status == 0 and calls.output_bytes(out, OUTPUTS) == first, (name, kw)


def test_null_dist_pointers_and_empty_sizes():
    c = cases.case('many_boxes')
    want = cases.restated('many_boxes')
    up = lambda k: None if c[k] is None else torch.from_numpy(np.array(c[k])).cuda()
    s = dm.shape_scores(up('a'), up('b'), up('mask_a'), up('mask_b'), c['thresholds'])
    assert s.dist_a is None and s.dist_b is None and s.names == dm.shape_metric_names(c['thresholds'])
    assert restatement.same_bits(s.counts.cpu().numpy(), want['counts'])
    assert s.sums.dtype == torch.float64 and s.table.dtype == torch.float32 and s.counts.dtype == torch.int32
    # (n, h, w, 3) clouds, (n, h, w, 1) masks
    a4, m4 = up('a').reshape(33, 15, 17, 3), up('mask_a').reshape(33, 15, 17, 1)
    s4 = dm.shape_scores(a4, up('b'), m4, up('mask_b'), c['thresholds'], want_dists=True)
    assert torch.equal(s4.counts, s.counts) and torch.equal(s4.sums.view(torch.int64), s.sums.view(torch.int64))
    assert restatement.same_bits(s4.dist_a.cpu().numpy(), want['dist_a'])
    # P == 0 or Q == 0: the rows of an empty side; n == 0: nothing
    for a, b in ((up('a')[:3, :0], up('b')[:3]), (up('a')[:3], up('b')[:3, :0]), (up('a')[:3, :0], up('b')[:3, :0])):
        e = dm.shape_scores(a.contiguous(), b.contiguous(), thresholds=(0.5,), want_dists=True)
        assert e.counts.cpu().tolist() == [[int(a.shape[1]), int(b.shape[1]), 0, 0]] * 3
        assert bool(torch.isnan(e.sums).all()) and bool(torch.isnan(e.table).all()) and tuple(e.table.shape) == (3, 8)
        assert bool(torch.isnan(e.dist_a).all()) and bool(torch.isnan(e.dist_b).all())
    z = dm.shape_scores(up('a')[:0], up('b')[:0], thresholds=())
    assert tuple(z.counts.shape) == (0, 2) and tuple(z.table.shape) == (0, 5) and tuple(z.sums.shape) == (0, 6)
    with pytest.raises(_lib.InvalidArgumentError, match='one float32 entry per point'):
        dm.shape_scores(up('a'), up('b'), up('mask_b'))
    with pytest.raises(_lib.InvalidArgumentError, match='one float32 entry per point'):
        dm.shape_scores(up('a')[:1, :1], up('b')[:1, :1], torch.tensor(1.0, device='cuda'))  # a mask without a shape
    with pytest.raises(_lib.InvalidArgumentError, match='boxes'):
        dm.shape_scores(up('a'), up('b')[:5])
    with pytest.raises(_lib.InvalidArgumentError, match='not increasing'):
        dm.shape_scores(up('a'), up('b'), thresholds=(0.2, 0.1))


def test_more_work_items_than_the_grid_has_workgroups():
    """2^19 + 3 boxes of one point against one point are 2^20 + 6 work items, more than the 2^20 workgroups the search
    kernel is launched with at most: the last six are reached by the grid's stride, and the step past them must end the
    loop.  One point a side makes the restatement a line of numpy: d = the pair's distance, every sum one term."""
    n = (1 << 19) + 3
    rng = np.random.default_rng(21)
    a, b = (rng.standard_normal((n, 1, 3)).astype(np.float32) for _ in range(2))
    ma, mb = ((rng.uniform(size=(n, 1)) < 0.9).astype(np.float32) for _ in range(2))
    ma[-1], mb[-1], ma[-2], mb[-2], ma[-3] = 1.0, 1.0, 1.0, 1.0, 0.0  # the strided items: two whole boxes, an empty side
    t = 1.5
    status, got, _ = _call(dict(a=a, b=b, mask_a=ma, mask_b=mb, thresholds=(t,)), poison=True)
    assert status == 0, _lib.lib().mpsr_last_error()
    both = (ma[:, 0] > 0) & (mb[:, 0] > 0)
    delta = b[:, 0] - a[:, 0]
    d = (delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2]
    assert d.dtype == np.float32 and 0 < both.sum() < n
    want_d = np.where(both, d, np.float32(np.nan)).astype(np.float32)
    assert restatement.same_bits(got['dist_a'][:, 0], want_d) and restatement.same_bits(got['dist_b'][:, 0], want_d)
    within = (both & (d.astype(np.float64) <= t * t)).astype(np.int32)
    want_counts = np.stack([(ma[:, 0] > 0).astype(np.int32), (mb[:, 0] > 0).astype(np.int32), within, within], 1)
    assert np.array_equal(got['counts'], want_counts)
    d64 = np.where(both, d.astype(np.float64), np.nan)
    root = np.sqrt(d64)
    assert restatement.same_bits(got['sums'][:, [1, 3, 4, 5]], np.stack([d64] * 4, 1))
    for k in (0, 2):  # a sum of one term: the root itself, within the bound's three ulps
        err = np.abs(np.where(both, got['sums'][:, k] - root, 0.0))
        assert np.array_equal(np.isnan(got['sums'][:, k]), ~both)
        assert bool((err <= restatement.sum_bound(1, np.where(both, root, 0.0))).all())
    own = np.full((n, 8), np.nan)
    r0, r2 = got['sums'][:, 0], got['sums'][:, 2]
    hit = within.astype(np.float64)
    own[:, 0], own[:, 1], own[:, 2], own[:, 3], own[:, 4] = r0, r2, (r0 + r2) / 2, d64 + d64, np.sqrt(d64)
    own[:, 5], own[:, 6], own[:, 7] = hit, hit, hit  # p = r = 0 or 1: the F-score is 0 or 2 / 2
    own[~both] = np.nan
    assert calls.neighbours(got['table'], own.astype(np.float32))


def test_argument_errors_leave_the_outputs_untouched():
    c = cases.case('short')
    for kw, status, text in ((dict(thresholds=(0.5, 0.25)), 1, b'not increasing'),
                             (dict(thresholds=(float('nan'),)), 1, b'finite'),
                             (dict(thresholds=tuple(range(1, 10))), 1, b'outside'),
                             (dict(workspace_short=8), 3, b'workspace')):
        got, out, before = _call(c, poison=True, offset=1, **kw)
        assert got == status and text in _lib.lib().mpsr_last_error(), kw
        for k in OUTPUTS:
            assert np.isnan(out[k]).all() if out[k].dtype.kind == 'f' else (out[k] == -1).all(), (kw, k)


# ---- end to end: the fixture split, a small random-weight net (built as tests/test_scene_score_gpu.py's setup)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_shape_score')))
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
    host = lambda ts, width: torch.cat(ts).reshape(total, -1, width).cpu().numpy() if width else \
        torch.cat(ts).reshape(total, -1).cpu().numpy()
    return dict(
        local=host([o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n] for o, n in zip(outs, counts)], 3),
        placed=host([instance_utils.tf_inst_xyz_map_local_to_global(
            o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n], roi, o[constants.KEY_VIEW_ANG][0:n],
            o[constants.KEY_CENTROIDS][0:n]) for o, n in zip(outs, counts)], 3),
        gt_local=host([s['gt_inst_xyz_maps_local'][0:n] for s, n in zip(samples, counts)], 3),
        gt_global=host([s['gt_inst_xyz_maps_global'][0:n] for s, n in zip(samples, counts)], 3),
        mask=host([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)], 0))


def _restate_chunks(chunks, a, b, thresholds):
    parts = [restatement.shape_scores(c[a], c[b], c['mask'], c['mask'], thresholds) for c in chunks]
    return {k: np.concatenate([p[k] for p in parts]) for k in ('counts', 'sums', 'table', 'terms', 'abs_sums')}


def _assert_table_and_stats(kept, want, stats, names):
    """The evaluator's table (table, counts, sums, frame) against the restated chunks, and the statistics against
    mpsr_metric_stats' restatement (scene_score_restatement.stats) of the restated table."""
    table, counts, sums, frame = kept
    assert np.array_equal(counts.cpu().numpy(), want['counts']) and frame.numel() == len(want['counts'])
    assert restatement.same_bits(sums[:, 4:6].cpu().numpy(), want['sums'][:, 4:6])
    live = np.isfinite(want['sums'][:, 0:4])
    err = np.abs(np.where(live, sums[:, 0:4].cpu().numpy(), 0.0) - np.where(live, want['sums'][:, 0:4], 0.0))
    assert bool((err <= restatement.sum_bound(want['terms'], np.where(live, want['abs_sums'], 0.0))).all())
    assert calls.neighbours(table.cpu().numpy(), want['table'])
    want_stats = scene_score_restatement.stats(want['table'])
    assert list(stats) == list(names) and len(names) == want['table'].shape[1]
    # the statistics of the evaluator's OWN table: only fp64 summation order separates the two (numpy adds pairwise,
    # the kernel thread by thread), n 2^-53 sum |x| on a sum of n terms; 8 n 2^-53 (mean |x| + std |x|) covers the
    # mean, the centred squares and the root
    own_stats = scene_score_restatement.stats(table.cpu().numpy())
    for k, name in enumerate(names):
        assert stats[name]['count'] == int(own_stats[k, 0]), name
        tight = 8 * max(int(own_stats[k, 0]), 1) * 2.0 ** -53 * (own_stats[k, 3] + own_stats[k, 4])
        for j, key in enumerate(('mean', 'std', 'mean_abs', 'std_abs')):
            w = own_stats[k, 1 + j]
            assert np.isnan(stats[name][key]) if np.isnan(w) else abs(stats[name][key] - w) <= tight, (name, key)
    for k, name in enumerate(names):
        st = stats[name]
        assert st['count'] == int(want_stats[k, 0]) and st['dropped'] == len(want['counts']) - st['count'], name
        # every entry may sit on a float32 neighbour of the restated one, 2^-23 relative: the mean moves by at most
        # 2^-23 mean |x|, a standard deviation by at most 2^-23 sqrt(mean x^2) <= 2^-23 (mean |x| + std |x|)
        tol = 2.0 ** -22 * (want_stats[k, 3] + want_stats[k, 4])
        for j, key in enumerate(('mean', 'std', 'mean_abs', 'std_abs')):
            w = want_stats[k, 1 + j]
            assert np.isnan(st[key]) if np.isnan(w) else abs(st[key] - w) <= tol, (name, key, st[key], w)


@pytest.fixture(scope='module')
def unfitted(setup, tmp_path_factory):
    """Evaluator(shape_metrics={'placed': True}) next to a plain run: (plain result, scored result, the evaluator, the
    chunks' clouds, the directory)."""
    _, _, model, val, _ = setup
    base = tmp_path_factory.mktemp('shape_runs')
    plain = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(base / 'plain'), batch_size=2,
                                metric_stats=True).run_once(5)
    chunks = []
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(base / 'scored'), batch_size=2,
                             metric_stats=True, shape_metrics={'placed': True},
                             chunk_hook=lambda rows, samples, outs: chunks.append(_clouds_of_chunk(model, samples, outs)))
    scored = ev.run_once(5)
    return plain, scored, ev, chunks, base


def test_evaluator_shape_stats_equal_the_restatement(setup, unfitted):
    _, _, model, val, test = setup
    plain, scored, ev, chunks, base = unfitted
    assert len(chunks) == (val.num_samples + 1) // 2 >= 2
    thr = dm.DEFAULT_SHAPE_THRESHOLDS
    shape = _restate_chunks(chunks, 'local', 'gt_local', thr)
    placed = _restate_chunks(chunks, 'placed', 'gt_global', thr)
    assert len(shape['counts']) == scored['num_predictions'] and int((shape['counts'][:, :2] > 0).all(1).sum()) >= 4
    _assert_table_and_stats(ev.shape_table, shape, scored['shape_stats'], dm.shape_metric_names(thr, 'shape_'))
    _assert_table_and_stats(ev.placed_table, placed, scored['placed_stats'], dm.shape_metric_names(thr, 'placed_'))
    # both CSVs: a header and one line
    for kind, stats in (('shape', scored['shape_stats']), ('placed', scored['placed_stats'])):
        path = os.path.join(str(base / 'scored'), 'metrics', val.data_split, '%s_metrics_%s.csv' % (kind, val.data_split))
        assert scored[kind + '_metrics_csv'] == path
        lines = open(path).read().splitlines()
        assert len(lines) == 2 and lines[0].split(',')[0].strip() == 'step' and lines[1].split(',')[0].strip() == '5'
        fields = [c.strip() for c in lines[1].split(',')]
        assert len(fields) == 1 + 3 * 14 and fields[1] == '%d' % stats[kind + '_accuracy']['count']
        assert float(fields[2]) == float('%.5f' % stats[kind + '_accuracy']['mean'])
        assert not os.path.exists(path.replace(str(base / 'scored'), str(base / 'plain')))
    # everything else is what it is without shape_metrics
    calls.same_elsewhere(plain, scored, {'shape_stats', 'placed_stats', 'shape_metrics_csv', 'placed_metrics_csv'}, val)
    assert 'shape_stats' not in plain
    with pytest.raises(ValueError):
        evaluator.Evaluator(model, test, THRESHOLD, shape_metrics={})


def test_evaluator_fitted_centroids_and_breakdown(setup, unfitted, tmp_path):
    """With centroid_fit the shape_* table keeps its bits and the placed_* table comes from the fitted centroids; with
    breakdown the kinds 'shape' and 'placed' appear and their slot over every row holds the unbinned statistics."""
    _, _, model, val, _ = setup
    _, _, ev0, chunks0, _ = unfitted
    chunks = []
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path), batch_size=2,
                             shape_metrics={'placed': True, 'thresholds': (0.1, 0.5)}, centroid_fit={}, breakdown={},
                             chunk_hook=lambda rows, samples, outs: chunks.append(_clouds_of_chunk(model, samples, outs)))
    result = ev.run_once(6)
    thr = (0.1, 0.5)
    # the object's own frame: the first five columns, the counts of valid points and the sums are the unfitted run's
    for k in range(len(chunks)):
        assert np.array_equal(chunks[k]['local'], chunks0[k]['local'])
    assert torch.equal(ev.shape_table[0][:, :5].view(torch.int32), ev0.shape_table[0][:, :5].view(torch.int32))
    assert torch.equal(ev.shape_table[1][:, :2], ev0.shape_table[1][:, :2])
    assert torch.equal(ev.shape_table[2].view(torch.int64), ev0.shape_table[2].view(torch.int64))
    # placed: from the fitted centroids, which the hook saw
    placed = _restate_chunks(chunks, 'placed', 'gt_global', thr)
    _assert_table_and_stats(ev.placed_table, placed, result['placed_stats'], dm.shape_metric_names(thr, 'placed_'))
    fit = result['centroid_fit']
    assert fit['converged'] + fit['capped'] > 0  # the fixture has boxes that are fitted: what follows is not vacuous
    moved = any(not np.array_equal(c['placed'], c0['placed']) for c, c0 in zip(chunks, chunks0))
    assert moved and not torch.equal(ev.placed_table[2].view(torch.int64), ev0.placed_table[2].view(torch.int64))
    # the breakdown's kinds, and slot 0
    bd = result['breakdown']
    assert {'object', 'shape', 'placed'} <= set(bd['all']) and {'shape', 'placed'} <= set(bd['tables'])
    for kind in ('shape', 'placed'):
        assert repr(bd['all'][kind]) == repr(result[kind + '_stats']), kind
        assert set(bd['tables'][kind]) == {'depth', 'difficulty', 'fed_box'}
    text = open(result['breakdown_csv']).read()
    assert ',shape,all,all,shape_accuracy,' in text and ',placed,depth,' in text


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


def test_run_evaluation_shape_metrics_command_line(setup, tmp_path, capsys):
    """--shape-metrics --shape-placed on the fixture split and one saved checkpoint: the shape and placed lines after
    the report, in shape_metric_names' order, and one line in each CSV."""
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
                                '--predictions-dir', str(tmp_path / 'scored'), '--shape-metrics', '--shape-placed',
                                '--shape-thresholds', '0.1', '0.4']) == 0
    printed = capsys.readouterr().out
    assert printed.startswith('step 40\n')
    lines = [l for l in printed.splitlines() if l.startswith(('shape_', 'placed_'))]
    assert [l.split()[0] for l in lines] == list(dm.shape_metric_names((0.1, 0.4), 'shape_') +
                                                 dm.shape_metric_names((0.1, 0.4), 'placed_'))
    for kind, first in (('shape', lines[0]), ('placed', lines[11])):
        rows = open(os.path.join(str(tmp_path / 'scored'), 'metrics', 'val', '%s_metrics_val.csv' % kind)).read().splitlines()
        assert len(rows) == 2 and rows[1].split(',')[0].strip() == '40'
        assert int(rows[1].split(',')[1]) == int(first.split()[2])

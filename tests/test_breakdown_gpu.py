"""mpsr_object_pairs and mpsr_metric_stats_binned on the device against tests/breakdown_restatement.py and numpy, the
functions of core/evaluation.py against the reference's recorded IoUs, and the Evaluator's breakdown on the fixture
split."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import breakdown_cases as C  # noqa: E402
import breakdown_restatement as BR  # noqa: E402
import mscnn_split  # noqa: E402
import test_kitti_eval as R  # noqa: E402  (golden())

from monopsr_amd import _lib  # noqa: E402
from monopsr_amd.core import config_utils, constants, evaluation, evaluator, evaluator_utils  # noqa: E402
from monopsr_amd.datasets.kitti import instance_utils, kitti_dataset, obj_utils  # noqa: E402

pytestmark = pytest.mark.gpu

IOU_TOL, DIST_RTOL = 1e-12, 1e-12          # tests/test_kitti_eval_gpu.py holds 1e-12 for this arithmetic
RASTER_BOUND_3D = 0.02                      # tests/test_kitti_eval_gpu.py
MEAN_TOL, STD_RTOL = 1e-10, 1e-9            # tests/test_metric_stats_gpu.py
THRESHOLD, BATCH = 0.1, 2


# ---- mpsr_object_pairs

@pytest.fixture(scope='module')
def cat():
    c = C.catalogue()
    c['restated'] = BR.object_pairs(c['pred'], c['gt'], c['fed'], c['info'], C.DEPTH_EDGES, C.BOX_IOU_EDGES)
    return c


def _pairs(pred, gt, fed, info, fill):
    """The entry point itself on buffers pre-filled with the byte `fill` -> host (overlaps, table, bins)."""
    n = len(pred)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    p, g, f, i = up(pred), up(gt), up(fed), up(info)
    raw = lambda nbytes: torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device='cuda')
    ov, tb, bn = raw(n * 32), raw(n * 36), raw(n * 12)
    dbl = lambda v: (ctypes.c_double * max(len(v), 1))(*v)
    _lib.check(_lib.lib().mpsr_object_pairs(
        _lib.ptr(p), _lib.ptr(g), _lib.ptr(f), _lib.ptr(i), n, dbl(C.DEPTH_EDGES), len(C.DEPTH_EDGES),
        dbl(C.BOX_IOU_EDGES), len(C.BOX_IOU_EDGES), ov.data_ptr(), tb.data_ptr(), bn.data_ptr(), _lib.stream()))
    torch.cuda.synchronize()
    return (ov[:n * 32].view(torch.float64).reshape(n, 4).cpu().numpy(),
            tb[:n * 36].view(torch.float32).reshape(n, 9).cpu().numpy(),
            bn[:n * 12].view(torch.int32).reshape(n, 3).cpu().numpy())


def _compare_pairs(got, want, what):
    (ov, tb, bn), (wov, wtb, wbn) = got, want
    assert np.array_equal(np.isnan(ov), np.isnan(wov)), what
    ok = ~np.isnan(wov)
    diff = np.abs(np.where(ok, ov - wov, 0.0))
    print('object_pairs %s: largest IoU difference %.3g, centre distance %.3g relative' % (
        what, diff[:, 0:3].max(initial=0.0), (diff[:, 3] / np.where(ok[:, 3], np.maximum(wov[:, 3], 1e-300), 1.0)).max(initial=0.0)))
    assert (diff[:, 0:3] <= IOU_TOL).all(), what
    assert (diff[:, 3] <= DIST_RTOL * np.where(ok[:, 3], wov[:, 3], 0.0)).all(), what
    assert np.array_equal(bn, wbn), what
    assert np.array_equal(tb[:, 4:9], wtb[:, 4:9], equal_nan=True), what
    # the table is the float32 rounding of the device's own overlaps
    assert np.array_equal(tb[:, 0:4], ov.astype(np.float32), equal_nan=True), what


@pytest.mark.parametrize('n', C.SIZES)
def test_object_pairs_catalogue(cat, n):
    """Largest differences seen on an MI355X over the six sizes: IoUs 4.9e-15 from the restatement's (bound 1e-12),
    centre distances equal to it; bins and hits exact."""
    assert C.margin_of(cat['restated'][0]) > C.MARGIN  # no IoU near a value that decides a hit or a bin
    args = [cat[k][:n] for k in ('pred', 'gt', 'fed', 'info')]
    want = tuple(a[:n] for a in cat['restated'])
    got = _pairs(*args, fill=0xFF)
    _compare_pairs(got, want, n)
    again = _pairs(*args, fill=0x00)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes(), n
    if n == max(C.SIZES):
        rows = cat['rows']
        ov = got[0]
        assert abs(ov[rows['identical'], 1] - 1) <= IOU_TOL and abs(ov[rows['identical'], 2] - 1) <= IOU_TOL
        assert abs(ov[rows['half_length'], 2] - 1 / 3) <= 1e-7  # (float32 inputs)
        assert ov[rows['corner_touching'], 1] == 0 and ov[rows['stacked'], 2] == 0 and ov[rows['stacked'], 1] > 0
        assert abs(ov[rows['turn_3'], 1] - 1) <= 1e-6 and ov[rows['contained'], 1] > 0 and ov[rows['far'], 2] > 0
        assert got[2][rows['on_depth_edge']:rows['on_depth_edge'] + 3, 0].tolist() == [1, 2, 5]
        a = rows['difficulty']
        assert got[2][a:a + len(C.DIFFICULTY), 1].tolist() == [w for _, w in C.DIFFICULTY]


@pytest.mark.parametrize('without', ['fed', 'info', 'both'])
def test_object_pairs_null_pointers(cat, without):
    n = 65
    fed = None if without in ('fed', 'both') else cat['fed'][:n]
    info = None if without in ('info', 'both') else cat['info'][:n]
    want = BR.object_pairs(cat['pred'][:n], cat['gt'][:n], fed, info, C.DEPTH_EDGES, C.BOX_IOU_EDGES)
    got = _pairs(cat['pred'][:n], cat['gt'][:n], fed, info, fill=0xFF)
    _compare_pairs(got, want, without)
    assert np.isnan(got[0][:, 0]).all() and np.isnan(got[1][:, 0]).all() and (got[2][:, 2] == -1).all()
    assert (got[2][:, 1] == -1).all() == (info is None)


def test_object_pairs_wrapper(cat):
    up = lambda k: torch.from_numpy(cat[k]).cuda()
    pred9 = torch.cat([up('pred'), torch.ones((257, 2), device='cuda')], 1)  # format_boxes' (n, 9): two more columns
    table, overlaps, bins = evaluator_utils.object_pairs(pred9, up('gt'), up('fed'), up('info'))
    assert table.dtype == torch.float32 and overlaps.dtype == torch.float64 and bins.dtype == torch.int32
    _compare_pairs((overlaps.cpu().numpy(), table.cpu().numpy(), bins.cpu().numpy()), cat['restated'], 'wrapper')
    t2, o2, b2 = evaluation.paired_overlaps(up('pred'), up('gt'), up('fed'), up('info'))
    assert torch.equal(o2.view(torch.int64), overlaps.view(torch.int64)) and torch.equal(b2, bins)
    empty = evaluator_utils.object_pairs(pred9[:0], up('gt')[:0])
    assert [tuple(t.shape) for t in empty] == [(0, 9), (0, 4), (0, 3)]


# ---- mpsr_metric_stats_binned

def _oracle(values, rows):
    out = np.zeros((C.N_METRICS, 6))
    for m in range(C.N_METRICS):
        x = values[rows][:, [c for c, k in enumerate(C.COLUMN_METRIC) if k == m]].astype(np.float64).reshape(-1)
        kept = x[~np.isnan(x)]
        out[m, 0], out[m, 5] = kept.size, x.size - kept.size
        out[m, 1:5] = (kept.mean(), kept.std(), np.abs(kept).mean(), np.abs(kept).std()) if kept.size else np.nan
    return out


def _compare_stats(got, want, what):
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg='count, %s' % (what,))
    np.testing.assert_array_equal(got[:, 5], want[:, 5], err_msg='dropped, %s' % (what,))
    empty = want[:, 0] == 0
    assert np.isnan(got[empty, 1:5]).all() and not np.isnan(got[~empty, 1:5]).any(), what
    g, w = got[~empty], want[~empty]
    assert (np.abs(g[:, 1] - w[:, 1]) <= MEAN_TOL * w[:, 3]).all(), what
    assert (np.abs(g[:, 3] - w[:, 3]) <= MEAN_TOL * w[:, 3]).all(), what
    np.testing.assert_allclose(g[:, 2], w[:, 2], rtol=STD_RTOL, atol=0, err_msg=str(what))
    np.testing.assert_allclose(g[:, 4], w[:, 4], rtol=STD_RTOL, atol=0, err_msg=str(what))


@pytest.mark.parametrize('n_rows,axis_bins,placement', C.STATS_CASES)
def test_binned_statistics(n_rows, axis_bins, placement):
    values = C.place_nans(C.stats_table(n_rows, 2000 + n_rows), placement)
    bins = C.stats_bins(n_rows, axis_bins, 3000 + n_rows)
    v, b = torch.from_numpy(values).cuda(), torch.from_numpy(bins).cuda()
    n_slots = 1 + sum(axis_bins)
    out = torch.full((n_slots, C.N_METRICS, 6), float('nan'), dtype=torch.float64, device='cuda')
    assert evaluator_utils.metric_stats_binned(v, b, C.COLUMN_METRIC, C.N_METRICS, axis_bins, out=out) is out
    got = out.cpu().numpy()
    assert not np.isnan(got[:, :, [0, 5]]).any()
    # slot 0: the bytes of mpsr_metric_stats under the entry rule
    frame = torch.zeros(n_rows, dtype=torch.int32, device='cuda')
    plain = evaluator_utils.metric_stats(v, frame, C.COLUMN_METRIC, C.N_METRICS, 1, evaluator_utils.NAN_RULE_ENTRY)
    assert got[0].tobytes() == plain.cpu().numpy().tobytes()
    slots = BR.slots_of(bins, axis_bins)
    assert len(slots) == n_slots
    for s, rows in enumerate(slots):
        _compare_stats(got[s], _oracle(values, rows), (n_rows, axis_bins, placement, s))
    for a, nb in enumerate(axis_bins):
        first = 1 + sum(axis_bins[:a])
        outside = int(((bins[:, a] < 0) | (bins[:, a] >= nb)).sum())
        for m in range(C.N_METRICS):
            width = C.COLUMN_METRIC.count(m)
            assert (got[first:first + nb, m, [0, 5]].sum() + outside * width == got[0, m, [0, 5]].sum()
                    == n_rows * width), (a, m)
        if nb >= 2:
            assert got[first + nb - 1, 0, 0] == 0 and np.isnan(got[first + nb - 1, 0, 1:5]).all()  # the empty bin
    again = evaluator_utils.metric_stats_binned(v, b, C.COLUMN_METRIC, C.N_METRICS, axis_bins).cpu().numpy()
    assert got.tobytes() == again.tobytes()
    zeros = torch.zeros_like(out)
    evaluator_utils.metric_stats_binned(v, b, C.COLUMN_METRIC, C.N_METRICS, axis_bins, out=zeros)
    assert zeros.cpu().numpy().tobytes() == got.tobytes()


# ---- core/evaluation.py against the reference's recorded values

def test_evaluation_against_the_reference_pins():
    g = R.golden()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a2, b2 = g['pin2d_a'], g['pin2d_b']
    got = np.empty(len(a2))
    k = 0
    while k < len(a2):  # runs of one box against the boxes recorded with it
        e = k
        while e < len(a2) and np.array_equal(a2[e], a2[k]):
            e += 1
        got[k:e] = evaluation.two_d_iou(dev(a2[k]), dev(b2[k:e])).cpu().numpy()
        k = e
    assert np.abs(got - g['pin2d_iou']).max() <= 1e-12
    a3, b3 = g['pin3d_a'], g['pin3d_b']
    got3, bev = np.empty(len(a3)), np.empty(len(a3))
    k = 0
    while k < len(a3):
        e = k
        while e < len(a3) and np.array_equal(a3[e], a3[k]):
            e += 1
        got3[k:e] = evaluation.three_d_iou(dev(a3[k]), dev(b3[k:e])).cpu().numpy()
        bev[k:e] = evaluation.bev_iou(dev(a3[k]), dev(b3[k:e])).cpu().numpy()
        k = e
    print('three_d_iou against the 174 pins: largest difference %.4f' % np.abs(got3 - g['pin3d_iou']).max())
    assert len(got3) == 174 and np.abs(got3 - g['pin3d_iou']).max() <= RASTER_BOUND_3D
    assert (bev >= got3 - 1e-12).all() and (got3 > 0).sum() >= 150
    # float32 boxes are widened without loss, and a single box gives one value
    one = evaluation.three_d_iou(dev(a3[0].astype(np.float32)), dev(b3[0].astype(np.float32)))
    order = [4, 5, 6, 1, 3, 2, 0]
    want = BR.box_overlaps(a3[0].astype(np.float32)[order], b3[0].astype(np.float32)[order])[1]
    assert tuple(one.shape) == (1,) and abs(float(one[0]) - want) <= 1e-12
    m1 = torch.zeros((4, 6), dtype=torch.uint8, device='cuda')
    m2 = torch.zeros((4, 6), dtype=torch.bool, device='cuda')
    m1[0:2], m2[1:4] = 1, True
    assert float(evaluation.mask_iou(m1, m2)) == 6 / 24


# ---- the Evaluator on the fixture split

@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_breakdown')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    ds = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    resident = ds.resident_bytes
    common = dict(batch_size=BATCH, metric_stats=True, scene_metrics=True)
    plain = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=str(tmp_path_factory.mktemp('plain')),
                                **common).run_once(7)
    assert ds.resident_bytes == resident  # the label table is uploaded when the breakdown first asks for it
    out = str(tmp_path_factory.mktemp('breakdown_out'))
    ev = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=out, breakdown={}, **common)
    return dict(model=model, ds=ds, ev=ev, result=ev.run_once(7), plain=plain, out=out, resident=resident)


def test_frame_label_info_is_the_label_files_rows(setup):
    ds = setup['ds']
    n = int(ds._num_objs_host.sum())
    assert ds.resident_bytes == setup['resident'] + n * 6 * 4
    info = ds.frame_label_info(np.arange(ds.num_samples))
    assert ds.resident_bytes == setup['resident'] + n * 6 * 4  # (uploaded once)
    truth = ds.frame_ground_truth(np.arange(ds.num_samples))
    samples = ds.get_sample_dict(np.argsort(np.asarray(ds.sample_list), kind='stable'), epoch=0)
    replaced = 0
    for r, name in enumerate(ds.sample_names):
        labels = obj_utils.read_labels(ds.kitti_label_dir, name)[truth[r]['instance_ids'].cpu().numpy()]
        want = np.asarray([[o.truncation, o.occlusion, o.x1, o.y1, o.x2, o.y2] for o in labels], np.float32)
        got = info[r].cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want.reshape(-1, 6)), name
        fed = samples[r]['boxes_2d'][:len(labels)].cpu().numpy()
        replaced += int((np.abs(fed[:, [1, 0, 3, 2]] - got[:, 2:6]).max(axis=1) > 0).sum())
    assert replaced > 0  # the merged labels carry MSCNN's boxes: frame_label_info does not
    with pytest.raises(IndexError):
        ds.frame_label_info([ds.num_samples])
    assert set(samples[0]) == set(ds.get_sample_dict([0], epoch=0)[0])


def _host_slot_stats(values, rows):
    x = values[rows].astype(np.float64).reshape(-1)
    kept = x[~np.isnan(x)]
    if not kept.size:
        return dict(count=0, dropped=int(x.size))
    return dict(count=int(kept.size), dropped=int(x.size - kept.size), mean=kept.mean(), std=kept.std(),
                mean_abs=np.abs(kept).mean(), std_abs=np.abs(kept).std())


def test_evaluator_breakdown_against_the_host(setup):
    from monopsr_amd.core.scene_reconstruction import SCENE_METRIC_NAMES
    ev, result = setup['ev'], setup['result']
    table, overlaps, bins, frame = ev.pair_table
    n = result['num_predictions']
    assert tuple(table.shape) == (n, 9) and tuple(overlaps.shape) == (n, 4) and tuple(bins.shape) == (n, 3)
    assert torch.equal(frame, ev.metric_table[1]) and n == 9
    bins_h = bins.cpu().numpy()
    b = result['breakdown']
    axes = b['axes']
    assert list(axes) == list(evaluator_utils.BREAKDOWN_AXES)
    assert axes['depth'] == ['<10', '10-20', '20-30', '30-40', '40-50', '>=50']
    assert axes['difficulty'] == list(evaluator_utils.DIFFICULTY_LABELS)
    assert axes['fed_box'] == ['<0.7', '0.7-0.8', '0.8-0.9', '>=0.9']
    tables = dict(object=(evaluator_utils.PAIR_COLUMNS, table.cpu().numpy(), list(range(9))),
                  metrics=(evaluator.METRIC_NAMES, ev.metric_table[0].cpu().numpy(), list(evaluator.COLUMN_METRIC)),
                  scene=(SCENE_METRIC_NAMES, ev.scene_table[0].cpu().numpy(), list(range(len(SCENE_METRIC_NAMES)))))
    assert set(b['tables']) == set(b['all']) == set(tables)
    checked = 0
    for kind, (names, values, column_metric) in tables.items():
        for m, name in enumerate(names):
            cols = [c for c, k in enumerate(column_metric) if k == m]
            slots = [('all', 'all', np.ones(n, bool), b['all'][kind][name])]
            for a, axis in enumerate(evaluator_utils.BREAKDOWN_AXES):
                assert list(b['tables'][kind][axis]) == axes[axis]
                slots += [(axis, label, bins_h[:, a] == k, b['tables'][kind][axis][label][name])
                          for k, label in enumerate(axes[axis])]
            for axis, label, rows, got in slots:
                want = _host_slot_stats(values[:, cols], rows)
                assert got['count'] == want['count'] and got['dropped'] == want['dropped'], (kind, name, axis, label)
                if not want['count']:
                    assert all(np.isnan(got[k]) for k in ('mean', 'std', 'mean_abs', 'std_abs'))
                    continue
                checked += 1
                assert abs(got['mean'] - want['mean']) <= MEAN_TOL * want['mean_abs']
                assert abs(got['mean_abs'] - want['mean_abs']) <= MEAN_TOL * want['mean_abs']
                np.testing.assert_allclose([got['std'], got['std_abs']], [want['std'], want['std_abs']],
                                           rtol=STD_RTOL, atol=0, err_msg=str((kind, name, axis, label)))
    assert checked > 3 * 9
    # the scene table's overall statistics are the ones scene_metrics reports (the entry rule both times)
    assert _same(b['all']['scene'], result['scene_stats'])
    # the label's depth and the fed boxes of this split fall into more than one bin
    assert len(set(bins_h[:, 0].tolist())) > 1 and (bins_h >= 0).all()


def test_pair_table_rows_are_the_restatements(setup):
    """The pair table against the restatement on the boxes the pass wrote into its label files' source: format_boxes of
    each frame, the samples' boxes and frame_label_info."""
    ev, ds, model = setup['ev'], setup['ds'], setup['model']
    table, overlaps, bins, frame = ev.pair_table
    want = _restated_pass(model, ds, None)
    _compare_pairs((overlaps.cpu().numpy(), table.cpu().numpy(), bins.cpu().numpy()), want, 'evaluator')


def _restated_pass(model, ds, centroid_fit):
    from monopsr_amd.core.instances import instance_metrics
    pred, gt, fed, info = [], [], [], []
    position = np.argsort(np.asarray(ds.sample_list), kind='stable')
    with torch.no_grad():
        for a in range(0, ds.num_samples, BATCH):
            rows = np.arange(a, min(a + BATCH, ds.num_samples))
            samples = ds.get_sample_dict(position[rows], epoch=0)
            outs = model.build_batch(samples)
            if centroid_fit is not None:
                outs, _ = instance_metrics.fit_centroids(model, samples, outs, **centroid_fit)
            for s, o, i in zip(samples, outs, ds.frame_label_info(rows)):
                n = int(s['num_objs'])
                b3, _ = instance_utils.format_boxes(
                    o[constants.KEY_LWH], o[constants.KEY_VIEW_ANG], o[constants.KEY_ALPHA_BINS],
                    o[constants.KEY_ALPHA_REGS], o[constants.KEY_CENTROIDS], s['boxes_2d'], s['label_scores'],
                    s['class_indices'], s['cam_p'], s['rgb_image'].shape, centroid_type=model.centroid_type,
                    post_process_cen_x=model.post_process_cen_x)
                pred.append(b3[0:n, 0:7].cpu().numpy())
                gt.append(s['boxes_3d'][0:n].cpu().numpy())
                fed.append(s['boxes_2d'][0:n].cpu().numpy())
                info.append(i.cpu().numpy())
    cat = lambda parts: np.concatenate(parts).astype(np.float32)
    return BR.object_pairs(cat(pred), cat(gt), cat(fed), cat(info), C.DEPTH_EDGES, C.BOX_IOU_EDGES)


def test_with_centroid_fit_the_pair_table_holds_the_fitted_boxes(setup):
    model, ds = setup['model'], setup['ds']
    ev = evaluator.Evaluator(model, ds, THRESHOLD, batch_size=BATCH, compute_metrics=False, compute_losses=False,
                             centroid_fit={}, breakdown={})
    result = ev.run_once(7)
    table, overlaps, bins, frame = ev.pair_table
    fitted = _restated_pass(model, ds, {})
    _compare_pairs((overlaps.cpu().numpy(), table.cpu().numpy(), bins.cpu().numpy()), fitted, 'fitted')
    assert result['centroid_fit']['converged'] + result['centroid_fit']['capped'] > 0
    unfitted = setup['ev'].pair_table[1].cpu().numpy()
    assert not np.array_equal(unfitted[:, 3], overlaps.cpu().numpy()[:, 3])  # the centre distances moved
    assert set(result['breakdown']['tables']) == {'object'}


def test_breakdown_csv_has_one_line_per_table_axis_bin_and_metric(setup):
    from monopsr_amd.core.scene_reconstruction import SCENE_METRIC_NAMES
    result, out = setup['result'], setup['out']
    path = os.path.join(out, 'metrics', 'val', 'breakdown_val.csv')
    assert result['breakdown_csv'] == path
    with open(path, newline='') as f:
        lines = f.read().split('\r\n')
    assert lines[-1] == '' and lines[0] == ','.join(evaluator_utils.BREAKDOWN_HEADER)
    fields = [line.split(',') for line in lines[1:-1]]
    n_metrics = dict(object=9, metrics=len(evaluator.METRIC_NAMES), scene=len(SCENE_METRIC_NAMES))
    assert len(fields) == (1 + 6 + 4 + 4) * sum(n_metrics.values())
    keys = [tuple(f[1:5]) for f in fields]
    assert len(set(keys)) == len(keys) and all(f[0] == '7' and len(f) == 11 for f in fields)
    b = result['breakdown']
    for f in fields:
        st = b['all'][f[1]][f[4]] if f[2] == 'all' else b['tables'][f[1]][f[2]][f[3]][f[4]]
        assert f[5:] == ['%d' % st['count']] + ['%.5f' % st[k] for k in ('mean', 'std', 'mean_abs', 'std_abs')] + \
            ['%d' % st['dropped']], f


def test_breakdown_adds_two_keys_and_nothing_else(setup):
    plain, result = setup['plain'], setup['result']
    assert set(result) - set(plain) == {'breakdown', 'breakdown_csv'} and set(plain) <= set(result)
    for key in ('report', 'metrics', 'losses', 'metric_stats', 'scene_stats', 'num_detections', 'num_predictions'):
        assert _same(plain[key], result[key]), key
    assert not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(plain['metrics_csv'][0])), 'val',
                                           'breakdown_val.csv'))


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, float) and a != a:
        return b != b
    return a == b

"""mpsr_metric_stats against numpy on float64 copies, and the Evaluator's metric table and CSVs on the fixture split."""
import os

import numpy as np
import pytest
import torch

import mscnn_split
from monopsr_amd.core import config_utils, constants, evaluator, evaluator_utils
from monopsr_amd.datasets.kitti import kitti_dataset

pytestmark = pytest.mark.gpu

COLS = evaluator.COLUMN_METRIC
N_METRICS = len(evaluator.METRIC_NAMES)
THRESHOLD = 0.1
BATCH = 2
# fp64 summation of n <= 2^18 values: n * eps ~ 3e-11, with a small margin
MEAN_TOL, STD_RTOL = 1e-10, 1e-9


def _table(n_rows, seed):
    """Unit normals times per-column scales of 0.01 .. 100 plus offsets of the same order (std is not small against
    the mean: the two-pass bound applies); frames in runs of 1 .. 32 rows."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.uniform(-2, 2, len(COLS))
    offset = scale * rng.uniform(-2, 2, len(COLS))
    values = (rng.standard_normal((n_rows, len(COLS))) * scale + offset).astype(np.float32)
    runs = []
    while sum(runs) < n_rows:
        runs.append(int(rng.integers(1, 33)))
    frame = np.repeat(np.arange(len(runs)), runs)[:n_rows].astype(np.int32)
    return values, frame, max(len(runs), 1)


def _place_nans(values, frame, placement):
    v = values.copy()
    n = len(v)
    if placement == 'none' or n == 0:
        return v
    if placement == 'single':       # one NaN in a single-column metric
        v[n // 2, 4] = np.nan
    elif placement == 'dim':        # one NaN in one of the three dimension columns
        v[n // 3, 8] = np.nan
    elif placement == 'all':        # every frame holds a NaN in one metric: the first row of each frame
        first = np.r_[True, frame[1:] != frame[:-1]]
        v[first, 2] = np.nan
    return v


def _oracle(values, frame, rule):
    """(n_metrics, 6) from numpy on float64 copies, after applying the rule in plain Python."""
    out = np.zeros((N_METRICS, 6))
    for m in range(N_METRICS):
        sub = values[:, [c for c, k in enumerate(COLS) if k == m]].astype(np.float64)
        if rule == 1:
            bad = set(frame[np.isnan(sub).any(axis=1)].tolist())
            keep = np.array([f not in bad for f in frame.tolist()], bool).reshape(-1)
            kept = sub[keep].reshape(-1)
        else:
            kept = sub.reshape(-1)
            kept = kept[~np.isnan(kept)]
        out[m, 0], out[m, 5] = kept.size, sub.size - kept.size
        out[m, 1:5] = (kept.mean(), kept.std(), np.abs(kept).mean(), np.abs(kept).std()) if kept.size else np.nan
    return out


_worst = {'mean': 0.0, 'mean_abs': 0.0, 'std': 0.0, 'std_abs': 0.0}


def _compare(got, want, what):
    assert got.shape == want.shape == (N_METRICS, 6)
    assert not np.isnan(got[:, [0, 5]]).any(), what
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg='count, %s' % (what,))
    np.testing.assert_array_equal(got[:, 5], want[:, 5], err_msg='dropped, %s' % (what,))
    empty = want[:, 0] == 0
    assert np.isnan(got[empty, 1:5]).all() and not np.isnan(got[~empty, 1:5]).any(), what
    g, w = got[~empty], want[~empty]
    dev = dict(mean=np.abs(g[:, 1] - w[:, 1]) / w[:, 3], mean_abs=np.abs(g[:, 3] - w[:, 3]) / w[:, 3],
               std=np.abs(g[:, 2] - w[:, 2]) / np.where(w[:, 2] > 0, w[:, 2], 1.0),
               std_abs=np.abs(g[:, 4] - w[:, 4]) / np.where(w[:, 4] > 0, w[:, 4], 1.0))
    for k, d in dev.items():
        if d.size:
            _worst[k] = max(_worst[k], float(d.max()))
    print('metric_stats %s: worst relative deviations so far %s' % (what, _worst))
    assert (np.abs(g[:, 1] - w[:, 1]) <= MEAN_TOL * w[:, 3]).all(), what
    assert (np.abs(g[:, 3] - w[:, 3]) <= MEAN_TOL * w[:, 3]).all(), what
    np.testing.assert_allclose(g[:, 2], w[:, 2], rtol=STD_RTOL, atol=0, err_msg=str(what))
    np.testing.assert_allclose(g[:, 4], w[:, 4], rtol=STD_RTOL, atol=0, err_msg=str(what))


def _run(values, frame, n_frames, rule):
    stats = torch.full((N_METRICS, 6), float('nan'), dtype=torch.float64, device='cuda')
    v, f = torch.from_numpy(values).cuda(), torch.from_numpy(frame).cuda()
    out = evaluator_utils.metric_stats(v, f, COLS, N_METRICS, n_frames, rule, out=stats)
    assert out is stats
    return stats.cpu().numpy()


# (an empty table has no place for a NaN)
CASES = [(n, p) for n in (0, 1, 63, 64, 65, 257, 70001) for p in ('none', 'single', 'dim', 'all') if n or p == 'none']


@pytest.mark.parametrize('n_rows,placement', CASES)
def test_kernel_against_numpy(n_rows, placement):
    """Both rules, every output element written over a NaN pre-fill, two calls bit-identical, and the rows of a frame
    given non-contiguously (a permutation of the table).
    Largest deviations seen on an MI355X over all 25 cases, both rules and the permutations: mean 1.8e-16 and
    mean_abs 4.3e-16 of mean_abs (bound 1e-10); std 4.1e-16 and std_abs 2.2e-16 relative (bound 1e-9)."""
    values, frame, n_frames = _table(n_rows, 1000 + n_rows)
    values = _place_nans(values, frame, placement)
    rng = np.random.default_rng(7)
    for rule in (1, 0):
        want = _oracle(values, frame, rule)
        got = _run(values, frame, n_frames, rule)
        _compare(got, want, (n_rows, placement, rule))
        again = _run(values, frame, n_frames, rule)
        assert got.tobytes() == again.tobytes(), (n_rows, placement, rule)
        perm = rng.permutation(n_rows)
        _compare(_run(values[perm], frame[perm], n_frames, rule), want, (n_rows, placement, rule, 'permuted'))
        if placement == 'dim' and n_rows:
            # the frame of the NaN: its rows' other two dimension columns drop under rule 1 and stay under rule 0
            rows_of_frame = int((frame == frame[n_rows // 3]).sum())
            assert want[7, 5] == (3 * rows_of_frame if rule == 1 else 1)
        if placement == 'all' and n_rows and rule == 1:
            assert want[2, 0] == 0 and want[2, 5] == n_rows and np.isnan(got[2, 1:5]).all()


def test_wrapper_checks():
    v = torch.zeros((4, 10), device='cuda')
    f = torch.zeros(4, dtype=torch.int32, device='cuda')
    from monopsr_amd import _lib
    with pytest.raises(_lib.InvalidArgumentError, match='nan_rule'):
        evaluator_utils.metric_stats(v, f, COLS, N_METRICS, 1, nan_rule=2)
    with pytest.raises(_lib.InvalidArgumentError, match='column_metric'):
        evaluator_utils.metric_stats(v, f, [0] * 9 + [8], N_METRICS, 1)
    with pytest.raises(ValueError, match='int32'):
        evaluator_utils.metric_stats(v, f.long(), COLS, N_METRICS, 1)
    # a frame outside [0, n_frames) is left out under rule 1 and not looked at under rule 0
    f[3] = 5
    got = evaluator_utils.metric_stats(v, f, COLS, N_METRICS, 1, 1).cpu().numpy()
    assert (got[:7, 0] == 3).all() and (got[:7, 5] == 1).all() and got[7, 0] == 9
    assert (evaluator_utils.metric_stats(v, f, COLS, N_METRICS, 1, 0).cpu().numpy()[:7, 0] == 4).all()


# ---- the Evaluator on the fixture split

@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_metric_stats')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    ds = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    out = str(tmp_path_factory.mktemp('metric_stats_out'))
    ev = evaluator.Evaluator(model, ds, THRESHOLD, batch_size=BATCH, metric_stats=True, predictions_base_dir=out)
    return model, ds, ev, ev.run_once(7), out


@pytest.fixture(scope='module')
def host_values(setup):
    """{metric: values} gathered frame by frame on the host under the reference's rule: a frame whose values of a
    metric hold a NaN adds nothing to that metric.  The six errors from evaluate_predictions on the 'val'-mode build
    and its gt_dict, EMD / Chamfer as tests/test_evaluator_gpu.py::test_loss_and_metric_means gathers them."""
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    model, ds = setup[0], setup[1]
    val = MonoPSRModel(model.model_config, model.dataset_config, model.device_net, 'val', fused_heads=False)
    samples = ds.get_sample_dict(np.arange(ds.num_samples), epoch=0)
    lists = {name: [] for name in evaluator.METRIC_NAMES}
    keys = (constants.KEY_PROP_CEN_Z, constants.KEY_CENTROIDS, constants.KEY_LWH + '_offs', constants.KEY_VIEW_ANG)
    with torch.no_grad():
        for s, fused in zip(samples, model.build_batch(samples)):
            out, _ = val.build(s)
            m = val.evaluate_predictions({k: out[k] for k in keys}, val.gt_dict, s['num_objs'])
            m.update(model.evaluate_predictions(
                {constants.KEY_INST_XYZ_MAP_LOCAL: fused[constants.KEY_INST_XYZ_MAP_LOCAL]},
                {constants.KEY_INST_XYZ_MAP_LOCAL: s['gt_inst_xyz_maps_local'],
                 constants.KEY_VALID_MASK_MAPS: s['gt_valid_mask_maps']}, s['num_objs']))
            assert set(m) == set(lists)
            for name, v in m.items():
                v = v.cpu().numpy().reshape(-1)
                assert v.dtype == np.float32
                if not np.isnan(v).any():
                    lists[name].extend(v.astype(np.float64).tolist())
    return lists


def test_evaluator_reports_the_eight_metrics(setup):
    result = setup[3]
    stats = result['metric_stats']
    assert set(stats) == set(evaluator.METRIC_NAMES) and len(stats) == 8
    kept = result['num_predictions']
    assert kept == 9
    for name, st in stats.items():
        assert set(st) == set(evaluator_utils.STAT_NAMES)
        assert st['count'] == kept * (3 if name == constants.METRIC_DIM_ERR else 1) and st['dropped'] == 0, (name, st)
    assert set(result['metrics']) == {constants.METRIC_EMD, constants.METRIC_CHAMFER}


@pytest.mark.parametrize('name', evaluator.METRIC_NAMES)
def test_evaluator_statistics_against_the_host(setup, host_values, name):
    """Each statistic against numpy over the values gathered frame by frame on the host, within test 5's tolerances.
    The host's values come from a second computation; every one of them, the EMD included (its partial costs are
    added in a fixed order, tests/test_emd_reproducible_gpu.py), is the same float32 as the pass saw."""
    st = setup[3]['metric_stats'][name]
    values = np.asarray(host_values[name])
    assert st['count'] == len(values)
    want = (values.mean(), values.std(), np.abs(values).mean(), np.abs(values).std())
    print('evaluator %s: got %r want %r' % (name, st, want))
    assert abs(st['mean'] - want[0]) <= MEAN_TOL * want[2]
    assert abs(st['mean_abs'] - want[2]) <= MEAN_TOL * want[2]
    np.testing.assert_allclose(st['std'], want[1], rtol=STD_RTOL, atol=0)
    np.testing.assert_allclose(st['std_abs'], want[3], rtol=STD_RTOL, atol=0)


@pytest.fixture(scope='module')
def plain(setup):
    model, ds = setup[0], setup[1]
    return evaluator.Evaluator(model, ds, THRESHOLD, batch_size=BATCH).run_once(7)


def test_metric_stats_add_two_keys_and_nothing_else(setup, plain):
    model, ds, ev, result, out = setup
    assert 'metric_stats' not in plain and 'metrics_csv' not in plain
    assert set(plain) == set(result) - {'metric_stats', 'metrics_csv', 'kitti_predictions_dir'}
    assert set(plain['metrics']) == set(result['metrics']) == {constants.METRIC_EMD, constants.METRIC_CHAMFER}
    assert result['losses'] == plain['losses'] and len(plain['losses']) >= 6
    assert result['report'] == plain['report'] and result['num_detections'] == plain['num_detections']
    # the statistics alone, with metrics and losses off: the 'val'-mode build is made for them
    alone = evaluator.Evaluator(model, ds, THRESHOLD, batch_size=BATCH, metric_stats=True, compute_metrics=False,
                                compute_losses=False).run_once(7)
    assert alone['metrics'] == {} and alone['losses'] == {} and set(alone['metric_stats']) == set(result['metric_stats'])
    assert alone['metric_stats'] == result['metric_stats']


@pytest.mark.parametrize('name', [constants.METRIC_EMD, constants.METRIC_CHAMFER])
def test_metrics_equal_a_run_without_metric_stats(setup, plain, name):
    """result['metrics'] is equal, value for value, to a run with metric_stats=False."""
    assert setup[3]['metrics'][name] == plain['metrics'][name]


def test_entry_rule_mean_is_the_evaluators_mean(setup):
    """The table's EMD / Chamfer columns under NAN_RULE_ENTRY are what result['metrics'] averages: the same nine
    float32 values of the same pass, summed in fp64 in another order."""
    model, ds, ev, result, out = setup
    table, frame = ev.metric_table
    assert tuple(table.shape) == (9, 10) and table.dtype == torch.float32 and frame.dtype == torch.int32
    by_entry = evaluator_utils.metric_stats(table, frame, COLS, N_METRICS, ds.num_samples,
                                            evaluator_utils.NAN_RULE_ENTRY).cpu().numpy()
    for k, name in enumerate((constants.METRIC_EMD, constants.METRIC_CHAMFER)):
        np.testing.assert_allclose(by_entry[k, 1], result['metrics'][name], rtol=1e-12, atol=0, err_msg=name)


def test_metrics_csvs(setup):
    model, ds, ev, result, out = setup
    d = os.path.join(out, 'metrics', 'val')
    assert sorted(os.listdir(d)) == ['metrics_avg_abs_val.csv', 'metrics_avg_val.csv', 'metrics_std_abs_val.csv',
                                     'metrics_std_val.csv']
    assert sorted(result['metrics_csv']) == sorted(os.path.join(d, f) for f in os.listdir(d))
    names = sorted(evaluator.METRIC_NAMES)
    for stem, stat in evaluator_utils.METRIC_FILES:
        with open(os.path.join(d, '%s_val.csv' % stem), newline='') as f:
            lines = f.read().split('\r\n')
        assert len(lines) == 3 and lines[2] == ''  # one header, one line
        assert lines[0] == ','.join(['    step'] + [n[len('metric_'):].rjust(12) for n in names])
        assert lines[1] == ','.join(['       7'] + [('%.5f' % result['metric_stats'][n][stat]).rjust(12) for n in names])

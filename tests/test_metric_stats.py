"""mpsr_metric_stats and what sits on it, without a device: the symbol and its argument checks, the metrics CSV writer
against the stated format, and the key gating of MonoPSRModel.evaluate_predictions."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from monopsr_amd.core import constants, evaluator, evaluator_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_and_bound():
    from monopsr_amd import _lib
    assert 'mpsr_metric_stats' in _lib.SIGNATURES
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    assert re.search(r'\bint mpsr_metric_stats\s*\(', header)
    assert 'MPSR_METRIC_STATS_MAX_COLS 32' in header
    assert _lib.ABI_VERSION == 13 and _lib.lib().mpsr_abi_version() == 13
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS\s*:=.*\bmetric_stats\.hip', mk, re.M)
    assert re.search(r'^[^\n]*\bmetric_stats\.o[^\n]*:[^\n]*\n\t\$\(HIPCC\) \$\(FLAGS\) \$\(NOFMA\)', mk, re.M)
    assert evaluator.COLUMN_METRIC == (0, 1, 2, 3, 4, 5, 6, 7, 7, 7) and len(evaluator.METRIC_NAMES) == 8


def test_argument_errors_need_no_gpu():
    """Status 1 with a message, before anything touches the device: the pointers below are never dereferenced."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    cm = (ctypes.c_int * 10)(0, 1, 2, 3, 4, 5, 6, 7, 7, 7)
    fake = 4096  # stands for a device pointer
    f = lib.mpsr_metric_stats

    def refused(*args):
        assert f(*args) == 1, args
        msg = lib.mpsr_last_error()
        assert msg, args
        return msg

    assert b'negative' in refused(fake, fake, -1, 10, cm, 8, 4, 1, fake, fake, None)
    assert b'negative' in refused(fake, fake, 5, -1, cm, 8, 4, 1, fake, fake, None)
    assert b'negative' in refused(fake, fake, 5, 10, cm, -1, 4, 1, fake, fake, None)
    assert b'negative' in refused(fake, fake, 5, 10, cm, 8, -4, 1, fake, fake, None)
    assert b'n_metrics' in refused(fake, fake, 5, 10, cm, 11, 4, 1, fake, fake, None)
    wide = (ctypes.c_int * 33)(*([0] * 33))
    assert b'limit' in refused(fake, fake, 5, 33, wide, 8, 4, 1, fake, fake, None)
    for bad in (8, -1):
        cm_bad = (ctypes.c_int * 10)(0, 1, 2, 3, 4, 5, 6, 7, 7, bad)
        assert b'column_metric[9]' in refused(fake, fake, 5, 10, cm_bad, 8, 4, 1, fake, fake, None)
    for rule in (2, -1):
        assert b'nan_rule' in refused(fake, fake, 5, 10, cm, 8, 4, rule, fake, fake, None)
    assert b'null' in refused(None, fake, 5, 10, cm, 8, 4, 1, fake, fake, None)    # values
    assert b'null' in refused(fake, None, 5, 10, cm, 8, 4, 1, fake, fake, None)    # frame, needed by rule 1
    assert b'null' in refused(fake, fake, 5, 10, cm, 8, 4, 1, None, fake, None)    # the flag table, rule 1
    assert b'null' in refused(fake, fake, 5, 10, cm, 8, 4, 1, fake, None, None)    # stats
    assert b'null' in refused(fake, fake, 5, 10, None, 8, 4, 1, fake, fake, None)  # column_metric
    assert f(None, None, 0, 0, None, 0, 0, 0, None, None, None) == 0               # nothing to write


def test_wrapper_refuses_cpu_tensors():
    from monopsr_amd import _lib
    with pytest.raises(_lib.MpsrError, match='GPU'):
        evaluator_utils.metric_stats(torch.zeros((3, 10)), torch.zeros(3, dtype=torch.int32), evaluator.COLUMN_METRIC,
                                     8, 2)
    with pytest.raises(ValueError, match='float32'):
        evaluator_utils.metric_stats(torch.zeros((3, 9)), torch.zeros(3, dtype=torch.int32), evaluator.COLUMN_METRIC,
                                     8, 2)


def _expected_csv(names, rows):
    """The file text from the stated format: 'step' to 8 and the names without 'metric_' to 12, then per row the step
    to 8 and '{:.5f}' to 12, ',' between fields, CRLF line ends (the csv module's default)."""
    text = ','.join(['%8s' % 'step'] + ['%12s' % n[len('metric_'):] for n in names]) + '\r\n'
    for step, values in rows:
        text += ','.join(['%8s' % step] + ['%12s' % ('%.5f' % v) for v in values]) + '\r\n'
    return text


def test_csv_writer_byte_for_byte(tmp_path):
    nan = float('nan')
    stats = {
        'metric_emd': dict(count=9, mean=0.123456789, std=1.5, mean_abs=0.2, std_abs=1.25, dropped=0),
        'metric_cen_x_err': dict(count=9, mean=-12.3456749, std=100.0, mean_abs=12.5, std_abs=0.000004, dropped=1),
        'metric_dim_err': dict(count=0, mean=nan, std=nan, mean_abs=nan, std_abs=nan, dropped=27),
    }
    names = ['metric_cen_x_err', 'metric_dim_err', 'metric_emd']  # sorted
    paths = evaluator_utils.save_metric_stats(str(tmp_path), 'val', 120000, stats)
    want_dir = os.path.join(str(tmp_path), 'metrics', 'val')
    assert [os.path.relpath(p, want_dir) for p in paths] == [
        'metrics_avg_val.csv', 'metrics_std_val.csv', 'metrics_avg_abs_val.csv', 'metrics_std_abs_val.csv']
    keys = ['mean', 'std', 'mean_abs', 'std_abs']
    first = {k: [stats[n][k] for n in names] for k in keys}
    for path, k in zip(paths, keys):
        with open(path, 'rb') as f:
            assert f.read() == _expected_csv(names, [(120000, first[k])]).encode(), path
    with open(paths[0], 'rb') as f:
        assert f.read() == (b'    step,   cen_x_err,     dim_err,         emd\r\n'
                            b'  120000,   -12.34567,         nan,     0.12346\r\n')
    # a second call appends one line and no header
    second = {n: dict(s, mean=s['mean'] * 2 if s['count'] else nan) for n, s in stats.items()}
    evaluator_utils.save_metric_stats(str(tmp_path), 'val', 130000, second)
    with open(paths[0], 'rb') as f:
        assert f.read() == _expected_csv(names, [(120000, first['mean']),
                                                 (130000, [second[n]['mean'] for n in names])]).encode()
    with open(paths[1], 'rb') as f:
        assert f.read() == _expected_csv(names, [(120000, first['std']), (130000, first['std'])]).encode()


def test_metric_stats_dict():
    d = evaluator_utils.metric_stats_dict(['a', 'b'], np.array([[3, 1.5, 0.5, 1.5, 0.5, 1], [0] + [np.nan] * 4 + [6]]))
    assert d['a'] == dict(count=3, mean=1.5, std=0.5, mean_abs=1.5, std_abs=0.5, dropped=1)
    assert d['b']['count'] == 0 and d['b']['dropped'] == 6 and math.isnan(d['b']['std_abs'])


@pytest.fixture(scope='module')
def model():
    from monopsr_amd.core import config_utils
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    cfg = config_utils.default_config()
    return MonoPSRModel(cfg.model_config, cfg.dataset_config, None, 'test')


def test_evaluate_predictions_key_gating(model):
    """Without the xyz key the EMD / Chamfer branch is skipped; the six errors are ground truth minus prediction over
    the first num_objs rows."""
    g = torch.Generator().manual_seed(5)
    B, n = 5, 3
    r = lambda *shape: torch.randn(shape, generator=g)
    lwh_offs = constants.KEY_LWH + '_offs'
    pred = {constants.KEY_PROP_CEN_Z: r(B, 1), constants.KEY_CENTROIDS: r(B, 3), lwh_offs: r(B, 3),
            constants.KEY_VIEW_ANG: r(B, 1), constants.KEY_LWH: r(B, 3)}
    gt = {constants.KEY_CENTROIDS: r(B, 3), lwh_offs: r(B, 3), constants.KEY_VIEW_ANG: r(B, 1)}
    m = model.evaluate_predictions(pred, gt, n)
    assert set(m) == {constants.METRIC_VIEW_ANG_ERR, constants.METRIC_PROP_CEN_Z_ERR, constants.METRIC_CEN_X_ERR,
                      constants.METRIC_CEN_Y_ERR, constants.METRIC_CEN_Z_ERR, constants.METRIC_DIM_ERR}
    cen = gt[constants.KEY_CENTROIDS][:n] - pred[constants.KEY_CENTROIDS][:n]
    assert torch.equal(m[constants.METRIC_CEN_X_ERR], cen[:, 0]) and m[constants.METRIC_CEN_X_ERR].shape == (n,)
    assert torch.equal(m[constants.METRIC_CEN_Y_ERR], cen[:, 1])
    assert torch.equal(m[constants.METRIC_CEN_Z_ERR], cen[:, 2])
    assert torch.equal(m[constants.METRIC_PROP_CEN_Z_ERR],
                       gt[constants.KEY_CENTROIDS][:n, 2:3] - pred[constants.KEY_PROP_CEN_Z][:n])
    assert m[constants.METRIC_PROP_CEN_Z_ERR].shape == (n, 1)
    assert torch.equal(m[constants.METRIC_DIM_ERR], gt[lwh_offs][:n] - pred[lwh_offs][:n])
    assert m[constants.METRIC_DIM_ERR].shape == (n, 3)
    assert torch.equal(m[constants.METRIC_VIEW_ANG_ERR], gt[constants.KEY_VIEW_ANG][:n] - pred[constants.KEY_VIEW_ANG][:n])
    # each group on its own, and only with its keys in BOTH dictionaries
    only = model.evaluate_predictions({lwh_offs: pred[lwh_offs]}, gt, n)
    assert set(only) == {constants.METRIC_DIM_ERR}
    only = model.evaluate_predictions(pred, {constants.KEY_VIEW_ANG: gt[constants.KEY_VIEW_ANG]}, n)
    assert set(only) == {constants.METRIC_VIEW_ANG_ERR}
    no_prop = {k: v for k, v in pred.items() if k != constants.KEY_PROP_CEN_Z}
    assert constants.METRIC_CEN_X_ERR not in model.evaluate_predictions(no_prop, gt, n)
    assert model.evaluate_predictions({}, {}, n) == {}
    assert model.evaluate_predictions(pred, gt)[constants.METRIC_DIM_ERR].shape == (B, 3)  # num_objs None: every row


def test_metric_names_are_the_references():
    assert (constants.METRIC_VIEW_ANG_ERR, constants.METRIC_PROP_CEN_Z_ERR, constants.METRIC_CEN_X_ERR,
            constants.METRIC_CEN_Y_ERR, constants.METRIC_CEN_Z_ERR, constants.METRIC_DIM_ERR) == (
        'metric_view_ang_error', 'metric_prop_cen_z_err', 'metric_cen_x_err', 'metric_cen_y_err', 'metric_cen_z_err',
        'metric_dim_err')

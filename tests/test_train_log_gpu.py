"""mpsr_train_log_append (csrc/train_log.hip) against numpy in float64, and DeviceTrainLog on top of it.

Bounds: the term columns, lr, n_clipped and n_nonfinite_vars are copies and counts, hence exact (the device's sqrtf is
correctly rounded, like numpy's float32 sqrt, so the strict comparison with clip_norm agrees on every element);
grad_norm = float32(sqrt(fp64 sum)) and max_var_norm = sqrtf(float32) are each one rounding of a value whose own error
is far below a float32 ulp, so 2 float32 ulps of the float64 value.  The summary's statistics: 1e-10 relative, the bound
tests/test_metric_stats_gpu.py holds the statistics kernel to."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL, STEP_SENTINEL = -777.0, -5
N_ROWS = 3


def _table(n_cols):
    rows = torch.full((N_ROWS, n_cols), SENTINEL, dtype=torch.float32, device='cuda')
    steps = torch.full((N_ROWS,), STEP_SENTINEL, dtype=torch.int64, device='cuda')
    return rows, steps


def _call(term_values, null_terms, sumsq, n_segments, clip, lr, step, rows, steps, row, n_terms=None, n_cols=None,
          rows_ptr=True, steps_ptr=True):
    """One call; term_values: a device tensor whose element i is term i.  -> status."""
    from monopsr_amd import _lib
    terms = _lib.TrainLogTerms()
    for i in range(min(term_values.numel(), 16)):
        if i not in null_terms:
            terms.p[i] = term_values.data_ptr() + 4 * i
    n_terms = term_values.numel() if n_terms is None else n_terms
    n_cols = rows.shape[1] if n_cols is None else n_cols
    return _lib.lib().mpsr_train_log_append(
        terms, n_terms, None if sumsq is None else sumsq.data_ptr(), n_segments, clip, lr, step,
        rows.data_ptr() if rows_ptr else None, steps.data_ptr() if steps_ptr else None, rows.shape[0], n_cols, row,
        _lib.stream())


def _reference(sumsq, clip):
    """float64 grad_norm and max_var_norm, exact n_clipped and n_nonfinite_vars of a float32 host array"""
    finite = np.isfinite(sumsq)
    v = sumsq[finite]
    norms32 = np.sqrt(v)  # float32, correctly rounded
    return (float(np.sqrt(v.astype(np.float64).sum())), float(np.sqrt(v.astype(np.float64)).max()) if v.size else 0.0,
            int((norms32 > np.float32(clip)).sum()) if clip > 0 else 0, int((~finite).sum()))


def _check_row(got, term_want, sumsq, clip, lr):
    n_terms = len(term_want)
    np.testing.assert_array_equal(got[:n_terms].view(np.uint32), term_want.view(np.uint32))
    grad_norm, max_norm, n_clipped, n_nonfinite = _reference(sumsq, clip)
    for name, value, want in (('grad_norm', got[n_terms], grad_norm), ('max_var_norm', got[n_terms + 1], max_norm)):
        ulp = float(np.spacing(np.float32(want)))
        print('%s: got %.9g, float64 %.17g, %.2f ulp' % (name, value, want, abs(float(value) - want) / ulp))
        assert abs(float(value) - want) <= 2 * ulp, (name, value, want)
    assert got[n_terms + 2] == n_clipped and got[n_terms + 3] == n_nonfinite
    assert got[n_terms + 4] == np.float32(lr)


@pytest.mark.parametrize('n_terms', [1, 7, 16])
@pytest.mark.parametrize('n_segments', [0, 1, 63, 64, 65, 257, 1000])
def test_row_against_float64(n_segments, n_terms):
    rng = np.random.default_rng(1000 * n_terms + n_segments)
    sumsq = (10.0 ** rng.uniform(-12, 6, n_segments)).astype(np.float32)
    term_host = rng.standard_normal(n_terms).astype(np.float32)
    null_terms = {n_terms // 2} if n_terms > 1 else set()
    clip, lr, step, row = 1.0, 8e-5, (1 << 40) + n_segments, 1
    rows, steps = _table(n_terms + 5)
    # (the scratch behind the norms holds the chunk partials in real use: poison it, it must not be read)
    d_sumsq = torch.from_numpy(np.concatenate([sumsq, np.full(7, np.nan, np.float32)])).cuda()
    terms = torch.from_numpy(term_host).cuda()
    assert _call(terms, null_terms, d_sumsq, n_segments, clip, lr, step, rows, steps, row) == 0
    first = rows.cpu().numpy()
    assert _call(terms, null_terms, d_sumsq, n_segments, clip, lr, step, rows, steps, row) == 0
    got, got_steps = rows.cpu().numpy(), steps.cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), first.view(np.uint32))  # two calls, equal bits
    want_terms = term_host.copy()
    for i in null_terms:
        assert np.isnan(got[row, i])
        want_terms[i] = got[row, i]
    _check_row(got[row], want_terms, sumsq, clip, lr)
    assert (np.delete(got, row, axis=0) == SENTINEL).all()
    assert got_steps.tolist() == [STEP_SENTINEL, step, STEP_SENTINEL]
    if n_segments >= 63:
        assert 0 < got[row, n_terms + 2] < n_segments  # (the data do straddle the clip norm)


def test_null_sumsq_and_every_term_null():
    rows, steps = _table(3 + 5)
    terms = torch.ones(3, device='cuda')
    assert _call(terms, {0, 1, 2}, None, 9, 1.0, 0.5, 7, rows, steps, 2) == 0
    got = rows.cpu().numpy()
    assert np.isnan(got[2, :3]).all() and got[2, 3:].tolist() == [0.0, 0.0, 0.0, 0.0, 0.5]
    assert (got[:2] == SENTINEL).all() and steps.cpu().tolist() == [STEP_SENTINEL, STEP_SENTINEL, 7]


@pytest.mark.parametrize('n_segments', [5, 300])
def test_nonfinite_norms_are_counted_and_left_out(n_segments):
    rng = np.random.default_rng(n_segments)
    sumsq = (10.0 ** rng.uniform(-3, 3, n_segments)).astype(np.float32)
    sumsq[[0, n_segments - 1]] = np.inf, np.nan
    sumsq[n_segments // 2] = -np.inf
    rows, steps = _table(2 + 5)
    terms = torch.tensor([float('inf'), float('nan')], device='cuda')
    assert _call(terms, set(), torch.from_numpy(sumsq).cuda(), n_segments, 1.0, 1e-3, 3, rows, steps, 0) == 0
    got = rows.cpu().numpy()[0]
    assert np.isposinf(got[0]) and np.isnan(got[1])  # terms are copied as they are
    assert np.isfinite(got[2:]).all() and got[5] == 3
    _check_row(got, got[:2].copy(), sumsq, 1.0, 1e-3)


def test_a_norm_equal_to_the_clip_norm_is_not_clipped():
    # sqrtf(2.25) == 1.5 exactly; the neighbours of 2.25 fall on either side
    v = np.float32(2.25)
    sumsq = np.array([v, np.nextafter(v, np.float32(3)), np.nextafter(v, np.float32(0)), 2.25, 100.0, 0.0], np.float32)
    rows, steps = _table(1 + 5)
    terms = torch.zeros(1, device='cuda')
    d = torch.from_numpy(sumsq).cuda()
    assert _call(terms, set(), d, 6, 1.5, 0.0, 0, rows, steps, 0) == 0
    got = rows.cpu().numpy()[0]
    want = int((np.sqrt(sumsq) > np.float32(1.5)).sum())
    assert got[3] == want and want in (1, 2)  # 100 for certain; never the two entries that are 2.25
    only_equal = torch.full((70,), 2.25, device='cuda')
    assert _call(terms, set(), only_equal, 70, 1.5, 0.0, 0, rows, steps, 0) == 0
    assert rows.cpu().numpy()[0, 3] == 0
    for clip in (0.0, -1.0):  # no clipping: nothing is counted, the norms are still reported
        assert _call(terms, set(), d, 6, clip, 0.0, 0, rows, steps, 0) == 0
        got = rows.cpu().numpy()[0]
        assert got[3] == 0 and got[2] == 10.0 and abs(got[1] - np.sqrt(sumsq.astype(np.float64).sum())) < 1e-5


def test_argument_errors_leave_the_table_alone():
    from monopsr_amd import _lib
    rows, steps = _table(2 + 5)
    wide = torch.zeros(17, device='cuda')
    terms = torch.zeros(2, device='cuda')
    sumsq = torch.ones(4, device='cuda')
    cases = [
        ('n_terms', dict(term_values=wide, n_terms=0, n_cols=5)),
        ('n_terms', dict(term_values=wide, n_terms=17, n_cols=22)),
        ('n_cols', dict(n_cols=8)),
        ('n_cols', dict(n_cols=6)),
        ('row', dict(row=-1)),
        ('row', dict(row=N_ROWS)),
        ('null', dict(rows_ptr=False)),
        ('null', dict(steps_ptr=False)),
        ('n_segments', dict(n_segments=-1)),
    ]
    for word, over in cases:
        kw = dict(term_values=terms, null_terms=set(), sumsq=sumsq, n_segments=4, clip=1.0, lr=0.1, step=1, rows=rows,
                  steps=steps, row=0)
        kw.update(over)
        status = _call(**kw)
        assert status == 1, (word, over, status)
        assert word in _lib.lib().mpsr_last_error().decode(), (word, _lib.lib().mpsr_last_error())
    torch.cuda.synchronize()
    assert (rows == SENTINEL).all() and (steps == STEP_SENTINEL).all()
    assert ctypes.sizeof(_lib.TrainLogTerms) == 16 * ctypes.sizeof(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ DeviceTrainLog

NAMES = ('lwh', 'cen_z', 'alpha')  # (given unsorted)


def _fill(log, first_step, values, nan_total_at=(), nan_var_at=()):
    """Append len(values) steps under the no-synchronisation mode.  -> the host's copy of what every row must hold."""
    n_seg = 70
    host = []
    torch.cuda.synchronize()
    for i, v in enumerate(values):
        step = first_step + i
        rng = np.random.default_rng(step)
        sumsq = (10.0 ** rng.uniform(-4, 2, n_seg)).astype(np.float32)
        if step in nan_var_at:
            sumsq[3] = np.nan
        losses = {'lwh': v, 'alpha': 2 * v}
        if step % 2 == 0:
            losses['cen_z'] = -v  # (absent on odd steps)
        total = float('nan') if step in nan_total_at else 3.5 * v
        d_losses = {k: torch.tensor(x, device='cuda') for k, x in losses.items()}
        d_total, d_sumsq = torch.tensor(total, device='cuda'), torch.from_numpy(sumsq).cuda()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            log.append(step, d_losses, d_total, 1e-4 * (step + 1), (None, None, None, d_sumsq, n_seg), 1.0)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        g = _reference(sumsq, 1.0)
        host.append([np.float32(2 * v), np.float32(losses.get('cen_z', np.nan)), np.float32(v), np.float32(total),
                     np.float32(g[0]), np.float32(g[1]), g[2], g[3], np.float32(1e-4 * (step + 1))])
    return np.asarray(host, np.float64)


def _check_summary(summary, log, host, first_step):
    table = log.rows.cpu().numpy()
    steps = log.steps.cpu().numpy()
    order = [int(np.nonzero(steps == first_step + i)[0][0]) for i in range(len(host))]
    mine = table[order].astype(np.float64)  # the device's own rows, in step order
    np.testing.assert_allclose(mine, host, rtol=3e-7, atol=0, equal_nan=True)  # (grad columns: within 2 ulps)
    assert summary['first_step'] == first_step and summary['last_step'] == first_step + len(host) - 1
    assert list(summary['columns']) == list(log.columns)
    for c, name in enumerate(log.columns):
        col, got = mine[:, c], summary['columns'][name]
        kept = col[~np.isnan(col)]
        assert got['count'] == kept.size and got['dropped'] == col.size - kept.size
        assert got['last'] == col[-1] or (np.isnan(got['last']) and np.isnan(col[-1]))
        if kept.size:
            for stat, want in (('mean', kept.mean()), ('std', kept.std())):
                print('%s %s: %.17g vs numpy %.17g' % (name, stat, got[stat], want))
                assert abs(got[stat] - want) <= 1e-10 * abs(want), (name, stat, got[stat], want)
        else:
            assert np.isnan(got['mean']) and np.isnan(got['std'])
    assert summary['max_var_norm_max'] == mine[:, log.columns.index('max_var_norm')].max()


def test_device_train_log_summary():
    from monopsr_amd.core import train_log
    log = train_log.DeviceTrainLog(NAMES, 5, 'cuda')
    assert log.columns == ('alpha', 'cen_z', 'lwh', 'total_loss', 'grad_norm', 'max_var_norm', 'n_clipped',
                           'n_nonfinite_vars', 'lr')
    assert tuple(log.rows.shape) == (5, 9) and log.rows.dtype == torch.float32 and log.steps.dtype == torch.int64
    values = [0.3, 1.7, -2.2, 4.1, 0.9]
    # a window of 5 rows that starts at row 0, all finite
    host = _fill(log, 10, values)
    s = log.summary(10, 14)
    _check_summary(s, log, host, 10)
    assert s['first_nonfinite_step'] is None and s['nonfinite_steps'] == 0 and s['nonfinite_onsets'] == 0
    assert s['columns']['cen_z']['dropped'] == 2  # the odd steps had no such term
    # the next window wraps around the table (steps 18, 19 sit in rows 3, 4; 20 .. 22 in rows 0 .. 2), one NaN total
    host = _fill(log, 18, values, nan_total_at={20})
    s = log.summary(18, 22)
    _check_summary(s, log, host, 18)
    assert s['first_nonfinite_step'] == 20 and s['nonfinite_steps'] == 1 and s['nonfinite_onsets'] == 1
    assert s['columns']['total_loss']['count'] == 4 and s['columns']['total_loss']['dropped'] == 1
    # a variable without a finite norm comes first; the NaN total behind it
    host = _fill(log, 30, values[:3], nan_total_at={32}, nan_var_at={31})
    s = log.summary(30, 32)
    _check_summary(s, log, host, 30)
    assert s['first_nonfinite_step'] == 31 and s['nonfinite_steps'] == 2
    assert s['nonfinite_onsets'] == 1  # step 32 follows one that was not finite already
    # ... also across two summaries, while the row in front of the window is still in the table
    s = log.summary(32, 32)
    assert (s['first_nonfinite_step'], s['nonfinite_steps'], s['nonfinite_onsets']) == (32, 1, 0)
    s = log.summary(31, 32)
    assert (s['first_nonfinite_step'], s['nonfinite_steps'], s['nonfinite_onsets']) == (31, 2, 1)
    assert s['columns']['n_nonfinite_vars']['last'] == 0 and np.isnan(s['columns']['total_loss']['last'])
    assert log.summary(30, 30)['first_nonfinite_step'] is None


def test_device_train_log_refuses_what_it_cannot_log():
    from monopsr_amd.core import train_log
    log = train_log.DeviceTrainLog(NAMES, 4, 'cuda')
    one = torch.tensor(1.0, device='cuda')
    with pytest.raises(ValueError, match='not columns'):
        log.append(0, {'depth': one}, one, 0.1)
    with pytest.raises(ValueError, match='float32 scalar'):
        log.append(0, {'lwh': one.double()}, one, 0.1)
    with pytest.raises(ValueError, match='float32 scalar'):
        log.append(0, {}, 1.0, 0.1)
    log.append(0, {}, one, 0.1)  # no clip table: zeros in the gradient columns
    log.append(1, {'lwh': one}, one, 0.1, None, 1.0)
    s = log.summary(0, 1)
    assert s['columns']['grad_norm']['mean'] == 0 and s['columns']['lwh']['count'] == 1
    with pytest.raises(ValueError, match='never appended'):
        log.summary(1, 2)
    with pytest.raises(ValueError, match='rows of this log'):
        log.summary(0, 4)
    with pytest.raises(ValueError):
        train_log.DeviceTrainLog(['t%d' % i for i in range(16)], 4, 'cuda')  # 16 terms and the total: 17
    with pytest.raises(ValueError):
        train_log.DeviceTrainLog(['total_loss'], 4, 'cuda')

"""The training log kept on the device.

A training loop that wants to see its losses has two bad choices: float(loss) every step, which makes the host wait for
the card on every step, or nothing.  DeviceTrainLog is the third: every step one mpsr_train_log_append launch copies the
step's loss terms (device scalars, never read by the host) and four figures of the gradient into a row of a small
device-resident table; every summary_interval steps `summary` takes the statistics of the rows written since with one
mpsr_metric_stats launch and brings them to the host in ONE copy, whatever the window's length.
"""
import ctypes

import numpy as np
import torch

from monopsr_amd import _lib
from monopsr_amd.core import evaluator_utils

MAX_TERMS = 16  # MPSR_TRAIN_LOG_MAX_TERMS
TOTAL = 'total_loss'
STAT_COLUMNS = ('grad_norm', 'max_var_norm', 'n_clipped', 'n_nonfinite_vars', 'lr')  # MPSR_TRAIN_LOG_STAT_COLS of them


class DeviceTrainLog:
    """columns: the term names sorted, 'total_loss', then STAT_COLUMNS.  rows (window, n_cols) float32 and steps
    (window,) int64 live on `device`; row step % window holds step's figures, steps[step % window] == step."""

    def __init__(self, term_names, window, device):
        names = sorted(str(n) for n in term_names)
        if TOTAL in names or len(set(names)) != len(names):
            raise ValueError('term names must be distinct and other than %r: %s' % (TOTAL, names))
        if len(names) + 1 > MAX_TERMS:
            raise ValueError('%d terms and their total: a row holds at most %d' % (len(names), MAX_TERMS))
        if int(window) < 1:
            raise ValueError('window %r < 1' % (window,))
        self.term_names = tuple(names)
        self.columns = self.term_names + (TOTAL,) + STAT_COLUMNS
        self.n_terms, self.n_cols, self.window = len(names) + 1, len(self.columns), int(window)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.MpsrError('DeviceTrainLog lives on the GPU; monopsr_amd has no CPU path')
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.rows = torch.full((self.window, self.n_cols), float('nan'), dtype=torch.float32, device=self.device)
        self.steps = torch.full((self.window,), -1, dtype=torch.int64, device=self.device)
        self._stats = torch.empty((self.n_cols, 6), dtype=torch.float64, device=self.device)
        self._frame = torch.zeros((self.window,), dtype=torch.int32, device=self.device)  # (not read under the entry rule)
        self._col = {name: i for i, name in enumerate(self.columns)}

    def _scalar(self, name, t):
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype == torch.float32 and t.numel() == 1):
            raise ValueError('%s must be a float32 scalar tensor on %s, got %r' % (
                name, self.device, (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t)))
        return t.detach().data_ptr()

    def append(self, step, losses_dict, total_loss, lr, clip_table=None, clip_norm=0.0):
        """Write `step`'s row: one launch on the current stream, no synchronisation, no allocation on the device.
        losses_dict: {term name: float32 device scalar}; a term of this log that is missing becomes NaN in its column,
        a name this log does not know is a ValueError.  clip_table: InstanceTrainer._clip after the step's
        apply_clipped_gradients (its scratch then holds the per-variable squared norms); None, or clip_norm <= 0 (the
        norms are then not computed), gives 0 in the gradient columns."""
        unknown = sorted(set(losses_dict) - set(self.term_names))
        if unknown:
            raise ValueError('terms %s are not columns of this log %s' % (unknown, list(self.term_names)))
        terms = _lib.TrainLogTerms()
        for i, name in enumerate(self.term_names):
            if name in losses_dict:
                terms.p[i] = self._scalar(name, losses_dict[name])
        terms.p[self.n_terms - 1] = self._scalar(TOTAL, total_loss)
        sumsq, nseg = None, 0
        clip_norm = float(clip_norm or 0.0)
        if clip_table is not None and clip_norm > 0.0:
            sumsq, nseg = clip_table[3], int(clip_table[4])
            if sumsq.dtype != torch.float32 or sumsq.numel() < nseg:
                raise ValueError('the clip table\'s scratch holds %d %s, needs %d float32' % (sumsq.numel(), sumsq.dtype,
                                                                                             nseg))
        step = int(step)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mpsr_train_log_append(
                terms, self.n_terms, _lib.ptr(sumsq), nseg, clip_norm, float(lr), step, _lib.ptr(self.rows),
                _lib.ptr(self.steps), self.window, self.n_cols, step % self.window, _lib.stream()))

    def summary(self, first_step, last_step):
        """Statistics of the rows of steps first_step .. last_step (at most `window` of them, all appended and none
        overwritten since): the rows are gathered in step order, one mpsr_metric_stats launch takes count / mean / std
        per column under the entry rule (a NaN is left out and counted in `dropped`), and one device-to-host copy brings
        everything over.  ->
          {'first_step', 'last_step',
           'columns': {column: {'count', 'mean', 'std', 'dropped', 'last' (the value at last_step)}},
           'max_var_norm_max': the window's largest per-variable gradient norm,
           'nonfinite_steps': how many of the steps are not finite (see below),
           'nonfinite_onsets': how many of them follow a step that was finite (the step in front of first_step counts
                               as finite when its row is no longer in the table, and for step 0),
           'first_nonfinite_step': the smallest step whose total is not finite or whose n_nonfinite_vars > 0, else None}
        A parameter that is not finite stays so, and every later step with it: nonfinite_steps then grows with the
        window, while nonfinite_onsets counts how often the run WENT wrong."""
        first_step, last_step = int(first_step), int(last_step)
        n = last_step - first_step + 1
        if n < 1 or n > self.window or first_step < 0:
            raise ValueError('steps %d .. %d are not 1 .. %d rows of this log' % (first_step, last_step, self.window))
        dev = self.device
        with torch.cuda.device(dev):
            # the rows in step order, with the row of the step in front of them (is it still in the table?) ahead
            want = torch.arange(first_step - 1, last_step + 1, dtype=torch.int64, device=dev)
            idx = want % self.window
            with_prev = self.rows.index_select(0, idx)
            steps_with_prev = self.steps.index_select(0, idx)
            values, steps = with_prev[1:], steps_with_prev[1:]
            evaluator_utils.metric_stats(values, self._frame[:n], range(self.n_cols), self.n_cols, 0,
                                         nan_rule=evaluator_utils.NAN_RULE_ENTRY, out=self._stats)
            bad_with_prev = (~torch.isfinite(with_prev[:, self._col[TOTAL]])
                             | (with_prev[:, self._col['n_nonfinite_vars']] > 0))
            bad = bad_with_prev[1:]
            before = bad_with_prev[:-1].clone()
            before[0] &= (steps_with_prev[0] == first_step - 1) & (first_step > 0)
            never = torch.iinfo(torch.int64).max
            extras = torch.stack([
                (steps != want[1:]).sum().double(),
                values[:, self._col['max_var_norm']].max().double(),
                bad.sum().double(),
                (bad & ~before).sum().double(),
                torch.where(bad, steps, torch.full_like(steps, never)).min().double()])  # (steps < 2^53: exact)
            packed = torch.cat([self._stats.reshape(-1), values[n - 1].double(), extras]).cpu().numpy()
        stats = packed[:6 * self.n_cols].reshape(self.n_cols, 6)
        last = packed[6 * self.n_cols:7 * self.n_cols]
        stale, max_norm, n_bad, n_onsets, first_bad = packed[7 * self.n_cols:]
        if stale:
            raise ValueError('%d of the steps %d .. %d were never appended, or were overwritten since' % (
                int(stale), first_step, last_step))
        k = {name: i for i, name in enumerate(evaluator_utils.STAT_NAMES)}
        columns = {name: {'count': int(stats[c, k['count']]), 'mean': float(stats[c, k['mean']]),
                          'std': float(stats[c, k['std']]), 'dropped': int(stats[c, k['dropped']]),
                          'last': float(np.float32(last[c]))} for c, name in enumerate(self.columns)}
        return {'first_step': first_step, 'last_step': last_step, 'columns': columns,
                'max_var_norm_max': float(max_norm), 'nonfinite_steps': int(n_bad), 'nonfinite_onsets': int(n_onsets),
                'first_nonfinite_step': int(first_bad) if n_bad else None}

"""The training loop of the reference's core/trainer.py:173-209 over an InstanceTrainer and a resident KittiDataset
(DESIGN.md section 7.6): checkpoints on their interval (the one of step 0 included, each written BEFORE its step runs),
a batch, a step, and on the summary interval a line on stdout and in logs/train/train_log.csv.  The losses are never read
by the host between two summaries: every step appends a row to a DeviceTrainLog.

Under <output_dir>:
  train_state/<name>-<step, 8 digits>.{index,data-00000-of-00001}   InstanceTrainer.save: what resumes the run
  train_state/<name>-<step, 8 digits>.dataset.npz                   KittiDataset.state_dict: where in the epoch it was
  checkpoints/<name>-<step, 8 digits>.{index,data-00000-of-00001}   InstanceTrainer.export_checkpoint: what
                                                                    run_evaluation sweeps
  logs/train/train_log.csv
TensorFlow event files are not written.
"""
import csv
import io
import os
import re
import time

import numpy as np

from monopsr_amd.core import checkpoint_utils, tf_checkpoint, train_log

DEFAULTS = (('summary_interval', 10), ('checkpoint_interval', 2000), ('max_checkpoints_to_keep', None),
            ('overwrite_checkpoints', False))


def read_train_config(train_config):
    """The loop's keys of train_config (a ConfigObj, a dict or any object with attributes) with the defaults of the keys
    that are absent; max_iterations has none."""
    get = train_config.get if hasattr(train_config, 'get') else lambda k, d=None: getattr(train_config, k, d)
    out = {'max_iterations': None if train_config is None else get('max_iterations')}
    if out['max_iterations'] is None:
        raise ValueError('train_config.max_iterations is missing: the loop would not know where to end')
    out['max_iterations'] = int(out['max_iterations'])
    for key, default in DEFAULTS:
        value = get(key)
        out[key] = default if value is None else value
    for key in ('summary_interval', 'checkpoint_interval'):
        out[key] = int(out[key])
        if out[key] < 1:
            raise ValueError('train_config.%s = %d < 1' % (key, out[key]))
    keep = out['max_checkpoints_to_keep']
    out['max_checkpoints_to_keep'] = None if not keep else int(keep)
    out['overwrite_checkpoints'] = bool(out['overwrite_checkpoints'])
    return out


def schedule(start, max_iterations, checkpoint_interval, summary_interval):
    """What core/trainer.py:175-209 does from global step `start`: -> {'steps', 'checkpoints', 'summaries'}, three lists
    of steps.  A checkpoint is written before its step runs, so the one named max_iterations holds max_iterations
    updates and the run ends after max_iterations + 1."""
    steps = list(range(int(start), int(max_iterations) + 1))
    return {'steps': steps, 'checkpoints': [s for s in steps if s % checkpoint_interval == 0],
            'summaries': [s for s in steps if s % summary_interval == 0]}


def csv_header(term_names):
    """term_names: the log's term columns, the total last (DeviceTrainLog.columns[:n_terms])."""
    names = ['lr', 'seconds']
    for n in term_names:
        names += [n, n + '_mean']
    names += ['grad_norm_mean', 'max_var_norm_max', 'n_clipped_mean', 'nonfinite_onsets']
    return ['step'.rjust(8)] + [n.rjust(12) for n in names]


def csv_row(summary, seconds, term_names):
    """One line of train_log.csv from DeviceTrainLog.summary's output: the step (last_step), the learning rate and the
    seconds since the previous summary, per term its value at that step and its mean over the window, the mean global
    gradient norm, the largest per-variable norm, the mean number of clipped variables per step and the number of steps
    at which the run went non-finite (DeviceTrainLog.summary's nonfinite_onsets: a step that is not finite behind one
    that was; once a parameter is not finite every later step is not, and the loss columns say so)."""
    col = summary['columns']
    fields = ['{:.6e}'.format(col['lr']['last']), '{:.3f}'.format(seconds)]
    for n in term_names:
        fields += ['{:.5f}'.format(col[n]['last']), '{:.5f}'.format(col[n]['mean'])]
    fields += ['{:.5f}'.format(col['grad_norm']['mean']), '{:.5f}'.format(summary['max_var_norm_max']),
               '{:.5f}'.format(col['n_clipped']['mean']), '{}'.format(summary['nonfinite_onsets'])]
    return ['{}'.format(summary['last_step']).rjust(8)] + [f.rjust(12) for f in fields]


def csv_text(summary, seconds, term_names, header):
    """The bytes appended for one summary, in the style of evaluator_utils.save_metric_stats: ',' between right-justified
    fields, the csv module's line ending (CRLF)."""
    buf = io.StringIO(newline='')
    writer = csv.writer(buf, delimiter=',')
    if header:
        writer.writerow(csv_header(term_names))
    writer.writerow(csv_row(summary, seconds, term_names))
    return buf.getvalue()


def append_csv(path, summary, seconds, term_names):
    """Append one summary to `path`; the header goes into an empty file only."""
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    with open(path, 'a', newline='') as f:
        f.write(csv_text(summary, seconds, term_names, header=f.tell() == 0))
    return path


def dataset_state_path(prefix):
    return prefix + '.dataset.npz'


def _clear_checkpoints(directory, name):
    if os.path.isdir(directory):
        for entry in os.listdir(directory):
            if re.match(r'^%s-\d{8}\..+$' % re.escape(name), entry):
                os.remove(os.path.join(directory, entry))


def train(trainer, dataset, train_config, output_dir, frames_per_step=1, name='monopsr', width_div=1,
          on_nonfinite='stop', log=print, on_step=None):
    """Run `trainer` on `dataset` from its global step (or, with overwrite_checkpoints False and a checkpoint in
    <output_dir>/train_state, from that checkpoint and the dataset position saved with it) to
    train_config.max_iterations.  train_config keys: max_iterations, summary_interval (10), checkpoint_interval (2000),
    max_checkpoints_to_keep (None: all), overwrite_checkpoints (False).
    on_step(step, batch) is called with every batch before its step.  on_nonfinite: what a summary does when a step of
    its window had a total loss that is not finite, or a variable whose gradient norm is not: 'stop' raises
    FloatingPointError naming the first such step before anything more is written (every checkpoint is preceded by such
    a look at the steps since the last summary, so a window that is not finite is never saved); 'continue' logs it.
    Returns the trainer's global step, max_iterations + 1."""
    if on_nonfinite not in ('stop', 'continue'):
        raise ValueError("on_nonfinite must be 'stop' or 'continue', not %r" % (on_nonfinite,))
    cfg = read_train_config(train_config)
    frames_per_step = int(frames_per_step)
    state_dir = os.path.join(output_dir, 'train_state')
    export_dir = os.path.join(output_dir, 'checkpoints')
    csv_path = os.path.join(output_dir, 'logs', 'train', 'train_log.csv')
    if cfg['overwrite_checkpoints']:
        _clear_checkpoints(state_dir, name)
        _clear_checkpoints(export_dir, name)
    elif os.path.exists(os.path.join(state_dir, 'checkpoint')):
        prefix = tf_checkpoint.resolve_prefix(state_dir)
        with np.load(dataset_state_path(prefix)) as f:
            dataset_state = {k: f[k] for k in f.files}
        trainer.restore(prefix)
        dataset.load_state_dict(dataset_state)
        log('{}: Restored {}'.format(name, prefix))
    start, max_iterations = trainer.global_step, cfg['max_iterations']
    log('Starting from step {} / {}'.format(start, max_iterations))

    tlog, first_pending = None, start

    def look(last_step):
        """The summary of the steps first_pending .. last_step, after on_nonfinite has had its say."""
        summary = tlog.summary(first_pending, last_step)
        bad = summary['first_nonfinite_step']
        if bad is not None:
            text = 'step {} is not finite (total loss or a gradient norm; {} of the steps {} .. {})'.format(
                bad, summary['nonfinite_steps'], first_pending, last_step)
            if on_nonfinite == 'stop':
                raise FloatingPointError(text)
            log('{}: {}'.format(name, text))
        return summary

    plan = schedule(start, max_iterations, cfg['checkpoint_interval'], cfg['summary_interval'])
    checkpoint_steps, summary_steps = set(plan['checkpoints']), set(plan['summaries'])
    last_time = time.time()
    for step in plan['steps']:
        if step in checkpoint_steps:
            if tlog is not None and first_pending < step:
                look(step - 1)
            prefix = trainer.save(state_dir, name)
            np.savez(dataset_state_path(prefix), **dataset.state_dict())
            trainer.export_checkpoint(export_dir, name, width_div)
            for directory in (state_dir, export_dir):
                checkpoint_utils.prune_checkpoints(directory, cfg['max_checkpoints_to_keep'])
            log('{}: Step {} / {}: Checkpoint saved to {}'.format(name, step, max_iterations, prefix))

        batch = dataset.next_batch(frames_per_step, shuffle=True)
        if on_step is not None:
            on_step(step, batch)
        lr = trainer.optimizer.learning_rate(trainer.global_step)
        loss = trainer.step_batch(batch)
        if tlog is None:
            # (one row more than a summary covers: the step in front of a window is still there to compare with)
            tlog = train_log.DeviceTrainLog(trainer.losses_dict, cfg['summary_interval'] + 1, loss.device)
        tlog.append(step, trainer.losses_dict, loss, lr, trainer._clip, trainer.clip_norm)

        if step in summary_steps:
            summary = look(step)
            first_pending = step + 1
            now = time.time()
            elapsed, last_time = now - last_time, now
            terms = tlog.columns[:tlog.n_terms]
            append_csv(csv_path, summary, elapsed, terms)
            log('{}: Step {}: Total Loss {:0.3f}, Time Elapsed {:0.3f} s'.format(
                name, step, summary['columns'][train_log.TOTAL]['last'], elapsed))
    return trainer.global_step

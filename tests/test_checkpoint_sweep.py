"""Checkpoint sweeps without a device: the listing, the order and the skipping, with a recording callable in place of
the evaluation."""
import os
import types

import pytest

from monopsr_amd.core import checkpoint_utils, evaluator


@pytest.fixture
def ckpt_dir(tmp_path):
    d = tmp_path / 'ckpts'
    d.mkdir()
    for name in ('monopsr-00000010.index', 'monopsr-00000030.index', 'monopsr-00000020.index', 'checkpoint',
                 'monopsr-00000020.data-00000-of-00001', 'monopsr-123.index', 'notes-0000001x.index'):
        (d / name).write_bytes(b'')
    return str(d)


class _Recording(evaluator.Evaluator):
    """Evaluator with the evaluation itself replaced: records what a sweep asks for."""

    def __init__(self, predictions_base_dir, **kw):
        dataset = types.SimpleNamespace(merges_mscnn=True, is_test=False, data_split='val')
        super().__init__(None, dataset, predictions_base_dir=predictions_base_dir, **kw)
        self.calls = []

    def run_checkpoint_once(self, path, width_div=1):
        self.calls.append((os.path.basename(path), width_div))
        step = int(path[-8:])
        return dict(global_step=step, report='report of %d\n' % step)


def test_listing(ckpt_dir):
    got = checkpoint_utils.list_checkpoints(ckpt_dir)
    assert got == [(s, os.path.join(ckpt_dir, 'monopsr-%08d' % s)) for s in (10, 20, 30)]


def test_sweep_function_order_and_skipping(ckpt_dir):
    ckpts = checkpoint_utils.list_checkpoints(ckpt_dir)
    seen = []
    run = lambda step, prefix: seen.append((step, prefix)) or step * 2
    evaluated = {20}
    assert evaluator.sweep_checkpoints(ckpts[::-1], evaluated, run) == [20, 60]
    assert seen == [ckpts[0], ckpts[2]] and evaluated == {10, 20, 30}
    assert evaluator.sweep_checkpoints(ckpts, evaluated, run) == [] and len(seen) == 2
    assert evaluator.sweep_checkpoints(ckpts, evaluated, run, -1) == [60]
    assert evaluator.sweep_checkpoints(ckpts, evaluated, run, [-1]) == [60]
    assert evaluator.sweep_checkpoints(ckpts, set(), run, [30, 10]) == [60, 20]
    before = len(seen)
    with pytest.raises(KeyError, match='25'):
        evaluator.sweep_checkpoints(ckpts, set(), run, [10, 25])
    assert len(seen) == before  # raised before anything ran
    with pytest.raises(KeyError):
        evaluator.sweep_checkpoints([], set(), run, -1)


def test_run_latest_checkpoints(ckpt_dir, tmp_path):
    out = tmp_path / 'out'
    out.mkdir()
    (out / 'evaluated_val.txt').write_text('20\n')
    ev = _Recording(str(out), iou='low')
    results = ev.run_latest_checkpoints(ckpt_dir, width_div=8)
    assert ev.calls == [('monopsr-00000010', 8), ('monopsr-00000030', 8)]
    assert [r['global_step'] for r in results] == [10, 30]
    assert (out / 'evaluated_val.txt').read_text() == '20\n10\n30\n'
    assert sorted(os.listdir(str(out / 'kitti_reports' / 'val'))) == ['00000010_low.txt', '00000030_low.txt']
    assert (out / 'kitti_reports' / 'val' / '00000030_low.txt').read_text() == 'report of 30\n'
    assert ev.run_latest_checkpoints(ckpt_dir) == [] and len(ev.calls) == 2
    ev.run_latest_checkpoints(ckpt_dir, -1)
    assert ev.calls[-1] == ('monopsr-00000030', 1)
    ev.run_latest_checkpoints(ckpt_dir, [20])
    assert ev.calls[-1] == ('monopsr-00000020', 1)
    with pytest.raises(KeyError, match='40'):
        ev.run_latest_checkpoints(ckpt_dir, [40])
    # without skipping, everything runs again
    again = _Recording(str(out), skip_evaluated_checkpoints=False)
    again.run_latest_checkpoints(ckpt_dir)
    assert [c[0] for c in again.calls] == ['monopsr-00000010', 'monopsr-00000020', 'monopsr-00000030']


def test_a_sweep_needs_a_predictions_dir(ckpt_dir):
    ev = _Recording(None)
    with pytest.raises(ValueError, match='predictions_base_dir'):
        ev.run_latest_checkpoints(ckpt_dir)
    with pytest.raises(ValueError, match='predictions_base_dir'):
        ev.repeated_checkpoint_run(ckpt_dir, 30, eval_wait_interval=0, max_idle_seconds=0)
    assert ev.calls == []


def test_repeated_run_stops_at_max_iterations(ckpt_dir, tmp_path):
    ev = _Recording(str(tmp_path / 'out'))
    results = ev.repeated_checkpoint_run(ckpt_dir, 20, eval_wait_interval=0)
    # one listing evaluates what is there, in step order; a step >= max_iterations among them ends the run
    assert [r['global_step'] for r in results] == [10, 20, 30]
    assert (tmp_path / 'out' / 'evaluated_val.txt').read_text() == '10\n20\n30\n'


def test_repeated_run_stops_when_idle(ckpt_dir, tmp_path):
    ev = _Recording(str(tmp_path / 'out'))
    results = ev.repeated_checkpoint_run(ckpt_dir, 1000, eval_wait_interval=0, max_idle_seconds=0)
    assert [r['global_step'] for r in results] == [10, 20, 30]
    assert ev.repeated_checkpoint_run(ckpt_dir, 1000, eval_wait_interval=0, max_idle_seconds=0) == []
    assert len(ev.calls) == 3


def test_repeated_sweep_picks_up_new_checkpoints():
    """A checkpoint that appears between two listings is evaluated on the next one; the sleeps are the caller's."""
    listings = [[(10, 'a-00000010')], [(10, 'a-00000010')], [(10, 'a-00000010'), (20, 'a-00000020')]]
    slept, seen = [], []
    results = evaluator.repeated_sweep(lambda: listings.pop(0), set(), lambda s, p: seen.append(s) or s, 20,
                                       eval_wait_interval=7, sleep=slept.append, clock=lambda: 0.0)
    assert results == [10, 20] and seen == [10, 20] and slept == [7] and not listings


def test_command_line_arguments():
    from monopsr_amd.experiments import run_evaluation
    need = ['cfg.yaml', '--checkpoint-dir', 'c', '--mscnn-dir', 'm', '--predictions-dir', 'p']
    a = run_evaluation.build_parser().parse_args(need)
    assert (a.config, a.checkpoint_dir, a.mscnn_dir, a.predictions_dir, a.data_split, a.ckpt_indices, a.repeat,
            a.wait_interval, a.max_idle, a.width_div, a.low_iou) == ('cfg.yaml', 'c', 'm', 'p', 'val', None, False, 30.0,
                                                                     None, 1, False)
    a = run_evaluation.build_parser().parse_args(need + ['--ckpt-indices', '10', '-1', '--repeat', '--wait-interval', '2',
                                                         '--max-idle', '5', '--width-div', '8', '--low-iou',
                                                         '--data-split', 'val_half'])
    assert (a.ckpt_indices, a.repeat, a.wait_interval, a.max_idle, a.width_div, a.low_iou, a.data_split) == \
        ([10, -1], True, 2.0, 5.0, 8, True, 'val_half')
    for missing in range(1, 7, 2):
        with pytest.raises(SystemExit):
            run_evaluation.build_parser().parse_args(need[:missing] + need[missing + 2:])

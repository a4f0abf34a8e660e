"""core/train_loop.train and experiments/run_training on a five-frame split: a run to the end, checkpoint rotation, a
resumed run against an uninterrupted one, no device-to-host copy added to the step, non-finite data, the command line.

Width divisor 8, both trunks, 8 boxes per frame, 2 frames per step, a constant learning rate; max_iterations 6 with a
checkpoint every 3 and a summary every 2 steps.  One trainer serves every run (reset to its initial state in between)."""
import os
import zlib

import numpy as np
import pytest
import torch

import train_loop_cases as C
from monopsr_amd.core.config_utils import ConfigObj

pytestmark = pytest.mark.gpu

CKPT_SUFFIXES = ['data-00000-of-00001', 'index']
STATE_SUFFIXES = ['data-00000-of-00001', 'dataset.npz', 'index']


@pytest.fixture(scope='module')
def root(tmp_path_factory):
    return C.write_split(str(tmp_path_factory.mktemp('kitti')))


@pytest.fixture(scope='module')
def trainer_and_params():
    tr = C.make_trainer()
    return tr, tr.net.params.clone()


@pytest.fixture
def fresh(trainer_and_params):
    tr, params0 = trainer_and_params
    C.reset(tr, params0)
    return tr


def _run(tr, root, out, log=None, **kw):
    from monopsr_amd.core import train_loop
    config = kw.pop('config', None) or C.train_config()
    lines = []
    step = train_loop.train(tr, kw.pop('dataset', None) or C.make_dataset(root), ConfigObj(config), str(out),
                            frames_per_step=C.FRAMES_PER_STEP, name=C.NAME, width_div=C.DIV,
                            log=log or lines.append, **kw)
    return step, lines


def _check_file_set(out, steps):
    assert C.steps_in(os.path.join(out, 'checkpoints')) == {s: CKPT_SUFFIXES for s in steps}
    assert C.steps_in(os.path.join(out, 'train_state')) == {s: STATE_SUFFIXES for s in steps}
    for d in ('checkpoints', 'train_state'):
        with open(os.path.join(out, d, 'checkpoint')) as f:
            assert 'model_checkpoint_path: "%s-%08d"' % (C.NAME, max(steps)) in f.read()


def _check_csv(out, steps):
    header, rows = C.read_csv(os.path.join(out, 'logs', 'train', 'train_log.csv'))
    assert header[:3] == ['step', 'lr', 'seconds'] and header[-4:] == ['grad_norm_mean', 'max_var_norm_max',
                                                                       'n_clipped_mean', 'nonfinite_onsets']
    assert 'total_loss' in header and 'total_loss_mean' in header
    assert [r[0] for r in rows] == steps and all(len(r) == len(header) for r in rows)
    return header, rows


def test_a_run_to_the_end(fresh, root, tmp_path):
    from monopsr_amd.core import checkpoint_utils
    out = str(tmp_path)
    step, lines = _run(fresh, root, out)
    assert step == 7 and fresh.global_step == 7
    _check_file_set(out, [0, 3, 6])
    header, rows = _check_csv(out, [0, 2, 4, 6])
    print(header, rows)
    assert np.isfinite(np.asarray(rows)).all()
    assert all(r[1] == C.LEARNING_RATE and r[-1] == 0 for r in rows)
    assert all(r[header.index('grad_norm_mean')] > 0 and r[header.index('total_loss')] > 0 for r in rows)
    summaries = [line for line in lines if 'Total Loss' in line]
    assert [line.split(':')[1].strip() for line in summaries] == ['Step 0', 'Step 2', 'Step 4', 'Step 6']
    assert summaries[0].startswith('monopsr: Step 0: Total Loss ') and summaries[0].endswith(' s')
    assert lines[0] == 'Starting from step 0 / 6'
    got = checkpoint_utils.load_checkpoint(os.path.join(out, 'checkpoints', 'monopsr-00000006'))
    want = fresh.net.export_weights(C.DIV)
    assert int(got.pop('global_step')) == 6
    assert {k: v.shape for k, v in got.items()} == {k: np.shape(v) for k, v in want.items()}


def test_rotation_keeps_the_newest_two(fresh, root, tmp_path):
    out = str(tmp_path)
    step, _ = _run(fresh, root, out, config=C.train_config(max_checkpoints_to_keep=2))
    assert step == 7
    _check_file_set(out, [3, 6])
    # overwrite_checkpoints: nothing is restored, and what the earlier run left under the name is gone
    C.reset(fresh, fresh.net.params.clone())  # (step 0 again; the trained weights serve as this run's initial ones)
    step, lines = _run(fresh, root, out, config=C.train_config(max_iterations=3, overwrite_checkpoints=True))
    assert step == 4 and lines[0] == 'Starting from step 0 / 3'
    _check_file_set(out, [0, 3])
    _check_csv(out, [0, 2, 4, 6, 0, 2])


def _recorder(records, batches=None):
    def on_step(step, batch):
        first = batch[0]
        records[step] = ([s['sample_name'] for s in batch], first['boxes_2d'].cpu().numpy().copy(),
                         zlib.crc32(first['rgb_image'].cpu().numpy().tobytes()))
        if batches is not None:
            batches[step] = batch
    return on_step


def _spy_losses(tr, losses):
    inner = tr.step_batch

    def step_batch(samples):
        loss = inner(samples)
        losses.append((tr.global_step - 1, loss))
        return loss
    tr.step_batch = step_batch
    return inner


def test_a_resumed_run_continues_the_uninterrupted_one(trainer_and_params, root, tmp_path):
    from monopsr_amd.core import tf_checkpoint
    tr, params0 = trainer_and_params
    # A: uninterrupted
    C.reset(tr, params0)
    run_a = {}
    _run(tr, root, tmp_path / 'a', on_step=_recorder(run_a))
    assert sorted(run_a) == list(range(7))
    # B: to step 3 ...
    C.reset(tr, params0)
    out = str(tmp_path / 'b')
    run_b = {}
    step, _ = _run(tr, root, out, config=C.train_config(max_iterations=3), on_step=_recorder(run_b))
    assert step == 4 and sorted(run_b) == [0, 1, 2, 3]
    _check_file_set(out, [0, 3])
    prefix = os.path.join(out, 'train_state', 'monopsr-00000003')
    saved = tf_checkpoint.read_checkpoint(prefix)
    with np.load(prefix + '.dataset.npz') as f:
        saved_position = {k: f[k] for k in f.files}
    # ... and again to 6, from a trainer and a dataset that hold nothing of the first half
    tr.net.params.zero_()
    tr.net.adam_m.fill_(7.0)
    tr.net.adam_v.fill_(7.0)
    tr.optimizer.shadow = None
    tr.net.step_count, tr.global_step = 99, 99
    dataset = C.make_dataset(root, seed=5)
    restored, lines, batches, losses = {}, [], {}, []

    def log(line):
        lines.append(line)
        if line.startswith('Starting from step'):  # right behind the restore, before anything runs
            restored.update(params=tr.net.params.cpu().numpy(), adam_m=tr.net.adam_m.cpu().numpy(),
                            adam_v=tr.net.adam_v.cpu().numpy(), shadow=tr.optimizer.shadow.cpu().numpy(),
                            step_count=tr.net.step_count, global_step=tr.global_step,
                            position=dataset.state_dict())
    inner = _spy_losses(tr, losses)
    try:
        step, _ = _run(tr, root, out, log=log, dataset=dataset, on_step=_recorder(run_b, batches))
    finally:
        tr.step_batch = inner
    assert step == 7 and 'Starting from step 3 / 6' in lines and sorted(batches) == [3, 4, 5, 6]
    for key, name in (('params', 'monopsr_amd/flat_params'), ('adam_m', 'monopsr_amd/flat_params/Adam'),
                      ('adam_v', 'monopsr_amd/flat_params/Adam_1'),
                      ('shadow', 'monopsr_amd/flat_params/ExponentialMovingAverage')):
        assert np.array_equal(restored[key].view(np.uint32), saved[name].view(np.uint32)), key
    assert restored['step_count'] == int(saved['monopsr_amd/adam_step']) == 3
    assert restored['global_step'] == int(saved['global_step']) == 3
    assert sorted(restored['position']) == sorted(saved_position)
    for k, v in saved_position.items():
        assert np.array_equal(restored['position'][k], v) and restored['position'][k].dtype == v.dtype, k
    assert int(saved_position['seed']) == 0 and dataset.seed == 0
    _check_file_set(out, [0, 3, 6])
    _check_csv(out, [0, 2, 4, 6])
    # the second half of B draws what A drew
    for s in range(7):
        names_a, boxes_a, crc_a = run_a[s]
        names_b, boxes_b, crc_b = run_b[s]
        assert names_a == names_b and crc_a == crc_b, s
        assert np.array_equal(boxes_a.view(np.uint32), boxes_b.view(np.uint32)), s
    # B's step 3 is the step a third trainer takes from the same state on the same batch
    assert losses[0][0] == 3
    loss_b = float(losses[0][1])
    third = C.make_trainer(seed=1)
    third.restore(prefix)
    assert third.global_step == 3
    want = float(third.step_batch(batches[3]))
    print('step 3 of the resumed run: total loss %.9g, a third trainer %.9g, rel %.3e' % (
        loss_b, want, abs(loss_b - want) / abs(want)))
    assert np.isfinite(want) and abs(loss_b - want) <= 1e-5 * abs(want)


def _count_dtoh(run):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        run()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()]
    return sum(1 for n in names if C.is_dtoh(n)), names


def test_the_loop_adds_no_device_to_host_copy(fresh, root, tmp_path):
    from monopsr_amd.core import train_loop
    tr = fresh
    dataset = C.make_dataset(root)
    far = 10 ** 6

    def bare():
        for _ in range(4):
            tr.step_batch(dataset.next_batch(C.FRAMES_PER_STEP, True))

    def loop():
        assert tr.global_step % far != 0
        config = ConfigObj(C.train_config(max_iterations=tr.global_step + 3, checkpoint_interval=far,
                                          summary_interval=far))
        train_loop.train(tr, dataset, config, str(tmp_path), frames_per_step=C.FRAMES_PER_STEP, width_div=C.DIV,
                         log=lambda line: None)

    bare()   # warm up both paths
    loop()
    torch.cuda.synchronize()
    assert tr.global_step == 8 and not os.path.exists(str(tmp_path / 'train_state'))
    control, names = _count_dtoh(lambda: torch.ones(64, device='cuda').cpu())
    assert control >= 1, sorted(set(names))  # the profiler does see such a copy
    n_bare, _ = _count_dtoh(bare)
    n_loop, names = _count_dtoh(loop)
    print('device-to-host copies: 4 bare steps %d, 4 loop iterations %d' % (n_bare, n_loop))
    assert any('train_log_append_kernel' in n for n in names), sorted(set(names))
    assert n_loop == n_bare
    assert tr.global_step == 16


def _nan_at_step_3(step, batch):
    if step == 3:
        for sample in batch:
            sample['boxes_3d'].fill_(float('nan'))


def test_nonfinite_data_stops_the_run(fresh, root, tmp_path):
    out = str(tmp_path)
    with pytest.raises(FloatingPointError, match=r'\bstep 3\b'):
        _run(fresh, root, out, on_step=_nan_at_step_3)
    assert fresh.global_step == 5  # the summary of step 4 raised
    _check_file_set(out, [0, 3])
    _check_csv(out, [0, 2])


def test_nonfinite_data_is_logged_when_told_to_continue(fresh, root, tmp_path):
    out = str(tmp_path)
    step, lines = _run(fresh, root, out, on_step=_nan_at_step_3, on_nonfinite='continue')
    assert step == 7
    assert any('step 3 is not finite' in line for line in lines), lines
    header, rows = _check_csv(out, [0, 2, 4, 6])
    print(header, rows)
    assert [r[-1] for r in rows[:2]] == [0, 0]
    assert rows[2][-1] == 1  # the window of steps 3 and 4: the run went non-finite once, at step 3 ...
    assert rows[3][-1] == 0 and np.isnan(rows[3][header.index('total_loss')])  # ... and stayed so: no new onset
    _check_file_set(out, [0, 3, 6])


def test_command_line(root, tmp_path, capsys):
    import yaml
    from monopsr_amd.core import config_utils
    from monopsr_amd.experiments import run_training
    base = config_utils.default_config()

    def plain(obj):
        return {k: plain(v) for k, v in vars(obj).items()} if isinstance(obj, ConfigObj) else obj
    config = dict(config_name='tiny', dataset_config=C.dataset_config(root), model_config=plain(base.model_config),
                  train_config=C.train_config())
    path = tmp_path / 'tiny.yaml'
    path.write_text(yaml.safe_dump(config))
    out = str(tmp_path / 'out')
    argv = [str(path), '--output-dir', out, '--synthetic-weights', '43', '--width-div', str(C.DIV)]
    assert run_training.main(argv) == 0
    assert C.steps_in(os.path.join(out, 'checkpoints'), 'tiny') == {s: CKPT_SUFFIXES for s in (0, 3, 6)}
    assert C.steps_in(os.path.join(out, 'train_state'), 'tiny') == {s: STATE_SUFFIXES for s in (0, 3, 6)}
    _check_csv(out, [0, 2, 4, 6])
    assert sorted(os.listdir(out)) == ['checkpoints', 'logs', 'tiny.yaml', 'train_state']
    assert open(os.path.join(out, 'tiny.yaml')).read() == path.read_text()
    text = capsys.readouterr().out
    assert 'Starting from step 0 / 6' in text and 'tiny: Step 6: Total Loss ' in text
    # a changed config: the old copy is kept under a timestamp; the run resumes from step 6 and needs no weights
    config['train_config']['max_iterations'] = 7
    path.write_text(yaml.safe_dump(config))
    assert run_training.main(argv[:3] + argv[5:]) == 0
    backups = [e for e in os.listdir(out) if e.startswith('tiny.yaml.')]
    assert len(backups) == 1 and len(backups[0]) > len('tiny.yaml.2000-01-01')
    assert open(os.path.join(out, 'tiny.yaml')).read() == path.read_text()
    assert 'Starting from step 6 / 7' in capsys.readouterr().out
    _check_csv(out, [0, 2, 4, 6, 6])

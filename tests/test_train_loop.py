"""The host side of training from a config (no GPU): the loop's schedule, the epoch bookkeeping's saved state, checkpoint
rotation, the training CSV's text, the config copy and the command line's weight options."""
import datetime
import os

import numpy as np
import pytest

from monopsr_amd.core import checkpoint_utils, config_utils, train_loop
from monopsr_amd.datasets.kitti.kitti_dataset import EpochIndex
from monopsr_amd.experiments import run_training


# ---------------------------------------------------------------------------------------------------- schedule

def test_schedule_of_a_fresh_run():
    s = train_loop.schedule(0, 6, 3, 2)
    assert s['checkpoints'] == [0, 3, 6] and s['summaries'] == [0, 2, 4, 6]
    assert s['steps'] == [0, 1, 2, 3, 4, 5, 6] and len(s['steps']) == 7


def test_schedule_after_a_resume():
    s = train_loop.schedule(3, 6, 3, 2)
    assert s['steps'] == [3, 4, 5, 6] and s['checkpoints'] == [3, 6] and s['summaries'] == [4, 6]
    assert train_loop.schedule(7, 6, 3, 2) == {'steps': [], 'checkpoints': [], 'summaries': []}


def test_train_config_defaults_and_the_missing_key():
    cfg = train_loop.read_train_config(config_utils.ConfigObj({'max_iterations': 6}))
    assert cfg == {'max_iterations': 6, 'summary_interval': 10, 'checkpoint_interval': 2000,
                   'max_checkpoints_to_keep': None, 'overwrite_checkpoints': False}
    cfg = train_loop.read_train_config({'max_iterations': 6, 'summary_interval': 2, 'checkpoint_interval': 3,
                                        'max_checkpoints_to_keep': 0, 'overwrite_checkpoints': True})
    assert cfg['max_checkpoints_to_keep'] is None and cfg['overwrite_checkpoints'] is True
    assert (cfg['summary_interval'], cfg['checkpoint_interval']) == (2, 3)
    # the packaged config has no training keys: everything but max_iterations has a default
    with pytest.raises(ValueError, match='max_iterations'):
        train_loop.read_train_config(config_utils.default_config().train_config)
    with pytest.raises(ValueError, match='max_iterations'):
        train_loop.read_train_config(None)
    with pytest.raises(ValueError, match='summary_interval'):
        train_loop.read_train_config({'max_iterations': 6, 'summary_interval': 0})


def test_the_example_config_loads_with_the_training_keys():
    path = os.path.join(os.path.dirname(os.path.abspath(config_utils.__file__)), '..', 'configs',
                        'monopsr_train_example.yaml')
    cfg = config_utils.parse_yaml_config(path)
    got = train_loop.read_train_config(cfg.train_config)
    assert got == {'max_iterations': 142000, 'summary_interval': 10, 'checkpoint_interval': 2000,
                   'max_checkpoints_to_keep': 10000, 'overwrite_checkpoints': False}
    base = config_utils.default_config()
    assert vars(cfg.model_config.loss_config) == vars(base.model_config.loss_config)
    assert vars(cfg.model_config.output_config) == vars(base.model_config.output_config)
    assert vars(cfg.train_config.optimizer.adam_optimizer) == vars(base.train_config.optimizer.adam_optimizer)


# ---------------------------------------------------------------------------------------------- EpochIndex state

def _draw(index, batch_size, shuffle, n_batches):
    return [[(part.tolist(), epoch) for part, epoch in index.next(batch_size, shuffle)] for _ in range(n_batches)]


def _through_npz(state, tmp_path):
    """as the loop stores it: np.savez and np.load without pickling"""
    path = str(tmp_path / 'state.npz')
    np.savez(path, **state)
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('shuffle', [True, False])
@pytest.mark.parametrize('batch_size', [1, 2, 5])
def test_epoch_index_state_continues_the_run(tmp_path, shuffle, batch_size):
    num_samples = 5
    per_epoch = -(-num_samples // batch_size)
    # k: the start, mid-epoch, and the batch that wraps around into the next epoch just drawn (5 samples: the third
    # batch of 2 takes one sample of the next epoch; a batch of 1 or 5 ends the epoch exactly)
    for k in sorted({0, 1, per_epoch - 1, per_epoch, per_epoch + 1}):
        whole = EpochIndex(num_samples, seed=7)
        _draw(whole, batch_size, shuffle, k)
        state = _through_npz(whole.state_dict(), tmp_path)
        if k == per_epoch:
            assert whole.epochs_completed == 1  # the save point sits exactly behind the wrap-around batch
        fresh = EpochIndex(num_samples, seed=12345)  # (another seed: everything comes from the state)
        fresh.load_state_dict(state)
        want = _draw(whole, batch_size, shuffle, 3 * per_epoch)
        got = _draw(fresh, batch_size, shuffle, 3 * per_epoch)
        assert got == want, (k, got, want)
        assert (fresh.epochs_completed, fresh._index_in_epoch) == (whole.epochs_completed, whole._index_in_epoch)
        assert fresh.sample_list.tolist() == whole.sample_list.tolist()
        if shuffle and batch_size == 1:
            orders = {tuple(p[0][0] for b in want[i:i + 5] for p in b if p[0]) for i in (0, 5, 10)}
            assert len(orders) > 1  # (the epochs really are shuffled anew)


def test_epoch_index_refuses_a_foreign_state():
    a, b = EpochIndex(5, seed=1), EpochIndex(4, seed=1)
    a.next(2, True)
    before = (b.sample_list.tolist(), b._index_in_epoch, b.epochs_completed, b._rng.bit_generator.state)
    with pytest.raises(ValueError, match='5 samples'):
        b.load_state_dict(a.state_dict())
    bad = a.state_dict()
    bad['sample_list'] = np.zeros(5, np.int64)
    with pytest.raises(ValueError, match='permutation'):
        EpochIndex(5).load_state_dict(bad)
    assert before == (b.sample_list.tolist(), b._index_in_epoch, b.epochs_completed, b._rng.bit_generator.state)


# ------------------------------------------------------------------------------------------------------ rotation

def _checkpoint_dir(tmp_path, steps, name='monopsr'):
    d = tmp_path / 'ckpt'
    d.mkdir()
    for s in steps:
        for suffix in ('index', 'data-00000-of-00001', 'dataset.npz'):
            (d / ('%s-%08d.%s' % (name, s, suffix))).write_bytes(b'')
    (d / 'checkpoint').write_text('model_checkpoint_path: "%s-%08d"\n' % (name, max(steps)))
    (d / 'notes.txt').write_text('not a checkpoint')
    return d


def _steps(d):
    return sorted({int(e.split('-')[1][:8]) for e in os.listdir(str(d)) if e.startswith('monopsr-')})


def test_prune_keeps_the_newest_steps(tmp_path):
    d = _checkpoint_dir(tmp_path, [0, 3, 6, 9])
    state = (d / 'checkpoint').read_text()
    assert checkpoint_utils.prune_checkpoints(str(d), 2) == [0, 3]
    assert sorted(os.listdir(str(d))) == sorted(
        ['checkpoint', 'notes.txt'] + ['monopsr-%08d.%s' % (s, x) for s in (6, 9)
                                       for x in ('index', 'data-00000-of-00001', 'dataset.npz')])
    assert (d / 'checkpoint').read_text() == state
    assert checkpoint_utils.list_checkpoints(str(d)) == [(6, str(d / 'monopsr-00000006')), (9, str(d / 'monopsr-00000009'))]


@pytest.mark.parametrize('keep', [None, 0, 4, 7])
def test_prune_keeps_everything(tmp_path, keep):
    d = _checkpoint_dir(tmp_path, [0, 3, 6, 9])
    before = sorted(os.listdir(str(d)))
    assert checkpoint_utils.prune_checkpoints(str(d), keep) == []
    assert sorted(os.listdir(str(d))) == before and _steps(d) == [0, 3, 6, 9]


# ----------------------------------------------------------------------------------------------------------- CSV

def _summary(last_step, nonfinite=0):
    col = lambda last, mean: {'count': 2, 'mean': mean, 'std': 0.0, 'dropped': 0, 'last': last}
    return {'first_step': last_step - 1, 'last_step': last_step, 'max_var_norm_max': 3.25,
            'nonfinite_steps': 2 * nonfinite, 'nonfinite_onsets': nonfinite, 'first_nonfinite_step': last_step if nonfinite else None,
            'columns': {'lwh': col(0.5, 0.75), 'cen_z': col(float('nan'), 1.0), 'total_loss': col(12.345678, 10.0),
                        'grad_norm': col(2.0, 1.5), 'max_var_norm': col(3.25, 2.0), 'n_clipped': col(1.0, 0.5),
                        'n_nonfinite_vars': col(0.0, 0.0), 'lr': col(8e-5, 8e-5)}}


def test_csv_text_byte_for_byte(tmp_path):
    terms = ('cen_z', 'lwh', 'total_loss')
    path = str(tmp_path / 'logs' / 'train' / 'train_log.csv')
    train_loop.append_csv(path, _summary(2), 1.5, terms)
    train_loop.append_csv(path, _summary(4, nonfinite=1), 0.25, terms)
    header = ('    step,          lr,     seconds,       cen_z,  cen_z_mean,         lwh,    lwh_mean,  total_loss,'
              'total_loss_mean,grad_norm_mean,max_var_norm_max,n_clipped_mean,nonfinite_onsets\r\n')
    row2 = ('       2,8.000000e-05,       1.500,         nan,     1.00000,     0.50000,     0.75000,    12.34568,'
            '    10.00000,     1.50000,     3.25000,     0.50000,           0\r\n')
    row4 = ('       4,8.000000e-05,       0.250,         nan,     1.00000,     0.50000,     0.75000,    12.34568,'
            '    10.00000,     1.50000,     3.25000,     0.50000,           1\r\n')
    with open(path, 'rb') as f:
        assert f.read() == (header + row2 + row4).encode('ascii')
    assert train_loop.csv_text(_summary(2), 1.5, terms, header=False) == row2


# --------------------------------------------------------------------------------------------------- config copy

def test_config_copy_and_backup(tmp_path, capsys):
    src = tmp_path / 'exp.yaml'
    src.write_text('train_config: {max_iterations: 6}\n')
    out = str(tmp_path / 'out')
    copy, backup = run_training.copy_config(str(src), out, 'exp')
    assert backup is None and copy == os.path.join(out, 'exp.yaml') and open(copy).read() == src.read_text()
    assert run_training.copy_config(str(src), out, 'exp') == (copy, None)  # unchanged: nothing happens
    assert os.listdir(out) == ['exp.yaml']
    src.write_text('train_config: {max_iterations: 9}\n')
    now = datetime.datetime(2020, 1, 2, 3, 4, 5, 678)
    copy, backup = run_training.copy_config(str(src), out, 'exp', now=now)
    assert backup == copy + '.2020-01-02 03:04:05.000678'
    assert open(backup).read() == 'train_config: {max_iterations: 6}\n'
    assert open(copy).read() == 'train_config: {max_iterations: 9}\n'
    assert sorted(os.listdir(out)) == ['exp.yaml', 'exp.yaml.2020-01-02 03:04:05.000678']
    assert 'Config file has changed' in capsys.readouterr().out


def test_config_name():
    assert run_training.config_name(config_utils.ConfigObj({'config_name': 'abc'}), '/x/y.yaml') == 'abc'
    assert run_training.config_name(config_utils.ConfigObj({}), '/x/monopsr_model_000.yaml') == 'monopsr_model_000'


# -------------------------------------------------------------------------------------------------------- parser

def test_parser_defaults_and_exclusive_weight_options(capsys):
    ap = run_training.build_parser()
    a = ap.parse_args(['c.yaml', '--output-dir', 'o'])
    assert (a.config, a.output_dir, a.data_split, a.frames_per_step, a.width_div, a.seed) == \
        ('c.yaml', 'o', 'train', None, 1, 0)
    assert (a.pretrained, a.init_checkpoint, a.synthetic_weights) == (None, None, None)
    assert (a.image_noise, a.decoder_bn, a.on_nonfinite) == (None, 'frozen', 'stop')
    a = ap.parse_args(['c.yaml', '--output-dir', 'o', '--synthetic-weights', '0', '--frames-per-step', '2',
                       '--on-nonfinite', 'continue', '--decoder-bn', 'batch', '--image-noise', 'composed'])
    assert a.synthetic_weights == 0 and a.frames_per_step == 2
    assert (a.image_noise, a.decoder_bn, a.on_nonfinite) == ('composed', 'batch', 'continue')
    for pair in (['--pretrained', 'a', '--init-checkpoint', 'b'], ['--pretrained', 'a', '--synthetic-weights', '1'],
                 ['--init-checkpoint', 'b', '--synthetic-weights', '1']):
        with pytest.raises(SystemExit):
            ap.parse_args(['c.yaml', '--output-dir', 'o'] + pair)
        assert 'not allowed with' in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ap.parse_args(['c.yaml'])  # --output-dir is required
    with pytest.raises(SystemExit):
        ap.parse_args(['c.yaml', '--output-dir', 'o', '--on-nonfinite', 'ignore'])


def test_nothing_to_initialise_the_weights_is_a_system_exit(tmp_path):
    cfg = tmp_path / 'exp.yaml'
    cfg.write_text('train_config: {max_iterations: 6}\n')
    out = tmp_path / 'out'
    with pytest.raises(SystemExit) as e:
        run_training.main([str(cfg), '--output-dir', str(out)])
    for option in ('--pretrained', '--init-checkpoint', '--synthetic-weights'):
        assert option in str(e.value)
    assert not out.exists()  # nothing was written
    # a checkpoint to resume from makes the options optional, unless the config overwrites it
    (out / 'train_state').mkdir(parents=True)
    (out / 'train_state' / 'checkpoint').write_text('model_checkpoint_path: "exp-00000003"\n')
    args = run_training.build_parser().parse_args([str(cfg), '--output-dir', str(out)])
    assert run_training.will_resume(config_utils.ConfigObj({'max_iterations': 6}), str(out))
    assert not run_training.will_resume(config_utils.ConfigObj({'max_iterations': 6, 'overwrite_checkpoints': True}),
                                        str(out))
    with pytest.raises(SystemExit):
        run_training.initial_weights(args, resume=False)
    bad = tmp_path / 'bad.yaml'
    bad.write_text('train_config: {summary_interval: 2}\n')
    with pytest.raises(SystemExit, match='max_iterations'):
        run_training.main([str(bad), '--output-dir', str(out), '--synthetic-weights', '0'])

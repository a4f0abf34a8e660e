"""The evaluator's command line and checkpoint entry on the CPU: argument parsing and the missing-variable error."""
import numpy as np
import pytest

from monopsr_amd.core import evaluator


def test_command_line_arguments():
    a = evaluator.build_parser().parse_args(['cfg.yaml', 'ckpt', '--mscnn-dir', 'dets'])
    assert (a.config, a.checkpoint, a.mscnn_dir, a.data_split, a.low_iou, a.predictions_dir, a.width_div) == \
        ('cfg.yaml', 'ckpt', 'dets', 'val', False, None, 1)
    a = evaluator.build_parser().parse_args(['c', 'k', '--mscnn-dir', 'd', '--data-split', 'val_half', '--low-iou',
                                             '--predictions-dir', 'out', '--width-div', '4'])
    assert (a.data_split, a.low_iou, a.predictions_dir, a.width_div) == ('val_half', True, 'out', 4)
    with pytest.raises(SystemExit):
        evaluator.build_parser().parse_args(['cfg.yaml', 'ckpt'])  # --mscnn-dir is required


def test_a_checkpoint_that_lacks_variables_is_refused_before_the_device(tmp_path):
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    weights = W.synthetic_weights(seed=3, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE))
    dropped = sorted(weights)[0]
    path = str(tmp_path / 'partial.npz')
    checkpoint_utils.save_npz(path, {k: v for k, v in weights.items() if k != dropped})
    ev = evaluator.Evaluator.__new__(evaluator.Evaluator)  # no dataset, no model: the check comes first
    with pytest.raises(ValueError, match='lacks 1 variables') as e:
        ev.run_checkpoint_once(path, width_div=8)
    assert dropped in str(e.value)


def test_constructor_checks():
    class _Plain:
        is_test, merges_mscnn = False, False
    with pytest.raises(ValueError, match='label_scores'):
        evaluator.Evaluator(None, _Plain())
    with pytest.raises(ValueError, match='iou'):
        evaluator.Evaluator(None, _Plain(), iou='loose')

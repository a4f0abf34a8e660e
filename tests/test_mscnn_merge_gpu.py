"""mpsr_merge_detections against the numpy restatement on the whole catalogue, in one launch and frame by frame."""
import numpy as np
import pytest

import merge_cases
import merge_restatement as mr
from monopsr_amd.datasets.kitti import mscnn_utils

pytestmark = pytest.mark.gpu

CASES = merge_cases.catalogue()


def _expected(c, min_iou=None, score_type=None):
    return mr.merge_frame(c['label_boxes'], c['label_z'], c['det_boxes'], c['det_scores'],
                          c['min_iou'] if min_iou is None else min_iou, score_type or c['score_type'])


def _same(got, want, name):
    for g, w, what in zip(got, want, ('boxes', 'scores', 'match')):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, what, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, what, g, w)


@pytest.mark.parametrize('min_iou,score_type', [(0.7, 'distance'), (0.5, 'distance'), (0.7, 'max'), (0.5, 'min')])
def test_whole_catalogue_in_one_launch(min_iou, score_type):
    """Every case is one frame of a ragged split; frames without labels or detections sit between the others."""
    args = [[c[k] for c in CASES] for k in ('label_boxes', 'label_z', 'det_boxes', 'det_scores')]
    boxes, scores, match = mscnn_utils.merge_frames(*args, min_iou=min_iou, default_score_type=score_type)
    assert len(boxes) == len(CASES)
    for k, c in enumerate(CASES):
        _same((boxes[k], scores[k], match[k]), _expected(c, min_iou, score_type), c['name'])


def test_each_case_with_its_own_threshold_and_score_type():
    matched = 0
    for c in CASES:
        got = mscnn_utils.merge_frames([c['label_boxes']], [c['label_z']], [c['det_boxes']], [c['det_scores']],
                                       c['min_iou'], c['score_type'])
        want = _expected(c)
        _same([g[0] for g in got], want, c['name'])
        matched += int((want[2] >= 0).sum())
    assert matched > 60  # the catalogue merges


def test_exact_thresholds_on_the_device():
    by = {c['name']: c for c in CASES}
    for name, match in (('seventy_of_100', 0), ('exact_half', 0), ('just_under', -1)):
        c = by[name]
        got = mscnn_utils.merge_frames([c['label_boxes']], [c['label_z']], [c['det_boxes']], [c['det_scores']],
                                       c['min_iou'], c['score_type'])
        assert got[2][0][0] == match, name


def test_no_frames_and_bad_arguments():
    assert mscnn_utils.merge_frames([], [], [], [], 0.7) == ([], [], [])
    with pytest.raises(ValueError):
        mscnn_utils.merge_frames([np.zeros((1, 4))], [np.zeros(1)], [np.zeros((0, 4))], [np.zeros(0)], 0.7, 'median')
    with pytest.raises(ValueError):
        mscnn_utils.merge_frames([np.zeros((1, 4))], [np.zeros(2)], [np.zeros((0, 4))], [np.zeros(0)], 0.7)

"""MSCNN merging on the CPU: the numpy restatement against the reference's own merge_kitti_and_mscnn_obj_labels
(tests/golden/mscnn_merge.npz, recorded by tests/golden/make_mscnn_merge_fixture.py), the two exact-threshold cases by
hand, and KittiDataset's option handling with and without mscnn_label_dir."""
import os

import numpy as np
import pytest

import merge_cases
import merge_restatement as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mscnn_merge.npz')
CASES = merge_cases.catalogue()


def test_the_catalogue_holds_what_it_must():
    by = {c['name']: c for c in CASES}
    assert len(by['no_labels']['label_boxes']) == 0 and len(by['no_detections']['det_boxes']) == 0
    assert by['wide_65x70']['label_boxes'].shape == (65, 4) and by['wide_65x70']['det_boxes'].shape == (70, 4)
    assert {c['score_type'] for c in CASES} == {'distance', 'max', 'min'}
    assert {c['min_iou'] for c in CASES} >= {0.7, 0.5}
    assert list(by['clip_z']['label_z']) == [0, 40.5, 45, 60]


def test_the_fixture_holds_the_catalogue():
    with np.load(GOLDEN) as fx:
        for c in CASES:
            for key in ('label_boxes', 'label_z', 'det_boxes', 'det_scores'):
                assert np.array_equal(fx['%s/%s' % (c['name'], key)], c[key]), (c['name'], key)
            assert float(fx['%s/min_iou' % c['name']]) == c['min_iou']
            assert str(fx['%s/score_type' % c['name']]) == c['score_type']


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_restatement_equals_the_recorded_reference(case):
    boxes, scores, match = mr.merge_frame(case['label_boxes'], case['label_z'], case['det_boxes'], case['det_scores'],
                                          case['min_iou'], case['score_type'])
    assert boxes.dtype == np.float32 and scores.dtype == np.float64 and match.dtype == np.int32
    if not len(case['label_boxes']):
        assert boxes.shape == (0, 4) and len(scores) == 0 and len(match) == 0  # the reference's np.argmax raises
        return
    with np.load(GOLDEN) as fx:
        ref_boxes, ref_scores = fx['%s/ref_boxes' % case['name']], fx['%s/ref_scores' % case['name']]
    assert np.array_equal(boxes.astype(np.float64), ref_boxes)
    # the sample's label_scores is float32 (kitti_dataset.py:389-390, 422-423): compared as the sample holds it
    assert np.array_equal(scores.astype(np.float32), ref_scores.astype(np.float32))
    # match index: a merged label holds its detection's box
    for k, d in enumerate(match):
        assert np.array_equal(boxes[k], case['det_boxes'][d] if d >= 0 else case['label_boxes'][k])


def test_exact_thresholds_by_hand():
    """70/100: inter 70, union 100 + 70 - 70 = 100; float32(0.7) widened is 0.699999988..., and the reference's
    two_d_iou returns it rounded to 3 decimals, 0.7 >= 0.7: accepted.  50/100 = 0.5 exactly."""
    unit = np.array([[0, 0, 10, 10]], np.float32)
    assert float(np.float32(70) / np.float32(100)) < 0.7
    iou = mr.two_d_iou(np.array([0, 0, 10, 7], np.float32), unit)
    assert iou.dtype == np.float64 and iou[0] == 0.7
    boxes, scores, match = mr.merge_frame(unit, [10], [[0, 0, 10, 7]], [0.8], 0.7)
    assert match[0] == 0 and scores[0] == 0.8 and list(boxes[0]) == [0, 0, 10, 7]
    assert mr.two_d_iou(np.array([0, 0, 10, 5], np.float32), unit)[0] == 0.5
    boxes, scores, match = mr.merge_frame(unit, [10], [[0, 0, 10, 5]], [0.8], 0.5)
    assert match[0] == 0 and scores[0] == 0.8 and list(boxes[0]) == [0, 0, 10, 5]
    # rounding makes ties: IoU 0.9004 and 0.9001 are both 0.9, and the lower index wins
    two = np.array([[0, 0, 100, 100], [0, 0, 100, 100.03]], np.float32)
    iou = mr.two_d_iou(np.array([0, 0, 100, 90.04], np.float32), two)
    assert iou[0] == iou[1] == 0.9 and mr.merge_frame(two, [10, 10], [[0, 0, 100, 90.04]], [0.5], 0.7)[2].tolist() == [0, -1]


def _config(tmp_path, **over):
    from monopsr_amd.core.config_utils import ConfigObj
    (tmp_path / 'training').mkdir(exist_ok=True)
    (tmp_path / 'train.txt').write_text('000000\n')
    cfg = dict(dataset_dir=str(tmp_path), data_split='train', data_split_dir='training', num_boxes=8, classes=['Car'],
               oversample=True, num_alpha_bins=12, alpha_bin_overlap=0.0, use_mscnn_detections=True,
               obj_filter_config=dict(difficulty_str='hard', box_2d_height=None, truncation=0.3, occlusion=None,
                                      depth_range=[5, 45]),
               aug_config=dict(use_image_aug=False, box_jitter_type=None), depth_version='multiscale',
               instance_version='depth_2_multiscale')
    cfg.update(over)
    return ConfigObj(cfg)


def test_options_with_and_without_mscnn_label_dir(tmp_path):
    from monopsr_amd.datasets.kitti import kitti_dataset
    # without the directory both recipes are refused in _check_options, before anything is read
    with pytest.raises(ValueError, match='use_mscnn_detections'):
        kitti_dataset.KittiDataset(_config(tmp_path, dataset_dir=str(tmp_path / 'missing')), 'val')
    with pytest.raises(ValueError, match='test'):
        kitti_dataset.KittiDataset(_config(tmp_path, dataset_dir=str(tmp_path / 'missing')), 'test')
    # with it (argument or config key) the check passes and the constructor goes on to the directories
    for kw, over in ((dict(mscnn_label_dir=str(tmp_path / 'mscnn')), {}),
                     ({}, dict(mscnn_label_dir=str(tmp_path / 'mscnn')))):
        for mode in ('val', 'test'):
            with pytest.raises(FileNotFoundError, match='Dataset path'):
                kitti_dataset.KittiDataset(_config(tmp_path, dataset_dir=str(tmp_path / 'missing'), **over), mode, **kw)
    ds = kitti_dataset.KittiDataset.__new__(kitti_dataset.KittiDataset)
    ds.train_val_test, ds.box_jitter_type, ds.use_mscnn_detections, ds.oversample = 'val', None, True, True
    ds.use_image_aug, ds.num_classes, ds.mscnn_label_dir = False, 1, '/somewhere'
    ds._check_options()
    assert ds.jitter_mode == 0
    ds.train_val_test = 'test'
    ds._check_options()
    ds.mscnn_label_dir = None
    with pytest.raises(ValueError, match='test'):
        ds._check_options()

"""KittiDataset's two evaluation recipes on the five-frame fixture split with synthetic MSCNN detection files
(tests/mscnn_split.py): 'val' with the detections merged into the labels, and 'test' from the detections alone."""
import copy
import os

import numpy as np
import pytest
import torch

import jitter_restatement as jr
import merge_restatement as mr
import mscnn_split
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils as iu, kitti_dataset, mscnn_utils, obj_utils

pytestmark = pytest.mark.gpu

VAL_KEYS = {'rgb_image', 'boxes_2d', 'boxes_2d_norm', 'cam_p', 'est_view_angs', 'class_indices', 'mean_lwh',
            'prop_cen_z_offset', 'boxes_3d', 'gt_alpha_bins', 'gt_alpha_regs', 'gt_alpha_valid_bins', 'gt_view_angs',
            'gt_inst_xyz_maps_local', 'gt_inst_xyz_maps_global', 'gt_valid_mask_maps', 'sample_name', 'num_objs',
            'oversample_indices', 'jitter_trials'}
TEST_KEYS = {'rgb_image', 'cam_p', 'sample_name', 'num_objs', 'boxes_2d', 'boxes_2d_norm', 'label_scores',
             'class_indices', 'mean_lwh', 'prop_cen_z_offset', 'est_view_angs'}


@pytest.fixture(scope='module')
def split(tmp_path_factory):
    return mscnn_split.build(str(tmp_path_factory.mktemp('kitti_mscnn')))


@pytest.fixture(scope='module')
def merged(split):
    root, mscnn = split
    return kitti_dataset.KittiDataset(mscnn_split.config(root), 'val', mscnn_label_dir=mscnn)


def _host_merged_labels(root, mscnn, name):
    """The reference's recipe on the host, with the numpy restatement of the merge."""
    kitti = obj_utils.read_labels(os.path.join(root, 'training', 'label_2'), name)
    dets = obj_utils.read_labels(mscnn, name)
    lb, lz, _ = mscnn_utils.label_arrays(kitti)
    db, _, dscore = mscnn_utils.label_arrays(dets)
    boxes, scores, _ = mr.merge_frame(lb, lz, db, dscore, 0.7, 'distance')
    out = copy.deepcopy(kitti)
    for o, b, s in zip(out, boxes, scores):
        o.y1, o.x1, o.y2, o.x2, o.score = b[0], b[1], b[2], b[3], float(s)
    flt = obj_utils.ObjectFilter(['Car'], **mscnn_split.FILTER)
    kept, mask = obj_utils.apply_obj_filter(out, flt)
    return kept, np.arange(len(out))[mask], len(obj_utils.apply_obj_filter(kitti, flt)[0])


def _eq(t, a, dtype=np.float32):
    a = np.asarray(a).astype(dtype)
    got = t.cpu().numpy()
    assert got.dtype == a.dtype and got.shape == a.shape, (got.dtype, a.dtype, got.shape, a.shape)
    assert np.array_equal(got, a)


def test_merged_val_samples(split, merged):
    root, mscnn = split
    ds = merged
    # 000000 keeps no Car; the merged box of 000001's only Car is 19.5 px high, under box_2d_height
    assert ds.sample_names == ['000006', '000010', '000002'] and ds.num_skipped == 3 and ds.num_samples == 3
    # 000011: the merged labels keep the Car (21.5 px), KITTI's own keep nothing (19.0 px): the second check skips it
    kept, _, kitti_kept = _host_merged_labels(root, mscnn, '000011')
    assert len(kept) == 1 and float(kept[0].y2 - kept[0].y1) == 21.5 and kitti_kept == 0
    assert _host_merged_labels(root, mscnn, '000001')[2] == 1 and len(_host_merged_labels(root, mscnn, '000001')[0]) == 0
    samples = ds.get_sample_dict([0, 1, 2])
    for s in samples:
        name = s['sample_name']
        assert set(s) == VAL_KEYS | {'label_scores'}
        kept, rows, _ = _host_merged_labels(root, mscnn, name)
        assert s['num_objs'] == len(kept)
        idx = s['oversample_indices'].cpu().numpy()
        assert np.array_equal(idx, jr.oversample_indices(len(kept), 8, mscnn_split.NAMES.index(name), 0, 0))
        labels = kept[idx]
        cam_p = depth_map_utils.read_calibration(os.path.join(root, 'training', 'calib', name + '.txt')).p2
        shape = tuple(s['rgb_image'].shape[0:2])
        boxes_2d = obj_utils.boxes_2d_from_obj_labels(labels)
        _eq(s['boxes_2d'], boxes_2d)
        _eq(s['boxes_2d_norm'], boxes_2d / np.tile(shape, 2))
        view = np.asarray([obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in boxes_2d], np.float32)
        _eq(s['est_view_angs'], view)
        _eq(s['label_scores'], [o.score for o in labels])
        boxes_3d = obj_utils.boxes_3d_from_obj_labels(labels)
        _eq(s['boxes_3d'], boxes_3d)
        _eq(s['gt_view_angs'], [obj_utils.get_viewing_angle_box_3d(b, cam_p) for b in boxes_3d])
        assert (s['jitter_trials'] == 0).all()
        # the maps are the crops of the sample's own (merged) boxes; instance ids are the label rows
        depth = depth_map_utils.read_depth_map(os.path.join(root, 'training', 'depth_2_multiscale', name + '.png'))
        inst = iu.read_instance_image(os.path.join(root, 'training', 'instance_2_depth_2_multiscale', name + '.png'))
        local, glob, valid = iu.instance_xyz_crops(depth[None], inst[None], np.asarray(cam_p, np.float32)[None],
                                                   np.zeros(8, np.int32), rows[idx], boxes_2d, boxes_3d, view, (48, 48),
                                                   'middle', True)
        assert torch.equal(s['gt_inst_xyz_maps_local'], local) and torch.equal(s['gt_inst_xyz_maps_global'], glob)
        assert torch.equal(s['gt_valid_mask_maps'], valid) and float(valid.sum()) > 0
    by = {s['sample_name']: s for s in samples}
    # 000006: all four cars matched (the second by the later of its two detections); 000010: two matched, two by distance
    assert np.allclose(by['000006']['label_scores'][:4].cpu().numpy(), [0.55, 0.93, 0.88, 0.76])
    assert list(by['000006']['boxes_2d'][1].cpu().numpy()) == [168.0, 504.5, 208.5, 575.0]
    want = [np.float32(1) - np.float32(48.22) / np.float32(45), 0.97, 0.88, np.float32(1) - np.float32(38.44) / np.float32(45)]
    want[0] = max(want[0], np.float32(0.1))
    assert np.array_equal(by['000010']['label_scores'][:4].cpu().numpy(), np.asarray(want, np.float32))
    # an empty detection file: KITTI's boxes, distance scores
    assert list(by['000002']['boxes_2d'][0].cpu().numpy()) == [np.float32(190.13), np.float32(657.39),
                                                               np.float32(223.39), np.float32(700.07)]
    assert ds.status() == (0, 0)


def test_test_mode_samples_come_from_the_detection_files(tmp_path):
    root, mscnn = mscnn_split.build(str(tmp_path / 'k'), with_labels=False)
    assert not os.path.exists(os.path.join(root, 'training', 'label_2'))
    ds = kitti_dataset.KittiDataset(mscnn_split.config(root, oversample=False), 'test', mscnn_label_dir=mscnn)
    # 000000 holds a Pedestrian only, 000002 an empty file
    assert ds.sample_names == ['000006', '000001', '000010', '000011'] and ds.num_skipped == 2
    assert not ds.has_kitti_labels
    for s in ds.get_sample_dict([0, 1, 2, 3]):
        name = s['sample_name']
        assert set(s) == TEST_KEYS
        dets = obj_utils.read_labels(mscnn, name)
        assert s['num_objs'] == len(dets) == len(mscnn_split.DETECTIONS[name])
        idx = jr.oversample_indices(len(dets), 8, mscnn_split.NAMES.index(name), 0, 0)
        labels = dets[idx]
        cam_p = depth_map_utils.read_calibration(os.path.join(root, 'training', 'calib', name + '.txt')).p2
        boxes_2d = obj_utils.boxes_2d_from_obj_labels(labels)
        _eq(s['boxes_2d'], boxes_2d)
        _eq(s['boxes_2d_norm'], boxes_2d / np.tile(tuple(s['rgb_image'].shape[0:2]), 2))
        _eq(s['est_view_angs'], [obj_utils.get_viewing_angle_box_2d(b, cam_p) for b in boxes_2d])
        _eq(s['label_scores'], [o.score for o in labels])
        _eq(s['class_indices'], np.ones((8, 1)), np.int32)
        _eq(s['mean_lwh'], np.tile([[3.892, 1.619, 1.530]], (8, 1)))
        assert s['prop_cen_z_offset'].shape == (8,) and s['rgb_image'].dtype == torch.float32
    os.remove(os.path.join(mscnn, '000010.txt'))
    with pytest.raises(FileNotFoundError):
        kitti_dataset.KittiDataset(mscnn_split.config(root), 'test', mscnn_label_dir=mscnn)


def _is_dtoh(name):
    n = name.lower().replace(' ', '').replace('_', '')
    return 'dtoh' in n or 'devicetohost' in n or 'device->host' in n or 'device->pageable' in n or 'device->pinned' in n


def test_batches_make_no_device_to_host_copy(split, merged):
    from torch.profiler import ProfilerActivity, profile
    root, mscnn = split
    test = kitti_dataset.KittiDataset(mscnn_split.config(root), 'test', mscnn_label_dir=mscnn)
    for ds in (merged, test):
        ds.get_sample_dict([0, 1])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            ds.get_sample_dict([0, 1, 2])
            ds.next_batch(2, False)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as control:
        torch.ones(64, device='cuda').cpu()
        torch.cuda.synchronize()
    assert any(_is_dtoh(e.name) for e in control.events()), sorted({e.name for e in control.events()})
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for ds in (merged, test):
            ds.next_batch(2, False)
            ds.get_sample_dict([2, 0])
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events()})
    assert not [n for n in names if _is_dtoh(n)], names
    assert any('sample_slots_kernel' in n for n in names), names


def test_existing_recipes_keep_their_keys_and_bits(split, merged):
    """'val' on KITTI's boxes and 'train' carry no label_scores; given mscnn_label_dir or not, their samples are the
    same bits, and the merged recipe's 3-D rows of a frame equal the plain recipe's."""
    root, mscnn = split
    plain = kitti_dataset.KittiDataset(mscnn_split.config(root, use_mscnn_detections=False), 'val')
    given = kitti_dataset.KittiDataset(mscnn_split.config(root, use_mscnn_detections=False), 'val',
                                       mscnn_label_dir=mscnn)
    train = kitti_dataset.KittiDataset(mscnn_split.config(root, data_split='train'), 'train', mscnn_label_dir=mscnn)
    assert plain.sample_names == ['000006', '000001', '000010', '000002'] == train.sample_names
    for a, b in zip(plain.get_sample_dict([0, 1, 2, 3]), given.get_sample_dict([0, 1, 2, 3])):
        assert set(a) == VAL_KEYS == set(b)
        for k in VAL_KEYS - {'sample_name', 'num_objs'}:
            assert torch.equal(a[k], b[k]), k
    assert set(train.next_batch(1, False)[0]) == VAL_KEYS
    # (the module's merged dataset has been through an epoch in the test above: the draw of a slot depends on it)
    a, m = plain.get_sample_dict([0], epoch=0)[0], merged.get_sample_dict([0], epoch=0)[0]
    assert a['sample_name'] == m['sample_name'] == '000006'
    for k in ('boxes_3d', 'gt_alpha_bins', 'gt_alpha_regs', 'gt_alpha_valid_bins', 'gt_view_angs', 'rgb_image', 'cam_p'):
        assert torch.equal(a[k], m[k]), k
    assert not torch.equal(a['boxes_2d'], m['boxes_2d'])

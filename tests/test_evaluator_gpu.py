"""Evaluator.run_once on the fixture split in 'val' merged mode with a small random-weight net, against the host path:
format_predictions per frame, kitti_eval.evaluate_predictions, export_kitti_labels."""
import os

import numpy as np
import pytest
import torch

import mscnn_split
from monopsr_amd.core import config_utils, constants, evaluator, evaluator_utils, kitti_eval
from monopsr_amd.datasets.kitti import kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_eval')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    ds = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    return root, mscnn, model, ds


def _host_predictions(model, ds):
    """format_predictions per kept frame; an empty entry for every skipped frame of the split."""
    empty = (np.zeros((0, 9), np.float32), np.zeros((0, 7), np.float32))
    predictions = {name: empty for name in ds.split_sample_names}
    samples = ds.get_sample_dict(np.arange(ds.num_samples), epoch=0)
    for s, out in zip(samples, model.build_batch(samples)):
        sample_dict = {constants.SAMPLE_NUM_OBJS: s['num_objs'], constants.SAMPLE_CAM_P: s['cam_p'].cpu().numpy(),
                       constants.SAMPLE_LABEL_SCORES: s['label_scores'].cpu().numpy(),
                       constants.SAMPLE_LABEL_BOXES_2D: s['boxes_2d'].cpu().numpy(),
                       'image_shape': tuple(s['rgb_image'].shape)}
        pred = model.format_predictions(model.output_types, out, sample_dict)
        predictions[s['sample_name']] = (pred[constants.KEY_BOX_3D], pred[constants.KEY_BOX_2D])
    return predictions


def _same_result(a, b):
    assert set(a) == set(b) and a
    for cls in a:
        assert set(a[cls]) == set(b[cls])
        for metric in a[cls]:
            for key in ('curve', 'ap11', 'ap40'):
                assert np.asarray(a[cls][metric][key]).tobytes() == np.asarray(b[cls][metric][key]).tobytes(), \
                    (cls, metric, key)


@pytest.mark.parametrize('project', [False, True])
def test_run_once_equals_the_host_path(setup, tmp_path, project):
    root, mscnn, model, ds = setup
    gt_dir = os.path.join(root, 'training', 'label_2')
    ev = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=str(tmp_path), batch_size=2,
                             project_3d_box=project, iou='low')
    result = ev.run_once(7)
    predictions = _host_predictions(model, ds)
    info = ds.frame_info
    want = kitti_eval.evaluate_predictions(predictions, ds.classes, THRESHOLD, gt_dir, project, info, iou='low')
    # (with projection the device's cos / sin differ from numpy's in the last bits; the rows are rounded to 3 decimals,
    # and none of this fixture's values lies on a rounding or keep boundary, so the AP arrays are equal there too)
    _same_result(result['kitti'], want)
    assert result['report'] == kitti_eval.format_report(want, 7)
    assert result['num_frames'] == 6 and result['num_predictions'] == sum(len(p[0]) for p in predictions.values()) == 9
    assert 0 < result['num_detections'] <= 9 and 1 <= result['num_frames_with_detections'] <= 3
    assert set(result['metrics']) == {constants.METRIC_EMD, constants.METRIC_CHAMFER}
    assert all(np.isfinite(v) and v > 0 for v in result['metrics'].values())
    # the written files: export_kitti_labels' text, byte for byte (without projection: the same fp64 rounding)
    out_dir = result['kitti_predictions_dir']
    assert out_dir == evaluator_utils.kitti_output_dir(str(tmp_path), 'val', THRESHOLD, 7)
    host_dir = str(tmp_path / 'host')
    evaluator_utils.export_kitti_labels(predictions, ds.classes, THRESHOLD, host_dir, ds.split_sample_names, project, info)
    assert sorted(os.listdir(out_dir)) == sorted(n + '.txt' for n in ds.split_sample_names)
    if not project:
        for name in ds.split_sample_names:
            with open(os.path.join(out_dir, name + '.txt'), 'rb') as a, open(os.path.join(host_dir, name + '.txt'), 'rb') as b:
                assert a.read() == b.read(), name
    from_files = kitti_eval.evaluate_dirs(gt_dir, os.path.dirname(out_dir), iou='low')
    _same_result(result['kitti'], from_files)


def test_loss_and_metric_means(setup):
    """The means of run_once against the same quantities taken frame by frame on the host: MonoPSRModel.loss on the
    'val'-mode build, evaluate_predictions on the fused build, NaN entries skipped."""
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    _, _, model, ds = setup
    result = evaluator.Evaluator(model, ds, THRESHOLD, batch_size=2).run_once()
    val = MonoPSRModel(model.model_config, model.dataset_config, model.device_net, 'val', fused_heads=False)
    samples = ds.get_sample_dict(np.arange(ds.num_samples), epoch=0)
    per_frame, metrics = [], {constants.METRIC_EMD: [], constants.METRIC_CHAMFER: []}
    with torch.no_grad():
        for s, fused in zip(samples, model.build_batch(samples)):
            out, _ = val.build(s)
            losses, total = val.loss(out, val.gt_dict, s['gt_alpha_valid_bins'])
            per_frame.append(dict({k: float(torch.as_tensor(v).sum()) for k, v in losses.items()},
                                  total_loss=float(torch.as_tensor(total).sum())))
            m = model.evaluate_predictions(
                {constants.KEY_INST_XYZ_MAP_LOCAL: fused[constants.KEY_INST_XYZ_MAP_LOCAL]},
                {constants.KEY_INST_XYZ_MAP_LOCAL: s['gt_inst_xyz_maps_local'],
                 constants.KEY_VALID_MASK_MAPS: s['gt_valid_mask_maps']}, s['num_objs'])
            for key in metrics:
                metrics[key].extend(m[key].cpu().numpy().astype(np.float64).tolist())
    names = set(per_frame[0])
    assert set(result['losses']) == names and 'total_loss' in names and len(names) >= 6, names
    assert constants.KEY_INST_XYZ_MAP_LOCAL in names and constants.KEY_LWH + '_offs' in names
    for key in names:
        want = np.nanmean([f[key] for f in per_frame])
        assert np.isfinite(want) and want > 0, key
        # the same kernels on the same inputs; float32 terms summed in fp64 on both sides
        np.testing.assert_allclose(result['losses'][key], want, rtol=1e-5, err_msg=key)
    parts = sum(v for k, v in result['losses'].items() if k != 'total_loss')
    np.testing.assert_allclose(result['losses']['total_loss'], parts, rtol=1e-5)
    for key, values in metrics.items():
        np.testing.assert_allclose(result['metrics'][key], np.nanmean(values), rtol=1e-5, err_msg=key)
    off = evaluator.Evaluator(model, ds, THRESHOLD, compute_losses=False, compute_metrics=False).run_once()
    assert off['losses'] == {} and off['metrics'] == {} and off['num_detections'] == result['num_detections']
    plain = kitti_dataset.KittiDataset(mscnn_split.config(setup[0], use_mscnn_detections=False), 'val')
    with pytest.raises(ValueError, match='label_scores'):
        evaluator.Evaluator(model, plain)


def _is_dtoh(name):
    n = name.lower().replace(' ', '').replace('_', '')
    return 'dtoh' in n or 'devicetohost' in n or 'device->host' in n or 'device->pageable' in n or 'device->pinned' in n


def test_copies_to_the_host_do_not_grow_with_the_split(setup):
    from torch.profiler import ProfilerActivity, profile
    root, mscnn, model, _ = setup
    counts = []
    for names in (['000006', '000010'], ['000000', '000006', '000010', '000002']):
        split = 'val%d' % len(names)
        with open(os.path.join(root, split + '.txt'), 'w') as f:
            f.write(''.join(n + '\n' for n in names))
        ds = kitti_dataset.KittiDataset(mscnn_split.config(root, data_split=split), 'val', mscnn_label_dir=mscnn)
        ev = evaluator.Evaluator(model, ds, THRESHOLD, batch_size=1)
        ev.run_once()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            ev.run_once()
            torch.cuda.synchronize()
        counts.append(sum(1 for e in prof.events() if _is_dtoh(e.name)))
    assert counts[0] == counts[1] and counts[0] >= 1, counts


def test_test_mode_without_labels_returns_detections_and_no_ap(setup, tmp_path):
    _, _, model, _ = setup
    root, mscnn = mscnn_split.build(str(tmp_path / 'k'), with_labels=False)
    ds = kitti_dataset.KittiDataset(mscnn_split.config(root), 'test', mscnn_label_dir=mscnn)
    result = evaluator.Evaluator(model, ds, THRESHOLD, predictions_base_dir=str(tmp_path / 'out')).run_once(3)
    assert result['kitti'] is None and result['report'] is None and result['metrics'] == {}
    assert result['num_predictions'] == 6 + 1 + 2 + 1 and result['num_detections'] > 0 and result['losses'] == {}
    files = sorted(os.listdir(result['kitti_predictions_dir']))
    assert files == sorted(n + '.txt' for n in mscnn_split.NAMES)
    assert os.path.getsize(os.path.join(result['kitti_predictions_dir'], '000002.txt')) == 0

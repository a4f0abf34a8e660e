"""mpsr_scene_score and what is built on it, on the GPU against tests/scene_score_restatement.py: the counts exactly,
the fp64 sums bit for bit where the catalogue makes them independent of their order and within the reordering bound
elsewhere."""
import os

import numpy as np
import pytest
import torch

import mscnn_split
import scene_score_cases as cases
import scene_score_restatement as restatement
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import scene_reconstruction as sr
from monopsr_amd.datasets.kitti import instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1


def _device_ground_truth(gt, dev):
    """Each frame's maps as slice 1 of a stack of two: a 5 x 7 or 6 x 13 instance image then starts at byte 35 or 78
    of its allocation, off every alignment."""
    depths, insts = [], []
    for d, im in zip(gt['depth_maps'], gt['instance_images']):
        depths.append(torch.from_numpy(np.stack([np.full_like(d, 1.0), d])).to(dev)[1])
        insts.append(torch.from_numpy(np.stack([np.full_like(im, 7), im])).to(dev)[1])
    return dict(depth_maps=depths, instance_images=insts, box_gt_id=np.asarray(gt['box_gt_id']))


def _run(name, with_gt=True, **kw):
    case = cases.case(name)
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    images = case.get('images')
    gt = _device_ground_truth(cases.ground_truth(name), dev) if with_gt else None
    return sr.project_instance_points(
        t(np.asarray(case['xyz'], np.float32)), case['box_frame'], case['cam_p'], case['shapes'],
        images=None if images is None else [t(im) for im in images],
        valid_mask=None if case.get('mask') is None else t(np.asarray(case['mask'], np.float32)),
        keep=None if case.get('keep') is None else t(np.asarray(case['keep'], np.int32)), ground_truth=gt, **kw)


def _assert_scores(name, result, what=''):
    want = cases.expected(name)
    s = result.scores
    assert s.counts.dtype == torch.int32 and s.sums.dtype == torch.float64
    counts, sums = s.counts.cpu().numpy(), s.sums.cpu().numpy()
    assert counts.shape == want['counts'].shape and sums.shape == want['sums'].shape
    assert np.array_equal(counts, want['counts']), (name, what)
    assert np.array_equal(counts[:, 0], result.kept_per_box.cpu().numpy())
    assert np.array_equal(counts[:, 2], result.visible_per_box.cpu().numpy())
    if name in cases.EXACT_NAMES:
        assert sums.tobytes() == want['sums'].tobytes(), (name, what)
    else:
        bound = restatement.sum_bounds(cases.case(name), cases.ground_truth(name), cases.scene(name))
        assert bool((np.abs(sums - want['sums']) <= bound).all()), (name, what, np.abs(sums - want['sums']).max())
    return counts, sums


@pytest.mark.parametrize('name', cases.NAMES)
def test_catalogue_equals_the_restatement(name):
    result = _run(name)
    counts, sums = _assert_scores(name, result)
    got = result.scores.table().cpu().numpy()
    want = restatement.table(counts, sums, cases.ground_truth(name)['box_gt_id'])
    # fp64 quotients and roots of the same counts and sums, rounded once to float32: one float32 ulp at the most apart
    assert got.dtype == np.float32 and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert bool((np.abs(np.nan_to_num(got) - np.nan_to_num(want)) <= 2.0 ** -23 * np.abs(np.nan_to_num(want))).all())


def test_identity_case_scores_one():
    table = _run('identity_2304').scores.table().cpu().numpy()
    assert np.array_equal(table, np.asarray([[1, 1, 1, 0, 0, 0]] * 2, np.float32))
    scaled = _run('scaled_2304').scores
    d = cases.ground_truth('scaled_2304')
    mine = d['depth_maps'][0].astype(np.float64)[d['instance_images'][0] == 254]
    assert scaled.sums[0].tolist() == [0.25 * mine.sum(), 0.25 * mine.sum(), (mine * mine).sum() / 16.0]
    assert scaled.counts[0].tolist() == [2304] * 6


def test_two_runs_return_the_same_bytes():
    name = cases.DETERMINISM_CASE
    a, b = _run(name).scores, _run(name).scores
    assert a.counts.cpu().numpy().tobytes() == b.counts.cpu().numpy().tobytes()
    assert a.sums.cpu().numpy().tobytes() == b.sums.cpu().numpy().tobytes()
    assert int(a.counts[:, 5].sum()) > 0


def test_poisoned_buffers_change_nothing(monkeypatch):
    """Every buffer the wrapper allocates (the workspace, the histogram scratch and the outputs) filled with 0xFF bytes
    beforehand -- NaN in every float, -1 in every count -- and then with 0x00 bytes: the scores are the restatement's."""
    real = sr._empty
    for fill in (255, 0):
        def poisoned(shape, dtype, device, fill=fill):
            t = real(shape, dtype, device)
            if t.numel():
                t.view(torch.uint8).fill_(fill)
            return t
        monkeypatch.setattr(sr, '_empty', poisoned)
        for name in ('zbuffer_three_boxes', 'dropped', 'grid_b3_p300', 'scaled_2304', cases.DETERMINISM_CASE):
            _assert_scores(name, _run(name), fill)


def test_scoring_changes_nothing_else():
    for name in ('grid_b70_p64', 'random_b3_p2304', 'identity'):
        for visible_only in (False, True):
            a, b = _run(name, True, visible_only=visible_only), _run(name, False, visible_only=visible_only)
            assert b.scores is None and a.scores is not None
            for k in ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'kept_per_box', 'visible_per_box'):
                x, y = getattr(a, k), getattr(b, k)
                assert (x is None) == (y is None), k
                if x is not None:
                    assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (name, k)
            for x, y in zip(a.depth_maps + a.instance_maps, b.depth_maps + b.instance_maps):
                assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name


def test_empty_inputs_and_bad_ground_truth():
    dev = torch.device('cuda', 0)
    cam = cases.scene_cases.pow2_camera(2.0, 0.0, 0.0)[None]
    gt = dict(depth_maps=[torch.ones((5, 7), device=dev)], instance_images=[torch.zeros((5, 7), dtype=torch.uint8,
                                                                                        device=dev)])
    r = sr.project_instance_points(torch.zeros((2, 0, 3), device=dev), [0, 0], cam, [(5, 7)],
                                   ground_truth=dict(gt, box_gt_id=[0, 1]))
    assert r.scores.counts.tolist() == [[0] * 6] * 2 and r.scores.sums.tolist() == [[0.0] * 3] * 2
    assert bool(torch.isnan(r.scores.table()).all())
    r = sr.project_instance_points(torch.zeros((0, 4, 3), device=dev), [], cam, [(5, 7)],
                                   ground_truth=dict(gt, box_gt_id=[]))
    assert tuple(r.scores.counts.shape) == (0, 6) and tuple(r.scores.table().shape) == (0, 6)
    xyz = torch.ones((2, 4, 3), device=dev)
    for bad in (dict(gt, box_gt_id=[0]), dict(gt, box_gt_id=[0.5, 1.0]), dict(gt), dict(gt, box_gt_id=[0, 1], depth_maps=[]),
                dict(gt, box_gt_id=[0, 1], depth_maps=[torch.ones((7, 5), device=dev)]),
                dict(gt, box_gt_id=[0, 1], instance_images=[torch.zeros((5, 7), device=dev)]),
                dict(gt, box_gt_id=[0, 1], depth_maps=[torch.ones((5, 7))]),
                dict(gt, box_gt_id=[0, 1], instance_images=[torch.zeros((5, 8), dtype=torch.uint8, device=dev)])):
        with pytest.raises(_lib.InvalidArgumentError):
            sr.project_instance_points(xyz, [0, 0], cam, [(5, 7)], ground_truth=bad)


# ---- end to end: the fixture split, a small random-weight net


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_scene_score')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    val = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    test = kitti_dataset.KittiDataset(mscnn_split.config(root, has_kitti_labels=True), 'test', mscnn_label_dir=mscnn)
    return root, mscnn, model, val, test


def test_frame_ground_truth(setup):
    _, _, _, val, test = setup
    rows = np.arange(val.num_samples)
    gts = val.frame_ground_truth(rows)
    samples = val.get_sample_dict(rows, epoch=0)  # (sample_list is in split order before any shuffle)
    assert len(gts) == val.num_samples and [s['sample_name'] for s in samples] == val.sample_names
    some = 0
    for r, (gt, s) in enumerate(zip(gts, samples)):
        assert sorted(gt) == ['depth_map', 'instance_ids', 'instance_image']
        g, local = val._groups[val._group_host[r]], int(val._local_host[r])
        h, w = g.shape
        assert gt['depth_map'].dtype == torch.float32 and gt['instance_image'].dtype == torch.uint8
        assert tuple(gt['depth_map'].shape) == (h, w) == tuple(gt['instance_image'].shape) == tuple(s['rgb_image'].shape[:2])
        # views: inside the resident stacks, at the frame's place
        assert gt['depth_map'].data_ptr() == g.depth.data_ptr() + 4 * local * h * w
        assert gt['instance_image'].data_ptr() == g.inst.data_ptr() + local * h * w
        n = int(s['num_objs'])
        ids = gt['instance_ids']
        assert ids.dtype == torch.int32 and ids.is_cuda and tuple(ids.shape) == (n,)
        ids = ids.cpu().tolist()
        assert len(set(ids)) == n and all(0 <= v <= 254 for v in ids)
        image = gt['instance_image'].cpu().numpy()
        boxes = s['boxes_2d'][0:n].cpu().numpy()  # y1, x1, y2, x2
        valid = s['gt_valid_mask_maps'][0:n].reshape(n, -1).sum(1).cpu().numpy()
        for k in range(n):
            if valid[k] > 0:
                y1, x1, y2, x2 = boxes[k]
                crop = image[max(int(np.floor(y1)), 0):int(np.ceil(y2)) + 1, max(int(np.floor(x1)), 0):int(np.ceil(x2)) + 1]
                assert bool((crop == ids[k]).any()), (r, k)
                some += 1
    assert some >= 4
    assert val.frame_ground_truth([]) == []
    with pytest.raises(IndexError):
        val.frame_ground_truth([val.num_samples])
    with pytest.raises(ValueError):
        test.frame_ground_truth([0])


def _case_of_chunk(model, samples, outs):
    counts = [int(s['num_objs']) for s in samples]
    roi = tuple(model.map_roi_size)
    glob = [instance_utils.tf_inst_xyz_map_local_to_global(
        o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n], roi, o[constants.KEY_VIEW_ANG][0:n], o[constants.KEY_CENTROIDS][0:n])
        for o, n in zip(outs, counts)]
    return dict(xyz=torch.cat(glob).reshape(sum(counts), -1, 3).cpu().numpy(),
                box_frame=np.repeat(np.arange(len(samples)), counts),
                cam_p=np.stack([s['cam_p'].cpu().numpy().astype(np.float64).reshape(3, 4) for s in samples]),
                shapes=[tuple(s['rgb_image'].shape[:2]) for s in samples],
                mask=torch.cat([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)]).reshape(
                    sum(counts), -1).cpu().numpy())


def test_evaluator_scene_stats_equal_the_restatement(setup, tmp_path):
    _, _, model, val, test = setup
    plain = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path / 'plain'), batch_size=2,
                                metric_stats=True).run_once(5)
    chunks = []

    def hook(rows, samples, outs):
        case = _case_of_chunk(model, samples, outs)
        gts = val.frame_ground_truth(rows)
        gt = dict(depth_maps=[g['depth_map'].cpu().numpy() for g in gts],
                  instance_images=[g['instance_image'].cpu().numpy() for g in gts],
                  box_gt_id=torch.cat([g['instance_ids'] for g in gts]).cpu().numpy())
        chunks.append((np.asarray(rows).copy(), case, gt))
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path / 'scored'), batch_size=2,
                             metric_stats=True, scene_metrics=True, chunk_hook=hook)
    scored = ev.run_once(5)
    assert len(chunks) == (val.num_samples + 1) // 2 >= 2
    assert np.array_equal(np.concatenate([c[0] for c in chunks]), np.arange(val.num_samples))
    # the per-box scores of every chunk, then their statistics
    want = [restatement.scores(case, gt) for _, case, gt in chunks]
    counts = np.concatenate([w['counts'] for w in want])
    sums = np.concatenate([w['sums'] for w in want])
    gid = np.concatenate([gt['box_gt_id'] for _, _, gt in chunks])
    table, got_counts, got_sums, frame = ev.scene_table
    assert np.array_equal(got_counts.cpu().numpy(), counts) and len(counts) == scored['num_predictions']
    bound = np.concatenate([restatement.sum_bounds(case, gt) for _, case, gt in chunks])
    assert bool((np.abs(got_sums.cpu().numpy() - sums) <= bound).all())
    assert int(counts[:, 0].sum()) > 0 and int(counts[:, 4].sum()) > 0
    want_stats = restatement.stats(restatement.table(counts, sums, gid))
    assert list(scored['scene_stats']) == list(sr.SCENE_METRIC_NAMES)
    for k, name in enumerate(sr.SCENE_METRIC_NAMES):
        st = scored['scene_stats'][name]
        assert st['count'] == int(want_stats[k, 0]), name
        assert st['dropped'] == len(counts) - st['count'], name
        for j, key in enumerate(('mean', 'std', 'mean_abs', 'std_abs')):
            w = want_stats[k, 1 + j]
            if np.isnan(w):
                assert np.isnan(st[key]), (name, key)
            else:
                # the float32 rounding of the table's entries is 2^-24 relative each: 1e-6 relative
                assert abs(st[key] - w) <= 1e-6 * abs(w), (name, key, st[key], w)
    # the CSV: a header and one line
    path = os.path.join(str(tmp_path / 'scored'), 'metrics', val.data_split, 'scene_metrics_%s.csv' % val.data_split)
    assert scored['scene_metrics_csv'] == path
    lines = open(path).read().splitlines()
    assert len(lines) == 2 and lines[0].split(',')[0].strip() == 'step' and lines[1].split(',')[0].strip() == '5'
    fields = [c.strip() for c in lines[1].split(',')]
    assert len(fields) == 1 + 3 * 6 and fields[1] == '%d' % scored['scene_stats']['scene_mask_iou']['count']
    # everything else is what it is without scene_metrics
    assert set(scored) - set(plain) == {'scene_stats', 'scene_metrics_csv'} and 'scene_stats' not in plain
    for key in plain:
        if key in ('kitti_predictions_dir', 'metrics_csv'):
            continue
        if key == 'kitti':
            assert scored['report'] == plain['report']
            continue
        assert repr(scored[key]) == repr(plain[key]), key
    for name in val.split_sample_names:
        with open(os.path.join(plain['kitti_predictions_dir'], name + '.txt'), 'rb') as a, \
                open(os.path.join(scored['kitti_predictions_dir'], name + '.txt'), 'rb') as b:
            assert a.read() == b.read(), name
    for a, b in zip(plain['metrics_csv'], scored['metrics_csv']):
        assert open(a, 'rb').read() == open(b, 'rb').read()
    assert not os.path.exists(os.path.join(str(tmp_path / 'plain'), 'metrics', val.data_split,
                                           'scene_metrics_%s.csv' % val.data_split))
    with pytest.raises(ValueError):
        evaluator.Evaluator(model, test, THRESHOLD, scene_metrics=True)


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


def test_run_evaluation_scene_metrics_command_line(setup, tmp_path, capsys):
    """--scene-metrics on the fixture split and one saved checkpoint: the six scene lines after the report, in
    SCENE_METRIC_NAMES order, and one line in scene_metrics_<split>.csv; without the flag neither."""
    import yaml
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    from monopsr_amd.experiments import run_evaluation
    root, mscnn, _, _, _ = setup
    ckpts = str(tmp_path / 'ckpts')
    os.makedirs(ckpts)
    checkpoint_utils.save_checkpoint(os.path.join(ckpts, 'monopsr'),
                                     W.synthetic_weights(seed=92, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)), 40)
    with open(os.path.join(os.path.dirname(config_utils.__file__), '..', 'configs', 'monopsr_model_000.yaml')) as f:
        cfg = yaml.safe_load(f)
    cfg['dataset_config'] = _plain(mscnn_split.config(root))
    config_path = str(tmp_path / 'config.yaml')
    with open(config_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    common = [config_path, '--checkpoint-dir', ckpts, '--mscnn-dir', mscnn, '--width-div', '8']
    capsys.readouterr()
    assert run_evaluation.main(common + ['--predictions-dir', str(tmp_path / 'scored'), '--scene-metrics']) == 0
    printed = capsys.readouterr().out
    assert run_evaluation.main(common + ['--predictions-dir', str(tmp_path / 'plain')]) == 0
    bare = capsys.readouterr().out
    scene_lines = [l for l in printed.splitlines() if l.startswith('scene_')]
    assert [l.split()[0] for l in scene_lines] == list(sr.SCENE_METRIC_NAMES)
    assert printed.startswith('step 40\n') and 'scene_' not in bare
    assert [l for l in printed.splitlines() if not l.startswith('scene_')] == bare.splitlines()
    csv_path = os.path.join(str(tmp_path / 'scored'), 'metrics', 'val', 'scene_metrics_val.csv')
    lines = open(csv_path).read().splitlines()
    assert len(lines) == 2 and lines[1].split(',')[0].strip() == '40'
    assert int(lines[1].split(',')[1]) == int(scene_lines[0].split()[2])
    assert not os.path.exists(os.path.join(str(tmp_path / 'plain'), 'metrics', 'val', 'scene_metrics_val.csv'))

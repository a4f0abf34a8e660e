"""csrc/scene.hip and core/scene_reconstruction.py on the GPU against tests/scene_restatement.py: every comparison is
exact (array_equal; depths as bits).  The projection runs in fp64 without contraction, so there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import mscnn_split
import scene_cases
import scene_restatement
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import scene_reconstruction as sr
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
FIELDS = ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'kept_per_box', 'visible_per_box')


def _run(case, visible_only=False):
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    images = case.get('images')
    return sr.project_instance_points(
        t(np.asarray(case['xyz'], np.float32)), case['box_frame'], case['cam_p'], case['shapes'],
        images=None if images is None else [t(im) for im in images],
        valid_mask=None if case.get('mask') is None else t(np.asarray(case['mask'], np.float32)),
        keep=None if case.get('keep') is None else t(np.asarray(case['keep'], np.int32)), visible_only=visible_only)


def _host(result):
    out = {k: getattr(result, k) for k in FIELDS}
    out = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    out['depth_maps'] = [d.cpu().numpy() for d in result.depth_maps]
    out['instance_maps'] = [d.cpu().numpy() for d in result.instance_maps]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what=''):
    for k in FIELDS:
        if want[k] is None:
            assert got[k] is None, (what, k)
        elif k in ('xyz', 'rgb'):
            assert got[k].shape == want[k].shape and np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
        else:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k)
    assert len(got['depth_maps']) == len(want['depth_maps']) == len(got['instance_maps'])
    for f, (d, i) in enumerate(zip(want['depth_maps'], want['instance_maps'])):
        assert got['depth_maps'][f].shape == d.shape and np.array_equal(_bits(got['depth_maps'][f]), _bits(d)), (what, f)
        assert got['instance_maps'][f].dtype == np.uint8 and np.array_equal(got['instance_maps'][f], i), (what, f)


@pytest.mark.parametrize('visible_only', [False, True])
@pytest.mark.parametrize('name', scene_cases.NAMES)
def test_catalogue_equals_the_restatement(name, visible_only):
    got = _host(_run(scene_cases.case(name), visible_only))
    want = scene_cases.expected(name, visible_only)
    _assert_same(got, want, name)
    m = int(want['visible_per_box'].sum() if visible_only else want['kept_per_box'].sum())
    assert got['xyz'].shape == (m, 3) and got['frame_offset'][-1] == m


def test_colours_come_from_the_points_pixel():
    """The image encodes (frame, row, col, channel): the gathered colour names the pixel the point fell on."""
    case = scene_cases.case('random_b70_p35')
    r = _run(case)
    got = _host(r)
    assert len(got['rgb']) > 50
    frame = np.asarray(case['box_frame'])[got['box']]
    w = np.asarray([s[1] for s in case['shapes']])[frame]
    row, col = got['pixel'] // w, got['pixel'] % w
    for c in range(3):
        assert np.array_equal(got['rgb'][:, c], (((frame * 64 + row) * 64 + col) * 4 + c).astype(np.float32))
    # the per-frame views: ordinals within the frame, the frame's own maps
    for f in range(3):
        fr = r.frame(f)
        lo, hi = got['frame_offset'][f], got['frame_offset'][f + 1]
        first = int(np.searchsorted(np.asarray(case['box_frame']), f))
        assert np.array_equal(fr.box.cpu().numpy(), got['box'][lo:hi] - first)
        assert np.array_equal(fr.xyz.cpu().numpy(), got['xyz'][lo:hi], equal_nan=True)
        assert fr.depth_map.data_ptr() == r.depth_maps[f].data_ptr()
        seen = set(np.unique(got['instance_maps'][f]).tolist()) - {255}
        assert seen <= set(np.unique(fr.box.cpu().numpy()).tolist())


def test_two_runs_return_the_same_bytes():
    case = scene_cases.case(scene_cases.DETERMINISM_CASE)
    for visible_only in (False, True):
        a, b = _host(_run(case, visible_only)), _host(_run(case, visible_only))
        for k in FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), k
        for x, y in zip(a['depth_maps'] + a['instance_maps'], b['depth_maps'] + b['instance_maps']):
            assert x.tobytes() == y.tobytes()
        _assert_same(a, scene_cases.expected(scene_cases.DETERMINISM_CASE, visible_only))


def test_poisoned_buffers_change_nothing(monkeypatch):
    """Every buffer the wrapper allocates (the workspace and the outputs) filled with 0xFF bytes beforehand -- NaN in
    every float, -1 in every index, the empty key in every z-buffer cell -- and then with 0x00 bytes -- a depth 0, point
    0 key everywhere: the results are those of the restatement, and nothing past the M rows is read back."""
    real = sr._empty
    for fill in (255, 0):
        def poisoned(shape, dtype, device, fill=fill):
            t = real(shape, dtype, device)
            if t.numel():
                t.view(torch.uint8).fill_(fill)
            return t
        monkeypatch.setattr(sr, '_empty', poisoned)
        for name in ('zbuffer_three_boxes', 'dropped', 'random_b3_p300', scene_cases.DETERMINISM_CASE):
            for visible_only in (False, True):
                _assert_same(_host(_run(scene_cases.case(name), visible_only)),
                             scene_cases.expected(name, visible_only), (name, fill))


def test_box_limits_and_bad_arguments():
    """255 boxes in one frame are accepted (the catalogue's boxes_255), 256 are refused on the host before a launch;
    so is everything else that is wrong."""
    with pytest.raises(_lib.InvalidArgumentError, match='255'):
        _run(scene_cases.many_boxes_case(256))
    # the C entry point's own refusal, with valid device pointers
    dev = torch.device('cuda', 0)
    bf = np.zeros(256, np.int32)
    bf_d = torch.from_numpy(bf).to(dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    depth = torch.zeros(64, device=dev)
    inst = torch.zeros(64, dtype=torch.uint8, device=dev)
    import ctypes
    status = _lib.lib().mpsr_scene_resolve(_lib.ptr(bf_d), bf.ctypes.data_as(ctypes.c_void_p), 1, 64, 256, 1,
                                           _lib.ptr(ws), ws.numel(), _lib.ptr(depth), _lib.ptr(inst), _lib.stream())
    assert status == 1 and b'more than 255' in _lib.lib().mpsr_last_error()
    case = scene_cases.case('zbuffer_three_boxes')
    for bad in (dict(box_frame=[0, 1, 0]), dict(box_frame=[0, 0]), dict(box_frame=[0, 0, 1]), dict(shapes=[(0, 7)]),
                dict(cam_p=np.zeros((2, 3, 4))), dict(mask=np.ones((3, 4), np.float32)), dict(keep=[1, 1]),
                dict(images=[])):
        with pytest.raises(_lib.InvalidArgumentError):
            _run(dict(case, **bad))
    with pytest.raises(_lib.InvalidArgumentError):
        sr.project_instance_points(torch.zeros((2, 5, 4), device=dev), [0, 0], case['cam_p'], case['shapes'])
    with pytest.raises(_lib.MpsrError):
        sr.project_instance_points(torch.zeros((2, 5, 3)), [0, 0], case['cam_p'], case['shapes'])


def test_empty_inputs():
    dev = torch.device('cuda', 0)
    cam = scene_cases.pow2_camera(2.0, 0.0, 0.0)[None]
    for xyz, bf in ((torch.zeros((0, 4, 3), device=dev), []), (torch.zeros((2, 0, 3), device=dev), [0, 0])):
        r = sr.project_instance_points(xyz, bf, cam, [(5, 7)], images=[torch.ones((5, 7, 3), device=dev)])
        assert r.xyz.shape == (0, 3) and r.rgb.shape == (0, 3) and r.box.shape == (0,) and r.pixel.shape == (0,)
        assert r.frame_offset.tolist() == [0, 0] and r.kept_per_box.tolist() == [0] * len(bf)
        assert r.depth_maps[0].shape == (5, 7) and not bool(r.depth_maps[0].any())
        assert bool((r.instance_maps[0] == 255).all())
    r = sr.project_instance_points(torch.zeros((0, 4, 3), device=dev), [], np.zeros((0, 3, 4)), [])
    assert r.xyz.shape == (0, 3) and r.depth_maps == [] and r.frame_offset.tolist() == [0] and r.rgb is None


def test_depth_map_equals_the_lidar_projection_on_distinct_pixels():
    """Independent code: depth_map_utils.project_depths, checked bit for bit against the reference elsewhere.  On a cloud
    whose kept points fall on distinct pixels with 0 < z < 100 (so that neither rule for duplicates nor the clamp at
    max_depth applies) both must render the same map."""
    case = scene_cases.distinct_pixels_case()
    got = _host(_run(case))
    pix = got['pixel']
    assert len(pix) == 40 == len(np.unique(pix)) and got['kept_per_box'].tolist() == [40]
    want = depth_map_utils.project_depths(case['xyz'][0].T, case['cam_p'][0], case['shapes'][0])
    assert int((want > 0).sum()) == 40 and float(want.max()) < 100.0
    assert np.array_equal(_bits(got['depth_maps'][0]), _bits(want))
    _assert_same(got, scene_restatement.scene(case))


def test_save_frame_reads_back(tmp_path):
    """Depths of 0.25 .. 12 m on small frames: the PLY returns the tensors, the depth PNG the map through
    save_depth_map's quantisation (1/256 m, values under 0.1 m read as 0), the instance PNG the map."""
    dirs = sr.scene_output_dirs(str(tmp_path))
    for name in ('zbuffer_three_boxes', 'random_b70_p35', 'no_images'):
        r = _run(scene_cases.case(name))
        want = scene_cases.expected(name)
        for f in range(r.num_frames):
            fr = r.frame(f)
            ply, depth_png, inst_png = sr.save_frame(dirs, '%s_%d' % (name, f), fr)
            xyz, rgb, box = sr.read_ply(ply)
            lo, hi = want['frame_offset'][f], want['frame_offset'][f + 1]
            assert np.array_equal(_bits(xyz), _bits(want['xyz'][lo:hi]))
            first = int(np.searchsorted(np.asarray(scene_cases.case(name)['box_frame']), f))
            assert np.array_equal(box, want['box'][lo:hi] - first)
            if want['rgb'] is None:
                assert not rgb.any()
            else:
                assert np.array_equal(rgb, sr.colours_to_uint8(want['rgb'][lo:hi]))
            depth = want['depth_maps'][f]
            assert float(depth.max()) < 256.0
            q = (depth * 256.0).astype(np.uint16) / 256.0
            q[q < 0.1] = 0.0
            got = depth_map_utils.read_depth_map(depth_png)
            assert np.array_equal(got, q.astype(np.float32))
            assert bool((got > 0).any()) == bool((depth > 0).any())
            assert np.array_equal(instance_utils.read_instance_image(inst_png), want['instance_maps'][f])


# ---- end to end: the fixture split, a small random-weight net


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_scene')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    val = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    test = kitti_dataset.KittiDataset(mscnn_split.config(root, has_kitti_labels=True), 'test', mscnn_label_dir=mscnn)
    return root, mscnn, model, val, test


def _case_of_chunk(model, samples, outs, min_score, with_mask):
    """The restatement's input from the same outs: the local maps placed by the existing geometry kernel."""
    counts = [int(s['num_objs']) for s in samples]
    roi = tuple(model.map_roi_size)
    glob = [instance_utils.tf_inst_xyz_map_local_to_global(
        o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n], roi, o[constants.KEY_VIEW_ANG][0:n], o[constants.KEY_CENTROIDS][0:n])
        for o, n in zip(outs, counts)]
    case = dict(xyz=torch.cat(glob).reshape(sum(counts), -1, 3).cpu().numpy(),
                box_frame=np.repeat(np.arange(len(samples)), counts),
                cam_p=np.stack([s['cam_p'].cpu().numpy().astype(np.float64).reshape(3, 4) for s in samples]),
                shapes=[tuple(s['rgb_image'].shape[:2]) for s in samples],
                images=[s['rgb_image'].cpu().numpy() for s in samples])
    if with_mask:
        case['mask'] = torch.cat([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)]).reshape(
            sum(counts), -1).cpu().numpy()
    if min_score is not None:
        case['keep'] = (torch.cat([s['label_scores'][0:n] for s, n in zip(samples, counts)]).cpu().numpy()
                        >= np.float32(min_score)).astype(np.int32)
    return case


@pytest.mark.parametrize('mode,min_score,visible_only', [('val', None, False), ('test', 0.6, True)])
def test_reconstruct_frames_equals_the_restatement(setup, mode, min_score, visible_only):
    _, _, model, val, test = setup
    ds = val if mode == 'val' else test
    samples = ds.get_sample_dict(np.arange(min(ds.num_samples, 3)), epoch=0)
    with torch.no_grad():
        outs = model.build_batch(samples)
        got = _host(sr.reconstruct_frames(model, samples, outs, min_score=min_score, visible_only=visible_only))
        case = _case_of_chunk(model, samples, outs, min_score, with_mask=mode == 'val')
    assert (samples[0].get('gt_valid_mask_maps') is not None) == (mode == 'val')
    want = scene_restatement.scene(case, visible_only)
    _assert_same(got, want, mode)
    if min_score is not None:
        assert 0 < int(case['keep'].sum()) < len(case['keep'])
        assert bool((want['kept_per_box'][case['keep'] == 0] == 0).all())


def test_evaluator_hook_writes_the_scenes_and_changes_nothing(setup, tmp_path):
    from monopsr_amd.experiments import run_inference
    _, _, model, _, test = setup
    plain = evaluator.Evaluator(model, test, THRESHOLD, predictions_base_dir=str(tmp_path / 'plain'),
                                batch_size=2).run_once(5)
    seen, frames = [], {}
    writer = run_inference.SceneWriter(model, run_inference.scene_dir(str(tmp_path / 'out'), test.data_split, 5),
                                       min_score=THRESHOLD)

    def hook(rows, samples, outs):
        seen.append((np.asarray(rows).copy(), [s['sample_name'] for s in samples]))
        scene = sr.reconstruct_frames(model, samples, outs, min_score=THRESHOLD)
        for f, s in enumerate(samples):
            fr = scene.frame(f)
            frames[s['sample_name']] = dict(num_objs=int(s['num_objs']), **{
                k: getattr(fr, k).cpu().numpy() for k in ('xyz', 'rgb', 'box', 'depth_map', 'instance_map')})
        writer(rows, samples, outs)
    ev = evaluator.Evaluator(model, test, THRESHOLD, predictions_base_dir=str(tmp_path / 'out'), batch_size=2,
                             chunk_hook=hook)
    hooked = ev.run_once(5)
    writer.finish(test)
    # the pass itself: the same result, the same label files
    assert hooked['report'] == plain['report'] and hooked['report'] is not None
    for key in ('num_frames', 'num_detections', 'num_predictions', 'num_frames_with_detections'):
        assert hooked[key] == plain[key]
    for name in test.split_sample_names:
        with open(os.path.join(plain['kitti_predictions_dir'], name + '.txt'), 'rb') as a, \
                open(os.path.join(hooked['kitti_predictions_dir'], name + '.txt'), 'rb') as b:
            assert a.read() == b.read(), name
    # the hook saw every sample once, in the order of the pass, in chunks of batch_size
    assert np.array_equal(np.concatenate([r for r, _ in seen]), np.arange(test.num_samples))
    assert [n for _, names in seen for n in names] == list(test.sample_names)
    assert all(len(names) <= 2 for _, names in seen)
    # one PLY, one depth PNG, one instance PNG per frame of the split
    base = os.path.join(str(tmp_path / 'out'), 'scenes', test.data_split, '5')
    for kind, ext in (('points', '.ply'), ('depth', '.png'), ('instances', '.png')):
        assert sorted(os.listdir(os.path.join(base, kind))) == sorted(n + ext for n in test.split_sample_names)
    assert sorted(writer.names) == sorted(test.split_sample_names)
    # reading the files back gives the tensors of the same chunks (the depth through save_depth_map's quantisation)
    empty = set(test.split_sample_names) - set(test.sample_names)
    assert '000002' in empty and set(frames) == set(test.sample_names)
    for name, fr in frames.items():
        xyz, rgb, box = sr.read_ply(os.path.join(base, 'points', name + '.ply'))
        assert np.array_equal(_bits(xyz), _bits(fr['xyz'])) and len(xyz) > 0, name
        assert np.array_equal(rgb, sr.colours_to_uint8(fr['rgb'])), name
        assert np.array_equal(box, fr['box']), name
        depth = fr['depth_map']
        # (the random-weight net places points kilometres away; save_frame stores what the 16 bits cannot hold as 0)
        want = (np.where(depth < 256.0, depth, np.float32(0.0)) * 256.0).astype(np.uint16) / 256.0
        want[want < 0.1] = 0.0
        got = depth_map_utils.read_depth_map(os.path.join(base, 'depth', name + '.png'))
        assert np.array_equal(got, want.astype(np.float32)) and bool((depth > 0).any()), name
        inst = instance_utils.read_instance_image(os.path.join(base, 'instances', name + '.png'))
        assert np.array_equal(inst, fr['instance_map']), name
        assert set(np.unique(inst).tolist()) - {255} <= set(range(fr['num_objs'])), name
        assert np.array_equal(inst != 255, depth > 0), name
    for name in empty:
        assert sr.read_ply(os.path.join(base, 'points', name + '.ply'))[0].shape == (0, 3)
        assert bool((instance_utils.read_instance_image(os.path.join(base, 'instances', name + '.png')) == 255).all())
        assert not depth_map_utils.read_depth_map(os.path.join(base, 'depth', name + '.png')).any()


def test_run_once_without_the_hook_is_what_it_was(setup, tmp_path):
    """The same setup as tests/test_evaluator_gpu.py: without a hook the result is the host path's."""
    from monopsr_amd.core import kitti_eval
    root, _, model, val, _ = setup
    ev = evaluator.Evaluator(model, val, THRESHOLD, batch_size=2, iou='low')
    assert ev.chunk_hook is None
    result = ev.run_once(7)
    empty = (np.zeros((0, 9), np.float32), np.zeros((0, 7), np.float32))
    predictions = {name: empty for name in val.split_sample_names}
    samples = val.get_sample_dict(np.arange(val.num_samples), epoch=0)
    for s, out in zip(samples, model.build_batch(samples)):
        sample_dict = {constants.SAMPLE_NUM_OBJS: s['num_objs'], constants.SAMPLE_CAM_P: s['cam_p'].cpu().numpy(),
                       constants.SAMPLE_LABEL_SCORES: s['label_scores'].cpu().numpy(),
                       constants.SAMPLE_LABEL_BOXES_2D: s['boxes_2d'].cpu().numpy(),
                       'image_shape': tuple(s['rgb_image'].shape)}
        pred = model.format_predictions(model.output_types, out, sample_dict)
        predictions[s['sample_name']] = (pred[constants.KEY_BOX_3D], pred[constants.KEY_BOX_2D])
    want = kitti_eval.evaluate_predictions(predictions, val.classes, THRESHOLD,
                                           os.path.join(root, 'training', 'label_2'), False, val.frame_info, iou='low')
    assert result['report'] == kitti_eval.format_report(want, 7)
    assert result['num_frames'] == 6 and result['num_predictions'] == 9


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


def test_run_inference_command_line(setup, tmp_path, capsys):
    """The command line on the fixture split and a saved checkpoint: the label files an Evaluator writes for the same
    'test'-mode dataset and checkpoint, the AP report (the split has labels) and three scene files per frame under
    scenes/<split>/<step>/; --no-scenes writes the label files only."""
    import yaml
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    from monopsr_amd.experiments import run_inference
    root, mscnn, model, _, test = setup
    os.makedirs(str(tmp_path / 'ckpts'))
    prefix = checkpoint_utils.save_checkpoint(
        os.path.join(str(tmp_path / 'ckpts'), 'monopsr'),
        W.synthetic_weights(seed=92, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)), 40)
    with open(os.path.join(os.path.dirname(config_utils.__file__), '..', 'configs', 'monopsr_model_000.yaml')) as f:
        cfg = yaml.safe_load(f)
    cfg['dataset_config'] = _plain(mscnn_split.config(root))
    config_path = str(tmp_path / 'config.yaml')
    with open(config_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    out = str(tmp_path / 'out')
    capsys.readouterr()
    assert run_inference.main([config_path, prefix, '--mscnn-dir', mscnn, '--output-dir', out, '--width-div', '8']) == 0
    printed = capsys.readouterr().out
    net_before = model.device_net
    try:
        want = evaluator.Evaluator(model, test, THRESHOLD, predictions_base_dir=str(tmp_path / 'want')) \
            .run_checkpoint_once(prefix, width_div=8)
    finally:
        model.device_net = net_before
    assert want['global_step'] == 40 and want['report'] and printed.startswith(want['report'])
    assert '%d scenes' % len(test.split_sample_names) in printed
    got_dir = evaluator.evaluator_utils.kitti_output_dir(out, 'val', THRESHOLD, 40)
    assert sorted(os.listdir(got_dir)) == sorted(n + '.txt' for n in test.split_sample_names)
    for name in test.split_sample_names:
        with open(os.path.join(got_dir, name + '.txt'), 'rb') as a, \
                open(os.path.join(want['kitti_predictions_dir'], name + '.txt'), 'rb') as b:
            assert a.read() == b.read(), name
    base = os.path.join(out, 'scenes', 'val', '40')
    for kind, ext in (('points', '.ply'), ('depth', '.png'), ('instances', '.png')):
        assert sorted(os.listdir(os.path.join(base, kind))) == sorted(n + ext for n in test.split_sample_names)
    assert any(len(sr.read_ply(os.path.join(base, 'points', n + '.ply'))[0]) for n in test.sample_names)
    bare = str(tmp_path / 'bare')
    assert run_inference.main([config_path, prefix, '--mscnn-dir', mscnn, '--output-dir', bare, '--width-div', '8',
                               '--no-scenes']) == 0
    assert not os.path.exists(os.path.join(bare, 'scenes'))
    assert os.path.isdir(evaluator.evaluator_utils.kitti_output_dir(bare, 'val', THRESHOLD, 40))

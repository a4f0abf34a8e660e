"""The surface rendering of csrc/scene.hip and what is built on it, on the GPU against tests/surface_restatement.py.
Every comparison is exact: depths as bits, counts as integers, the fp64 sums as bits."""
import os

import numpy as np
import pytest
import torch

import mscnn_split
import surface_cases as cases
import surface_restatement as restatement
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import scene_reconstruction as sr
from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
# the end-to-end tests: a random-weight net's maps are no surfaces, so no depth limit, and a span the restatement's
# per-pixel loops can afford
SURFACES = dict(max_edge_dz=float('inf'), max_span_px=6)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _device_ground_truth(gt, dev):
    """Each frame's maps as slice 1 of a stack of two: off every alignment (tests/test_scene_score_gpu.py)."""
    depths, insts = [], []
    for d, im in zip(gt['depth_maps'], gt['instance_images']):
        depths.append(torch.from_numpy(np.stack([np.full_like(d, 1.0), d])).to(dev)[1])
        insts.append(torch.from_numpy(np.stack([np.full_like(im, 7), im])).to(dev)[1])
    return dict(depth_maps=depths, instance_images=insts, box_gt_id=np.asarray(gt['box_gt_id']))


def _render_case(case, gt=None, want_tri=True):
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return sr.render_instance_surfaces(
        t(np.asarray(case['xyz'], np.float32)), case['box_frame'], case['cam_p'], case['shapes'],
        valid_mask=None if case.get('mask') is None else t(np.asarray(case['mask'], np.float32)),
        keep=None if case.get('keep') is None else t(np.asarray(case['keep'], np.int32)),
        max_edge_dz=case.get('max_edge_dz', 1.0), max_span_px=case.get('max_span_px', 64),
        ground_truth=None if gt is None else _device_ground_truth(gt, dev), want_tri=want_tri)


def _run(name, with_gt=True, want_tri=True):
    return _render_case(cases.case(name), cases.ground_truth(name) if with_gt else None, want_tri)


def _assert_rendering(got, want, what=''):
    assert len(got.depth_maps) == len(want['depth_maps']) == len(got.instance_maps)
    for f in range(len(want['depth_maps'])):
        d, inst = got.depth_maps[f], got.instance_maps[f]
        assert d.dtype == torch.float32 and inst.dtype == torch.uint8
        assert tuple(d.shape) == want['depth_maps'][f].shape == tuple(inst.shape)
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(want['depth_maps'][f])), (what, f)
        assert np.array_equal(inst.cpu().numpy(), want['instance_maps'][f]), (what, f)
        if got.tri_maps is not None:
            assert got.tri_maps[f].dtype == torch.int32
            assert np.array_equal(got.tri_maps[f].cpu().numpy(), want['tri_maps'][f]), (what, f)
    assert got.tris_per_box.dtype == torch.int32 and got.pixels_per_box.dtype == torch.int32
    assert np.array_equal(got.tris_per_box.cpu().numpy(), want['tris']), what
    first = np.searchsorted(np.asarray(want['box_frame']), np.arange(len(want['depth_maps'])))
    pixels = np.zeros(len(want['tris']), np.int64)
    for f, inst in enumerate(want['instance_maps']):
        k, n = np.unique(inst[inst != 255], return_counts=True)
        pixels[first[f] + k.astype(np.int64)] += n
    assert np.array_equal(got.pixels_per_box.cpu().numpy(), pixels), what


def _assert_scores(got, want, what=''):
    s = got.scores
    assert s.counts.dtype == torch.int32 and s.sums.dtype == torch.float64
    counts, sums = s.counts.cpu().numpy(), s.sums.cpu().numpy()
    assert counts.shape == want['counts'].shape and sums.shape == want['sums'].shape
    assert np.array_equal(counts, want['counts']), what
    assert sums.tobytes() == want['sums'].tobytes(), (what, sums, want['sums'])
    return counts, sums


def _assert_case(name, got, what=''):
    _assert_rendering(got, dict(cases.expected(name), box_frame=cases.case(name)['box_frame']), (name, what))
    if got.scores is not None:
        return _assert_scores(got, cases.expected_scores(name), (name, what))


@pytest.mark.parametrize('name', cases.NAMES)
def test_catalogue_equals_the_restatement(name):
    got = _run(name)
    counts, sums = _assert_case(name, got)
    assert np.array_equal(counts[:, 0], got.tris_per_box.cpu().numpy())
    assert np.array_equal(counts[:, 1], got.pixels_per_box.cpu().numpy())
    table = got.scores.table().cpu().numpy()
    want = restatement.table(counts, sums, cases.ground_truth(name)['box_gt_id'])
    # fp64 quotients and roots of the same counts and sums, rounded once to float32: one float32 ulp at the most apart
    assert table.dtype == np.float32 and table.shape == want.shape and np.array_equal(np.isnan(table), np.isnan(want))
    assert bool((np.abs(np.nan_to_num(table) - np.nan_to_num(want)) <= 2.0 ** -23 * np.abs(np.nan_to_num(want))).all())


@pytest.mark.parametrize('name', cases.DETERMINISM_CASES)
def test_two_runs_return_the_same_bytes(name):
    a, b = _run(name), _run(name)
    for x, y in zip(a.depth_maps + a.instance_maps + a.tri_maps, b.depth_maps + b.instance_maps + b.tri_maps):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    for key in ('counts', 'sums'):
        assert getattr(a.scores, key).cpu().numpy().tobytes() == getattr(b.scores, key).cpu().numpy().tobytes()
    assert int(a.scores.counts[:, 4].sum()) > 0


def test_poisoned_buffers_change_nothing(monkeypatch):
    """Every buffer the wrapper allocates (the workspace, the histogram scratch and the outputs) filled with 0xFF bytes
    beforehand and then with 0x00 bytes: the maps and the scores are the restatement's."""
    real = sr._empty
    for fill in (255, 0):
        def poisoned(shape, dtype, device, fill=fill):
            t = real(shape, dtype, device)
            if t.numel():
                t.view(torch.uint8).fill_(fill)
            return t
        monkeypatch.setattr(sr, '_empty', poisoned)
        for name in ('cell_2x2', 'invalid_vertices', 'off_image', 'random_b12_5x4', 'big_48x48'):
            _assert_case(name, _run(name), fill)
            _assert_case(name, _run(name, with_gt=False, want_tri=False), fill)


def test_without_ground_truth_and_without_triangle_maps():
    for name in ('identical_boxes', 'random_b12_5x4', 'degenerate'):
        got = _run(name, with_gt=False, want_tri=False)
        assert got.scores is None and got.tri_maps is None and got.num_frames == len(cases.case(name)['shapes'])
        _assert_case(name, got)
        assert got.frame(0).tri_map is None and got.frame(0).depth_map is got.depth_maps[0]
    got = _run('identical_boxes', with_gt=False)
    assert got.pixels_per_box.tolist()[1] == 0 and got.pixels_per_box.tolist()[0] > 0


def test_surface_fills_the_mask_the_points_cannot():
    """The point of the feature.  One box whose 48 x 48 map is a fronto-parallel plane with vertices two pixels apart
    and a ground-truth instance that is exactly the rectangle it spans: the surface's IoU is 1, the points' is bounded
    by their number."""
    case, gt = cases.case('feature_94'), cases.ground_truth('feature_94')
    dev = torch.device('cuda', 0)
    surface = _run('feature_94')
    table = surface.scores.table().cpu().numpy()
    assert sr.SURFACE_METRIC_NAMES[0] == 'surface_mask_iou' and table[0, 0] == 1.0
    assert table[0].tolist() == [1.0, 1.0, 1.0, -0.25, 0.25, 0.25]
    assert surface.scores.counts[0].tolist() == [4418, 8836, 8836, 8836, 8836]
    points = sr.project_instance_points(torch.from_numpy(case['xyz']).to(dev), case['box_frame'], case['cam_p'],
                                        case['shapes'], ground_truth=_device_ground_truth(gt, dev))
    iou = float(points.scores.table()[0, 0])
    assert sr.SCENE_METRIC_NAMES[0] == 'scene_mask_iou' and 0.0 < iou <= 2304.0 / 8836.0
    assert points.scores.counts[0].tolist()[2] == 2304 and points.scores.counts[0].tolist()[4] == 8836


def test_surface_depth_equals_point_depth_at_vertex_pixels():
    """Vertices on integer pixels, depths that vary from vertex to vertex, no triangle dropped: at the pixel of every
    interior vertex the surface's depth is the point z-buffer's, the vertex's own z, bit for bit."""
    rng = np.random.default_rng(5)
    i, j = np.meshgrid(np.arange(7), np.arange(9), indexing='ij')
    z = 5.0 + 0.3 * np.sin(i) + 0.2 * np.cos(2.0 * j) + rng.uniform(-0.1, 0.1, i.shape)
    case = cases._case([cases.at_pixels(2 + 3 * j, 1 + 2 * i, z)], [0], [(16, 30)], max_edge_dz=cases.INF)
    surface = _render_case(case)
    assert surface.tris_per_box.tolist() == [2 * 6 * 8]
    dev = torch.device('cuda', 0)
    points = sr.project_instance_points(torch.from_numpy(case['xyz']).to(dev), case['box_frame'], case['cam_p'],
                                        case['shapes'])
    assert points.visible_per_box.tolist() == [63]
    sd, pd = surface.depth_maps[0].cpu().numpy(), points.depth_maps[0].cpu().numpy()
    rows, cols = (1 + 2 * i)[1:-1, 1:-1], (2 + 3 * j)[1:-1, 1:-1]
    assert np.array_equal(_bits(sd[rows, cols]), _bits(pd[rows, cols]))
    assert np.array_equal(_bits(pd[rows, cols]), _bits(case['xyz'][0, 1:-1, 1:-1, 2])) and len(np.unique(pd[rows, cols])) == 35
    _assert_rendering(surface, dict(restatement.render(case), box_frame=case['box_frame']))


def test_arguments_and_empty_inputs():
    dev = torch.device('cuda', 0)
    cam = cases.scene_cases.pow2_camera(4.0, 0.0, 0.0)[None]
    maps = torch.from_numpy(cases.plane(1, 1, 2, 2, 3, 3)[None]).to(dev)
    for bad in (dict(max_edge_dz=0.0), dict(max_edge_dz=-1.0), dict(max_edge_dz=float('nan')), dict(max_span_px=0),
                dict(max_span_px=1025)):
        with pytest.raises(_lib.InvalidArgumentError):
            sr.render_instance_surfaces(maps, [0], cam, [(8, 8)], **bad)
    for shape in ((1, 1, 3, 3), (1, 3, 1, 3), (1, 9, 3), (1, 3, 3, 2)):
        with pytest.raises(_lib.InvalidArgumentError):
            sr.render_instance_surfaces(torch.zeros(shape, device=dev), [0], cam, [(8, 8)])
    with pytest.raises(_lib.MpsrError):
        sr.render_instance_surfaces(maps.cpu(), [0], cam, [(8, 8)])
    with pytest.raises(_lib.InvalidArgumentError):
        sr.render_instance_surfaces(maps, [1], cam, [(8, 8)])
    got = sr.render_instance_surfaces(maps[:0], [], cam, [(8, 8)], want_tri=True,
                                      ground_truth=dict(depth_maps=[torch.ones((8, 8), device=dev)],
                                                        instance_images=[torch.zeros((8, 8), dtype=torch.uint8, device=dev)],
                                                        box_gt_id=[]))
    assert not got.depth_maps[0].any() and bool((got.instance_maps[0] == 255).all()) and bool((got.tri_maps[0] == -1).all())
    assert tuple(got.scores.counts.shape) == (0, 5) and tuple(got.scores.table().shape) == (0, 6)
    assert tuple(got.tris_per_box.shape) == (0,) == tuple(got.pixels_per_box.shape)
    # the device argument: where the maps are is the default
    assert sr.render_instance_surfaces(maps, [0], cam, [(8, 8)], device=dev).pixels_per_box.tolist() == [16]
    inf = sr.render_instance_surfaces(maps, [0], cam, [(8, 8)], max_edge_dz=float('inf'), max_span_px=1024)
    assert inf.tris_per_box.tolist() == [8]


# ---- end to end: the fixture split, a small random-weight net


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_scene_surface')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    val = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    test = kitti_dataset.KittiDataset(mscnn_split.config(root, has_kitti_labels=True), 'test', mscnn_label_dir=mscnn)
    return root, mscnn, model, val, test


def _case_of_chunk(model, samples, outs, min_score, with_mask, options):
    """The restatement's input from the same network outputs: the local maps placed by the existing geometry kernel."""
    counts = [int(s['num_objs']) for s in samples]
    roi = tuple(model.map_roi_size)
    glob = [instance_utils.tf_inst_xyz_map_local_to_global(
        o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n], roi, o[constants.KEY_VIEW_ANG][0:n], o[constants.KEY_CENTROIDS][0:n])
        for o, n in zip(outs, counts)]
    case = dict(xyz=torch.cat(glob).reshape((sum(counts),) + roi + (3,)).cpu().numpy(),
                box_frame=np.repeat(np.arange(len(samples)), counts),
                cam_p=np.stack([s['cam_p'].cpu().numpy().astype(np.float64).reshape(3, 4) for s in samples]),
                shapes=[tuple(s['rgb_image'].shape[:2]) for s in samples], **options)
    if with_mask:
        case['mask'] = torch.cat([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)]).reshape(
            (sum(counts),) + roi).cpu().numpy()
    if min_score is not None:
        case['keep'] = (torch.cat([s['label_scores'][0:n] for s, n in zip(samples, counts)]).cpu().numpy()
                        >= np.float32(min_score)).astype(np.int32)
    return case


def _ground_truth_of(ds, rows):
    gts = ds.frame_ground_truth(rows)
    return dict(depth_maps=[g['depth_map'] for g in gts], instance_images=[g['instance_image'] for g in gts],
                box_gt_id=torch.cat([g['instance_ids'] for g in gts]))


def test_reconstruct_frames_with_surfaces_equals_the_restatement(setup):
    _, _, model, val, _ = setup
    rows = np.arange(min(val.num_samples, 3))
    samples = val.get_sample_dict(rows, epoch=0)
    gt = _ground_truth_of(val, rows)
    with torch.no_grad():
        outs = model.build_batch(samples)
        plain = sr.reconstruct_frames(model, samples, outs, ground_truth=gt)
        both = sr.reconstruct_frames(model, samples, outs, ground_truth=gt, surfaces=SURFACES)
        case = _case_of_chunk(model, samples, outs, None, True, SURFACES)
    # surfaces=None is what it was, and asking for the surfaces changes nothing else
    assert plain.surfaces is None and isinstance(both.surfaces, sr.SurfaceResult)
    for key in ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'kept_per_box', 'visible_per_box'):
        assert getattr(plain, key).cpu().numpy().tobytes() == getattr(both, key).cpu().numpy().tobytes(), key
    for x, y in zip(plain.depth_maps + plain.instance_maps, both.depth_maps + both.instance_maps):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert plain.scores.counts.cpu().numpy().tobytes() == both.scores.counts.cpu().numpy().tobytes()
    assert plain.scores.sums.cpu().numpy().tobytes() == both.scores.sums.cpu().numpy().tobytes()
    # the surfaces are the restatement's of the same network outputs
    want = restatement.render(case)
    _assert_rendering(both.surfaces, dict(want, box_frame=case['box_frame']))
    host_gt = dict(depth_maps=[d.cpu().numpy() for d in gt['depth_maps']],
                   instance_images=[im.cpu().numpy() for im in gt['instance_images']],
                   box_gt_id=gt['box_gt_id'].cpu().numpy())
    counts, _ = _assert_scores(both.surfaces, restatement.scores(case, host_gt, want))
    assert int(counts[:, 0].sum()) > 0 and int(counts[:, 1].sum()) > 0 and int(counts[:, 3].sum()) > 0
    with pytest.raises(ValueError):
        sr.reconstruct_frames(model, samples, outs, surfaces=dict(max_edge_dx=1.0))


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


@pytest.fixture(scope='module')
def command_line(setup, tmp_path_factory):
    """A saved checkpoint and a config file for the two command lines."""
    import yaml
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    root, mscnn, _, _, _ = setup
    base = tmp_path_factory.mktemp('surface_cli')
    ckpts = str(base / 'ckpts')
    os.makedirs(ckpts)
    prefix = checkpoint_utils.save_checkpoint(
        os.path.join(ckpts, 'monopsr'), W.synthetic_weights(seed=92, width_div=8, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)), 40)
    with open(os.path.join(os.path.dirname(config_utils.__file__), '..', 'configs', 'monopsr_model_000.yaml')) as f:
        cfg = yaml.safe_load(f)
    cfg['dataset_config'] = _plain(mscnn_split.config(root))
    config_path = str(base / 'config.yaml')
    with open(config_path, 'w') as f:
        yaml.safe_dump(cfg, f)
    return config_path, ckpts, prefix


def _tree(base):
    return sorted(os.path.relpath(os.path.join(d, f), base) for d, _, files in os.walk(base) for f in files)


def test_run_inference_surfaces_command_line(setup, command_line, tmp_path, capsys):
    """--surfaces writes depth_surface/ and instances_surface/ beside the three: read back, they are the device maps
    of the same chunks.  Without the flag the output tree is today's, and the three files do not change."""
    from monopsr_amd.experiments import run_inference
    _, mscnn, model, _, test = setup
    config_path, _, prefix = command_line
    out, bare = str(tmp_path / 'out'), str(tmp_path / 'bare')
    common = [config_path, prefix, '--mscnn-dir', mscnn, '--width-div', '8']
    assert run_inference.main(common + ['--output-dir', out, '--surfaces', '--max-edge-dz', 'inf',
                                        '--max-span-px', '%d' % SURFACES['max_span_px']]) == 0
    assert run_inference.main(common + ['--output-dir', bare]) == 0
    capsys.readouterr()
    with_surfaces, without = _tree(out), _tree(bare)
    names = test.split_sample_names
    extra = sorted(os.path.join('scenes', 'val', '40', kind, n + '.png') for kind in sr.SURFACE_DIRS for n in names)
    assert sorted(set(with_surfaces) - set(without)) == extra and set(without) <= set(with_surfaces)
    assert sorted(os.listdir(os.path.join(bare, 'scenes', 'val', '40'))) == sorted(sr.SCENE_DIRS)
    for rel in without:
        if rel.startswith('scenes'):
            assert open(os.path.join(out, rel), 'rb').read() == open(os.path.join(bare, rel), 'rb').read(), rel
    # the device maps of the same chunks, from the checkpoint the command line restored
    net_before = model.device_net
    frames = {}

    def hook(rows, samples, outs):
        scene = sr.reconstruct_frames(model, samples, outs, min_score=THRESHOLD, surfaces=SURFACES)
        for f, s in enumerate(samples):
            fr = scene.surfaces.frame(f)
            frames[s['sample_name']] = (fr.depth_map.cpu().numpy(), fr.instance_map.cpu().numpy())
    try:
        ev = evaluator.Evaluator(model, test, THRESHOLD, chunk_hook=hook)
        ev.restore_checkpoint(prefix, width_div=8)
        ev.run_once(40)
    finally:
        model.device_net = net_before
    base = os.path.join(out, 'scenes', 'val', '40')
    assert set(frames) == set(test.sample_names) and any(bool((d > 0).any()) for d, _ in frames.values())
    for name, (depth, inst) in frames.items():
        want = (np.where(depth < 256.0, depth, np.float32(0.0)) * 256.0).astype(np.uint16) / 256.0
        want[want < 0.1] = 0.0
        got = depth_map_utils.read_depth_map(os.path.join(base, 'depth_surface', name + '.png'))
        assert np.array_equal(got, want.astype(np.float32)), name
        assert np.array_equal(instance_utils.read_instance_image(os.path.join(base, 'instances_surface', name + '.png')),
                              inst), name
        assert np.array_equal(inst != 255, depth > 0), name
    for name in set(names) - set(test.sample_names):
        assert not depth_map_utils.read_depth_map(os.path.join(base, 'depth_surface', name + '.png')).any()
        assert bool((instance_utils.read_instance_image(os.path.join(base, 'instances_surface', name + '.png')) == 255).all())


def test_evaluator_surface_metrics_add_their_two_keys(setup, tmp_path):
    _, _, model, val, test = setup
    scored = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path / 'scene'), batch_size=2,
                                 scene_metrics=True).run_once(5)
    ev = evaluator.Evaluator(model, val, THRESHOLD, predictions_base_dir=str(tmp_path / 'surface'), batch_size=2,
                             scene_metrics='surface')
    surfaced = ev.run_once(5)
    assert set(surfaced) - set(scored) == {'surface_stats', 'surface_metrics_csv'} and set(scored) <= set(surfaced)
    assert repr(surfaced['scene_stats']) == repr(scored['scene_stats'])
    assert list(surfaced['surface_stats']) == list(sr.SURFACE_METRIC_NAMES)
    for key in scored:
        if key in ('kitti_predictions_dir', 'scene_metrics_csv', 'kitti'):
            continue
        assert repr(surfaced[key]) == repr(scored[key]), key
    # the per-object tables beside the scene's, and their statistics
    table, counts, sums, frame = ev.surface_table
    assert tuple(table.shape) == (surfaced['num_predictions'], 6) and tuple(counts.shape) == (surfaced['num_predictions'], 5)
    assert tuple(sums.shape) == (surfaced['num_predictions'], 3) and len(ev.scene_table) == 4
    assert frame.cpu().numpy().tobytes() == ev.scene_table[3].cpu().numpy().tobytes()
    host = table.cpu().numpy().astype(np.float64)
    for k, name in enumerate(sr.SURFACE_METRIC_NAMES):
        st, x = surfaced['surface_stats'][name], host[:, k][~np.isnan(host[:, k])]
        assert st['count'] == len(x) and st['dropped'] == len(host) - len(x), name
        if len(x):
            assert abs(st['mean'] - x.mean()) <= 1e-6 * max(abs(x.mean()), 1e-30) + 1e-12, name
    path = os.path.join(str(tmp_path / 'surface'), 'metrics', val.data_split, 'surface_metrics_%s.csv' % val.data_split)
    assert surfaced['surface_metrics_csv'] == path
    lines = open(path).read().splitlines()
    assert len(lines) == 2 and lines[0].split(',')[0].strip() == 'step' and lines[1].split(',')[0].strip() == '5'
    assert int(lines[1].split(',')[1]) == surfaced['surface_stats']['surface_mask_iou']['count']
    assert not os.path.exists(os.path.join(str(tmp_path / 'scene'), 'metrics', val.data_split,
                                           'surface_metrics_%s.csv' % val.data_split))
    with pytest.raises(ValueError):
        evaluator.Evaluator(model, test, THRESHOLD, scene_metrics='surface')
    with pytest.raises(ValueError):
        evaluator.Evaluator(model, val, THRESHOLD, scene_metrics='surfaces')


def test_run_evaluation_surface_metrics_command_line(setup, command_line, tmp_path, capsys):
    """--surface-metrics: the scene lines and then the surface lines after the report, and both CSVs; without the flag
    neither the lines nor the file."""
    from monopsr_amd.experiments import run_evaluation
    _, mscnn, _, _, _ = setup
    config_path, ckpts, _ = command_line
    common = [config_path, '--checkpoint-dir', ckpts, '--mscnn-dir', mscnn, '--width-div', '8']
    capsys.readouterr()
    assert run_evaluation.main(common + ['--predictions-dir', str(tmp_path / 'surface'), '--surface-metrics']) == 0
    printed = capsys.readouterr().out
    assert run_evaluation.main(common + ['--predictions-dir', str(tmp_path / 'scene'), '--scene-metrics']) == 0
    scene_only = capsys.readouterr().out
    surface_lines = [l for l in printed.splitlines() if l.startswith('surface_')]
    assert [l.split()[0] for l in surface_lines] == list(sr.SURFACE_METRIC_NAMES)
    assert [l for l in printed.splitlines() if not l.startswith('surface_')] == scene_only.splitlines()
    assert [l.split()[0] for l in printed.splitlines() if l.startswith('scene_')] == list(sr.SCENE_METRIC_NAMES)
    for kind, there in (('surface', True), ('scene', False)):
        path = os.path.join(str(tmp_path / kind), 'metrics', 'val', 'surface_metrics_val.csv')
        assert os.path.exists(path) == there
        assert os.path.exists(os.path.join(str(tmp_path / kind), 'metrics', 'val', 'scene_metrics_val.csv'))
    lines = open(os.path.join(str(tmp_path / 'surface'), 'metrics', 'val', 'surface_metrics_val.csv')).read().splitlines()
    assert len(lines) == 2 and lines[1].split(',')[0].strip() == '40'
    assert int(lines[1].split(',')[1]) == int(surface_lines[0].split()[2])

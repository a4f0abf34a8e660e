"""The mesh extraction of csrc/scene.hip and what is built on it, on the GPU against tests/mesh_restatement.py.  Every
comparison is exact: indices and counts as integers, xyz, rgb, normal and the fp64 areas as bits."""
import os

import numpy as np
import pytest
import torch

import mesh_cases as cases
import mesh_restatement as restatement
import mscnn_split
from monopsr_amd import _lib
from monopsr_amd.core import config_utils, constants, evaluator
from monopsr_amd.core import scene_reconstruction as sr
from monopsr_amd.datasets.kitti import instance_utils, kitti_dataset

pytestmark = pytest.mark.gpu

THRESHOLD = 0.1
# the end-to-end tests: a random-weight net's maps are no surfaces, so no depth limit, and a span the restatement's
# per-pixel loops can afford (tests/test_scene_surface_gpu.py)
SURFACES = dict(max_edge_dz=float('inf'), max_span_px=6)
FLOATS = ('xyz', 'rgb', 'normal')
OFFSETS = ('vertex_box_offset', 'vertex_frame_offset', 'face_box_offset', 'face_frame_offset')


def _args(case):
    dev = torch.device('cuda', 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return (t(np.asarray(case['xyz'], np.float32)), case['box_frame'], case['cam_p'], case['shapes']), dict(
        valid_mask=None if case.get('mask') is None else t(np.asarray(case['mask'], np.float32)),
        keep=None if case.get('keep') is None else t(np.asarray(case['keep'], np.int32)),
        max_edge_dz=case.get('max_edge_dz', 1.0), max_span_px=case.get('max_span_px', 64))


def _extract(case, visible_only, images=None):
    args, kw = _args(case)
    if images is not None:
        # each image as slice 1 of a stack of two: a view, off the allocator's alignment
        images = [torch.from_numpy(np.stack([np.zeros_like(im), im])).to(args[0].device)[1] for im in images]
    return sr.extract_instance_meshes(*args, images=images, visible_only=visible_only, **kw)


def _run(name, visible_only, with_images=True):
    return _extract(cases.case(name), visible_only, cases.images(name) if with_images else None)


def _host(got):
    return {k: getattr(got, k).cpu().numpy() for k in sr.MeshResult.__slots__ if torch.is_tensor(getattr(got, k))}


def _assert_mesh(got, want, what=''):
    assert isinstance(got, sr.MeshResult)
    for key in FLOATS:
        assert getattr(got, key).dtype == torch.float32
    for key in ('vertex_box', 'faces', 'face_box'):
        assert getattr(got, key).dtype == torch.int32
    assert got.area_per_box.dtype == torch.float64 and all(getattr(got, k).dtype == torch.int64 for k in OFFSETS)
    h = _host(got)
    for key in OFFSETS:
        assert np.array_equal(h[key], want[key]), (what, key, h[key], want[key])
    for key in FLOATS:
        assert h[key].shape == want[key].shape, (what, key)
        assert np.array_equal(h[key].view(np.uint32), want[key].view(np.uint32)), (what, key)
    assert np.array_equal(h['vertex_box'], want['vertex_box']), what
    assert h['faces'].shape == want['faces'].shape and np.array_equal(h['faces'], want['faces']), what
    assert np.array_equal(h['face_box'], want['face_box']), what
    assert h['area_per_box'].tobytes() == want['area'].tobytes(), (what, h['area_per_box'], want['area'])
    assert np.array_equal(got.vertex_frame_offset_host, want['vertex_frame_offset'])
    assert np.array_equal(got.face_frame_offset_host, want['face_frame_offset'])
    return h


def _points_of_vertices(h, xyz_in):
    """The map point of every vertex from the outputs alone: within a box the vertices are a subsequence of the box's
    points with the same bits (the case's points are distinct)."""
    nb, npts = xyz_in.shape[0], xyz_in.shape[1] * xyz_in.shape[2]
    flat = np.ascontiguousarray(xyz_in, np.float32).reshape(nb, npts, 3).view(np.uint32)
    assert all(len(np.unique(flat[b], axis=0)) == npts for b in range(nb))
    keys = [{flat[b, p].tobytes(): p for p in range(npts)} for b in range(nb)]
    v = h['xyz'].view(np.uint32)
    points = np.asarray([b * npts + keys[b][v[k].tobytes()] for k, b in enumerate(h['vertex_box'].tolist())], np.int64)
    return points.reshape(-1)


def _triangles_of_faces(h, points, xyz_in, box_frame):
    """The triangle id of every face from its three vertices' map points: (a, c, b) with b = a + 1 is k = 0 of the cell
    whose v00 is a; otherwise a is the v11 of a k = 1."""
    nb, mh, mw = xyz_in.shape[:3]
    f_of_box = np.asarray(box_frame, np.int64)
    out = []
    for (ra, rc, rb), b in zip(h['faces'].tolist(), h['face_box'].tolist()):
        base = int(h['vertex_frame_offset'][f_of_box[b]])
        a, c, bb = (int(points[base + r]) - b * mh * mw for r in (ra, rc, rb))
        if bb == a + 1:
            assert c == a + mw
            i, j, k = a // mw, a % mw, 0
        else:
            assert bb == a - 1 and c == a - mw
            i, j, k = a // mw - 1, a % mw - 1, 1
        out.append(((b * (mh - 1) + i) * (mw - 1) + j) * 2 + k)
    return np.asarray(out, np.int64).reshape(-1)


@pytest.mark.parametrize('visible_only', (False, True))
@pytest.mark.parametrize('name', cases.NAMES)
def test_catalogue_equals_the_restatement(name, visible_only):
    case, want = cases.case(name), cases.expected(name, visible_only)
    h = _assert_mesh(_run(name, visible_only), want, (name, visible_only))
    # indices stay inside the frame's vertices and inside the face's own box
    f_of_box = np.asarray(case['box_frame'], np.int64)
    for f in range(len(case['shapes'])):
        t0, t1 = int(h['face_frame_offset'][f]), int(h['face_frame_offset'][f + 1])
        n = int(h['vertex_frame_offset'][f + 1] - h['vertex_frame_offset'][f])
        assert t0 == t1 or (0 <= int(h['faces'][t0:t1].min()) and int(h['faces'][t0:t1].max()) < n)
    if len(h['faces']):
        b = h['face_box']
        lo = (h['vertex_box_offset'][b] - h['vertex_frame_offset'][f_of_box[b]])[:, None]
        hi = (h['vertex_box_offset'][b + 1] - h['vertex_frame_offset'][f_of_box[b]])[:, None]
        assert bool(((lo <= h['faces']) & (h['faces'] < hi)).all())
    # against what exists: the renderer's per-box triangle counts and its triangle id maps
    args, kw = _args(case)
    rendered = sr.render_instance_surfaces(*args, want_tri=True, **kw)
    faces_per_box = np.diff(h['face_box_offset'])
    if not visible_only:
        assert np.array_equal(faces_per_box, rendered.tris_per_box.cpu().numpy())
    else:
        assert bool((faces_per_box <= rendered.tris_per_box.cpu().numpy()).all())
        for f, tri in enumerate(rendered.tri_maps):
            ids = np.unique(tri.cpu().numpy())
            assert int(h['face_frame_offset'][f + 1] - h['face_frame_offset'][f]) == int((ids >= 0).sum()), (name, f)
    if name in cases.DISTINCT_POINTS:
        # xyz of every vertex is the input map's bits at its point; the faces' triangle ids, from the outputs alone
        points = _points_of_vertices(h, case['xyz'])
        assert np.array_equal(points, want['point']) and bool((np.diff(points) > 0).all())
        ids = _triangles_of_faces(h, points, case['xyz'], case['box_frame'])
        assert np.array_equal(ids, want['tri']) and bool((np.diff(ids) > 0).all())
        if visible_only:
            for f, tri in enumerate(rendered.tri_maps):
                won = np.unique(tri.cpu().numpy())
                mine = ids[int(h['face_frame_offset'][f]):int(h['face_frame_offset'][f + 1])]
                assert np.array_equal(mine, won[won >= 0]), (name, f)


@pytest.mark.parametrize('name', cases.DETERMINISM_CASES)
def test_two_runs_return_the_same_bytes(name):
    for visible_only in (False, True):
        a, b = _host(_run(name, visible_only)), _host(_run(name, visible_only))
        assert sorted(a) == sorted(b) and len(a['faces']) > 0
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), (name, visible_only, key)


def test_poisoned_buffers_change_nothing(monkeypatch):
    """Every buffer the wrapper allocates (both workspaces and the outputs) filled with 0xFF bytes (NaN as a float)
    beforehand and then with 0x00 bytes: the meshes are the restatement's."""
    real = sr._empty
    for fill in (255, 0):
        def poisoned(shape, dtype, device, fill=fill):
            t = real(shape, dtype, device)
            if t.numel():
                t.view(torch.uint8).fill_(fill)
            return t
        monkeypatch.setattr(sr, '_empty', poisoned)
        for name in ('cell_2x2', 'spike_3x3', 'hidden_box', 'random_b12_5x4', 'big_48x48'):
            for visible_only in (False, True):
                _assert_mesh(_run(name, visible_only), cases.expected(name, visible_only), (name, visible_only, fill))


def test_without_images_the_colours_are_zero():
    for name in ('off_image', 'random_b12_5x4'):
        got = _run(name, False, with_images=False)
        _assert_mesh(got, cases.expected(name, False, with_images=False), name)
        assert len(got.rgb) > 0 and not bool(got.rgb.any())
        assert bool(_run(name, False).rgb.any())


def test_frames_are_meshes_of_their_own():
    name = 'random_b12_5x4'
    got, want = _run(name, False), cases.expected(name, False)
    assert got.num_frames == 3
    for f in range(3):
        fm = got.frame(f)
        v0, v1 = int(want['vertex_frame_offset'][f]), int(want['vertex_frame_offset'][f + 1])
        t0, t1 = int(want['face_frame_offset'][f]), int(want['face_frame_offset'][f + 1])
        b0 = int(np.searchsorted(cases.case(name)['box_frame'], f))
        assert np.array_equal(fm.xyz.cpu().numpy().view(np.uint32), want['xyz'][v0:v1].view(np.uint32))
        assert np.array_equal(fm.faces.cpu().numpy(), want['faces'][t0:t1])
        assert np.array_equal(fm.box.cpu().numpy(), want['vertex_box'][v0:v1] - b0)
        assert np.array_equal(fm.face_box.cpu().numpy(), want['face_box'][t0:t1] - b0)
        assert t0 == t1 or int(fm.faces.max()) < v1 - v0
    assert len(got.frame(1).xyz) == 0 and len(got.frame(1).faces) == 0 and len(got.frame(1).area_per_box) == 0


def test_arguments_and_empty_inputs():
    dev = torch.device('cuda', 0)
    cam = cases.surface_cases.scene_cases.pow2_camera(4.0, 0.0, 0.0)[None]
    maps = torch.from_numpy(cases.plane(1, 1, 2, 2, 3, 3)[None]).to(dev)
    for bad in (dict(max_edge_dz=0.0), dict(max_edge_dz=float('nan')), dict(max_span_px=0), dict(max_span_px=1025)):
        with pytest.raises(_lib.InvalidArgumentError):
            sr.extract_instance_meshes(maps, [0], cam, [(8, 8)], **bad)
    for shape in ((1, 1, 3, 3), (1, 3, 1, 3), (1, 9, 3)):
        with pytest.raises(_lib.InvalidArgumentError):
            sr.extract_instance_meshes(torch.zeros(shape, device=dev), [0], cam, [(8, 8)])
    with pytest.raises(_lib.MpsrError):
        sr.extract_instance_meshes(maps.cpu(), [0], cam, [(8, 8)])
    with pytest.raises(_lib.InvalidArgumentError):
        sr.extract_instance_meshes(maps, [0], cam, [(8, 8)], images=[])
    with pytest.raises(_lib.InvalidArgumentError):
        sr.extract_instance_meshes(maps, [0], cam, [(8, 8)], images=[torch.zeros((8, 7, 3), device=dev)])
    # no box: no vertex, no face, zeroed offsets
    none = sr.extract_instance_meshes(maps[:0], [], cam, [(8, 8)], images=[torch.zeros((8, 8, 3), device=dev)])
    assert tuple(none.xyz.shape) == (0, 3) == tuple(none.faces.shape) and tuple(none.area_per_box.shape) == (0,)
    assert none.vertex_frame_offset.tolist() == [0, 0] == none.face_frame_offset.tolist()
    assert none.vertex_box_offset.tolist() == [0] == none.face_box_offset.tolist()
    assert len(none.frame(0).xyz) == 0 and none.num_frames == 1
    # the library's own empty path zeroes the tables it is given
    lib = _lib.lib()
    tables = torch.full((4, 3), 7, dtype=torch.int64, device=dev)
    assert lib.mpsr_scene_surface_mesh(
        None, None, None, None, None, None, None, None, None, 2, 0, 3, 3, 1.0, 64, 0, None, 0, None, 0, None, None, None,
        None, None, None, None, tables[0].data_ptr(), tables[1].data_ptr(), tables[2].data_ptr(), tables[3].data_ptr(),
        _lib.stream()) == 0
    assert tables.cpu().numpy().tolist() == [[0, 7, 7], [0, 0, 0], [0, 7, 7], [0, 0, 0]]
    # one whole box, all options
    got = sr.extract_instance_meshes(maps, [0], cam, [(8, 8)], device=dev, max_edge_dz=float('inf'), max_span_px=1024)
    assert len(got.xyz) == 9 and len(got.faces) == 8 and float(got.area_per_box[0]) == 16.0
    assert bool((got.normal == torch.tensor([0.0, 0.0, -1.0], device=dev)).all()) and not bool(got.rgb.any())


# ---- end to end: the fixture split, a small random-weight net (as tests/test_scene_surface_gpu.py sets it up)


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from monopsr_amd.core import device_net as dn
    from monopsr_amd.core import weights as W
    from monopsr_amd.core.models.monopsr.monopsr_model import MonoPSRModel
    root, mscnn = mscnn_split.build(str(tmp_path_factory.mktemp('kitti_scene_mesh')))
    div = 8
    cfg = config_utils.default_config()
    net = dn.DeviceNet(W.synthetic_weights(seed=91, width_div=div, scopes=(W.CROP_SCOPE, W.FULL_SCOPE)),
                       width_div=div, full_trunk=True)
    dcfg = mscnn_split.config(root)
    model = MonoPSRModel(cfg.model_config, dcfg, net, 'test')
    val = kitti_dataset.KittiDataset(dcfg, 'val', mscnn_label_dir=mscnn)
    test = kitti_dataset.KittiDataset(mscnn_split.config(root, has_kitti_labels=True), 'test', mscnn_label_dir=mscnn)
    return root, mscnn, model, val, test


def _case_of_chunk(model, samples, outs, min_score, options):
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
    if all(s.get('gt_valid_mask_maps') is not None for s in samples):
        case['mask'] = torch.cat([s['gt_valid_mask_maps'][0:n] for s, n in zip(samples, counts)]).reshape(
            (sum(counts),) + roi).cpu().numpy()
    if min_score is not None:
        case['keep'] = (torch.cat([s['label_scores'][0:n] for s, n in zip(samples, counts)]).cpu().numpy()
                        >= np.float32(min_score)).astype(np.int32)
    return case


SCENE_KEYS = ('xyz', 'rgb', 'box', 'pixel', 'frame_offset', 'kept_per_box', 'visible_per_box')


def test_reconstruct_frames_with_meshes_equals_the_restatement(setup):
    _, _, model, val, _ = setup
    rows = np.arange(min(val.num_samples, 3))
    samples = val.get_sample_dict(rows, epoch=0)
    with torch.no_grad():
        outs = model.build_batch(samples)
        without = sr.reconstruct_frames(model, samples, outs, surfaces=SURFACES)
        meshed = sr.reconstruct_frames(model, samples, outs, surfaces=dict(SURFACES, mesh=True))
        visible = sr.reconstruct_frames(model, samples, outs, surfaces=dict(SURFACES, mesh=True, mesh_visible_only=True))
        off = sr.reconstruct_frames(model, samples, outs, surfaces=dict(SURFACES, mesh=False))
        case = _case_of_chunk(model, samples, outs, None, SURFACES)
    # without the key everything is what it was, and asking for the meshes changes nothing else
    assert without.meshes is None and off.meshes is None and sr.reconstruct_frames(model, samples, outs).meshes is None
    for other in (meshed, visible):
        assert isinstance(other.meshes, sr.MeshResult)
        for key in SCENE_KEYS:
            assert getattr(without, key).cpu().numpy().tobytes() == getattr(other, key).cpu().numpy().tobytes(), key
        for x, y in zip(without.depth_maps + without.instance_maps + without.surfaces.depth_maps +
                        without.surfaces.instance_maps, other.depth_maps + other.instance_maps +
                        other.surfaces.depth_maps + other.surfaces.instance_maps):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert without.surfaces.tris_per_box.cpu().numpy().tobytes() == other.surfaces.tris_per_box.cpu().numpy().tobytes()
    # the meshes are the restatement's of the same network outputs, coloured from the frames' images
    rendering = restatement.surface_restatement.render(case)
    images = [s['rgb_image'].cpu().numpy().astype(np.float32) for s in samples]
    h = _assert_mesh(meshed.meshes, restatement.mesh(case, rendering, False, images))
    _assert_mesh(visible.meshes, restatement.mesh(case, rendering, True, images))
    assert len(h['faces']) > 0 and bool(h['rgb'].any())
    assert np.array_equal(np.diff(h['face_box_offset']), meshed.surfaces.tris_per_box.cpu().numpy())
    assert len(visible.meshes.faces) <= len(h['faces'])
    with pytest.raises(ValueError):
        sr.reconstruct_frames(model, samples, outs, surfaces=dict(meshes=True))


def _plain(obj):
    if isinstance(obj, config_utils.ConfigObj):
        return {k: _plain(v) for k, v in obj.__dict__.items()}
    return obj


@pytest.fixture(scope='module')
def command_line(setup, tmp_path_factory):
    """A saved checkpoint and a config file for the command line."""
    import yaml
    from monopsr_amd.core import checkpoint_utils
    from monopsr_amd.core import weights as W
    root, mscnn, _, _, _ = setup
    base = tmp_path_factory.mktemp('mesh_cli')
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


def test_run_inference_meshes_command_line(setup, command_line, tmp_path, capsys):
    """--meshes writes mesh/<name>.ply beside the other files, one per frame of the split: read back, they are the
    device meshes of the same chunks.  Without the flag the output tree is what --surfaces alone gives, file for file."""
    from monopsr_amd.experiments import run_inference
    _, mscnn, model, _, test = setup
    config_path, _, prefix = command_line
    out, bare = str(tmp_path / 'out'), str(tmp_path / 'bare')
    common = [config_path, prefix, '--mscnn-dir', mscnn, '--width-div', '8', '--max-edge-dz', 'inf',
              '--max-span-px', '%d' % SURFACES['max_span_px']]
    assert run_inference.main(common + ['--output-dir', out, '--meshes']) == 0  # (implies --surfaces)
    assert run_inference.main(common + ['--output-dir', bare, '--surfaces']) == 0
    capsys.readouterr()
    with_meshes, without = _tree(out), _tree(bare)
    names = test.split_sample_names
    extra = sorted(os.path.join('scenes', 'val', '40', 'mesh', n + '.ply') for n in names)
    assert sorted(set(with_meshes) - set(without)) == extra and set(without) <= set(with_meshes)
    assert sorted(os.listdir(os.path.join(bare, 'scenes', 'val', '40'))) == sorted(sr.SCENE_DIRS + sr.SURFACE_DIRS)
    for rel in without:
        if rel.startswith('scenes'):
            assert open(os.path.join(out, rel), 'rb').read() == open(os.path.join(bare, rel), 'rb').read(), rel
    # the device meshes of the same chunks, from the checkpoint the command line restored
    net_before = model.device_net
    frames = {}

    def hook(rows, samples, outs):
        scene = sr.reconstruct_frames(model, samples, outs, min_score=THRESHOLD, surfaces=dict(SURFACES, mesh=True))
        for f, s in enumerate(samples):
            fm = scene.meshes.frame(f)
            frames[s['sample_name']] = {k: getattr(fm, k).cpu().numpy() for k in ('xyz', 'faces', 'rgb', 'normal', 'box')}
    try:
        ev = evaluator.Evaluator(model, test, THRESHOLD, chunk_hook=hook)
        ev.restore_checkpoint(prefix, width_div=8)
        ev.run_once(40)
    finally:
        model.device_net = net_before
    base = os.path.join(out, 'scenes', 'val', '40', 'mesh')
    assert set(frames) == set(test.sample_names) and any(len(m['faces']) for m in frames.values())
    for name, m in frames.items():
        xyz, faces, rgb, normal, box = sr.read_mesh_ply(os.path.join(base, name + '.ply'))
        assert len(xyz) == len(m['xyz']) and len(faces) == len(m['faces']), name
        assert np.array_equal(xyz.view(np.uint32), m['xyz'].view(np.uint32)) and np.array_equal(faces, m['faces']), name
        assert np.array_equal(normal.view(np.uint32), m['normal'].view(np.uint32)) and np.array_equal(box, m['box']), name
        assert np.array_equal(rgb, sr.colours_to_uint8(m['rgb'])), name
    for name in set(names) - set(test.sample_names):
        empty = sr.read_mesh_ply(os.path.join(base, name + '.ply'))
        assert len(empty[0]) == 0 and len(empty[1]) == 0

"""Scene reconstruction without a GPU: the restatement against its own per-point loop, the PLY files, the C entry
points' host-side argument checks, the command line's parser and the Evaluator's hook argument."""
import inspect
import os
import re

import numpy as np
import pytest

import scene_cases
import scene_restatement

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ('mpsr_scene_workspace_bytes', 'mpsr_scene_project', 'mpsr_scene_resolve', 'mpsr_scene_compact')


@pytest.mark.parametrize('name', scene_cases.NAMES)
def test_vectorised_restatement_equals_its_loop(name):
    case = scene_cases.case(name)
    pix = scene_restatement.project(case)
    assert np.array_equal(pix, scene_restatement.project_loop(case))
    shapes = case['shapes']
    hw = np.asarray([shapes[int(f)][0] * shapes[int(f)][1] for f in case['box_frame']])[:, None]
    assert pix.min() >= -1 and bool((pix < hw).all())


def test_the_catalogue_holds_what_it_is_meant_to_hold():
    """Every property the catalogue is there for shows in the restatement's own results."""
    ex = scene_cases.expected
    r = ex('rounding_5x7')
    c = scene_cases.case('rounding_5x7')
    pix = scene_restatement.project(c)[0]
    # x at -0.5 - ulp, -0.5, -0.5 + ulp: outside, column 0 (-0.0), column 0; 0.5 -> 0, 1.5 -> 2, 2.5 -> 2: half to even
    assert pix[:3].tolist() == [-1, 7, 7] and pix[3:6].tolist() == [7, 7, 8] and pix[6:9].tolist() == [8, 9, 9]
    assert pix[9:12].tolist() == [9, 9, 10]
    # w - 0.5 = 6.5 -> 6 (even) stays inside, one ulp more rounds to 7 = w: outside
    assert pix[18:21].tolist() == [13, 13, -1]
    # h - 0.5 = 4.5 -> 4 (inside), one ulp more -> 5 = h (outside)
    assert pix[-3:].tolist() == [4 * 7 + 2, 4 * 7 + 2, -1]
    assert r['kept_per_box'][0] == (pix >= 0).sum()
    d = ex('dropped')
    # box 0: the first point and the one of the five copies whose mask is > 0; box 1: all but z = 2 and z = 5; keep = 0
    assert d['kept_per_box'].tolist() == [2, 18, 0] and scene_cases.case('dropped')['xyz'].shape[1] == 20
    z = ex('zbuffer_three_boxes')
    assert z['instance_maps'][0][2, 3] == 2 and z['depth_maps'][0][2, 3] == 2.0   # the nearest of three boxes
    assert z['instance_maps'][0][1, 1] == 2 and z['depth_maps'][0][4, 6] == 1.0   # the nearer hit of one box
    assert z['visible_per_box'].sum() < z['kept_per_box'].sum()
    e = ex('zbuffer_equal_depth')
    assert e['instance_maps'][0][2, 3] == 0 and e['instance_maps'][0][1, 1] == 0  # equal depth: the lower point index
    assert ex('zbuffer_equal_depth', True)['xyz'].shape[0] == e['visible_per_box'].sum()
    big = ex(scene_cases.DETERMINISM_CASE)
    assert big['kept_per_box'][0] == 0 and big['kept_per_box'][-1] == 0 and big['kept_per_box'][1] == 300
    assert big['frame_offset'][1] == big['frame_offset'][2] and 0 < big['frame_offset'][1] < big['frame_offset'][3]
    for f, n in ((0, 30), (2, 40)):
        ids = set(np.unique(big['instance_maps'][f]).tolist()) - {255}
        assert ids and max(ids) < n
    assert bool((big['instance_maps'][1] == 255).all()) and not big['depth_maps'][1].any()
    assert ex('boxes_255')['instance_maps'][0].max() == 254


def test_ply_round_trip(tmp_path):
    from monopsr_amd.core import scene_reconstruction as sr
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((17, 3)).astype(np.float32)
    xyz[0] = [np.nan, np.inf, -0.0]
    rgb = rng.integers(0, 256, (17, 3)).astype(np.uint8)
    box = rng.integers(-5, 300, 17).astype(np.int32)
    path = str(tmp_path / 'a.ply')
    sr.write_ply(path, xyz, rgb, box)
    got = sr.read_ply(path)
    assert got[0].tobytes() == xyz.tobytes() and got[1].tobytes() == rgb.tobytes() and got[2].tobytes() == box.tobytes()
    assert got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    data = open(path, 'rb').read()
    assert data.startswith(b'ply\nformat binary_little_endian 1.0\nelement vertex 17\n')
    assert len(data) == data.index(b'end_header\n') + len(b'end_header\n') + 17 * (12 + 3 + 4)
    # an empty cloud
    sr.write_ply(path, np.zeros((0, 3), np.float32))
    got = sr.read_ply(path)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0,)
    # without colours or boxes: zeros
    sr.write_ply(path, xyz)
    got = sr.read_ply(path)
    assert got[0].tobytes() == xyz.tobytes() and not got[1].any() and not got[2].any()
    with open(path, 'wb') as f:
        f.write(data[:-1])
    with pytest.raises(ValueError):
        sr.read_ply(path)


def test_ply_colours_clip_then_round_half_to_even(tmp_path):
    from monopsr_amd.core import scene_reconstruction as sr
    vals = np.asarray([[254.5, 255.5, -0.5], [300.0, 0.5, 1.5], [2.5, 127.49, 253.5]], np.float32)
    want = np.asarray([[254, 255, 0], [255, 0, 2], [2, 127, 254]], np.uint8)
    assert np.array_equal(sr.colours_to_uint8(vals), want)
    path = str(tmp_path / 'c.ply')
    sr.write_ply(path, np.zeros((3, 3), np.float32), vals)
    assert np.array_equal(sr.read_ply(path)[1], want)


def test_new_names_are_declared_and_bound():
    from monopsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'monopsr_hip.h')).read()
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES
        assert re.search(r'\b%s\s*\(' % name, header), name
    assert _lib.ABI_VERSION == 13
    mk = open(os.path.join(ROOT, 'monopsr_amd', 'csrc', 'Makefile')).read()
    assert 'scene.hip' in re.search(r'^SRCS\s*:=\s*(.*\.hip.*)$', mk, re.M).group(1).split()
    assert re.search(r'^[^\n#]*\bscene\.o\b[^\n]*:[^\n]*\n\t[^\n]*\$\(NOFMA\)', mk, re.M)


def test_entry_points_check_their_arguments_without_a_gpu():
    from monopsr_amd import _lib
    lib = _lib.lib()
    N = None
    project = lambda nf, nb, npts: lib.mpsr_scene_project(N, N, N, N, N, N, N, N, N, N, nf, nb, npts, N, 0, N)
    resolve = lambda nf, tp, nb, npts: lib.mpsr_scene_resolve(N, N, nf, tp, nb, npts, N, 0, N, N, N)
    compact = lambda nf, tp, nb, npts: lib.mpsr_scene_compact(N, N, N, N, nf, tp, nb, npts, 0, N, 0, N, N, N, N, N, N,
                                                              N, N)
    # empty sizes: no-ops
    for nf, nb, npts in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (0, 0, 0)):
        assert project(nf, nb, npts) == 0
        assert resolve(nf, 10, nb, npts) == 0
        assert compact(nf, 10, nb, npts) == 0
    assert resolve(2, 0, 3, 4) == 0 and compact(2, 0, 3, 4) == 0
    # negative sizes
    for nf, nb, npts in ((-1, 3, 4), (2, -3, 4), (2, 3, -4)):
        for status in (project(nf, nb, npts), resolve(nf, 10, nb, npts), compact(nf, 10, nb, npts)):
            assert status == 1
            assert b'negative' in lib.mpsr_last_error()
    assert resolve(2, -10, 3, 4) == 1 and b'negative' in lib.mpsr_last_error()
    assert compact(2, -10, 3, 4) == 1 and b'negative' in lib.mpsr_last_error()
    # null pointers with non-empty sizes
    assert project(2, 3, 4) == 1 and b'null' in lib.mpsr_last_error()
    assert resolve(2, 10, 3, 4) == 1 and b'null' in lib.mpsr_last_error()
    assert compact(2, 10, 3, 4) == 1 and b'null' in lib.mpsr_last_error()
    # the point index must fit the key's 32 bits: an argument error, never a truncation
    assert project(1, 65536, 65536) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert resolve(1, 10, 65536, 65536) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert compact(1, 10, 65536, 65536) == 1 and b'32 bits' in lib.mpsr_last_error()
    assert project(1, 65535, 65536) == 1 and b'null' in lib.mpsr_last_error()   # 2^32 - 65536 points: past that check
    # the size helper
    wb = lib.mpsr_scene_workspace_bytes
    assert wb(0, 10, 3, 4) == 0 and wb(2, 0, 3, 4) == 0 and wb(2, 10, 0, 4) == 0 and wb(2, 10, 3, 0) == 0
    assert wb(-1, 10, 3, 4) == 0 and wb(1, 10, 65536, 65536) == 0
    assert wb(2, 100, 3, 4) >= 100 * 8 + 12 * 4 + 3 * 4 + 4 * 8
    big = wb(2, 100, 3, 2304)
    assert big >= 100 * 8 + 3 * 2304 * 4 + 3 * 4 + 4 * 8 and big - wb(2, 100, 3, 4) >= 3 * 2300 * 4 - 256


def test_host_checks_of_the_frame_tables_need_no_gpu():
    """Host copies are checked before anything is launched: with them wrong, the (invalid) device pointers are never
    used."""
    import ctypes
    from monopsr_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(256)  # never dereferenced: every call below fails its host checks first
    arr = lambda values, dtype: np.ascontiguousarray(np.asarray(values, dtype))
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def project(box_frame, hw, offs, nb=3):
        bf, hw, offs = arr(box_frame, np.int32), arr(hw, np.int32), arr(offs, np.int64)
        return lib.mpsr_scene_project(fake, None, fake, host(bf), None, fake, fake, host(hw), fake, host(offs),
                                      len(hw), nb, 4, None, 0, None)
    assert project([0, 1, 1], [[5, 7], [8, 8]], [1, 36, 100]) == 1 and b'pixel_offset[0]' in lib.mpsr_last_error()
    assert project([0, 1, 1], [[5, 7], [8, 8]], [0, 35, 100]) == 1 and b'spans' in lib.mpsr_last_error()
    assert project([0, 1, 1], [[5, 0], [8, 8]], [0, 0, 64]) == 1 and b'frame 0 is' in lib.mpsr_last_error()
    assert project([0, 2, 1], [[5, 7], [8, 8]], [0, 35, 99]) == 1 and b'of frame 2' in lib.mpsr_last_error()
    assert project([1, 0, 1], [[5, 7], [8, 8]], [0, 35, 99]) == 1 and b'decreases' in lib.mpsr_last_error()
    assert project([0, -1, 1], [[5, 7], [8, 8]], [0, 35, 99]) == 1 and b'of frame -1' in lib.mpsr_last_error()
    # all tables right: the workspace is the next thing missing (status 3), still before any launch
    assert project([0, 1, 1], [[5, 7], [8, 8]], [0, 35, 99]) == 3 and b'workspace' in lib.mpsr_last_error()
    # more than 255 boxes in a frame: refused by resolve
    bf = arr([0] * 256 + [1], np.int32)
    assert lib.mpsr_scene_resolve(fake, host(bf), 2, 99, 257, 4, None, 0, fake, fake, None) == 1
    assert b'more than 255' in lib.mpsr_last_error()
    bf = arr([0] * 255 + [1] * 2, np.int32)
    assert lib.mpsr_scene_resolve(fake, host(bf), 2, 99, 257, 4, None, 0, fake, fake, None) == 3  # the workspace


def test_run_inference_parser():
    from monopsr_amd.experiments import run_inference
    ap = run_inference.build_parser()
    a = ap.parse_args(['cfg.yaml', 'ckpt', '--mscnn-dir', 'm', '--output-dir', 'o'])
    assert (a.config, a.checkpoint, a.mscnn_dir, a.output_dir) == ('cfg.yaml', 'ckpt', 'm', 'o')
    assert a.data_split == 'val' and a.width_div == 1 and a.no_scenes is False and a.min_score is None
    assert a.visible_only is False
    a = ap.parse_args(['cfg.yaml', 'ckpt', '--mscnn-dir', 'm', '--output-dir', 'o', '--data-split', 'test',
                       '--width-div', '8', '--no-scenes', '--min-score', '0.35', '--visible-only'])
    assert a.data_split == 'test' and a.width_div == 8 and a.no_scenes and a.min_score == 0.35 and a.visible_only
    for missing in (['cfg.yaml', 'ckpt', '--mscnn-dir', 'm'], ['cfg.yaml', 'ckpt', '--output-dir', 'o'],
                    ['cfg.yaml', '--mscnn-dir', 'm', '--output-dir', 'o']):
        with pytest.raises(SystemExit):
            ap.parse_args(missing)
    assert callable(run_inference.main)
    assert run_inference.scene_dir('o', 'val', 7) == os.path.join('o', 'scenes', 'val', '7')


def test_evaluator_hook_defaults_to_none():
    from monopsr_amd.core import evaluator
    sig = inspect.signature(evaluator.Evaluator.__init__)
    assert sig.parameters['chunk_hook'].default is None
    assert list(sig.parameters)[-1] == 'chunk_hook'  # appended: positional calls mean what they meant


def test_save_empty_frame(tmp_path):
    from monopsr_amd.core import scene_reconstruction as sr
    from monopsr_amd.datasets.kitti import depth_map_utils, instance_utils
    dirs = sr.scene_output_dirs(str(tmp_path))
    assert sorted(dirs) == ['depth', 'instances', 'points'] and all(os.path.isdir(d) for d in dirs.values())
    ply, depth, inst = sr.save_empty_frame(dirs, '000002', (5, 7))
    assert sr.read_ply(ply)[0].shape == (0, 3)
    assert depth_map_utils.read_depth_map(depth).shape == (5, 7) and not depth_map_utils.read_depth_map(depth).any()
    assert bool((instance_utils.read_instance_image(inst) == 255).all())

"""GPU checks of csrc/depth_fill.hip: the projection and IP-Basic completion, bit for bit against the reference's
results committed under tests/golden and against the restatement (tests/ip_basic_restatement.py) run live; the command
line end to end; poisoned scratch, short workspaces, bad kernels and CPU tensors."""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import depth_cases as dc
import ip_basic_restatement as rs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from monopsr_amd.datasets.kitti import depth_map_utils
    from monopsr_amd.ip_basic import ip_basic
    return depth_map_utils, ip_basic


def _calib(dmu, name):
    return dmu.FrameCalib(*dc.calib(name))


def _gpu_fill(ipb, maps, **kw):
    out, stages = ipb.fill_in_multiscale_batch(np.asarray(maps, np.float32), show_process=True, **kw)
    return out, stages


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ------------------------------------------------------------------------------------------------------ projection

@pytest.mark.parametrize('name', dc.frames())
def test_projection_equals_reference(mods, name):
    dmu, _ = mods
    m = dmu.project_depths_batch([dc.velodyne(name)], [_calib(dmu, name)], dc.shape(name))
    assert _same(m[0].cpu().numpy(), dc.projected(name))


def test_projection_batch_equals_single_calls(mods):
    dmu, _ = mods
    names = ['000001', '000002', '000001']
    shape = dc.shape('000001')
    batch = dmu.project_depths_batch([dc.velodyne(n) for n in names], [_calib(dmu, n) for n in names], shape)
    for k, n in enumerate(names):
        assert _same(batch[k].cpu().numpy(), dc.projected(n))


P2 = np.array([[100.0, 0, 50, 0], [0, 100, 40, 0], [0, 0, 1, 0]])
EYE = np.eye(4)[:3]


def _live(dmu, pts, shape=(80, 100), max_depth=100.0):
    got = dmu.project_depths_rows([pts], [EYE], [P2], shape, max_depth)[0].cpu().numpy()
    want = rs.project_depths(pts, EYE, P2, shape, max_depth)
    assert _same(got, want)
    return got


def test_projection_duplicates_last_wins(mods):
    dmu, _ = mods
    rng = np.random.default_rng(0)
    z = rng.uniform(2, 60, 4000).astype(np.float32)
    px = rng.integers(0, 6, 4000).astype(np.float32)  # 6 x 6 pixels hit by 4000 points
    py = rng.integers(0, 6, 4000).astype(np.float32)
    pts = np.stack([(px - 50 + 20) * z / 100, (py - 40 + 20) * z / 100, z], 1).astype(np.float32)
    m = _live(dmu, pts)
    assert np.count_nonzero(m) > 30


def test_projection_behind_camera_and_beyond_max_depth(mods):
    dmu, _ = mods
    pts = np.array([[0, 0, 10], [0, 0, -5], [1, 1, -20], [2, 0, 150], [-3, 2, 100.0], [0.5, 0, 100], [1.5, 0, 100]],
                   np.float32)
    m = _live(dmu, pts)
    assert m[35, 45] == -20  # behind the camera, projected through the negative w: kept with its negative depth
    assert m[40, 50] == 100  # -5 landed here first; (0.5, 0, 100) at u = 50.5 rounds to the even 50 and comes last
    assert m[40, 51] == 100 and m[40, 52] == 100  # 150 m stores max_depth; 51.5 rounds to 52


def test_projection_non_finite_and_outside(mods):
    dmu, _ = mods
    pts = np.array([[np.nan, 0, 10], [0, np.inf, 10], [0, 0, np.inf], [-np.inf, 0, 5], [0, 0, 0], [1e30, 0, 1],
                    [-60, 0, 10], [0, 0, 10]], np.float32)
    m = _live(dmu, pts)
    assert np.count_nonzero(m) == 1


def test_projection_empty_cloud(mods):
    dmu, _ = mods
    m = _live(dmu, np.zeros((0, 3), np.float32))
    assert not m.any()
    both = dmu.project_depths_rows([np.zeros((0, 3), np.float32), np.array([[0, 0, 10]], np.float32)], [EYE, EYE],
                                   [P2, P2], (80, 100))
    assert not both[0].any() and both[1].cpu().numpy()[40, 50] == 10


def test_project_depths_reference_signature(mods):
    dmu, _ = mods
    pts = np.array([[0, 0, 10], [1, 2, 30]], np.float32)
    got = dmu.project_depths(pts.T, P2, (80, 100))
    assert _same(got, rs.project_depths(pts, EYE, P2, (80, 100)))


# ------------------------------------------------------------------------------------------------------ completion

@pytest.mark.parametrize('blur', dc.BLURS)
def test_fill_equals_reference_frames(mods, blur):
    _, ipb = mods
    for name in dc.frames():
        out, stages = _gpu_fill(ipb, dc.projected(name)[None], blur_type=blur)
        got = [hashlib.sha256(np.ascontiguousarray(stages[0, k]).tobytes()).hexdigest() for k in range(8)]
        assert got == dc.stage_hashes(name, blur), (name, [g == w for g, w in zip(got, dc.stage_hashes(name, blur))])
        assert _same(out[0], stages[0, 7])
        if blur == 'bilateral':
            assert np.array_equal((out[0] * 256.0).astype(np.uint16), dc.golden_png(name))


@pytest.mark.parametrize('n', range(4))
def test_fill_equals_reference_windows(mods, n):
    _, ipb = mods
    w = dc.windows()
    for blur in dc.BLURS:
        for ex in (0, 1):
            _, stages = _gpu_fill(ipb, w['in_%d' % n][None], blur_type=blur, extrapolate=bool(ex))
            ref = w['st_%d_%s_%d' % (n, blur, ex)]
            for k in range(8):
                assert _same(stages[0, k], ref[k]), (n, blur, ex, rs.STAGES[k])


def _check_live(ipb, frame, **kw):
    out, stages = _gpu_fill(ipb, frame[None], **kw)
    want, st = rs.fill_in_multiscale(frame, **kw)
    for k, name in enumerate(rs.STAGES):
        assert _same(stages[0, k], st[name]), (name, int((stages[0, k] != st[name]).sum()))
    assert _same(out[0], want)
    return out[0]


@pytest.mark.parametrize('blur', dc.BLURS)
@pytest.mark.parametrize('extrapolate', [False, True])
def test_fill_synthetic_bin_edges_and_negatives(mods, blur, extrapolate):
    _, ipb = mods
    _check_live(ipb, dc.bin_edges(), blur_type=blur, extrapolate=extrapolate)
    f = dc.synthetic(61, 97, 1)
    f[30, 10:20] = -np.arange(10, dtype=np.float32)
    _check_live(ipb, f, blur_type=blur, extrapolate=extrapolate)


@pytest.mark.parametrize('blur', dc.BLURS)
def test_fill_degenerate_frames(mods, blur):
    _, ipb = mods
    zero = np.zeros((20, 33), np.float32)
    assert not _check_live(ipb, zero, blur_type=blur).any()
    _check_live(ipb, np.random.default_rng(2).uniform(0.2, 80, (21, 35)).astype(np.float32), blur_type=blur)
    _check_live(ipb, np.full((19, 31), 42.5, np.float32), blur_type=blur)  # constant: the bilateral copy
    cols = dc.synthetic(40, 50, 3)
    cols[:, ::7] = 0  # columns without a valid pixel
    cols[:, 20:30] = 0
    _check_live(ipb, cols, blur_type=blur)
    _check_live(ipb, cols, blur_type=blur, extrapolate=True)


@pytest.mark.parametrize('blur', dc.BLURS)
def test_fill_custom_kernels(mods, blur):
    _, ipb = mods
    f = dc.synthetic(45, 67, 4, density=0.1)
    one, full3, k4 = np.ones((1, 1), np.uint8), np.ones((3, 3), np.uint8), np.ones((4, 4), np.uint8)
    k4[0, 3] = 0
    odd = np.zeros((15, 15), np.uint8)
    odd[0, 0] = odd[14, 7] = odd[7, 7] = 1
    _check_live(ipb, f, blur_type=blur, dilation_kernel_far=one, dilation_kernel_med=full3, dilation_kernel_near=k4)
    _check_live(ipb, f, blur_type=blur, dilation_kernel_far=k4, dilation_kernel_med=odd,
                dilation_kernel_near=np.ones((2, 5), np.uint8))


@pytest.mark.parametrize('shape', [(5, 5), (7, 113), (131, 9), (375, 1242)])
def test_fill_odd_sizes(mods, shape):
    _, ipb = mods
    for blur in dc.BLURS:
        _check_live(ipb, dc.synthetic(shape[0], shape[1], shape[0] * shape[1]), blur_type=blur)


def test_fill_batch_equals_single_calls(mods):
    _, ipb = mods
    frames = np.stack([dc.synthetic(50, 70, s) for s in range(5)])
    frames[3] = 0
    frames[4] = 7.0
    for blur in dc.BLURS:
        out, stages = _gpu_fill(ipb, frames, blur_type=blur)
        for k in range(len(frames)):
            o1, s1 = _gpu_fill(ipb, frames[k:k + 1], blur_type=blur)
            assert _same(out[k], o1[0]) and _same(stages[k], s1[0])


def test_fill_tensor_api_and_process_dict(mods):
    import torch
    _, ipb = mods
    f = dc.synthetic(30, 40, 9)
    out, proc = ipb.fill_in_multiscale(torch.from_numpy(f).cuda(), show_process=True)
    assert out.is_cuda and list(proc)[0] == 's0_depths_in' and list(proc)[-1] == 's9_depths_out'
    want, st = rs.fill_in_multiscale(f)
    assert _same(out.cpu().numpy(), want) and _same(proc['s4_blurred_depths'].cpu().numpy(), st['s4_blurred_depths'])
    out_np, none = ipb.fill_in_multiscale(f)
    assert none is None and isinstance(out_np, np.ndarray) and _same(out_np, want)


# ------------------------------------------------------------------------------------------------------ end to end

def test_command_line_end_to_end(mods):
    from PIL import Image
    tmp = tempfile.mkdtemp(prefix='depth_cli_')
    try:
        split = os.path.join(tmp, 'training')
        for d in ('velodyne', 'calib', 'image_2'):
            os.makedirs(os.path.join(split, d))
        for name in dc.frames():
            v = dc.velodyne(name)
            v4 = np.concatenate([v, np.zeros((len(v), 1), np.float32)], 1)
            v4.tofile(os.path.join(split, 'velodyne', name + '.bin'))
            p2, r0, tr = dc.calib(name)
            with open(os.path.join(split, 'calib', name + '.txt'), 'w') as f:
                for key, m in (('P0', np.zeros(12)), ('P1', np.zeros(12)), ('P2', p2), ('P3', np.zeros(12)),
                               ('R0_rect', r0), ('Tr_velo_to_cam', tr)):
                    f.write('%s: %s\n' % (key, ' '.join(repr(float(x)) for x in np.ravel(m))))
            h, w = dc.shape(name)
            Image.new('RGB', (w, h)).save(os.path.join(split, 'image_2', name + '.png'))
        out = os.path.join(tmp, 'depth')
        r = subprocess.run([sys.executable, '-m', 'monopsr_amd.datasets.kitti.depth_map_utils', split, out, '--batch',
                            '2'], cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        for name in dc.frames():
            got = np.asarray(Image.open(os.path.join(out, name + '.png')))
            assert got.dtype == np.uint16 and np.array_equal(got, dc.golden_png(name)), name
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ------------------------------------------------------------------------------------------------------ robustness

def test_poisoned_scratch_gives_the_clean_result(mods):
    from monopsr_amd import _debug
    dmu, ipb = mods
    name = '000006'
    clean_proj = dmu.project_depths_batch([dc.velodyne(name)], [_calib(dmu, name)], dc.shape(name))
    clean = [ipb.fill_in_multiscale_batch(clean_proj, blur_type=b, show_process=True) for b in dc.BLURS]
    with _debug.poison_uninitialised():
        proj = dmu.project_depths_batch([dc.velodyne(name)], [_calib(dmu, name)], dc.shape(name))
        poisoned = [ipb.fill_in_multiscale_batch(proj, blur_type=b, show_process=True) for b in dc.BLURS]
    assert _same(proj.cpu(), clean_proj.cpu())
    for (o1, s1), (o2, s2) in zip(clean, poisoned):
        assert _same(o1.cpu(), o2.cpu()) and _same(s1.cpu(), s2.cpu())


def test_short_workspace(mods):
    import torch
    from monopsr_amd import _lib
    _, ipb = mods
    lib = _lib.lib()
    t = torch.zeros((2, 20, 30), device='cuda')
    out = torch.empty_like(t)
    need = lib.mpsr_depth_fill_workspace_bytes(2, 20, 30)
    ws = torch.empty(need - 1, dtype=torch.uint8, device='cuda')
    opts = ipb._opts(100.0, (ipb.CROSS_KERNEL_3, ipb.CROSS_KERNEL_5, ipb.CROSS_KERNEL_7), False, 'bilateral')
    st = lib.mpsr_depth_fill_multiscale(_lib.ptr(t), 2, 20, 30, ctypes.byref(opts), _lib.ptr(out), None,
                                        _lib.ptr(ws), need - 1, _lib.stream())
    assert st == 3  # MPSR_ERR_WORKSPACE
    need = lib.mpsr_lidar_project_workspace_bytes(1, 20, 30)
    pts = torch.zeros((1, 4), device='cuda')
    offs = np.array([0, 1], np.int64)
    offs_d = torch.from_numpy(offs).cuda()
    mat = torch.zeros((1, 3, 4), dtype=torch.float64, device='cuda')
    st = lib.mpsr_lidar_project_depths(_lib.ptr(pts), _lib.ptr(offs_d), offs.ctypes.data_as(ctypes.c_void_p), 1,
                                       _lib.ptr(mat), _lib.ptr(mat), 20, 30, 100.0, _lib.ptr(out), _lib.ptr(ws),
                                       need - 1, _lib.stream())
    assert st == 3
    torch.cuda.synchronize()


def test_bad_sizes_and_kernels(mods):
    from monopsr_amd import _lib
    _, ipb = mods
    f = np.zeros((20, 20), np.float32)
    for bad in (np.ones((16, 3), np.uint8), np.ones((3, 16), np.uint8), np.ones((0, 3), np.uint8)):
        with pytest.raises(_lib.InvalidArgumentError):
            ipb.fill_in_multiscale(f, dilation_kernel_near=bad)
    with pytest.raises(_lib.InvalidArgumentError):
        ipb.fill_in_multiscale(f, dilation_kernel_far=np.ones(3, np.uint8))
    for shape in ((4, 20), (20, 4), (1, 1)):
        with pytest.raises(_lib.InvalidArgumentError):
            ipb.fill_in_multiscale(np.zeros(shape, np.float32))
    with pytest.raises(_lib.InvalidArgumentError):
        ipb.fill_in_multiscale(f, blur_type='median')


def test_cpu_tensors_are_refused(mods):
    import torch
    from monopsr_amd import _lib
    _, ipb = mods
    with pytest.raises(_lib.MpsrError):
        ipb.fill_in_multiscale(torch.zeros((20, 20)))
    with pytest.raises(_lib.MpsrError):
        ipb.fill_in_multiscale_batch(torch.zeros((2, 20, 20)))

"""CPU checks of the LiDAR depth-map work: the cv2 stand-in's known answers, the restatement of the projection and of
IP-Basic against the committed reference results, the calibration parser, the PNG formulas, the command line's argument
errors, and an audit of the compiled depth_fill kernels (no scratch, no spills)."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cv2_standin as cv2
import depth_cases as dc
import ip_basic_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- stand-in known answers

def test_dilate_ignores_the_border():
    a = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    k = np.ones((3, 3), np.uint8)
    assert cv2.dilate(a, k).tolist() == [[5, 6, 6], [8, 9, 9], [8, 9, 9]]
    assert cv2.erode(a, k).tolist() == [[1, 1, 2], [1, 1, 2], [4, 4, 5]]
    neg = -np.ones((3, 3), np.float32)
    assert (cv2.dilate(neg, k) == -1).all()  # no zero padding: the border takes no part


def test_even_kernel_anchor():
    a = np.zeros((5, 5), np.float32)
    a[2, 2] = 1
    k = np.zeros((4, 4), np.uint8)
    k[0, 0] = 1  # offset (-2, -2) from the anchor (2, 2)
    d = cv2.dilate(a, k)
    assert d[4, 4] == 1 and (d == 1).sum() == 1
    assert d[0, 0] == -cv2.FLT_MAX  # every tap outside the image: the border value itself
    k = np.zeros((2, 4), np.uint8)
    k[1, 3] = 1  # anchor (2, 1): offset (0, +1)
    d = cv2.dilate(a, k)
    assert d[2, 1] == 1 and (d == 1).sum() == 1


def test_close_is_dilate_then_erode():
    a = np.zeros((7, 7), np.float32)
    a[3, 2] = a[3, 4] = 5
    c = cv2.morphologyEx(a, cv2.MORPH_CLOSE, np.ones((3, 3), np.uint8))
    assert c[3, 3] == 5 and c[3, 2] == 5 and c[0, 0] == 0


def test_median_replicates_the_border():
    a = np.arange(25, dtype=np.float32).reshape(5, 5)
    m = cv2.medianBlur(a, 5)
    assert m[2, 2] == 12
    # corner (0, 0): rows 0,0,0,1,2 x cols 0,0,0,1,2 -> values of a 3x3 block weighted by replication
    win = a[np.ix_([0, 0, 0, 1, 2], [0, 0, 0, 1, 2])].ravel()
    assert m[0, 0] == np.sort(win)[12]


def test_gaussian_reflect101_and_weights():
    a = np.zeros((5, 7), np.float32)
    a[2, 3] = 256
    g = cv2.GaussianBlur(a, (5, 5), 0)
    k = np.array([1, 4, 6, 4, 1], np.float32) / 16
    assert g[2, 3] == 256 * k[2] * k[2]
    assert g[0, 3] == 256 * k[2] * (k[0] + k[4])  # reflect101: rows -2 and +2 of row 0 are both row 2
    b = np.zeros((5, 5), np.float32)
    b[0, 1] = 16  # reflect101: column -1 mirrors column 1
    gb = cv2.GaussianBlur(b, (5, 5), 0)
    assert gb[0, 0] == np.float32(16 * (0.375 * 2 * 0.25))  # rows: row 0 centre; cols: x-1 and x+1 both hit column 1


def test_bilateral_has_13_taps():
    taps = cv2.bilateral_space_taps(5, 2.0)
    assert len(taps) == 13
    assert [(dy, dx) for dy, dx, _ in taps][:3] == [(-2, 0), (-1, -1), (-1, 0)]
    w = {(dy, dx): v for dy, dx, v in taps}
    assert w[(0, 0)] == 1 and w[(0, 1)] == np.float32(np.exp(-0.125)) and (2, 1) not in w


def test_bilateral_constant_frame_is_copied():
    a = np.full((6, 6), 3.5, np.float32)
    a[0, 0] = np.float32(3.5) + np.float32(1e-7)  # max - min < FLT_EPSILON
    assert cv2.bilateralFilter(a, 5, 0.5, 2.0).tobytes() == a.tobytes()


def test_bilateral_known_answer():
    a = np.zeros((5, 5), np.float32)
    a[2, 2] = 1.0
    out = cv2.bilateralFilter(a, 5, 0.5, 2.0)
    table, scale = cv2.bilateral_exp_table(0.0, 1.0, 0.5)
    assert scale == 4096 and table[0] == 1 and table[4096] == np.float32(np.exp(-2.0))
    # centre: 12 neighbours of value 0 at colour distance 1, the centre itself at distance 0
    taps = cv2.bilateral_space_taps(5, 2.0)
    wsum, s = np.float32(0), np.float32(0)
    for dy, dx, sw in taps:
        val = np.float32(1.0 if (dy, dx) == (0, 0) else 0.0)
        wgt = sw * (table[0] if val == 1 else table[4096])
        wsum, s = wsum + wgt, s + val * wgt
    assert out[2, 2] == s / wsum


# ------------------------------------------------------------------------------------------- restatement vs reference

@pytest.mark.parametrize('n', range(4))
def test_restatement_equals_reference_windows(n):
    w = dc.windows()
    for blur in dc.BLURS:
        for ex in (0, 1):
            _, st = rs.fill_in_multiscale(w['in_%d' % n], blur_type=blur, extrapolate=bool(ex))
            ref = w['st_%d_%s_%d' % (n, blur, ex)]
            for k, name in enumerate(rs.STAGES):
                assert st[name].tobytes() == ref[k].tobytes(), (n, blur, ex, name)


@pytest.mark.parametrize('name', dc.frames())
def test_restatement_equals_reference_frames(name):
    p2, r0, tr = dc.calib(name)
    m = rs.project_depths(dc.velodyne(name), rs.velo_to_cam0(r0, tr), p2, dc.shape(name))
    assert m.tobytes() == dc.projected(name).tobytes()
    for blur in dc.BLURS:
        out, st = rs.fill_in_multiscale(m, blur_type=blur)
        got = [hashlib.sha256(st[k].tobytes()).hexdigest() for k in rs.STAGES]
        assert got == dc.stage_hashes(name, blur), blur
        if blur == 'bilateral':
            assert np.array_equal((out * 256.0).astype(np.uint16), dc.golden_png(name))


def test_restatement_projection_quirks():
    eye = np.eye(4)[:3]
    p2 = np.array([[100.0, 0, 50, 0], [0, 100, 40, 0], [0, 0, 1, 0]])
    pts = np.array([[0, 0, 10], [0, 0, 20], [0, 0, -5], [np.nan, 0, 1], [0, np.inf, 1]], np.float32)
    m = rs.project_depths(pts, eye, p2, (80, 100))
    assert m[40, 50] == np.float32(-5.0) and np.count_nonzero(m) == 1  # the last point wins, behind the camera too
    half = np.array([[0.5, 0, 100], [1.5, 0, 100]], np.float32)     # u = 50.5 and 51.5 exactly: half to even
    m = rs.project_depths(half, eye, p2, (80, 100))
    assert m[40, 50] == 100 and m[40, 52] == 100 and np.count_nonzero(m) == 2
    m = rs.project_depths(np.array([[0, 0, 250]], np.float32), eye, p2, (80, 100))
    assert m[40, 50] == np.float32(100.0)  # beyond max_depth stores max_depth


# ------------------------------------------------------------------------------------------- host utilities

def _dmu():
    from monopsr_amd.datasets.kitti import depth_map_utils
    return depth_map_utils


def test_calibration_parser():
    dmu = _dmu()
    name = dc.frames()[1]
    p2, r0, tr = dc.calib(name)
    text = 'P0: %s\nP2: %s\nR0_rect: %s\nTr_velo_to_cam: %s\nTr_imu_to_velo: 1 2\n\n' % (
        ' '.join('0' for _ in range(12)), ' '.join('%.12e' % v for v in p2.ravel()),
        ' '.join('%.12e' % v for v in r0.ravel()), ' '.join('%.12e' % v for v in tr.ravel()))
    c = dmu.parse_calibration(text)
    assert np.array_equal(c.p2, p2) and np.array_equal(c.r0_rect, r0) and np.array_equal(c.velo_to_cam, tr)
    assert np.array_equal(dmu.velo_to_cam0(c), rs.velo_to_cam0(r0, tr))
    with pytest.raises(ValueError):
        dmu.parse_calibration('P2: 1 2 3\nR0_rect: 1 0 0 0 1 0 0 0 1\nTr_velo_to_cam: %s' % ' '.join(['0'] * 12))
    with pytest.raises(ValueError):
        dmu.parse_calibration('P2: %s' % ' '.join(['0'] * 12))


def test_png_round_trip():
    dmu = _dmu()
    rng = np.random.default_rng(3)
    d = rng.uniform(0, 90, (20, 30)).astype(np.float32)
    d[:3] = 0
    d[5, 5] = np.float32(0.05)
    tmp = tempfile.mkdtemp()
    try:
        path = os.path.join(tmp, 'x.png')
        dmu.save_depth_map(path, d)
        from PIL import Image
        raw = np.asarray(Image.open(path))
        assert raw.dtype == np.uint16 and np.array_equal(raw, (d * 256.0).astype(np.uint16))
        back = dmu.read_depth_map(path)
        want = raw / 256.0
        want[want < 0.1] = 0.0
        assert back.dtype == np.float32 and np.array_equal(back, want.astype(np.float32))
        assert back[5, 5] == 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _cli(*args):
    return subprocess.run([sys.executable, '-m', 'monopsr_amd.datasets.kitti.depth_map_utils'] + list(args), cwd=ROOT,
                          capture_output=True, text=True, timeout=120)


def test_cli_argument_errors():
    r = _cli()
    assert r.returncode == 2 and 'split_dir' in r.stderr
    tmp = tempfile.mkdtemp()
    try:
        r = _cli(tmp, os.path.join(tmp, 'out'), '--batch', '0')
        assert r.returncode == 2 and '--batch' in r.stderr
        r = _cli(tmp, os.path.join(tmp, 'out'), '--blur', 'median')
        assert r.returncode == 2 and 'invalid choice' in r.stderr
        r = _cli(os.path.join(tmp, 'missing'), os.path.join(tmp, 'out'))
        assert r.returncode == 2 and 'no such directory' in r.stderr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ------------------------------------------------------------------------------------------- build audit

def test_depth_fill_kernels_use_no_scratch():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    csrc = os.path.join(ROOT, 'monopsr_amd', 'csrc')
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert re.search(r'^[^\n]*depth_fill\.o[^\n]*:\s*%\.o', mk, re.M), 'depth_fill.o must use the NOFMA rule'
    tmp = tempfile.mkdtemp(prefix='depth_audit_')
    try:
        subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off',
                               '-I' + os.path.join(ROOT, 'include'), '-I' + csrc, '-save-temps', '-c',
                               os.path.join(csrc, 'depth_fill.hip'), '-o', os.path.join(tmp, 'a.o')], cwd=tmp,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = [f for f in os.listdir(tmp) if f.endswith('gfx950.s')]
        text = open(os.path.join(tmp, asm[0])).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    kernels = re.findall(r'\.name:\s+(_Z\S*kernel\S*)', text)
    assert len(kernels) >= 12, kernels
    for blk in text.split('.name:')[1:]:
        if '_kernel' not in blk.split('\n', 1)[0]:
            continue
        name = blk.split('\n', 1)[0].strip()
        assert re.search(r'\.private_segment_fixed_size:\s+0\b', blk), name
        assert re.search(r'\.vgpr_spill_count:\s+0\b', blk), name
        assert re.search(r'\.sgpr_spill_count:\s+0\b', blk), name

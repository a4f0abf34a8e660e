"""Loads the LiDAR depth-map fixtures of tests/golden (written by tests/golden/make_depth_fixture.py) and builds the
synthetic frames the depth tests share."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BLURS = ('bilateral', 'gaussian')


def fixture():
    return np.load(os.path.join(GOLDEN, 'depth_fixture.npz'))


def windows():
    return np.load(os.path.join(GOLDEN, 'depth_windows.npz'))


def frames():
    return [str(f) for f in fixture()['frames']]


def velodyne(name):
    """The fixture's velodyne xyz (N, 3) float32: the raw cloud of 000000, the in-image points of the others."""
    path = os.path.join(GOLDEN, 'depth_velo_%s.npy' % name)
    if os.path.exists(path):
        return np.load(path)
    return np.concatenate([np.load(os.path.join(GOLDEN, 'depth_velo_%s_%s.npy' % (name, h))) for h in 'ab'])


def calib(name):
    d = fixture()
    return d['p2_%s' % name], d['r0_rect_%s' % name], d['velo_to_cam_%s' % name]


def shape(name):
    return tuple(int(v) for v in fixture()['shape_%s' % name])


def projected(name):
    """The reference's projected map of a fixture frame, (h, w) float32."""
    d = fixture()
    h, w = shape(name)
    m = np.zeros(h * w, np.float32)
    m[d['proj_idx_%s' % name]] = d['proj_val_%s' % name]
    return m.reshape(h, w)


def stage_hashes(name, blur):
    return [str(s) for s in fixture()['sha_%s_%s' % (blur, name)]]


def golden_png(name):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, 'depth_%s.png' % name)))


def synthetic(h, w, seed, density=0.06):
    """A sparse map like a projected LiDAR frame: empty top rows, depths 0.1 .. 90 m, a few negatives."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.float32)
    hit = rng.random((h, w)) < density
    hit[: max(1, h // 5)] = False
    m[hit] = rng.uniform(1.0, 90.0, int(hit.sum())).astype(np.float32)
    neg = rng.random((h, w)) < 0.002
    m[neg] = -rng.uniform(0.0, 5.0, int(neg.sum())).astype(np.float32)
    return m


def bin_edges(h=24, w=40):
    """Every bin edge (0.1, 15, 30) and the next float32 on either side, scattered over a frame."""
    vals = []
    for e in (0.1, 15.0, 30.0):
        f = np.float32(e)
        vals += [np.nextafter(f, np.float32(-1)), f, np.nextafter(f, np.float32(100))]
    m = np.zeros((h, w), np.float32)
    rng = np.random.default_rng(7)
    for k in range(h * w // 5):
        m[rng.integers(h), rng.integers(w)] = vals[k % len(vals)]
    return m

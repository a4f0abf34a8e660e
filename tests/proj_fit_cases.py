"""A seeded catalogue of boxes for the projection fit (csrc/proj_fit.hip): one dict per launch.

Kinds of box:
  planted  the expected grid back-projected at a smooth depth and moved to the local frame of a known placement
           x* = (d*, cy*, va*) (rounded to float32 first): the objective is 0 there, up to the float32 rounding of the
           stored points; the start is off by up to +-20 % in d, +-0.5 m in cy and (n = 3) +-0.05 rad in va
  noisy    planted plus Gaussian noise (2 cm) on the points
  masked   planted, but the first quarter of the points is all zeros and masked out
  cy0      planted with the start at cy = 0 exactly: the 0.00025 branch of the initial simplex (n = 2; the n = 3 start
           of such a box is an ordinary one)
  novalid  all points zero: no valid point
  badcam   a camera index out of range
Depths 4-60 m, local points within 3 m, cameras: a KITTI P2 and the same with P[0,3] = 0.
"""
import numpy as np

import proj_fit_restatement as R

P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
               [0.0, 0.0, 1.0, 0.002745884]], np.float32)  # a KITTI P2 (training/calib/000000.txt of the fixtures)
P2_NO_SHIFT = P2.copy()
P2_NO_SHIFT[0, 3] = 0.0
CAMS = np.stack([P2, P2_NO_SHIFT])

PLANTED_KINDS = ('planted', 'masked', 'cy0')
FITTED_KINDS = PLANTED_KINDS + ('noisy',)


def _backproject(cam, u, v, z, cam0_shift):
    """The point of depth z that projects to (u, v), in the frame the placed cloud lives in."""
    cam = cam.astype(np.float64)
    wc = z + cam[2, 3]
    x = (u * wc - cam[0, 2] * z - cam[0, 3]) / cam[0, 0]
    y = (v * wc - cam[1, 2] * z - cam[1, 3]) / cam[1, 1]
    if cam0_shift:
        x = x - (-cam[0, 3] / cam[0, 0])
    return np.stack([x, y, z], -1)


def _box(rng, kind, h, w, cam, flags):
    f = float(cam[0, 0])
    zc = rng.uniform(4.0, 55.0)
    uc, vc = rng.uniform(150.0, 1050.0), rng.uniform(120.0, 260.0)
    if kind == 'cy0':
        vc = float(cam[1, 2]) + 0.2 * f / zc
    bw, bh = f * rng.uniform(1.0, 2.5) / zc, f * rng.uniform(1.0, 2.0) / zc
    box = np.asarray([vc - bh / 2, uc - bw / 2, vc + bh / 2, uc + bw / 2], np.float32)
    centre = _backproject(cam, uc, vc, zc, flags['cam0_shift'])
    star = np.asarray([np.hypot(centre[0], centre[2]), centre[1], np.arctan2(centre[0], centre[2])], np.float32)
    eu, ev = R.exp_grid(box, h, w, flags['round_box_2d'], flags['use_pixel_centres'])
    i = np.arange(h * w)
    z = zc + 0.5 + 0.3 * np.sin(2 * np.pi * (i // w) / h) * np.cos(2 * np.pi * (i % w) / w)
    glob = _backproject(cam, eu, ev, z, flags['cam0_shift'])
    d, cy, va = star.astype(np.float64)
    rel = glob - np.asarray([d * np.sin(va), cy, d * np.cos(va)])
    if flags['rotate_view']:  # the inverse of R_y(va)
        c, s = np.cos(va), np.sin(va)
        rel = np.stack([c * rel[:, 0] - s * rel[:, 2], rel[:, 1], s * rel[:, 0] + c * rel[:, 2]], 1)
    if kind == 'noisy':
        rel = rel + rng.normal(0.0, 0.02, rel.shape)
    mask = np.ones(h * w, np.float32)
    if kind == 'masked':
        q = max(1, (h * w) // 4)
        rel[:q] = 0.0
        mask[:q] = 0.0
    if kind == 'novalid':
        rel[:] = 0.0
    assert np.abs(rel).max() < 3.0
    x0 = star.copy()
    x0[0] = star[0] * (1.0 + rng.uniform(-0.2, 0.2))
    # (away from 0: the simplex's edge in cy is 5 % of the start)
    away = float(np.copysign(rng.uniform(0.3, 0.5), star[1]))
    x0[1] = 0.0 if kind == 'cy0' else star[1] + away
    x0_3 = x0.copy()
    x0_3[2] = star[2] + rng.uniform(-0.05, 0.05)
    if kind == 'cy0':  # (with three coordinates SciPy's rule collapses on the 0.00025 edge before it has moved: n = 2 only)
        x0_3[1] = star[1] + away
    return box, rel.astype(np.float32), mask, star, x0, x0_3


def _launch(seed, h, w, kinds, flags, with_mask=True, with_index=True):
    rng = np.random.RandomState(seed)
    flags = dict(R.FLAGS, **flags)
    b = len(kinds)
    out = dict(h=h, w=w, b=b, kinds=list(kinds), flags=flags, cams=CAMS if with_index else CAMS[:1],
               local=np.zeros((b, h * w, 3), np.float32), boxes=np.zeros((b, 4), np.float32),
               mask=np.ones((b, h * w), np.float32) if with_mask else None,
               cam_index=np.zeros(b, np.int32) if with_index else None,
               star=np.full((b, 3), np.nan, np.float32), x0={2: np.zeros((b, 3), np.float32),
                                                              3: np.zeros((b, 3), np.float32)})
    for k, kind in enumerate(kinds):
        ci = int(rng.randint(0, 2)) if with_index else 0
        box, local, mask, star, x0, x0_3 = _box(rng, kind, h, w, CAMS[ci], flags)
        out['boxes'][k], out['local'][k], out['x0'][2][k], out['x0'][3][k] = box, local, x0, x0_3
        if with_mask:
            out['mask'][k] = mask
        else:
            assert kind != 'masked'
        if with_index:
            out['cam_index'][k] = ci
        if kind in PLANTED_KINDS:
            out['star'][k] = star
        if kind == 'badcam':
            out['cam_index'][k] = (len(CAMS), -1)[k % 2]
    return out


def _mix(b):
    cycle = ('planted', 'noisy', 'planted', 'masked', 'cy0', 'planted', 'noisy', 'novalid', 'planted', 'badcam',
             'badcam')
    return [cycle[k % len(cycle)] for k in range(b)]


def camera_of(launch, k):
    """The (3,4) matrix of box k, or None where its index is out of range."""
    if launch['cam_index'] is None:
        return launch['cams'][0]
    i = int(launch['cam_index'][k])
    return launch['cams'][i] if 0 <= i < len(launch['cams']) else None


def mask_of(launch, k):
    return None if launch['mask'] is None else launch['mask'][k]


def launches():
    """name -> launch.  Map sizes 48x48 (nine points per thread), 17x16 (272 points: one stride and a tail), 5x7 (less
    than a wave) and 1x1; batches of 0, 1 and 33.  The seeds are ones at which the restatement's own fit recovers every
    planted placement with two and with three coordinates, with a float64 and with a float32 objective
    (tests/test_proj_fit.py asserts both): SciPy's rule can collapse early on this piecewise-linear objective, more
    readily under float32 noise, and a box on which the restatement itself does is no test of the kernel."""
    return {
        '48x48_b33': _launch(100, 48, 48, _mix(33), {}),
        '17x16_b33_centres': _launch(104, 17, 16, _mix(33), dict(use_pixel_centres=True, cam0_shift=False)),
        '17x16_b1_rounded': _launch(100, 17, 16, ['planted'], dict(round_box_2d=True)),
        '5x7_b1_unrotated': _launch(100, 5, 7, ['planted'], dict(rotate_view=False), with_mask=False, with_index=False),
        '5x7_b33': _launch(106, 5, 7, _mix(33), dict(use_pixel_centres=True)),
        '1x1_b33': _launch(100, 1, 1, ['planted', 'novalid', 'badcam'] * 11, {}),
        '48x48_b0': _launch(100, 48, 48, [], {}),
    }


# a 1x1 map has one point: two equations, so (d, cy) is determined and (d, cy, va) is not
def recoverable(launch, n_fit):
    return not (launch['h'] * launch['w'] == 1 and n_fit == 3)


# ---- what the tests share: the restatement's fits and the float32 probe, computed once per process

_CACHE = {}


def cached_launches():
    if 'launches' not in _CACHE:
        _CACHE['launches'] = launches()
    return _CACHE['launches']


def objective_at(launch, k, x, dtype=np.float64):
    return R.objective(launch['local'][k], x, launch['boxes'][k], camera_of(launch, k), launch['h'], launch['w'],
                       mask_of(launch, k), dtype=dtype, **launch['flags'])


def reference_fit(name, n_fit, dtype=np.float64, max_iter=None):
    """The restatement's fit of every box of a launch -> a list of fit dicts."""
    key = (name, n_fit, np.dtype(dtype).name, max_iter)
    if key not in _CACHE:
        L = cached_launches()[name]
        _CACHE[key] = [R.fit(L['local'][k], L['x0'][n_fit][k], L['boxes'][k], camera_of(L, k), L['h'], L['w'], n_fit,
                             mask_of(L, k), max_iter=max_iter, dtype=dtype, **L['flags']) for k in range(L['b'])]
    return _CACHE[key]


def recovery_bound(dtype=np.float64):
    """The largest |x - x*| per coordinate of the restatement's own fits over the planted boxes of the catalogue.
    The GPU tests' bound is the float64 restatement's (the default); tests/test_proj_fit.py prints the figure of the
    fits with a float32 objective beside it."""
    key = ('recovery', np.dtype(dtype).name)
    if key not in _CACHE:
        worst = np.zeros(3)
        for name, L in cached_launches().items():
            for n_fit in (2, 3):
                if not recoverable(L, n_fit):
                    continue
                for k, fit in enumerate(reference_fit(name, n_fit, dtype)):
                    if L['kinds'][k] in PLANTED_KINDS:
                        worst = np.maximum(worst, np.abs(fit['x'] - L['star'][k].astype(np.float64)))
        _CACHE[key] = worst
    return _CACHE[key]


def probe():
    """float32 numpy against float64 numpy on the catalogue -> dict(uv, err, fit): the largest differences of the
    projected points and of the objective at the starts, and of the float64 objective at the end of a fit whose
    objective is float32 from the one at the end of the float64 fit."""
    if 'probe' not in _CACHE:
        uv_d = err_d = fit_d = 0.0
        for name, L in cached_launches().items():
            for k in range(L['b']):
                cam = camera_of(L, k)
                if cam is None:
                    continue
                for n_fit in (2, 3):
                    x = L['x0'][n_fit][k]
                    fl = {f: L['flags'][f] for f in ('rotate_view', 'cam0_shift')}
                    uv64, ok64, _, _ = R.proj_points(L['local'][k], x, cam, mask_of(L, k), **fl)
                    uv32, ok32, _, _ = R.proj_points(L['local'][k], x, cam, mask_of(L, k), dtype=np.float32, **fl)
                    assert np.array_equal(ok64, ok32)
                    if ok64.any():
                        uv_d = max(uv_d, float(np.abs(uv32.astype(np.float64) - uv64)[:, ok64].max()))
                        err_d = max(err_d, abs(objective_at(L, k, x, np.float32) - objective_at(L, k, x)))
            for n_fit in (2, 3):
                for k, (f64, f32) in enumerate(zip(reference_fit(name, n_fit),
                                                   reference_fit(name, n_fit, np.float32))):
                    if L['kinds'][k] in FITTED_KINDS:
                        fit_d = max(fit_d, abs(objective_at(L, k, f32['x'].astype(np.float32)) -
                                               objective_at(L, k, f64['x'].astype(np.float32))))
        _CACHE['probe'] = dict(uv=uv_d, err=err_d, fit=fit_d)
    return _CACHE['probe']

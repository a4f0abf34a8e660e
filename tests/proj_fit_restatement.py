"""A numpy restatement of the projection-error objective and of its Nelder-Mead minimiser (csrc/proj_fit.hip), written
from the text of the reference's proj_points, get_exp_proj_uv_map and np_proj_error and of SciPy's Nelder-Mead rule
as include/monopsr_hip.h spells them out.  One box at a time, float64 unless a dtype is given: the float32 form is the
probe that sizes the GPU tests' margins (tests/test_proj_fit.py)."""
import numpy as np

FLAGS = dict(rotate_view=True, cam0_shift=True, round_box_2d=False, use_pixel_centres=False)


def exp_grid(box, h, w, round_box_2d=False, use_pixel_centres=False, dtype=np.float64):
    """-> (eu, ev), each (h * w,), point i at row i // w, column i % w"""
    box = np.asarray(box, dtype)
    if round_box_2d:
        box = np.round(box)
    v1, u1, v2, u2 = box
    su, sv = (u2 - u1) / dtype(w), (v2 - v1) / dtype(h)
    if use_pixel_centres:
        gu = np.linspace(u1 + su / dtype(2), u2 - su / dtype(2), w, dtype=dtype)
        gv = np.linspace(v1 + sv / dtype(2), v2 - sv / dtype(2), h, dtype=dtype)
    else:
        gu = np.linspace(u1, u2 - su, w, dtype=dtype)
        gv = np.linspace(v1, v2 - sv, h, dtype=dtype)
    eu, ev = np.meshgrid(gu, gv)
    return eu.reshape(-1).astype(dtype), ev.reshape(-1).astype(dtype)


def place(local, x, rotate_view=True, dtype=np.float64):
    """-> (rotated (P,3), global (P,3), sum of |rotated| (P,))"""
    local = np.asarray(local, dtype)
    d, cy, va = (dtype(v) for v in x)
    c, s = np.cos(va), np.sin(va)
    if rotate_view:
        rot = np.stack([c * local[:, 0] + s * local[:, 2], local[:, 1], -s * local[:, 0] + c * local[:, 2]], 1)
    else:
        rot = local
    glob = rot + np.asarray([d * s, cy, d * c], dtype)
    return rot, glob, np.abs(rot).sum(1)


def proj_points(local, x, cam_p, mask=None, rotate_view=True, cam0_shift=True, dtype=np.float64):
    """-> (uv (2,P), valid (P,) bool, projective depth (P,), sum of |rotated| (P,))"""
    cam = np.asarray(cam_p, dtype).reshape(3, 4)
    rot, glob, l1 = place(local, x, rotate_view, dtype)
    with np.errstate(invalid='ignore'):
        valid = l1 > dtype(0.1)
    if mask is not None:
        valid = valid & (np.asarray(mask).reshape(-1) != 0)
    if cam0_shift:
        glob = glob + np.asarray([-cam[0, 3] / cam[0, 0], 0, 0], dtype)
    hom = glob @ cam[:, :3].T + cam[:, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        uv = (hom[:, :2] / hom[:, 2:3]).T
    return np.where(valid[None], uv, dtype(0)).astype(dtype), valid, hom[:, 2], l1


def proj_error(uv, valid, depth, eu, ev):
    """The mean of |u - eu| + |v - ev| over the valid points, summed in float64: NaN without one, +inf where a valid
    point is not in front of the camera."""
    if not valid.any():
        return float('nan')
    if (depth[valid] <= 0).any():
        return float('inf')
    t = np.abs(uv[0] - eu) + np.abs(uv[1] - ev)
    return float(t[valid].astype(np.float64).sum() / valid.sum())


def objective(local, x, box, cam_p, h, w, mask=None, rotate_view=True, cam0_shift=True, round_box_2d=False,
              use_pixel_centres=False, dtype=np.float64):
    if cam_p is None:
        return float('nan')
    eu, ev = exp_grid(box, h, w, round_box_2d, use_pixel_centres, dtype)
    uv, valid, depth, _ = proj_points(local, x, cam_p, mask, rotate_view, cam0_shift, dtype)
    return proj_error(uv, valid, depth, eu, ev)


class _Capped(Exception):
    pass


def nelder_mead(func, x0, xatol=1e-4, fatol=1e-4, max_iter=None):
    """SciPy's rule (reflection 1, expansion 2, contractions 0.5, shrink 0.5) -> (x, f, nit, nfev, final fsim)."""
    x0 = np.asarray(x0, np.float64)
    n = len(x0)
    cap = 200 * n if max_iter is None else int(max_iter)
    calls = [0]

    def f(x):
        if calls[0] >= cap:
            raise _Capped()
        calls[0] += 1
        return func(x)

    sim = np.tile(x0, (n + 1, 1))
    for k in range(n):
        sim[k + 1, k] = (1 + 0.05) * x0[k] if x0[k] != 0 else 0.00025
    fsim = np.full(n + 1, np.inf)

    def order():
        ind = np.argsort(fsim, kind='stable')
        return sim[ind], fsim[ind]

    try:
        for k in range(n + 1):
            fsim[k] = f(sim[k])
    except _Capped:
        pass
    sim, fsim = order()
    nit = 1
    while calls[0] < cap and nit < cap:
        try:
            with np.errstate(invalid='ignore'):
                if np.max(np.abs(sim[1:] - sim[0])) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol:
                    break
            xbar = np.add.reduce(sim[:-1], 0) / n
            xr = 2.0 * xbar - 1.0 * sim[-1]
            fxr = f(xr)
            shrink = False
            if fxr < fsim[0]:
                xe = 3.0 * xbar - 2.0 * sim[-1]
                fxe = f(xe)
                if fxe < fxr:
                    sim[-1], fsim[-1] = xe, fxe
                else:
                    sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-2]:
                sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-1]:
                xc = 1.5 * xbar - 0.5 * sim[-1]
                fxc = f(xc)
                if fxc <= fxr:
                    sim[-1], fsim[-1] = xc, fxc
                else:
                    shrink = True
            else:
                xcc = 0.5 * xbar + 0.5 * sim[-1]
                fxcc = f(xcc)
                if fxcc < fsim[-1]:
                    sim[-1], fsim[-1] = xcc, fxcc
                else:
                    shrink = True
            if shrink:
                for j in range(1, n + 1):
                    sim[j] = sim[0] + 0.5 * (sim[j] - sim[0])
                    fsim[j] = f(sim[j])
            nit += 1
        except _Capped:
            pass
        finally:
            sim, fsim = order()
    return sim[0].copy(), float(fsim[0]), nit, calls[0], fsim.copy()


def fit(local, x0, box, cam_p, h, w, n_fit=2, mask=None, xatol=1e-4, fatol=1e-4, max_iter=None, dtype=np.float64,
        **flags):
    """The kernel's fit of one box -> dict(x (3,), err, err0, iters, evals, status).  The objective sees the float32
    rounding of every vertex, as the kernel's does; an evaluation without a valid point ranks as +inf."""
    x0 = np.asarray(x0, np.float32).astype(np.float64)
    nan = float('nan')
    if cam_p is None:
        return dict(x=x0.copy(), err=nan, err0=nan, iters=0, evals=0, status=2)

    def at(v):
        x = np.asarray(list(v) + list(x0[len(v):]), np.float32)
        return objective(local, x, box, cam_p, h, w, mask, dtype=dtype, **flags)

    err0 = at(x0[:n_fit])
    if np.isnan(err0):
        return dict(x=x0.copy(), err=nan, err0=nan, iters=0, evals=1, status=2)

    def func(v):
        e = at(v)
        return np.inf if np.isnan(e) else e

    cap = 200 * n_fit if max_iter is None else int(max_iter)
    x, f, nit, nfev, _ = nelder_mead(func, x0[:n_fit], xatol, fatol, cap)
    out = x0.copy()
    out[:n_fit] = np.asarray(x, np.float32)
    return dict(x=out, err=f, err0=err0, iters=nit, evals=nfev, status=1 if (nfev >= cap or nit >= cap) else 0)

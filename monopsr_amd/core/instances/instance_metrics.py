"""Projection error of a placed instance cloud against its 2-D box, and the fit that minimises it: the reference's
core/instances/instance_metrics.py (np_proj_error, scipy_proj_error, scipy_proj_error_with_viewing_angle) with the
minimiser on the card (csrc/proj_fit.hip).

    uv, valid = instance_utils.proj_points(xz_dist, cen_y, view_ang, local_points, cam_p)
    err = proj_error(uv, valid, instance_utils.get_exp_proj_uv_map(boxes_2d, (48, 48)))
    fit = fit_proj_error(local_points, boxes_2d, cam_p, xz_dist, cen_y, view_ang)      # ProjFit: x, err, err0, ...
    outs, fit = fit_centroids(model, samples, outs)                                    # a chunk of build_batch

Where the reference hands its objective to scipy.optimize.minimize one box at a time, fit_proj_error runs SciPy's
Nelder-Mead rule for every box in one launch, one workgroup per box.
"""
import collections

import torch

from monopsr_amd import _lib
from monopsr_amd.core import constants
from monopsr_amd.datasets.kitti import instance_utils

STATUS_CONVERGED, STATUS_CAPPED, STATUS_NO_FIT = 0, 1, 2

# x (N,3) float32 [xz_dist, centroid_y, viewing_angle]; err, err0 (N,) float64: the objective at x and at the start;
# iters, evals, status (N,) int32 (status: 0 converged, 1 stopped at the cap, 2 no valid point or no camera: x is the start)
ProjFit = collections.namedtuple('ProjFit', ['x', 'err', 'err0', 'iters', 'evals', 'status', 'n_fit'])


def proj_error(points_uv, points_mask, exp_grid_uv):
    """np_proj_error for N boxes: points_uv (N,2,P), points_mask (N,P), exp_grid_uv (N,H,W,2) with P = H W ->
    (N,) float64: the sum of |u - eu| + |v - ev| over the masked points, divided by their number (NaN where there is
    none)."""
    n = int(points_uv.shape[0])
    uv = points_uv.reshape(n, 2, -1).double()
    exp = exp_grid_uv.reshape(n, -1, 2).permute(0, 2, 1).double()
    mask = (points_mask.reshape(n, 1, -1) != 0).double()
    total = ((uv - exp).abs() * mask).sum((1, 2))
    return total / mask.sum((1, 2))


def fit_proj_error(inst_points_local, boxes_2d, cam_p, xz_dist, centroid_y, viewing_angle, fit_viewing_angle=False,
                   valid_mask=None, rotate_view=True, cam0_shift=True, round_box_2d=False, use_pixel_centres=False,
                   cam_index=None, xatol=1e-4, fatol=1e-4, max_iter=None):
    """Minimises the projection error of every box over (xz_dist, centroid_y), or with fit_viewing_angle over
    (xz_dist, centroid_y, viewing_angle), starting from the given values: mpsr_proj_fit.  inst_points_local (N,H,W,3)
    (the map's size is the grid's), boxes_2d (N,4) [y1,x1,y2,x2], cam_p (3,4) or (n_cams,3,4) with cam_index (N);
    valid_mask None or one entry per point.  max_iter: the cap on iterations and on evaluations, None: 200 per fitted
    coordinate.  -> ProjFit of device tensors."""
    if inst_points_local.dim() != 4 or inst_points_local.shape[3] != 3:
        raise _lib.InvalidArgumentError("inst_points_local must be (N, H, W, 3)")
    n, h, w = (int(v) for v in inst_points_local.shape[:3])
    if tuple(boxes_2d.shape) != (n, 4):
        raise _lib.InvalidArgumentError("boxes_2d must be (N,4)")
    if valid_mask is not None and valid_mask.numel() != n * h * w:
        raise _lib.InvalidArgumentError("valid_mask must hold one entry per point")
    if max_iter is not None and int(max_iter) < 1:
        raise _lib.InvalidArgumentError("max_iter %r" % (max_iter,))
    instance_utils._check_cams(cam_p, cam_index, n)
    dev = inst_points_local.device
    f32 = instance_utils._f32
    local = f32(inst_points_local).reshape(n, h * w, 3)
    x0 = instance_utils._placement(xz_dist, centroid_y, viewing_angle, n).to(dev)
    boxes, cam, idx = f32(boxes_2d), f32(cam_p).reshape(-1), instance_utils._cam_index(cam_index)
    mask = None if valid_mask is None else f32(valid_mask).reshape(n, h * w)
    n_fit = 3 if fit_viewing_angle else 2
    x = torch.empty((n, 3), dtype=torch.float32, device=dev)
    err, err0 = (torch.empty((n,), dtype=torch.float64, device=dev) for _ in range(2))
    iters, evals, status = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(3))
    _lib.check(_lib.lib().mpsr_proj_fit(
        _lib.ptr(local), _lib.ptr(x0), _lib.ptr(boxes), _lib.ptr(cam), cam.numel() // 12, _lib.ptr(idx), _lib.ptr(mask),
        n, h, w, n_fit, int(bool(rotate_view)), int(bool(cam0_shift)), int(bool(round_box_2d)),
        int(bool(use_pixel_centres)), float(xatol), float(fatol), 0 if max_iter is None else int(max_iter),
        _lib.ptr(x), _lib.ptr(err), _lib.ptr(err0), _lib.ptr(iters), _lib.ptr(evals), _lib.ptr(status), _lib.stream()))
    return ProjFit(x, err, err0, iters, evals, status, n_fit)


def fit_centroids(model, samples, outs, fit_viewing_angle=False, use_pixel_centres=True, cam0_shift=False):
    """Slides every predicted object of a chunk along its viewing ray (and in height) until its cloud fills its 2-D box.
    `samples` as dataset.get_sample_dict returns them, `outs` as model.build_batch returns them; the first num_objs
    boxes of every frame are fitted in ONE launch with per-box cameras, from x0 = (hypot(cx, cz), cy, KEY_VIEW_ANG) of
    KEY_CENTROIDS, masked by gt_valid_mask_maps where every sample carries them (as reconstruct_frames masks them).
    -> (new outs, ProjFit over those boxes, frame after frame).  In the new outs KEY_CENTROIDS is
    (d sin va, cy, d cos va), KEY_CEN_X / _Y / _Z are its columns, and with fit_viewing_angle KEY_VIEW_ANG is the
    fitted angle; a box of status 2 and the rows past num_objs keep what they had.  The inputs are not modified.
    The model's KEY_CENTROIDS x carries the cam0 offset -P[0,3]/P[0,0] (about 6 cm), so x0 is that centroid put on the
    ray of its viewing angle, and err0 is the objective there: not the error of the scene the given outs reconstruct.
    The defaults are the ones under which the fitted err is the error of the scene reconstruct_frames builds from the
    new outs: that path projects a cloud where it stands (no shift into the cam0 frame), and the grid of pixel centres
    is the one the training loss (proj_err_maps_norm) measures against."""
    if len(samples) != len(outs):
        raise ValueError('%d samples, %d outputs' % (len(samples), len(outs)))
    if len(samples) == 0:
        raise ValueError('fit_centroids needs at least one frame')
    roi = tuple(int(v) for v in model.map_roi_size)
    dev = samples[0]['boxes_2d'].device
    counts = [int(s['num_objs']) for s in samples]
    with_mask = all(s.get('gt_valid_mask_maps') is not None for s in samples)
    with torch.cuda.device(dev), torch.no_grad():
        cat = lambda ts, tail: torch.cat([t[0:n].reshape((n,) + tail) for t, n in zip(ts, counts)], 0)
        local = cat([o[constants.KEY_INST_XYZ_MAP_LOCAL] for o in outs], roi + (3,))
        view = cat([o[constants.KEY_VIEW_ANG] for o in outs], ())
        cen = cat([o[constants.KEY_CENTROIDS] for o in outs], (3,))
        boxes = cat([s['boxes_2d'] for s in samples], (4,))
        mask = cat([s['gt_valid_mask_maps'] for s in samples], roi) if with_mask else None
        cam_p = torch.stack([s['cam_p'].reshape(3, 4) for s in samples], 0)
        cam_index = torch.cat([torch.full((n,), f, dtype=torch.int32, device=dev) for f, n in enumerate(counts)])
        fit = fit_proj_error(local, boxes, cam_p, torch.hypot(cen[:, 0], cen[:, 2]), cen[:, 1], view,
                             fit_viewing_angle=fit_viewing_angle, valid_mask=mask, cam0_shift=cam0_shift,
                             use_pixel_centres=use_pixel_centres, cam_index=cam_index)
        d, cy, va = fit.x[:, 0], fit.x[:, 1], fit.x[:, 2]
        fitted = (fit.status < STATUS_NO_FIT)[:, None]
        new_cen = torch.where(fitted, torch.stack([d * torch.sin(va), cy, d * torch.cos(va)], 1), cen)
        new_view = torch.where(fitted[:, 0], va, view)
        new_outs, lo = [], 0
        for o, n in zip(outs, counts):
            o = dict(o)
            c = o[constants.KEY_CENTROIDS].clone()
            c[0:n] = new_cen[lo:lo + n]
            o[constants.KEY_CENTROIDS] = c
            for k, key in enumerate((constants.KEY_CEN_X, constants.KEY_CEN_Y, constants.KEY_CEN_Z)):
                if key in o:  # the columns the centroid was put together from
                    o[key] = c[:, k].reshape(o[key].shape).clone()
            if fit_viewing_angle:
                v = o[constants.KEY_VIEW_ANG].clone()
                v[0:n] = new_view[lo:lo + n].reshape(v[0:n].shape)
                o[constants.KEY_VIEW_ANG] = v
            new_outs.append(o)
            lo += n
    return new_outs, fit


def fit_summary(fits):
    """Counts by status and the means of err0 and err over the boxes of status < 2, of a list of ProjFit: reduced on
    the card, -> one (5,) float64 device tensor [n status 0, n status 1, n status 2, sum err0, sum err]."""
    status = torch.cat([f.status for f in fits])
    ok = status < STATUS_NO_FIT
    zero = torch.zeros((), dtype=torch.float64, device=status.device)
    return torch.stack([(status == k).sum().double() for k in range(3)] +
                       [torch.where(ok, torch.cat([getattr(f, name) for f in fits]), zero).sum()
                        for name in ('err0', 'err')])

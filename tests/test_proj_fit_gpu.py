"""mpsr_proj_points and mpsr_proj_fit (csrc/proj_fit.hip) against the numpy restatement on the seeded catalogue, and
the fit through the model: fit_centroids and the Evaluator's centroid_fit.  The margins are twice what float32 numpy
differs from float64 numpy on the same catalogue (proj_fit_cases.probe, asserted to be sane in tests/test_proj_fit.py)."""
import os

import numpy as np
import pytest
import torch

import proj_fit_cases as C
import proj_fit_restatement as R
from monopsr_amd import _lib
from monopsr_amd.core import constants, evaluator, scene_reconstruction
from monopsr_amd.core.instances import instance_metrics
from monopsr_amd.datasets.kitti import instance_utils
from test_scene_reconstruction_gpu import setup  # noqa: F401  (the tiny width-divided net and the synthetic split)

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NAMES = ['48x48_b33', '17x16_b33_centres', '17x16_b1_rounded', '5x7_b1_unrotated', '5x7_b33', '1x1_b33']


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _points(L, x, want_points=True):
    return instance_utils.proj_points_err(
        _dev(x), _dev(L['local']), _dev(L['boxes']), _dev(L['cams']), (L['h'], L['w']), valid_mask=_dev(L['mask']),
        cam_index=_dev(L['cam_index']), want_points=want_points, **L['flags'])


def _fit(L, n_fit, max_iter=None):
    x0 = _dev(L['x0'][n_fit])
    return instance_metrics.fit_proj_error(
        _dev(L['local']).reshape(L['b'], L['h'], L['w'], 3), _dev(L['boxes']), _dev(L['cams']), x0[:, 0], x0[:, 1],
        x0[:, 2], fit_viewing_angle=n_fit == 3, valid_mask=_dev(L['mask']), cam_index=_dev(L['cam_index']),
        max_iter=max_iter, **L['flags'])


@pytest.mark.parametrize('name', NAMES)
def test_proj_points_is_the_restatement(name):
    L = C.cached_launches()[name]
    probe = C.probe()
    worst_uv = worst_err = 0.0
    for n_fit in (2, 3):
        x = L['x0'][n_fit]
        uv, valid, err = _points(L, x)
        _, _, err_only = _points(L, x, want_points=False)  # NULL uv and NULL valid
        again = _points(L, x)
        assert np.array_equal(_bits(err), _bits(err_only))
        for a, b in zip((uv, valid, err), again):
            assert np.array_equal(_bits(a.to(torch.uint8) if a.dtype == torch.bool else a),
                                  _bits(b.to(torch.uint8) if b.dtype == torch.bool else b))
        uv, valid, err = uv.cpu().numpy(), valid.cpu().numpy(), err.cpu().numpy()
        for k, kind in enumerate(L['kinds']):
            cam = C.camera_of(L, k)
            if cam is None:
                assert np.isnan(uv[k]).all() and not valid[k].any() and np.isnan(err[k]), (name, k)
                continue
            fl = {f: L['flags'][f] for f in ('rotate_view', 'cam0_shift')}
            want_uv, want_valid, _, l1 = R.proj_points(L['local'][k], x[k], cam, C.mask_of(L, k), **fl)
            assert not (np.abs(l1 - 0.1) < 1e-5).any()
            assert np.array_equal(valid[k], want_valid), (name, k)
            assert not uv[k][:, ~want_valid].any()
            want_err = C.objective_at(L, k, x[k])
            if kind == 'novalid':
                assert np.isnan(err[k]) and np.isnan(want_err)
                continue
            worst_uv = max(worst_uv, float(np.abs(uv[k] - want_uv)[:, want_valid].max()))
            worst_err = max(worst_err, abs(float(err[k]) - want_err))
    print('%s: |uv - restatement| %.3e px (probe %.3e)  |err - restatement| %.3e px (probe %.3e)'
          % (name, worst_uv, probe['uv'], worst_err, probe['err']))
    assert worst_uv <= 2 * probe['uv'] and worst_err <= 2 * probe['err']


def test_proj_points_behind_the_camera_is_inf_and_batch_zero_is_a_no_op():
    L = C.cached_launches()['5x7_b1_unrotated']
    x = L['x0'][2].copy()
    x[:, 0] = -x[:, 0]
    _, valid, err = _points(L, x)
    assert bool(valid.all()) and float(err[0]) == float('inf') and C.objective_at(L, 0, x[0]) == float('inf')
    E = C.cached_launches()['48x48_b0']
    uv, valid, err = _points(E, E['x0'][2])
    assert tuple(uv.shape) == (0, 2, 48 * 48) and tuple(valid.shape) == (0, 48 * 48) and tuple(err.shape) == (0,)
    fit = _fit(E, 2)
    assert all(tuple(t.shape)[0] == 0 for t in fit[:6])
    lib = _lib.lib()
    assert lib.mpsr_proj_points(None, None, None, None, 1, None, None, None, None, None, 0, 48, 48, 1, 1, 0, 0, None) == 0
    assert lib.mpsr_proj_fit(None, None, None, None, 1, None, None, 0, 48, 48, 2, 1, 1, 0, 0, 1e-4, 1e-4, 0, None, None,
                             None, None, None, None, None) == 0


def test_bad_arguments_are_refused():
    lib = _lib.lib()
    assert lib.mpsr_proj_points(None, None, None, None, 1, None, None, None, None, None, 1, 4, 4, 1, 1, 0, 0, None) == 1
    assert b'null' in lib.mpsr_last_error()
    assert lib.mpsr_proj_points(None, None, None, None, 1, None, None, None, None, None, -1, 4, 4, 1, 1, 0, 0, None) == 1
    args = lambda b, h, w, n_fit, n_cams=1: (None, None, None, None, n_cams, None, None, b, h, w, n_fit, 1, 1, 0, 0, 1e-4,
                                             1e-4, 0, None, None, None, None, None, None, None)
    assert lib.mpsr_proj_fit(*args(1, 4, 4, 2)) == 1 and b'null' in lib.mpsr_last_error()
    assert lib.mpsr_proj_fit(*args(0, 49, 48, 2)) == 1 and b'2304' in lib.mpsr_last_error()
    assert lib.mpsr_proj_fit(*args(0, 4, 4, 4)) == 1 and b'n_fit' in lib.mpsr_last_error()
    assert lib.mpsr_proj_fit(*args(0, 4, 0, 2)) == 1 and lib.mpsr_proj_fit(*args(0, 4, 4, 2, n_cams=0)) == 1
    with pytest.raises(_lib.InvalidArgumentError):
        instance_metrics.fit_proj_error(torch.zeros((2, 4, 4, 3), device=DEV), torch.zeros((3, 4), device=DEV),
                                        torch.zeros((3, 4), device=DEV), [1.0, 1.0], [0.0, 0.0], [0.0, 0.0])


@pytest.mark.parametrize('n_fit', [2, 3])
@pytest.mark.parametrize('name', NAMES)
def test_proj_fit(name, n_fit):
    L = C.cached_launches()[name]
    probe, bound = C.probe(), 2 * C.recovery_bound()
    ref = C.reference_fit(name, n_fit)
    fit = _fit(L, n_fit)
    again = _fit(L, n_fit)
    for a, b in zip(fit[:6], again[:6]):
        assert np.array_equal(_bits(a), _bits(b))
    # err0 and err are mpsr_proj_points at x0 and at x, bit for bit
    _, _, at_x0 = _points(L, L['x0'][n_fit], want_points=False)
    _, _, at_x = _points(L, fit.x.cpu().numpy(), want_points=False)
    x, err, err0 = fit.x.cpu().numpy(), fit.err.cpu().numpy(), fit.err0.cpu().numpy()
    iters, evals, status = fit.iters.cpu().numpy(), fit.evals.cpu().numpy(), fit.status.cpu().numpy()
    done = status < 2
    assert np.array_equal(_bits(fit.err0)[done], _bits(at_x0)[done])
    assert np.array_equal(_bits(fit.err)[done], _bits(at_x)[done])
    assert (err[done] <= err0[done]).all()
    if n_fit == 2:
        assert np.array_equal(x[:, 2], L['x0'][2][:, 2])
    worst_f, worst_dx = -np.inf, np.zeros(3)
    for k, kind in enumerate(L['kinds']):
        if kind in ('novalid', 'badcam'):
            assert (status[k], iters[k], evals[k]) == (ref[k]['status'], ref[k]['iters'], ref[k]['evals']), (name, k)
            assert status[k] == 2 and np.isnan(err[k]) and np.isnan(err0[k])
            assert np.array_equal(x[k], L['x0'][n_fit][k])
            continue
        assert status[k] < 2 and 1 <= iters[k] and n_fit + 1 <= evals[k] <= 200 * n_fit, (name, k, status[k])
        over = C.objective_at(L, k, x[k]) - C.objective_at(L, k, ref[k]['x'].astype(np.float32))
        worst_f = max(worst_f, over)
        assert over <= 2 * probe['fit'], (name, n_fit, k, kind, over)
        if kind in C.PLANTED_KINDS and C.recoverable(L, n_fit):
            dx = np.abs(x[k].astype(np.float64) - L['star'][k].astype(np.float64))
            worst_dx = np.maximum(worst_dx, dx)
            assert (dx <= bound).all(), (name, n_fit, k, kind, dx, bound)
    print('%s n = %d: objective over the restatement\'s %.3e px (probe %.3e); |x - x*| %s (restatement %s); '
          'evaluations per box %.1f' % (name, n_fit, worst_f, probe['fit'], worst_dx, C.recovery_bound(),
                                        float(evals.mean())))


@pytest.mark.parametrize('n_fit', [2, 3])
def test_proj_fit_stops_at_the_cap(n_fit):
    L = C.cached_launches()['5x7_b33']
    fit = _fit(L, n_fit, max_iter=3)
    ref = C.reference_fit('5x7_b33', n_fit, max_iter=3)
    status, iters, evals = fit.status.cpu().numpy(), fit.iters.cpu().numpy(), fit.evals.cpu().numpy()
    for k, kind in enumerate(L['kinds']):
        if kind in C.FITTED_KINDS:
            assert status[k] == 1 and iters[k] <= 3 and evals[k] <= 3
            assert (iters[k], evals[k]) == (ref[k]['iters'], ref[k]['evals'])
        else:
            assert status[k] == 2
    done = status < 2
    assert bool((fit.err[done] <= fit.err0[done]).all())


def test_python_wrappers_agree_with_the_kernel():
    L = C.cached_launches()['17x16_b33_centres']
    x = L['x0'][3]
    keep = np.asarray([C.camera_of(L, k) is not None for k in range(L['b'])])
    uv, valid, err = _points(L, x)
    puv, pvalid = instance_utils.proj_points(_dev(x[:, 0]), _dev(x[:, 1]), _dev(x[:, 2]), _dev(L['local']),
                                             _dev(L['cams']), cam0_shift=False, cam_index=_dev(L['cam_index']))
    mask = _dev(L['mask']) != 0
    assert bool(((pvalid & mask) == valid)[_dev(keep)].all())
    sel = valid[:, None].expand_as(uv)  # (without a mask the wrapper also projects the masked points)
    assert torch.equal(puv[sel], uv[sel]) and int(valid.sum()) > 0
    grid = instance_utils.get_exp_proj_uv_map(_dev(L['boxes']), (L['h'], L['w']), use_pixel_centres=True)
    assert tuple(grid.shape) == (L['b'], L['h'], L['w'], 2)
    for k in (0, 5):
        eu, ev = R.exp_grid(L['boxes'][k], L['h'], L['w'], False, True)
        assert np.abs(grid[k, :, :, 0].reshape(-1).cpu().numpy() - eu).max() < 2e-4
        assert np.abs(grid[k, :, :, 1].reshape(-1).cpu().numpy() - ev).max() < 2e-4
    got = instance_metrics.proj_error(puv, valid, grid).cpu().numpy()
    want = err.cpu().numpy()
    ok = np.isfinite(want)
    assert ok.sum() >= 24 and np.abs(got[ok] - want[ok]).max() <= 2 * C.probe()['err']
    assert np.isnan(got[~ok & keep]).all()


# ---- through the model


def _chunk(model, ds):
    samples = ds.get_sample_dict(np.arange(min(ds.num_samples, 3)), epoch=0)
    with torch.no_grad():
        return samples, model.build_batch(samples)


@pytest.mark.parametrize('fit_viewing_angle', [False, True])
def test_fit_centroids(setup, fit_viewing_angle, monkeypatch):
    _, _, model, val, _ = setup
    samples, outs = _chunk(model, val)
    before = [{k: (v.clone() if torch.is_tensor(v) else v) for k, v in o.items()} for o in outs]
    ids = [{k: id(v) for k, v in o.items()} for o in outs]
    new_outs, fit = instance_metrics.fit_centroids(model, samples, outs, fit_viewing_angle=fit_viewing_angle)
    counts = [int(s['num_objs']) for s in samples]
    assert fit.x.shape[0] == sum(counts) > 0 and fit.n_fit == (3 if fit_viewing_angle else 2)
    # the inputs are what they were
    for o, b, i in zip(outs, before, ids):
        assert set(o) == set(b) and {k: id(v) for k, v in o.items()} == i
        for k, v in o.items():
            if torch.is_tensor(v):
                assert torch.equal(v, b[k]) or (torch.isnan(v) == torch.isnan(b[k])).all(), k
    status = fit.status.cpu().numpy()
    done = status < 2
    assert done.any()
    x = fit.x.double().cpu().numpy()
    lo = 0
    for o, new, n in zip(outs, new_outs, counts):
        assert set(new) == set(o)
        cen, old = new[constants.KEY_CENTROIDS].double().cpu().numpy(), o[constants.KEY_CENTROIDS].double().cpu().numpy()
        va = new[constants.KEY_VIEW_ANG].double().cpu().numpy().reshape(-1)
        old_va = o[constants.KEY_VIEW_ANG].double().cpu().numpy().reshape(-1)
        assert np.array_equal(cen[n:], old[n:]) and np.array_equal(va[n:], old_va[n:])
        for k in range(n):
            if not done[lo + k]:
                assert np.array_equal(cen[k], old[k]) and va[k] == old_va[k]
                continue
            d, cy, a = x[lo + k]
            assert a == va[k] and (fit_viewing_angle or a == old_va[k])
            # on the viewing ray: no component across it, the fitted distance along it, the fitted height
            scale = max(abs(d), 1.0)
            assert abs(cen[k, 0] * np.cos(a) - cen[k, 2] * np.sin(a)) <= 1e-6 * scale
            assert abs(cen[k, 0] * np.sin(a) + cen[k, 2] * np.cos(a) - d) <= 1e-6 * scale
            assert cen[k, 1] == cy
        for j, key in enumerate((constants.KEY_CEN_X, constants.KEY_CEN_Y, constants.KEY_CEN_Z)):
            assert np.array_equal(new[key].double().cpu().numpy().reshape(-1), cen[:, j])
        for key in o:
            if key not in (constants.KEY_CENTROIDS, constants.KEY_CEN_X, constants.KEY_CEN_Y, constants.KEY_CEN_Z,
                           constants.KEY_VIEW_ANG):
                assert new[key] is o[key], key
        if not fit_viewing_angle:
            assert new[constants.KEY_VIEW_ANG] is o[constants.KEY_VIEW_ANG]
        lo += n
    assert bool((fit.err[fit.status < 2] <= fit.err0[fit.status < 2]).all())

    # identity: the clouds reconstruct_frames places from the new outs (what it hands to project_instance_points: the
    # global maps, their boxes' frames, the cameras and the mask), projected as project_instance_points projects them
    # (the full matrix in float64, no shift to cam0), lie at the mean L1 distance from the grid of pixel centres that
    # the fit reported
    handed = {}
    project = scene_reconstruction.project_instance_points

    def capture(xyz_global, box_frame, cam_p, frame_shapes, **kw):
        handed.update(glob=xyz_global, frame=np.asarray(box_frame), cams=cam_p, mask=kw.get('valid_mask'))
        return project(xyz_global, box_frame, cam_p, frame_shapes, **kw)
    monkeypatch.setattr(scene_reconstruction, 'project_instance_points', capture)
    scene = scene_reconstruction.reconstruct_frames(model, samples, new_outs)
    monkeypatch.undo()
    total = sum(counts)
    assert scene.kept_per_box.shape[0] == total and int(scene.kept_per_box.sum()) == scene.xyz.shape[0] > 0
    roi = tuple(model.map_roi_size)
    glob = handed['glob'].reshape(total, -1, 3).double().cpu().numpy()
    frame, cams = handed['frame'], handed['cams'].reshape(-1, 3, 4).double().cpu().numpy()
    assert np.array_equal(frame, np.repeat(np.arange(len(samples)), counts))
    boxes = torch.cat([s['boxes_2d'][0:n] for s, n in zip(samples, counts)])
    local = torch.cat([o[constants.KEY_INST_XYZ_MAP_LOCAL][0:n] for o, n in zip(new_outs, counts)])
    _, valid, at_x = instance_utils.proj_points_err(
        fit.x, local, boxes, handed['cams'], roi, valid_mask=handed['mask'], cam0_shift=False, use_pixel_centres=True,
        cam_index=torch.as_tensor(frame, dtype=torch.int32, device=boxes.device))
    assert np.array_equal(_bits(at_x)[done], _bits(fit.err)[done])
    grid = instance_utils.get_exp_proj_uv_map(boxes, roi, use_pixel_centres=True).reshape(total, -1, 2)
    grid, valid, err = grid.double().cpu().numpy(), valid.cpu().numpy(), fit.err.cpu().numpy()
    worst = far = 0.0
    checked = 0
    for k in range(total):
        if not done[k] or not np.isfinite(err[k]):
            continue
        cam = cams[int(frame[k])]
        hom = glob[k] @ cam[:, :3].T + cam[:, 3]
        uv = hom[:, :2] / hom[:, 2:3]
        l1 = np.abs(uv - grid[k]).sum(1)[valid[k]].mean()
        print('box %d: |scene L1 - fit err| %.3e px  max |uv| %.1f px  depth %.2f..%.2f m  x %s'
              % (k, abs(l1 - err[k]), np.abs(uv[valid[k]]).max(), hom[valid[k], 2].min(), hom[valid[k], 2].max(), x[k]))
        worst, far = max(worst, abs(l1 - err[k])), max(far, float(np.abs(uv[valid[k]]).max()))
        checked += 1
    print('identity over %d boxes: |scene L1 - fit err| %.3e px (probe %.3e), max |uv| %.1f px'
          % (checked, worst, C.probe()['err'], far))
    assert checked and worst <= 2 * C.probe()['err']


def _lines(path):
    with open(path) as f:
        return [line.split() for line in f.read().splitlines() if line]


def test_evaluator_centroid_fit(setup, tmp_path):
    _, _, model, val, _ = setup
    kw = dict(score_threshold=0.0, batch_size=2, compute_metrics=False, compute_losses=False)
    plain = evaluator.Evaluator(model, val, predictions_base_dir=str(tmp_path / 'plain'), **kw).run_once(3)
    none = evaluator.Evaluator(model, val, predictions_base_dir=str(tmp_path / 'plain'), centroid_fit=None,
                               **kw).run_once(3)
    assert set(none) == set(plain) and 'centroid_fit' not in plain
    for key in plain:
        if key == 'kitti':
            assert repr(none[key]) == repr(plain[key]) or none['report'] == plain['report']
        else:
            assert none[key] == plain[key], key
    status = {}

    def hook(rows, samples, outs):
        with torch.no_grad():
            _, fit = instance_metrics.fit_centroids(model, samples, model.build_batch(samples))
        st, lo = fit.status.cpu().numpy(), 0
        for s in samples:
            n = int(s['num_objs'])
            status[s['sample_name']] = st[lo:lo + n]
            lo += n
    ev = evaluator.Evaluator(model, val, predictions_base_dir=str(tmp_path / 'fit'), centroid_fit={}, chunk_hook=hook,
                             **kw)
    assert ev.centroid_fit == {}
    fitted = ev.run_once(3)
    summary = fitted['centroid_fit']
    every = np.concatenate(list(status.values()))
    assert summary['converged'] == int((every == 0).sum()) and summary['capped'] == int((every == 1).sum())
    assert summary['not_fitted'] == int((every == 2).sum())
    assert summary['converged'] + summary['capped'] > 0 and summary['mean_err'] <= summary['mean_err0']
    assert set(fitted) == set(plain) | {'centroid_fit'} and fitted['num_predictions'] == plain['num_predictions']
    changed = 0
    for name in val.split_sample_names:
        a = _lines(os.path.join(plain['kitti_predictions_dir'], name + '.txt'))
        b = _lines(os.path.join(fitted['kitti_predictions_dir'], name + '.txt'))
        assert len(a) == len(b) == len(status.get(name, ()))
        for la, lb, st in zip(a, b, status.get(name, ())):
            assert la[:8] == lb[:8] and la[8:11] == lb[8:11]  # the class, alpha, the 2-D box and the dimensions stay
            if st == 2:
                assert la == lb
            else:
                changed += la != lb
    assert changed > 0

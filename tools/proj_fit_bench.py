"""Times the projection fit (csrc/proj_fit.hip) on seeded planted and noisy boxes.

    python tools/proj_fit_bench.py [--boxes 256] [--launches 20] [--warmup 3] [--scipy 8]

256 boxes of 48 x 48 points (tests/proj_fit_cases.py's generator: every second box noisy), fitted with n = 2
(xz_dist, centroid_y) and n = 3 (and the viewing angle).  Reports, as one JSON line:
  * fit_ms: the median device time of one mpsr_proj_fit launch on prepared tensors (events around the bare library
    call, for each of --launches launches after --warmup), and its minimum and maximum;
  * wrapper_ms: the same around instance_metrics.fit_proj_error, which also stacks the start, converts and reshapes its
    arguments and allocates the six outputs: the host's enqueue latency is inside that window;
  * evals_per_box / iters_per_box: the mean of the kernel's counts; status: how many boxes converged / stopped at the cap;
  * us_per_evaluation: fit_ms (the bare launch) over the evaluations of the slowest box (the launch lasts as long as its longest fit);
  * with --scipy N: scipy_ms_per_box, the host time of scipy.optimize.minimize(method='Nelder-Mead') on the numpy
    float64 restatement of the objective (tests/proj_fit_restatement.py) for the first N of the same boxes, and the
    largest difference of the float64 objective at the two results.
A measurement path that finds no GPU fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--boxes', type=int, default=256)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--scipy', type=int, default=0, help='also fit this many of the boxes with SciPy on the host')
    a = ap.parse_args()
    import torch
    import proj_fit_cases as C
    from monopsr_amd import _lib
    from monopsr_amd.core.instances import instance_metrics
    if not torch.cuda.is_available():
        raise SystemExit('proj_fit_bench needs a GPU')
    dev = torch.device('cuda', 0)
    L = C._launch(2024, 48, 48, ['planted', 'noisy'] * (a.boxes // 2) + ['planted'] * (a.boxes % 2), {})
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    local, boxes, cams = t(L['local']).reshape(L['b'], 48, 48, 3), t(L['boxes']), t(L['cams'])
    mask, index = t(L['mask']), t(L['cam_index'])
    result = dict(boxes=L['b'], map=[48, 48], launches=a.launches)
    for n_fit in (2, 3):
        x0 = t(L['x0'][n_fit])

        def wrapper():
            return instance_metrics.fit_proj_error(local, boxes, cams, x0[:, 0], x0[:, 1], x0[:, 2],
                                                   fit_viewing_angle=n_fit == 3, valid_mask=mask, cam_index=index)
        fit = wrapper()
        # the bare launch: the wrapper's arguments prepared once, its outputs written again and again
        flat = local.reshape(L['b'], 48 * 48, 3).contiguous()
        cam_flat = cams.reshape(-1).contiguous()
        lib, stream = _lib.lib(), _lib.stream()

        def bare():
            _lib.check(lib.mpsr_proj_fit(
                _lib.ptr(flat), _lib.ptr(x0), _lib.ptr(boxes), _lib.ptr(cam_flat), cam_flat.numel() // 12,
                _lib.ptr(index), _lib.ptr(mask), L['b'], 48, 48, n_fit, 1, 1, 0, 0, 1e-4, 1e-4, 0, _lib.ptr(fit.x),
                _lib.ptr(fit.err), _lib.ptr(fit.err0), _lib.ptr(fit.iters), _lib.ptr(fit.evals), _lib.ptr(fit.status),
                stream))

        def timed(run):
            for _ in range(a.warmup):
                run()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            return times
        wrapped = timed(wrapper)
        before = [t.clone() for t in fit[:6]]
        times = timed(bare)
        assert all(torch.equal(a_, b_) or bool((a_.isnan() == b_.isnan()).all()) for a_, b_ in zip(before, fit[:6]))
        evals, status = fit.evals.cpu().numpy(), fit.status.cpu().numpy()
        r = dict(fit_ms=float(np.median(times)), fit_ms_min=float(min(times)), fit_ms_max=float(max(times)),
                 wrapper_ms=float(np.median(wrapped)),
                 evals_per_box=float(evals.mean()), evals_max=int(evals.max()),
                 iters_per_box=float(fit.iters.float().mean()),
                 status=[int((status == k).sum()) for k in range(3)],
                 us_per_evaluation=float(np.median(times)) * 1e3 / max(1, int(evals.max())),
                 mean_err0=float(fit.err0.mean()), mean_err=float(fit.err.mean()))
        if a.scipy:
            from scipy.optimize import minimize
            x = fit.x.cpu().numpy()
            worst, t0 = 0.0, time.perf_counter()
            got = []
            for k in range(min(a.scipy, L['b'])):
                start = L['x0'][n_fit][k].astype(np.float64)
                func = lambda v: C.objective_at(L, k, np.asarray(list(v) + list(start[len(v):]), np.float32))
                got.append(minimize(func, start[:n_fit], method='Nelder-Mead', options=dict(xatol=1e-4, fatol=1e-4)))
            r['scipy_ms_per_box'] = (time.perf_counter() - t0) * 1e3 / len(got)
            r['scipy_evals_per_box'] = float(np.mean([g.nfev for g in got]))
            for k, g in enumerate(got):
                worst = max(worst, abs(C.objective_at(L, k, x[k]) - g.fun))
            r['objective_difference_px'] = worst
        result['n%d' % n_fit] = r
    print(json.dumps(result))
    return 0


if __name__ == '__main__':
    sys.exit(main())

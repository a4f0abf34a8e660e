"""What tests/test_shape_score_gpu.py and tests/test_surface_score_gpu.py share: buffers with guard elements around one
call of a C entry point, and the comparisons both make (the restatements: tests/shape_score_restatement.py)."""
import os

import numpy as np
import torch

from shape_score_restatement import same_bits, sum_bound


def device(array, offset):
    """The array on the device, `offset` elements into a larger allocation with one more element behind it."""
    if array is None:
        return None, None
    t = torch.from_numpy(np.array(array)).reshape(-1)
    whole = torch.zeros(t.numel() + offset + 1, dtype=t.dtype).cuda()
    whole[offset:offset + t.numel()] = t.cuda()
    return whole, whole[offset:offset + t.numel()]


def guarded_call(inputs, shapes, workspace_bytes, launch, poison, offset):
    """One call with every output of shapes ({name: (shape, dtype)}) and the workspace `offset` elements into an
    allocation with a guard element behind it; poison fills them with NaN / 0xFF first (else with zeros).
    launch(pointers of the inputs, {name: pointer of the output}, pointer of the workspace) -> status.
    -> (status, {name: numpy array}, the buffers' values before)."""
    assert workspace_bytes % 8 == 0
    keep = [device(x, offset) for x in inputs]
    whole, view = {}, {}
    for name, (shape, dtype) in shapes.items():
        size = int(np.prod(shape))
        fill = (-1 if dtype == torch.int32 else float('nan')) if poison else 0
        whole[name] = torch.full((size + offset + 1,), fill, dtype=dtype, device='cuda')
        view[name] = whole[name][offset:offset + size]
    ws_whole = torch.full((workspace_bytes // 8 + offset + 1,), -1 if poison else 0, dtype=torch.int64, device='cuda')
    ws = ws_whole[offset:offset + workspace_bytes // 8]
    before = {k: v.clone() for k, v in whole.items()}
    p = lambda t: None if t is None else t.data_ptr()
    status = launch([p(v) for _, v in keep], {k: p(v) for k, v in view.items()}, p(ws))
    torch.cuda.synchronize()
    out = {k: view[k].cpu().numpy().reshape(shapes[k][0]) for k in shapes}
    # the guard elements around every output and the workspace keep their fill
    for k in shapes:
        for at in list(range(offset)) + [-1]:
            assert same_bits(whole[k][at].cpu().numpy(), before[k][at].cpu().numpy()), (k, at)
    for at in list(range(offset)) + [-1]:
        assert int(ws_whole[at]) == (-1 if poison else 0)
    return status, out, before


def neighbours(got, want):
    """got is want or one of its float32 neighbours, NaN for NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    if not np.array_equal(nan, np.isnan(got)):
        return False
    lo, hi = np.nextafter(want, np.float32(-np.inf)), np.nextafter(want, np.float32(np.inf))
    return bool(((got[~nan] >= lo[~nan]) & (got[~nan] <= hi[~nan])).all())


def output_bytes(out, names):
    return b''.join(out[k].tobytes() for k in names)


def assert_sums_within_the_bound(name, got_sums, want, exact=()):
    """The four sums within (m + 2) 2^-52 sum |term| (one ulp per root plus any summation order: sum_bound); NaN and
    +inf where the restatement has them (an empty side, an overflow); the columns of `exact` bit for bit."""
    gs, ws = got_sums[:, 0:4], want['sums'][:, 0:4]
    special = ~np.isfinite(ws)
    assert same_bits(np.where(special, gs, 0.0), np.where(special, ws, 0.0)), name
    bound = sum_bound(want['terms'], np.where(special, 0.0, want['abs_sums']))
    err = np.abs(np.where(special, 0.0, gs) - np.where(special, 0.0, ws))
    print('%s: largest sum error %.3g of its bound' % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert bool((err <= bound).all()), (name, float(err.max()))
    for k in exact:
        assert same_bits(gs[:, k], ws[:, k]), (name, k)


def same_elsewhere(plain, scored, extra, val):
    """An evaluator's result with a scoring option is the plain one but for the keys of `extra`."""
    assert set(scored) - set(plain) == extra
    for key in plain:
        if key in ('kitti_predictions_dir', 'metrics_csv', 'breakdown_csv'):
            continue
        if key == 'kitti':
            assert scored['report'] == plain['report']
            continue
        assert repr(scored[key]) == repr(plain[key]), key
    for name in val.split_sample_names:
        with open(os.path.join(plain['kitti_predictions_dir'], name + '.txt'), 'rb') as a, \
                open(os.path.join(scored['kitti_predictions_dir'], name + '.txt'), 'rb') as b:
            assert a.read() == b.read(), name
    for a, b in zip(plain['metrics_csv'], scored['metrics_csv']):
        assert open(a, 'rb').read() == open(b, 'rb').read()

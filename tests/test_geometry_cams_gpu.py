"""Per-box cameras and per-instance loss scales of geometry.hip: mpsr_proj_err_norm(_grad)_cams,
mpsr_depth_map_local_to_global(_grad)_cams and mpsr_huber_loss_grad_scales against the single-camera / single-scale entry
points they generalise.  A box's arithmetic must not depend on the route, so everything here is bit for bit.

Three cameras (the three distinct P2 of tests/golden/instance_fixture.npz) with 2, 5 and 1 boxes; 48x48 maps and a
non-square 6x10; one instance without a valid pixel."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'instance_fixture.npz'))
CAMS = np.stack([FIX['p2_000000'], FIX['p2_000001'], FIX['p2_000006']]).astype(np.float32)  # (3,3,4), all different
COUNTS = (2, 5, 1)
SIZES = [(48, 48), (6, 10)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _case(h, w):
    """Inputs of B = 8 boxes on the device + cam_index + the per-camera row ranges."""
    rng = np.random.default_rng(100 * h + w)
    n = sum(COUNTS)
    y1, x1 = rng.uniform(0, 200, n), rng.uniform(0, 1000, n)
    boxes = np.stack([y1, x1, y1 + rng.uniform(20, 170, n), x1 + rng.uniform(20, 220, n)], 1).astype(np.float32)
    xyz = np.empty((n, h, w, 3), np.float32)
    xyz[..., 2] = rng.uniform(6, 40, (n, h, w))
    xyz[..., 0] = rng.uniform(-0.5, 0.5, (n, h, w)) * xyz[..., 2]
    xyz[..., 1] = rng.uniform(-0.1, 0.15, (n, h, w)) * xyz[..., 2]
    xyz[0, 0, 0] = [500.0, 0.0, 5.0]  # far off: the clip
    mask = (rng.uniform(size=(n, h, w)) > 0.3).astype(np.float32)
    mask[3] = 0  # an instance without a valid pixel
    c = dict(xyz=_dev(xyz), boxes=_dev(boxes), mask=_dev(mask), cams=_dev(CAMS.reshape(3, 12)),
             gnorm=_dev(rng.standard_normal(n).astype(np.float32)),
             z=_dev(rng.uniform(6, 40, n).astype(np.float32)), va=_dev(rng.uniform(-0.6, 0.6, n).astype(np.float32)),
             gdepth=_dev(rng.standard_normal((n, h, w)).astype(np.float32)),
             index=_dev(np.repeat(np.arange(3), COUNTS).astype(np.int32)))
    lo = np.concatenate([[0], np.cumsum(COUNTS)])
    c['ranges'] = [(int(lo[i]), int(lo[i + 1])) for i in range(3)]
    assert not np.array_equal(CAMS[0], CAMS[1]) and not np.array_equal(CAMS[1], CAMS[2]) \
        and not np.array_equal(CAMS[0], CAMS[2])
    return c


def _run(c, h, w, rotate, rows=None, cam=None, index='none', n_cams=3):
    """All four operators on the boxes `rows` -> dict of outputs.  cam: a camera number = the OLD single-camera entry
    points on that camera; None = the _cams entry points with `index` (a tensor, or None for a NULL index)."""
    from monopsr_amd import _lib
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    lo, hi = rows if rows is not None else (0, c['xyz'].shape[0])
    n = hi - lo
    xyz, boxes, mask = c['xyz'][lo:hi].contiguous(), c['boxes'][lo:hi].contiguous(), c['mask'][lo:hi].contiguous()
    gnorm, z, va = c['gnorm'][lo:hi].contiguous(), c['z'][lo:hi].contiguous(), c['va'][lo:hi].contiguous()
    gdepth = c['gdepth'][lo:hi].contiguous()
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device='cuda')
    o = dict(maps=f(n, h, w, 2), norm=f(n), gxyz=f(n, h, w, 3), depth=f(n, h, w), gz=f(n))
    if cam is not None:
        P = c['cams'][cam].contiguous()
        _lib.check(lib.mpsr_proj_err_norm(p(xyz), p(boxes), p(P), p(mask), p(o['maps']), p(o['norm']), n, h, w, st))
        _lib.check(lib.mpsr_proj_err_norm_grad(p(gnorm), p(xyz), p(boxes), p(P), p(mask), p(o['gxyz']), n, h, w, st))
        _lib.check(lib.mpsr_depth_map_local_to_global(xyz.data_ptr() + 8, 3, p(z), p(boxes), p(va), p(P), p(o['depth']),
                                                      n, h, w, rotate, st))
        _lib.check(lib.mpsr_depth_map_local_to_global_grad(p(gdepth), p(boxes), p(va), p(P), p(o['gz']), n, h, w, rotate,
                                                           st))
    else:
        P, ix = c['cams'], (None if index is None else index[lo:hi].contiguous())
        _lib.check(lib.mpsr_proj_err_norm_cams(p(xyz), p(boxes), p(P), n_cams, p(ix), p(mask), p(o['maps']),
                                               p(o['norm']), n, h, w, st))
        _lib.check(lib.mpsr_proj_err_norm_grad_cams(p(gnorm), p(xyz), p(boxes), p(P), n_cams, p(ix), p(mask),
                                                    p(o['gxyz']), n, h, w, st))
        _lib.check(lib.mpsr_depth_map_local_to_global_cams(xyz.data_ptr() + 8, 3, p(z), p(boxes), p(va), p(P), n_cams,
                                                           p(ix), p(o['depth']), n, h, w, rotate, st))
        _lib.check(lib.mpsr_depth_map_local_to_global_grad_cams(p(gdepth), p(boxes), p(va), p(P), n_cams, p(ix),
                                                                p(o['gz']), n, h, w, rotate, st))
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("rotate", [0, 1])
@pytest.mark.parametrize("h,w", SIZES)
def test_each_cameras_slice_equals_the_single_camera_entry_points(h, w, rotate):
    c = _case(h, w)
    got = _run(c, h, w, rotate, index=c['index'])
    for cam, (lo, hi) in enumerate(c['ranges']):
        want = _run(c, h, w, rotate, rows=(lo, hi), cam=cam)
        for k in want:
            assert torch.equal(got[k][lo:hi], want[k]), (k, cam)
        assert bool(torch.isfinite(want['norm']).all()) and bool(torch.isfinite(want['depth']).all())
    # the cameras matter: camera 0's boxes under camera 1 give other numbers
    lo, hi = c['ranges'][0]
    other = _run(c, h, w, rotate, rows=(lo, hi), cam=1)
    assert not torch.equal(other['norm'], got['norm'][lo:hi])
    assert torch.equal(other['depth'], got['depth'][lo:hi]) == (not rotate)  # read only when rotate_view is set


@pytest.mark.parametrize("h,w", SIZES)
def test_null_index_reads_the_first_camera_and_a_bad_index_gives_nan(h, w):
    from monopsr_amd import _lib
    c = _case(h, w)
    n = c['xyz'].shape[0]
    for rotate in (0, 1):
        first = _run(c, h, w, rotate, cam=0)
        null = _run(c, h, w, rotate, index=None)
        for k in first:
            assert torch.equal(null[k], first[k]), k
        good = _run(c, h, w, rotate, index=c['index'])
        for bad_value, row in ((3, 4), (-1, 0), (1 << 30, 7)):
            index = c['index'].clone()
            index[row] = bad_value
            before = _lib.lib().mpsr_last_error()
            got = _run(c, h, w, rotate, index=index)
            assert _lib.lib().mpsr_last_error() == before  # nothing recorded
            keep = torch.ones(n, dtype=torch.bool, device='cuda')
            keep[row] = False
            for k in got:
                assert torch.equal(got[k][keep], good[k][keep]), (k, bad_value)
                dependent = k in ('maps', 'norm', 'gxyz') or rotate
                if dependent:
                    assert bool(torch.isnan(got[k][row]).all()), (k, bad_value)
                else:
                    assert torch.equal(got[k][row], good[k][row]), (k, bad_value)


def test_host_mirror_routes_to_the_per_box_kernels():
    """instance_utils.proj_err_maps_norm / tf_inst_depth_map_local_to_global with cam_p (n_cams,3,4) + cam_index: values and
    gradients equal the single-camera calls per camera; a (3,4) camera without an index is the old call."""
    from monopsr_amd.datasets.kitti import instance_utils as iu
    h, w = 6, 10
    c = _case(h, w)
    cams = c['cams'].reshape(3, 3, 4)
    mask4 = c['mask'].reshape(-1, h, w, 1)

    def both(xyz, z, boxes, va, mask, cam_p, index):
        xyz, z = xyz.clone().requires_grad_(), z.clone().requires_grad_()
        norm, maps = iu.proj_err_maps_norm(xyz, boxes, cam_p, mask, want_maps=True, cam_index=index)
        depth = iu.tf_inst_depth_map_local_to_global(xyz[..., 2:3], z.reshape(-1, 1), boxes, va.reshape(-1, 1), (h, w),
                                                     cam_p, True, cam_index=index)
        (norm.sum() * 3 + (depth * depth).sum()).backward()
        return norm.detach(), maps, depth.detach(), xyz.grad, z.grad
    got = both(c['xyz'], c['z'], c['boxes'], c['va'], mask4, cams, c['index'])
    for cam, (lo, hi) in enumerate(c['ranges']):
        want = both(c['xyz'][lo:hi], c['z'][lo:hi], c['boxes'][lo:hi], c['va'][lo:hi], mask4[lo:hi], cams[cam], None)
        for g, wv in zip(got, want):
            assert torch.equal(g[lo:hi], wv), cam
    with pytest.raises(ValueError):
        iu.proj_err_maps_norm(c['xyz'], c['boxes'], cams, mask4)  # three cameras and no index
    with pytest.raises(ValueError):
        iu.proj_err_maps_norm(c['xyz'], c['boxes'], cams, mask4, cam_index=c['index'][:3])


@pytest.mark.parametrize("ch", [1, 3])
def test_huber_loss_grad_scales(ch):
    from monopsr_amd import _lib
    lib, p, st = _lib.lib(), _lib.ptr, _lib.stream()
    rng = np.random.default_rng(ch)
    b, P = 8, 6 * 10
    pred = _dev((rng.standard_normal((b, P, ch)) * 2).astype(np.float32))
    target = _dev(rng.standard_normal((b, P, ch)).astype(np.float32))
    weights = _dev((rng.uniform(size=(b, P)) > 0.3).astype(np.float32))
    weights[3] = 0
    one = _dev(np.array([0.37], np.float32))
    want, got = torch.empty_like(pred), torch.full_like(pred, 7.0)
    _lib.check(lib.mpsr_huber_loss_grad(p(pred), p(target), p(weights), p(one), b, P, ch, 1.0, p(want), st))
    _lib.check(lib.mpsr_huber_loss_grad_scales(p(pred), p(target), p(weights), p(one.repeat(b).contiguous()), b, P, ch,
                                               1.0, p(got), st))
    assert torch.equal(got, want)
    scales = _dev(rng.uniform(0.1, 2.0, b).astype(np.float32))
    _lib.check(lib.mpsr_huber_loss_grad_scales(p(pred), p(target), p(weights), p(scales), b, P, ch, 1.0, p(got), st))
    for i in range(b):
        row = torch.empty_like(pred[i:i + 1])
        _lib.check(lib.mpsr_huber_loss_grad(p(pred[i:i + 1].contiguous()), p(target[i:i + 1].contiguous()),
                                            p(weights[i:i + 1].contiguous()), p(scales[i:i + 1].contiguous()), 1, P, ch,
                                            1.0, p(row), st))
        assert torch.equal(got[i:i + 1], row), i
    assert float(got[3].abs().max()) == 0.0 and float(got.abs().max()) > 0

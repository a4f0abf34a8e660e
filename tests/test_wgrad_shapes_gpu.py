"""GPU half of the transform-domain weight-gradient sweep (tests/wgrad_shape_cases.py; the plans are asserted on the
host in tests/test_wgrad_shapes.py): the F(4x4,3x3) and F(3x3,3x3) weight-gradient kernels on ragged schedules -- partial
and dead K steps, steps that straddle images, maps one tile high or wide, FastDiv of 1 and of non-powers of two, an
early-returning group of workgroups -- against float64 on the WHOLE (N, 9 C) dw and the whole db.

The reference has no tiles, slices or transforms of its own: x padded by the dilation, and per tap (a, b) one float64
matrix product dy(M, N)^T @ x_shifted(a, b)(M, C); db = the column sums of dy.

Tolerance: the bound of tests/test_backward_gpu.py, 1e-4 of max |ref| (fp32 accumulation over up to 10^5 pixels; atomics
reorder sums); every case here has M <= 147456 pixels, the size at which the comparisons there hold it.  Measured on the
MI355X (DESIGN.md section 2 has the table): F(4x4,3x3) dw 5.8e-6 .. 1.2e-5, db 4.3e-7 .. 7.7e-7; F(3x3,3x3) dw and db
2.6e-7 .. 3.0e-7, with and without the bias gradient; the direct kernel on the same inputs dw 6.2e-7 .. 1.4e-6."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_shape_cases as S

pytestmark = pytest.mark.gpu

TOL = 1e-4
SENTINEL = 3.0e37  # scratch pre-fill of the F(4x4,3x3) form: finite, and anything it survives into is far off every bound


def _operands(case):
    """x = relu(randn), dy = randn (ReLU-masked in the F(3x3,3x3) cases): what tests/test_backward_gpu.py feeds them."""
    B, H, W, C, N = case.shape
    g = torch.Generator(device="cuda").manual_seed(1000 + 7 * B + C)
    x = torch.randn((B, H, W, C), device="cuda", generator=g).clamp_(min=0)
    dy = torch.randn((B, H, W, N), device="cuda", generator=g)
    if case.kind == 4:
        dy = dy * (torch.rand((B, H, W, N), device="cuda", generator=g) > 0.5)
    return x, dy


def _reference(case, x, dy):
    """float64: nine matrix products over the pixels, one per tap, and dy's column sums."""
    B, H, W, C, N = case.shape
    d, M = case.dil, case.pixels
    xp = F.pad(x.double(), (0, 0, d, d, d, d))
    dyt = dy.double().reshape(M, N).t().contiguous()
    dw = torch.empty((N, 9 * C), dtype=torch.float64, device="cuda")
    for a in range(3):
        for b in range(3):
            xs = xp[:, a * d:a * d + H, b * d:b * d + W, :].reshape(M, C)
            dw[:, (3 * a + b) * C:(3 * a + b + 1) * C] = dyt @ xs
    return dw, dyt.sum(1)


def _launch(case, x, dy, with_db=True):
    """mpsr_conv2d_wgrad_ws_f32 into a dw pre-filled with 0.25 and a db pre-filled with -0.5 (both are accumulated into);
    -> what the call added, in float64."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    B, H, W, C, N = case.shape
    dw = torch.full((N, 9 * C), 0.25, device="cuda")
    db = torch.full((N,), -0.5, device="cuda") if with_db else None
    nws = case.scratch_floats
    ws = torch.full((max(nws, 64),), SENTINEL, device="cuda")  # (a missing clear of the scratch would show)
    _lib.check(lib.mpsr_conv2d_wgrad_ws_f32(x.data_ptr(), dy.data_ptr(), B, H, W, C, N, 3, 3, case.dil, dw.data_ptr(),
                                            db.data_ptr() if with_db else None, ws.data_ptr(), max(nws, 64), _lib.stream()))
    torch.cuda.synchronize()
    return dw.double() - 0.25, (db.double() + 0.5) if with_db else None


def _err(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("case", S.NEW_CASES, ids=repr)
def test_wgrad_ragged_schedule_against_float64(case):
    from monopsr_amd import _lib
    lib = _lib.lib()
    # the kernel and the schedule first: a retuned threshold fails here instead of silently testing the direct kernel
    S.check_case_plan(case)
    x, dy = _operands(case)
    ref_dw, ref_db = _reference(case, x, dy)
    errs = {}
    dw, db = _launch(case, x, dy)
    errs["dw"], errs["db"] = _err(dw, ref_dw), _err(db, ref_db)
    if case.kind == 4:  # the training path of a BatchNorm layer: no bias gradient
        dw_nodb, _ = _launch(case, x, dy, with_db=False)
        errs["dw, db = NULL"] = _err(dw_nodb, ref_dw)
    # second witness: the direct kernel on the same inputs (switch off: the plan says so too)
    lib.mpsr_debug_set_wgrad_winograd(0)
    try:
        assert S.case_plan(case) == (0, 0, 0, 0)
        dw0, db0 = _launch(case, x, dy)
    finally:
        lib.mpsr_debug_set_wgrad_winograd(1)
    errs["dw vs direct"] = float((dw - dw0).abs().max() / dw0.abs().max())
    errs["db vs direct"] = float((db - db0).abs().max() / db0.abs().max())
    errs["direct dw"], errs["direct db"] = _err(dw0, ref_dw), _err(db0, ref_db)
    print("wgrad case %s %s dil %d, kind %d, %d tiles = %d slices x %d steps: %s" % (
        case.name, case.shape, case.dil, case.kind, case.tiles, case.nslices, case.steps,
        ", ".join("%s %.2e" % kv for kv in errs.items())))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, "%s (%s): over %.0e of max |ref|: %s" % (case.name, case.what, TOL, bad)
    # the kernels differ in the order of their sums: identical bits would mean the direct kernel ran twice (the plan is
    # the real check of that; this one is kept from the older tests)
    assert not torch.equal(dw, dw0)

"""Host-side half of the transform-domain weight-gradient sweep (tests/wgrad_shape_cases.py; the GPU half is
tests/test_wgrad_shapes_gpu.py): the plan -- which kernel mpsr_conv2d_wgrad_ws_f32 picks for every case and the slice
schedule it runs there -- the edge of the schedule each case is named for, and the fallbacks on the other side of every
floor.  mpsr_conv2d_wgrad_plan is host code of libmonopsr_hip.so and needs no GPU."""
import pytest

import wgrad_shape_cases as S


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_case_plans_its_kernel_and_schedule(case):
    kind, tiles, steps, nslices = S.check_case_plan(case)
    kt = S.KT[kind]
    # the table's own columns agree with each other and with the launchers' arithmetic restated
    assert tiles == case.B * case.tiles_per_image
    assert S.restated_schedule(kind, tiles, case.C, case.N) == (case.steps_raw, steps, nslices)
    assert steps % 2 == 0 and steps - case.steps_raw in (0, 1)
    assert (nslices - 1) * steps * kt < tiles <= nslices * steps * kt  # the last slice holds a tile, none is left over
    assert tiles - (nslices - 1) * steps * kt == case.last_live
    # the floor of its kernel is passed, and M stays where the older comparisons hold the file's 1e-4
    if kind == 3:
        assert case.pixels >= S.FLOOR_PIXELS and case.H % 4 == 0 and case.W % 4 == 0
    else:
        assert tiles >= S.FLOOR_TILES and case.H == case.W == 3 * case.dil
    assert case.pixels <= 147456
    assert (case.pixels * case.C + case.pixels * case.N) * 4 <= 0.31e9  # operands of the GPU half
    # the edges the case exists for
    assert case.edges and set(case.edges) <= set(S.EDGE_PREDICATES), case.name
    for name, want in case.edges.items():
        got = S.EDGE_PREDICATES[name](case, tiles, steps, nslices)
        assert got == want, "%s: %s is %r, the case exists for %r (%s)" % (case.name, name, got, want, case.what)


def test_sweep_reaches_every_edge_of_the_schedules():
    """Over the new cases, per kernel: a partial last step, a rounded step count, an early return, whole dead steps and
    a step that straddles images; FastDiv of 1, of a non-power of two and of a power of two; both signs of N - C; for
    F(4x4,3x3) both signs of H - W, a map one tile high, one tile wide and both, the 8-slice minimum and a single
    image.  The older tests' shapes have no partial step."""
    def vals(cases, name):
        return [S.EDGE_PREDICATES[name](c, c.tiles, c.steps, c.nslices) for c in cases]
    for kind in (3, 4):
        new = [c for c in S.NEW_CASES if c.kind == kind]
        old = [c for c in S.CASES if c.kind == kind and c not in S.NEW_CASES]
        assert len(old) == (1 if kind == 3 else 3)
        assert any(vals(new, "tiles_mod_kt")) and not any(vals(old, "tiles_mod_kt"))
        assert any(vals(new, "rounded")) and any(vals(new, "nslices_mod_8")) and any(vals(new, "straddle"))
        assert max(vals(new, "dead_steps")) >= 25
        divisors = {d for pair in vals(new, "fastdiv") for d in pair}
        assert 1 in divisors and any(d & (d - 1) for d in divisors)  # FastDiv(1) and of a non-power of two
        assert any(d > 1 and not d & (d - 1) for pair in vals(new + old, "fastdiv") for d in pair)  # ... of a power of two
        assert {-1, 1} <= set(vals(new, "n_ne_c"))
    w4 = [c for c in S.NEW_CASES if c.kind == 3]
    assert {-1, 1} <= {S.EDGE_PREDICATES["h_ne_w"](c, 0, 0, 0) for c in w4}
    shapes = {(c.H // 4 == 1, c.W // 4 == 1) for c in w4}
    assert shapes == {(False, False), (True, False), (False, True), (True, True)}
    assert any(512 // (c.N // 32 * (c.C // 32)) < 8 for c in w4) and any(c.B == 1 for c in w4)


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_below_the_floor_the_direct_kernel_serves(case):
    """The case's map and channels at the smallest batch that passes its kernel's floor, and one image fewer:
    conv_wgrad_kernel (kind 0, no schedule).  (A case's own batch is the first from the floor on that has its edge.)"""
    if case.kind == 3:
        floor_B = -(-S.FLOOR_PIXELS // (case.H * case.W))
    else:
        floor_B = -(-S.FLOOR_TILES // (case.dil * case.dil))
    assert S.case_plan(case, B=floor_B)[0] == case.kind
    assert S.case_plan(case, B=floor_B - 1) == (0, 0, 0, 0)
    assert floor_B <= case.B
    if case.name == "F":  # a single image has no smaller batch: a map one tile row shorter
        assert floor_B == 1 and S.wgrad_plan(1, case.H - 4, case.W, case.C, case.N, 3, 1, case.scratch_floats) == (0, 0, 0, 0)


@pytest.mark.parametrize("case", S.W4_CASES, ids=repr)
def test_f4_without_its_scratch_is_the_direct_kernel(case):
    assert S.case_plan(case, ws_floats=36 * case.N * case.C)[0] == 3
    assert S.case_plan(case, ws_floats=36 * case.N * case.C - 1) == (0, 0, 0, 0)
    assert S.case_plan(case, ws_floats=0) == (0, 0, 0, 0)


@pytest.mark.parametrize("case", S.W3_CASES, ids=repr)
def test_f3_needs_no_scratch(case):
    assert S.case_plan(case, ws_floats=0) == (4, case.tiles, case.steps, case.nslices)


def test_switch_off_plans_the_direct_kernel_everywhere():
    from monopsr_amd import _lib
    lib = _lib.lib()
    lib.mpsr_debug_set_wgrad_winograd(0)
    try:
        for case in S.CASES:
            assert S.case_plan(case) == (0, 0, 0, 0), case.name
    finally:
        lib.mpsr_debug_set_wgrad_winograd(1)
    for case in S.CASES:
        assert S.case_plan(case)[0] == case.kind  # (restored)


def test_pointwise_and_head_layers():
    """A 1x1 layer is conv_wgrad_kernel's, or pw_wgrad_direct_kernel's (kind 1) under mpsr_debug_set_wgrad_direct -- which
    moves no 3x3 layer; an N = 4 head is the thin kernel's (kind 2) at the channel counts it is instantiated for."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    assert S.wgrad_plan(256, 12, 12, 256, 1024, 1, 1, 0) == (0, 0, 0, 0)
    lib.mpsr_debug_set_wgrad_direct(1)
    try:
        assert S.wgrad_plan(256, 12, 12, 256, 1024, 1, 1, 0) == (1, 0, 0, 0)
        assert S.wgrad_plan(8, 12, 12, 256, 256, 3, 4, 0) == (0, 0, 0, 0)
        assert S.check_case_plan(S.BY_NAME["A"]) and S.check_case_plan(S.BY_NAME["G"])
    finally:
        lib.mpsr_debug_set_wgrad_direct(0)
    assert S.wgrad_plan(256, 12, 12, 256, 1024, 1, 1, 0) == (0, 0, 0, 0)
    assert S.wgrad_plan(32, 48, 48, 64, 4, 3, 1, 0) == (2, 0, 0, 0)
    assert S.wgrad_plan(32, 48, 48, 96, 4, 3, 1, 0) == (0, 0, 0, 0)   # not one of its channel counts
    assert S.wgrad_plan(32, 48, 48, 64, 4, 3, 2, 0) == (0, 0, 0, 0)   # atrous


def test_plan_checks_arguments_like_the_launch_and_takes_null_outputs():
    import ctypes
    from monopsr_amd import _lib
    lib = _lib.lib()
    a = S.BY_NAME["A"]
    assert lib.mpsr_conv2d_wgrad_plan(a.B, a.H, a.W, a.C, a.N, 3, 3, 1, a.scratch_floats, None, None, None, None) == 0
    kind = ctypes.c_int(-1)
    assert lib.mpsr_conv2d_wgrad_plan(a.B, a.H, a.W, a.C, a.N, 3, 3, 1, a.scratch_floats, ctypes.byref(kind), None, None,
                                      None) == 0 and kind.value == 3
    assert lib.mpsr_conv2d_wgrad_plan(1, 4, 4, 6, 8, 3, 3, 1, 0, ctypes.byref(kind), None, None, None) == 1
    assert b"multiples of 4" in lib.mpsr_last_error()
    assert lib.mpsr_conv2d_wgrad_plan(1, 4, 4, 8, 8, 2, 3, 1, 0, None, None, None, None) == 1  # even filter
    assert lib.mpsr_conv2d_wgrad_plan(1, 4, 4, 8, 8, 3, 3, 0, 0, None, None, None, None) == 1  # dilation 0
    assert lib.mpsr_conv2d_wgrad_plan(1 << 22, 4, 4, 8, 8, 3, 3, 1, 0, None, None, None, None) == 1  # 2^24 pixels
    assert lib.mpsr_conv2d_wgrad_plan(0, 4, 4, 8, 8, 3, 3, 1, 0, ctypes.byref(kind), None, None, None) == 0
    assert kind.value == 0  # empty batch: no launch at all

"""Host-side half of the direct batch-norm kernel tests (tests/batch_norm_cases.py; the GPU half is
tests/test_batch_norm_kernels_gpu.py): the float64 restatements the kernels are held to are checked against
torch.nn.functional.batch_norm under float64 autograd; every claim a case comment makes about the launch geometry is
asserted from the restated slicing / RowMap; the exact builders' exactness is verified; the summation bounds are shown
to be smaller than the effect of one dropped row; deliberately wrong variants of the kernels' loop and mask fail the
exact comparison by bit mismatch (on an emulation of the loop, here, never on the GPU); and the launchers' refusals
are exercised without a launch.

Rounding counts: APPLY_K = 2, GRAD_K = 5, MOVING_K = 4 (derived in tests/batch_norm_cases.py).  No tolerance in these
tests was tuned against the code under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import batch_norm_cases as B


# ================================================================================================ restatements

@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,C", [(2, 4), (7, 12), (129, 8), (33, 260)])
def test_composed_restatements_equal_torch_batch_norm_under_float64_autograd(M, C, relu):
    """stats -> finalize -> apply -> grad_sums -> grad_finalize -> grad, composed, against F.batch_norm(training=True)
    (+ ReLU) and its autograd: output, dz, dbeta and both moving statistics to 1e-12."""
    g = torch.Generator().manual_seed(M * 31 + C)
    z = (torch.randn((M, C), generator=g, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    beta = (torch.randn(C, generator=g, dtype=torch.float64) * 0.5).requires_grad_(True)
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    mm0, mv0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    eps, decay = B.f32(B.EPS), 0.5
    rm, rv = mm0.clone(), mv0.clone()
    y = F.batch_norm(z, rm, rv, None, beta, True, 1.0 - decay, eps)
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    got = B.composed_ref(z.detach(), beta.detach(), dy, relu, eps, decay, mm0, mv0)
    dbeta, _, _ = B.grad_finalize_ref(got.sum_g, got.sum_gz, float(M), None)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(got.y, y.detach()) and close(got.dz, z.grad) and close(got.sum_g, beta.grad)
    assert close(got.stats.moving_mean, rm) and close(got.stats.moving_variance, rv)
    assert not torch.equal(rm, mm0) and not torch.equal(rv, mv0)
    # ... and the same through autograd of the restatement itself (what the operator-level GPU test differentiates)
    z2 = z.detach().clone().requires_grad_(True)
    b2 = beta.detach().clone().requires_grad_(True)
    B.composed_ref(z2, b2, dy, relu, eps, decay, mm0, mv0, mask=got.mask).y.backward(dy)
    assert close(z2.grad, z.grad) and close(b2.grad, beta.grad)


def test_one_row_has_zero_variance_and_an_unbias_factor_of_one():
    z = torch.tensor([[3.0, -1.0, 0.5, 7.0]], dtype=torch.float64)
    s, q = B.stats_ref(z)
    st = B.finalize_ref(s, q, z[0], 1, 1e-3, 0.5, torch.ones(4), torch.ones(4))
    assert not s.any() and not q.any() and st.unbias == 1.0
    assert torch.equal(st.mean, z[0]) and not st.var.any()
    assert torch.equal(st.moving_variance, torch.full((4,), 0.5, dtype=torch.float64))


# ================================================================================================ geometry

@pytest.mark.parametrize("M", B.ROWS)
def test_slicing_claims(M):
    assert B.slicing(M) == B.SLICING_CLAIMS[M]
    blocks, rows, last = B.slicing(M)
    assert (blocks - 1) * rows + last == M and 1 <= last <= rows and blocks <= B.MAX_BLOCKS


def test_slicing_edges():
    assert [B.slicing(M)[0] for M in (256, 257)] == [1, 2]                  # one block up to M = 256
    assert (256 + 255) // 256 == 1 and (65536 + 255) // 256 == 256 and (65537 + 255) // 256 == 257  # the cap binds from 65537
    assert B.slicing(65537)[1] > 256 >= B.slicing(65536)[1]
    assert B.slicing(257)[1:] == (129, 128) and B.slicing(65537)[1:] == (257, 2)


@pytest.mark.parametrize("C", B.CHANNELS)
def test_row_map_claims(C):
    groups, rstride, idle = B.row_map(C)
    assert (groups, rstride, idle) == B.ROW_MAP_CLAIMS[C]
    assert groups * rstride + idle == B.R_THREADS and idle < groups
    assert (idle > 0) == (1024 % groups != 0)


def test_three_widths_do_not_divide_the_workgroup():
    assert [C for C in B.CHANNELS if B.row_map(C)[2]] == [12, 260, 1020]
    assert [B.row_map(C)[2] for C in (12, 260, 1020)] == [1, 49, 4]
    assert min(B.row_map(C)[1] for C in B.CHANNELS) == 4  # M = 3: fewer rows than thread rows at every C


@pytest.mark.parametrize("C", B.CHANNELS)
def test_unroll_boundary_cases_sit_on_the_boundary(C):
    st = B.row_map(C)[1]
    rows = [B.slicing(M)[1] for M in B.unroll_boundary_rows(C)]
    assert rows == [4 * st - 1, 4 * st, 4 * st + 1]
    # 4 st - 1: the last thread row takes no trip of the four-row loop and three tail rows, every other one trip, no tail
    assert B.unrolled_trips(rows[0], st, st - 1) == (0, 3)
    assert all(B.unrolled_trips(rows[0], st, r0) == (1, 0) for r0 in {0, st // 2, max(st - 2, 0)} - {st - 1})
    # 4 st: one trip, no tail, for every thread row
    assert {B.unrolled_trips(rows[1], st, r0) for r0 in range(st)} == {(1, 0)}
    # 4 st + 1: thread row 0 takes one trip and one tail row
    assert B.unrolled_trips(rows[2], st, 0) == (1, 1)
    assert all(B.unrolled_trips(rows[2], st, r0) == (1, 0) for r0 in range(1, st))
    for M in B.unroll_boundary_rows(C):  # every block of these cases is full
        blocks, r, last = B.slicing(M)
        assert last == r and blocks == (1 if r <= 256 else 256)


@pytest.mark.parametrize("C,M", [(C, M) for C in B.CHANNELS for M in [1, 3, 255, 256, 257, 513, 4097]] +
                         [(C, M) for C in (12, 260, 1020) for M in B.unroll_boundary_rows(C)] + [(1024, 65537), (260, 65537)])
def test_the_emulated_loops_visit_every_row_once(C, M):
    """thread_rows is the kernels' loop written out; with it every row of every block is visited exactly once."""
    assert bool((B.row_visits(M, C) == 1).all())


def test_the_large_case_takes_a_second_trip_of_the_grid_stride_loop():
    n4 = B.LARGE_M * (B.LARGE_C // 4)
    assert n4 > B.STREAM_MAX_BLOCKS * B.STREAM_THREADS == 2 ** 24
    assert B.stream_grid(n4) == B.STREAM_MAX_BLOCKS and B.second_trip_threads(B.LARGE_M, B.LARGE_C) == 4097
    assert all(B.second_trip_threads(M, C) == 0 for C, M in B.EXACT_CASES if M * (C // 4) <= 2 ** 24)
    # (1024, 65537) holds 256 more than 2^24 float4 as well: one workgroup's threads come back
    assert {(C, M): B.second_trip_threads(M, C) for C, M in B.EXACT_CASES if M * (C // 4) > 2 ** 24} == \
        {(1024, 65537): 256}
    assert B.terms_per_thread(4097, 260) == 17 and B.terms_per_thread(65537, 8) == 1 and B.terms_per_thread(65537, 1024) == 65
    assert B.slicing(1031) == (5, 207, 203)


# ================================================================================================ builders

@pytest.mark.parametrize("C,M", [(4, 1), (12, 3), (12, 257), (260, 61), (8, 513), (1020, 17)])
def test_exact_builder_keeps_every_intermediate_representable(C, M):
    p = B.exact_problem(M, C)
    assert p.z.abs().max() <= 8 and p.dy.abs().max() <= 8 and (p.z - p.z[0]).abs().max() <= 16
    assert (p.z - p.mean).abs().max() <= 11 and bool(((p.inv_std == 0.25) | (p.inv_std == 0.5) | (p.inv_std == 1) | (p.inv_std == 2)).all())
    for v in (p.beta, p.mean_g, p.mean_gz):
        assert torch.equal(v * 8, torch.round(v * 8))
    assert torch.equal(p.mean, torch.round(p.mean)) and p.mean_g.abs().max() <= 1 and p.mean_gz.abs().max() <= 2

    def fits(x64):  # survives the round trip through float32
        return torch.equal(x64.float().double(), x64)

    a = B.preact_ref(p.z, p.mean, p.inv_std, p.beta)
    zc = p.z.double() - p.mean.double()
    zhat = zc * p.inv_std.double()
    mask = a > 0
    g = B.masked(p.dy, mask)
    r = g - p.mean_g.double() - zhat * p.mean_gz.double()
    d = p.z.double() - p.z.double()[0]
    for x in (a, zc, zhat, g * zc, g * zhat, zhat * p.mean_gz.double(), g - p.mean_g.double(), r, p.inv_std.double() * r, d, d * d):
        assert fits(x)
    # per-thread partials: n terms, each at most 256 (squares) or 176 in steps of 1/4
    assert (d * d).max() <= 256 and (g * zhat).abs().max() <= 176 and torch.equal(g * zhat * 4, torch.round(g * zhat * 4))
    assert 704 * p.n < B.EXACT_LIMIT
    # the ties: exactly zero where j = 0, one step either side where j = +-1, on every planted row -- with a gradient
    planted = a[B.planted_rows(M)]
    assert planted.shape[0] == (M + B.PLANT_EVERY - 2) // B.PLANT_EVERY or M == 1 and planted.shape[0] == 1
    assert torch.equal(planted, (p.j.double() / 8).expand_as(planted)) and bool((p.dy[B.planted_rows(M)] == 5).all())
    share = float((a == 0).double().mean())
    assert share >= 1 / (B.PLANT_EVERY * 3 + 2) and bool(((a == 0) & (p.dy != 0)).any())
    if M * C >= 36:
        assert bool((a == 0.125).any()) and bool((a == -0.125).any())


def test_exact_builder_precondition_holds_on_every_case():
    for C, M in B.EXACT_CASES + [(B.LARGE_C, B.LARGE_M)]:
        n = B.terms_per_thread(M, C)
        assert 256 * n < B.EXACT_LIMIT and 704 * n < B.EXACT_LIMIT
    assert max(B.terms_per_thread(M, C) for C, M in B.EXACT_CASES) == 65


# ================================================================================================ bounds

def test_summation_bounds_are_smaller_than_one_dropped_row_everywhere():
    """A reducing kernel that drops one average row changes a channel's sum by sum|term| / M; the bound is
    (n + 3) u sum|term| at most.  So the bound sees the row wherever (n + 3) u M < 1 -- which holds at EVERY real-valued
    and conditioning case (the list of cases that must rely on the exact tests alone is empty); the worst is
    (1020, 65537) and (1024, 65537) with n = 65, at 0.27."""
    worst = {}
    for C, M in B.REAL_CASES + [(c[2], c[1]) for c in B.CONDITIONING_CASES] + [(C, M) for M, C in B.OPERATOR_CASES]:
        worst[(C, M)] = (B.terms_per_thread(M, C) + 3) * B.U * M
    assert [k for k, v in worst.items() if v >= 1] == []
    assert max(worst.values()) == worst[(1024, 65537)] == worst[(1020, 65537)] and 0.26 < worst[(1024, 65537)] < 0.27


@pytest.mark.parametrize("C,M", [(12, 257), (260, 257), (8, 4097)])
def test_summation_bounds_see_a_dropped_row_on_the_drawn_inputs(C, M):
    """The same on the inputs the GPU test draws: dropping the row closest to average in |z - z[0]| moves both sums by
    more than their bounds, in every channel."""
    g = torch.Generator().manual_seed(5)
    z = torch.randn((M, C), generator=g) * 2 + 1
    bS, bQ = B.stats_bounds(z, B.terms_per_thread(M, C))
    d = z.double() - z.double()[0]
    row = int((d.abs().mean(1) - d.abs().mean()).abs()[1:].argmin()) + 1
    assert bool((d[row].abs() > bS).float().mean() > 0.95) and bool(((d[row] ** 2) > bQ).float().mean() > 0.95)
    assert float((bS / d.abs().sum(0)).max()) < 1e-5


def test_conditioning_cases_keep_the_variance_bound_meaningful():
    """The derived variance bound is below 1e-2 of the true variance at each conditioning case (the GPU test asserts the
    same on the device before it trusts the bound)."""
    for name, M, C in B.CONDITIONING_CASES:
        z = B.conditioned_z(name, M, C, "cpu")
        sb = B.statistics_bounds(z, B.terms_per_thread(M, C), B.f32(B.EPS))
        print("%s: variance bound / variance = %.3e" % (name, float((sb.e_var / sb.var).max())))
        assert float((sb.e_var / sb.var).max()) < 1e-2
        rest = z[1:].double()
        if name.startswith("row 0"):
            assert 25 < float(((z[0] - rest.mean(0)) / rest.std(0)).abs().min())
        else:
            assert float((rest.mean(0) / rest.std(0)).min()) > 0.9 * float(name.split()[2])
            assert float(((z[0] - rest.mean(0)) / rest.std(0)).abs().max()) < 6  # an ordinary row 0


def test_ulp32_is_the_spacing_of_float32():
    x = torch.tensor([1.0, 1.5, 2.0, 0.75, 1e-3, 12345.678, -3.0], dtype=torch.float64)
    assert np.array_equal(B.ulp32(x).numpy(), np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


# ================================================================================================ mutation checks

MUTATION_CASES = [(4, 3), (12, 257), (260, 61), (8, 513), (1020, 17)]


@pytest.mark.parametrize("C,M", MUTATION_CASES)
def test_a_loop_that_drops_a_blocks_last_row_fails_the_exact_comparison(C, M):
    """The exact tests' power, shown on the host: sums taken with the emulated loop equal the restatement bit for bit,
    and the same loop with its tail one row short (the last row of every block dropped) does not -- in the channels the
    dropped rows are non-zero in, which is nearly all."""
    p = B.exact_problem(M, C)
    d = p.z.double() - p.z.double()[0]
    a = B.preact_ref(p.z, p.mean, p.inv_std, p.beta)
    g = B.masked(p.dy, a > 0)
    zhat = (p.z.double() - p.mean.double()) * p.inv_std.double()
    refs = B.stats_ref(p.z) + B.grad_sums_ref(p.dy, a > 0, p.z, p.mean, p.inv_std)
    for drop in (False, True):
        v = B.row_visits(M, C, drop_tail=drop)[:, None]
        got = [(v * t).sum(0) for t in (d, d * d, g, g * zhat)]
        same = [torch.equal(x, y) for x, y in zip(got, refs)]
        if not drop:
            assert all(same)
        else:
            assert int((v == 0).sum()) == B.slicing(M)[0]
            assert not same[1] and not same[2], same  # sum of squares and sum of g: a dropped row always shows somewhere
            assert float((got[1] != refs[1]).double().mean()) > 0.5


@pytest.mark.parametrize("C,M", MUTATION_CASES)
def test_a_mask_that_lets_zero_through_fails_the_exact_comparison(C, M):
    """`>= 0` in place of `> 0`: sum_g, sum_gz' companion dz, and the masked gradient all differ from the restatement
    bit for bit on the exact inputs (y itself cannot tell: relu(0) = 0 either way)."""
    p = B.exact_problem(M, C)
    a = B.preact_ref(p.z, p.mean, p.inv_std, p.beta)
    right, wrong = a > 0, a >= 0
    assert int((right != wrong).sum()) >= 1
    sg, _ = B.grad_sums_ref(p.dy, right, p.z, p.mean, p.inv_std)
    sg_wrong, _ = B.grad_sums_ref(p.dy, wrong, p.z, p.mean, p.inv_std)
    assert not torch.equal(sg, sg_wrong)
    dz = B.grad_ref(p.dy, right, p.z, p.mean, p.inv_std, p.mean_g, p.mean_gz)
    dz_wrong = B.grad_ref(p.dy, wrong, p.z, p.mean, p.inv_std, p.mean_g, p.mean_gz)
    assert not torch.equal(dz.float().view(torch.int32), dz_wrong.float().view(torch.int32))
    assert int((dz != dz_wrong).sum()) == int(((right != wrong) & (p.dy != 0)).sum())


# ================================================================================================ C-ABI refusals

OK_PTR, ODD_PTR = 0x10000, 0x10004  # fabricated addresses: passed ONLY to calls that are refused, never dereferenced


def _launchers():
    """name -> (call(M, C, pointers), names of its pointer arguments, those that may be NULL, those read as float4)."""
    from monopsr_amd import _lib
    lib = _lib.lib()

    def mk(fn, order):
        def call(M, C, p):
            return fn(*[M if a == "M" else C if a == "C" else None if a == "stream" else a[1] if isinstance(a, tuple) else p[a]
                        for a in order])
        return call

    relu = ("const", 1)
    return lib, {
        "stats": (mk(lib.mpsr_batch_norm_stats, ["z", "M", "C", "sum", "sumsq", "stream"]),
                  ["z", "sum", "sumsq"], [], ["z"]),
        "apply": (mk(lib.mpsr_batch_norm_apply, ["z", "M", "C", "mean", "inv_std", "beta", relu, "y", "stream"]),
                  ["z", "mean", "inv_std", "beta", "y"], [], ["z", "mean", "inv_std", "beta", "y"]),
        "grad_sums": (mk(lib.mpsr_batch_norm_grad_sums, ["dy", "y", "z", "M", "C", "mean", "inv_std", "sum_g", "sum_gz", "stream"]),
                      ["dy", "y", "z", "mean", "inv_std", "sum_g", "sum_gz"], ["y"], ["dy", "y", "z", "mean", "inv_std"]),
        "grad_sums_z": (mk(lib.mpsr_batch_norm_grad_sums_z,
                           ["dy", "z", "M", "C", "mean", "inv_std", "beta", "sum_g", "sum_gz", "stream"]),
                        ["dy", "z", "mean", "inv_std", "beta", "sum_g", "sum_gz"], [], ["dy", "z", "mean", "inv_std", "beta"]),
        "grad": (mk(lib.mpsr_batch_norm_grad, ["dy", "y", "z", "M", "C", "mean", "inv_std", "mean_g", "mean_gz", "dz", "stream"]),
                 ["dy", "y", "z", "mean", "inv_std", "mean_g", "mean_gz", "dz"], ["y"],
                 ["dy", "y", "z", "mean", "inv_std", "mean_g", "mean_gz", "dz"]),
        "grad_z": (mk(lib.mpsr_batch_norm_grad_z,
                      ["dy", "z", "M", "C", "mean", "inv_std", "beta", "mean_g", "mean_gz", "dz", "stream"]),
                   ["dy", "z", "mean", "inv_std", "beta", "mean_g", "mean_gz", "dz"], [],
                   ["dy", "z", "mean", "inv_std", "beta", "mean_g", "mean_gz", "dz"]),
        "finalize": (mk(lib.mpsr_batch_norm_finalize, ["sum", "sumsq", "z", "M", "C", ("const", 1e-3), ("const", 0.5),
                                                       "moving_mean", "moving_variance", "mean", "inv_std", "stream"]),
                     ["sum", "sumsq", "z", "moving_mean", "moving_variance", "mean", "inv_std"],
                     ["moving_mean", "moving_variance"], []),
    }


def _refused(lib, rc, *words):
    msg = lib.mpsr_last_error()
    assert rc != 0 and msg, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.parametrize("name", ["stats", "apply", "grad_sums", "grad_sums_z", "grad", "grad_z", "finalize"])
def test_launchers_refuse_bad_shapes_null_and_misaligned_pointers_before_any_launch(name):
    """C = 0, 6, 1028 and M = 0; each required pointer NULL in turn; each float4-read pointer four bytes off a multiple
    of 16 in turn (the optional y too, when given) -- status non-zero and a message, nothing launched."""
    lib, table = _launchers()
    call, ptrs, optional, vec = table[name]
    good = {p: OK_PTR for p in ptrs}
    for M, C in ((64, 0), (64, 6), (64, 1028), (0, 8), (-1, 8)):
        _refused(lib, call(M, C, good), b"batch_norm_" + name.encode())
    for p in ptrs:
        if p not in optional:
            _refused(lib, call(64, 8, dict(good, **{p: None})), b"null")
    for p in vec:
        _refused(lib, call(64, 8, dict(good, **{p: ODD_PTR})), b"misaligned")
        _refused(lib, call(64, 8, dict(good, **{p: OK_PTR + 8})), b"misaligned")
    # a refusal with the optional operands NULL is still about the operand that is wrong
    if optional and vec:
        _refused(lib, call(64, 8, dict(good, **{optional[0]: None, vec[0]: ODD_PTR})), b"misaligned")


def test_finalize_launchers_refuse_bad_scalars():
    """mpsr_batch_norm_finalize: eps < 0, decay outside [0, 1].  mpsr_batch_norm_grad_finalize takes a channel count of
    its own (any C > 0: it reads no float4) and the row count as `count`: C = 0, count = 0 and each required pointer
    NULL are refused."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    P = OK_PTR
    for eps, decay in ((-1e-3, 0.5), (1e-3, -0.1), (1e-3, 1.5)):
        _refused(lib, lib.mpsr_batch_norm_finalize(P, P, P, 64, 8, eps, decay, None, None, P, P, None), b"batch_norm_finalize")
    _refused(lib, lib.mpsr_batch_norm_grad_finalize(P, P, 64.0, 0, None, P, P, None), b"batch_norm_grad_finalize")
    _refused(lib, lib.mpsr_batch_norm_grad_finalize(P, P, 0.0, 8, None, P, P, None), b"batch_norm_grad_finalize")
    for i in (0, 1, 5, 6):
        args = [P, P, 64.0, 8, None, P, P, None]
        args[i] = None
        _refused(lib, lib.mpsr_batch_norm_grad_finalize(*args), b"null")

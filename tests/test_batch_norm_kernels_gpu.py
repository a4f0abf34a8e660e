"""The eight training-mode batch-norm entry points of csrc/batchnorm.hip, called directly through the C ABI and compared
with the float64 restatements of tests/batch_norm_cases.py: mpsr_batch_norm_stats, _finalize, _apply, _grad_sums,
_grad_sums_z, _grad_finalize, _grad and _grad_z.

EXACT tests are the row-coverage check: on inputs whose every fp32 intermediate is exactly representable the sums, y and
dz must equal the restatement bit for bit over the whole C x M grid (every RowMap geometry, every slicing branch, one
row either side of the four-row loop's boundary, the elementwise kernels' second grid-stride trip), with outputs placed
between sentinels and pre-filled with NaN / garbage.  BOUNDED tests run real-valued inputs against bounds derived from
the reference (rounding counts APPLY_K = 2, GRAD_K = 5, MOVING_K = 4; summation (n + 1) u and (n + 3) u with n the
per-thread term count -- see the cases module).  No tolerance or timing in this module was tuned against the code under
test.

Worst observed error / bound on an MI355X over all bounded cases (every bounded test prints its own):
  stats             sum 0.155, sumsq 0.105
  finalize          against the kernel's own sums, in ulp: mean, variance, inv_std 0.500 (the conversion's rounding)
                    against the statistics of z: mean 0.497, variance 0.140, inv_std 0.225
                    moving mean 0.497, moving variance 0.454
  apply             0.995 (two roundings, both counted: the bound is tight)
  grad_sums[_z]     sum_g 0.027, sum_gz 0.048
  grad_finalize     mean_g, mean_gz 0.500 ulp; dbeta bit-exact
  grad[_z]          dz 0.705
  operator          y 0.317, dz 0.266, dbeta 0.027, moving mean 0.164, moving variance 0.129
  conditioning      derived variance bound / variance 3.0e-5 (mean at 1e3 and 1e4 sigma), 4.4e-4 (row 0 at 30 sigma);
                    relative variance error 1.3e-7, 3.9e-7, 1.6e-7
"""
import numpy as np
import pytest
import torch

import batch_norm_cases as B

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 64          # elements on either side of an output (a multiple of 16 bytes in fp32 and fp64)
GARBAGE = -1.2345e6  # what the fp64 sums hold before a call: a launcher that accumulated would return it plus the sum
EPS = B.f32(B.EPS)
CASE_IDS = ["C%d-M%d" % c for c in B.EXACT_CASES]


def _api():
    from monopsr_amd import _lib
    return _lib, _lib.lib()


class _Guarded:
    """An output tensor of `shape` between two runs of sentinel values, itself pre-filled with `fill`."""

    def __init__(self, shape, fill=float("nan"), dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def check_guards(self, name):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), \
            name + ": wrote outside its output"


def _same_bits(got, ref64, name):
    """got (float32, device) against a float64 reference that float32 holds exactly: bit for bit."""
    want = ref64.float()
    assert torch.equal(want.double(), ref64), name + ": reference not representable"
    g, w = got.reshape(-1).view(torch.int32), want.reshape(-1).view(torch.int32)
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w).reshape(-1)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at flat index %d (got %r, want %r)" % (
            name, bad.numel(), g.numel(), i, float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def _same_sums(got, ref64, name):
    """fp64 sums: equal as values."""
    if not torch.equal(got, ref64):
        bad = torch.nonzero(~(got == ref64)).reshape(-1)
        i = int(bad[0])
        raise AssertionError("%s: %d of %d channels differ, first channel %d (got %r, want %r)" % (
            name, bad.numel(), got.numel(), i, float(got[i]), float(ref64[i])))


class _SumPair:
    """Two fp64 (C,) outputs holding garbage: one (2, C) allocation back to back, or two separate ones -- the two branches
    of the launchers' zeroing."""

    def __init__(self, C, together):
        if together:
            self.bufs = [_Guarded((2, C), GARBAGE, torch.float64)]
            self.a, self.b = self.bufs[0].t[0], self.bufs[0].t[1]
            assert self.b.data_ptr() == self.a.data_ptr() + 8 * C
        else:
            self.bufs = [_Guarded((C,), GARBAGE, torch.float64), _Guarded((C,), GARBAGE, torch.float64)]
            self.a, self.b = self.bufs[0].t, self.bufs[1].t
            assert self.b.data_ptr() != self.a.data_ptr() + 8 * C

    def check(self, ref_a, ref_b, name):
        _same_sums(self.a, ref_a, name + ": first sum")
        _same_sums(self.b, ref_b, name + ": second sum")
        for g in self.bufs:
            g.check_guards(name)


def _stats(z, pair):
    _lib, lib = _api()
    M, C = z.shape
    _lib.check(lib.mpsr_batch_norm_stats(z.data_ptr(), M, C, pair.a.data_ptr(), pair.b.data_ptr(), _lib.stream()))


def _apply(z, mean, inv_std, beta, relu, y):
    _lib, lib = _api()
    M, C = z.shape
    _lib.check(lib.mpsr_batch_norm_apply(z.data_ptr(), M, C, mean.data_ptr(), inv_std.data_ptr(), beta.data_ptr(), int(relu),
                                         y.data_ptr(), _lib.stream()))


def _grad_sums(dy, y, z, mean, inv_std, beta, pair):
    """beta given: the form that rebuilds the mask from z; else the form that reads y (y None: no mask)."""
    _lib, lib = _api()
    M, C = z.shape
    if beta is not None:
        _lib.check(lib.mpsr_batch_norm_grad_sums_z(dy.data_ptr(), z.data_ptr(), M, C, mean.data_ptr(), inv_std.data_ptr(),
                                                   beta.data_ptr(), pair.a.data_ptr(), pair.b.data_ptr(), _lib.stream()))
    else:
        _lib.check(lib.mpsr_batch_norm_grad_sums(dy.data_ptr(), None if y is None else y.data_ptr(), z.data_ptr(), M, C,
                                                 mean.data_ptr(), inv_std.data_ptr(), pair.a.data_ptr(), pair.b.data_ptr(),
                                                 _lib.stream()))


def _grad(dy, y, z, mean, inv_std, beta, mean_g, mean_gz, dz):
    _lib, lib = _api()
    M, C = z.shape
    if beta is not None:
        _lib.check(lib.mpsr_batch_norm_grad_z(dy.data_ptr(), z.data_ptr(), M, C, mean.data_ptr(), inv_std.data_ptr(),
                                              beta.data_ptr(), mean_g.data_ptr(), mean_gz.data_ptr(), dz.data_ptr(),
                                              _lib.stream()))
    else:
        _lib.check(lib.mpsr_batch_norm_grad(dy.data_ptr(), None if y is None else y.data_ptr(), z.data_ptr(), M, C,
                                            mean.data_ptr(), inv_std.data_ptr(), mean_g.data_ptr(), mean_gz.data_ptr(),
                                            dz.data_ptr(), _lib.stream()))


def _finalize(sums, z, eps, decay, mm, mv):
    """-> (mean, inv_std) as a (2, C) float tensor."""
    _lib, lib = _api()
    M, C = z.shape
    out = _Guarded((2, C))
    _lib.check(lib.mpsr_batch_norm_finalize(sums[0].data_ptr(), sums[1].data_ptr(), z.data_ptr(), M, C, eps, decay,
                                            None if mm is None else mm.data_ptr(), None if mv is None else mv.data_ptr(),
                                            out.t[0].data_ptr(), out.t[1].data_ptr(), _lib.stream()))
    out.check_guards("finalize")
    assert not bool(torch.isnan(out.t).any()) or bool(torch.isnan(sums).any())
    return out.t


# ================================================================================================ exact

@pytest.mark.parametrize("C,M", B.EXACT_CASES, ids=CASE_IDS)
def test_stats_are_exact_and_overwrite_their_outputs(C, M):
    """sum and sumsq_shifted equal the restatement exactly; what the outputs held before is gone (both placements of the
    pair); nothing outside them is written; z is not."""
    p = B.exact_problem(M, C, "cuda")
    before = p.z.clone()
    ref_s, ref_q = B.stats_ref(p.z)
    for together in (True, False):
        pair = _SumPair(C, together)
        _stats(p.z, pair)
        pair.check(ref_s, ref_q, "stats C=%d M=%d %s" % (C, M, "back to back" if together else "separate"))
    assert torch.equal(p.z, before)
    if M > 1:
        assert bool(ref_q.any())


def _exact_apply(p, relu):
    y = _Guarded((p.M, p.C))
    _apply(p.z, p.mean, p.inv_std, p.beta, relu, y.t)
    _same_bits(y.t, B.apply_ref(p.z, p.mean, p.inv_std, p.beta, relu), "apply C=%d M=%d relu=%d" % (p.C, p.M, relu))
    y.check_guards("apply")
    return y.t


@pytest.mark.parametrize("C,M", B.EXACT_CASES, ids=CASE_IDS)
def test_apply_is_exact(C, M):
    p = B.exact_problem(M, C, "cuda")
    before = p.z.clone()
    for relu in (0, 1):
        y = _exact_apply(p, relu)
    a = B.preact_ref(p.z, p.mean, p.inv_std, p.beta)
    assert bool((y[a == 0] == 0).all()) and int((a == 0).sum()) > 0
    assert torch.equal(p.z, before)


def _exact_backward(p, tag):
    """Every backward entry point on one exact problem, in all three mask forms (from y, rebuilt from z, none)."""
    a = B.preact_ref(p.z, p.mean, p.inv_std, p.beta)
    mask = a > 0
    ties = (a == 0) & (p.dy != 0)
    assert int(ties.sum()) > 0  # zero pre-activations with a gradient behind them: `>= 0` would let it through
    y = _exact_apply(p, 1)
    assert torch.equal(y > 0, mask)
    forms = [("mask from y", y, None, mask), ("mask from z", None, p.beta, mask), ("no mask", None, None, None)]
    for i, (form, yy, beta, mk) in enumerate(forms):
        name = "%s %s" % (tag, form)
        ref_g, ref_gz = B.grad_sums_ref(p.dy, mk, p.z, p.mean, p.inv_std)
        pair = _SumPair(p.C, together=(i + p.M) % 2 == 0)
        _grad_sums(p.dy, yy, p.z, p.mean, p.inv_std, beta, pair)
        pair.check(ref_g, ref_gz, "grad_sums " + name)
        dz = _Guarded((p.M, p.C))
        _grad(p.dy, yy, p.z, p.mean, p.inv_std, beta, p.mean_g, p.mean_gz, dz.t)
        want = B.grad_ref(p.dy, mk, p.z, p.mean, p.inv_std, p.mean_g, p.mean_gz)
        _same_bits(dz.t, want, "grad " + name)
        dz.check_guards("grad " + name)
        if mk is not None:  # the tie: with g = 0 there, dz = inv_std (-mean_g - zhat mean_gz)
            tie_ref = B.grad_ref(torch.zeros_like(p.dy), None, p.z, p.mean, p.inv_std, p.mean_g, p.mean_gz)
            assert torch.equal(dz.t[ties].double(), tie_ref[ties]), name + ": a zero pre-activation let its gradient through"


@pytest.mark.parametrize("C,M", B.EXACT_CASES, ids=CASE_IDS)
def test_backward_sums_and_dz_are_exact_in_all_three_mask_forms(C, M):
    """sum_g, sum_gz of _grad_sums / _grad_sums_z and dz of _grad / _grad_z, and both with y == NULL (no mask), equal the
    restatement exactly; a pre-activation of exactly zero masks its gradient on the y path and on the z path."""
    p = B.exact_problem(M, C, "cuda")
    before = (p.z.clone(), p.dy.clone())
    _exact_backward(p, "C=%d M=%d" % (C, M))
    assert torch.equal(p.z, before[0]) and torch.equal(p.dy, before[1])


def test_elementwise_kernels_on_the_large_case():
    """C = 4, M = 2^24 + 4097 (270 MB per tensor, built on the device): 4097 threads of _apply, _grad and _grad_z take a
    second trip of the grid-stride loop.  The reducing kernels run too (n = 65 terms per thread still satisfies the
    exactness precondition)."""
    p = None
    try:
        p = B.exact_problem(B.LARGE_M, B.LARGE_C, "cuda")
        _exact_apply(p, 0)
        _exact_backward(p, "large")
    finally:
        del p
        torch.cuda.empty_cache()


# ================================================================================================ bounded

def _ratio(name, got, ref, bound, ratios):
    r = B.worst_ratio((got.double() - ref).abs(), bound)
    ratios[name] = max(ratios.get(name, 0.0), r)
    assert r <= 1.0, "%s: error / bound = %.3f" % (name, r)


def _real_chain(z, dy, beta, tag):
    """stats -> finalize -> apply -> grad_sums(_z) -> grad_finalize -> grad(_z) on real-valued inputs, every stage held to
    its derived bound; returns the worst error / bound per stage."""
    M, C = z.shape
    n = B.terms_per_thread(M, C)
    ratios = {}
    # ---- stats
    pair = _SumPair(C, True)
    _stats(z, pair)
    sums = pair.bufs[0].t
    ref_s, ref_q = B.stats_ref(z)
    bS, bQ = B.stats_bounds(z, n)
    _ratio("stats sum", sums[0], ref_s, bS, ratios)
    _ratio("stats sumsq", sums[1], ref_q, bQ, ratios)
    pair.bufs[0].check_guards("stats")
    # ---- finalize: decay 0 from zero moving statistics shows (float)mean and (float)(var * unbias) themselves
    own = B.finalize_ref(sums[0], sums[1], z[0], M, EPS, 0.0)
    mm, mv = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    st = _finalize(sums, z, B.EPS, 0.0, mm, mv)
    mean, inv_std = st[0], st[1]
    assert torch.equal(mm, mean)
    _ratio("finalize mean vs own sums / ulp", mean, own.mean, B.ulp32(own.mean), ratios)
    _ratio("finalize inv_std vs own sums / ulp", inv_std, own.inv_std, B.ulp32(own.inv_std), ratios)
    _ratio("finalize variance vs own sums / ulp", mv, own.var * own.unbias, B.ulp32(own.var * own.unbias), ratios)
    sb = B.statistics_bounds(z, n, EPS)
    _ratio("finalize mean vs z", mean, sb.mean, sb.e_mean, ratios)
    _ratio("finalize inv_std vs z", inv_std, sb.inv_std, sb.e_inv_std, ratios)
    _ratio("finalize variance vs z", mv, sb.var * own.unbias, own.unbias * sb.e_var + B.ulp32(sb.var * own.unbias), ratios)
    if M == 1:
        assert own.unbias == 1.0 and not bool(mv.any()) and torch.equal(mean, z[0])
    g = torch.Generator(device="cuda").manual_seed(M + C)
    mm0, mv0 = torch.randn(C, device="cuda", generator=g), torch.rand(C, device="cuda", generator=g) + 0.5
    for decay in (0.5, 0.999):
        d32 = B.f32(decay)
        mm, mv = mm0.clone(), mv0.clone()
        st2 = _finalize(sums, z, B.EPS, decay, mm, mv)
        assert torch.equal(st2, st)
        # (the kernel rounds mean and var * unbias to float first: 1 ulp each, scaled by 1 - decay, on top of its arithmetic)
        _ratio("moving mean decay %g" % decay, mm, mm0.double() * d32 + (1 - d32) * own.mean,
               B.moving_bound(mm0, d32, own.mean), ratios)
        _ratio("moving variance decay %g" % decay, mv, mv0.double() * d32 + (1 - d32) * own.var * own.unbias,
               B.moving_bound(mv0, d32, own.var * own.unbias), ratios)
        assert not torch.equal(mm, mm0) and not torch.equal(mv, mv0)
        if M == 1 and decay == 0.5:
            assert torch.equal(mv, mv0 * 0.5)
    # NULL moving statistics: the same mean / inv_std, and a tensor that was not passed keeps its bits
    mm, mv = mm0.clone(), mv0.clone()
    assert torch.equal(_finalize(sums, z, B.EPS, 0.5, None, None), st)
    assert torch.equal(_finalize(sums, z, B.EPS, 0.5, None, mv), st)
    assert torch.equal(mm, mm0) and not torch.equal(mv, mv0)
    mv_only = mv.clone()
    assert torch.equal(_finalize(sums, z, B.EPS, 0.5, mm, None), st)
    assert not torch.equal(mm, mm0) and torch.equal(mv, mv_only)
    # ---- apply: the reference takes the kernel's own float vectors
    ys = {}
    for relu in (0, 1):
        y = _Guarded((M, C))
        _apply(z, mean, inv_std, beta, relu, y.t)
        _ratio("apply relu=%d" % relu, y.t, B.apply_ref(z, mean, inv_std, beta, relu), B.apply_bound(z, mean, inv_std, beta), ratios)
        y.check_guards("apply")
        ys[relu] = y.t
    assert torch.equal(ys[1], torch.clamp(ys[0], min=0.0))
    # ---- backward: the mask is the one the checked y gives
    y, mask = ys[1], ys[1] > 0
    for form, yy, bb, mk in (("y", y, None, mask), ("z", None, beta, mask), ("none", None, None, None)):
        pair = _SumPair(C, form != "z")
        _grad_sums(dy, yy, z, mean, inv_std, bb, pair)
        ref_g, ref_gz = B.grad_sums_ref(dy, mk, z, mean, inv_std)
        bG, bGZ = B.grad_sums_bounds(dy, mk, z, mean, inv_std, n)
        _ratio("grad_sums sum_g (mask %s)" % form, pair.a, ref_g, bG, ratios)
        _ratio("grad_sums sum_gz (mask %s)" % form, pair.b, ref_gz, bGZ, ratios)
        for gb in pair.bufs:
            gb.check_guards("grad_sums")
        # grad_finalize on the kernel's sums: (float)(sum / count) to an ulp, dbeta accumulated in fp32, NULL dbeta allowed
        _lib, lib = _api()
        db0 = torch.randn(C, device="cuda", generator=g)
        db, means = db0.clone(), _Guarded((2, C))
        _lib.check(lib.mpsr_batch_norm_grad_finalize(pair.a.data_ptr(), pair.b.data_ptr(), float(M), C, db.data_ptr(),
                                                     means.t[0].data_ptr(), means.t[1].data_ptr(), _lib.stream()))
        want_db, want_mg, want_mgz = B.grad_finalize_ref(pair.a, pair.b, float(M), db0)
        assert torch.equal(db, want_db)
        _ratio("grad_finalize mean_g / ulp", means.t[0], want_mg, B.ulp32(want_mg), ratios)
        _ratio("grad_finalize mean_gz / ulp", means.t[1], want_mgz, B.ulp32(want_mgz), ratios)
        means.check_guards("grad_finalize")
        means2 = torch.empty((2, C), device="cuda")
        _lib.check(lib.mpsr_batch_norm_grad_finalize(pair.a.data_ptr(), pair.b.data_ptr(), float(M), C, None,
                                                     means2[0].data_ptr(), means2[1].data_ptr(), _lib.stream()))
        assert torch.equal(means2, means.t)
        mg, mgz = means.t[0], means.t[1]
        dz = _Guarded((M, C))
        _grad(dy, yy, z, mean, inv_std, bb, mg, mgz, dz.t)
        _ratio("grad dz (mask %s)" % form, dz.t, B.grad_ref(dy, mk, z, mean, inv_std, mg, mgz),
               B.grad_bound(dy, mk, z, mean, inv_std, mg, mgz), ratios)
        dz.check_guards("grad")
    print("%s: worst error / bound: %s" % (tag, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
    return ratios


@pytest.mark.parametrize("C,M", B.REAL_CASES, ids=["C%d-M%d" % c for c in B.REAL_CASES])
def test_real_valued_inputs_stay_inside_the_derived_bounds(C, M):
    """z = randn * 2 + 1, dy = randn: every entry point against float64 within the bounds of the cases module."""
    g = torch.Generator(device="cuda").manual_seed(7919 * C + M)
    z = torch.randn((M, C), device="cuda", generator=g) * 2 + 1
    dy = torch.randn((M, C), device="cuda", generator=g)
    beta = torch.randn(C, device="cuda", generator=g) * 0.5
    _real_chain(z, dy, beta, "real C=%d M=%d" % (C, M))


@pytest.mark.parametrize("name,M,C", B.CONDITIONING_CASES, ids=[c[0].replace(" ", "_") for c in B.CONDITIONING_CASES])
def test_conditioning(name, M, C):
    """The per-channel mean 1e3 and 1e4 sigma from zero, and row 0 (the shift) 30 sigma from the rest: the same bounds.
    That the bound is not too loose to mean anything is asserted first: the derived variance bound is below 1e-2 of the
    true variance."""
    z = B.conditioned_z(name, M, C, "cuda")
    sb = B.statistics_bounds(z, B.terms_per_thread(M, C), EPS)
    loose = float((sb.e_var / sb.var).max())
    print("%s: derived variance bound / variance = %.3e" % (name, loose))
    assert loose < 1e-2
    g = torch.Generator(device="cuda").manual_seed(M)
    dy = torch.randn((M, C), device="cuda", generator=g)
    beta = torch.randn(C, device="cuda", generator=g) * 0.5
    ratios = _real_chain(z, dy, beta, name)
    mv = torch.zeros(C, device="cuda")
    pair = _SumPair(C, True)
    _stats(z, pair)
    _finalize(pair.bufs[0].t, z, B.EPS, 0.0, None, mv)
    rel = float(((mv.double() / (M / (M - 1)) - sb.var).abs() / sb.var).max())
    print("%s: relative variance error %.3e" % (name, rel))
    assert ratios["finalize variance vs z"] <= 1.0


# ================================================================================================ NaN

@pytest.mark.parametrize("M,C", B.NAN_CASES)
def test_a_nan_poisons_its_channel_and_no_other(M, C):
    """One NaN in one channel of z: every other channel's sum, sumsq, mean, inv_std, y and moving statistics keep their
    bits; in the poisoned channel the sums, mean, inv_std, BOTH moving statistics and y (before the ReLU, whose maximum
    with zero does not hand a NaN on) are NaN."""
    g = torch.Generator(device="cuda").manual_seed(M * C)
    z = torch.randn((M, C), device="cuda", generator=g) * 2 + 1
    beta = torch.randn(C, device="cuda", generator=g) * 0.5
    mm0, mv0 = torch.randn(C, device="cuda", generator=g), torch.rand(C, device="cuda", generator=g) + 0.5
    bad_row, bad = M // 3 + 1, C // 2 + 1
    out = {}
    for poisoned in (False, True):
        zz = z.clone()
        if poisoned:
            zz[bad_row, bad] = float("nan")
        pair = _SumPair(C, True)
        _stats(zz, pair)
        sums = pair.bufs[0].t
        mm, mv = mm0.clone(), mv0.clone()
        st = _finalize(sums, zz, B.EPS, 0.5, mm, mv)
        ys = []
        for relu in (0, 1):
            y = _Guarded((M, C))
            _apply(zz, st[0], st[1], beta, relu, y.t)
            y.check_guards("apply")
            ys.append(y.t)
        out[poisoned] = dict(sum=sums[0], sumsq=sums[1], mean=st[0], inv_std=st[1], moving_mean=mm, moving_variance=mv,
                             y=ys[0], y_relu=ys[1])
    keep = torch.arange(C, device="cuda") != bad
    for name in out[True]:
        a, b = out[False][name], out[True][name]
        assert not bool(torch.isnan(a).any()), name
        assert torch.equal(a[..., keep], b[..., keep]), name + ": a clean channel changed"
        if name != "y_relu":
            assert bool(torch.isnan(b[..., bad]).all()), name + ": the poisoned channel is not NaN"


# ================================================================================================ operator

@pytest.mark.parametrize("from_z", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("M,C", B.OPERATOR_CASES)
def test_operator_vs_float64_autograd_within_the_propagated_bounds(M, C, relu, from_z):
    """BatchNormReluFn.apply on a z tensor (no convolution in front), with and without ReLU, with the backward's mask
    rebuilt from z and read from y: y, dz, dbeta and both moving statistics against float64 autograd through the composed
    restatement, within the bounds of operator_bounds.  The reference uses the operator's own mask; where that differs
    from the float64 mask the pre-activation must be inside its own tolerance of zero."""
    from monopsr_amd.core import autograd_ops as ops
    g = torch.Generator(device="cuda").manual_seed(M + C)
    z = (torch.randn((M, C), device="cuda", generator=g) * 2 + 1).requires_grad_(True)
    dy = torch.randn((M, C), device="cuda", generator=g)
    beta = torch.randn(C, device="cuda", generator=g) * 0.5
    mm0, mv0 = torch.randn(C, device="cuda", generator=g), torch.rand(C, device="cuda", generator=g) + 0.5
    decay = 0.5
    layer = ops.LayerRef(None, beta, None, torch.zeros(C, device="cuda"), C, C, 1, 1, 1, relu)
    layer.batch_norm = ops.BatchNormState(mm0.clone(), mv0.clone(), eps=B.EPS, decay=decay)
    token = torch.zeros((), device="cuda", requires_grad=True)
    saved = ops.BN_MASK_FROM_Z
    ops.BN_MASK_FROM_Z = from_z
    try:
        y = ops.BatchNormReluFn.apply(z, layer, token)
        y.backward(dy)
    finally:
        ops.BN_MASK_FROM_Z = saved
    y = y.detach()
    mask = (y > 0) if relu else None
    n = B.terms_per_thread(M, C)
    ob = B.operator_bounds(z.detach(), beta, dy, mask, n, EPS, decay, mm0, mv0)
    # float64 autograd through the restatement
    z64 = z.detach().double().requires_grad_(True)
    b64 = beta.double().requires_grad_(True)
    ref = B.composed_ref(z64, b64, dy.double(), relu, EPS, decay, mm0, mv0, mask=mask)
    ref.y.backward(dy.double())
    assert float((z64.grad - ob.ref.dz).abs().max()) <= 1e-12 * float(ob.ref.dz.abs().max())
    if relu:
        flipped = mask != (ref.a.detach() > 0)
        assert bool((ref.a.detach().abs()[flipped] <= ob.y[flipped]).all())
        assert 0.2 < float(mask.float().mean()) < 0.9
    ratios = {}
    _ratio("operator y", y, ref.y.detach(), ob.y, ratios)
    _ratio("operator dz", z.grad, z64.grad, ob.dz, ratios)
    _ratio("operator dbeta", layer.db, b64.grad, ob.dbeta, ratios)
    _ratio("operator moving mean", layer.batch_norm.moving_mean, ob.ref.stats.moving_mean, ob.moving_mean, ratios)
    _ratio("operator moving variance", layer.batch_norm.moving_variance, ob.ref.stats.moving_variance, ob.moving_variance, ratios)
    print("operator M=%d C=%d relu=%d from_z=%d: worst error / bound: %s" % (
        M, C, relu, from_z, ", ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))

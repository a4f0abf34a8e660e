"""The optimiser tail called directly through the C ABI, off the trainer's table: mpsr_clip_by_norm_segments
(seg_sumsq_kernel, seg_sum_kernel, seg_scale_kernel) and mpsr_clip_adam_ema_step (the same norms, then
clip_adam_ema_kernel), csrc/optim.hip, against the float64 restatements of tests/optim_cases.py.

The tables, the kernel branch each one reaches, the exactness argument (gradients that are integers times 2^-6: sumsq
must equal the float64 sum BIT FOR BIT) and the derived error bounds are in that module.  The sumsq scratch is filled
with NaN before every call, and whatever lies outside every chunk must keep its bits.

Measured on an MI355X (worst case over the cases of each test; u = 2^-24; each test prints its own figures):
  sumsq, exact gradients              bit-identical to float64 on every table
  sumsq, standard_normal * 0.02       1.79 u relative (MANY_CHUNKS; bound 23 u for that segment), 0.04 u (FULL_CHUNKS; 82 u)
  clipped gradient, exact gradients   2.11 u relative (LONG_TABLE)                                bound 4 u
  clipped gradient, real-valued       1.79 u (MANY_CHUNKS; bound 17 u), 1.20 u (FULL_CHUNKS; bound 45 u)
  p, m, v, moving average             at most 0.048 of the tolerance rtol 1e-5 + 4 u, atol 1e-7 (test_fused_step_against_float64)
"""
import functools

import numpy as np
import pytest
import torch

import optim_cases as C

pytestmark = pytest.mark.gpu

NAN = float("nan")
LR, B1, B2, EPS, DECAY = 1e-2, 0.9, 0.999, 1e-8, 0.99


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared cases are read-only)


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(got, want, name):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at %d (got %r, want %r)" % (
        name, bad.size, g.size, bad[0], g[bad[0]:bad[0] + 1].view(np.float32)[0], w[bad[0]:bad[0] + 1].view(np.float32)[0])


@functools.lru_cache(maxsize=None)
def _device_table(name):
    t = C.THRESHOLD if name == "THRESHOLD" else C.TABLES[name]
    return t, (_dev(t.chunk_seg), _dev(t.chunk_begin), _dev(t.chunk_len))


def _scratch(t):
    return torch.full((t.n_segments + len(t.chunk_seg),), NAN, device="cuda")


def _clip(name, g, clip):
    """mpsr_clip_by_norm_segments on a fresh copy of g (host array) -> (clipped g, the whole sumsq scratch), on the host."""
    from monopsr_amd import _lib
    t, (seg, begin, length) = _device_table(name)
    gt, sumsq = _dev(g), _scratch(t)
    assert gt.numel() == t.size and gt.data_ptr() % 256 == 0  # begin % 4 == 0 <=> the 16-byte branch
    _lib.check(_lib.lib().mpsr_clip_by_norm_segments(_lib.ptr(gt), _lib.ptr(seg), _lib.ptr(begin), _lib.ptr(length),
                                                     len(t.chunk_seg), _lib.ptr(sumsq), sumsq.numel(), t.n_segments,
                                                     clip, _lib.stream()))
    return gt.cpu().numpy(), sumsq.cpu().numpy()


def _fused(name, state, g, clip, lr, step, decay=DECAY, with_sumsq=True):
    """mpsr_clip_adam_ema_step in place on state = [p, m, v, shadow or None] (device tensors); g is a device tensor.
    Returns the sumsq scratch on the host (None when called without one: sumsq NULL, n_segments 0)."""
    from monopsr_amd import _lib
    t, (seg, begin, length) = _device_table(name)
    assert all(a is None or (a.numel() == t.size and a.data_ptr() % 256 == 0) for a in state + [g])
    sumsq = _scratch(t) if with_sumsq else None
    _lib.check(_lib.lib().mpsr_clip_adam_ema_step(
        _lib.ptr(state[0]), _lib.ptr(g), _lib.ptr(state[1]), _lib.ptr(state[2]), _lib.ptr(state[3]), _lib.ptr(seg),
        _lib.ptr(begin), _lib.ptr(length), len(t.chunk_seg), _lib.ptr(sumsq), sumsq.numel() if with_sumsq else 0,
        t.n_segments if with_sumsq else 0, clip, lr, B1, B2, EPS, step, decay, _lib.stream()))
    return sumsq.cpu().numpy() if with_sumsq else None


def _adam_step(state, g, lr, step):
    """mpsr_adam_step with grad_scale 1 over the whole buffers, in place on state = [p, m, v]."""
    from monopsr_amd import _lib
    _lib.check(_lib.lib().mpsr_adam_step(_lib.ptr(state[0]), _lib.ptr(g), _lib.ptr(state[1]), _lib.ptr(state[2]),
                                         g.numel(), lr, B1, B2, EPS, step, 1.0, _lib.stream()))


def _rel_err(got, ref):
    """Worst relative error over the non-zero reference elements; where the reference is zero the result must be."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    zero = ref == 0
    assert (got[zero] == 0).all(), "a zero did not stay zero"
    if zero.all():
        return 0.0, np.zeros(ref.shape)
    err = np.zeros(ref.shape)
    err[~zero] = np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])
    return float(err.max()), err


def _check_clip(name, t, g, got, sumsq, clip, element_bound):
    """The clipped gradient against clip_ref: within element_bound (per segment) where scaled, the same bits where not,
    and the same bits outside every chunk.  Returns the worst relative error."""
    ref_sumsq, ref = C.clip_ref(g, t, clip)
    idx, seg = C.elements(t)
    scaled = (np.sqrt(ref_sumsq) > clip)[seg]
    worst, err = _rel_err(got[idx], ref[idx])
    over = np.nonzero(err > element_bound[seg])[0]
    assert over.size == 0, "%s: %d elements past the bound, first at %d: %.3e > %.3e (got %r, want %r)" % (
        name, over.size, idx[over[0]], err[over[0]], element_bound[seg][over[0]], got[idx][over[0]], ref[idx][over[0]])
    _same_bits(got[idx][~scaled], g[idx][~scaled], name + ": a segment at or under the threshold")
    gaps = ~C.covered(t)
    _same_bits(got[gaps], g[gaps], name + ": outside every chunk")
    return worst


# ================================================================================================ clip_by_norm_segments

@pytest.mark.parametrize("name", sorted(C.TABLES))
def test_clip_by_norm_exact_gradients(name):
    """Every table with gradients that are integers times 2^-6: sumsq[:n_segments] equals the float64 sums bit for bit,
    a segment without chunks gets exactly 0 (the scratch came filled with NaN), the clipped gradient is within 4 u of
    clip_ref, segments at or under the threshold and everything outside the chunks keep their bits, and a second run
    gives the same bits.  Measured worst clipped-gradient error (bound 4 u): ALIGNMENT 2.08 u, MANY_CHUNKS 1.61 u,
    EMPTY_MIDDLE 1.01 u, EMPTY_FRONT 0.57 u, ONE_CHUNK 0 (not scaled), LONG_TABLE 2.11 u = 1.26e-7, FULL_CHUNKS 0.79 u."""
    t = C.TABLES[name]
    g, ref_sumsq, _ = C.exact_case(name)
    got, sumsq = _clip(name, g, C.EXACT_CLIP)
    _same_bits(sumsq[:t.n_segments], ref_sumsq.astype(np.float32), name + ": sumsq")
    empty = C.chunks_per_segment(t) == 0
    assert (_bits(sumsq[:t.n_segments])[empty] == 0).all(), "an empty segment's norm must be written as +0"
    assert np.isfinite(sumsq).all(), "a chunk's partial sum was not written"
    worst = _check_clip(name, t, g, got, sumsq, C.EXACT_CLIP, np.full(t.n_segments, C.CLIP_EXACT_BOUND))
    print("clip exact %s: worst clipped-gradient error %.3e = %.2f u (bound 4 u)" % (name, worst, worst / C.U))
    again, sumsq2 = _clip(name, g, C.EXACT_CLIP)
    _same_bits(again, got, name + ": second run, gradient")
    _same_bits(sumsq2, sumsq, name + ": second run, sumsq and partials")


@pytest.mark.parametrize("unit", [1.0, C.GRAD_UNIT], ids=["clip5", "clip5_2e-6"])
def test_clip_at_the_threshold_is_strict(unit):
    """norm == clip is NOT scaled (sumsq 25 and 0 against clip 5: the bits stay), sumsq 26 is; the same at 2^-6."""
    t = C.THRESHOLD
    g = C.threshold_grad(unit)
    clip = C.THRESHOLD_CLIP * unit
    got, sumsq = _clip("THRESHOLD", g, clip)
    _same_bits(sumsq[:t.n_segments], (np.array([25, 25, 0, 26, 25, 26]) * unit ** 2).astype(np.float32), "sumsq")
    _check_clip("THRESHOLD", t, g, got, sumsq, clip, np.full(t.n_segments, C.CLIP_EXACT_BOUND))
    idx, seg = C.elements(t)
    moved = np.isin(seg, C.THRESHOLD_SCALED)
    assert (got[idx][moved] != g[idx][moved]).all(), "sumsq 26 must be scaled"
    # the fused step decides the same way: one step from m = v = 0, where p moves by -lr_t m / (sqrt(v) + eps)
    state = [_dev(np.zeros(t.size, np.float32)) for _ in range(4)]
    f_sumsq = _fused("THRESHOLD", state, _dev(g), clip, LR, 1)
    _same_bits(f_sumsq[:t.n_segments], sumsq[:t.n_segments], "fused sumsq")
    ref = C.clip_adam_ema_ref(*[np.zeros(t.size)] * 4, g, t, clip, LR, B1, B2, EPS, 1, DECAY)
    m = state[1].cpu().numpy()
    np.testing.assert_allclose(m[idx], ref[1][idx], rtol=C.ADAM_RTOL, atol=0)
    # (an unscaled m is (1 - b1) g: the scaled one is smaller by 5 / sqrt(26) = 0.98, 2e5 times the tolerance)
    _same_bits(m[idx][~moved], (np.float32(1) - np.float32(B1)) * g[idx][~moved], "m of the unscaled segments")


def test_infinite_norm_against_infinite_clip_is_norm_equal_clip():
    """The one input on which `norm > clip` and `norm >= clip` differ.  For a finite norm == clip the scale would be
    clip / norm == 1 exactly and g * 1 has g's bits, so the two rules cannot be told apart; with clip = +inf (clipping
    switched off by its threshold) and a segment that holds +inf the norm equals the clip, and by the documented strict
    rule the segment keeps its bits -- a `>=` would scale by inf / inf = NaN and wipe out the variable's finite
    elements too.  (tf.clip_by_norm's g * clip / max(norm, clip) has no answer here, it is inf / inf for every element;
    what is pinned is the strictness the header documents.)"""
    t = C.THRESHOLD
    idx, seg = C.elements(t)
    g = C.threshold_grad(1.0)
    inf_at, beside = idx[seg == 0]
    g[inf_at] = np.inf
    ref_sumsq, ref = C.clip_ref(g, t, np.inf)
    assert ref_sumsq[0] == np.inf and np.array_equal(ref[idx], g[idx].astype(np.float64))
    got, sumsq = _clip("THRESHOLD", g, float("inf"))
    _same_bits(sumsq[:t.n_segments], ref_sumsq.astype(np.float32), "sumsq")
    _same_bits(got, g, "no segment's norm exceeds +inf: every bit stays")
    state = [_dev(np.zeros(t.size, np.float32)) for _ in range(4)]
    _fused("THRESHOLD", state, _dev(g), float("inf"), LR, 1)
    m = state[1].cpu().numpy()
    assert np.isinf(m[inf_at])
    keep = idx[idx != inf_at]
    _same_bits(m[keep], (np.float32(1) - np.float32(B1)) * g[keep], "m of an unscaled step")
    assert m[beside] != 0


@pytest.mark.parametrize("name", C.REAL_TABLES)
def test_clip_by_norm_real_valued_gradients(name):
    """standard_normal * 0.02: sumsq within (d + 1) u of the float64 sum, d = optim_cases.sumsq_depth read from the
    kernels; the clipped gradient within 4 u plus half of that.  Measured (worst segment / element):
      FULL_CHUNKS   sumsq 2.28e-9 = 0.04 u (bound 82 u)                     clipped 7.15e-8 = 1.20 u (bound 45 u)
      MANY_CHUNKS   sumsq 1.07e-7 = 1.79 u (bound 23 u there, 26 u at most)  clipped 1.07e-7 = 1.79 u (bound 17 u at most)"""
    t = C.TABLES[name]
    g, _ = C.real_grad(7, name)
    clip = C.REAL_CLIP[name]
    got, sumsq = _clip(name, g, clip)
    ref_sumsq, _ = C.clip_ref(g, t, clip)
    bound = C.sumsq_bound(t)
    worst_sq, err = _rel_err(sumsq[:t.n_segments], ref_sumsq)
    print("clip real %s: worst sumsq error %.3e = %.2f u (bound %.1f u at that segment, largest bound %.1f u)" % (
        name, worst_sq, worst_sq / C.U, bound[err.argmax()] / C.U, bound.max() / C.U))
    assert (err <= bound).all(), (name, int((err - bound).argmax()), float((err - bound).max()))
    worst = _check_clip(name, t, g, got, sumsq, clip, C.CLIP_EXACT_BOUND + bound / 2)
    print("clip real %s: worst clipped-gradient error %.3e = %.2f u (largest bound %.1f u)" % (
        name, worst, worst / C.U, (C.CLIP_EXACT_BOUND + bound.max() / 2) / C.U))
    assert np.isnan(got[~C.covered(t)]).all()


# ================================================================================================ the fused step

def _start_state(rng, t, still):
    """Non-trivial p, m, v and moving average (host, float32) -- m = v = 0 on the `still` elements."""
    p = rng.standard_normal(t.size).astype(np.float32)
    m = (rng.standard_normal(t.size) * 0.05).astype(np.float32)
    v = (np.square(rng.standard_normal(t.size) * 0.05) + 1e-4).astype(np.float32)
    shadow = (p + 0.01 * rng.standard_normal(t.size)).astype(np.float32)
    m[still], v[still] = 0.0, 0.0
    return [p, m, v, shadow]


def _still(t):
    """Elements kept at g = m = v = 0: the first, a middle and the last covered one."""
    idx, _ = C.elements(t)
    return np.unique(idx[[0, idx.size // 2, idx.size - 1]])


def _step_grad(rng, t, still):
    g = C.exact_grad(rng, t, gap=np.nan)
    g[still] = 0.0
    C.check_exact(g, t)
    return g


def _adam_errors(got, ref, idx):
    """(worst |got - ref| / (atol + rtol |ref|), worst absolute error) over the covered elements."""
    err = np.abs(got[idx].astype(np.float64) - ref[idx])
    return float((err / (C.ADAM_ATOL + C.ADAM_RTOL * np.abs(ref[idx]))).max()), float(err.max())


@pytest.mark.parametrize("name", C.FUSED_TABLES)
def test_fused_step_against_float64(name):
    """Three consecutive steps with a falling lr and one call at step = 100000, from non-trivial m, v and moving
    average, against clip_adam_ema_ref carried in float64: p, m, v and the average within rtol 1e-5 + 4 u, atol 1e-7;
    the gradient buffer keeps its bits; sumsq[:n_segments] is bit-identical to mpsr_clip_by_norm_segments' for the same
    gradients; outside every chunk p, m, v and the average keep their bits although the gradient holds NaN there; an
    element with g = m = v = 0 keeps its p bits.
    Measured, worst over the six tables and four steps, as a fraction of the tolerance (and absolute): p 0.048
    (4.65e-7), m 0.014 (1.66e-8), v 0.012 (5.28e-9), average 0.020 (4.30e-7)."""
    t = C.TABLES[name]
    idx, _ = C.elements(t)
    gaps = ~C.covered(t)
    still = _still(t)
    rng = np.random.default_rng(C.FUSED_TABLES.index(name) + 40)
    start = _start_state(rng, t, still)
    state = [_dev(a) for a in start]
    ref = [a.astype(np.float64) for a in start]
    worst = dict.fromkeys(("p", "m", "v", "average"), (0.0, 0.0))
    for step, lr in ((1, 1e-2), (2, 5e-3), (3, 2.5e-3), (100000, 1e-3)):
        g = _step_grad(rng, t, still)
        _, clip_sumsq = _clip(name, g, C.EXACT_CLIP)
        gt = _dev(g)
        sumsq = _fused(name, state, gt, C.EXACT_CLIP, lr, step)
        *ref, ref_sumsq = C.clip_adam_ema_ref(*ref, g, t, C.EXACT_CLIP, lr, B1, B2, EPS, step, DECAY)
        _same_bits(gt, g, "step %d: the gradient buffer" % step)
        _same_bits(sumsq[:t.n_segments], clip_sumsq[:t.n_segments], "step %d: sumsq of the two entry points" % step)
        _same_bits(sumsq[:t.n_segments], ref_sumsq.astype(np.float32), "step %d: sumsq" % step)
        for key, dev, r, s0 in zip(worst, state, ref, start):
            got = dev.cpu().numpy()
            _same_bits(got[gaps], s0[gaps], "step %d: %s outside every chunk" % (step, key))
            worst[key] = tuple(max(a, b) for a, b in zip(worst[key], _adam_errors(got, r, idx)))
            np.testing.assert_allclose(got[idx], r[idx], rtol=C.ADAM_RTOL, atol=C.ADAM_ATOL,
                                       err_msg="step %d: %s" % (step, key))
        _same_bits(state[0].cpu().numpy()[still], start[0][still], "step %d: p where g = m = v = 0" % step)
    print("fused %s: worst error / tolerance (absolute): %s" % (
        name, ", ".join("%s %.4f (%.2e)" % (k, a, b) for k, (a, b) in worst.items())))
    assert float(np.abs(state[0].cpu().numpy()[idx] - start[0][idx]).max()) > 1e-3  # (the parameters really moved)


@pytest.mark.parametrize("name", ["ALIGNMENT", "MANY_CHUNKS"])
def test_fused_step_variants(name):
    """shadow == NULL leaves p, m, v as with a moving average; clip_norm = 0 with sumsq = NULL and n_segments = 0 is
    mpsr_adam_step with grad_scale 1 on the covered elements (and differs from the clipped run where a norm exceeds the
    clip); ema_decay = 0 makes the average the new p; ema_decay = 1 keeps the average's bits."""
    t = C.TABLES[name]
    idx, seg = C.elements(t)
    gaps = ~C.covered(t)
    rng = np.random.default_rng(61)
    start = _start_state(rng, t, _still(t))
    g = _step_grad(rng, t, _still(t))
    gt = _dev(g)
    step, lr = 2, 5e-3

    base = [_dev(a) for a in start]
    _fused(name, base, gt, C.EXACT_CLIP, lr, step)
    base = [a.cpu().numpy() for a in base]

    # shadow == NULL
    no_avg = [_dev(a) for a in start[:3]] + [None]
    sumsq = _fused(name, no_avg, gt, C.EXACT_CLIP, lr, step)
    assert np.isfinite(sumsq[:t.n_segments]).all()
    for key, a, b in zip("pmv", no_avg, base):
        _same_bits(a, b, "shadow NULL: " + key)

    # no clipping, no scratch
    plain = [_dev(a) for a in start]
    assert _fused(name, plain, gt, 0.0, lr, step, with_sumsq=False) is None
    plain = [a.cpu().numpy() for a in plain]
    adam = [_dev(a) for a in start[:3]]
    g0 = _dev(np.where(gaps, np.float32(0), g))  # (the whole-buffer pass reads the gaps too)
    _adam_step(adam, g0, lr, step)
    ref = C.clip_adam_ema_ref(*start, g, t, 0.0, lr, B1, B2, EPS, step, DECAY)
    for key, a, b, s0, r in zip(("p", "m", "v", "average"), plain, adam + [None], start, ref):
        _same_bits(a[gaps], s0[gaps], "no clipping: %s outside every chunk" % key)
        np.testing.assert_allclose(a[idx], r[idx], rtol=C.ADAM_RTOL, atol=C.ADAM_ATOL, err_msg="no clipping: " + key)
        if b is not None:
            np.testing.assert_allclose(a[idx], b.cpu().numpy()[idx], rtol=C.ADAM_RTOL, atol=C.ADAM_ATOL,
                                       err_msg="no clipping against mpsr_adam_step: " + key)
    # clipping really was off: the segment with the largest norm (scaled by well under 1 in the clipped run) differs in m
    ref_sumsq = C.clip_ref(g, t, C.EXACT_CLIP)[0]
    big = idx[seg == int(ref_sumsq.argmax())]
    assert np.sqrt(ref_sumsq.max()) > 2 * C.EXACT_CLIP
    moved = g[big] != 0
    assert moved.any() and (np.abs(plain[1][big][moved] - base[1][big][moved]) > 1e-4).all()

    # ema_decay = 0: the average is the new p -- exactly where p - shadow is exact (Sterbenz: shadow / 2 <= p <=
    # 2 shadow), within the Adam tolerance elsewhere (shadow + fl(p - shadow) rounds twice)
    for decay in (0.0, 1.0):
        run = [_dev(a) for a in start]
        _fused(name, run, gt, C.EXACT_CLIP, lr, step, decay=decay)
        run = [a.cpu().numpy() for a in run]
        for key, a, b in zip("pmv", run, base):
            _same_bits(a, b, "ema_decay %g: %s" % (decay, key))
        if decay == 1.0:
            _same_bits(run[3], start[3], "ema_decay 1: the average keeps its bits")
            continue
        _same_bits(run[3][gaps], start[3][gaps], "ema_decay 0: the average outside every chunk")
        p, sh0 = run[0][idx].astype(np.float64), start[3][idx].astype(np.float64)
        sterbenz = (p * sh0 > 0) & (np.abs(p) <= 2 * np.abs(sh0)) & (np.abs(sh0) <= 2 * np.abs(p))
        assert sterbenz.mean() > 0.9
        _same_bits(run[3][idx][sterbenz], run[0][idx][sterbenz], "ema_decay 0: the average is the new p")
        np.testing.assert_allclose(run[3][idx], p, rtol=C.ADAM_RTOL, atol=C.ADAM_ATOL)


# ================================================================================================ non-finite gradients

def test_nonfinite_gradients_stay_in_their_segment():
    """One NaN element in one segment, one +inf element in another (MANY_CHUNKS: segments of 65 and 128 chunks).
    mpsr_clip_by_norm_segments: the NaN segment's norm is NaN and the segment keeps its bits; the inf segment's norm is
    inf, its finite elements become +-0 (sign kept) and the inf element NaN -- g * clip / max(norm, clip); every other
    segment is as without them.  The fused step: the NaN segment is updated with scale 1 and only the NaN element's own
    p, m, v (and average) become NaN; the inf segment's finite elements are updated with a zero gradient."""
    name, t = "MANY_CHUNKS", C.MANY_CHUNKS
    idx, seg = C.elements(t)
    nan_seg, inf_seg = C.MANY_COUNTS.index(65), C.MANY_COUNTS.index(128)
    g = C.exact_case(name)[0].copy()
    g[~C.covered(t)] = np.nan
    nan_at, inf_at = idx[seg == nan_seg][150], idx[seg == inf_seg][301]
    g[nan_at], g[inf_at] = np.nan, np.inf
    ref_sumsq, ref = C.clip_ref(g, t, C.EXACT_CLIP)

    got, sumsq = _clip(name, g, C.EXACT_CLIP)
    assert np.isnan(sumsq[nan_seg]) and sumsq[inf_seg] == np.inf
    others = np.setdiff1d(np.arange(t.n_segments), [nan_seg, inf_seg])
    _same_bits(sumsq[others], ref_sumsq[others].astype(np.float32), "sumsq of the finite segments")
    _same_bits(got[idx[seg == nan_seg]], g[idx[seg == nan_seg]], "the NaN segment keeps its bits")
    finite = idx[(seg == inf_seg) & (idx != inf_at)]
    assert (g[finite] < 0).any() and (g[finite] > 0).any()
    _same_bits(got[finite], ref[finite].astype(np.float32), "the inf segment's finite elements become +-0")
    assert (got[finite] == 0).all() and np.isnan(got[inf_at])
    rest = idx[np.isin(seg, others)]
    worst, _ = _rel_err(got[rest], ref[rest])
    assert worst <= C.CLIP_EXACT_BOUND
    _same_bits(got[~C.covered(t)], g[~C.covered(t)], "outside every chunk")

    rng = np.random.default_rng(71)
    start = _start_state(rng, t, _still(t))
    state = [_dev(a) for a in start]
    f_sumsq = _fused(name, state, _dev(g), C.EXACT_CLIP, LR, 1)
    _same_bits(f_sumsq[:t.n_segments], sumsq[:t.n_segments], "sumsq of the two entry points")
    want = C.clip_adam_ema_ref(*start, g, t, C.EXACT_CLIP, LR, B1, B2, EPS, 1, DECAY)
    # (scale 1 in the NaN segment: its norm without the NaN element is far over the clip, a scaled m would be far off)
    assert np.sqrt(np.nansum(np.square(g[idx[seg == nan_seg]].astype(np.float64)))) > 2 * C.EXACT_CLIP
    for key, dev, r, s0 in zip(("p", "m", "v", "average"), state, want, start):
        a = dev.cpu().numpy()
        nans = np.nonzero(np.isnan(a))[0]
        assert sorted(nans.tolist()) == sorted([int(nan_at), int(inf_at)]), (key, nans)
        np.testing.assert_allclose(a[idx], r[idx], rtol=C.ADAM_RTOL, atol=C.ADAM_ATOL, equal_nan=True, err_msg=key)
        _same_bits(a[~C.covered(t)], s0[~C.covered(t)], key + " outside every chunk")


# ================================================================================================ a wrong-scale detector

def _detector_cases():
    first = int(np.nonzero(C.MANY_CHUNKS.chunk_seg == C.MANY_SEG_129)[0][0])
    cases = [("MANY_CHUNKS", first + k, "129 chunks, chunk %d" % (k + 1)) for k in (128, 64, 0)]
    for mod in (0, 1, 3):  # the float4 branch's tail loop; the scalar branch
        cases.append(("ALIGNMENT", C.alignment_segment(mod, 1027), "1027 floats, begin %% 4 == %d" % mod))
    return cases


@pytest.mark.parametrize("name,chunk,what", _detector_cases(), ids=[c[2] for c in _detector_cases()])
def test_one_dropped_chunk_or_tail_element_flips_the_clip_decision(name, chunk, what):
    """The LAST element of one chunk alone carries the segment over the threshold: the segment's other elements have a
    norm under clip / 1.5, with that element it is over 3 clip.  A kernel that loses the chunk (the 129th, the 65th or
    the first of 129: the tail, a middle trip and the start of seg_sum_kernel's loop) or the element (the last of 1027:
    seg_sumsq_kernel's tail loop, and the end of its scalar loop) leaves the whole segment unscaled -- a factor of three
    in every element, more in sumsq, and a factor of three in the fused step's m, not an ulp."""
    t = C.TABLES[name]
    idx, seg = C.elements(t)
    s = int(t.chunk_seg[chunk])
    at = int(t.chunk_begin[chunk] + t.chunk_len[chunk] - 1)
    clip, planted = 5.0, 16.0  # (16 = 2^10 * 2^-6: its square adds 2^20 to the integer sum, far below 2^24)
    g = C.exact_case(name)[0].copy()
    g[at] = 0.0
    assert np.sqrt(C.clip_ref(g, t, clip)[0][s]) < clip / 1.5
    g[at] = planted
    C.check_exact(g, t)
    ref_sumsq, ref = C.clip_ref(g, t, clip)
    assert np.sqrt(ref_sumsq[s]) > 1.5 * clip and (np.sqrt(np.delete(ref_sumsq, s)) < clip).all()
    got, sumsq = _clip(name, g, clip)
    _same_bits(sumsq[:t.n_segments], ref_sumsq.astype(np.float32), what + ": sumsq")
    _check_clip(name, t, g, got, sumsq, clip, np.full(t.n_segments, C.CLIP_EXACT_BOUND))
    mine = idx[seg == s]
    assert np.sqrt(ref_sumsq[s]) > 3 * clip
    assert (np.abs(got[mine]) <= 0.34 * np.abs(g[mine])).all(), "the segment must be scaled by less than a third"
    # the fused step from m = v = 0: m = (1 - b1) * scale * g
    state = [_dev(np.zeros(t.size, np.float32)) for _ in range(4)]
    f_sumsq = _fused(name, state, _dev(g), clip, LR, 1)
    _same_bits(f_sumsq[:t.n_segments], sumsq[:t.n_segments], what + ": fused sumsq")
    want = C.clip_adam_ema_ref(*[np.zeros(t.size)] * 4, g, t, clip, LR, B1, B2, EPS, 1, DECAY)
    m = state[1].cpu().numpy()
    np.testing.assert_allclose(m[idx], want[1][idx], rtol=C.ADAM_RTOL, atol=0, err_msg=what)
    assert (np.abs(m[mine]) <= 0.34 * 0.1 * np.abs(g[mine])).all()

"""The elementwise kernels of the backward pass, called directly through the C ABI at their edges: mpsr_act_bias_grad,
mpsr_bias_grad, mpsr_relu_grad, mpsr_relu_bitmask, mpsr_max_pool_grad, mpsr_resize_bilinear_grad,
mpsr_crop_and_resize_grad and mpsr_adam_step_lr_dev (csrc/backward.hip, csrc/crop_grad.hip).

These kernels pass gradients through or sum them.  With small-integer gradients every fp32 partial sum is an exactly
representable integer in any order, atomics included, so the results are compared with the float64 restatements of
tests/backward_elementwise_cases.py EXACTLY -- an off-by-one row, a dropped tail or a wrong tie rule cannot hide in a
tolerance.  The case lists, and which launcher branch each case reaches, are in that module."""
import numpy as np
import pytest
import torch

import backward_elementwise_cases as C

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
GUARD = 64  # floats on either side of an output (256 bytes: the view between them stays 16-byte aligned)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _place(a, offset):
    """The array on the device; offset: inside a larger allocation, one float past its (aligned) start."""
    t = _dev(a)
    if not offset:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty((t.numel() + 8,), dtype=t.dtype, device="cuda")
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


class _Guarded:
    """An output tensor of `shape` between two runs of sentinel values, itself pre-filled with `fill`."""

    def __init__(self, shape, offset=False, fill=float("nan"), dtype=torch.float32):
        n = int(np.prod(shape))
        self.lo = GUARD + (1 if offset else 0)
        self.buf = torch.full((self.lo + n + GUARD,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype,
                              device="cuda")
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (4 if offset else 0)
        self.n = n

    def ptr(self):
        return self.t.data_ptr()

    def check_guards(self, name):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == SENTINEL).all() and (b[self.lo + self.n:] == SENTINEL).all(), name + ": wrote outside its output"


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same_bits(got, ref64, name):
    """got (float32, device) against a float64 reference that float32 holds exactly: bit for bit."""
    want = ref64.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), ref64), name + ": reference not representable"
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at flat index %d (got %r, want %r)" % (
        name, bad.size, g.size, bad[0], g[bad[0]:bad[0] + 1].view(np.float32)[0], w[bad[0]:bad[0] + 1].view(np.float32)[0])


def _assert_same_values(got, ref64, name):
    """Exact equality of values (sums: +0 and -0 are the same sum)."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    bad = np.nonzero(~(got.reshape(-1) == ref64.reshape(-1)))[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at flat index %d (got %r, want %r)" % (
        name, bad.size, got.size, bad[0], got.reshape(-1)[bad[0]], ref64.reshape(-1)[bad[0]])


def _nonzero_ints(rng, n):
    return (rng.integers(1, 9, n) * rng.choice([-1, 1], n)).astype(np.float32)


# ================================================================================================ act_bias_grad

def _act_takes_fast(N, *ptrs):
    """The launcher's predicate, restated."""
    return N % 4 == 0 and N <= 1024 and 256 % (N // 4) == 0 and all(p is None or p % 16 == 0 for p in ptrs)


def _act_forms(dy, y, g, offset=()):
    """All call forms of mpsr_act_bias_grad on one problem; `offset` names the operands placed one float off 16-byte
    alignment.  Returns the bits of dx of the full form."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    M, N = dy.shape
    rng = np.random.default_rng(M + N)
    dyt, yt = _place(dy, "dy" in offset), _place(y, "y" in offset)
    colsum_g, colsum_dy = C.bias_grad_ref(g), C.bias_grad_ref(dy)
    tag = "M=%d N=%d offset=%s" % (M, N, sorted(offset))

    def inputs_untouched(form):
        assert np.array_equal(_bits(dyt), _bits(dy)) and np.array_equal(_bits(yt), _bits(y)), "%s %s: inputs changed" % (tag, form)

    # full: dx = g bit for bit, db accumulated INTO
    db0 = _nonzero_ints(rng, N)
    dbt, dx = _Guarded((N,), fill=0.0), _Guarded((M, N), "dx" in offset)
    dbt.t.copy_(_dev(db0))
    _lib.check(lib.mpsr_act_bias_grad(dyt.data_ptr(), yt.data_ptr(), dx.ptr(), dbt.ptr(), M, N, _lib.stream()))
    _assert_same_bits(dx.t, g, tag + " full: dx")
    _assert_same_values(dbt.t, db0.astype(np.float64) + colsum_g, tag + " full: db")
    dx.check_guards(tag + " full: dx")
    dbt.check_guards(tag + " full: db")
    inputs_untouched("full")
    full_bits = _bits(dx.t).copy()
    flat = dx.t.reshape(-1).cpu().numpy()
    for p, name, _, keep, _ in C.planted(M * N):
        assert flat[p] == 5.0 * keep, "%s: y = %s at %d" % (tag, name, p)

    # db == NULL: the same dx and nothing else
    dx2 = _Guarded((M, N), "dx" in offset)
    _lib.check(lib.mpsr_act_bias_grad(dyt.data_ptr(), yt.data_ptr(), dx2.ptr(), None, M, N, _lib.stream()))
    _assert_same_bits(dx2.t, g, tag + " no db: dx")
    dx2.check_guards(tag + " no db: dx")
    inputs_untouched("no db")

    # y == dx == NULL: column sums of dy itself
    db1 = _nonzero_ints(rng, N)
    dbt.t.copy_(_dev(db1))
    _lib.check(lib.mpsr_act_bias_grad(dyt.data_ptr(), None, None, dbt.ptr(), M, N, _lib.stream()))
    _assert_same_values(dbt.t, db1.astype(np.float64) + colsum_dy, tag + " sums only: db")
    dbt.check_guards(tag + " sums only: db")
    inputs_untouched("sums only")

    # y without dx: the fast kernel sums the masked gradient without storing it; the generic path has nowhere to keep it
    # and says so (which is also how a test sees WHICH path a call took)
    db2 = _nonzero_ints(rng, N)
    dbt.t.copy_(_dev(db2))
    rc = lib.mpsr_act_bias_grad(dyt.data_ptr(), yt.data_ptr(), None, dbt.ptr(), M, N, _lib.stream())
    if _act_takes_fast(N, dyt.data_ptr(), yt.data_ptr(), None):
        _lib.check(rc)
        _assert_same_values(dbt.t, db2.astype(np.float64) + colsum_g, tag + " y without dx: db")
    else:
        assert rc != 0 and b"dx required on the generic path" in lib.mpsr_last_error(), tag
        _assert_same_values(dbt.t, db2.astype(np.float64), tag + " refused call: db")
    dbt.check_guards(tag + " y without dx: db")
    inputs_untouched("y without dx")
    return full_bits


def _act_problem(M, N):
    rng = np.random.default_rng(100003 * N + M)
    dy = C.int_grad(rng, (M, N))
    y = C.activations(rng, (M, N), dy)
    return dy, y, C.relu_grad_ref(dy, y)


@pytest.mark.parametrize("M", C.ACT_M)
@pytest.mark.parametrize("N", C.ACT_FAST_N + C.ACT_GENERIC_N)
def test_act_bias_grad_every_form_is_exact(N, M):
    """Fast-path N and generic N at M on both sides of every row slice; the call forms full, db == NULL, y == dx == NULL
    and y without dx (an error on the generic path)."""
    dy, y, g = _act_problem(M, N)
    assert _act_takes_fast(N, 0, 0, 0) == (N in C.ACT_FAST_N)
    _act_forms(dy, y, g)


@pytest.mark.parametrize("M", C.ACT_M)
@pytest.mark.parametrize("N", C.ACT_FAST_N)
def test_act_bias_grad_misaligned_views_take_the_generic_path_with_the_same_bits(N, M):
    """The fast-path widths through views offset by one float: the alignment test sends them to relu_grad_kernel +
    bias_grad_kernel (seen by the documented refusal of `y without dx`), and dx is bit-identical to the fast path's."""
    dy, y, g = _act_problem(M, N)
    aligned = _act_forms(dy, y, g)
    shifted = _act_forms(dy, y, g, offset=("dy", "y", "dx"))
    assert np.array_equal(aligned, shifted)


@pytest.mark.parametrize("which", ["dy", "y", "dx"])
def test_act_bias_grad_one_misaligned_operand_is_enough(which):
    dy, y, g = _act_problem(257, 64)
    assert np.array_equal(_act_forms(dy, y, g), _act_forms(dy, y, g, offset=(which,)))


def test_act_bias_grad_real_valued_sums_within_the_fp32_summation_bound():
    """standard_normal dy at (4097, 256): dx is still a pass-through (bit for bit); db is held to the worst-case bound of
    fp32 summation in ANY order, |db - ref| <= (M + 2) 2^-24 sum_m |g[m][n]| per column (derived, not measured: M - 1
    additions of relative error 2^-24 each to first order, one more for the atomic that meets db, and the rounding of
    the result)."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    M, N = C.ACT_REAL_CASE
    rng = np.random.default_rng(11)
    dy = rng.standard_normal((M, N)).astype(np.float32)
    y = C.activations(rng, (M, N), dy)
    g = C.relu_grad_ref(dy, y)
    dx, db = _Guarded((M, N)), torch.zeros((N,), device="cuda")
    dyt, yt = _dev(dy), _dev(y)
    _lib.check(lib.mpsr_act_bias_grad(dyt.data_ptr(), yt.data_ptr(), dx.ptr(), db.data_ptr(), M, N, _lib.stream()))
    _assert_same_bits(dx.t, g, "dx")
    dx.check_guards("dx")
    err = np.abs(db.cpu().numpy().astype(np.float64) - g.sum(0))
    bound = (M + 2) * 2.0 ** -24 * np.abs(g).sum(0)
    print("act_bias_grad real-valued: max err / bound = %.3e" % float((err / bound).max()))
    assert (err <= bound).all()


# ================================================================================================ bias_grad, relu_grad

def _bias_grad_case(M, N):
    from monopsr_amd import _lib
    rng = np.random.default_rng(7919 * N + M)
    dy = C.int_grad(rng, (M, N), wide=M < 100000)
    db0 = _nonzero_ints(rng, N)
    db = _Guarded((N,), fill=0.0)
    db.t.copy_(_dev(db0))
    dyt = _dev(dy)
    _lib.check(_lib.lib().mpsr_bias_grad(dyt.data_ptr(), M, N, db.ptr(), _lib.stream()))
    _assert_same_values(db.t, db0.astype(np.float64) + C.bias_grad_ref(dy), "bias_grad M=%d N=%d" % (M, N))
    db.check_guards("db")
    assert np.array_equal(_bits(dyt), _bits(dy))


@pytest.mark.parametrize("M", C.BIAS_M)
@pytest.mark.parametrize("N", C.BIAS_N)
def test_bias_grad_is_exact_and_accumulates(N, M):
    _bias_grad_case(M, N)


@pytest.mark.parametrize("N", C.BIAS_LONG_N)
def test_bias_grad_past_the_slice_cap(N):
    """M = 2048 * 512 + 513: 2048 slices of 513 rows, of which the grid needs 2046."""
    _bias_grad_case(C.BIAS_LONG_M, N)


@pytest.mark.parametrize("total", C.RELU_TOTALS)
def test_relu_grad_is_exact(total):
    from monopsr_amd import _lib
    rng = np.random.default_rng(total)
    dy = C.int_grad(rng, (total,))
    y = C.activations(rng, (total,), dy)
    dx = _Guarded((total,))
    dyt, yt = _dev(dy), _dev(y)
    _lib.check(_lib.lib().mpsr_relu_grad(dyt.data_ptr(), yt.data_ptr(), dx.ptr(), total, _lib.stream()))
    _assert_same_bits(dx.t, C.relu_grad_ref(dy, y), "relu_grad total=%d" % total)
    dx.check_guards("dx")
    flat = dx.t.cpu().numpy()
    for p, name, _, keep, _ in C.planted(total):
        assert flat[p] == 5.0 * keep, (name, p)


def test_relu_grad_and_act_bias_grad_on_the_large_case():
    """N = 4, M = 2^24 + 4097 (270 MB per tensor, built on the device): relu_grad's grid-stride loop takes its second
    trip, act_bias_grad runs at its 4096-block cap with a ragged last block.  The reference is torch.where and a float64
    torch.sum on the device -- an independent implementation; dy is drawn from {-1, 0, 1} so that the sums stay exact."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    M, N = C.LARGE_M, C.LARGE_N
    total = M * N
    gen = torch.Generator(device="cuda").manual_seed(2024)
    dy = y = dx = want = None
    try:
        dy = torch.randint(-1, 2, (M, N), device="cuda", generator=gen, dtype=torch.float32)
        y = torch.randn((M, N), device="cuda", generator=gen)
        # planted values: the usual four, and +inf / 0.0 on the first two elements of the loop's second trip
        flat_y, flat_dy = y.view(-1), dy.view(-1)
        second_trip = 262144 * 256
        assert second_trip + 1 < total
        planted = [(p, value, keep) for p, _, value, keep, _ in C.planted(total)]
        planted += [(second_trip, np.float32(np.inf), 1), (second_trip + 1, np.float32(0.0), 0)]
        for p, value, _ in planted:
            flat_y[p] = float(value)
            flat_dy[p] = 1.0
        assert float(dy.abs().sum(0, dtype=torch.float64).max()) < C.EXACT_LIMIT
        want = torch.where(y > 0, dy, torch.zeros_like(dy))
        want_db = want.sum(0, dtype=torch.float64)
        assert 0.2 < float((want != 0).float().mean()) < 0.5

        dx = torch.full_like(dy, 7.0)
        _lib.check(lib.mpsr_relu_grad(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), total, _lib.stream()))
        assert torch.equal(dx.view(torch.int32), want.view(torch.int32)), "relu_grad"
        for p, _, keep in planted:
            assert float(dx.view(-1)[p]) == float(keep)

        dx.fill_(7.0)
        db0 = torch.tensor([3.0, -5.0, 7.0, -2.0], device="cuda")
        db = db0.clone()
        _lib.check(lib.mpsr_act_bias_grad(dy.data_ptr(), y.data_ptr(), dx.data_ptr(), db.data_ptr(), M, N, _lib.stream()))
        assert torch.equal(dx.view(torch.int32), want.view(torch.int32)), "act_bias_grad dx"
        assert torch.equal(db.double(), db0.double() + want_db), (db, want_db)

        db = db0.clone()
        _lib.check(lib.mpsr_act_bias_grad(dy.data_ptr(), None, None, db.data_ptr(), M, N, _lib.stream()))
        assert torch.equal(db.double(), db0.double() + dy.sum(0, dtype=torch.float64))
    finally:
        del dy, y, dx, want
        torch.cuda.empty_cache()


# ================================================================================================ relu_bitmask

@pytest.mark.parametrize("M,N", [(M, N) for N in C.BITMASK_N for M in C.BITMASK_M] + C.BITMASK_EXTRA)
def test_relu_bitmask_words_follow_the_documented_layout(M, N):
    """Every word against the NumPy restatement of the layout the pointwise kernel's epilogue shares:
    bit b <-> row 32 (m >> 5) + mask_row(b); rows past M read as zero although `bits` came in as all ones."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(50 * M + N)
    dy = np.zeros((M, N), np.float32)
    y = C.activations(rng, (M, N), dy)
    words = int(lib.mpsr_relu_bitmask_words(M, N))
    assert words == (M + 31) // 32 * N
    bits = _Guarded((words,), fill=-1, dtype=torch.int32)
    yt = _dev(y)
    _lib.check(lib.mpsr_relu_bitmask(yt.data_ptr(), M, N, bits.ptr(), _lib.stream()))
    got = bits.t.cpu().numpy().view(np.uint32)
    want = C.relu_bitmask_ref(y, M, N)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "M=%d N=%d: %d of %d words differ, first %d: got %08x want %08x" % (
        M, N, bad.size, words, bad[0], got[bad[0]], want[bad[0]])
    bits.check_guards("bits")
    row_of = [C.mask_row(b) for b in range(32)]
    last = got.reshape(-1, N)[-1]
    for b in range(32):  # rows past M
        if (M - 1) // 32 * 32 + row_of[b] >= M:
            assert not ((last >> np.uint32(b)) & np.uint32(1)).any(), b
    for p, name, _, _, bit in C.planted(M * N):
        m, n = divmod(p, N)
        assert (int(got[(m >> 5) * N + n]) >> row_of.index(m & 31)) & 1 == bit, (name, p)
    assert np.array_equal(_bits(yt), _bits(y))


# ================================================================================================ max_pool_grad

@pytest.mark.parametrize("shape,k,s,pad", C.MAX_POOL_CASES, ids=["%s-k%ds%d%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3])
                                                                 for c in C.MAX_POOL_CASES])
def test_max_pool_grad_routes_ties_to_the_first_maximum(shape, k, s, pad):
    """Post-ReLU-like inputs (two thirds exact zeros): most windows tie, and the gradient must go to the first maximum in
    row-major window order, padded cells skipped -- exactly, with integer gradients."""
    from monopsr_amd import _lib
    rng = np.random.default_rng(sum(shape) + k)
    x = C.pool_input(rng, shape)
    dy = C.int_grad(rng, C.max_pool_out_shape(shape, k, s, pad))
    dy[dy == 0] = 3.0  # every output cell's route is visible
    want = C.max_pool_grad_ref(x, dy, k, s, pad)
    dx = _Guarded(shape)
    B, H, W, Cc = shape
    xt, dyt = _dev(x), _dev(dy)
    _lib.check(_lib.lib().mpsr_max_pool_grad(xt.data_ptr(), dyt.data_ptr(), B, H, W, Cc, k, s, int(pad == "SAME"), dx.ptr(),
                                             _lib.stream()))
    _assert_same_values(dx.t, want, "max_pool_grad %s" % (shape,))
    dx.check_guards("dx")


# ================================================================================================ resize_bilinear_grad

def _resize_grad(dy, h, w, ac, offset):
    from monopsr_amd import _lib
    B, OH, OW, Cc = dy.shape
    dyt = _place(dy, offset)
    dx = _Guarded((B, h, w, Cc), offset)
    _lib.check(_lib.lib().mpsr_resize_bilinear_grad(dyt.data_ptr(), B, h, w, Cc, OH, OW, int(ac), dx.ptr(), _lib.stream()))
    dx.check_guards("resize dx")
    assert np.array_equal(_bits(dyt), _bits(dy))
    return dx.t


@pytest.mark.parametrize("variant", C.RESIZE_VARIANTS)
@pytest.mark.parametrize("case", C.RESIZE_EXACT_CASES, ids=["%dx%d-%dx%d" % (c[0] + c[1]) for c in C.RESIZE_EXACT_CASES])
def test_resize_bilinear_grad_is_exact_at_dyadic_scales(case, variant):
    """Both values of align_corners, up- and downsampling, the gather / scatter switch at its boundary (scale 0.25), and
    the two ways to the scatter form other than the scale: C % 4 != 0 and a misaligned view.  dx comes in as NaN and is
    fully overwritten (inputs that no output reads get 0)."""
    (h, w), (OH, OW), ac, _ = case
    Cc = 3 if variant == "c3" else 4
    dy = C.int_grad(np.random.default_rng(OH * 100 + OW + Cc), (C.RESIZE_B, OH, OW, Cc))
    want = C.resize_grad_ref(dy, h, w, ac)
    got = _resize_grad(dy, h, w, ac, variant == "c4_offset")
    _assert_same_values(got, want, "resize_bilinear_grad %s %s (%s form)" % (case[:3], variant, C.resize_form(case, variant)))


@pytest.mark.parametrize("Cc", [4, 3])
@pytest.mark.parametrize("case", C.RESIZE_TOL_CASES, ids=["%dx%d-%dx%d" % (c[0] + c[1]) for c in C.RESIZE_TOL_CASES])
def test_resize_bilinear_grad_at_other_scales(case, Cc):
    """Non-dyadic scales, real-valued dy: 1e-5 of the gradient's scale, as test_resize_bilinear_gradient."""
    (h, w), (OH, OW), ac = case
    dy = np.random.default_rng(h + OW + Cc).standard_normal((C.RESIZE_B, OH, OW, Cc)).astype(np.float32)
    want = C.resize_grad_ref(dy, h, w, ac)
    got = _resize_grad(dy, h, w, ac, False).cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("resize_bilinear_grad %s C=%d: max err / scale = %.3e" % (case, Cc, err))
    assert err <= 1e-5


# ================================================================================================ crop_and_resize_grad

def _crop_grad(dy, boxes, ind, Cc):
    from monopsr_amd import _lib
    nimg, H, W = C.CROP_IMAGE
    nb, ch, cw, _ = dy.shape
    dimg = _Guarded((nimg, H, W, Cc))  # NaN: whatever is not overwritten shows
    indt = _dev(ind) if ind is not None else None
    dyt, boxt = _dev(dy), _dev(boxes)
    _lib.check(_lib.lib().mpsr_crop_and_resize_grad(dyt.data_ptr(), nimg, H, W, Cc, boxt.data_ptr(),
                                                    indt.data_ptr() if indt is not None else None, nb, ch, cw, dimg.ptr(),
                                                    _lib.stream()))
    dimg.check_guards("grad_image")
    return dimg.t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("mode", C.CROP_IND_MODES)
@pytest.mark.parametrize("size", C.CROP_SIZES, ids=["%dx%d" % s for s in C.CROP_SIZES])
@pytest.mark.parametrize("Cc", C.CROP_C)
def test_crop_and_resize_grad_on_the_forward_tests_boxes(Cc, size, mode):
    """Inside, whole-image, partly outside, zero-area, flipped, narrow and fully-outside boxes against float64 autograd
    through oracle.net.tf_crop_and_resize; box_ind given, NULL, and with one index out of range (that box contributes
    nothing -- the reference is the problem without it)."""
    nimg, H, W = C.CROP_IMAGE
    nb = len(C.CROP_BOXES)
    dy = np.random.default_rng(Cc * 100 + size[0] * 10 + size[1]).standard_normal((nb, size[0], size[1], Cc)).astype(np.float32)
    with_all = C.crop_grad_ref(dy, nimg, H, W, C.CROP_BOXES, C.CROP_IND)
    if mode == "given":
        ind, want = C.CROP_IND, with_all
    elif mode == "null":
        ind, want = None, C.crop_grad_ref(dy, nimg, H, W, C.CROP_BOXES, np.zeros(nb, np.int32))
        assert not want[1].any() and want[0].any()
    else:
        ind = C.CROP_IND.copy()
        ind[C.CROP_BAD_BOX] = nimg if mode == "past_end" else -1
        keep = [i for i in range(nb) if i != C.CROP_BAD_BOX]
        want = C.crop_grad_ref(dy[keep], nimg, H, W, C.CROP_BOXES[keep], C.CROP_IND[keep])
        assert np.abs(want - with_all).max() > 1e-3  # the box that is dropped would have been seen
    got = _crop_grad(dy, C.CROP_BOXES, ind, Cc)
    assert np.isfinite(got).all(), "grad_image not fully overwritten"
    err = np.abs(got - want).max()
    print("crop_and_resize_grad C=%d %s %s: max err %.3e (scale %.3e)" % (Cc, size, mode, err, np.abs(want).max()))
    assert err <= 1e-5 * max(1.0, np.abs(want).max())
    # the fully-outside box alone: the image gradient is overwritten with exact zeros
    one = [C.CROP_OUTSIDE]
    alone = _crop_grad(dy[one], C.CROP_BOXES[one], None if ind is None else np.zeros(1, np.int32), Cc)
    assert not C.crop_grad_ref(dy[one], nimg, H, W, C.CROP_BOXES[one], np.zeros(1, np.int32)).any()
    assert (alone == 0).all()


# ================================================================================================ adam_step_lr_dev

@pytest.mark.parametrize("grad_scale", C.ADAM_GRAD_SCALES)
@pytest.mark.parametrize("n", C.ADAM_N)
def test_adam_step_lr_dev_is_adam_step_with_the_rate_in_memory(n, grad_scale):
    """Three steps: with the device scalar set to float32(lr sqrt(1 - b2^t) / (1 - b1^t)) (float64 arithmetic on the
    float32 hyper-parameters, as the host side of mpsr_adam_step) p, m and v are bit-identical to mpsr_adam_step's, both
    match the TensorFlow formula in float64, and an element whose g, m and v are zero keeps its bits."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    rng = np.random.default_rng(n)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    p0 = rng.standard_normal(n).astype(np.float32)
    still = n // 2 if n > 1 else None
    host = [torch.from_numpy(p0).cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    dev = [t.clone() for t in host]
    ref = [p0.astype(np.float64), np.zeros(n), np.zeros(n)]
    lr_t = torch.zeros((1,), device="cuda")
    for step in range(1, C.ADAM_STEPS + 1):
        g = rng.standard_normal(n).astype(np.float32)
        if still is not None:
            g[still] = 0.0
        gt = _dev(g)
        _lib.check(lib.mpsr_adam_step(host[0].data_ptr(), gt.data_ptr(), host[1].data_ptr(), host[2].data_ptr(), n, lr, b1, b2,
                                      eps, step, grad_scale, _lib.stream()))
        lr_t.fill_(float(np.float32(C.adam_lr_t(lr, b1, b2, step))))
        _lib.check(lib.mpsr_adam_step_lr_dev(dev[0].data_ptr(), gt.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n,
                                             lr_t.data_ptr(), b1, b2, eps, grad_scale, _lib.stream()))
        ref = list(C.adam_ref(ref[0], ref[1], ref[2], g, lr, b1, b2, eps, step, grad_scale))
        for name, a, b, r in zip("pmv", host, dev, ref):
            assert np.array_equal(_bits(a), _bits(b)), "step %d: %s differs between the two entry points" % (step, name)
            np.testing.assert_allclose(b.cpu().numpy(), r, rtol=1e-5, atol=1e-7, err_msg="step %d: %s" % (step, name))
        assert np.array_equal(_bits(gt), _bits(g))
    assert float((dev[0] - torch.from_numpy(p0).cuda()).abs().max()) > 1e-3
    if still is not None:
        assert _bits(dev[0])[still] == _bits(p0)[still] and float(dev[1][still]) == 0.0 and float(dev[2][still]) == 0.0

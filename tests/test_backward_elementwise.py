"""Host-side half of the elementwise backward tests (tests/backward_elementwise_cases.py; the GPU half is
tests/test_backward_elementwise_gpu.py): the float64 restatements the kernels are held to are themselves checked here,
against float64 autograd through the oracle where there is one, and the conditions that make the GPU comparisons exact
are asserted on the references."""
import numpy as np
import pytest

import backward_elementwise_cases as C


@pytest.mark.parametrize("shape,k,s,pad", C.MAX_POOL_CASES, ids=["%s-k%ds%d%s" % ("x".join(map(str, c[0])), c[1], c[2], c[3])
                                                                 for c in C.MAX_POOL_CASES])
def test_max_pool_restatement_equals_autograd_on_tied_inputs(shape, k, s, pad):
    """"First maximum in row-major window order" written as loops == float64 autograd through oracle.net.tf_max_pool,
    on post-ReLU-like inputs in which most windows tie."""
    rng = np.random.default_rng(sum(shape) + k)
    x = C.pool_input(rng, shape)
    assert 0.55 < float((x == 0).mean()) < 0.8
    dy = C.int_grad(rng, C.max_pool_out_shape(shape, k, s, pad))
    got = C.max_pool_grad_ref(x, dy, k, s, pad)
    want = C.max_pool_grad_autograd(x, dy, k, s, pad)
    assert np.array_equal(got, want)
    assert got.sum() == dy.astype(np.float64).sum()  # every output cell routed its gradient exactly once
    # ... and the inputs really tie: routing to the LAST maximum instead gives another answer
    flipped = C.max_pool_grad_ref(x[:, ::-1, ::-1], dy[:, ::-1, ::-1], k, s, pad)[:, ::-1, ::-1] \
        if _symmetric_windows(shape, k, s, pad) else None
    if flipped is not None:
        assert not np.array_equal(flipped, got)


def _symmetric_windows(shape, k, s, pad):
    """True where mirroring the image maps the set of pooling windows onto itself (then "first maximum" of the mirrored
    problem is "last maximum" of the original)."""
    for size in shape[1:3]:
        if pad == "SAME":
            out, before = C.same_padding(size, k, s)
            after = max((out - 1) * s + k - size, 0) - before
        else:
            out, before = (size - k) // s + 1, 0
            after = (out - 1) * s + k - size
        if before != after:
            return False
    return True


def test_mirror_check_runs_somewhere():
    assert sum(_symmetric_windows(*c) for c in C.MAX_POOL_CASES) >= 3


@pytest.mark.parametrize("case", C.RESIZE_EXACT_CASES, ids=["%dx%d-%dx%d" % (c[0] + c[1]) for c in C.RESIZE_EXACT_CASES])
def test_dyadic_resize_gradients_are_exact_in_float32(case):
    """With integer dy the reference gradient at every dyadic case is an integer after multiplying by 256 and survives
    the round trip through float32 -- so the GPU test may ask for equality -- and the predicate of the launcher gives the
    form the case list names."""
    (h, w), (OH, OW), ac, form = case
    for C_ in (3, 4):
        dy = C.int_grad(np.random.default_rng(OH * 100 + OW + C_), (C.RESIZE_B, OH, OW, C_))
        ref = C.resize_grad_ref(dy, h, w, ac)
        assert ref.shape == (C.RESIZE_B, h, w, C_)
        assert np.array_equal(ref * 256, np.round(ref * 256))
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
        assert np.abs(ref).max() * 256 < C.EXACT_LIMIT
        assert ref.sum() == dy.astype(np.float64).sum()  # the weights of an output sum to one
    scales = [np.float32(i - 1) / np.float32(o - 1) if ac and o > 1 else np.float32(i) / np.float32(o)
              for i, o in ((h, OH), (w, OW))]
    few = all(np.float32(2.0) / sc + np.float32(4.0) <= np.float32(12.0) for sc in scales)
    assert ("gather" if few else "scatter") == form
    if (h, w) in ((9, 9), (8, 8)):  # downsampling: inputs off the sample grid receive nothing
        assert (ref == 0).mean() > 0.5


def test_bitmask_restatement_is_a_permutation_of_rows():
    """mask_row is a bijection on 0..31, so the words hold exactly the (y > 0) bits of the rows that exist."""
    assert sorted(C.mask_row(b) for b in range(32)) == list(range(32))
    rng = np.random.default_rng(3)
    for M, N in ((1, 4), (33, 8), (69, 12)):
        dy = np.zeros((M, N), np.float32)
        y = C.activations(rng, (M, N), dy)
        words = C.relu_bitmask_ref(y, M, N)
        assert words.shape == ((M + 31) // 32 * N,) and words.dtype == np.uint32
        assert sum(bin(int(wd)).count("1") for wd in words) == int((y > 0).sum())
        for m in range(M):
            b = [C.mask_row(i) for i in range(32)].index(m & 31)
            assert np.array_equal((words.reshape(-1, N)[m >> 5] >> np.uint32(b)) & np.uint32(1), (y[m] > 0).astype(np.uint32))


def test_planted_values_and_their_expected_effect():
    rng = np.random.default_rng(4)
    dy = C.int_grad(rng, (31, 12))
    y = C.activations(rng, (31, 12), dy)
    g = C.relu_grad_ref(dy, y)
    assert len(C.planted(y.size)) == 12
    for p, name, value, keep, bit in C.planted(y.size):
        got = y.reshape(-1)[p]
        assert (np.isnan(got) and np.isnan(value)) or (got == value and np.signbit(got) == np.signbit(value)), name
        assert dy.reshape(-1)[p] == 5.0 and g.reshape(-1)[p] == 5.0 * keep, name
        assert int(got > 0) == bit, name
    assert [q[0] for q in C.planted(1)] == [0] and len(C.planted(3)) == 3 and len(C.planted(63)) == 4
    assert {q[0] % 4 for q in C.planted(64) if q[1] == "zero"} == {q[0] % 4 for q in C.planted(64) if q[1] == "negative zero"} \
        == {0, 1, 2, 3}
    assert np.array_equal(C.bias_grad_ref(g), g.sum(0))


def test_exactness_condition_holds_for_every_case_list():
    """sum_m |dy[m][n]| < 2^24 by construction: the widest integers times the tallest case they are used at."""
    assert 8 * max(C.ACT_M + C.BIAS_M) < C.EXACT_LIMIT
    assert 1 * C.BIAS_LONG_M < C.EXACT_LIMIT
    # the large case draws from {-1, 0, 1}: about two thirds of M, asserted on the device at run time
    assert C.LARGE_M > 2 ** 24 > 0.75 * C.LARGE_M
    assert C.LARGE_M * C.LARGE_N > 262144 * 256           # relu_grad's grid-stride loop takes a second trip
    assert -(-C.LARGE_M * C.LARGE_N // 4 // 4096) > 4096  # act_bias_grad asks for more blocks than its cap


def test_adam_restatement_first_step():
    """After one step from m = v = 0 the update is -lr * sign(g) (up to eps), whatever the gradient's size."""
    g = np.array([3.0, -0.5, 0.0], np.float32)
    p, m, v = C.adam_ref(np.zeros(3), np.zeros(3), np.zeros(3), g, 1e-2, 0.9, 0.999, 1e-8, 1, 1.0)
    np.testing.assert_allclose(p, [-1e-2, 1e-2, 0.0], rtol=1e-6)
    assert p[2] == 0.0 and m[2] == 0.0 and v[2] == 0.0

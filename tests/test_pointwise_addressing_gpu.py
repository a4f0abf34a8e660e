"""Addressing of the persistent pointwise kernel (csrc/pointwise.hip): one descriptor per tile or per 32-row block of
it, the rows inside as per-lane byte offsets.  Shapes are chosen for where that can go wrong, not for the workload:
ragged and nearly-empty last row groups, all-dead padded tiles, dead wave columns, the four-stage and the eight-stage
store schedules, one / two / three tiles per workgroup (both accumulator sets, odd and even last tile).  Every result
is compared with a float64 x @ w.T + bias + residual (ReLU) at the tolerance of test_conv2d_pointwise_vs_fp64, and every
output lies in front of 96 guard rows that must keep their sentinel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5          # max |got - ref| / max |ref|: tests/test_net_gpu.py::test_conv2d_pointwise_vs_fp64
GUARD = 96          # rows behind row M
SENTINEL = -12345.0
ROW_OF = [(b & 3) + 8 * ((b >> 2) & 3) + 4 * (b >> 4) for b in range(32)]  # bit b of a mask word <-> row of its block

SHAPES = [
    # M, N, K
    (432, 160, 128),      # 4.5 row groups, second column block with one live wave; four stages
    (432, 160, 192),      # six stages, stores over the first four
    (432, 160, 256),      # eight stages: the long form
    (432, 160, 1024),     # 32 stages
    (432, 32, 192),       # one live wave in the only column block
    (97, 32, 128),        # one row into the second group; tiles 2 .. 7 all dead
    (97, 32, 256),
    (97, 160, 1024),
    (6912, 1024, 256),    # 576 tiles on <= 512 workgroups: one and two tiles
    (13824, 1024, 256),   # 1152 tiles: two and three
]
VARIANTS = [(res, relu, bias) for res in (False, True) for relu in (False, True) for bias in (False, True)]


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """Host operands and the float64 product of a shape, made once and shared by its tests (on the device)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((M, N)).astype(np.float32)
    prod = x.astype(np.float64) @ w.T.astype(np.float64)
    return tuple(torch.from_numpy(a).cuda() for a in (x, w, bias, res, prod))


def _guarded(M, N):
    return torch.full((M + GUARD, N), SENTINEL, dtype=torch.float32, device="cuda")


def _check(y, M, ref, name):
    sent = torch.tensor(SENTINEL, dtype=torch.float32, device="cuda")
    assert bool((y[M:] == sent).all()), "%s: wrote behind row M" % name
    scale = float(ref.abs().max()) + 1e-30
    err = float((y[:M].double() - ref).abs().max()) / scale
    print("%s: max err / scale = %.3e" % (name, err))
    assert err <= TOL, "%s: max err / scale = %.3e (scale %.3e)" % (name, err, scale)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_pointwise_addressing_vs_fp64(M, N, K):
    from monopsr_amd import _lib
    lib = _lib.lib()
    x, w, bias, res, prod = _operands(M, N, K)
    lib.mpsr_debug_set_conv_pointwise(1)
    try:
        kind, flops = ctypes.c_int(-1), ctypes.c_double(0)
        _lib.check(lib.mpsr_conv2d_plan(1, 1, M, K, N, 1, 1, 1, ctypes.byref(kind), ctypes.byref(flops)))
        assert kind.value == 5
        for has_res, relu, has_bias in VARIANTS:
            y = _guarded(M, N)
            _lib.check(lib.mpsr_conv2d_nhwc_f32(_lib.ptr(x), 1, 1, M, K, _lib.ptr(w), _lib.ptr(bias) if has_bias else None,
                                                _lib.ptr(res) if has_res else None, _lib.ptr(y), N, 1, 1, 1, int(relu),
                                                1, None, 0, _lib.stream()))
            ref = prod
            if has_bias:
                ref = ref + bias.double()
            if has_res:
                ref = ref + res.double()
            if relu:
                ref = torch.relu(ref)
            _check(y, M, ref, "M=%d N=%d K=%d res=%d relu=%d bias=%d" % (M, N, K, has_res, relu, has_bias))
    finally:
        lib.mpsr_debug_set_conv_pointwise(-1)


def _expected_words(pos, M, N):
    """Mask words of a (M, N) bool array: bit b of word [g][n] <-> row 32 g + ROW_OF[b]; rows >= M zero; and the bits
    whose rows exist."""
    G = (M + 31) // 32
    padded = np.zeros((G * 32, N), dtype=bool)
    padded[:M] = pos
    exists = np.zeros((G * 32, 1), dtype=bool)
    exists[:M] = True
    words = np.zeros((G, N), dtype=np.uint32)
    valid = np.zeros((G, 1), dtype=np.uint32)
    for b in range(32):
        words |= padded.reshape(G, 32, N)[:, ROW_OF[b]].astype(np.uint32) << np.uint32(b)
        valid |= exists.reshape(G, 32, 1)[:, ROW_OF[b]].astype(np.uint32) << np.uint32(b)
    return words, valid


def test_pointwise_emit_addressing():
    """conv1x1_pointwise_emit at a ragged M with a dead-wave column block: y against float64, the words against y > 0,
    and nothing written behind row M of y or behind the last word row."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    M, N, K = 432, 160, 256
    x, w, bias, res, prod = _operands(M, N, K)
    assert lib.mpsr_conv1x1_masked_applies(M, K, N) == 1
    nwords = lib.mpsr_relu_bitmask_words(M, N)
    assert nwords == (M + 31) // 32 * N
    gwords = 3 * N  # the word rows a tile's blocks past the last one would land in
    bits = torch.full((nwords + gwords,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    y = _guarded(M, N)
    _lib.check(lib.mpsr_conv1x1_relu_bitmask_f32(_lib.ptr(x), M, K, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(res), 1,
                                                 _lib.ptr(y), _lib.ptr(bits), N, _lib.stream()))
    _check(y, M, torch.relu(prod + bias.double() + res.double()), "emit M=%d N=%d K=%d" % (M, N, K))
    got = bits.cpu().numpy().view(np.uint32)
    assert (got[nwords:] == 0x5a5a5a5a).all(), "wrote behind the last word row"
    want, valid = _expected_words(y[:M].cpu().numpy() > 0, M, N)
    assert np.array_equal(got[:nwords].reshape(-1, N) & valid, want)
    assert 0.2 < float((y[:M] > 0).float().mean()) < 0.8


def test_pointwise_masked_addressing():
    """conv1x1_pointwise_masked at the same shape: kept elements against float64, the others exactly zero."""
    from monopsr_amd import _lib
    lib = _lib.lib()
    M, N, K = 432, 160, 256
    x, w, bias, res, prod = _operands(M, N, K)
    keep = np.random.default_rng(5).random((M, N)) < 0.5
    words, _ = _expected_words(keep, M, N)
    bits = torch.from_numpy(words.view(np.int32).reshape(-1)).cuda()
    y = _guarded(M, N)
    _lib.check(lib.mpsr_conv1x1_masked_f32(_lib.ptr(x), M, K, _lib.ptr(w), None, _lib.ptr(res), _lib.ptr(bits),
                                           _lib.ptr(y), N, _lib.stream()))
    keep_d = torch.from_numpy(keep).cuda()
    ref = torch.where(keep_d, prod + res.double(), torch.zeros_like(prod))
    _check(y, M, ref, "masked M=%d N=%d K=%d" % (M, N, K))
    assert bool((y[:M][~keep_d] == 0).all())

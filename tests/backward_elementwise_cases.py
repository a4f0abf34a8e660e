"""Case lists and plain float64 restatements for the direct tests of the backward pass's elementwise kernels
(tests/test_backward_elementwise.py on the host, tests/test_backward_elementwise_gpu.py on the GPU).

All of these kernels pass gradients through or sum them, so the GPU tests compare EXACTLY: with small-integer
gradients every fp32 partial sum is an integer below 2^24 in any summation order (atomics included), and the result
must equal the float64 reference bit for bit.

Every shape below was chosen from the launchers' own predicates (csrc/backward.hip, csrc/crop_grad.hip); the comments
name the branch a case reaches.
"""
import math

import numpy as np
import torch

from oracle import net as onet

EXACT_LIMIT = float(2 ** 24)  # integers below this are exact in fp32, and so is every partial sum of them

# ------------------------------------------------------------------------------------------------ act_bias_grad
#
# mpsr_act_bias_grad takes act_bias_grad_kernel ("fast") iff N % 4 == 0, N <= 1024, 256 % (N / 4) == 0 and dy, y, dx
# are 16-byte aligned; everything else runs relu_grad_kernel (when y is given) and bias_grad_kernel (when db is).
#   N     groups = N/4   rows per pass = 256/groups
#   4     1              256
#   8     2              128
#   64    16             16
#   256   64             4
#   1024  256            1
ACT_FAST_N = [4, 8, 64, 256, 1024]
#   12    N/4 = 3 does not divide 256          36    N/4 = 9 does not divide 256
#   1028  N > 1024 (N/4 = 257)                 2048  N > 1024 (N/4 = 512)
#   6     N % 4 != 0                           1     N % 4 != 0, one column
ACT_GENERIC_N = [12, 36, 1028, 2048, 6, 1]
# Row slicing.  Fast path: blocks = min(ceil(M N / 4 / 4096), 4096), rows_per_block = ceil(M / blocks), grid =
# ceil(M / rows_per_block); generic path: slices = min(ceil(M / 512), 2048), rows = ceil(M / slices).
#   M = 1     one block, one row (255 of 256 threads idle at N = 4)
#   M = 31    one block; fewer rows than a pass covers at N <= 8 (threads with r0 >= M idle)
#   M = 257   N = 4: one block, second pass holds ONE row; N = 1024: 17 blocks of 16 rows, the last block holds one
#             row; generic: one slice
#   M = 4097  N = 4: 2 blocks of 2049 rows, the last holds 2048; N = 1024: 257 blocks of 16 rows, the last holds one;
#             generic: 9 slices of 456 rows, the last holds 449
ACT_M = [1, 31, 257, 4097]
ACT_REAL_CASE = (4097, 256)  # standard_normal dy: 65 blocks of 64 rows (the last holds one), 4 rows per pass

# The large case shared by relu_grad and act_bias_grad: N = 4, M = 2^24 + 4097 = 4096 * 4097 + 1.
#   relu_grad: 67125252 elements > 262144 * 256 = 67108864, so 16388 threads take a second trip of the grid-stride loop.
#   act_bias_grad: ceil(M / 4096) = 4098 blocks asked, capped at 4096 -> rows_per_block = 4098, grid = 4096 (the last
#   block holds 3 rows: 4095 * 4098 = 16781310).
LARGE_M, LARGE_N = 2 ** 24 + 4097, 4

# ------------------------------------------------------------------------------------------------ bias_grad
#
# bias_grad_kernel: grid = (ceil(N / 256), ceil(M / rows)), rows = ceil(M / min(ceil(M / 512), 2048)).
#   N: 1, 3 (one thread / three threads of a block), 255, 256, 257 (one short of, exactly, one past a block), 1030 (5 blocks)
#   M: 1, 511, 512 (one slice), 513 (two slices of 257 rows, the last holds 256)
BIAS_N = [1, 3, 255, 256, 257, 1030]
BIAS_M = [1, 511, 512, 513]
# past the 2048-slice cap: ceil(M / 512) = 2050 -> 2048 slices of 513 rows, grid.y = 2046 (the last holds 4 rows)
BIAS_LONG_M = 2048 * 512 + 513
BIAS_LONG_N = [1, 3]

RELU_TOTALS = [1, 255, 256, 257]  # one block short by 255 / by one / full / a second block with one element

# ------------------------------------------------------------------------------------------------ relu_bitmask
#
# A thread owns 32 rows x 4 columns; rows == 32 takes the unrolled branch, fewer the guarded loop.
#   M = 1, 31   one row group on the guarded branch        M = 32  one full group
#   M = 33      a full group and a group of ONE row        M = 69  two full groups and a group of 5 rows
#   N = 4, 8, 12 (1, 2, 3 column groups), 260 (65 column groups: a thread's rows are 1040 bytes apart)
# (129, 260) is 5 x 65 = 325 threads: the only case with a second block, whose last 187 threads have nothing to do.
BITMASK_M = [1, 31, 32, 33, 69]
BITMASK_N = [4, 8, 12, 260]
BITMASK_EXTRA = [(129, 260)]

# ------------------------------------------------------------------------------------------------ max_pool_grad
MAX_POOL_CASES = [
    # shape (B,H,W,C), k, s, padding
    ((2, 7, 9, 4), 3, 2, "SAME"),    # odd sizes: total padding 2, top = left = 1
    ((1, 8, 8, 3), 3, 2, "SAME"),    # even sizes: total padding 1, top = left = 0 (bottom / right padded); C % 4 != 0
    ((2, 6, 6, 4), 2, 2, "VALID"),
    ((1, 1, 5, 4), 3, 2, "SAME"),    # height 1: two of three window rows are padding
    ((1, 9, 10, 2), 3, 1, "SAME"),   # overlapping windows: several outputs route to one cell (atomics meet)
]

# ------------------------------------------------------------------------------------------------ resize_bilinear_grad
#
# scale = (in - 1) / (out - 1) with align_corners (out > 1), else in / out.  The gather kernel runs iff
# 2 / scale + 4 <= RG_MAX = 12 on BOTH axes (scale >= 0.25), C % 4 == 0 and dy, dx are 16-byte aligned; otherwise
# memset + scatter kernel.  Dyadic scales make every weight a multiple of 1/8 per axis: exact in fp32.
RESIZE_EXACT_CASES = [
    # (h, w), (OH, OW), align_corners, form at C = 4 aligned
    ((3, 3), (9, 9), True, "gather"),     # 2/8 = 0.25 on both axes: 2 / 0.25 + 4 == 12, the last ratio the gather form takes
    ((2, 3), (9, 5), True, "scatter"),    # 1/8 vertically: 20 > 12
    ((5, 3), (9, 5), True, "gather"),     # 0.5, 0.5
    ((4, 2), (8, 16), False, "scatter"),  # 0.5, 1/8
    ((2, 2), (16, 4), False, "scatter"),  # 1/8, 0.5
    ((9, 9), (5, 3), True, "gather"),     # 2, 4: downsampling, inputs off the sample grid receive nothing
    ((8, 8), (4, 2), False, "gather"),    # 2, 4
]
RESIZE_VARIANTS = ["c4", "c3", "c4_offset"]  # C = 3 and the view offset by one float force the scatter form
RESIZE_TOL_CASES = [
    ((5, 7), (9, 4), False),      # 5/9, 7/4
    ((37, 12), (32, 10), False),  # 37/32, 1.2
    ((7, 9), (13, 9), True),      # 0.5, 1
]
RESIZE_B = 2


def resize_form(case, variant):
    """The kernel the launcher's predicate picks."""
    return case[3] if variant == "c4" else "scatter"


# ------------------------------------------------------------------------------------------------ crop_and_resize_grad
# the seven boxes of test_crop_and_resize_vs_oracle: inside, whole image, partly outside, zero area, flipped, narrow,
# fully outside
CROP_BOXES = np.array([[0.1, 0.2, 0.6, 0.9], [0.0, 0.0, 1.0, 1.0], [-0.2, 0.3, 0.5, 1.3], [0.4, 0.4, 0.4, 0.4],
                       [0.9, 0.1, 0.2, 0.8], [0.25, 0.25, 0.75, 0.5], [2.0, 2.0, 3.0, 3.0]], np.float32)
CROP_IND = np.array([0, 1, 0, 1, 0, 1, 0], np.int32)
CROP_OUTSIDE = 6          # index of the fully-outside box
CROP_IMAGE = (2, 9, 11)   # nimg, H, W
CROP_C = [3, 4]
CROP_SIZES = [(5, 7), (1, 1), (1, 4)]  # (1, 1) and (1, 4): a one-sample axis reads the box's centre line
# box_ind given; NULL (every box reads image 0); the whole-image box pointed past the last image / before the first
CROP_IND_MODES = ["given", "null", "past_end", "negative"]
CROP_BAD_BOX = 1

ADAM_N = [1, 257, 10007]  # one thread; a second block with one element; 40 blocks, the last ragged
ADAM_GRAD_SCALES = [1.0, 0.25]
ADAM_STEPS = 3


# ================================================================================================ inputs

def int_grad(rng, shape, wide=True):
    """Integer gradients as float32: [-8, 8], or {-1, 0, 1} for the tall cases."""
    lo, hi = (-8, 9) if wide else (-1, 2)
    return rng.integers(lo, hi, shape).astype(np.float32)


# kind -> (value planted in y, multiplier of dy in the gradient, mask bit)
SPECIALS = [("zero", np.float32(0.0), 0, 0), ("negative zero", np.float32(-0.0), 0, 0),
            ("infinity", np.float32(np.inf), 1, 1), ("nan", np.float32(np.nan), 0, 0)]


def planted(total):
    """(flat position, name, value, multiplier of dy, mask bit) of every planted value: the four kinds at the first
    element, one third, two thirds and the last element (as many as fit a tiny tensor), and -- from 64 elements on --
    0.0 and -0.0 on eight consecutive elements from a multiple of four near the middle, so that every lane of a float4
    access meets both zeros."""
    pos = [0, total // 3, 2 * total // 3, total - 1] if total >= 4 else list(range(total))
    out = [(p,) + s for p, s in zip(pos, SPECIALS)]
    if total >= 64:
        base = 4 * (total // 8)
        out += [(base + j,) + SPECIALS[j >> 2] for j in range(8)]
    assert len({o[0] for o in out}) == len(out) and all(0 <= o[0] < total for o in out)
    return out


def activations(rng, shape, dy=None):
    """standard_normal float32 with exact 0.0, -0.0, +inf and NaN planted (see planted); dy (if given) is made non-zero
    there, so that a kernel that lets a gradient through where it must not is seen."""
    y = rng.standard_normal(shape).astype(np.float32)
    flat = y.reshape(-1)
    for p, _, value, _, _ in planted(flat.size):
        flat[p] = value
        if dy is not None:
            dy.reshape(-1)[p] = 5.0
    return y


def pool_input(rng, shape):
    """max(integers in [-3, 3), 0): two thirds exact zeros, so most windows tie at zero and many at 1 or 2."""
    return np.maximum(rng.integers(-3, 3, shape), 0).astype(np.float32)


# ================================================================================================ restatements

def mask_row(b):
    return (b & 3) + 8 * ((b >> 2) & 3) + 4 * (b >> 4)


def relu_grad_ref(dy, y):
    """dy * (y > 0) in float64 (NaN > 0 is false)."""
    return np.where(y > 0, dy.astype(np.float64), 0.0)


def bias_grad_ref(g):
    """Column sums in float64; also asserts the exactness condition sum_m |g[m][n]| < 2^24."""
    g = np.asarray(g, np.float64)
    assert np.abs(g).sum(0).max() < EXACT_LIMIT
    return g.sum(0)


def relu_bitmask_ref(y, M, N):
    """bit b of word[(m >> 5) * N + n] = y[32 (m >> 5) + mask_row(b)][n] > 0, zero where that row is >= M."""
    y = np.asarray(y).reshape(M, N)
    groups = (M + 31) // 32
    words = np.zeros((groups, N), np.uint32)
    for g in range(groups):
        for b in range(32):
            m = 32 * g + mask_row(b)
            if m >= M:
                continue
            for n in range(N):
                if y[m, n] > 0:
                    words[g, n] |= np.uint32(1 << b)
    return words.reshape(-1)


def same_padding(size, k, s):
    out = -(-size // s)
    return out, max((out - 1) * s + k - size, 0) // 2


def max_pool_grad_ref(x, dy, k, s, padding):
    """Every output cell scans its window in (ky, kx) order, skips padded cells and routes its gradient to the first
    strict maximum (TensorFlow's rule)."""
    B, H, W, C = x.shape
    if padding == "SAME":
        (OH, pt), (OW, pl) = same_padding(H, k, s), same_padding(W, k, s)
    else:
        OH, OW, pt, pl = (H - k) // s + 1, (W - k) // s + 1, 0, 0
    assert dy.shape == (B, OH, OW, C), (dy.shape, (B, OH, OW, C))
    dx = np.zeros(x.shape, np.float64)
    for b in range(B):
        for oy in range(OH):
            for ox in range(OW):
                for c in range(C):
                    best, at = -math.inf, None
                    for ky in range(k):
                        yy = oy * s - pt + ky
                        if yy < 0 or yy >= H:
                            continue
                        for kx in range(k):
                            xx = ox * s - pl + kx
                            if xx < 0 or xx >= W:
                                continue
                            if x[b, yy, xx, c] > best:
                                best, at = x[b, yy, xx, c], (yy, xx)
                    if at is not None:
                        dx[b, at[0], at[1], c] += float(dy[b, oy, ox, c])
    return dx


def max_pool_out_shape(shape, k, s, padding):
    B, H, W, C = shape
    if padding == "SAME":
        return (B, same_padding(H, k, s)[0], same_padding(W, k, s)[0], C)
    return (B, (H - k) // s + 1, (W - k) // s + 1, C)


def max_pool_grad_autograd(x, dy, k, s, padding):
    xr = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    onet.tf_max_pool(xr, k, s, padding).backward(torch.from_numpy(np.asarray(dy, np.float64)))
    return xr.grad.numpy()


def resize_grad_ref(dy, h, w, align_corners):
    """float64 autograd through oracle.net.tf_resize_bilinear (linear in its input: the point it is taken at is free)."""
    B, OH, OW, C = dy.shape
    xr = torch.zeros((B, h, w, C), dtype=torch.float64, requires_grad=True)
    onet.tf_resize_bilinear(xr, OH, OW, align_corners).backward(torch.from_numpy(np.asarray(dy, np.float64)))
    return xr.grad.numpy()


def crop_grad_ref(dy, nimg, H, W, boxes, ind):
    """float64 autograd through oracle.net.tf_crop_and_resize (linear in the image)."""
    nb, ch, cw, C = dy.shape
    xr = torch.zeros((nimg, H, W, C), dtype=torch.float64, requires_grad=True)
    if nb == 0:
        return np.zeros((nimg, H, W, C))
    out = onet.tf_crop_and_resize(xr, boxes, ind, ch, cw, 0.0)
    # (+ 0 * sum: when every sample is extrapolated the crop does not depend on the image at all)
    ((out * torch.from_numpy(np.asarray(dy, np.float64))).sum() + 0.0 * xr.sum()).backward()
    return xr.grad.numpy()


def adam_lr_t(lr, b1, b2, step):
    """lr * sqrt(1 - b2^t) / (1 - b1^t) in float64, from the float32 hyper-parameters the C ABI receives."""
    lr, b1, b2 = float(np.float32(lr)), float(np.float32(b1)), float(np.float32(b2))
    return lr * math.sqrt(1.0 - math.pow(b2, step)) / (1.0 - math.pow(b1, step))


def adam_ref(p, m, v, g, lr, b1, b2, eps, step, grad_scale):
    """One step of the TensorFlow formula in float64 (hyper-parameters rounded to the float32 the C ABI takes)."""
    b1, b2, eps = float(np.float32(b1)), float(np.float32(b2)), float(np.float32(eps))
    g = g.astype(np.float64) * grad_scale
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - adam_lr_t(lr, b1, b2, step) * m / (np.sqrt(v) + eps)
    return p, m, v

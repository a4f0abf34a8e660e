"""Case lists, launch geometry, float64 restatements and error bounds for the direct tests of the training-mode
batch-norm entry points of csrc/batchnorm.hip (tests/test_batch_norm_kernels.py on the host,
tests/test_batch_norm_kernels_gpu.py on the GPU).

Two kinds of comparison:

EXACT.  With the inputs of exact_problem (small integers and dyadic fractions) every fp32 difference, product, fused
multiply-add and per-thread partial sum of the kernels is exactly representable, in any order and under any
contraction, and the fp64 atomics add integers or multiples of 1/4.  The results must then equal the float64
restatements bit for bit: a dropped row, a wrong loop tail or a wrong tie rule cannot hide in a tolerance.

BOUNDED.  With real-valued inputs the kernels are held to bounds DERIVED from the reference (u = 2^-24, the unit
roundoff of fp32); none of them was tuned against the code under test.
  per-channel sums   a thread adds n = terms_per_thread(M, C) terms in fp32; everything after that is fp64.  The
                     standard bound of recursive summation gives, with one more rounding for the difference z - z[0]
                     (two more, squared, plus the product's, for the squares; the three of g * (z - mean) * inv_std),
                       |sum - ref| <= (n + 1) u sum|term|,      |sumsq - ref| <= (n + 3) u sum term^2
  elementwise        k u (sum of the magnitudes of the terms), k = the roundings an input meets on its way out, counted
                     to first order from the kernel's expression (a contraction only removes roundings):
                       APPLY_K = 2   y = fma(z - mean, inv_std, beta):           the difference, the fma
                       GRAD_K  = 5   dz = inv_std * (g - mean_g - ((z - mean) * inv_std) * mean_gz):
                                     the difference, two products, the subtraction from g - mean_g, the last product
                                     (g itself meets three: g - mean_g, the subtraction, the last product)
                       MOVING_K = 4  m * decay + (1 - decay) * (float)stat:  1 - decay, the conversion, the product, the sum
  propagated         where a result is compared with the statistics of z itself and not with the kernel's own vectors,
                     the bounds above are carried through the formulas to first order (operator_bounds).

The launch geometry (slicing, RowMap, stream_grid) is restated here as plain functions; every shape below was chosen
from it, and the comments name the branch a case reaches (tests/test_batch_norm_kernels.py asserts each claim).
"""
from types import SimpleNamespace

import torch

U = 2.0 ** -24
EXACT_LIMIT = 2 ** 24  # integers below this are exact in fp32, and so is every partial sum of them
APPLY_K, GRAD_K, MOVING_K = 2, 5, 4

# ================================================================================================ launch geometry
R_THREADS = 1024          # threads of a reducing workgroup
MAX_BLOCKS = 256          # cap of the reducing kernels' grid
STREAM_THREADS = 256      # threads of an elementwise workgroup
STREAM_MAX_BLOCKS = 65536  # cap of the elementwise kernels' grid


def slicing(M):
    """(blocks, rows per block, rows of the last block) of the reducing kernels."""
    b = min((M + 255) // 256, MAX_BLOCKS)
    rows = (M + b - 1) // b
    blocks = (M + rows - 1) // rows
    return blocks, rows, M - (blocks - 1) * rows


def row_map(C):
    """(groups, rstride, idle threads): thread t reads float4 column group t % groups of the rows t // groups,
    t // groups + rstride, ...; threads with t // groups >= rstride have nothing to do."""
    groups = C // 4
    rstride = R_THREADS // groups
    return groups, rstride, R_THREADS - groups * rstride


def terms_per_thread(M, C):
    """n: the most terms one thread adds in fp32."""
    return -(-slicing(M)[1] // row_map(C)[1])


def stream_grid(n4):
    return min((n4 + STREAM_THREADS - 1) // STREAM_THREADS, STREAM_MAX_BLOCKS)


def second_trip_threads(M, C):
    """Threads of an elementwise kernel that take a second trip of the grid-stride loop."""
    return max(0, M * (C // 4) - stream_grid(M * (C // 4)) * STREAM_THREADS)


def thread_rows(m0, m1, r0, st, drop_tail=False):
    """The rows one thread of a reducing kernel visits in block [m0, m1): the loop with four rows in flight, then its
    tail, written as the kernel writes them.  drop_tail: the deliberately wrong variant of the host-side mutation check
    (the tail loop stops one row early)."""
    out, r = [], m0 + r0
    while r + 3 * st < m1:
        out += [r, r + st, r + 2 * st, r + 3 * st]
        r += 4 * st
    while r < (m1 - 1 if drop_tail else m1):
        out.append(r)
        r += st
    return out


def row_visits(M, C, drop_tail=False):
    """How often the reducing kernels' loops visit each row (per column group): all ones when they are right."""
    blocks, rows, _ = slicing(M)
    _, st, _ = row_map(C)
    visits = torch.zeros(M, dtype=torch.float64)
    for b in range(blocks):
        m0, m1 = b * rows, min(M, (b + 1) * rows)
        for r0 in range(st):
            for r in thread_rows(m0, m1, r0, st, drop_tail):
                visits[r] += 1
    return visits


def unrolled_trips(rows_in_block, st, r0):
    """(trips of the four-row loop, rows left to the tail) of thread row r0 in a block of that many rows."""
    trips, r = 0, r0
    while r + 3 * st < rows_in_block:
        trips, r = trips + 1, r + 4 * st
    return trips, len(thread_rows(0, rows_in_block, r0, st)) - 4 * trips


def rows_for_block_rows(target):
    """The M whose blocks hold `target` rows each: M = target in one block up to 256, else 256 full blocks."""
    M = target if target <= 256 else MAX_BLOCKS * target
    assert slicing(M)[1] == target
    return M


def unroll_boundary_rows(C):
    """M that put a block's row count at 4 rstride - 1, 4 rstride, 4 rstride + 1:
       4 st - 1   the thread rows r0 < st - 1 take one trip of the four-row loop, r0 = st - 1 takes none: three tail rows
       4 st       every thread takes exactly one trip and no tail
       4 st + 1   r0 = 0 takes one trip and one tail row"""
    st = row_map(C)[1]
    return [rows_for_block_rows(4 * st + d) for d in (-1, 0, 1)]


#   C     groups  rstride  idle threads   reduce_columns reads pa[r * groups + t]
#   4     1       1024     0
#   8     2       512      0
#   12    3       341      1              stride 3: not a power of two
#   260   65      15       49             stride 65
#   1020  255     4        4              stride 255
#   1024  256     4        0
CHANNELS = [4, 8, 12, 260, 1020, 1024]
ROW_MAP_CLAIMS = {4: (1, 1024, 0), 8: (2, 512, 0), 12: (3, 341, 1), 260: (65, 15, 49), 1020: (255, 4, 4), 1024: (256, 4, 0)}

#   M       blocks x rows (last)
#   1       1 x 1            one row: the shift IS the row, every sum is 0; the unbias clamp M / max(M - 1, 1) = 1
#   3       1 x 3            fewer rows than thread rows at every C (rstride >= 4): the thread rows r0 >= 3 add nothing
#   255     1 x 255          one block, one short of the slicing step
#   256     1 x 256          the last M in one block
#   257     2 x 129 (128)    the first M in two blocks
#   513     3 x 171
#   4097    17 x 241
#   65536   256 x 256        the last M below the cap of 256 blocks
#   65537   256 x 257 (2)    past the cap: 257 blocks asked; the last block holds two rows
ROWS = [1, 3, 255, 256, 257, 513, 4097, 65536, 65537]
SLICING_CLAIMS = {1: (1, 1, 1), 3: (1, 3, 3), 255: (1, 255, 255), 256: (1, 256, 256), 257: (2, 129, 128),
                  513: (3, 171, 171), 4097: (17, 241, 241), 65536: (256, 256, 256), 65537: (256, 257, 2)}

# the full grid, and per C the three M around the boundary of the four-row loop (C = 4: 256 blocks of 4095 / 4096 / 4097
# rows; C = 260: one block of 59 / 60 / 61 rows; C = 1020, 1024: 15 / 16 / 17 rows)
EXACT_CASES = [(C, M) for C in CHANNELS for M in ROWS] + [(C, M) for C in CHANNELS for M in unroll_boundary_rows(C)]

# elementwise kernels only: n4 = M exceeds 65536 * 256 = 2^24 threads, so 4097 threads take a second trip of the loop
LARGE_C, LARGE_M = 4, 2 ** 24 + 4097

# real-valued inputs: every C, M in {one row, two blocks, 17 ragged blocks, past the cap}
REAL_ROWS = [1, 257, 4097, 65537]
REAL_CASES = [(C, M) for C in CHANNELS for M in REAL_ROWS]

# conditioning: (name, M, C); see conditioned_z
CONDITIONING_CASES = [("mean at 1e3 sigma", 4097, 260), ("mean at 1e4 sigma", 4097, 260), ("row 0 at 30 sigma", 65537, 8)]

NAN_CASES = [(257, 12), (4097, 260)]
OPERATOR_CASES = [(1031, 12), (1031, 260)]  # 1031 is prime: 5 blocks of 207 rows (203 in the last)

EPS = 1e-3  # slim.batch_norm's default; the C ABI takes it as a float


def f32(x):
    """A Python float rounded to float32, as the C ABI receives eps and decay."""
    return float(torch.tensor(x, dtype=torch.float32).double())


# ================================================================================================ exact inputs
PLANT_EVERY = 5  # every fifth row holds z = mean + k: pre-activation exactly 0, +1/8 or -1/8 by channel


def planted_rows(M):
    """Rows 1, 6, 11, ... (row 0 when it is the only one).  Row 0 stays ordinary: it is the shift of the sums, and were
    it planted every planted row would have z - z[0] = 0 and be invisible to them."""
    return slice(min(1, M - 1), None, PLANT_EVERY)


def exact_problem(M, C, device="cpu", seed=None):
    """z, dy in [-8, 8] (integers); mean in [-3, 3] (integer); inv_std in {0.25, 0.5, 1, 2}; beta = -k inv_std + j / 8
    with k in [-3, 3] and j = 0, +1, -1 for channel % 3 = 0, 1, 2 (multiples of 1/8); mean_g in [-1, 1] and mean_gz in
    [-2, 2] (multiples of 1/8).  Every PLANT_EVERY-th row (planted_rows) holds z = mean + k, whose pre-activation
    (z - mean) inv_std + beta is EXACTLY j / 8: zero in a third of the channels and one step of the grid either side of
    zero in the others; dy is 5 there, so a gradient let through at a zero pre-activation is seen.  Elsewhere z is
    uniform, so about 1/17 of the remaining pre-activations of the j = 0 channels are zero as well."""
    n = terms_per_thread(M, C)
    # the preconditions of exactness, on the largest per-thread partials there can be:
    #   (z - z[0])^2 <= 16^2 = 256 per term;  g (z - mean) inv_std <= 8 * 11 * 2 = 176 in steps of 1/4 (704 quarter units)
    assert 256 * n < EXACT_LIMIT and 704 * n < EXACT_LIMIT, (M, C, n)
    g = torch.Generator(device=device).manual_seed(1000003 * C + M if seed is None else seed)

    def ints(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, device=device, generator=g, dtype=torch.float32)

    mean, k = ints(-3, 3, (C,)), ints(-3, 3, (C,))
    inv_std = torch.exp2(ints(-2, 1, (C,)))
    j = torch.tensor([0.0, 1.0, -1.0], device=device)[torch.arange(C, device=device) % 3]
    beta = -k * inv_std + j / 8
    mean_g, mean_gz = ints(-8, 8, (C,)) / 8, ints(-16, 16, (C,)) / 8
    z, dy = ints(-8, 8, (M, C)), ints(-8, 8, (M, C))
    z[planted_rows(M)] = mean + k
    dy[planted_rows(M)] = 5.0
    return SimpleNamespace(M=M, C=C, n=n, z=z, dy=dy, mean=mean, inv_std=inv_std, beta=beta, mean_g=mean_g, mean_gz=mean_gz,
                           j=j)


def conditioned_z(name, M, C, device, seed=0):
    """Real-valued z = randn * 2 + offset (sigma = 2): the per-channel mean 1e3 or 1e4 sigma from zero with an ordinary
    row 0 (the shift by row 0 then takes the mean out before anything is squared), or row 0 itself 30 sigma from the
    rest (the shift then ADDS an offset of 30 sigma to every term)."""
    g = torch.Generator(device=device).manual_seed(seed + M + C)
    z = torch.randn((M, C), device=device, generator=g) * 2
    if name == "mean at 1e3 sigma":
        z += 2e3
    elif name == "mean at 1e4 sigma":
        z += 2e4
    elif name == "row 0 at 30 sigma":
        z += 1
        z[0] += 60
    else:
        raise KeyError(name)
    return z


# ================================================================================================ restatements (float64)

def stats_ref(z):
    """sum_m (z - z[0]), sum_m (z - z[0])^2."""
    d = z.double() - z.double()[0]
    return d.sum(0), (d * d).sum(0)


def finalize_ref(s, q, z0, M, eps, decay, moving_mean=None, moving_variance=None):
    """mean, biased variance, inv_std, and the moving statistics' update with the unbiased variance."""
    d = s / M
    mean = z0.double() + d
    var = torch.clamp(q / M - d * d, min=0.0)
    inv_std = 1.0 / torch.sqrt(var + eps)
    unbias = M / max(M - 1, 1)
    mm = None if moving_mean is None else moving_mean.double() * decay + (1.0 - decay) * mean
    mv = None if moving_variance is None else moving_variance.double() * decay + (1.0 - decay) * var * unbias
    return SimpleNamespace(d=d, mean=mean, var=var, inv_std=inv_std, unbias=unbias, moving_mean=mm, moving_variance=mv)


def preact_ref(z, mean, inv_std, beta):
    return (z.double() - mean.double()) * inv_std.double() + beta.double()


def apply_ref(z, mean, inv_std, beta, relu):
    a = preact_ref(z, mean, inv_std, beta)
    return torch.clamp(a, min=0.0) if relu else a


def masked(dy, mask):
    """g = dy where the mask holds (mask None: no ReLU)."""
    return dy.double() if mask is None else torch.where(mask, dy.double(), torch.zeros((), dtype=torch.float64, device=dy.device))


def grad_sums_ref(dy, mask, z, mean, inv_std):
    """sum_m g, sum_m g zhat."""
    g = masked(dy, mask)
    zhat = (z.double() - mean.double()) * inv_std.double()
    return g.sum(0), (g * zhat).sum(0)


def grad_finalize_ref(sum_g, sum_gz, count, dbeta):
    """dbeta + (float)sum_g (in fp32, as the kernel deposits it), sum_g / count, sum_gz / count."""
    return (None if dbeta is None else dbeta + sum_g.float()), sum_g / count, sum_gz / count


def grad_ref(dy, mask, z, mean, inv_std, mean_g, mean_gz):
    """dz = inv_std (g - mean_g - zhat mean_gz)."""
    g = masked(dy, mask)
    zhat = (z.double() - mean.double()) * inv_std.double()
    return inv_std.double() * (g - mean_g.double() - zhat * mean_gz.double())


def composed_ref(z, beta, dy, relu, eps, decay, moving_mean, moving_variance, mask=None):
    """All restatements in a row on float64 inputs: what BatchNormReluFn computes.  mask: the ReLU mask to use in place
    of the reference's own (the GPU tests pass the kernel's, so that a sign at the rounding edge decides nothing)."""
    M = z.shape[0]
    s, q = stats_ref(z)
    st = finalize_ref(s, q, z[0], M, eps, decay, moving_mean, moving_variance)
    a = preact_ref(z, st.mean, st.inv_std, beta)
    if relu and mask is None:
        mask = a > 0
    y = torch.where(mask, a, torch.zeros((), dtype=torch.float64, device=a.device)) if relu else a
    sg, sgz = grad_sums_ref(dy, mask if relu else None, z, st.mean, st.inv_std)
    _, mg, mgz = grad_finalize_ref(sg, sgz, float(M), None)
    dz = grad_ref(dy, mask if relu else None, z, st.mean, st.inv_std, mg, mgz)
    return SimpleNamespace(stats=st, a=a, y=y, mask=mask if relu else None, sum_g=sg, sum_gz=sgz, mean_g=mg, mean_gz=mgz, dz=dz)


# ================================================================================================ bounds

def ulp32(x):
    """The spacing of float32 at |x| (2^-24 at zero: only ever added to a tolerance)."""
    _, e = torch.frexp(x.double().abs())
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), torch.clamp(e - 24, min=-149))


def summation_bounds(n, abs_sum, sq_sum):
    """(n + 1) u sum|term| for a plain sum, (n + 3) u sum|term| for a sum of products."""
    return (n + 1) * U * abs_sum, (n + 3) * U * sq_sum


def stats_bounds(z, n):
    d = z.double() - z.double()[0]
    return summation_bounds(n, d.abs().sum(0), (d * d).sum(0))


def moving_bound(m0, decay, stat):
    """The kernel's own roundings in m0 * decay + (1 - decay) * (float)stat (the conversion included)."""
    return MOVING_K * U * ((m0.double() * decay).abs() + ((1.0 - decay) * stat).abs())


def apply_bound(z, mean, inv_std, beta):
    return APPLY_K * U * (((z.double() - mean.double()) * inv_std.double()).abs() + beta.double().abs())


def grad_bound(dy, mask, z, mean, inv_std, mean_g, mean_gz):
    g = masked(dy, mask)
    zhat = (z.double() - mean.double()) * inv_std.double()
    return GRAD_K * U * inv_std.double() * (g.abs() + mean_g.double().abs() + (zhat * mean_gz.double()).abs())


def grad_sums_bounds(dy, mask, z, mean, inv_std, n):
    g = masked(dy, mask)
    zhat = (z.double() - mean.double()) * inv_std.double()
    return summation_bounds(n, g.abs().sum(0), (g * zhat).abs().sum(0))


def statistics_bounds(z, n, eps):
    """The _stats bounds carried into mean, variance and inv_std, against the statistics of z.double() itself:
       |mean - ref| <= bS / M (+ 1 ulp for the conversion),  |var - ref| <= bQ / M + 2 |d| bS / M,
       |inv_std - ref| <= inv_std^3 / 2 * (the variance's) + 1 ulp."""
    M = z.shape[0]
    z64 = z.double()
    bS, bQ = stats_bounds(z, n)
    s, q = stats_ref(z)
    d = s / M
    mean, var = z64.mean(0), z64.var(0, unbiased=False) if M > 1 else torch.zeros_like(d)
    inv_std = 1.0 / torch.sqrt(var + eps)
    e_var = bQ / M + 2 * d.abs() * bS / M
    return SimpleNamespace(mean=mean, var=var, inv_std=inv_std, bS=bS, bQ=bQ, e_mean_exact=bS / M, e_mean=bS / M + ulp32(mean),
                           e_var=e_var, e_inv_std=0.5 * inv_std ** 3 * e_var + ulp32(inv_std))


def operator_bounds(z, beta, dy, mask, n, eps, decay, moving_mean, moving_variance):
    """Tolerances of the whole operator against composed_ref on the same float64 inputs, to first order: the kernels'
    own roundings (above) plus what the errors of mean and inv_std do to everything downstream of them.
       zhat = (z - mean) inv_std:     e_zhat = inv_std e_mean + |z - mean| e_inv
       y = zhat + beta:               APPLY_K u (|zhat| + |beta|) + e_zhat
       sum_g:                         bG
       sum_gz:                        bGZ + sum_m |g| e_zhat                   (the kernel sums with ITS zhat)
       mean_g, mean_gz:               the sums' / M + 1 ulp
       dz = inv_std r, r = g - mean_g - zhat mean_gz:
                                      GRAD_K u inv_std (|g| + |mean_g| + |zhat mean_gz|) + e_inv |r|
                                      + inv_std (e_mean_g + e_zhat |mean_gz| + |zhat| e_mean_gz)
       moving statistics:             MOVING_K u (|m0 decay| + |(1 - decay) stat|) + (1 - decay) (the statistic's)"""
    M = z.shape[0]
    sb = statistics_bounds(z, n, eps)
    ref = composed_ref(z.double(), beta.double(), dy.double(), mask is not None, eps, decay, moving_mean, moving_variance, mask)
    inv = ref.stats.inv_std
    zc = z.double() - ref.stats.mean
    zhat = zc * inv
    e_zhat = inv * sb.e_mean + zc.abs() * sb.e_inv_std
    g = masked(dy, mask)
    bG, bGZ = summation_bounds(n, g.abs().sum(0), (g * zhat).abs().sum(0))
    bGZ = bGZ + (g.abs() * e_zhat).sum(0)
    e_mg, e_mgz = bG / M + ulp32(ref.mean_g), bGZ / M + ulp32(ref.mean_gz)
    r = g - ref.mean_g - zhat * ref.mean_gz
    e_dz = GRAD_K * U * inv * (g.abs() + ref.mean_g.abs() + (zhat * ref.mean_gz).abs()) + sb.e_inv_std * r.abs() \
        + inv * (e_mg + e_zhat * ref.mean_gz.abs() + zhat.abs() * e_mgz)
    unb = ref.stats.unbias
    return SimpleNamespace(
        ref=ref, y=APPLY_K * U * (zhat.abs() + beta.double().abs()) + e_zhat, dz=e_dz, dbeta=bG + ulp32(ref.sum_g),
        moving_mean=moving_bound(moving_mean, decay, ref.stats.mean) + (1.0 - decay) * sb.e_mean,
        moving_variance=moving_bound(moving_variance, decay, ref.stats.var * unb)
        + (1.0 - decay) * (unb * sb.e_var + ulp32(ref.stats.var * unb)))


def worst_ratio(err, bound):
    """max err / bound; where the bound is zero the error must be."""
    err, bound = (t.reshape(-1) for t in torch.broadcast_tensors(err.double(), bound.double()))
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an error where the bound is zero"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / bound[~zero]).max())

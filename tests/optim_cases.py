"""Chunk tables, gradients and plain float64 restatements for the direct tests of the optimiser tail, csrc/optim.hip:
per-variable squared norms (seg_sumsq_kernel, seg_sum_kernel), tf.clip_by_norm (seg_scale_kernel) and the fused clip ->
Adam -> moving average pass (clip_adam_ema_kernel).  tests/test_optim_cases.py checks this module on the host,
tests/test_optim_gpu.py runs the kernels against it through the C ABI.

The trainer only ever builds one shape of table (InstanceTrainer._clip_table: 256-byte aligned chunks of exactly 16384
floats but a variable's last, a few dozen chunks per variable, no empty segment, no empty chunk).  The C ABI promises
any ascending table; the tables below were chosen from the kernels' own predicates, and the comment beside each names the
branch it reaches.

Exactness.  The gradients are integers times 2^-6, so every square is an integer times 2^-12 and -- as long as a
segment's INTEGER sum of squares stays below 2^24 -- every partial sum of squares is exact in fp32 in any order, fused
multiply-adds included: sumsq must equal the float64 sum bit for bit.  exact_grad narrows the integers to {-1, 0, 1}
wherever a segment could reach 2^24, and check_exact asserts the condition for every segment.

Nothing here imports monopsr_amd.
"""
import collections
import functools
import math

import numpy as np

from backward_elementwise_cases import EXACT_LIMIT, adam_lr_t, adam_ref

U = 2.0 ** -24          # unit roundoff of fp32
GRAD_UNIT = 2.0 ** -6   # exact gradients are integers times this
THREADS = 256           # kThreads of optim.hip
GAP_FILL = -77.0        # finite value kept in the elements outside every chunk

# chunk_seg (int32), chunk_begin (int64), chunk_len (int32), n_segments, buffer length in floats
Table = collections.namedtuple("Table", "chunk_seg chunk_begin chunk_len n_segments size")


def make_table(chunks, n_segments=None, tail=5):
    """(segment id, begin, length) triples -> Table.  n_segments defaults to the last id + 1; the buffer ends `tail`
    untouched floats behind the last chunk."""
    seg = np.array([c[0] for c in chunks], np.int32)
    begin = np.array([c[1] for c in chunks], np.int64)
    length = np.array([c[2] for c in chunks], np.int32)
    if n_segments is None:
        n_segments = int(seg.max()) + 1
    return Table(seg, begin, length, int(n_segments), int((begin + length).max()) + tail)


def place(items, gaps=(1, 2, 3, 4, 5), start=3):
    """(segment id, begin % 4 or None, length) -> (segment id, begin, length): chunks laid out one behind the other with
    gaps cycling through `gaps`; where begin % 4 is asked for, the gap is the one of 1..5 that gives it (two fit when
    the alignment allows: they alternate)."""
    out, cursor, k = [], start, 0
    for seg, mod, n in items:
        if mod is None:
            gap = gaps[k % len(gaps)]
        else:
            fit = [g for g in range(1, 6) if (cursor + g) % 4 == mod]
            gap = fit[k % len(fit)]
        k += 1
        out.append((seg, cursor + gap, n))
        cursor += gap + n
    return out


def elements(table):
    """(flat index, segment id) of every element some chunk covers, in table order."""
    idx = [np.arange(b, b + n, dtype=np.int64) for b, n in zip(table.chunk_begin, table.chunk_len)]
    seg = [np.full(n, s, np.int64) for s, n in zip(table.chunk_seg, table.chunk_len)]
    return np.concatenate(idx), np.concatenate(seg)


def covered(table):
    mask = np.zeros(table.size, bool)
    mask[elements(table)[0]] = True
    return mask


def chunks_per_segment(table):
    return np.bincount(table.chunk_seg, minlength=table.n_segments)


# ------------------------------------------------------------------------------------------------ ALIGNMENT
#
# seg_sumsq_kernel takes the float4 loop iff the chunk's first BYTE address is a multiple of 16.  The buffer is 256-byte
# aligned (the GPU test asserts it), so begin % 4 == 0 takes the 16-byte branch and begin % 4 in {1, 2, 3} the scalar one.
# One chunk per segment; per class of begin % 4 the lengths
#   0                 nothing to sum: the partial is 0, the variable's norm 0
#   1, 2, 3           n < 4: the float4 loop has no trip, the tail loop sums everything
#   4                 one float4, no tail           5, 7     one float4 + a tail of 1 / 3
#   255               n < 256: 63 float4 + tail 3; scalar branch: thread 255 idle
#   256, 257          64 float4 (lanes 64.. idle), tail 0 / 1; scalar branch: one full trip / a second trip of ONE thread
#   1023              255 float4 + tail 3: thread 255 has no float4
#   1024, 1025, 1027  256 float4: one full trip of the float4 loop, tail 0 / 1 / 3; scalar branch: 4 trips (+ 1 / + 3)
# Gaps of 1 to 5 floats between chunks are never touched.
ALIGNMENT_LENGTHS = [0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 1027]
ALIGNMENT_CLASS = {}  # segment id -> (begin % 4, length)


def _alignment():
    items = []
    for mod in range(4):
        for n in ALIGNMENT_LENGTHS:
            ALIGNMENT_CLASS[len(items)] = (mod, n)
            items.append((len(items), mod, n))
    return make_table(place(items))


ALIGNMENT = _alignment()


def alignment_segment(mod, n):
    return next(s for s, c in ALIGNMENT_CLASS.items() if c == (mod, n))


# ------------------------------------------------------------------------------------------------ MANY_CHUNKS
#
# seg_sum_kernel: one wave per segment, lane l sums partial[first + l], [first + l + 64], ...: the `c += 64`
# continuation is the only thing that reaches a variable's chunks past its 64th.
#   1 chunk     lanes 1..63 idle                  63    lane 63 idle
#   64          every lane one chunk, no 2nd trip 65    lane 0 alone takes a second trip
#   128         two full trips                    129   two full trips + lane 0's third (the wrong-scale detector's)
#   200         three full trips + 8 lanes' fourth
# The many-chunk segments alternate with one-chunk segments, so each binary search lands between a long run of equal ids
# and a single one, on either side.  Chunk lengths cycle through 1..9, gaps through 0, 1, 2, 3, 5: the chunks of one
# segment start at every alignment, so both branches of seg_sumsq_kernel feed one sum.
MANY_COUNTS = [63, 1, 64, 1, 65, 1, 128, 1, 129, 1, 200]


def _many_chunks():
    items, k = [], 0
    for seg, count in enumerate(MANY_COUNTS):
        for _ in range(count):
            items.append((seg, None, 1 + k % 9))
            k += 1
    return make_table(place(items, gaps=(0, 1, 2, 3, 5)))


MANY_CHUNKS = _many_chunks()
MANY_SEG_129 = MANY_COUNTS.index(129)

# ------------------------------------------------------------------------------------------------ EMPTY_SEGMENTS
#
# seg_sum_kernel's two binary searches (first chunk with id >= s, first with id > s) for an id that no chunk carries:
# both must land on the same chunk, the sum is over nothing and sumsq[s] is WRITTEN as 0.
#   EMPTY_MIDDLE   ids 0 1 3 4 7 used, n_segments = 10: 2 empty between used ids, 5 and 6 consecutive empties, 8 and 9
#                  past the last chunk (both searches run off the end: lo == n_chunks)
#   EMPTY_FRONT    first used id is 2: ids 0 and 1 search below the first chunk (lo == 0)
#   ONE_CHUNK      n_chunks == 1 (hi == 1: one probe per search), the id of that chunk being 1 of 3
EMPTY_MIDDLE = make_table(place([(0, None, 6), (0, None, 3), (1, None, 300), (3, None, 5), (4, None, 1), (4, None, 0),
                                 (4, None, 9), (7, None, 260), (7, None, 2)]), n_segments=10)
EMPTY_MIDDLE_IDS = [2, 5, 6, 8, 9]
EMPTY_FRONT = make_table(place([(2, None, 7), (2, None, 4), (3, None, 258), (5, None, 3)]), n_segments=6)
EMPTY_FRONT_IDS = [0, 1, 4]
ONE_CHUNK = make_table(place([(1, None, 37)]), n_segments=3)
ONE_CHUNK_IDS = [0, 2]

# ------------------------------------------------------------------------------------------------ LONG_TABLE
#
# 70000 chunks of length 1..3: the searches run 17 probes; segment LONG_SEG holds 40000 chunks = 625 trips of the
# `c += 64` loop for every lane; the other 30000 chunks are spread over 2000 segments of 15.  (One workgroup per chunk:
# 70000 tiny workgroups, a sub-second launch.)
LONG_SEG, LONG_SEG_CHUNKS, LONG_OTHER_SEGS, LONG_OTHER_CHUNKS = 1000, 40000, 2000, 15


def _long_table():
    items, k = [], 0
    for seg in range(LONG_OTHER_SEGS + 1):
        for _ in range(LONG_SEG_CHUNKS if seg == LONG_SEG else LONG_OTHER_CHUNKS):
            items.append((seg, None, 1 + k % 3))
            k += 1
    return make_table(place(items, gaps=(0, 1, 0, 2)))


LONG_TABLE = _long_table()

# ------------------------------------------------------------------------------------------------ FULL_CHUNKS
#
# The trainer's own shape: one variable, 256-byte aligned, three chunks of 16384 floats (16 trips of the float4 loop for
# every thread, no tail) and a last chunk of 5.  Ties this restatement to what tests/test_backward_gpu.py covers.
FULL_CHUNKS = make_table([(0, 64, 16384), (0, 64 + 16384, 16384), (0, 64 + 2 * 16384, 16384), (0, 64 + 3 * 16384, 5)])

# ------------------------------------------------------------------------------------------------ THRESHOLD
#
# The strict `norm > clip` at norm == clip, with clip = 5.  Integer patterns per segment (one chunk each, and two
# patterns once more split over two chunks):
#   (3, 4)  (5, 0, 0)  (0, 0)  (3 | 4)   sumsq <= 25 exactly: NOT scaled, the bits stay
#   (5, 1)  (5 | 1)                      sumsq == 26: scaled by 5 / sqrt(26)
# and the same patterns times 2^-6 with clip = 5 * 2^-6 (sumsq == 25 * 2^-12).  This relies on the device's sqrtf
# returning exactly 5 for 25 (and 5 * 2^-6 for 25 * 2^-12): the library is built with hipcc's default, correctly
# rounded, sqrt and division -- csrc/Makefile has no fast-math flag -- and a correctly rounded sqrt of a perfect
# square is exact.
THRESHOLD_PATTERNS = [((3, 4),), ((5, 0, 0),), ((0, 0),), ((5, 1),), ((3,), (4,)), ((5,), (1,))]
THRESHOLD_SCALED = [3, 5]  # the segments whose norm exceeds 5
THRESHOLD_CLIP = 5.0
THRESHOLD = make_table(place([(s, None, len(c)) for s, pat in enumerate(THRESHOLD_PATTERNS) for c in pat]))

TABLES = {"ALIGNMENT": ALIGNMENT, "MANY_CHUNKS": MANY_CHUNKS, "EMPTY_MIDDLE": EMPTY_MIDDLE, "EMPTY_FRONT": EMPTY_FRONT,
          "ONE_CHUNK": ONE_CHUNK, "LONG_TABLE": LONG_TABLE, "FULL_CHUNKS": FULL_CHUNKS}
EMPTY_IDS = {"EMPTY_MIDDLE": EMPTY_MIDDLE_IDS, "EMPTY_FRONT": EMPTY_FRONT_IDS, "ONE_CHUNK": ONE_CHUNK_IDS}
FUSED_TABLES = ["ALIGNMENT", "MANY_CHUNKS", "EMPTY_MIDDLE", "EMPTY_FRONT", "ONE_CHUNK", "FULL_CHUNKS"]
REAL_TABLES = ["FULL_CHUNKS", "MANY_CHUNKS"]

# clip_norm of the exact cases: with integers in [-8, 8] times 2^-6 a segment of n elements has a norm of about
# 0.077 sqrt(n), so 0.5 is passed from ~40 elements on: every table but the one-variable ones has segments on either side
EXACT_CLIP = 0.5
# the real-valued case, standard_normal * 0.02: norm ~ 0.02 sqrt(n) -- FULL_CHUNKS' variable (49157 elements) ~ 4.4,
# MANY_CHUNKS' segments 0.05 .. 0.65
REAL_CLIP = {"FULL_CHUNKS": 1.0, "MANY_CHUNKS": 0.4}
REAL_MARGIN = 1e-4  # no real-valued norm within this relative distance of the clip: fp32 rounding cannot decide


# ================================================================================================ gradients

def exact_grad(rng, table, gap=GAP_FILL):
    """float32 buffer: integers in [-8, 8] times 2^-6 inside the chunks -- {-1, 0, 1} times 2^-6 in a segment whose
    integer sum of squares could otherwise reach 2^24 (64 per element) -- and `gap` outside every chunk."""
    idx, seg = elements(table)
    count = np.bincount(seg, minlength=table.n_segments)
    wide = rng.integers(-8, 9, idx.size)
    narrow = rng.integers(-1, 2, idx.size)
    ints = np.where(64 * count[seg] >= EXACT_LIMIT, narrow, wide)
    g = np.full(table.size, gap, np.float32)
    g[idx] = (ints * GRAD_UNIT).astype(np.float32)
    return g


def integer_sumsq(g, table):
    """Per segment, the sum of squares of g / 2^-6 as Python-exact integers (int64)."""
    idx, seg = elements(table)
    ints = g[idx].astype(np.float64) / GRAD_UNIT
    assert np.array_equal(ints, np.round(ints)), "not integers times 2^-6"
    return np.bincount(seg, weights=ints * ints, minlength=table.n_segments).astype(np.int64)


def check_exact(g, table):
    """The 2^24 condition: every segment's integer sum of squares is below 2^24, so every partial sum of the squares
    (integers times 2^-12) is exact in fp32 whatever the order."""
    total = integer_sumsq(g, table)
    assert total.max() < EXACT_LIMIT, "segment %d: integer sum of squares %d" % (int(total.argmax()), int(total.max()))
    return total


def real_grad(seed, name, scale=0.02):
    """standard_normal * 0.02 (float32), NaN outside every chunk; redrawn until no segment's float64 norm lies within a
    relative REAL_MARGIN of the clip.  Returns (gradient, the number of draws)."""
    table, clip = TABLES[name], REAL_CLIP[name]
    idx, _ = elements(table)
    for draw in range(1, 9):
        rng = np.random.default_rng([seed, draw])
        g = np.full(table.size, np.nan, np.float32)
        g[idx] = (rng.standard_normal(idx.size) * scale).astype(np.float32)
        norm = np.sqrt(clip_ref(g, table, clip)[0])
        if (np.abs(norm / clip - 1.0) > REAL_MARGIN).all():
            return g, draw
    raise AssertionError("no draw clear of the clip threshold")


def threshold_grad(unit, gap=GAP_FILL):
    """THRESHOLD's patterns times `unit` (1 or 2^-6); the clip is THRESHOLD_CLIP * unit."""
    g = np.full(THRESHOLD.size, gap, np.float32)
    values = [v for pat in THRESHOLD_PATTERNS for c in pat for v in c]
    g[elements(THRESHOLD)[0]] = np.array(values, np.float32) * np.float32(unit)
    return g


# ================================================================================================ error bounds

def sumsq_depth(n, k, aligned):
    """d(n, k): the longest chain of fp32 roundings between a gradient element and its variable's sumsq, read from
    optim.hip as written (a fused multiply-add only shortens it), for a variable of k chunks whose longest chunk has n
    elements:
      seg_sumsq_kernel  1                                      the square
                        4 ceil(n4 / 256) + ceil(tail / 256)    a thread's own chain: four additions per float4 trip
                                                               (n4 = n >> 2, tail = n & 3), one per tail trip; the
                                                               scalar branch of an unaligned chunk: ceil(n / 256)
                        6                                      __shfl_down by 32, 16, 8, 4, 2, 1
                        3                                      scratch[0] + scratch[1] + scratch[2] + scratch[3]
      seg_sum_kernel    ceil(k / 64)                           a lane's chain over the variable's partials
                        6                                      the shuffle steps
    All terms are non-negative, so the relative error of sumsq is at most (1 + u)^d - 1 <= (d + 1) u while d u << 1."""
    if aligned:
        own = 4 * math.ceil((n >> 2) / THREADS) + math.ceil((n & 3) / THREADS)
    else:
        own = math.ceil(n / THREADS)
    return 1 + own + 6 + 3 + math.ceil(k / 64) + 6


def sumsq_bound(table):
    """Per segment: (d + 1) u with d = the deepest chain over the segment's chunks (0 for a segment without chunks)."""
    k = chunks_per_segment(table)
    bound = np.zeros(table.n_segments)
    for s, b, n in zip(table.chunk_seg, table.chunk_begin, table.chunk_len):
        bound[s] = max(bound[s], (sumsq_depth(int(n), int(k[s]), b % 4 == 0) + 1) * U)
    return bound


# clipped gradient, exact gradients: sumsq is exact, then sqrtf, clip / norm and g * scale round once each:
# (1 + u)^3 - 1 < 4 u relative per non-zero element; zeros stay zeros.
CLIP_EXACT_BOUND = 4 * U
# real-valued gradients: sqrt halves the relative error of sumsq -- add half the sumsq bound of the element's segment.

# p, m, v and the moving average against float64: the project's own Adam tolerance
# (test_adam_step_lr_dev_is_adam_step_with_the_rate_in_memory), the clip scale of exact gradients adding at most 4 u
ADAM_RTOL, ADAM_ATOL = 1e-5 + CLIP_EXACT_BOUND, 1e-7


# ================================================================================================ restatements

def clip_ref(g, table, clip):
    """tf.clip_by_norm per segment in float64, by the documented rule: a segment is scaled by clip / norm iff
    norm > clip (strictly); a NaN norm compares false and leaves the segment as it is; an infinite norm scales by 0
    (finite elements become +-0, infinite ones NaN).  Returns (sumsq per segment, clipped g as float64).  Only covered
    elements enter the arithmetic; the others are carried over as they are."""
    idx, seg = elements(table)
    g64 = np.asarray(g, np.float64).copy()
    x = g64[idx]
    with np.errstate(invalid="ignore", over="ignore"):
        sumsq = np.bincount(seg, weights=x * x, minlength=table.n_segments)
        norm = np.sqrt(sumsq)
        scaled = norm > clip
        scale = np.where(scaled, clip / np.where(scaled, norm, 1.0), 1.0)
        g64[idx] = np.where(scaled[seg], x * scale[seg], x)
    return sumsq, g64


def clip_adam_ema_ref(p, m, v, shadow, g, table, clip, lr, b1, b2, eps, step, decay):
    """One fused step in float64: clip_ref (clip > 0) -> adam_ref with grad_scale 1 -> shadow + (1 - decay) (p - shadow)
    (shadow may be None), on the covered elements only.  Returns (p, m, v, shadow, sumsq); sumsq is None without
    clipping."""
    idx, _ = elements(table)
    sumsq, gc = clip_ref(g, table, clip) if clip > 0 else (None, np.asarray(g, np.float64))
    out = [np.asarray(a, np.float64).copy() for a in (p, m, v)]
    with np.errstate(invalid="ignore"):
        pn, mn, vn = adam_ref(out[0][idx], out[1][idx], out[2][idx], gc[idx], lr, b1, b2, eps, step, 1.0)
    for a, new in zip(out, (pn, mn, vn)):
        a[idx] = new
    sh = None
    if shadow is not None:
        sh = np.asarray(shadow, np.float64).copy()
        with np.errstate(invalid="ignore"):
            sh[idx] = sh[idx] + (1.0 - float(np.float32(decay))) * (pn - sh[idx])
    return out[0], out[1], out[2], sh, sumsq


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(gradient, sumsq, clipped gradient) of a table's exact case at EXACT_CLIP: computed once, shared, read-only."""
    table = TABLES[name]
    g = exact_grad(np.random.default_rng(sorted(TABLES).index(name) + 11), table)
    check_exact(g, table)
    sumsq, clipped = clip_ref(g, table, EXACT_CLIP)
    for a in (g, sumsq, clipped):
        a.setflags(write=False)
    return g, sumsq, clipped

// 3x3 SAME convolution of a bilinearly UPSAMPLED map without ever forming the upsampled map: the map decoder's
// conv2_1 and conv3_1 (reference graph monopsr/builders/net_builder.py:72-77 and :81-85 -- tf.image.resize_bilinear
// (align_corners) straight into slim.conv2d 3x3).
//
// Channel mixing commutes with a per-channel spatial operator.  With U = the bilinear upsampling (out pixel q reads four
// source pixels s with weights a[q][s] that depend on q only), tap t = (dy, dx) and g = the (N, 3, 3, C) filter:
//     y[p][n] = bias[n] + sum_t [p + t inside the upsampled image] sum_c g[n][t][c] U(x)[p + t][c]
//             = bias[n] + sum_t [p + t inside]                      sum_s a[p + t][s] z[s][t][n],
//     z[s][t][n] = sum_c g[n][t][c] x[s][c]                 -- a 1x1 convolution of the SOURCE map with 9 N outputs.
// Stage 1 is therefore a plain GEMM [source pixels x C] . [C x 9 N] on the persistent pointwise kernel (pointwise.hip):
// the same 1/4 of the direct form's multiply-adds that F(4x4,3x3) on the upsampled map issues (a quarter of the pixels,
// nine times the columns), but with no input / output transforms, no patch gathers, exact-fp32 GEMM error (1e-6 instead
// of F(4x4)'s 1.5e-5), and the two resize launches (0.9 GB written and re-read per step) are gone.  Stage 2
// (upconv_gather_kernel) is the 9-tap x 4-corner weighted sum above, as a horizontal pass per source row and a vertical
// pass per output row (a[q][s] is a product of a row and a column weight): one workgroup per (image, 8-channel block)
// rolls the source rows through LDS and a thread sums 6 float4 per pass item for 4 channels -- LDS / vector-ALU work on
// 1/9 of the GEMM's flops, reading z once and writing the layer's output once (channel-blocked for the F(4x4,3x3) layer
// that follows, or NHWC).
//
// Column order of z (ours to choose): j = (n / 8) * 72 + t * 8 + (n % 8) -- the nine taps of an 8-channel block are 288
// contiguous bytes per source pixel.  The GEMM's weight matrix W'[j][c] = g[n][t][c] is a re-ordering of the filter
// rows (upconv_weights_kernel; kept in the caller's filter cache when there is one).  9 N columns are cut into parts of
// 1152 = 9 column blocks of the pointwise kernel (its persistent grid then fills the chip: 504 of 512 workgroup slots),
// i.e. one part per 128 output channels.
#include <atomic>

#include "common.h"

namespace {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int PART = 1152;  // z columns per GEMM launch = 16 channel blocks x 9 taps x 8 channels
constexpr size_t kGatherLdsBytes = 80 * 1024;  // most LDS a gather workgroup takes (two per CU)

// W'[j][c] = g[n][t*C + c], j = (n / 8) * 72 + t * 8 + (n % 8).  One thread per float4 of W'.
__global__ __launch_bounds__(256) void upconv_weights_kernel(const float *__restrict__ g, int N, int C, float *__restrict__ wp)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C / 4;
    if (i >= (long long)9 * N * c4) return;
    const int j = (int)(i / c4), q = (int)(i - (long long)j * c4);
    const int blk = j / 72, r = j - blk * 72, t = r >> 3, n = blk * 8 + (r & 7);
    reinterpret_cast<float4 *>(wp)[i] = reinterpret_cast<const float4 *>(g + ((size_t)n * 9 + t) * C)[q];
}

struct UpcParams {
    const float *z, *bias;
    float *y;
    size_t part_stride;  // floats between the z parts (source pixels x 1152)
    int B, h, w, H, W, N, relu;
    int RB, cap, stg;    // output rows per band; source rows the Hrow ring holds (>= the rows one band reaches); z rows staged at once
    mpsr::FastDiv capdiv;  // r % cap by multiply-high (common.h)
    float hscale, wscale;
};

// float4 registers per thread that carry source pixels on their way into LDS (8 of them cost the kernel its fifth wave
// per SIMD, i.e. the third workgroup per CU: 118 against 92 vector registers)
constexpr int kPf = 4;
std::atomic<int> g_upconv_band{0};  // mpsr_debug_set_upconv_band: output rows per band of the rolling window (0 = 8)

// One workgroup per (8-channel block, image) walks the image in bands of RB output rows.  The 9-tap x 4-corner sum is
// done in two passes (the bilinear weights are a product of a row and a column weight):
//     Hrow[r][dy][x] = sum_dx sum_c wx[dx][c] z[r][col(x + dx, c)][(dy, dx)]      -- once per SOURCE row r: 6 LDS reads
//     y[Y][x]        = bias + sum_dy sum_a wy[dy][a] Hrow[row(Y + dy, a)][dy][x]   -- once per output row:  6 LDS reads
// (about h 18 + H 6 float4 reads per output column instead of H 36: the one-pass form sat at the LDS pipe's rate).  LDS is
// a ring of `cap` Hrow rows, [row % cap][dy][column][half of the 8 channels], next to a staging area for the z rows a band
// ADDS, [row][column][tap][8 channels], at most `stg` rows at a time: while a chunk of rows is summed the next chunk is
// already on its way into registers, and moves into the staging area between two barriers -- every z row is read exactly
// once and its horizontal pass runs once.  Two things measured on the way (r04): an integer division costs hipcc ~35
// vector instructions, so nothing in the loops divides by a run-time value: thread = (row of a pass, output column x, half
// of the 8 channels) with blockDim.x = rpp * 2 W (a thread's column, its three tap columns, their LDS offsets and weights
// never change) and, as a loader, (pixel group, 16-byte piece of a pixel's 288 bytes) walking pixels by addition.  And a
// load -> LDS-store loop waits for every load in turn: loads are issued kPf at a time into registers, then stored.
// WIDE: a z row is wider than the prefetch registers (gather_geometry then stages ONE row per chunk): loaded in rounds,
// nothing requested ahead.  (A template parameter: as a run-time branch it cost the kernel 8 vector registers, and with
// them its fifth wave per SIMD.)
template <bool OUT_C8, bool WIDE = false>
__global__ __launch_bounds__(512) void upconv_gather_kernel(const UpcParams p)
{
    extern __shared__ __attribute__((aligned(16))) float4 lds4[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    // Workgroup i runs on XCD i % 8 (speed only): XCD x takes the images x, x + 8, ... and the N / 8 channel blocks of an
    // image back to back.  A block's 288-byte slice of a pixel straddles cache lines it shares with its neighbours, and
    // an image's z slab (0.7 - 2.7 MB) is read by all its blocks: one L2 then fetches every line once (with the blocks
    // of an image spread over the eight L2s the same bytes came in 1.44 times).
    const int nblk = p.N >> 3;
    const int xcd = blockIdx.x & 7, jx = blockIdx.x >> 3;
    const int bq = jx / nblk, blk = jx - bq * nblk, b = bq * 8 + xcd;
    if (b >= p.B) return;  // block-uniform
    const int lpr = 2 * p.W, rpp = nthr / lpr;
    const int rr = tid / lpr, l = tid - rr * lpr, x = l >> 1, half = l & 1;
    const int n0 = blk * 8;
    const int rowf4 = p.w * 18;  // float4 per staged z row
    const int hrow4 = 3 * lpr;   // float4 per Hrow row
    float4 *hr = lds4;                               // ring  [cap][3][W][2]
    float4 *zs = lds4 + (size_t)p.cap * hrow4;       // stage [stg][w][18]
    auto slot = [&](int r) __attribute__((always_inline)) { return r - p.cap * mpsr::fdiv(r, p.capdiv); };  // r % cap
    const float *zp = p.z + (size_t)(blk >> 4) * p.part_stride + (size_t)(blk & 15) * 72 + (size_t)b * p.h * p.w * PART;
    // loader role: piece `lpiece` of the pixels lgrp, lgrp + lgroups, ... of a chunk of whole rows (row-major, rows are
    // contiguous in z); (lrow0, lcol0) = this thread's first pixel, (drow, dcol) = the step of lgroups pixels
    const int lgroups = nthr / 18, lgrp = tid / 18, lpiece = tid - lgrp * 18;
    const bool loader = lgrp < lgroups;
    const int lrow0 = lgrp / p.w, lcol0 = lgrp - lrow0 * p.w;
    const int drow = lgroups / p.w, dcol = lgroups - drow * p.w;
    f32x4 pf[kPf];
    // pixels [first, first + kPf * lgroups) of the chunk of rows that starts at row ra, npix pixels long
    auto issue = [&](int ra, int npix, int first) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            // (an unconditional load through a selected address -- unused slots re-read one cached line; a conditional
            // load, or HIP's float4 struct as the element type, sends the register array to scratch memory)
            const int pix = first + lgrp + j * lgroups;
            const bool live = loader && pix < npix;
            pf[j] = *reinterpret_cast<const f32x4 *>(live ? zp + ((size_t)ra * p.w + pix) * PART + 4 * lpiece : zp);
        }
    };
    // a chunk that fits the registers (npix <= kPf * lgroups), rows and columns walked by addition
    auto commit = [&](int npix) __attribute__((always_inline)) {
        int row = lrow0, col = lcol0;
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            const int pix = lgrp + j * lgroups;
            if (loader && pix < npix) reinterpret_cast<f32x4 *>(zs)[row * rowf4 + col * 18 + lpiece] = pf[j];
            row += drow;
            col += dcol;
            if (col >= p.w) {
                col -= p.w;
                ++row;
            }
        }
    };

    // one round of a single staged row: pixel = column
    auto commit_row = [&](int npix, int first) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kPf; ++j) {
            const int pix = first + lgrp + j * lgroups;
            if (loader && pix < npix) reinterpret_cast<f32x4 *>(zs)[pix * 18 + lpiece] = pf[j];
        }
    };
    constexpr bool wide = WIDE;

    // last source row band k's taps (output rows k RB - 1 .. (k + 1) RB, clamped) interpolate from
    auto band_hi = [&](int k) __attribute__((always_inline)) {
        const int yl = min(k * p.RB + p.RB, p.H) - 1;
        return min((int)floorf((float)min(yl + 1, p.H - 1) * p.hscale) + 1, p.h - 1);
    };
    // tap column d - 1 of this thread's output column: staging offsets of the two source columns (tap column and channel
    // half folded in) and their weights (zero when the tap falls outside the upsampled image: the convolution's SAME
    // padding)
    int co[3][2];
    float wx[3][2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int qx = x + d - 1;
        const bool vx = qx >= 0 && qx < p.W;
        const float sx = (float)min(max(qx, 0), p.W - 1) * p.wscale;
        const int c0 = (int)floorf(sx), c1 = min(c0 + 1, p.w - 1);
        const float lx = sx - (float)c0;
        co[d][0] = c0 * 18 + 2 * d + half;
        co[d][1] = c1 * 18 + 2 * d + half;
        wx[d][0] = vx ? 1.f - lx : 0.f;
        wx[d][1] = vx ? lx : 0.f;
    }
    const float4 bias4 = p.bias ? *reinterpret_cast<const float4 *>(p.bias + n0 + 4 * half) : make_float4(0.f, 0.f, 0.f, 0.f);

    const int nbands = (p.H + p.RB - 1) / p.RB;
    int have = -1;  // last source row whose Hrow is in the ring
    int pn = wide ? 0 : min(band_hi(0) + 1, p.stg);  // rows of the chunk on its way: (have, have + pn]
    if (pn > 0) issue(0, pn * p.w, 0);
    // Every item stores its result at once.  (Holding a band's results in registers until the next rows are committed,
    // so that the stores no longer share a wait with the prefetch loads, measured slower on the one-pass form: 243 vs
    // 176 us on conv2_1 -- DESIGN.md 4.1 (h).)
    for (int k = 0; k < nbands; ++k) {
        const int bhi = band_hi(k);
        while (have < bhi) {  // block-uniform
            if (wide) {
                for (int first = 0; first < p.w; first += kPf * lgroups) {
                    issue(have + 1, p.w, first);
                    commit_row(p.w, first);
                }
                pn = 1;
            } else {
                if (pn == 0) {  // (a band before this one added no rows: nothing was requested ahead)
                    pn = min(bhi - have, p.stg);
                    issue(have + 1, pn * p.w, 0);
                }
                commit(pn * p.w);
            }
            __syncthreads();  // the chunk is staged; every read of the ring for the previous band is done
            const int c0 = have + 1, cn = pn;
            have += pn;
            // the chunk after this one: the rest of this band's rows, or the first rows the next band adds
            const int tgt = (have < bhi || k + 1 == nbands) ? bhi : band_hi(k + 1);
            pn = wide ? 0 : min(tgt - have, p.stg);
            if (pn > 0) issue(have + 1, pn * p.w, 0);
            // horizontal pass: item = (staged row, tap row) of this thread's column
            for (int q = rr; q < 3 * cn; q += rpp) {
                const int rl = q / 3, dy = q - 3 * rl;
                const float4 *zr = zs + rl * rowf4 + 6 * dy;
                f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
#pragma unroll
                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                    for (int c = 0; c < 2; ++c) {
                        const float4 v = zr[co[dx][c]];
                        const f32x2 w2 = {wx[dx][c], wx[dx][c]};
                        a01 = __builtin_elementwise_fma(w2, f32x2{v.x, v.y}, a01);
                        a23 = __builtin_elementwise_fma(w2, f32x2{v.z, v.w}, a23);
                    }
                hr[(slot(c0 + rl) * 3 + dy) * lpr + l] = make_float4(a01.x, a01.y, a23.x, a23.y);
            }
            __syncthreads();  // the chunk's Hrow rows are in the ring; the staging area may be overwritten
        }
        // vertical pass: the band's output rows
        const int y0 = k * p.RB, ylast = min(y0 + p.RB, p.H) - 1;
        for (int y = y0 + rr; y <= ylast; y += rpp) {
            int ro[3][2];
            float wy[3][2];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int qy = y + d - 1;
                const bool vy = qy >= 0 && qy < p.H;
                const float sy = (float)min(max(qy, 0), p.H - 1) * p.hscale;
                const int r0 = (int)floorf(sy), r1 = min(r0 + 1, p.h - 1);
                const float ly = sy - (float)r0;
                ro[d][0] = (slot(r0) * 3 + d) * lpr + l;
                ro[d][1] = (slot(r1) * 3 + d) * lpr + l;
                wy[d][0] = vy ? 1.f - ly : 0.f;
                wy[d][1] = vy ? ly : 0.f;
            }
            f32x2 a01 = {bias4.x, bias4.y}, a23 = {bias4.z, bias4.w};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    const float4 v = hr[ro[dy][a]];
                    const f32x2 w2 = {wy[dy][a], wy[dy][a]};
                    a01 = __builtin_elementwise_fma(w2, f32x2{v.x, v.y}, a01);
                    a23 = __builtin_elementwise_fma(w2, f32x2{v.z, v.w}, a23);
                }
            float4 acc = make_float4(a01.x, a01.y, a23.x, a23.y);
            if (p.relu) {
                acc.x = fmaxf(acc.x, 0.f);
                acc.y = fmaxf(acc.y, 0.f);
                acc.z = fmaxf(acc.z, 0.f);
                acc.w = fmaxf(acc.w, 0.f);
            }
            float *o = OUT_C8 ? p.y + ((((size_t)b * (p.N / 8) + blk) * p.H + y) * p.W + x) * 8 + 4 * half
                              : p.y + (((size_t)b * p.H + y) * p.W + x) * p.N + n0 + 4 * half;
            *reinterpret_cast<float4 *>(o) = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// dz = gather^T(dy): dz[s][t][n] = sum over the upsampled pixels q that interpolate from source pixel s of
// a[q][s] * dy[q - t][n] (q - t inside the output) -- the transpose of upconv_gather_kernel, written as a gather so that
// nothing is scattered and the sum order is fixed.  One workgroup per (32-channel group, source row, image): the dy rows
// that source row reaches (the upsampled rows that interpolate from it, one more on each side for the taps) sit in LDS
// as [row][x][32 channels] -- 128 contiguous bytes per pixel of the NHWC gradient, whole lines (a first version with one
// workgroup per (image, 8-channel block) read 32 of every 128 bytes and took 1.06 ms on conv3_1) -- next to the
// (upsampled index, weight) pairs of this source row and of every source column.  Item = (source column, tap, channel quad).
constexpr int kGtMax = 8;  // most upsampled rows (columns) that interpolate from one source row (column)
constexpr int kGtPf = 6;   // float4 registers per thread that carry the rows a step adds on their way into the ring
constexpr int kGtItemsA = 6, kGtItemsB = 8;  // most items per thread of the two passes of a step (3 W 8 / 256, 72 w / 256)

struct UpcGradParams {
    const float *dy;
    float *dz;
    int B, h, w, H, W, N, rows_max, cap;  // cap: rows of the ring, a power of two >= rows_max
    float hscale, wscale;
};

// One workgroup per (32-channel group, image) WALKS the source rows: the dy rows a source row reaches (the upsampled rows
// that interpolate from it, one more on each side for the taps) live in a ring of `cap` rows in LDS, [row][x][32 channels]
// = whole 128-byte lines of the NHWC gradient; a step adds the (about `scale`) rows its successor needs -- requested into
// registers before the step's arithmetic, written to the ring after it -- so every dy row is fetched ONCE (the first form,
// one workgroup per source row, fetched each ~3.5 times and waited for its whole window in front of 4 us of arithmetic:
// 0.58 ms on conv3_1; r04).  Per step, separable: V[dy][x] = sum_ky wy[ky] dy[yq[ky] - dy][x] for the three tap rows, then
// dz[sy][sx][t] = sum_kx wx[kx] V[dy(t)][xq[kx] - dx(t)].  The (index, weight) tables of every source row and column are
// made once per workgroup by the forward kernel's own arithmetic.
__global__ __launch_bounds__(256) void upconv_gather_t_kernel(const UpcGradParams p)
{
    extern __shared__ __attribute__((aligned(16))) float4 g4[];  // ring [cap][W][8] | V [3][W][8] | tables
    const int tid = threadIdx.x;
    const int grp = blockIdx.x, b = blockIdx.y;
    const int rowq = p.W * 8;  // float4 per dy row of this channel group
    float4 *V = g4 + (size_t)p.cap * rowq;
    int *xq = reinterpret_cast<int *>(V + (size_t)3 * rowq);  // [w][kGtMax]
    float *xw = reinterpret_cast<float *>(xq + p.w * kGtMax);
    int *xc = reinterpret_cast<int *>(xw + p.w * kGtMax);     // [w]
    int *yq = xc + ((p.w + 3) & ~3);                           // [h][kGtMax] (16-byte aligned: read as int4)
    float *yw = reinterpret_cast<float *>(yq + p.h * kGtMax);
    int *yc = reinterpret_cast<int *>(yw + p.h * kGtMax);     // [h]
    int *ylo = yc + p.h, *yhi = ylo + p.h;                     // [h]: first / last dy row a source row reaches
    // (upsampled index, weight) pairs: q interpolates from s iff floor(q scale) is s - 1 or s -- only q in
    // [(s - 1) / scale, (s + 1) / scale] need a look.  Thread t < h: source row t; h <= t < h + w: source column t - h.
    for (int t = tid; t < p.h + p.w; t += 256) {
        const bool row = t < p.h;
        const int sv = row ? t : t - p.h, n_in = row ? p.h : p.w, n_out = row ? p.H : p.W;
        const float scale = row ? p.hscale : p.wscale;
        const int q_lo = max((int)floorf((float)(sv - 1) / scale) - 1, 0), q_hi = min((int)ceilf((float)(sv + 1) / scale) + 1, n_out - 1);
        int *oq = row ? yq + sv * kGtMax : xq + sv * kGtMax;
        float *ow = row ? yw + sv * kGtMax : xw + sv * kGtMax;
        int c = 0, lo = n_out, hi = -1;
        for (int q = q_lo; q <= q_hi; ++q) {
            const float sq = (float)q * scale;
            const int r0 = (int)floorf(sq), r1 = min(r0 + 1, n_in - 1);
            const float l = sq - (float)r0;
            if ((r0 == sv || r1 == sv) && c < kGtMax) {
                oq[c] = q;
                ow[c] = (r0 == sv ? 1.f - l : 0.f) + (r1 == sv ? l : 0.f);
                ++c;
                lo = min(lo, q);
                hi = max(hi, q);
            }
        }
        if (row) {
            yc[sv] = c;
            ylo[sv] = c ? max(lo - 1, 0) : 0;
            yhi[sv] = c ? min(hi + 1, p.H - 1) : -1;
        } else {
            xc[sv] = c;
        }
    }
    __syncthreads();
    const float *src = p.dy + ((size_t)b * p.H * p.W) * p.N + grp * 32;  // this image, this channel group
    const int mask = p.cap - 1;
    f32x4 pf[kGtPf];
    // rows [r0, r1] of dy: requests into the registers (items tid, tid + 256, ...), then the ring
    auto request = [&](int r0, int r1) __attribute__((always_inline)) {
        const int total = (r1 - r0 + 1) * rowq;
#pragma unroll
        for (int j = 0; j < kGtPf; ++j) {
            const int i = j * 256 + tid;
            const int r = r0 + i / rowq, c = i - (i / rowq) * rowq;
            pf[j] = *reinterpret_cast<const f32x4 *>(i < total ? src + ((size_t)r * p.W + (c >> 3)) * p.N + 4 * (c & 7) : src);
        }
    };
    auto commit = [&](int r0, int r1) __attribute__((always_inline)) {
        const int total = (r1 - r0 + 1) * rowq;
#pragma unroll
        for (int j = 0; j < kGtPf; ++j) {
            const int i = j * 256 + tid;
            const int r = r0 + i / rowq, c = i - (i / rowq) * rowq;
            if (i < total) reinterpret_cast<f32x4 *>(g4)[(size_t)(r & mask) * rowq + c] = pf[j];
        }
    };
    // the first source row's window, kGtPf * 256 float4 at a time
    int have = -1;  // last dy row in the ring
    {
        int hi0 = -1;
        for (int sy = 0; sy < p.h && hi0 < 0; ++sy) hi0 = yhi[sy];  // (a source row that nothing interpolates from has no window)
        const int lo0 = 0;
        const int rows_per = max(1, (kGtPf * 256) / rowq);
        for (int r = lo0; r <= hi0; r += rows_per) {
            const int re = min(hi0, r + rows_per - 1);
            request(r, re);
            commit(r, re);
        }
        have = hi0;
    }
    __syncthreads();
    float *dzimg = p.dz + ((size_t)b * p.h * p.w) * 9 * p.N + (size_t)grp * 4 * 72;
    // a thread's items are the same for every source row: decoded once (the divisions were a third of the kernel's
    // instructions -- it is bound by its vector instructions, not by memory)
    int a_d[kGtItemsA], a_r[kGtItemsA];
#pragma unroll
    for (int k = 0; k < kGtItemsA; ++k) {
        const int it = tid + 256 * k;
        a_d[k] = it < 3 * rowq ? it / rowq : -1;
        a_r[k] = it - max(a_d[k], 0) * rowq;  // x * 8 + quad
    }
    int b_sx[kGtItemsB], b_v[kGtItemsB], b_dx[kGtItemsB], b_out[kGtItemsB];
#pragma unroll
    for (int k = 0; k < kGtItemsB; ++k) {
        const int it = tid + 256 * k;
        // (m = the float4's place in the 1152 contiguous bytes of (source pixel, channel group): consecutive lanes
        // write consecutive pieces -- a wave's store is eight whole lines)
        const int sx = it / 72, m = it - sx * 72, blk = m / 18, rem = m - 18 * blk, t = rem >> 1, quad = 2 * blk + (rem & 1);
        const int d = t / 3;
        b_sx[k] = it < p.w * 72 ? sx : -1;
        b_v[k] = d * rowq + quad;
        b_dx[k] = t - d * 3 - 1;
        b_out[k] = sx * 9 * p.N + 4 * m;
    }
    for (int sy = 0; sy < p.h; ++sy) {
        // the rows the NEXT source row adds: requested now, in the ring after this row's arithmetic
        const int next_hi = sy + 1 < p.h ? max(yhi[sy + 1], have) : have;
        const bool more = next_hi > have;
        if (more) request(have + 1, next_hi);
        // (the first four (index, weight) pairs of a row / column as one 16-byte read each and branch-free -- a pair
        // that does not apply gets weight 0 and a clamped address --, so that an item is two LDS round trips deep
        // instead of two per pair: the kernel was bound by those dependent reads at two waves per SIMD)
        const int ny = yc[sy];
        const int4 yq4 = *reinterpret_cast<const int4 *>(yq + sy * kGtMax);
        const float4 yw4 = *reinterpret_cast<const float4 *>(yw + sy * kGtMax);
#pragma unroll
        for (int k = 0; k < kGtItemsA; ++k) {
            const int d = a_d[k], r = a_r[k], it = tid + 256 * k;
            if (d < 0) continue;
            const int py0 = yq4.x - (d - 1), py1 = yq4.y - (d - 1), py2 = yq4.z - (d - 1), py3 = yq4.w - (d - 1);
            const float w0 = (ny > 0 && py0 >= 0 && py0 < p.H) ? yw4.x : 0.f, w1 = (ny > 1 && py1 >= 0 && py1 < p.H) ? yw4.y : 0.f;
            const float w2 = (ny > 2 && py2 >= 0 && py2 < p.H) ? yw4.z : 0.f, w3 = (ny > 3 && py3 >= 0 && py3 < p.H) ? yw4.w : 0.f;
            const float4 v0 = g4[(size_t)(py0 & mask) * rowq + r], v1 = g4[(size_t)(py1 & mask) * rowq + r];
            const float4 v2 = g4[(size_t)(py2 & mask) * rowq + r], v3 = g4[(size_t)(py3 & mask) * rowq + r];
            f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
            auto acc = [&](float wv, const float4 &v) __attribute__((always_inline)) {
                const f32x2 w2_ = {wv, wv};
                a01 = __builtin_elementwise_fma(w2_, f32x2{v.x, v.y}, a01);
                a23 = __builtin_elementwise_fma(w2_, f32x2{v.z, v.w}, a23);
            };
            // (a slot whose weight is 0 may hold anything, NaN included: select, do not multiply)
            if (w0 != 0.f) acc(w0, v0);
            if (w1 != 0.f) acc(w1, v1);
            if (w2 != 0.f) acc(w2, v2);
            if (w3 != 0.f) acc(w3, v3);
            for (int ky = 4; ky < ny; ++ky) {
                const int py = yq[sy * kGtMax + ky] - (d - 1);
                if (py < 0 || py >= p.H) continue;
                acc(yw[sy * kGtMax + ky], g4[(size_t)(py & mask) * rowq + r]);
            }
            V[it] = make_float4(a01.x, a01.y, a23.x, a23.y);
        }
        __syncthreads();  // V complete; every read of the ring for this source row is done
        float *dzrow = dzimg + (size_t)sy * p.w * 9 * p.N;
#pragma unroll
        for (int k = 0; k < kGtItemsB; ++k) {  // item = (source column, tap, channel quad)
            const int sx = b_sx[k], dx = b_dx[k];
            if (sx < 0) continue;
            const int nx = xc[sx];
            const int4 q4 = *reinterpret_cast<const int4 *>(xq + sx * kGtMax);
            const float4 w4 = *reinterpret_cast<const float4 *>(xw + sx * kGtMax);
            const float4 *row = V + b_v[k];
            const int px0 = q4.x - dx, px1 = q4.y - dx, px2 = q4.z - dx, px3 = q4.w - dx;
            const bool ok0 = nx > 0 && px0 >= 0 && px0 < p.W, ok1 = nx > 1 && px1 >= 0 && px1 < p.W;
            const bool ok2 = nx > 2 && px2 >= 0 && px2 < p.W, ok3 = nx > 3 && px3 >= 0 && px3 < p.W;
            const float4 v0 = row[(ok0 ? px0 : 0) * 8], v1 = row[(ok1 ? px1 : 0) * 8];
            const float4 v2 = row[(ok2 ? px2 : 0) * 8], v3 = row[(ok3 ? px3 : 0) * 8];
            f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
            auto acc = [&](float wv, const float4 &v) __attribute__((always_inline)) {
                const f32x2 w2_ = {wv, wv};
                a01 = __builtin_elementwise_fma(w2_, f32x2{v.x, v.y}, a01);
                a23 = __builtin_elementwise_fma(w2_, f32x2{v.z, v.w}, a23);
            };
            if (ok0) acc(w4.x, v0);
            if (ok1) acc(w4.y, v1);
            if (ok2) acc(w4.z, v2);
            if (ok3) acc(w4.w, v3);
            for (int kx = 4; kx < nx; ++kx) {
                const int px = xq[sx * kGtMax + kx] - dx;
                if (px < 0 || px >= p.W) continue;
                acc(xw[sx * kGtMax + kx], row[px * 8]);
            }
            *reinterpret_cast<float4 *>(dzrow + b_out[k]) = make_float4(a01.x, a01.y, a23.x, a23.y);
        }
        // (as late as possible: the requests have had the whole step to land; overwrites rows below the next window --
        // cap >= the widest window -- that nobody reads any more since the barrier above)
        if (more) commit(have + 1, next_hi);
        have = next_hi;
        __syncthreads();  // the ring holds the next window; V may be overwritten
    }
}

// wt[c][j] = g[n][t*C + c], j = (n / 8) * 72 + t * 8 + (n % 8): the (C, 9 N) weight matrix of the data-gradient GEMM
__global__ __launch_bounds__(256) void upconv_weights_t_kernel(const float *__restrict__ g, int N, int C, float *__restrict__ wt)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int K = 9 * N;
    if (i >= (long long)C * K) return;
    const int c = (int)(i / K), j = (int)(i - (long long)c * K);
    const int blk = j / 72, r = j - blk * 72, t = r >> 3, n = blk * 8 + (r & 7);
    wt[i] = g[((size_t)n * 9 + t) * C + c];
}

// dw[n][t*C + c] += dwp[j][c]: folds the tap GEMM's weight gradient back into the filter's layout
__global__ __launch_bounds__(256) void upconv_fold_dw_kernel(const float *__restrict__ dwp, int N, int C, float *__restrict__ dw)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C / 4;
    if (i >= (long long)9 * N * c4) return;
    const int j = (int)(i / c4), q = (int)(i - (long long)j * c4);
    const int blk = j / 72, r = j - blk * 72, t = r >> 3, n = blk * 8 + (r & 7);
    float4 *d = reinterpret_cast<float4 *>(dw + ((size_t)n * 9 + t) * C) + q;
    const float4 a = *d, v = reinterpret_cast<const float4 *>(dwp)[i];
    *d = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w);
}

// Launch geometry of the gather: threads = rpp x 2 W (rows of a pass x (column, channel half)), rpp a power of two with
// at most 512 threads; RB = output rows per band (8, or rpp if larger); cap = the Hrow ring's rows >= the rows any band
// reaches; stage = the z rows staged at once (a band's new rows travel through the prefetch registers in chunks of that
// many).  false: the map is too wide for this kernel.
bool gather_geometry(int h, int w, int H, int W, float hscale, int *threads, int *RB, int *cap, int *stage)
{
    if (2 * W > 512 || w < 1) return false;
    int rpp = 1;
    while (rpp * 2 <= 16 && rpp * 2 * 2 * W <= 512) rpp *= 2;
    const int nthr = rpp * 2 * W;
    if (nthr < 18) return false;
    // a map whose source rows all fit a third of the LDS is ONE band (its Hrow rows all stay in the ring); otherwise bands
    // of 8 rows (or one pass) with the next band's rows prefetched
    int rb = rpp > 8 ? rpp : 8;
    if (g_upconv_band.load() > 0) {  // (tuning knob: bands of this many rows, also where one band would do)
        rb = (g_upconv_band.load() + rpp - 1) / rpp * rpp;
    } else if ((size_t)h * w * 288 <= kGatherLdsBytes * 3 / 5) {
        rb = (H + rpp - 1) / rpp * rpp;
    }
    // the kernel's own band arithmetic: the most rows a band reaches, the most a band adds (the first: all it reaches)
    int rows = 0, add = 0, first = 0, prev_hi = -1;
    for (int k = 0; k * rb < H; ++k) {
        const int y0 = k * rb, yl = (y0 + rb < H ? y0 + rb : H) - 1;
        const int lo = (int)floorf((float)(y0 - 1 > 0 ? y0 - 1 : 0) * hscale);
        int hi = (int)floorf((float)(yl + 1 < H - 1 ? yl + 1 : H - 1) * hscale) + 1;
        if (hi > h - 1) hi = h - 1;
        if (hi - lo + 1 > rows) rows = hi - lo + 1;
        if (k > 0 && hi - prev_hi > add) add = hi - prev_hi;
        if (k == 0) first = hi + 1;
        prev_hi = hi;
    }
    // whole rows the prefetch registers carry (none: a wide row is staged alone, in rounds)
    const int per_chunk = kPf * (nthr / 18) / w > 1 ? kPf * (nthr / 18) / w : 1;
    // (the envelope stays inside the one-pass form's -- the decoder's plans are written against it: the rows a band
    // reaches fit the LDS budget as z rows, the rows a band adds fit 8 float4 per loader thread.  What it loses: maps
    // whose Hrow ring is too large, below -- an Hrow row outgrows its z row beyond a 3x upscale in width)
    if ((size_t)rows * w * 288 > kGatherLdsBytes || add * w > 8 * (nthr / 18)) return false;
    // three workgroups per CU (3/5 of the two-per-CU budget each) where the ring and one staged row leave room for it
    const size_t ring = (size_t)rows * 3 * W * 32, zrow = (size_t)w * 288;
    const size_t budget = ring + zrow <= kGatherLdsBytes * 3 / 5 ? kGatherLdsBytes * 3 / 5 : kGatherLdsBytes;
    int stg = first > add ? first : add;
    if (stg > per_chunk) stg = per_chunk;
    while (stg > 1 && ring + stg * zrow > budget) --stg;
    if (ring + stg * zrow > kGatherLdsBytes) return false;
    *threads = nthr;
    *RB = rb;
    *cap = rows;
    *stage = stg;
    return true;
}

}  // namespace

// images per GEMM + gather round, as MB of z (0 = the whole batch at once); see conv3x3_upsampled
static std::atomic<int> g_upconv_chunk_mb{0};
extern "C" void mpsr_debug_set_upconv_chunk_mb(int mb) { g_upconv_chunk_mb = mb > 0 ? mb : 0; }
extern "C" void mpsr_debug_set_upconv_band(int rows) { g_upconv_band = rows > 0 ? rows : 0; }

namespace mpsr {

static bool upconv_geometry_ok(int h, int w, int OH, int OW, int align_corners)
{
    int t, rb, cap, stg;
    const float hs = (align_corners && OH > 1) ? (float)(h - 1) / (float)(OH - 1) : (float)h / (float)OH;
    return gather_geometry(h, w, OH, OW, hs, &t, &rb, &cap, &stg);
}

size_t upconv_weight_floats(int C, int N) { return (size_t)9 * N * C; }
size_t upconv_z_floats(long long Msrc, int N) { return (size_t)Msrc * 9 * (size_t)N; }

// x (B,h,w,C) NHWC, 3x3 filter (N, 9 C), output (B,OH,OW,N): N a multiple of 128 (whole GEMM parts), the source map a
// shape the pointwise kernel takes, 32-bit byte offsets inside z parts
bool upconv_applies(int B, int h, int w, int C, int OH, int OW, int N, int align_corners)
{
    const long long M = (long long)B * h * w;
    return B > 0 && h >= 1 && w >= 1 && OH >= 1 && OW >= 1 && N >= 128 && N % 128 == 0 && C % 4 == 0 &&
           pointwise_applies(M, C, PART) && upconv_geometry_ok(h, w, OH, OW, align_corners) && B <= 65535 &&
           (long long)B * OH * OW * N * 4 < 0x7fffffffffLL;
}

int conv3x3_upsampled(const float *x, int B, int h, int w, int C, int OH, int OW, int align_corners, const float *g,
                      const float *bias, int relu, float *y, int N, int out_c8, float *z, size_t z_floats, float *ws,
                      size_t ws_floats, hipStream_t s, LayerExtras *ex)
{
    MPSR_REQUIRE(upconv_applies(B, h, w, C, OH, OW, N, align_corners), "conv3x3_upsampled: unsupported shape (B=%d %dx%dx%d -> %dx%dx%d)",
                 B, h, w, C, OH, OW, N);
    const long long M = (long long)B * h * w;
    if (!z || z_floats < upconv_z_floats(M, N))
        return fail(MPSR_ERR_WORKSPACE, "conv3x3_upsampled: z scratch holds %zu floats, needs %zu", z_floats,
                    upconv_z_floats(M, N));
    // re-ordered filter rows: in the caller's filter cache if it has a slice for this layer, else in `ws`, which must
    // then hold them
    const FilterPlace f = place_filters(ex, g, upconv_weight_floats(C, N), FILTER_FORM_UPCONV, ws, ws_floats);
    float *wp = f.u;
    if (wp == ws && (!ws || ws_floats < upconv_weight_floats(C, N)))
        return fail(MPSR_ERR_WORKSPACE, "conv3x3_upsampled: scratch holds %zu floats, needs %zu", ws_floats,
                    upconv_weight_floats(C, N));
    if (!f.ready) {
        const long long total = (long long)9 * N * (C / 4);
        hipLaunchKernelGGL(upconv_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, N, C, wp);
        MPSR_CHECK_LAUNCH("upconv_weights_kernel");
    }
    const int parts = N / 128;
    UpcParams p;
    p.bias = bias;
    p.part_stride = (size_t)M * PART;
    p.h = h; p.w = w; p.H = OH; p.W = OW; p.N = N; p.relu = relu;
    p.hscale = (align_corners && OH > 1) ? (float)(h - 1) / (float)(OH - 1) : (float)h / (float)OH;
    p.wscale = (align_corners && OW > 1) ? (float)(w - 1) / (float)(OW - 1) : (float)w / (float)OW;
    int threads = 0;
    if (!gather_geometry(h, w, OH, OW, p.hscale, &threads, &p.RB, &p.cap, &p.stg))
        return fail(MPSR_ERR_UNSUPPORTED, "conv3x3_upsampled: no gather geometry for a %dx%d -> %dx%d map", h, w, OH, OW);
    p.capdiv = make_fastdiv(p.cap);
    const size_t lds = (size_t)p.cap * 3 * OW * 32 + (size_t)p.stg * w * 288;  // Hrow ring | staged z rows
    // Images in chunks: GEMM of a chunk, then its gather -- with the chunk's z (images x h w x 9 N floats) no larger than
    // the Infinity Cache holds next to the other operands, the gather finds most of what the GEMM just wrote still on
    // the die instead of in HBM (g_upconv_chunk_mb; 0 = the whole batch at once)
    const int chunk_mb = g_upconv_chunk_mb.load();
    int bc = B;
    if (chunk_mb > 0) {
        const double per_image = (double)h * w * 9.0 * N * 4.0;
        bc = (int)((double)chunk_mb * 1048576.0 / per_image);
        bc = bc < 8 ? 8 : bc / 8 * 8;
        const int nch = ceil_div(B, bc);
        bc = ceil_div(ceil_div(B, nch), 8) * 8;  // even chunks, whole groups of 8 images (one per XCD)
    }
    for (int b0 = 0; b0 < B; b0 += bc) {
        const int nb = B - b0 < bc ? B - b0 : bc;
        const size_t pix0 = (size_t)b0 * h * w;
        for (int pidx = 0; pidx < parts; ++pidx) {
            const int rc = conv1x1_pointwise(x + pix0 * C, (long long)nb * h * w, C, wp + (size_t)pidx * PART * C, nullptr,
                                             nullptr, 0, z + (size_t)pidx * M * PART + pix0 * PART, PART, s);
            if (rc) return rc;
        }
        p.z = z + pix0 * PART;
        p.y = y + (size_t)b0 * OH * OW * N;
        p.B = nb;
        const dim3 grid((unsigned)(8 * ceil_div(nb, 8) * (N / 8)));
        const bool wide = p.stg * w > kPf * (threads / 18);
        const auto kern = out_c8 ? (wide ? upconv_gather_kernel<true, true> : upconv_gather_kernel<true, false>)
                                 : (wide ? upconv_gather_kernel<false, true> : upconv_gather_kernel<false, false>);
        if (int rc = launch_dynamic_lds("upconv_gather_kernel", kern, grid, dim3(threads), lds, s, p)) return rc;
    }
    return MPSR_OK;
}

}  // namespace mpsr

namespace mpsr {

// most dy rows one source row reaches in upconv_gather_t_kernel: the upsampled rows that interpolate from it + one on
// each side (the kernel's own arithmetic)
static int gather_t_rows(int h, int OH, float hscale)
{
    int most = 1;
    for (int sy = 0; sy < h; ++sy) {
        int lo = OH, hi = -1;
        for (int q = 0; q < OH; ++q) {
            const float sq = (float)q * hscale;
            const int r0 = (int)floorf(sq), r1 = r0 + 1 < h - 1 ? r0 + 1 : h - 1;
            if (r0 == sy || r1 == sy) {
                lo = q < lo ? q : lo;
                hi = q > hi ? q : hi;
            }
        }
        if (hi >= lo) {
            const int a = lo - 1 > 0 ? lo - 1 : 0, b = hi + 1 < OH - 1 ? hi + 1 : OH - 1;
            most = b - a + 1 > most ? b - a + 1 : most;
        }
    }
    return most;
}
static int gather_t_cap(int rows)
{
    int cap = 1;
    while (cap < rows) cap *= 2;
    return cap;
}
// LDS of upconv_gather_t_kernel: the ring (cap rows x 32 channels), the three row-reduced rows V, the row / column tables
static size_t gather_t_lds_bytes(int rows, int h, int w, int OW)
{
    return (size_t)(gather_t_cap(rows) + 3) * OW * 128 + (size_t)w * (kGtMax * 8 + 4) + 16 + (size_t)h * (kGtMax * 8 + 12);
}
// most dy rows a step adds (the next source row's window beyond this one's)
static int gather_t_new_rows(int h, int OH, float hscale)
{
    int most = 0, have = -1;
    for (int sy = 0; sy < h; ++sy) {
        int hi = -1;
        for (int q = 0; q < OH; ++q) {
            const float sq = (float)q * hscale;
            const int r0 = (int)floorf(sq), r1 = r0 + 1 < h - 1 ? r0 + 1 : h - 1;
            if (r0 == sy || r1 == sy) hi = q;
        }
        if (hi >= 0) {
            const int e = hi + 1 < OH - 1 ? hi + 1 : OH - 1;
            if (have >= 0 && e - have > most) most = e - have;
            if (e > have) have = e;
        }
    }
    return most;
}

bool upconv_bwd_applies(int B, int h, int w, int C, int OH, int OW, int N, int align_corners)
{
    const long long M = (long long)B * h * w;
    // (at most kGtMax upsampled rows per source row: scales down to 1/3)
    const bool scale_ok = (long long)OH <= 3LL * h && (long long)OW <= 3LL * w;
    const float hs = (align_corners && OH > 1) ? (float)(h - 1) / (float)(OH - 1) : (float)h / (float)OH;
    return upconv_applies(B, h, w, C, OH, OW, N, align_corners) && scale_ok && OH <= 65535 && h <= 65535 &&
           gather_t_lds_bytes(gather_t_rows(h, OH, hs), h, w, OW) <= 80 * 1024 &&
           gather_t_new_rows(h, OH, hs) * OW * 8 <= kGtPf * 256 && 3 * OW * 8 <= kGtItemsA * 256 && 72 * w <= kGtItemsB * 256 &&
           pointwise_applies(M, 9 * N, C) &&
           M * 9 * N * 4 < 0xfffff000LL && M < (1LL << 24);
}

// floats: dz (M x 9N) | dW' (9N x C) | W'^T (C x 9N)
size_t upconv_bwd_scratch_floats(int B, int h, int w, int C, int N)
{
    const size_t M = (size_t)B * h * w;
    return align_up(M * 9 * N, 64) + 2 * align_up((size_t)9 * N * C, 64);
}

// Backward of conv3x3_upsampled (bias-free part): dy (B,OH,OW,N) NHWC -> dw (N, 9 C) += weight gradient, dx (B,h,w,C) =
// data gradient (or nullptr).  dz = gather^T(dy) at the SOURCE resolution; dW' = dz^T x (a 1x1 weight gradient with 9 N
// outputs) folded back into the filter layout; dx = dz W' (a 1x1 GEMM with K = 9 N on the pointwise kernel) -- the
// resize gradient, the F(4x4) data gradient on the upsampled map and the Winograd-domain weight gradient in one.
int conv3x3_upsampled_bwd(const float *x, const float *dy, int B, int h, int w, int C, int OH, int OW, int align_corners,
                          const float *g, int N, float *dw, float *dx, float *ws, size_t ws_floats, hipStream_t s)
{
    MPSR_REQUIRE(upconv_bwd_applies(B, h, w, C, OH, OW, N, align_corners), "conv3x3_upsampled_bwd: unsupported shape");
    if (!ws || ws_floats < upconv_bwd_scratch_floats(B, h, w, C, N))
        return fail(MPSR_ERR_WORKSPACE, "conv3x3_upsampled_bwd: scratch holds %zu floats, needs %zu", ws_floats,
                    upconv_bwd_scratch_floats(B, h, w, C, N));
    const size_t M = (size_t)B * h * w, wf = align_up((size_t)9 * N * C, 64);
    float *dz = ws, *dwp = ws + align_up(M * 9 * N, 64), *wt = dwp + wf;
    UpcGradParams p;
    p.dy = dy; p.dz = dz;
    p.B = B; p.h = h; p.w = w; p.H = OH; p.W = OW; p.N = N;
    p.hscale = (align_corners && OH > 1) ? (float)(h - 1) / (float)(OH - 1) : (float)h / (float)OH;
    p.wscale = (align_corners && OW > 1) ? (float)(w - 1) / (float)(OW - 1) : (float)w / (float)OW;
    p.rows_max = gather_t_rows(h, OH, p.hscale);
    p.cap = gather_t_cap(p.rows_max);
    const size_t lds = gather_t_lds_bytes(p.rows_max, h, w, OW);
    if (int rc = launch_dynamic_lds("upconv_gather_t_kernel", upconv_gather_t_kernel, dim3((unsigned)(N / 32), (unsigned)B),
                                    dim3(256), lds, s, p))
        return rc;
    // weight gradient of the tap GEMM, folded back into (N, 9 C)
    MPSR_CHECK_HIP(hipMemsetAsync(dwp, 0, (size_t)9 * N * C * sizeof(float), s));
    if (int rc = mpsr_conv2d_wgrad_f32(x, dz, B, h, w, C, 9 * N, 1, 1, 1, dwp, nullptr, reinterpret_cast<mpsr_stream_t>(s))) return rc;
    {
        const long long total = (long long)9 * N * (C / 4);
        hipLaunchKernelGGL(upconv_fold_dw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, dwp, N, C, dw);
        MPSR_CHECK_LAUNCH("upconv_fold_dw_kernel");
    }
    if (dx) {
        const long long total = (long long)C * 9 * N;
        hipLaunchKernelGGL(upconv_weights_t_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, N, C, wt);
        MPSR_CHECK_LAUNCH("upconv_weights_t_kernel");
        if (int rc = conv1x1_pointwise(dz, (long long)M, 9 * N, wt, nullptr, nullptr, 0, dx, C, s)) return rc;
    }
    return MPSR_OK;
}

}  // namespace mpsr

extern "C" int mpsr_conv3x3_upsampled_applies(int B, int h, int w, int C, int OH, int OW, int N, int align_corners)
{
    return mpsr::upconv_applies(B, h, w, C, OH, OW, N, align_corners) ? (mpsr::upconv_bwd_applies(B, h, w, C, OH, OW, N, align_corners) ? 2 : 1) : 0;
}

extern "C" size_t mpsr_conv3x3_upsampled_bwd_scratch_floats(int B, int h, int w, int C, int N)
{
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || N <= 0) return 0;
    return mpsr::upconv_bwd_scratch_floats(B, h, w, C, N);
}

extern "C" int mpsr_conv3x3_upsampled_bwd_f32(const float *x, const float *dy, int B, int h, int w, int C, int OH, int OW,
                                              int align_corners, const float *weights, int N, float *dw, float *dx,
                                              float *ws, size_t ws_floats, mpsr_stream_t stream)
{
    MPSR_REQUIRE(B >= 0 && h > 0 && w > 0 && C > 0 && OH > 0 && OW > 0 && N > 0, "conv3x3_upsampled_bwd: bad shape");
    if (B == 0) return MPSR_OK;
    MPSR_REQUIRE(x && dy && weights && dw && ws, "conv3x3_upsampled_bwd: null pointer");
    if (!mpsr::upconv_bwd_applies(B, h, w, C, OH, OW, N, align_corners))
        return mpsr::fail(MPSR_ERR_UNSUPPORTED, "conv3x3_upsampled_bwd: shape outside what the tap-GEMM backward takes "
                                                "(B=%d %dx%dx%d -> %dx%dx%d); use the resize / conv gradients", B, h, w, C, OH, OW, N);
    return mpsr::conv3x3_upsampled_bwd(x, dy, B, h, w, C, OH, OW, align_corners, weights, N, dw, dx, ws, ws_floats,
                                       mpsr::as_stream(stream));
}

extern "C" size_t mpsr_conv3x3_upsampled_scratch_floats(int B, int h, int w, int C, int N)
{
    if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || N <= 0) return 0;
    return mpsr::align_up(mpsr::upconv_z_floats((long long)B * h * w, N), 64) + mpsr::upconv_weight_floats(C, N);
}

extern "C" int mpsr_conv3x3_upsampled_f32(const float *x, int B, int h, int w, int C, int OH, int OW, int align_corners,
                                          const float *weights, const float *bias, int relu, float *y, int N,
                                          float *ws, size_t ws_floats, mpsr_stream_t stream)
{
    MPSR_REQUIRE(B >= 0 && h > 0 && w > 0 && C > 0 && OH > 0 && OW > 0 && N > 0, "conv3x3_upsampled: bad shape");
    if (B == 0) return MPSR_OK;
    MPSR_REQUIRE(x && weights && y && ws, "conv3x3_upsampled: null pointer");
    if (!mpsr::upconv_applies(B, h, w, C, OH, OW, N, align_corners))
        return mpsr::fail(MPSR_ERR_UNSUPPORTED,
                          "conv3x3_upsampled: needs N %% 128 == 0, C %% 64 == 0 and >= 128 (B=%d %dx%dx%d -> %dx%dx%d); use "
                          "mpsr_resize_bilinear + mpsr_conv2d_nhwc_f32",
                          B, h, w, C, OH, OW, N);
    const size_t zf = mpsr::align_up(mpsr::upconv_z_floats((long long)B * h * w, N), 64);
    if (ws_floats < zf + mpsr::upconv_weight_floats(C, N))
        return mpsr::fail(MPSR_ERR_WORKSPACE, "conv3x3_upsampled: scratch holds %zu floats, needs %zu", ws_floats,
                          zf + mpsr::upconv_weight_floats(C, N));
    return mpsr::conv3x3_upsampled(x, B, h, w, C, OH, OW, align_corners, weights, bias, relu, y, N, 0, ws, zf, ws + zf,
                                   ws_floats - zf, mpsr::as_stream(stream));
}

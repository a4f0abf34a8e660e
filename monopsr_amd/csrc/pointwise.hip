// 1x1 convolution (pointwise GEMM) of the trunk's wide layers on fp32 MFMA:
//     y[m][n] = act( sum_k x[m][k] w[n][k] + bias[n] + residual[m][n] ),   m = pixel (NHWC row), K = C.
// ResNet-101 block3's conv1 / conv3, the projection shortcut, block2's conv3 and the squash layers (reference graph
// object_detection/nets/resnet_v1.py:104-131 bottleneck(), monopsr/core/feature_extractors/resnet.py) -- 9 of the
// step's 16 ms went through the general implicit GEMM (conv_mfma.hip), whose tiles pass BOTH operands through LDS
// (one ds_write_b128 per 16-byte piece, 20-45 cycles of matrix-pipe time each: profiles/r03_mfma_with_lds_stores.txt),
// re-read them as 4 fragments per 12 MFMAs, and load the residual / store the result in an epilogue.  The short-K,
// wide-N layers (block3's conv3: K = 256, N = 1024, + residual) move 8 bytes per output element (residual in, result
// out) for 2 K = 512 flops -- 300 of the layer's 340 MB -- and with prologue / epilogue traffic every CU loads and stores
// at once, in bursts, next to an idle matrix pipe.
//
// Here a PERSISTENT workgroup (4 waves) walks a sequence of 96 x 128 tiles (wave = 3 row tiles x 32 columns, 48
// accumulator registers per set) and a tile's traffic rides on its neighbours' K loops:
//   * A (activations) is shared by the four waves through LDS: 32 k per stage, two stages (128-byte rows, the 16-byte
//     pieces XOR-swizzled by (row >> 1) & 7: ds_read_b128 fragment reads and ds_write_b128 fills are conflict-free);
//     global -> registers a whole stage ahead, registers -> LDS early in the next stage, one barrier per stage.
//   * B (weights) never touches LDS: wave w is the only consumer of its 32 rows of w, lane (n, k half) loads 16 bytes
//     = 4 consecutive k straight from the (N, K) matrix (L2-resident), three 8-k chunks ahead.
//   * K order inside an 8-k chunk: lane half h supplies k = 8 kb + 4 h + s to MFMA s on BOTH operands.
//   * the residual of tile t + 1 is fetched during the K loop of tile t (16-byte loads, six per thread in each of two
//     stages) into a 48 KB LDS copy of the tile; tile t + 1 starts its accumulators from that copy (48 ds_read_b32,
//     then + bias as one more MFMA k: A = 1, B = bias): no residual load waits in front of an MFMA, none occupies a
//     register across a K loop, no vector-ALU arithmetic in front of the stores except the ReLU;
//   * two accumulator sets alternate: a finished tile is stored from its set during the first eight stages of the next
//     tile (ReLU + one store per element -- 2 x 128 contiguous bytes per instruction -- every eighth MFMA slot; issued
//     in one burst behind the K loop the same stores held the wave for 9000 cycles);
//   * the A stages and B chunks run on across tile boundaries as one stream (the next tile's first two stages are
//     requested during this tile's last two);
//   * tile sequence of workgroup b: b, b + G, ...; G is a multiple of 8 x column blocks, so b keeps its XCD and its
//     column block (the same 32 rows of w per wave for its whole life); consecutive workgroups of an XCD share the
//     row group (A from L2).  Tiles past the last row group are all-zero work behind zero-length descriptors;
//   * every descriptor is built in the scalar ALU (base = a row, length = bytes up to row M: rows past M vanish in
//     the range check), ONE per tile (A, mask / emit words) or per 32-row block of it (residual, result); the rows
//     inside it are per-lane constants of the launch and wait in vector registers as ready byte offsets: an access
//     costs its own instruction and no address arithmetic.
// M = batch x 144 pixels on the 12x12 trunk maps: 96-row groups divide it exactly, and at batch 256 the 384 groups x
// N / 128 column blocks are 1.5 (N = 256), 3 (512) or 6 (1024) tiles for each of the 512 resident workgroups.
// What is left: one vmcnt counts loads AND stores in order, so the first wait after a store or a
// residual request also waits for those -- stages 1-2 of a tile take ~3x a plain stage.
#include <atomic>
#include <type_traits>

#include "common.h"
#include "wino3_filter.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

// (The transposed accumulator layout -- 16-byte stores of four channels -- is bit-identical and measured slower: a dword
// store already writes two full lines, the 16-byte form 32 partial ones; DESIGN.md 4.1 (f),
// profiles/r04_pointwise_wide_stores.txt.)
// Cache-policy bits of the residual loads and of the result stores: 2 = non-temporal.  The residual passes through ONCE
// (151 MB on block3's conv3) next to operands that are re-read for the whole launch -- the 1 MB of filters by every
// tile, a row group's activations by all its column blocks: marked streaming it stops evicting those from the 4 MB L2.
// Step, interleaved on one board, three boards: 13.50 -> 13.41 ms (-1.2 %) with the residual loads alone.  The result
// stores are a smaller and mixed effect: streaming them helps the launches WITHOUT a residual (conv1 / shortcut / tap
// GEMMs: 13.41 -> 13.39) and costs on conv3 (its result is the next launch's input: 13.43 with every store streaming).
// The same hint on the activations' loads cost +0.2 .. +0.36 ms (every row group is read by all of its column blocks),
// and on the Winograd kernels' and the upsampling gather's loads and stores it measured equal or slower: everything
// that is read twice or read back at once wants the default policy.
namespace pws {
constexpr int RES_AUX = 2;  // the residual loads stream
constexpr int WT = 3, ROWS = 96, COLS = 128, KS = 32;
constexpr int TILE_B = 32 * KS * 4;          // 4096
constexpr int STAGE_B = WT * TILE_B;         // 12288
constexpr int RES_OFF = 2 * STAGE_B;         // the residual tile behind the two A stages
constexpr int RES_B = ROWS * COLS * 4;       // 49152
constexpr int LDS_B = RES_OFF + RES_B;       // 73728: two workgroups per CU
constexpr unsigned OOB = 0x80000000u;
template <int V>
using IC = std::integral_constant<int, V>;
}  // namespace pws

struct PwsParams {
    const float *x, *w, *bias, *residual;
    float *y;
    int M, N, K, relu;
    int rgroups, cblocks, ntiles;  // ntiles: padded to 8 x column blocks
    unsigned wbytes;
    // tail job: the F(3x3,3x3) filter transform of the 3x3 layer that follows (wino3_filter.h), shared by all workgroups
    const float *fw;
    float *fu;
    int fN, fC, fform;  // fform 0: F(3x3,3x3) filters (25 positions), 1: the sixteen-product form
    // MASK instantiations (training, data-gradient launches): a bit of mask[(row >> 5) * N + column] says whether the
    // output element is kept or written as zero -- the ReLU mask of the tensor this gradient belongs to, applied in the
    // store path instead of by an elementwise pass over the result.  Bit b of a word <-> row 32 g + (b & 3) +
    // 8 ((b >> 2) & 3) + 4 (b >> 4): the accumulator layout of v_mfma_f32_32x32x2_f32 (lane half h = b >> 4 holds element
    // e = b & 15), so a lane's 16 elements of a 32-row tile are one halfword.
    // EMIT instantiations (training, forward launches): the same words written for THIS launch's result (y > 0), one
    // 2-byte store per lane and 32 x 32 block, so that no pass has to read y back to make them (mpsr_relu_bitmask).
    const unsigned *mask;
    unsigned *emit;
    unsigned maskbytes;
};

// LONG: K >= 256 (eight or more stages: the stores of a tile are spread over the next tile's first eight); otherwise
// four stages carry them.
template <bool RES, bool LONG, bool MASK = false, bool EMIT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_conv_kernel(const PwsParams p)
{
    using namespace pws;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nst = p.K / KS;  // even, >= 4
    constexpr int STORE_AUX = RES ? 0 : 2;  // the result stores stream unless the launch adds a residual (see RES_AUX)
    // (a static issue priority between the two co-resident workgroups' waves measured slower: DESIGN.md 0)

    // this workgroup's tiles: i -> row group; the column block is fixed
    const int G = gridDim.x;
    const int xcd = blockIdx.x & 7, l0 = blockIdx.x >> 3;
    const int cb = l0 % p.cblocks;
    const int rgl0 = l0 / p.cblocks, rgstep = (G >> 3) / p.cblocks;
    const int n_my = (p.ntiles - (int)blockIdx.x + G - 1) / G;
    auto r0_of = [&](int i) __attribute__((always_inline)) { return ((rgl0 + i * rgstep) * 8 + xcd) * ROWS; };
    const int n0 = cb * COLS;

    // (lo, hi, left) = address of a row of a tensor and the bytes from there to the tensor's end (row M)
    struct RowRef {
        unsigned lo, hi, left;
    };
    auto row_ref = [&](const float *base, int width, int row, bool live) __attribute__((always_inline)) {
        const bool in = live && base && row >= 0 && row < p.M;  // (a dead reference points at row 0 with length 0)
        const unsigned long long a = reinterpret_cast<unsigned long long>(base + (size_t)(in ? row : 0) * width);
        RowRef r;
        r.lo = (unsigned)a;
        r.hi = (unsigned)(a >> 32);
        r.left = in ? (unsigned)(p.M - row) * (unsigned)width * 4u : 0u;
        return r;
    };
    auto rsrc_of = [&](RowRef r) __attribute__((always_inline)) {
        const unsigned long long a = ((unsigned long long)r.hi << 32) | r.lo;
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(a), 0, (int)r.left, 0x00020000);
    };
    // descriptor `rows` rows further on.  max(left - off, 0) in the scalar ALU (hipcc picks the vector ALU's saturating
    // subtract and a waterfall loop otherwise); the asm also keeps the descriptor of a 32-row block in the slot that
    // first uses it (hipcc otherwise builds a tile's descriptors ahead of its first stage and spills them).
    auto rsrc_at = [&](RowRef r, int rows, int width) __attribute__((always_inline)) {
        const unsigned off = (unsigned)rows * (unsigned)width * 4u;
        unsigned left;
        asm volatile("s_sub_u32 %0, %1, %2\n\ts_cselect_b32 %0, 0, %0" : "=&s"(left) : "s"(r.left), "s"(off) : "scc");
        asm volatile("" : "+s"(r.lo), "+s"(r.hi));
        const unsigned long long a = (((unsigned long long)r.hi << 32) | r.lo) + off;
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(a), 0, (int)left, 0x00020000);
    };

    // ---- A producer: thread = (row prow of each 32-row tile, 16-byte piece pslot of the row's 128 bytes)
    const int prow = tid >> 3, pslot = tid & 7;
    unsigned avoff[WT];  // row prow of 32-row tile j of the row group, as a byte offset behind the group's first row
#pragma unroll
    for (int j = 0; j < WT; ++j) {
        avoff[j] = (unsigned)(32 * j + prow) * (unsigned)p.K * 4u + (unsigned)pslot * 16u;
        asm volatile("" : "+v"(avoff[j]));  // (held, not rebuilt per request)
    }
    const unsigned awoff = (unsigned)prow * 128u + (unsigned)((pslot ^ ((prow >> 1) & 7)) << 4);
    float4 stg[WT];
    auto load_a = [&](__amdgpu_buffer_rsrc_t xd, int stage, int j) __attribute__((always_inline)) {
        stg[j] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(xd, avoff[j], stage * (KS * 4), 0));
    };
    auto store_a = [&](int buf, int j) __attribute__((always_inline)) {
        *reinterpret_cast<float4 *>(lds + buf * STAGE_B + j * TILE_B + awoff) = stg[j];
    };

    // ---- B fragments: lane = (n = lane & 31, k half = lane >> 5), 16 bytes = k 8 kb + 4 h .. + 3 of row n of w
    const int ncol = n0 + 32 * wave + (lane & 31);
    const bool wave_live = n0 + 32 * wave < p.N;  // wave-uniform
    const unsigned bvoff = wave_live ? (unsigned)ncol * (unsigned)p.K * 4u + (unsigned)(lane >> 5) * 16u : OOB;
    float4 fb[4];
    auto load_b = [&](bool live, int stage, int kb) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rr =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w), 0, live ? (int)p.wbytes : 0, 0x00020000);
        fb[kb] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, bvoff + 32u * kb, stage * (KS * 4), 0));
    };

    // ---- A fragments: lane = (row fr of the tile, k half fh); piece 2 kb + fh of the row, swizzled
    const int fr = lane & 31, fh = lane >> 5, ff = (fr >> 1) & 7;
    unsigned aro[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) aro[kb] = (unsigned)(fr * 128 + (((2 * kb + fh) ^ ff) << 4));
    float4 fa[2][3];
    auto read_a = [&](int buf, int kb, int set) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            fa[set][j] = *reinterpret_cast<const float4 *>(lds + buf * STAGE_B + j * TILE_B + aro[kb]);
    };

    // ---- residual staging: piece P = tid + 256 jj of the 96 x 128 tile (row-major, 32 pieces per row): row
    // (tid >> 5) + 8 jj, columns 4 (tid & 31) .. + 3
    // rvoff[u]: row (tid >> 5) + 8 u as a byte offset behind the first row of a 32-row block; piece jj is u = jj & 3 of
    // block jj >> 2, whose descriptor `rd` is built in front of the block's first request
    unsigned rvoff[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        rvoff[u] = ((unsigned)((tid >> 5) + 8 * u) * (unsigned)p.N + (unsigned)(n0 + 4 * (tid & 31))) * 4u;
        if constexpr (RES) asm volatile("" : "+v"(rvoff[u]));
    }
    __amdgpu_buffer_rsrc_t rd;
    const unsigned rwoff = (unsigned)(RES_OFF + (tid >> 5) * 512 + (tid & 31) * 16);
    float4 rst[6];
    auto load_r = [&](RowRef rr, int jj) __attribute__((always_inline)) {
        if (jj % 4 == 0) rd = rsrc_at(rr, 8 * jj, p.N);
        rst[jj % 6] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rd, rvoff[jj & 3], 0, RES_AUX));
    };
    auto store_r = [&](int jj) __attribute__((always_inline)) {
        *reinterpret_cast<float4 *>(lds + rwoff + jj * 4096) = rst[jj % 6];
    };
    // element (q, e) of a lane: row 32 q + (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the tile, column 32 wave + (lane & 31)
    const unsigned rroff = (unsigned)(RES_OFF + (4 * (lane >> 5)) * 512 + (32 * wave + (lane & 31)) * 4);
    // ... as a byte offset behind the first row of 32-row block q, whose descriptor `yd` is built in front of the
    // block's first store
    unsigned evoff[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        evoff[e] = ((unsigned)((e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)) * (unsigned)p.N + (unsigned)ncol) * 4u;
        asm volatile("" : "+v"(evoff[e]));
    }
    __amdgpu_buffer_rsrc_t yd;

    const float bias = (p.bias && wave_live) ? p.bias[ncol] : 0.f;
    const float one = lane < 32 ? 1.f : 0.f;
    const float relu_lo = p.relu ? 0.f : -__builtin_inff();
    // MASK: the three mask words (32 rows x this lane's column) of the tile that accumulates in set S, requested when the
    // tile starts and used a whole tile later; out_bits() = what a store writes for element (q, e) of a set
    unsigned mw[2][WT];
    const unsigned mvoff = wave_live ? (unsigned)ncol * 4u : OOB;
    // the words of the 32-row blocks from row r0 (< M when live) on: block q of the tile is q rows of N words further,
    // in the vector offset -- a block past the last one vanishes in the range check
    auto words_rsrc = [&](const unsigned *base, int r0, bool live) __attribute__((always_inline)) {
        const unsigned off = live ? (unsigned)(r0 / 32) * (unsigned)p.N * 4u : 0u;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(reinterpret_cast<const char *>(base)) + off, 0,
                                                 live ? (int)(p.maskbytes - off) : 0, 0x00020000);
    };
    auto load_mask = [&](auto set_c, int r0, bool live) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
        const __amdgpu_buffer_rsrc_t rr = words_rsrc(p.mask, r0, live);
#pragma unroll
        for (int q = 0; q < WT; ++q)
            mw[S][q] = __builtin_amdgcn_raw_buffer_load_b32(rr, mvoff + (unsigned)q * (unsigned)p.N * 4u, 0, 0);
    };
    const unsigned mshift = 16u * (unsigned)(lane >> 5);
    unsigned mb[2][WT];  // EMIT: the halfword of set S's tile gathering while its elements are stored
    const unsigned emvoff = wave_live ? (unsigned)ncol * 4u + 2u * (unsigned)(lane >> 5) : OOB;
    f32x16 acc[2][WT];  // a tile accumulates in one set while the previous tile is stored from the other
    auto out_bits = [&](auto set_c, int q, int e) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
        if constexpr (MASK) {
            const int keep = __builtin_amdgcn_sbfe((int)mw[S][q], mshift + (unsigned)e, 1u);
            const float v = acc[S][q][e];  // (bit_cast of the vector-element lvalue itself picks element 0)
            return (unsigned)keep & __builtin_bit_cast(unsigned, v);
        } else {
            const float v = fmaxf(acc[S][q][e], relu_lo);
            if constexpr (EMIT) mb[S][q] = (e ? mb[S][q] : 0u) | (v > 0.f ? 1u << e : 0u);
            return __builtin_bit_cast(unsigned, v);
        }
    };
    // EMIT: after element 15 of block q of the tile at row r0 the halfword is complete
    auto emit_bits = [&](auto set_c, int q, int r0, bool live) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
        __builtin_amdgcn_raw_buffer_store_b16((short)mb[S][q], words_rsrc(p.emit, r0, live),
                                              emvoff + (unsigned)q * (unsigned)p.N * 4u, 0, 0);
    };
#pragma unroll
    for (int q = 0; q < WT; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[1][q][e] = 0.f;


    // One stage = 4 units (kb) of 12 MFMAs on the three accumulators, k outermost.  Slot D = 12 kb + m carries: the next
    // unit's fragment reads (m = 0); the A staging of tile j (registers -> LDS at D = 4 + 12 j, the request two stages on
    // at D + 2); the B chunk of the next stage (m = 11); and the residual duty -- DUTY 1 / 2: the first / second six
    // pieces of the next tile's residual requested (D = 9 + 6 n); DUTY 2 / 3: the first / second six written to LDS
    // (D = 7 + 6 n).
    // SE0 >= 0: also ReLU + store of elements SE0, SE0 + 1, ... of the previous tile (the other accumulator set), one
    // every SSTEP slots (D = 1 + SSTEP n) -- the 48 stores of a tile are spread over its first eight stages (four when
    // K = 128 / 192): one in-order counter covers loads and stores, so every wait for an A / B request also waits for
    // the stores issued before it, and those complete sooner the thinner they are spread (12 KB per wave in one burst
    // behind the K loop held the wave for 9000 cycles; over three stages the stages after them took 3x as long).
    auto stage_body = [&](auto set_c, auto buf_c, auto duty_c, auto se0_c, auto sstep_c, int s, RowRef xc, bool clive,
                          RowRef xn, bool nlive, RowRef rn, RowRef yp, int r0p = 0, bool plive = false)
                          __attribute__((always_inline)) {
        constexpr int SET = decltype(set_c)::value, buf = decltype(buf_c)::value, DUTY = decltype(duty_c)::value,
                      SE0 = decltype(se0_c)::value, SSTEP = decltype(sstep_c)::value;
        read_a(buf, 0, 0);
        // stage s + 2 of this tile, or stage s + 2 - nst of the next one (scalar selects)
        const bool wrap2 = s + 2 >= nst;
        RowRef xa;
        xa.lo = wrap2 ? xn.lo : xc.lo;
        xa.hi = wrap2 ? xn.hi : xc.hi;
        xa.left = wrap2 ? xn.left : xc.left;
        const __amdgpu_buffer_rsrc_t xd = rsrc_of(xa);
        const int a_st = wrap2 ? s + 2 - nst : s + 2;
        const bool wrap1 = s + 1 >= nst;
        const int b_st = wrap1 ? 0 : s + 1;
        const bool b_live = wrap1 ? nlive : clive;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            const int set = kb & 1;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const int m = 3 * k + j, D = 12 * kb + m;
                    const float av = k == 0 ? fa[set][j].x : k == 1 ? fa[set][j].y : k == 2 ? fa[set][j].z : fa[set][j].w;
                    const float bv = k == 0 ? fb[kb].x : k == 1 ? fb[kb].y : k == 2 ? fb[kb].z : fb[kb].w;
                    acc[SET][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[SET][j], 0, 0, 0);
                    if (m == 0 && kb < 3) read_a(buf, kb + 1, set ^ 1);
                    if constexpr (SE0 >= 0) if (D % SSTEP == 1 && SE0 + D / SSTEP < 16 * WT) {
                        const int q = (SE0 + D / SSTEP) / 16, e = (SE0 + D / SSTEP) % 16;
                        if (e == 0) yd = rsrc_at(yp, 32 * q, p.N);
                        __builtin_amdgcn_raw_buffer_store_b32(out_bits(IC<SET ^ 1>{}, q, e), yd, evoff[e], 0, STORE_AUX);
                        if constexpr (EMIT) if (e == 15) emit_bits(IC<SET ^ 1>{}, q, r0p, plive);
                    }
                    if (D >= 4 && D < 4 + 12 * WT && (D - 4) % 12 == 0) store_a(buf ^ 1, (D - 4) / 12);
                    if (D >= 6 && D < 6 + 12 * WT && (D - 6) % 12 == 0) load_a(xd, a_st, (D - 6) / 12);
                    if (m == 11) load_b(b_live, b_st, kb);
                    if constexpr (RES) {
                        // (stage 2 first writes piece n of the first six out of its register, then requests piece
                        // 6 + n into it)
                        if ((DUTY == 2 || DUTY == 3) && D >= 7 && D < 7 + 36 && (D - 7) % 6 == 0)
                            store_r((DUTY - 2) * 6 + (D - 7) / 6);
                        if ((DUTY == 1 || DUTY == 2) && D >= 9 && D < 9 + 36 && (D - 9) % 6 == 0)
                            load_r(rn, (DUTY - 1) * 6 + (D - 9) / 6);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
    };

    // ---- prologue: the first tile's residual into its LDS copy, its stage 0 into LDS, stage 1 into the staging
    // registers, the B chunks of stage 0
    {
        const __amdgpu_buffer_rsrc_t x0 = rsrc_of(row_ref(p.x, p.K, r0_of(0), true));
#pragma unroll
        for (int j = 0; j < WT; ++j) load_a(x0, 0, j);
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) load_b(true, 0, kb);
        if constexpr (RES) {
            const RowRef r0r = row_ref(p.residual, p.N, r0_of(0), true);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int jj = 0; jj < 6; ++jj) load_r(r0r, 6 * h + jj);
#pragma unroll
                for (int jj = 0; jj < 6; ++jj) store_r(6 * h + jj);
            }
        }
#pragma unroll
        for (int j = 0; j < WT; ++j) store_a(0, j);
#pragma unroll
        for (int j = 0; j < WT; ++j) load_a(x0, 1, j);
        __syncthreads();
    }

    auto tile_body = [&](auto set_c, int i) __attribute__((always_inline)) {
        constexpr int SET = decltype(set_c)::value;
        const int r0c = r0_of(i), r0n = r0_of(i + 1);
        const bool nlive = i + 1 < n_my;
        const RowRef xc = row_ref(p.x, p.K, r0c, true), xn = row_ref(p.x, p.K, r0n, nlive);
        const RowRef rn = row_ref(p.residual, p.N, r0n, nlive);
        const RowRef yp = row_ref(p.y, p.N, r0_of(i - 1), i > 0 && wave_live);
        if constexpr (MASK) load_mask(IC<SET>{}, r0c, r0c < p.M);
        // the accumulators start from the residual (its LDS copy) ...
#pragma unroll
        for (int q = 0; q < WT; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                acc[SET][q][e] = RES ? *reinterpret_cast<const float *>(lds + rroff + (32 * q + (e & 3) + 8 * (e >> 2)) * 512) : 0.f;
        // ... + bias as one more k: A = (1, 0) over the lane halves, B = bias of the lane's column
#pragma unroll
        for (int q = 0; q < WT; ++q) acc[SET][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(one, bias, acc[SET][q], 0, 0, 0);
        // stage (s, buffer s & 1, residual duty, first stored element, slots per store)
#define PWS_STAGE(S_, DUTY_, SE0_, SSTEP_)                                                                            \
    stage_body(IC<SET>{}, IC<(S_) & 1>{}, IC<DUTY_>{}, IC<SE0_>{}, IC<SSTEP_>{}, S_, xc, true, xn, nlive, rn, yp,     \
               r0_of(i - 1), i > 0 && r0_of(i - 1) < p.M);                                                            \
    __syncthreads()
        if constexpr (LONG) {
            PWS_STAGE(0, 0, 0, 8);  // (after this barrier every wave has read its part of the residual copy: the
            PWS_STAGE(1, 1, 6, 8);  //  next tile's may be written)
            PWS_STAGE(2, 2, 12, 8);
            PWS_STAGE(3, 3, 18, 8);
            PWS_STAGE(4, 0, 24, 8);
            PWS_STAGE(5, 0, 30, 8);
            PWS_STAGE(6, 0, 36, 8);
            PWS_STAGE(7, 0, 42, 8);
            for (int s = 8; s < nst; s += 2) {
                stage_body(IC<SET>{}, IC<0>{}, IC<0>{}, IC<-1>{}, IC<1>{}, s, xc, true, xn, nlive, rn, yp);
                __syncthreads();
                stage_body(IC<SET>{}, IC<1>{}, IC<0>{}, IC<-1>{}, IC<1>{}, s + 1, xc, true, xn, nlive, rn, yp);
                __syncthreads();
            }
        } else {
            PWS_STAGE(0, 0, 0, 4);
            PWS_STAGE(1, 1, 12, 4);
            PWS_STAGE(2, 2, 24, 4);
            PWS_STAGE(3, 3, 36, 4);
            for (int s = 4; s < nst; s += 2) {
                stage_body(IC<SET>{}, IC<0>{}, IC<0>{}, IC<-1>{}, IC<1>{}, s, xc, true, xn, nlive, rn, yp);
                __syncthreads();
                stage_body(IC<SET>{}, IC<1>{}, IC<0>{}, IC<-1>{}, IC<1>{}, s + 1, xc, true, xn, nlive, rn, yp);
                __syncthreads();
            }
        }
#undef PWS_STAGE
    };
    int i = 0;
    for (; i < n_my; i += 2) {
        tile_body(IC<0>{}, i);
        if (i + 1 >= n_my) break;
        tile_body(IC<1>{}, i + 1);
    }
    // ---- the last tile's stores (the 16-pass MFMA needs 18 wait states before its result is read; explicit as in
    // conv_mfma.hip): set 0 when the workgroup had an odd number of tiles
    const int last = n_my - 1;
    int r0s = r0_of(last);
    asm volatile("s_nop 15\n\ts_nop 7"
                 : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]),
                   "+s"(r0s));
    const RowRef yl = row_ref(p.y, p.N, r0s, wave_live);
    auto finish = [&](auto set_c) __attribute__((always_inline)) {
        constexpr int SET = decltype(set_c)::value;
#pragma unroll
        for (int q = 0; q < WT; ++q)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                if (e == 0) yd = rsrc_at(yl, 32 * q, p.N);
                __builtin_amdgcn_raw_buffer_store_b32(out_bits(IC<SET>{}, q, e), yd, evoff[e], 0, STORE_AUX);
                if constexpr (EMIT) if (e == 15) emit_bits(IC<SET>{}, q, r0s, r0s < p.M);
            }
    };
    if (last & 1) finish(IC<1>{});  // block-uniform
    else finish(IC<0>{});
    if (p.fw) {  // block-uniform
        const long long total = (long long)p.fN * p.fC;
        for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)gridDim.x * 256)
            if (p.fform) mpsr::wino3z_filter_one(p.fw, p.fN, p.fC, p.fu, i);
            else mpsr::wino3_filter_one(p.fw, p.fN, p.fC, p.fu, i);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Fully-connected layers with few rows (the heads: M = batch = 256 rows, K ~ 1024, N = 1024 / 27 / 2; reference
// monopsr_output_builder.py:126-302).  A 64 x 64-tile GEMM makes 64 workgroups of them -- a quarter of the CUs, each
// running a 1000-deep K loop alone (36 us per layer).  Here a workgroup owns ONE 32 x 32 output tile (8 x 32 = 256
// workgroups for 256 x 1024) and its four waves split K; both operands' fragments come straight from global memory
// (lane = (row, k half), 16 bytes: the four 8-k chunks of a 128-byte line are requested together, eight chunks in
// flight per wave), no LDS in the K loop; the four partial tiles are summed through LDS and wave 0 applies bias /
// residual / ReLU.
// SPLIT = 1 (img_fc at the reference's 32 boxes per image: 32 rows x K = 18432 -> N = 2048): K is longer than four
// waves can stream (64 workgroups would read the 151 MB of weights), so blockIdx.y selects one of several K slabs and
// the workgroup stores its partial tile into slab blockIdx.y of a scratch tensor; winograd_finish_slices (winograd3z.hip)
// adds the slabs in order + bias + ReLU.  Every weight byte is read once per 32-row block: memory-bound.
template <int SPLIT>
__global__ __launch_bounds__(256) void fc_rows_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                      const float *__restrict__ bias, const float *__restrict__ residual,
                                                      float *__restrict__ y, int M, int N, int K, int relu,
                                                      unsigned xbytes, unsigned wbytes, int kslab)
{
    __shared__ __attribute__((aligned(16))) float part[3][16][64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntn = (N + 31) >> 5;
    const int r0 = (blockIdx.x / ntn) * 32, n0 = (blockIdx.x % ntn) * 32;
    const int kper = kslab >> 2;        // the slab (= K unless SPLIT) a multiple of 32: every wave gets whole 8-k chunks
    const int nch = kper >> 3;          // chunks per wave
    const int i = lane & 31, h = lane >> 5;
    const unsigned OOB = 0x80000000u;
    const unsigned koff = (unsigned)((SPLIT ? (int)blockIdx.y * kslab : 0) + wave * kper + 4 * h) * 4u;
    const unsigned aoff = r0 + i < M ? (unsigned)(r0 + i) * (unsigned)K * 4u + koff : OOB;
    const unsigned boff = n0 + i < N ? (unsigned)(n0 + i) * (unsigned)K * 4u + koff : OOB;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, (int)xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w), 0, (int)wbytes, 0x00020000);
    constexpr int PF = 8;  // chunks in flight
    float4 fa[PF], fb[PF];
    auto request = [&](int c, int slot) __attribute__((always_inline)) {
        const bool live = c < nch;
        const __amdgpu_buffer_rsrc_t rxl =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, live ? (int)xbytes : 0, 0x00020000);
        const __amdgpu_buffer_rsrc_t rwl =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(w), 0, live ? (int)wbytes : 0, 0x00020000);
        fa[slot] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rxl, aoff, (live ? c : 0) * 32, 0));
        fb[slot] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rwl, boff, (live ? c : 0) * 32, 0));
    };
    (void)rx;
    (void)rw;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int c = 0; c < PF; ++c) request(c, c);
    for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const float4 a = fa[u], b = fb[u];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            request(c0 + PF + u, u);
        }
    }
    // (the 16-pass MFMA needs 18 wait states before its result is read; explicit as in conv_mfma.hip)
    asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc));
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) part[wave - 1][e][lane] = acc[e];
    }
    __syncthreads();
    if (wave > 0) return;
    // accumulator element e of a lane: row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31
    const int col = n0 + i;
    const float bv = (!SPLIT && bias && col < N) ? bias[col] : 0.f;
    float *yo = SPLIT ? y + (size_t)blockIdx.y * M * N : y;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = r0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        float v = ((acc[e] + part[0][e][lane]) + part[1][e][lane]) + part[2][e][lane] + bv;
        if (row < M && col < N) {
            if (!SPLIT && residual) v += residual[(size_t)row * N + col];
            if (!SPLIT && relu) v = fmaxf(v, 0.f);
            yo[(size_t)row * N + col] = v;
        }
    }
}

std::atomic<int> g_pw_override{-1};  // -1 heuristic, 0 never, 1 wherever it applies
std::atomic<int> g_pws_per_cu{2};

}  // namespace

extern "C" void mpsr_debug_set_conv_pointwise(int mode) { g_pw_override = mode; }
extern "C" void mpsr_debug_set_pointwise_per_cu(int n) { g_pws_per_cu = n > 0 ? n : 2; }

namespace mpsr {

int pointwise_override() { return g_pw_override.load(); }

// Shapes the kernel takes: K a multiple of 64 and >= 128 (whole pairs of 32-k stages, four of them carry the residual
// and store duties), N a multiple of 32, 32-bit byte offsets, few enough column blocks for a persistent grid whose
// stride keeps a workgroup on one column block.
bool pointwise_applies(long long M, int K, int N)
{
    return M > 0 && K >= 128 && K % 64 == 0 && N >= 32 && N % 32 == 0 && (N + 127) / 128 <= 32 &&
           M * K * 4 < 0x7f000000LL && M * N * 4 < 0xfffffff0LL && (long long)N * K * 4 < 0x7f000000LL;
}

// Shapes whose result can leave through a ReLU bit mask (conv1x1_pointwise_masked): the long-K instantiations
bool pointwise_masked_applies(long long M, int K, int N)
{
    return pointwise_applies(M, K, N) && K / pws::KS >= 8;
}

static int pointwise_launch(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                            int relu, const unsigned *mask, unsigned *emit, float *y, int N, hipStream_t s, LayerExtras *ex);

int conv1x1_pointwise(const float *x, long long M, int K, const float *w, const float *bias,
                             const float *residual, int relu, float *y, int N, hipStream_t s, LayerExtras *ex)
{
    MPSR_REQUIRE(pointwise_applies(M, K, N), "conv1x1_pointwise: unsupported shape (M=%lld K=%d N=%d)", M, K, N);
    return pointwise_launch(x, M, K, w, bias, residual, relu, nullptr, nullptr, y, N, s, ex);
}

// conv1x1_pointwise that also writes the ReLU bit mask of its result (bits of rows >= M unspecified)
int conv1x1_pointwise_emit(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                           int relu, float *y, unsigned *bits, int N, hipStream_t s)
{
    MPSR_REQUIRE(pointwise_masked_applies(M, K, N), "conv1x1_pointwise_emit: unsupported shape (M=%lld K=%d N=%d)", M, K, N);
    MPSR_REQUIRE(bits, "conv1x1_pointwise_emit: null mask");
    return pointwise_launch(x, M, K, w, bias, residual, relu, nullptr, bits, y, N, s, nullptr);
}

// y[m][n] = keep(m, n) ? sum_k x[m][k] w[n][k] + bias[n] + residual[m][n] : 0, keep = bit (m & 31) of
// mask[(m >> 5) * N + n] ((M + 31) / 32 * N words, mpsr_relu_bitmask)
int conv1x1_pointwise_masked(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                             const unsigned *mask, float *y, int N, hipStream_t s)
{
    MPSR_REQUIRE(pointwise_masked_applies(M, K, N), "conv1x1_pointwise_masked: unsupported shape (M=%lld K=%d N=%d)", M, K, N);
    MPSR_REQUIRE(mask, "conv1x1_pointwise_masked: null mask");
    return pointwise_launch(x, M, K, w, bias, residual, 0, mask, nullptr, y, N, s, nullptr);
}

static int pointwise_launch(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                            int relu, const unsigned *mask, unsigned *emit, float *y, int N, hipStream_t s, LayerExtras *ex)
{
    using namespace pws;
    PwsParams p;
    p.mask = mask;
    p.emit = emit;
    p.maskbytes = (unsigned)(((M + 31) / 32) * N * 4);
    p.x = x; p.w = w; p.bias = bias; p.residual = residual; p.y = y;
    p.M = (int)M; p.N = N; p.K = K; p.relu = relu;
    p.rgroups = (int)((M + ROWS - 1) / ROWS);
    p.cblocks = ceil_div(N, COLS);
    p.ntiles = ceil_div(p.rgroups, 8) * 8 * p.cblocks;
    p.wbytes = (unsigned)((long long)N * K * 4);
    // CU count of the CURRENT device, cached per device id (a process may drive several GPUs; the count only sizes
    // the persistent grid)
    static std::atomic<int> cu_count[64];
    int dev = 0;
    MPSR_CHECK_HIP(hipGetDevice(&dev));
    int cus = dev >= 0 && dev < 64 ? cu_count[dev].load() : 0;
    if (cus == 0) {
        int n = 256;
        MPSR_CHECK_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        cus = n > 0 ? n : 256;
        if (dev >= 0 && dev < 64) cu_count[dev] = cus;
    }
    // persistent grid: g_pws_per_cu workgroups per CU, rounded down to a multiple of 8 x column blocks
    const int unit = 8 * p.cblocks;
    int grid = g_pws_per_cu.load() * cus / unit * unit;
    if (grid < unit) grid = unit;
    if (grid > p.ntiles) grid = p.ntiles;
    // the caller's filter-transform job rides on this launch
    const FilterTailJob job = ex ? ex->tail : FilterTailJob();
    p.fw = job.w; p.fu = job.u; p.fN = job.N; p.fC = job.C; p.fform = job.form;
    if (ex) ex->tail_taken = job.w != nullptr;
    // instantiation <RES, LONG, MASK, EMIT>: masked and emitting launches are LONG ones
    const int pick = (residual ? 1 : 0) | (mask ? 4 : emit ? 6 : K / KS >= 8 ? 2 : 0);
    void (*const kernels[8])(const PwsParams) = {
        pw_conv_kernel<false, false>, pw_conv_kernel<true, false>, pw_conv_kernel<false, true>, pw_conv_kernel<true, true>,
        pw_conv_kernel<false, true, true>, pw_conv_kernel<true, true, true>,
        pw_conv_kernel<false, true, false, true>, pw_conv_kernel<true, true, false, true>};
    return launch_dynamic_lds("pw_conv_kernel", kernels[pick], dim3(grid), dim3(256), (size_t)LDS_B, s, p);
}


// Few-row fully-connected layers (fc_rows_kernel): K a multiple of 32 up to 4096 (longer K: the stream-K kernel, whose
// tiles share the operand traffic), 32-bit byte offsets.
bool fc_rows_applies(long long M, int K, int N)
{
    return M > 0 && M <= 2048 && K >= 128 && K <= 4096 && K % 32 == 0 && N > 0 && M * K * 4 < 0x7f000000LL &&
           (long long)N * K * 4 < 0x7f000000LL;
}

int fc_rows(const float *x, long long M, int K, const float *w, const float *bias, const float *residual, int relu,
            float *y, int N, hipStream_t s)
{
    MPSR_REQUIRE(fc_rows_applies(M, K, N), "fc_rows: unsupported shape (M=%lld K=%d N=%d)", M, K, N);
    const unsigned grid = (unsigned)(((M + 31) / 32) * ((N + 31) / 32));
    hipLaunchKernelGGL(fc_rows_kernel<0>, dim3(grid), dim3(256), 0, s, x, w, bias, residual, y, (int)M, N, K, relu,
                       (unsigned)(M * K * 4), (unsigned)((long long)N * K * 4), K);
    MPSR_CHECK_LAUNCH("fc_rows_kernel");
    return MPSR_OK;
}

std::atomic<int> g_fc_split_rows{96};  // mpsr_debug_set_fc_split_rows: the K-split few-row kernel up to this many rows (0: never)

// K slabs of the split form for a long-K layer with few rows: enough workgroups to stream the weights from every CU
static int fc_rows_slabs(long long M, int K, int N)
{
    const long long tiles = ((M + 31) / 32) * ((N + 31) / 32);
    int s = 1;
    while (tiles * s < 512 && s < 16 && K % (64 * s) == 0) s *= 2;
    return s;
}

// img_fc at small batches: few rows, K too long for the four waves of one workgroup (fc_rows_applies stops at 4096)
bool fc_rows_split_applies(long long M, int K, int N, const float *bias, const float *y, const float *ws, size_t ws_floats)
{
    const int rows = g_fc_split_rows.load();
    if (!(M > 0 && M <= rows && K > 4096 && K % 64 == 0 && N > 0 && N % 4 == 0 && ws && M * K * 4 < 0x7f000000LL &&
          (long long)N * K * 4 < 0x7f000000LL))
        return false;
    const int slabs = fc_rows_slabs(M, K, N);
    return slabs > 1 && (size_t)slabs * M * N <= ws_floats && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)y & 15) == 0 &&
           (!bias || ((uintptr_t)bias & 15) == 0);
}

int fc_rows_split(const float *x, long long M, int K, const float *w, const float *bias, int relu, float *y, int N,
                  float *ws, hipStream_t s)
{
    const int slabs = fc_rows_slabs(M, K, N);
    const dim3 grid((unsigned)(((M + 31) / 32) * ((N + 31) / 32)), (unsigned)slabs);
    hipLaunchKernelGGL(fc_rows_kernel<1>, grid, dim3(256), 0, s, x, w, nullptr, nullptr, ws, (int)M, N, K, 0,
                       (unsigned)(M * K * 4), (unsigned)((long long)N * K * 4), K / slabs);
    MPSR_CHECK_LAUNCH("fc_rows_kernel");
    return winograd_finish_slices(ws, bias, y, (size_t)M * N, slabs, N, relu, s);
}

}  // namespace mpsr

extern "C" void mpsr_debug_set_fc_split_rows(int rows) { mpsr::g_fc_split_rows = rows; }

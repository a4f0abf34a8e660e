// The Winograd kernel of the atrous 3x3 layers whose pixel sub-grids are single 3x3 tiles (ResNet-101 block3's conv2 at
// output stride 4: 12x12 maps, dilation 4, 23 launches per step) in the form where ONE WAVE OWNS ALL POSITIONS of its
// (32 tiles x 32 output channels) block, written once over a compile-time FORM: F(3x3,3x3) with 25 positions
// (winograd3w.hip) and the sixteen-product form of a zero-padded tile (winograd3z.hip) describe and instantiate it.
//
// winograd3.hip spreads a tile's positions over eight waves (6-7 positions each), so the output transform A^T M A needs
// every wave's accumulators: a 100 KB exchange through LDS in two rounds, and a workgroup lives for only 32 short K steps
// around it (measured: ~25 % of the launch is prologue / exchange / epilogue).  Here a wave keeps NP x 16 accumulator
// registers -- the first 16 positions in the accumulator half of the register file under literal names (acc_named.h), the
// rest (Form::NP - 16: nine or none) in the vector half, one wave per SIMD -- every position's 32x32 tile has the same lane
// layout, so the NP values of one (tile, channel) sit in ONE LANE and the output transform is lane-local: no exchange, no
// second round.
//
// Workgroup = 4 waves = 32 tiles x 128 output channels.  The transformed patches (A operand) of a K step (8 channels) are
// produced once per workgroup -- one patch per thread and step -- and shared through LDS by the four waves, i.e. the
// vector instructions + LDS stores of a patch are amortised over 128 output channels (every vector instruction next to an
// fp32 MFMA costs ~4 cycles of the SIMD's matrix time, DESIGN 4.1 finding 6: the transform is THE overhead of this kernel).
// B fragments come straight from the transformed filters (L2), layout U[cb][pos][n][8] of wino3_filter.h, so the filter
// cache and the tail-job transform serve these kernels too.
// (WM = 1 in the body: the producer is written for WM patches per thread, but 64 tiles x 64 channels with two patches per
// thread cannot run -- hipcc runs out of vector registers there and parks values in a0..a8, i.e. inside position 0's
// accumulators -- so it is a constant, not a parameter.)
//
// K step = 4 NP MFMAs (position-major, 4 per position), double-buffered A with ONE barrier per step at slot 4 (NP - 2): a
// step's last A read (position NP - 1) is issued one position earlier, the next step's first right behind the barrier, and
// the producer's stores of the next step's patches sit in the first slots (they target the buffer whose reads ended at the
// previous barrier).  A fragments two positions ahead in a ring of four register quads (colours Form::cA), B fragments
// Form::BPRE positions ahead in a ring of Form::BRING (colours Form::cB): inside a step the transformed filters of a layer
// come from the Infinity Cache, not from L2, and a wave alone on its SIMD has nobody to hide a late fragment behind.
// (the non-temporal cache policy on the transformed-filter loads or the result stores measured slower: DESIGN.md 4.1 (f))
//
// A form gives:
//   NP, E                   positions per tile and the patch edge (NP = E * E)
//   COL0                    patch column that data column 0 is transformed into (the row pass reads columns COL0 .. COL0 + 2)
//   bt<S>(a, b, c, o)       the input transform of three values into o[0], o[S], ..., o[(E - 1) S]
//   at(m, y0, y1, y2)       the output transform of E values into three
//   cA(q), cB(q), BPRE, BRING   the fragment rings
//   REQ0                    first slot of the next-but-one step's nine requests (the patch is transformed in slots
//                           0 .. 2 E + 3: three columns, then a row every other slot with its stores behind it in two slots)
//   HAS_SPLIT               whether the SPLIT instantiation (K slices into a scratch tensor) exists
#pragma once
#include "acc_named.h"
#include "common.h"

namespace mpsr {

struct Wino3OneParams {
    const float *x, *u, *bias, *mask;
    float *y;
    int H, W, C, N, dil, T;  // T = B * dil * dil tiles (one per pixel sub-grid)
    int cblocks, nblocks, mblocks, relu;
    unsigned xbytes, ubytes, ybytes;
    FastDiv div_tpi, div_d;  // tiles per image = dil^2, dil
    // SPLIT: K slices; slice k runs channel steps [k * steps, (k + 1) * steps) and stores into part + k * ybytes / 4
    float *part;
    int nslices, steps;
};

namespace w3one {
constexpr int KC = 8, MT = 32, NT = 128;  // channels per K step; tiles and output channels per workgroup
constexpr unsigned OOB = 0x80000000u;
using f32x16 = __attribute__((ext_vector_type(16))) float;
}  // namespace w3one

// MASK: a data-gradient launch of the training path (p.mask = a tensor shaped like y; an output is kept where the mask is
// positive: the ReLU gradient of the layer the gradient belongs to, applied in the store path)
template <class Form, bool MASK, bool SPLIT>
__device__ __forceinline__ void wino3_onewave_body(const Wino3OneParams p)
{
    static_assert(!(MASK && SPLIT), "the masked (training) launches are never split");
    static_assert(!SPLIT || Form::HAS_SPLIT, "this form has no SPLIT instantiation");
    using namespace w3one;
    constexpr int NP = Form::NP, E = Form::E, COL0 = Form::COL0, BPRE = Form::BPRE;
    constexpr int NVEC = NP - 16;  // positions in the vector half of the register file
    static_assert(NP == E * E && (NVEC == 0 || NVEC == 9), "the wait-state statement below names the vector-half tuples");
    constexpr int WM = 1;            // 32-tile blocks of a workgroup = patches per thread and step (see above)
    constexpr int APOS = MT * KC;    // floats per position of an A buffer
    constexpr int ABUF = NP * APOS;  // one A buffer
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int xcd = blockIdx.x & 7, l_ = blockIdx.x >> 3;
    const int nb = l_ % p.nblocks;
    int l2_ = l_ / p.nblocks, slice = 0;
    if constexpr (SPLIT) {
        slice = l2_ % p.nslices;
        l2_ /= p.nslices;
    }
    const int mb = l2_ * 8 + xcd;
    if (mb >= p.mblocks) return;  // block-uniform
    const int n0 = nb * NT, t0 = mb * MT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mi = wave % WM, ni = wave / WM;
    const int s0 = SPLIT ? slice * p.steps : 0;                 // first channel step of this workgroup
    const int send = SPLIT ? s0 + p.steps : p.cblocks, d = p.dil, tpi = d * d;

    // ---- A producer: thread = (tile, channel of the step) for WM patches per step; nine 4-byte requests per patch
    const int ch = lane & 7;
    unsigned abase[WM];
    float *awr[WM];
#pragma unroll
    for (int r = 0; r < WM; ++r) {
        const int lt = 32 * r + 8 * wave + (lane >> 3);
        const int t = t0 + lt;
        const int img = fdiv(t, p.div_tpi), sub = t - img * tpi;
        const int a = fdiv(sub, p.div_d), b = sub - a * d;
        abase[r] = t < p.T ? (unsigned)(((img * p.H + a) * p.W + b) * p.C + ch) * 4u : OOB;
        // A[buf][pos][tile][8 channels], 16-byte halves swapped on odd 8-row blocks
        awr[r] = lds + lt * 8 + 4 * ((ch >> 2) ^ ((lt >> 3) & 1)) + (ch & 3);
    }
    float raw[WM][9];  // column by column: raw[3 j + i] = sub-grid pixel (row i, column j)
    // (requests past the last K step are not special-cased: they read the neighbouring channels / positions or fall outside
    // the descriptor's range and return zeros; nothing consumes them)
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)p.xbytes, 0x00020000);
    auto load_raw = [&](int step, auto rc, auto Lc) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value, L = decltype(Lc)::value, j = L / 3, i = L % 3;
        const unsigned so = (unsigned)((d * i * p.W + d * j) * p.C + step * KC) * 4u;
        raw[r][L] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, abase[r], so, 0));
    };
    float pa[NP];  // the E x E transformed patch being built: pa[E u + v]
    auto vertical = [&](auto rc, auto jc) __attribute__((always_inline)) {  // data column j -> the E rows of patch column COL0 + j
        constexpr int r = decltype(rc)::value, j = decltype(jc)::value;
        Form::template bt<E>(raw[r][3 * j], raw[r][3 * j + 1], raw[r][3 * j + 2], pa + COL0 + j);
    };
    auto horizontal = [&](auto ic) __attribute__((always_inline)) {  // row i: its three column values -> E
        constexpr int i = decltype(ic)::value;
        float t_[E];
        Form::template bt<1>(pa[E * i + COL0], pa[E * i + COL0 + 1], pa[E * i + COL0 + 2], t_);
#pragma unroll
        for (int v = 0; v < E; ++v) pa[E * i + v] = t_[v];
    };
    auto store_a = [&](auto rc, int buf, int pos) __attribute__((always_inline)) {
        constexpr int r = decltype(rc)::value;
        awr[r][buf * ABUF + pos * APOS] = pa[pos];
    };
    // producer duty of slot m of a K step: the patch transformed in slots 0 .. 2 E + 3 (3 columns, then a row every other slot
    // with its E stores behind it, in two slots), the next-but-one step's nine requests from slot REQ0 on
    auto duty = [&](int s, auto bufc, auto mc) __attribute__((always_inline)) {
        constexpr int m = decltype(mc)::value, nbuf = decltype(bufc)::value ^ 1;
        static_for<WM>([&](auto rc) __attribute__((always_inline)) {
            constexpr int o = m;
            if constexpr (o >= 0 && o < 3) vertical(rc, IC<o>{});
            if constexpr (o >= 3 && o < 3 + 2 * E && ((o - 3) & 1) == 0) horizontal(IC<(o - 3) / 2>{});
            if constexpr (o >= 4 && o < 4 + 2 * E) {
                constexpr int i = (o - 4) / 2, first = (E + 1) / 2;
                if constexpr (((o - 4) & 1) == 0) {
#pragma unroll
                    for (int v = 0; v < first; ++v) store_a(rc, nbuf, E * i + v);
                } else {
#pragma unroll
                    for (int v = first; v < E; ++v) store_a(rc, nbuf, E * i + v);
                }
            }
            constexpr int L = m - Form::REQ0;
            if constexpr (L >= 0 && L < 9) load_raw(s + 2, rc, IC<L>{});
        });
    };

    // ---- B fragments from the transformed filters U[cb][pos][n][8], lane = (n = lane & 31, k half = lane >> 5)
    const int nB = n0 + 32 * ni + (lane & 31);
    const unsigned bvoff = nB < p.N ? (unsigned)(nB * KC + 4 * (lane >> 5)) * 4u : OOB;
    const unsigned bpstride = (unsigned)p.N * KC * 4u;
    float4 fb[Form::BRING];
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.u), 0, (int)p.ubytes, 0x00020000);
    auto load_b = [&](int step, auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        const unsigned so = ((unsigned)step * (unsigned)NP + (unsigned)q) * bpstride;
        fb[Form::cB(q)] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(ru, bvoff, so, 0));
    };
    // ---- A fragments: lane = (tile = lane & 31 of the workgroup's 32, k half = lane >> 5)
    const float *ard = lds + (32 * mi + (lane & 31)) * 8 + 4 * ((lane >> 5) ^ (((lane & 31) >> 3) & 1));
    float4 fa[4];
    auto load_a = [&](int buf, auto qc) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        fa[Form::cA(q)] = *reinterpret_cast<const float4 *>(ard + buf * ABUF + q * APOS);
    };

    f32x16 accV[NVEC ? NVEC : 1];  // positions 16 .. NP - 1, in the vector half of the register file (0..15: a[0:255] by name)
    auto mfma = [&](auto qc, float av, float bv) __attribute__((always_inline)) {
        constexpr int q = decltype(qc)::value;
        if constexpr (q < 16) {
            ACC_MFMA_A(q, av, bv);
        } else {
            f32x16 &ac = accV[q - 16];  // (a reference first: an asm operand alone does not make the lambda capture the array)
            ACC_MFMA_V(ac, av, bv);
        }
    };

    // ---- prologue: requests of step 0, the first B fragments, accumulators, A of step 0, requests of step 1
    static_for<WM>([&](auto rc) __attribute__((always_inline)) {
        static_for<9>([&](auto Lc) __attribute__((always_inline)) { load_raw(s0, rc, Lc); });
    });
    static_for<BPRE>([&](auto qc) __attribute__((always_inline)) { load_b(s0, qc); });
    ACC_CLAIM_ACC();
    static_for<16>([&](auto qc) __attribute__((always_inline)) { ACC_ZERO16(16 * decltype(qc)::value); });
#pragma unroll
    for (int q = 0; q < NVEC; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) accV[q][e] = 0.f;
    static_for<WM>([&](auto rc) __attribute__((always_inline)) {
        static_for<3>([&](auto jc) __attribute__((always_inline)) { vertical(rc, jc); });
        static_for<E>([&](auto ic) __attribute__((always_inline)) { horizontal(ic); });
#pragma unroll
        for (int i = 0; i < NP; ++i) store_a(rc, 0, i);
        static_for<9>([&](auto Lc) __attribute__((always_inline)) { load_raw(s0 + 1, rc, Lc); });
    });
    __syncthreads();
    load_a(0, IC<0>{});
    load_a(0, IC<1>{});

    // ---- K loop: slot m = MFMA k = m % 4 of position q = m / 4, followed by the slot's loads and producer work
    auto kstep = [&](int s, auto bufc) __attribute__((always_inline)) {
        constexpr int buf = decltype(bufc)::value;
        static_for<4 * NP>([&](auto mc) __attribute__((always_inline)) {
            constexpr int m = decltype(mc)::value, q = m / 4, k = m % 4;
            constexpr int ca = Form::cA(q), cb = Form::cB(q);
            const float av = k == 0 ? fa[ca].x : k == 1 ? fa[ca].y : k == 2 ? fa[ca].z : fa[ca].w;
            const float bv = k == 0 ? fb[cb].x : k == 1 ? fb[cb].y : k == 2 ? fb[cb].z : fb[cb].w;
            mfma(IC<q>{}, av, bv);
            if constexpr (k == 0) {
                if constexpr (m == 4 * (NP - 2)) __syncthreads();
                if constexpr (q + 2 < NP) load_a(buf, IC<(q + 2) % NP>{});
                else load_a(buf ^ 1, IC<(q + 2) % NP>{});
            }
            if constexpr (k == 1) {
                if constexpr (q + BPRE < NP) load_b(s, IC<(q + BPRE) % NP>{});
                else load_b(s + 1, IC<(q + BPRE) % NP>{});
            }
            duty(s, bufc, mc);
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    for (int s = s0; s < send; s += 2) {
        kstep(s, IC<0>{});
        kstep(s + 1, IC<1>{});
    }
    // the last MFMAs' results: 18 wait states before anything reads them (hipcc pads nothing behind inline asm)
    int lane2 = lane;
    if constexpr (NVEC == 9)
        asm volatile("s_nop 15\n\ts_nop 7"
                     : "+v"(accV[0]), "+v"(accV[1]), "+v"(accV[2]), "+v"(accV[3]), "+v"(accV[4]), "+v"(accV[5]), "+v"(accV[6]),
                       "+v"(accV[7]), "+v"(accV[8]), "+v"(lane2));
    else asm volatile("s_nop 15\n\ts_nop 7" : "+v"(lane2));

    // ---- epilogue, lane-local: register e of every position belongs to tile (e & 3) + 8 (e >> 2) + 4 (lane >> 5) of the
    // workgroup's 32 and to channel lane & 31: A^T M A on the lane's own NP values, bias, ReLU / mask, nine strided pixels out
    const int n = n0 + 32 * ni + (lane2 & 31);
    // (SPLIT: the slice's partial outputs, no bias, no activation: wino3z_finish_kernel)
    const float bias_v = (!SPLIT && p.bias && n < p.N) ? p.bias[n] : 0.f;
    const float floor_v = (!SPLIT && p.relu) ? 0.f : -__builtin_inff();  // ReLU as one max
    float *ydst = SPLIT ? p.part + (size_t)slice * (p.ybytes / 4) : p.y;
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(ydst, 0, (int)p.ybytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rm =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.mask), 0, MASK ? (int)p.ybytes : 0, 0x00020000);
    unsigned so[9];  // byte offset of output pixel (i, j) of a tile from its pixel (0, 0): so[3 j + i]
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) so[3 * j + i] = (unsigned)((d * i * p.W + d * j) * p.N) * 4u;
    static_for<16>([&](auto ec) __attribute__((always_inline)) {
        constexpr int e = decltype(ec)::value;
        const int t = t0 + 32 * mi + (e & 3) + 8 * (e >> 2) + 4 * (lane2 >> 5);
        const int img = fdiv(t, p.div_tpi), sub = t - img * tpi;
        const int a = fdiv(sub, p.div_d), b = sub - a * d;
        const unsigned voff = (t < p.T && n < p.N) ? (unsigned)(((img * p.H + a) * p.W + b) * p.N + n) * 4u : OOB;
        float mk[9];
        if constexpr (MASK) {
#pragma unroll
            for (int o = 0; o < 9; ++o)
                mk[o] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, voff, so[o], 0));
        }
        float z[E][3];
#pragma unroll
        for (int u = 0; u < E; ++u) {
            float mv[E];
#pragma unroll
            for (int v = 0; v < E; ++v) {
                const int q = E * u + v;
                if (q < 16) ACC_READ_ACC(mv[v], 16 * q + e);
                else mv[v] = accV[q >= 16 ? q - 16 : 0][e];
            }
            Form::at(mv, z[u][0], z[u][1], z[u][2]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float zc[E], yv[3];
#pragma unroll
            for (int u = 0; u < E; ++u) zc[u] = z[u][j];
            Form::at(zc, yv[0], yv[1], yv[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float v = fmaxf(yv[i] + bias_v, floor_v);
                if constexpr (MASK) v = mk[3 * j + i] > 0.f ? v : 0.f;
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), ry, voff, so[3 * j + i], 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // (one register column at a time: hipcc otherwise hoists all NP x 16 reads)
    });
}

// ---- host side: what the two launchers share
using Wino3OneKernel = void (*)(const Wino3OneParams);

// fills everything but the SPLIT fields (one slice); `blocks` = workgroups of the unsplit launch, whole XCD rounds
template <class Form>
inline int wino3_onewave_params(Wino3OneParams &p, long long &blocks, const float *x, int B, int H, int W, int C,
                                const float *u, const float *bias, int relu, float *y, int N, int dilation,
                                const float *mask)
{
    using namespace w3one;
    p.x = x; p.u = u; p.bias = bias; p.mask = mask; p.y = y;
    p.H = H; p.W = W; p.C = C; p.N = N; p.dil = dilation;
    p.T = B * dilation * dilation;
    p.cblocks = C / KC;
    p.nblocks = ceil_div(N, NT);
    p.mblocks = ceil_div(p.T, MT);
    p.relu = relu;
    p.xbytes = (unsigned)((long long)B * H * W * C * 4);
    p.ubytes = (unsigned)((size_t)Form::NP * N * C * 4);
    p.ybytes = (unsigned)((long long)B * H * W * N * 4);
    p.div_tpi = make_fastdiv(dilation * dilation);
    p.div_d = make_fastdiv(dilation);
    p.part = nullptr;
    p.nslices = 1;
    p.steps = p.cblocks;
    blocks = 8LL * ceil_div(p.mblocks, 8) * p.nblocks;
    if (blocks > 0x7fffffffLL) return fail(MPSR_ERR_UNSUPPORTED, "conv3x3_winograd3: grid too large");
    return MPSR_OK;
}

template <class Form>
inline int wino3_onewave_launch(Wino3OneKernel kern, const char *name, const Wino3OneParams &p, long long blocks, hipStream_t s)
{
    using namespace w3one;
    const size_t ldsb = (size_t)2 * Form::NP * MT * KC * sizeof(float);  // two A buffers
    return launch_dynamic_lds(name, kern, dim3((unsigned)blocks), dim3(256), ldsb, s, p);
}

}  // namespace mpsr

// Matrix-pipe microbenchmarks (mpsr_debug_*: tools/mfma_peak.py, bench.py's calibration figure).  They launch no
// convolution; they measure what the MFMA, LDS and dispatch hardware sustain, in the instruction mixes of the implicit
// GEMM's K loop (conv_mfma.hip).
#include "common.h"

namespace {
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int LDS_STRIDE = 32 + 4;  // floats per LDS row, as in conv_mfma.hip
}  // namespace

// ------------------------------------------------------------------------------------------------ calibration
// What this box's matrix pipes sustain in fp32: nothing but v_mfma_f32_32x32x2_f32 on `chains` independent
// accumulators per wave (1 = one dependent chain, like a 32x32 wave tile; 4 = like a 64x64 wave tile).  MI355X boards
// differ in sustained clock under this load by up to ~20 % (power capping), so bench.py and the tuning tools quote
// kernel rates next to this figure measured in the same process, not only next to the 2.4 GHz datasheet peak.
namespace {
template <int CHAINS>
__global__ __launch_bounds__(256) void mfma_peak_kernel(float *out, int iters, float a0, float b0)
{
    f32x16 acc[CHAINS];
#pragma unroll
    for (int c = 0; c < CHAINS; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
    float a = a0 + threadIdx.x * 1e-6f, b = b0;
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int r = 0; r < 16 / CHAINS; ++r)
#pragma unroll
            for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[c], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CHAINS; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) s += acc[c][e];
    if (s == 12345.678f) out[0] = s;  // keeps the chain live; never true for the inputs used
}
}  // namespace

namespace {
// The K loop's instruction mix without its memory traffic: per step 8 ds_read_b128 feeding 16 dependent MFMAs, waits
// placed as hipcc places them in conv_igemm_kernel<64,64> (MODE 1), or reads issued but never waited for (MODE 0).
template <int MODE>
__global__ __launch_bounds__(256) void mfma_lds_kernel(float *out, int iters)
{
    __shared__ __attribute__((aligned(16))) float lds[128 * LDS_STRIDE];
    for (int i = threadIdx.x; i < 128 * LDS_STRIDE; i += 256) lds[i] = 1e-3f * (float)(i & 15);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *Aw = lds + ((wave >> 1) * 32 + (lane & 31)) * LDS_STRIDE + (lane >> 5) * 4;
    const float *Bw = lds + (64 + (wave & 1) * 32 + (lane & 31)) * LDS_STRIDE + (lane >> 5) * 4;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4 keep = {1.f, 1.f, 1.f, 1.f};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            f32x4 a = *reinterpret_cast<const f32x4 *>(Aw + kb * 8 + (i & 1) * 4);
            f32x4 b = *reinterpret_cast<const f32x4 *>(Bw + kb * 8 + (i & 1) * 4);
            if (MODE == 0) {
                asm volatile("" ::"v"(a), "v"(b));
                a = keep;
                b = keep;
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[e];
    if (s == 12345.678f) out[0] = s;
}
}  // namespace

namespace {
// One dependent MFMA chain per wave with NV independent vector-ALU instructions issued after every MFMA: does ordinary
// VALU work of the resident waves take time away from the matrix pipe?  (tools/mfma_peak.py --valu)
template <int NV, int KIND = 0>
__global__ __launch_bounds__(256) void mfma_valu_kernel(float *out, int iters, float av, float bv)
{
    __shared__ __attribute__((aligned(16))) float buf[256 * 4 + 64];
    buf[threadIdx.x * 4] = av;
    __syncthreads();
    const float *lp = buf + (threadIdx.x & 63) * 4;
    __shared__ __attribute__((aligned(16))) float wbuf[256 * 4 + 2048];
    const unsigned wp = (unsigned)(size_t)(wbuf + threadIdx.x), wp2 = (unsigned)(size_t)(wbuf + threadIdx.x * 2),
                   wp4 = (unsigned)(size_t)(wbuf + threadIdx.x * 4);
    __attribute__((ext_vector_type(2))) float w2 = {av, bv};
    int sreg = iters;
    f32x4 lv = {0.f, 0.f, 0.f, 0.f};
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = av * (float)(threadIdx.x + e);
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (KIND == 0) asm volatile("v_fma_f32 %0, %0, %1, %1" : "+v"(v[(u * NV + q) & 15]) : "v"(bv));
                if (KIND == 1) asm volatile("s_add_u32 %0, %0, 1" : "+s"(sreg));
                if (KIND == 2) asm volatile("ds_read_b128 %0, %1" : "=v"(lv) : "v"((unsigned)(size_t)lp) : "memory");
                if (KIND == 3) asm volatile("s_nop 0");
                // LDS stores of this thread's own slot (conflict-free): 4, 8, 16 bytes, and the paired 4-byte form
                if (KIND == 4) asm volatile("ds_write_b32 %0, %1" ::"v"(wp), "v"(v[q & 15]) : "memory");
                if (KIND == 5) asm volatile("ds_write_b64 %0, %1" ::"v"(wp2), "v"(w2) : "memory");
                if (KIND == 6) asm volatile("ds_write_b128 %0, %1" ::"v"(wp4), "v"(lv) : "memory");
                if (KIND == 7) asm volatile("ds_write2st64_b32 %0, %1, %2 offset1:4" ::"v"(wp), "v"(v[q & 15]), "v"(v[(q + 1) & 15]) : "memory");
            }
            if (KIND == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) s += acc[e] + v[e];
    s += lv.x + (float)sreg;
    if (s == 12345.678f) out[0] = s;
}
}  // namespace

namespace {
__global__ __launch_bounds__(256) void empty_kernel(float *out, int spin)
{
    extern __shared__ float dyn[];
    float v = 0.f;
    for (int i = 0; i < spin; ++i) asm volatile("s_sleep 1");
    if (out && threadIdx.x == 1000) out[0] = v + dyn[0];
}
}  // namespace

// Workgroup dispatch rate: `blocks` workgroups of 256 threads with `lds_bytes` of LDS that do nothing (spin = 0) or
// sleep for spin * 64 cycles.
extern "C" int mpsr_debug_dispatch(float *out, int blocks, int lds_bytes, int spin, mpsr_stream_t stream)
{
    MPSR_REQUIRE(blocks > 0 && lds_bytes >= 0 && lds_bytes <= 64 * 1024, "dispatch: bad arguments");
    hipLaunchKernelGGL(empty_kernel, dim3((unsigned)blocks), dim3(256), (size_t)lds_bytes, mpsr::as_stream(stream), out, spin);
    MPSR_CHECK_LAUNCH("empty_kernel");
    return MPSR_OK;
}

// kind 0: vector ALU, 1: scalar ALU, 2: LDS reads (ds_read_b128), 3: s_nop, 4-7: LDS stores (ds_write_b32 / _b64 /
// _b128 / ds_write2st64_b32); nv = 1, 2 (stores only), 4 or 8 of them after every MFMA
extern "C" int mpsr_debug_mfma_mix(float *out, int cus, int waves_per_simd, int nv, int kind, int iters,
                                   mpsr_stream_t stream)
{
    MPSR_REQUIRE(out && cus > 0 && waves_per_simd >= 1 && waves_per_simd <= 8 && iters > 0 &&
                     (nv == 4 || nv == 8 || ((nv == 1 || nv == 2) && kind >= 4)) && kind >= 0 && kind <= 7,
                 "mfma_mix: bad arguments");
    const dim3 grid((unsigned)(cus * waves_per_simd));
    hipStream_t s = mpsr::as_stream(stream);
#define MIX(NV_, K_) hipLaunchKernelGGL((mfma_valu_kernel<NV_, K_>), grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f)
    if (kind >= 4) {
        if (nv == 1) { if (kind == 4) MIX(1, 4); else if (kind == 5) MIX(1, 5); else if (kind == 6) MIX(1, 6); else MIX(1, 7); }
        else if (nv == 2) { if (kind == 4) MIX(2, 4); else if (kind == 5) MIX(2, 5); else if (kind == 6) MIX(2, 6); else MIX(2, 7); }
        else if (nv == 4) { if (kind == 4) MIX(4, 4); else if (kind == 5) MIX(4, 5); else if (kind == 6) MIX(4, 6); else MIX(4, 7); }
        else { if (kind == 4) MIX(8, 4); else if (kind == 5) MIX(8, 5); else if (kind == 6) MIX(8, 6); else MIX(8, 7); }
    } else if (nv == 4) {
        if (kind == 0) MIX(4, 0); else if (kind == 1) MIX(4, 1); else if (kind == 2) MIX(4, 2); else MIX(4, 3);
    } else {
        if (kind == 0) MIX(8, 0); else if (kind == 1) MIX(8, 1); else if (kind == 2) MIX(8, 2); else MIX(8, 3);
    }
#undef MIX
    MPSR_CHECK_LAUNCH("mfma_valu_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_debug_mfma_valu(float *out, int cus, int waves_per_simd, int nv, int iters, mpsr_stream_t stream)
{
    MPSR_REQUIRE(out && cus > 0 && waves_per_simd >= 1 && waves_per_simd <= 8 && iters > 0, "mfma_valu: bad arguments");
    const dim3 grid((unsigned)(cus * waves_per_simd));
    hipStream_t s = mpsr::as_stream(stream);
    switch (nv) {
    case 0: hipLaunchKernelGGL(mfma_valu_kernel<0>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 1: hipLaunchKernelGGL(mfma_valu_kernel<1>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 2: hipLaunchKernelGGL(mfma_valu_kernel<2>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 4: hipLaunchKernelGGL(mfma_valu_kernel<4>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 6: hipLaunchKernelGGL(mfma_valu_kernel<6>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 8: hipLaunchKernelGGL(mfma_valu_kernel<8>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 12: hipLaunchKernelGGL(mfma_valu_kernel<12>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    case 16: hipLaunchKernelGGL(mfma_valu_kernel<16>, grid, dim3(256), 0, s, out, iters, 1.f, 1e-3f); break;
    default: return mpsr::fail(MPSR_ERR_INVALID_ARG, "mfma_valu: nv must be 0, 1, 2, 4, 6, 8, 12 or 16");
    }
    MPSR_CHECK_LAUNCH("mfma_valu_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_debug_mfma_lds(float *out, int cus, int waves_per_simd, int mode, int iters, mpsr_stream_t stream)
{
    MPSR_REQUIRE(out && cus > 0 && waves_per_simd >= 1 && waves_per_simd <= 8 && iters > 0, "mfma_lds: bad arguments");
    const dim3 grid((unsigned)(cus * waves_per_simd));
    if (mode == 0) hipLaunchKernelGGL(mfma_lds_kernel<0>, grid, dim3(256), 0, mpsr::as_stream(stream), out, iters);
    else hipLaunchKernelGGL(mfma_lds_kernel<1>, grid, dim3(256), 0, mpsr::as_stream(stream), out, iters);
    MPSR_CHECK_LAUNCH("mfma_lds_kernel");
    return MPSR_OK;
}

// Launches `waves_per_simd` waves on every SIMD of `cus` CUs, each issuing iters * 16 MFMAs.  The caller times it
// (FLOP = cus * 4 * waves_per_simd * iters * 16 * 4096).
extern "C" int mpsr_debug_mfma_peak(float *out, int cus, int waves_per_simd, int chains, int iters, mpsr_stream_t stream)
{
    MPSR_REQUIRE(out && cus > 0 && waves_per_simd >= 1 && waves_per_simd <= 8 && iters > 0 && (chains == 1 || chains == 4),
                 "mfma_peak: bad arguments");
    const dim3 grid((unsigned)(cus * waves_per_simd));
    if (chains == 1) hipLaunchKernelGGL(mfma_peak_kernel<1>, grid, dim3(256), 0, mpsr::as_stream(stream), out, iters, 1.f, 1e-3f);
    else hipLaunchKernelGGL(mfma_peak_kernel<4>, grid, dim3(256), 0, mpsr::as_stream(stream), out, iters, 1.f, 1e-3f);
    MPSR_CHECK_LAUNCH("mfma_peak_kernel");
    return MPSR_OK;
}

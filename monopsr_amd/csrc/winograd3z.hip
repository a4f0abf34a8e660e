// The atrous 3x3 layers whose pixel sub-grids are single 3x3 tiles (ResNet-101 block3's conv2 at output stride 4: 12x12
// maps, dilation 4, 23 launches per step; reference graph object_detection/nets/resnet_v1.py:116-127,
// resnet_utils.py:194-196) in SIXTEEN products per (channel pair, tile).
//
// Such a sub-grid reads nothing outside itself (everything a tap reaches beyond it is SAME-padding zeros), so in one
// dimension its outputs are the MIDDLE three coefficients of the product of two quadratics -- a bilinear map of rank 4,
// not the 5 that F(3,3) spends on a general 5-point input (derivation, matrices and error: wino3_transforms.h).  Nested
// in two dimensions: Y (3x3) = A^T [ sum_c (G g G^T) (.) (B^T d B) ] A with 4x4 = 16 element positions where
// F(3x3,3x3) (winograd3.hip, winograd3w.hip) has 25 and the direct form 81; transform constants 2, 3/2, 1/2: the fp32
// error of a direct convolution (5e-7 of the tensor scale, 1.8e-4 element-wise on heavy-tailed maps, where F(3x3,3x3)
// measures 4e-6 / 1.2e-3).  36 % fewer MFMAs, a cheaper input transform (42 operations + 16 LDS stores per patch instead of
// 56 + 25), and 16 x 16 = 256 accumulator registers: exactly the accumulator half of the register file.
//
// Kernel = the sixteen-product form of wino3_onewave.h: ONE WAVE OWNS ALL 16 POSITIONS of its (32 tiles x 32 output
// channels) block, all of them under literal names in the accumulator half of the register file; K step = 64 MFMAs per
// wave, the barrier at slot 56, the producer's stores in slots 4-11, the requests from slot 16 on; A ring colours
// 0 1 2 x 4, then 0 1 2 3, B fragments seven positions ahead in a ring of eight.
//
// SPLIT instantiation (small batches: the reference's 32 boxes per image).  A wave's K loop is 2048 MFMAs long whatever
// the batch, so a launch that cannot fill the chip takes ~76 us at ANY batch up to 128 (32 workgroups at B = 32).  There
// the channel range is cut into slices: workgroup (tile block, channel block, slice) runs K / slices channels and stores
// its PARTIAL 3x3 outputs (the output transform is linear) into its slice of a scratch tensor; a second small launch adds
// the slices in a fixed order, applies bias / ReLU and writes y -- deterministic, no atomics, no zero-fill.
#include <atomic>

#include "common.h"
#include "wino3_filter.h"
#include "wino3_onewave.h"
#include "wino3_transforms.h"

namespace {

struct FormZ16 {
    static constexpr int NP = 16, E = 4, COL0 = 0, REQ0 = 16;
    static constexpr bool HAS_SPLIT = true;
    static constexpr int cA(int p) { return p < 12 ? p % 3 : p - 12; }  // ring colour of position p's A fragment (4 quads)
    static constexpr int BPRE = 7, BRING = 8;  // B fragments requested this many positions ahead (28 MFMAs), ring of eight: 16 = 8 + 8
    static constexpr int cB(int p) { return p % 8; }  // ... of its B fragment
    template <int S>
    static __device__ __forceinline__ void bt(float a, float b, float c, float *o)
    {
        mpsr::w3t::bt4z(a, b, c, o[0], o[S], o[2 * S], o[3 * S]);
    }
    static __device__ __forceinline__ void at(const float *m, float &y0, float &y1, float &y2)
    {
        mpsr::w3t::at3z(m[0], m[1], m[2], m[3], y0, y1, y2);
    }
};

template <bool MASK, bool SPLIT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wino3z_conv_kernel(const mpsr::Wino3OneParams p)
{
    mpsr::wino3_onewave_body<FormZ16, MASK, SPLIT>(p);
}

}  // namespace

namespace {
// the filter transform of this form as a launch of its own (when no cache / tail job made it)
__global__ __launch_bounds__(256) void wino3z_filter_kernel(const float *__restrict__ w, int N, int C, float *__restrict__ u)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)N * C) mpsr::wino3z_filter_one(w, N, C, u, i);
}
}  // namespace

namespace {
// y = act(bias + sum of the K slices' partial outputs), slices added in index order; 16 bytes per thread
__global__ __launch_bounds__(256) void wino3z_finish_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                            float *__restrict__ y, long long total4, long long slice4,
                                                            int nslices, int N4, int relu)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    float4 a = reinterpret_cast<const float4 *>(part)[i];
    for (int k = 1; k < nslices; ++k) {
        const float4 b = reinterpret_cast<const float4 *>(part)[i + k * slice4];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (bias) {
        const float4 b = reinterpret_cast<const float4 *>(bias)[i % N4];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (relu) a = make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f));
    reinterpret_cast<float4 *>(y)[i] = a;
}
}  // namespace

namespace mpsr {

static std::atomic<int> g_w3z_split{-1};  // mpsr_debug_set_wino3z_split: -1 by launch size, 0 never, k > 1 = k slices

// K slices of a launch: enough workgroups for every CU (up to `want_blocks`), at least `min_steps` channel steps each
// and an even number of them, a power of two that divides the steps; 1 = not split.  (Depends on the batch only through
// the workgroup count rounded up to whole XCD rounds.)  Shared with the F(2x2,3x3) kernel (winograd.hip).
int winograd_slices(long long blocks, int want_blocks, int cblocks, int min_steps, size_t part_floats, size_t y_floats)
{
    const int forced = g_w3z_split.load();
    if (forced == 0 || (y_floats & 3)) return 1;
    int s = 1;
    if (forced > 1) s = forced;
    else
        while (blocks * s * 2 <= want_blocks && s < 16) s *= 2;
    while (s > 1 && (cblocks % (2 * s) != 0 || cblocks / s < min_steps || (size_t)s * y_floats > part_floats)) s /= 2;
    return s;
}

int winograd_finish_slices(const float *part, const float *bias, float *y, size_t y_floats, int nslices, int N, int relu,
                           hipStream_t s)
{
    const long long total4 = (long long)(y_floats / 4);
    hipLaunchKernelGGL(wino3z_finish_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, part, bias, y, total4,
                       total4, nslices, N / 4, relu);
    MPSR_CHECK_LAUNCH("wino3z_finish_kernel");
    return MPSR_OK;
}

// launches the kernel on filters already transformed by wino3z_filter_one (wino3_filter.h: U[cb][16 positions][n][8])
int launch_winograd3z(const float *x, int B, int H, int W, int C, const float *u, const float *bias, int relu, float *y,
                      int N, int dilation, hipStream_t s, const float *mask, float *part, size_t part_floats)
{
    Wino3OneParams p;
    long long blocks;
    if (int rc = wino3_onewave_params<FormZ16>(p, blocks, x, B, H, W, C, u, bias, relu, y, N, dilation, mask)) return rc;
    const size_t y_floats = (size_t)B * H * W * N;
    const bool splittable = part && N % 4 == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)part & 15) == 0 &&
                            (!bias || ((uintptr_t)bias & 15) == 0);
    p.nslices = mask ? 1 : winograd_slices(blocks, 256, p.cblocks, 4, splittable ? part_floats : 0, y_floats);
    p.steps = p.cblocks / p.nslices;
    p.part = part;
    if (p.nslices > 1) {
        if (int rc = wino3_onewave_launch<FormZ16>(wino3z_conv_kernel<false, true>, "wino3z_conv_kernel", p,
                                                   blocks * p.nslices, s))
            return rc;
        return winograd_finish_slices(part, bias, y, y_floats, p.nslices, N, relu, s);
    }
    return wino3_onewave_launch<FormZ16>(mask ? wino3z_conv_kernel<true> : wino3z_conv_kernel<false>, "wino3z_conv_kernel",
                                         p, blocks, s);
}

int launch_winograd3z_filter(const float *w, int N, int C, float *u, hipStream_t s)
{
    const long long total = (long long)N * C;
    hipLaunchKernelGGL(wino3z_filter_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, N, C, u);
    MPSR_CHECK_LAUNCH("wino3z_filter_kernel");
    return MPSR_OK;
}

}  // namespace mpsr

extern "C" void mpsr_debug_set_wino3z_split(int slices) { mpsr::g_w3z_split = slices; }


// Winograd F(3x3,3x3) for the atrous 3x3 layers whose pixel sub-grids are single 3x3 tiles (reference graph
// object_detection/nets/resnet_v1.py:116-127, resnet_utils.py:194-196), in the form where ONE WAVE OWNS ALL 25 POSITIONS
// of its (32 tiles x 32 output channels) block: the F(3x3,3x3) form of wino3_onewave.h, which holds the kernel.
//
// 25 x 16 = 400 accumulator registers: 16 positions in the accumulator half of the register file, 9 in the vector half.
// The 56 vector instructions + 25 LDS stores of a patch are amortised over 128 output channels (1 patch per 100 MFMAs
// against 1 per 52 in winograd3.hip) and each wave issues 4x the MFMAs per epilogue.  Same transformed filters and the
// same accumulation order per output as winograd3.hip: the two kernels return identical bits.
//
// K step = 100 MFMAs, the barrier at slot 92, the producer's stores in slots 4..13, the requests from slot 30 on.  A ring:
// 25 is not a multiple of 3, the colours are 0 1 2 x 7, then 0 1 2 3.  B fragments seven positions (28 MFMAs, ~1800
// cycles) ahead in a ring of nine (colours 0..7, 0..7, 0..8).
#include "common.h"
#include "wino3_onewave.h"
#include "wino3_transforms.h"

namespace {

struct FormF33 {
    static constexpr int NP = 25, E = 5, COL0 = 1, REQ0 = 30;
    static constexpr bool HAS_SPLIT = false;
    static constexpr int cA(int p) { return p < 21 ? p % 3 : p - 21; }  // ring colour of position p's A fragment (4 quads)
    // B fragments requested this many positions ahead (28 MFMAs), ring of nine: 25 = 8 + 8 + 9.  Four ahead is late inside
    // a step, eleven measured equal
    static constexpr int BPRE = 7, BRING = 9;
    static constexpr int cB(int p) { return p < 16 ? p % 8 : p - 16; }  // ... of its B fragment
    template <int S>
    static __device__ __forceinline__ void bt(float a, float b, float c, float *o)
    {
        mpsr::w3t::bt5(a, b, c, o[0], o[S], o[2 * S], o[3 * S], o[4 * S]);
    }
    static __device__ __forceinline__ void at(const float *m, float &y0, float &y1, float &y2)
    {
        mpsr::w3t::at3(m[0], m[1], m[2], m[3], m[4], y0, y1, y2);
    }
};

template <int WM, bool MASK>  // WM = 1: 32 tiles x 128 channels per workgroup, the only shape that can run (wino3_onewave.h)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void wino3w_conv_kernel(const mpsr::Wino3OneParams p)
{
    static_assert(WM == 1);
    mpsr::wino3_onewave_body<FormF33, MASK, false>(p);
}

}  // namespace

namespace mpsr {

// the one-wave-per-tile-block form applies where a sub-grid is one tile (th == 1); worth it once its workgroups fill the chip
bool winograd3w_applies(int B, int H, int W, int C, int N, int dilation)
{
    return dilation >= 1 && H == W && H == 3 * dilation && C % 16 == 0 && C >= 16 && N >= 1 &&
           (long long)B * H * W * N * 4 < 0x7ff00000LL;
}

// workgroups of a launch (32 tiles x 128 channels each)
long long winograd3w_workgroups(int B, int N, int dilation)
{
    return (long long)ceil_div(B * dilation * dilation, 32) * ceil_div(N, 128);
}

// launches the kernel on already transformed filters `u` (layout of wino3_filter.h)
int launch_winograd3w(const float *x, int B, int H, int W, int C, const float *u, const float *bias, int relu, float *y,
                      int N, int dilation, hipStream_t s, const float *mask)
{
    Wino3OneParams p;
    long long blocks;
    if (int rc = wino3_onewave_params<FormF33>(p, blocks, x, B, H, W, C, u, bias, relu, y, N, dilation, mask)) return rc;
    return wino3_onewave_launch<FormF33>(mask ? wino3w_conv_kernel<1, true> : wino3w_conv_kernel<1, false>,
                                         "wino3w_conv_kernel", p, blocks, s);
}

}  // namespace mpsr

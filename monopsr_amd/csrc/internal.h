// Everything that crosses a translation unit inside libmonopsr_hip.so without being part of the C ABI
// (include/monopsr_hip.h): each function and each variable is declared here once, grouped by the file that defines it,
// and default arguments live here only.  Included through common.h, which every .hip includes; no .hip declares
// another file's function or an `extern` of its own (tests/test_internal_header.py).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>

#include "monopsr_hip.h"

namespace mpsr {

// ---- api.hip
// Thread-local last-error buffer behind mpsr_last_error().
char *error_buffer();
// Per-call overrides of the process-wide arithmetic mode / Winograd policy (mpsr_net_opts.math / .winograd_policy,
// mpsr_conv2d_nhwc_f32_ex): an entry point runs on its caller's thread from start to end, so a thread-local set for
// the duration of the call IS per call, and two threads with different options never see each other's.  -1 = none.
// (set by common.h's CallOptsGuard)
extern thread_local int t_call_math;
extern thread_local int t_call_wino_policy;

// ---- per-layer arguments of the convolution launchers
// What a network-level entry point (network.hip) knows about one layer beyond its tensors, passed down through conv2d()
// as `LayerExtras *` (nullptr: nothing): a launcher without the argument, or a caller that passes none, sees none of it.
//
// A filter-transform job that a 1x1 layer's launch carries behind its own tiles (wino3_filter.h): the filters of the
// 3x3 layer that follows.
struct FilterTailJob {
    const float *w = nullptr;  // nullptr: no job
    float *u = nullptr;
    int N = 0, C = 0;
    int form = 0;  // 0: F(3x3,3x3), 25 positions (wino3_filter_one); 1: the sixteen-product form (wino3z_filter_one)
};
// The slice of the caller's filter cache (mpsr_net_opts.filter_cache) that belongs to a 3x3 layer: the Winograd launchers
// and conv3x3_upsampled then keep the transformed filters in `u` instead of their scratch and skip the transform when the
// slice already holds them.
struct FilterCacheSlot {
    const float *w = nullptr;
    float *u = nullptr;  // nullptr: no slice
    size_t floats = 0;
    bool ready = false;  // the caller vouches for the slices (mpsr_net_opts.filter_cache_valid)
    int *tag = nullptr;  // caller's note of what the slice holds (mpsr_net_opts.filter_cache_tags), or nullptr
    // true when the slice already holds form `kind` of this layer's filters; notes `kind` for the next call either way
    // (the consumer is about to write it if not)
    bool holds(int kind) const
    {
        const bool ok = ready && (!tag || *tag == kind);
        if (tag) *tag = kind;
        return ok;
    }
};
enum { FILTER_FORM_WINO4 = 1, FILTER_FORM_WINO3 = 2, FILTER_FORM_UPCONV = 3, FILTER_FORM_WINO3Z = 4, FILTER_FORM_WINO2 = 5 };
struct LayerExtras {
    // 3x3 layers (conv2d()'s three Winograd branches, conv3x3_upsampled)
    FilterCacheSlot cache;
    const float *filters_at = nullptr;  // an earlier launch's tail job already wrote the form this call reads there
    // 1x1 layers (conv2d()'s conv1x1_pointwise branch)
    FilterTailJob tail;       // in: a job to append to this launch
    bool tail_taken = false;  // out: the launch carried it
};
// Where a 3x3 layer's transformed filters live: `need` floats of form `form` (FILTER_FORM_*) of the filters `w`.
//   u:     the cache slice if `ex` offers one for `w` that is large enough (its tag then notes `form`), else `ws`
//   ready: `u` already holds them -- a slice the caller vouches for, tagged `form`, or the address a tail job wrote
//   rest:  what is left of `ws` for other scratch: behind the filters when they live there, else all of it
// (whether `ws` itself holds `need` floats is the caller's check)
struct FilterPlace {
    float *u;
    bool ready;
    float *rest;
    size_t rest_floats;
};
inline FilterPlace place_filters(const LayerExtras *ex, const float *w, size_t need, int form, float *ws, size_t ws_floats)
{
    FilterPlace f{ws, false, ws, ws_floats};
    if (ex && ex->cache.w == w && ex->cache.u && ex->cache.floats >= need) {
        f.u = ex->cache.u;
        f.ready = ex->cache.holds(form);
    } else {
        const size_t off = (need + 63) / 64 * 64;
        f.rest = ws ? ws + off : nullptr;
        f.rest_floats = ws && ws_floats > off ? ws_floats - off : 0;
    }
    if (ex && ex->filters_at && ex->filters_at == f.u) f.ready = true;
    return f;
}

// ---- conv_mfma.hip
int conv2d(const float *x, int B, int H, int W, int C, const float *w, const float *bias, const float *residual,
           float *y, int N, int KH, int KW, int dilation, int relu, int split_k, float *ws, size_t ws_floats,
           hipStream_t stream, LayerExtras *ex = nullptr);
size_t conv_scratch_floats(long long M, int N);
bool conv2d_takes_winograd4(int B, int H, int W, int C, int N, const float *ws, size_t ws_floats);
bool conv2d_takes_winograd3(int B, int H, int W, int C, int N, int KH, int KW, int dilation, int split_k, const float *ws,
                            size_t ws_floats);
bool conv2d_takes_pointwise(long long M, int C, int N, int KH, int KW, int split_k);
int conv2d_winograd_choice(int B, int H, int W, int C, int N, int KH, int KW, int dilation, bool residual, int split_k,
                           const float *ws, size_t ws_floats);

// ---- image_ops.hip
int conv3x3_narrow(const float *x, int B, int H, int W, int C, const float *w, const float *bias, int relu, float *y,
                   int N, hipStream_t s, int in_c8);
bool conv3x3_narrow_takes_mfma(const float *x, int B, int H, int W, int C, int N, const float *w);
int resize_bilinear_c8(const float *in, int B, int H, int W, int C, int OH, int OW, int align_corners, float *out,
                       hipStream_t s);

// ---- winograd.hip
size_t winograd_scratch_floats(int C, int N);
bool winograd_applies(int H, int W, int C, int N);
bool winograd_applies_dilated(int H, int W, int C, int N, int dilation);
int conv3x3_winograd(const float *x, int B, int H, int W, int C, const float *w, const float *bias, int relu, float *y,
                     int N, float *ws, size_t ws_floats, hipStream_t s, int dilation, LayerExtras *ex = nullptr);
extern std::atomic<int> g_wino_waves;  // mpsr_debug_set_wino_waves

// ---- winograd4.hip
size_t winograd4_scratch_floats(int C, int N);
bool winograd4_applies(int H, int W, int C, int N);
int conv3x3_winograd4(const float *x, int B, int H, int W, int C, const float *w, const float *bias, int relu,
                      float *y, int N, float *ws, size_t ws_floats, hipStream_t s, int in_c8, int out_c8, float *part,
                      size_t part_floats, LayerExtras *ex = nullptr);
size_t winograd4_split_floats(int B, int H, int W, int N);
extern std::atomic<int> g_wino4_split;  // mpsr_debug_set_wino4_split

// ---- winograd3.hip
size_t winograd3_scratch_floats(int C, int N);
bool winograd3_applies(int H, int W, int C, int dilation);
double winograd3_executed_flops(int B, int H, int C, int N, int dilation);
int winograd3_form(int B, int H, int W, int C, int N, int dilation);
int winograd3_filter_form(int B, int H, int W, int C, int N, int dilation);
int conv3x3_winograd3(const float *x, int B, int H, int W, int C, const float *w, const float *bias, int relu,
                      float *y, int N, int dilation, float *ws, size_t ws_floats, hipStream_t s,
                      const float *mask = nullptr, LayerExtras *ex = nullptr);

// ---- winograd3w.hip: the layer of winograd3.hip with one wave owning all 25 positions of its tile block
bool winograd3w_applies(int B, int H, int W, int C, int N, int dilation);
long long winograd3w_workgroups(int B, int N, int dilation);
int launch_winograd3w(const float *x, int B, int H, int W, int C, const float *u, const float *bias, int relu, float *y,
                      int N, int dilation, hipStream_t s, const float *mask);

// ---- winograd3z.hip: the same layer in SIXTEEN products per tile (a one-tile sub-grid reads nothing outside itself: rank 4
// per dimension instead of F(3,3)'s 5), one wave owning all 16 positions of its tile block
int launch_winograd3z(const float *x, int B, int H, int W, int C, const float *u, const float *bias, int relu, float *y,
                      int N, int dilation, hipStream_t s, const float *mask, float *part, size_t part_floats);
int launch_winograd3z_filter(const float *w, int N, int C, float *u, hipStream_t s);
// K slices of a small launch and the launch that adds them (also winograd.hip's F(2x2,3x3) kernel and pointwise.hip's
// K-split few-row kernel)
int winograd_slices(long long blocks, int want_blocks, int cblocks, int min_steps, size_t part_floats, size_t y_floats);
int winograd_finish_slices(const float *part, const float *bias, float *y, size_t y_floats, int nslices, int N, int relu,
                           hipStream_t s);

// ---- winograd4_wgrad.hip: the tile slices of the two transform-domain weight gradients (launchers and
// mpsr_conv2d_wgrad_plan): `nslices` slices of `steps` K steps of kt tiles cover `tiles` tiles
struct WgradSlices {
    int tiles, steps, nslices;
};
WgradSlices wgrad_tile_slices(int tiles, int blocks, int workgroups, int kt);

// ---- winograd3_wgrad.hip: the atrous layers whose pixel sub-grids are single 3x3 tiles (block3's conv2)
bool winograd3_wgrad_applies(int B, int H, int W, int C, int N, int KH, int KW, int dilation);
WgradSlices winograd3_wgrad_slices(int B, int dilation, int C, int N);
int conv3x3_wgrad_winograd3(const float *x, const float *dy, int B, int H, int W, int C, int N, int dilation, float *dw,
                            float *db, hipStream_t s);

// ---- pointwise.hip
bool pointwise_applies(long long M, int K, int N);
bool pointwise_masked_applies(long long M, int K, int N);
int pointwise_override();
int conv1x1_pointwise(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                      int relu, float *y, int N, hipStream_t s, LayerExtras *ex = nullptr);
int conv1x1_pointwise_masked(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                             const unsigned *mask, float *y, int N, hipStream_t s);
int conv1x1_pointwise_emit(const float *x, long long M, int K, const float *w, const float *bias, const float *residual,
                           int relu, float *y, unsigned *bits, int N, hipStream_t s);
bool fc_rows_applies(long long M, int K, int N);
bool fc_rows_split_applies(long long M, int K, int N, const float *bias, const float *y, const float *ws, size_t ws_floats);
int fc_rows_split(const float *x, long long M, int K, const float *w, const float *bias, int relu, float *y, int N,
                  float *ws, hipStream_t s);
int fc_rows(const float *x, long long M, int K, const float *w, const float *bias, const float *residual, int relu,
            float *y, int N, hipStream_t s);

// ---- backward.hip
// The argument checks of mpsr_conv2d_wgrad_f32 and the kernel that serves the shape there: 0 = conv_wgrad_kernel, 1 =
// pw_wgrad_direct_kernel, 2 = thin_wgrad (dy_aligned: dy sits on a 16-byte boundary).  The entry point and
// mpsr_conv2d_wgrad_plan both go through it.
int conv2d_wgrad_direct_plan(int B, int H, int W, int C, int N, int KH, int KW, int dilation, bool dy_aligned, int *kind);

// ---- thin_conv.hip
bool thin_input_conv_applies(int B, int H, int W, int C, int N, int KH, int KW, int dilation);
int thin_input_conv(const float *x, int B, int H, int W, const float *w, const float *bias, int relu, float *y, int N,
                    hipStream_t s);
bool thin_wgrad_applies(int B, int H, int W, int C, int N, int KH, int KW, int dilation);
int thin_wgrad(const float *x, const float *dy, int B, int H, int W, int C, float *dw, float *db, hipStream_t s);

// ---- upconv.hip: 3x3 convolution of a bilinearly upsampled map as a low-resolution tap GEMM + gather
bool upconv_applies(int B, int h, int w, int C, int OH, int OW, int N, int align_corners);
size_t upconv_z_floats(long long Msrc, int N);
size_t upconv_weight_floats(int C, int N);
int conv3x3_upsampled(const float *x, int B, int h, int w, int C, int OH, int OW, int align_corners, const float *g,
                      const float *bias, int relu, float *y, int N, int out_c8, float *z, size_t z_floats, float *ws,
                      size_t ws_floats, hipStream_t s, LayerExtras *ex = nullptr);

}  // namespace mpsr

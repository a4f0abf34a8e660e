// LiDAR depth maps on the device: the projection of velodyne clouds into image 2 (depth_map_utils.py:305-348, as
// demos/depth_completion/save_lidar_depth_maps.py calls it) and IP-Basic's multi-scale completion
// (src/ip_basic/ip_basic.py:40-193), for batches of frames that share one image size.
//
// mpsr_lidar_project_depths: one thread per point computes, in fp64 without contraction, velodyne -> cam0 -> pixel and
//   raises the pixel's point index with an int atomicMax (numpy's fancy assignment keeps the LAST duplicate); a second
//   kernel writes max_depth - max(0, max_depth - z) of that point, rounded once to float32.  No float atomics.
// mpsr_depth_fill_multiscale: a chain of stencil kernels over (frame, pixel), every frame of the batch in each launch:
//   s1 + s2 (bin masks, inversion, three masked dilations with the caller's kernels), the 5x5 closing as four separable
//   max / min passes, the 5x5 median (25 values in registers, exact rank selection), the top-row column scans, the 9x9
//   hole fill and the six masked 5x5 dilations as separable passes with a select epilogue, the final median, an exact
//   per-frame min / max (int atomics on order-preserving keys), the bilateral colour table per frame and the bilateral
//   (table in LDS) or gaussian (row pass, then column pass) blur fused with the s8 inversion.
// Every selection stage (max, min, median) is exact; the blurs follow tests/cv2_standin.py's arithmetic order.
#include "common.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = MPSR_DEPTH_MAX_KERNEL;
constexpr int kLut = 4096 + 2;           // kExpNumBins + 2 (bilateralFilter_32f)
constexpr int kBilateralPixels = 8;      // pixels per thread of the bilateral kernel (the table load is per block)
constexpr int kBilateralTaps = 13;       // radius 2: (i, j) with i^2 + j^2 <= 4
constexpr double kColorCoeff = -0.5 / (0.5 * 0.5);  // -0.5 / sigmaColor^2, sigmaColor = 0.5
constexpr double kSpaceCoeff = -0.5 / (2.0 * 2.0);  // -0.5 / sigmaSpace^2, sigmaSpace = 2.0

struct Plane {  // frame f of a plane lives at p + f * fs
    float *p;
    long long fs;
};

struct Taps {
    int n[3];
    signed char dy[3][kMaxK * kMaxK], dx[3][kMaxK * kMaxK];
};

struct BilateralTaps {
    int dy[kBilateralTaps], dx[kBilateralTaps];
    float w[kBilateralTaps];
};

__device__ __forceinline__ float s1_of(float v, float md) { return v > 0.1f ? md - v : v; }

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// ---------------------------------------------------------------------------------------------------- projection

__device__ __forceinline__ void rows3(const double *m, double x, double y, double z, double *o)
{
    for (int r = 0; r < 3; ++r) o[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

__global__ void __launch_bounds__(kThreads) project_scatter_kernel(const float *__restrict__ pts,
                                                                   const long long *__restrict__ offs,
                                                                   const double *__restrict__ velo_to_cam0,
                                                                   const double *__restrict__ p2, int h, int w,
                                                                   int *__restrict__ last)
{
    const int f = blockIdx.y;
    const long long p0 = offs[f], n = offs[f + 1] - p0;
    const double *T = velo_to_cam0 + 12 * f, *P = p2 + 12 * f;
    int *lf = last + (long long)f * h * w;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
        const float *q = pts + 4 * (p0 + j);
        double c[3], u[3];
        rows3(T, (double)q[0], (double)q[1], (double)q[2], c);
        rows3(P, c[0], c[1], c[2], u);
        const double col = rint(u[0] / u[2]), row = rint(u[1] / u[2]);
        // NaN fails every comparison; +-inf fails the range test
        if (col >= 0.0 && col < (double)w && row >= 0.0 && row < (double)h)
            atomicMax(lf + (long long)row * w + (long long)col, (int)j);
    }
}

__global__ void __launch_bounds__(kThreads) project_write_kernel(const float *__restrict__ pts,
                                                                 const long long *__restrict__ offs,
                                                                 const double *__restrict__ velo_to_cam0,
                                                                 const int *__restrict__ last, long long hw,
                                                                 double max_depth, float *__restrict__ out)
{
    const int f = blockIdx.y;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const int j = last[f * hw + i];
    float v = 0.0f;
    if (j >= 0) {
        const float *q = pts + 4 * (offs[f] + j);
        const double *T = velo_to_cam0 + 12 * f;
        const double z = ((T[8] * (double)q[0] + T[9] * (double)q[1]) + T[10] * (double)q[2]) + T[11];
        const double inv = max_depth - z;
        v = (float)(max_depth - (inv > 0.0 ? inv : 0.0));  // python max(0.0, inv)
    }
    out[f * hw + i] = v;
}

// ---------------------------------------------------------------------------------------------------- completion

// s1 (inversion) and s2 (three binned, masked dilations combined far -> med -> near); the bins are tested on the input.
__global__ void __launch_bounds__(kThreads) stage12_kernel(const float *__restrict__ in, int h, int w, float md,
                                                           Taps taps, Plane s1, Plane s2)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *src = in + f * hw;
    const int y = (int)(i / w), x = (int)(i % w);
    const float v = s1_of(src[i], md);
    float d[3];
    for (int b = 0; b < 3; ++b) {  // 0 far (> 30), 1 med (15, 30], 2 near (0.1, 15]
        float m = -FLT_MAX;        // cv2.dilate's default border value: the border takes no part
        for (int t = 0; t < taps.n[b]; ++t) {
            const int yy = y + taps.dy[b][t], xx = x + taps.dx[b][t];
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const float e = src[(long long)yy * w + xx];
            const bool in_bin = b == 0 ? e > 30.0f : (b == 1 ? (e > 15.0f && e <= 30.0f) : (e > 0.1f && e <= 15.0f));
            m = fmaxf(m, in_bin ? md - e : 0.0f);
        }
        d[b] = m;
    }
    float o = v;
    for (int b = 0; b < 3; ++b)
        if (d[b] > 0.1f) o = d[b];
    s1.p[f * s1.fs + i] = v;
    s2.p[f * s2.fs + i] = o;
}

enum { EPI_PLAIN = 0, EPI_HOLE = 1, EPI_EMPTY = 2 };

// One separable pass of a full (2r+1) window: max (dilate) or min (erode) over the in-image neighbours along x or y.
// Epilogues: EPI_HOLE  out = (!(orig > 0.1) && row >= top[col]) ? m : orig        (s5 hole fill)
//            EPI_EMPTY out = (orig < 0.1 && (top == null || row >= top[col])) ? m : orig   (s7 masked dilation)
// orig and dst may be the same plane: each thread reads and writes only its own pixel of them.
__global__ void __launch_bounds__(kThreads) sep_kernel(Plane src, int h, int w, int r, int along_y, int is_max,
                                                       int epi, Plane orig, const int *__restrict__ top, Plane dst)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *s = src.p + f * src.fs;
    const int y = (int)(i / w), x = (int)(i % w);
    float m = is_max ? -FLT_MAX : FLT_MAX;
    if (along_y) {
        for (int k = max(0, y - r); k <= min(h - 1, y + r); ++k) {
            const float e = s[(long long)k * w + x];
            m = is_max ? fmaxf(m, e) : fminf(m, e);
        }
    } else {
        for (int k = max(0, x - r); k <= min(w - 1, x + r); ++k) {
            const float e = s[(long long)y * w + k];
            m = is_max ? fmaxf(m, e) : fminf(m, e);
        }
    }
    if (epi != EPI_PLAIN) {
        const float o = orig.p[f * orig.fs + i];
        const bool below = top == nullptr || y >= top[(long long)f * w + x];
        const bool empty = epi == EPI_HOLE ? !(o > 0.1f) : o < 0.1f;
        m = (empty && below) ? m : o;
    }
    dst.p[f * dst.fs + i] = m;
}

// dst = (src > 0.1 && (top == null || row >= top[col])) ? median5x5(src) : src, BORDER_REPLICATE.  The median is the
// value whose rank range [#less, #less-or-equal) holds 12: the 13th of 25, as a sorting network gives it.
__global__ void __launch_bounds__(kThreads) median_kernel(Plane src, int h, int w, const int *__restrict__ top,
                                                          Plane dst)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *s = src.p + f * src.fs;
    const int y = (int)(i / w), x = (int)(i % w);
    const float c = s[i];
    float o = c;
    if (c > 0.1f && (top == nullptr || y >= top[(long long)f * w + x])) {
        float v[25];
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const long long row = (long long)min(max(y + dy - 2, 0), h - 1) * w;
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) v[dy * 5 + dx] = s[row + min(max(x + dx - 2, 0), w - 1)];
        }
        float med = v[0];
#pragma unroll
        for (int a = 0; a < 25; ++a) {
            int lt = 0, le = 0;
#pragma unroll
            for (int b = 0; b < 25; ++b) {
                lt += v[b] < v[a];
                le += v[b] <= v[a];
            }
            med = (lt <= 12 && le >= 13) ? v[a] : med;
        }
        o = med;
    }
    dst.p[f * dst.fs + i] = o;
}

// np.argmax(plane > 0.1, axis=0): the first row above 0.1 of each column, 0 for a column without one.
__global__ void __launch_bounds__(kThreads) top_rows_kernel(Plane src, int h, int w, int *__restrict__ top)
{
    const int f = blockIdx.y, x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= w) return;
    const float *s = src.p + f * src.fs;
    int t = 0;
    for (int y = 0; y < h; ++y)
        if (s[(long long)y * w + x] > 0.1f) {
            t = y;
            break;
        }
    top[(long long)f * w + x] = t;
}

// s6: the top value of each column copied upwards (extrapolate) or s5 unchanged.
__global__ void __launch_bounds__(kThreads) extend_kernel(Plane s5, int h, int w, const int *__restrict__ top,
                                                          int extrapolate, Plane s6)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *s = s5.p + f * s5.fs;
    const int y = (int)(i / w), x = (int)(i % w);
    const int t = top[(long long)f * w + x];
    s6.p[f * s6.fs + i] = (extrapolate && y < t) ? s[(long long)t * w + x] : s[i];
}

// float -> int with the same order (no NaN in the maps)
__device__ __forceinline__ int order_key(float v)
{
    const int b = __float_as_int(v);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__global__ void minmax_init_kernel(int n_frames, int *__restrict__ mm)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    mm[2 * f] = INT_MAX;
    mm[2 * f + 1] = INT_MIN;
}

// the frame's global min and max (minMaxLoc), exact and order-independent
__global__ void __launch_bounds__(kThreads) minmax_kernel(Plane src, long long hw, int *__restrict__ mm)
{
    const int f = blockIdx.y;
    const float *s = src.p + f * src.fs;
    int lo = INT_MAX, hi = INT_MIN;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (long long)gridDim.x * blockDim.x) {
        const int k = order_key(s[i]);
        lo = min(lo, k);
        hi = max(hi, k);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(mm + 2 * f, lo);
        atomicMax(mm + 2 * f + 1, hi);
    }
}

// bilateralFilter_32f's colour table of each frame: lut[i] = (float) exp(val^2 * coeff), val = (double)(i / scale_index)
// with the division in float; once an entry is 0 the rest are 0.
__global__ void __launch_bounds__(kThreads) bilateral_lut_kernel(const int *__restrict__ mm, double color_coeff,
                                                                 float *__restrict__ lut)
{
    const int f = blockIdx.x;
    const double vmin = key_value(mm[2 * f]), vmax = key_value(mm[2 * f + 1]);
    const float len = (float)(vmax - vmin);
    const float scale = 4096.0f / len;
    for (int i = threadIdx.x; i < kLut; i += blockDim.x) {
        const double val = (double)((float)i / scale);
        lut[(long long)f * kLut + i] = (float)exp(val * val * color_coeff);
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // the table's lastExpVal rule (exp is monotone here, so this changes nothing in practice)
        bool zero = false;
        for (int i = 0; i < kLut; ++i) {
            float *e = lut + (long long)f * kLut + i;
            if (zero) *e = 0.0f;
            zero = zero || *e == 0.0f;
        }
    }
}

__device__ __forceinline__ void write_s7_s8(float s7v, float md, long long f, long long i, Plane s7, Plane s8,
                                            float *out, long long hw)
{
    const float s8v = s7v > 0.1f ? md - s7v : s7v;
    s7.p[f * s7.fs + i] = s7v;
    s8.p[f * s8.fs + i] = s8v;
    out[f * hw + i] = s8v;
}

// s7 = valid ? bilateralFilter(m, 5, 0.5, 2.0) : m with valid = (pre > 0.1) & top mask (the mask of the last median);
// then s8.  kBilateralPixels pixels per thread, the frame's colour table in LDS.
__global__ void __launch_bounds__(kThreads) bilateral_kernel(Plane m, Plane pre, int h, int w,
                                                             const int *__restrict__ top, const int *__restrict__ mm,
                                                             const float *__restrict__ lut, BilateralTaps taps,
                                                             float md, Plane s7, Plane s8, float *__restrict__ out)
{
    __shared__ float T[kLut];
    const int f = blockIdx.y;
    const long long hw = (long long)h * w;
    for (int k = threadIdx.x; k < kLut; k += blockDim.x) T[k] = lut[(long long)f * kLut + k];
    __syncthreads();
    const double vmin = key_value(mm[2 * f]), vmax = key_value(mm[2 * f + 1]);
    const bool flat = fabs(vmin - vmax) < (double)FLT_EPSILON;
    const float scale = 4096.0f / (float)(vmax - vmin);
    const float *s = m.p + f * m.fs;
    for (int k = 0; k < kBilateralPixels; ++k) {
        const long long i = ((long long)blockIdx.x * kBilateralPixels + k) * blockDim.x + threadIdx.x;
        if (i >= hw) return;
        const int y = (int)(i / w), x = (int)(i % w);
        const float rval = s[i];
        float o = rval;
        const bool valid = pre.p[f * pre.fs + i] > 0.1f && (top == nullptr || y >= top[(long long)f * w + x]);
        if (valid && !flat) {
            float sum = 0.0f, wsum = 0.0f;
            for (int t = 0; t < kBilateralTaps; ++t) {
                const float val = s[(long long)reflect101(y + taps.dy[t], h) * w + reflect101(x + taps.dx[t], w)];
                float alpha = fabsf(val - rval) * scale;
                const int idx = min(max((int)floorf(alpha), 0), kLut - 2);
                alpha -= (float)idx;
                const float wt = taps.w[t] * (T[idx] + alpha * (T[idx + 1] - T[idx]));
                wsum += wt;
                sum += val * wt;
            }
            o = sum / wsum;
        }
        write_s7_s8(o, md, f, i, s7, s8, out, hw);
    }
}

__device__ __forceinline__ float gauss5(float a, float b, float c, float d, float e)
{
    float s = 0.0625f * a;
    s = s + 0.25f * b;
    s = s + 0.375f * c;
    s = s + 0.25f * d;
    return s + 0.0625f * e;
}

// GaussianBlur((5, 5), 0), BORDER_REFLECT_101: the row pass
__global__ void __launch_bounds__(kThreads) gauss_rows_kernel(Plane src, int h, int w, Plane dst)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *s = src.p + f * src.fs + (i / w) * w;
    const int x = (int)(i % w);
    dst.p[f * dst.fs + i] = gauss5(s[reflect101(x - 2, w)], s[reflect101(x - 1, w)], s[x], s[reflect101(x + 1, w)],
                                   s[reflect101(x + 2, w)]);
}

// the column pass, then s7 = valid ? blur : m with valid = (m > 0.1) & top mask (recomputed), then s8
__global__ void __launch_bounds__(kThreads) gauss_cols_kernel(Plane rows, Plane m, int h, int w,
                                                              const int *__restrict__ top, float md, Plane s7, Plane s8,
                                                              float *__restrict__ out)
{
    const int f = blockIdx.y;
    const long long hw = (long long)h * w, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hw) return;
    const float *r = rows.p + f * rows.fs;
    const int y = (int)(i / w), x = (int)(i % w);
    const float c = m.p[f * m.fs + i];
    float o = c;
    if (c > 0.1f && (top == nullptr || y >= top[(long long)f * w + x]))
        o = gauss5(r[(long long)reflect101(y - 2, h) * w + x], r[(long long)reflect101(y - 1, h) * w + x], r[i],
                   r[(long long)reflect101(y + 1, h) * w + x], r[(long long)reflect101(y + 2, h) * w + x]);
    write_s7_s8(o, md, f, i, s7, s8, out, hw);
}

// workspace: [8 stage planes per frame (unused when the caller passes `stages`)] [tmp] [pre] [top4] [top5] [min/max]
// [colour tables]
struct FillLayout {
    size_t stages, tmp, pre, top4, top5, mm, lut, total;
};

FillLayout fill_layout(int n_frames, int h, int w)
{
    FillLayout L;
    const size_t plane = (size_t)n_frames * h * w * sizeof(float);
    size_t o = 0;
    L.stages = o;
    o += mpsr::align_up(8 * plane, 256);
    L.tmp = o;
    o += mpsr::align_up(plane, 256);
    L.pre = o;
    o += mpsr::align_up(plane, 256);
    L.top4 = o;
    o += mpsr::align_up((size_t)n_frames * w * sizeof(int), 256);
    L.top5 = o;
    o += mpsr::align_up((size_t)n_frames * w * sizeof(int), 256);
    L.mm = o;
    o += mpsr::align_up((size_t)n_frames * 2 * sizeof(int), 256);
    L.lut = o;
    o += mpsr::align_up((size_t)n_frames * kLut * sizeof(float), 256);
    L.total = o;
    return L;
}

int check_fill_shape(int n_frames, int h, int w)
{
    MPSR_REQUIRE(n_frames >= 0, "depth_fill: n_frames %d < 0", n_frames);
    MPSR_REQUIRE(h >= 5 && w >= 5, "depth_fill: image %d x %d is smaller than 5 x 5", h, w);
    MPSR_REQUIRE((long long)h * w <= (1LL << 30), "depth_fill: image %d x %d is too large", h, w);
    MPSR_REQUIRE(n_frames <= 65535, "depth_fill: %d frames in one batch (at most 65535)", n_frames);
    return MPSR_OK;
}

}  // namespace

extern "C" size_t mpsr_lidar_project_workspace_bytes(int n_frames, int h, int w)
{
    if (n_frames <= 0 || h <= 0 || w <= 0) return 0;
    return (size_t)n_frames * h * w * sizeof(int);
}

extern "C" int mpsr_lidar_project_depths(const float *points, const long long *frame_offsets,
                                         const long long *frame_offsets_host, int n_frames,
                                         const double *velo_to_cam0, const double *p2, int h, int w, double max_depth,
                                         float *out, void *workspace, size_t workspace_bytes, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_frames >= 0 && n_frames <= 65535, "lidar_project: n_frames %d (0..65535)", n_frames);
    MPSR_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "lidar_project: bad image size %d x %d", h, w);
    if (n_frames == 0) return MPSR_OK;
    MPSR_REQUIRE(frame_offsets_host && frame_offsets, "lidar_project: frame offsets are null");
    MPSR_REQUIRE(frame_offsets_host[0] == 0, "lidar_project: frame_offsets[0] = %lld, expected 0",
                 frame_offsets_host[0]);
    long long most = 0;
    for (int f = 0; f < n_frames; ++f) {
        const long long n = frame_offsets_host[f + 1] - frame_offsets_host[f];
        MPSR_REQUIRE(n >= 0 && n <= INT_MAX, "lidar_project: frame %d has %lld points", f, n);
        most = n > most ? n : most;
    }
    MPSR_REQUIRE(most == 0 || points, "lidar_project: points is null");
    MPSR_REQUIRE(velo_to_cam0 && p2 && out, "lidar_project: calibration or output is null");
    const size_t need = mpsr_lidar_project_workspace_bytes(n_frames, h, w);
    if (!workspace || workspace_bytes < need)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "lidar_project: workspace %zu bytes < %zu", workspace_bytes, need);
    hipStream_t s = mpsr::as_stream(stream);
    int *last = static_cast<int *>(workspace);
    MPSR_CHECK_HIP(hipMemsetAsync(last, 0xff, need, s));  // -1: no point
    if (most > 0) {
        const long long blocks = (most + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(project_scatter_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024), n_frames),
                           dim3(kThreads), 0, s, points, frame_offsets, velo_to_cam0, p2, h, w, last);
        MPSR_CHECK_LAUNCH("lidar_project scatter");
    }
    const long long hw = (long long)h * w;
    hipLaunchKernelGGL(project_write_kernel, dim3((unsigned)((hw + kThreads - 1) / kThreads), n_frames), dim3(kThreads),
                       0, s, points, frame_offsets, velo_to_cam0, last, hw, max_depth, out);
    MPSR_CHECK_LAUNCH("lidar_project write");
    return MPSR_OK;
}

extern "C" size_t mpsr_depth_fill_workspace_bytes(int n_frames, int h, int w)
{
    if (n_frames <= 0 || h <= 0 || w <= 0) return 0;
    return fill_layout(n_frames, h, w).total;
}

extern "C" int mpsr_depth_fill_multiscale(const float *depths, int n_frames, int h, int w,
                                          const mpsr_depth_fill_opts *opts, float *out, float *stages,
                                          void *workspace, size_t workspace_bytes, mpsr_stream_t stream)
{
    int st = check_fill_shape(n_frames, h, w);
    if (st) return st;
    MPSR_REQUIRE(opts, "depth_fill: opts is null");
    MPSR_REQUIRE(opts->blur_type == MPSR_DEPTH_BLUR_BILATERAL || opts->blur_type == MPSR_DEPTH_BLUR_GAUSSIAN,
                 "depth_fill: unknown blur_type %d", opts->blur_type);
    Taps taps{};
    for (int b = 0; b < 3; ++b) {
        const int kh = opts->kernel_h[b], kw = opts->kernel_w[b];
        MPSR_REQUIRE(kh >= 1 && kw >= 1 && kh <= kMaxK && kw <= kMaxK,
                     "depth_fill: dilation kernel %d is %d x %d (1 x 1 .. %d x %d)", b, kh, kw, kMaxK, kMaxK);
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j)
                if (opts->kernels[b][i * kMaxK + j]) {
                    taps.dy[b][taps.n[b]] = (signed char)(i - kh / 2);  // cv2's default anchor (kw / 2, kh / 2)
                    taps.dx[b][taps.n[b]] = (signed char)(j - kw / 2);
                    ++taps.n[b];
                }
    }
    if (n_frames == 0) return MPSR_OK;
    MPSR_REQUIRE(depths && out, "depth_fill: input or output is null");
    const FillLayout L = fill_layout(n_frames, h, w);
    if (!workspace || workspace_bytes < L.total)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "depth_fill: workspace %zu bytes < %zu", workspace_bytes, L.total);

    char *ws = static_cast<char *>(workspace);
    const long long hw = (long long)h * w;
    float *stage_base = stages ? stages : reinterpret_cast<float *>(ws + L.stages);
    Plane S[9];
    for (int k = 1; k <= 8; ++k) S[k] = Plane{stage_base + (k - 1) * hw, 8 * hw};
    const Plane tmp{reinterpret_cast<float *>(ws + L.tmp), hw}, pre{reinterpret_cast<float *>(ws + L.pre), hw};
    int *top4 = reinterpret_cast<int *>(ws + L.top4), *top5 = reinterpret_cast<int *>(ws + L.top5);
    int *mm = reinterpret_cast<int *>(ws + L.mm);
    float *lut = reinterpret_cast<float *>(ws + L.lut);
    const float md = opts->max_depth;
    const int *top_mask = opts->extrapolate ? nullptr : top5;
    const Plane none{nullptr, 0};
    hipStream_t s = mpsr::as_stream(stream);
    const dim3 grid((unsigned)((hw + kThreads - 1) / kThreads), n_frames), cols((w + kThreads - 1) / kThreads, n_frames);

    hipLaunchKernelGGL(stage12_kernel, grid, dim3(kThreads), 0, s, depths, h, w, md, taps, S[1], S[2]);
    // s3: MORPH_CLOSE with FULL_KERNEL_5 -- dilate (rows, columns), then erode (rows, columns)
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, S[2], h, w, 2, 0, 1, (int)EPI_PLAIN, none, nullptr, tmp);
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, tmp, h, w, 2, 1, 1, (int)EPI_PLAIN, none, nullptr, S[3]);
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, S[3], h, w, 2, 0, 0, (int)EPI_PLAIN, none, nullptr, tmp);
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, tmp, h, w, 2, 1, 0, (int)EPI_PLAIN, none, nullptr, S[3]);
    // s4: median where s3 > 0.1
    hipLaunchKernelGGL(median_kernel, grid, dim3(kThreads), 0, s, S[3], h, w, nullptr, S[4]);
    // s5: 9x9 dilation into the empty pixels below each column's top
    hipLaunchKernelGGL(top_rows_kernel, cols, dim3(kThreads), 0, s, S[4], h, w, top4);
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, S[4], h, w, 4, 0, 1, (int)EPI_PLAIN, none, nullptr, tmp);
    hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, tmp, h, w, 4, 1, 1, (int)EPI_HOLE, S[4], top4, S[5]);
    // s6: top rows of s5; extend them upwards or keep them as the top mask
    hipLaunchKernelGGL(top_rows_kernel, cols, dim3(kThreads), 0, s, S[5], h, w, top5);
    hipLaunchKernelGGL(extend_kernel, grid, dim3(kThreads), 0, s, S[5], h, w, top5, opts->extrapolate, S[6]);
    // s7: six masked 5x5 dilations, each over the result of the previous one (in `pre`), then the masked median
    for (int it = 0; it < 6; ++it) {
        hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, it ? pre : S[6], h, w, 2, 0, 1, (int)EPI_PLAIN,
                           none, nullptr, tmp);
        hipLaunchKernelGGL(sep_kernel, grid, dim3(kThreads), 0, s, tmp, h, w, 2, 1, 1, (int)EPI_EMPTY,
                           it ? pre : S[6], top_mask, pre);
    }
    hipLaunchKernelGGL(median_kernel, grid, dim3(kThreads), 0, s, pre, h, w, top_mask, tmp);  // tmp: s7 after the median
    if (opts->blur_type == MPSR_DEPTH_BLUR_BILATERAL) {
        // bilateralFilter(s7, 5, 0.5, 2.0): radius 2, the taps with r <= 2 in row-major order, space weights in double
        BilateralTaps bt{};
        int nt = 0;
        for (int i = -2; i <= 2; ++i)
            for (int j = -2; j <= 2; ++j) {
                const double r = std::sqrt((double)i * i + (double)j * j);
                if (r > 2.0) continue;
                bt.dy[nt] = i;
                bt.dx[nt] = j;
                bt.w[nt++] = (float)std::exp(r * r * kSpaceCoeff);
            }
        hipLaunchKernelGGL(minmax_init_kernel, dim3((n_frames + 63) / 64), dim3(64), 0, s, n_frames, mm);
        const long long mblocks = (hw + kThreads * 16 - 1) / (kThreads * 16);
        hipLaunchKernelGGL(minmax_kernel, dim3((unsigned)mblocks, n_frames), dim3(kThreads), 0, s, tmp, hw, mm);
        hipLaunchKernelGGL(bilateral_lut_kernel, dim3(n_frames), dim3(kThreads), 0, s, mm, kColorCoeff,
                           lut);
        const long long bblocks = (hw + kThreads * kBilateralPixels - 1) / (kThreads * kBilateralPixels);
        hipLaunchKernelGGL(bilateral_kernel, dim3((unsigned)bblocks, n_frames), dim3(kThreads), 0, s, tmp, pre, h, w,
                           top_mask, mm, lut, bt, md, S[7], S[8], out);
    } else {  // MPSR_DEPTH_BLUR_GAUSSIAN; `pre` is free again
        hipLaunchKernelGGL(gauss_rows_kernel, grid, dim3(kThreads), 0, s, tmp, h, w, pre);
        hipLaunchKernelGGL(gauss_cols_kernel, grid, dim3(kThreads), 0, s, pre, tmp, h, w, top_mask, md, S[7], S[8], out);
    }
    MPSR_CHECK_LAUNCH("depth_fill");
    return MPSR_OK;
}

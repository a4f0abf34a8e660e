// One step's row of the training log (core/train_log.py): the step's loss terms, read from the
// device scalars that hold them, and four figures of the reduced, unclipped gradient taken from the per-variable squared
// norms that segment_norms (optim.hip) leaves in the clip table's scratch.  One launch of one workgroup, nothing read
// back: the training loop never waits for a loss.  fp64 sums in a fixed order (strided per-thread partials, then a
// tree over LDS), no atomics, plain vector stores: two calls on the same inputs give the same bits.
#include "common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;

struct SumOp {
    template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct MaxOp {
    __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
};

// every thread's v combined, to every thread: a tree over LDS, the same pairs in the same order on every call
template <class T, class Op> __device__ __forceinline__ T block_reduce(T v, T *lds, Op op)
{
    const int t = threadIdx.x;
    __syncthreads();  // (the previous reduction's readers are done with lds)
    lds[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if (t < s) lds[t] = op(lds[t], lds[t + s]);
        __syncthreads();
    }
    return lds[0];
}

__global__ void __launch_bounds__(kThreads) train_log_append_kernel(
    mpsr_train_log_terms terms, int n_terms, const float *__restrict__ sumsq, int n_segments, float clip, float lr,
    long long step, float *__restrict__ row_out, long long *__restrict__ step_out)
{
    __shared__ double lds[kThreads];
    const int t = threadIdx.x;
    // thread i < n_terms stores term i (the pointer is picked with uniform compares: no per-lane index into the arguments)
    if (t < n_terms) {
        const float *p = nullptr;
#pragma unroll
        for (int i = 0; i < MPSR_TRAIN_LOG_MAX_TERMS; ++i)
            if (t == i) p = terms.p[i];
        row_out[t] = p ? *p : __int_as_float(0x7fc00000);
    }
    // thread t owns the variables t, t + 256, ...
    double sum = 0.0;
    float max_norm = 0.f;
    int n_clipped = 0, n_nonfinite = 0;
    for (int s = t; s < n_segments; s += kThreads) {
        const float v = sumsq[s];
        if (v != v || fabsf(v) == INFINITY) {
            ++n_nonfinite;
            continue;
        }
        const float norm = sqrtf(v);  // (the norm clip_adam_ema_kernel compares with clip_norm, same rounding)
        sum += (double)v;
        max_norm = fmaxf(max_norm, norm);
        if (clip > 0.f && norm > clip) ++n_clipped;
    }
    sum = block_reduce(sum, lds, SumOp());
    max_norm = block_reduce(max_norm, reinterpret_cast<float *>(lds), MaxOp());
    n_clipped = block_reduce(n_clipped, reinterpret_cast<int *>(lds), SumOp());
    n_nonfinite = block_reduce(n_nonfinite, reinterpret_cast<int *>(lds), SumOp());
    if (t == 0) {
        float *g = row_out + n_terms;
        g[0] = (float)sqrt(sum);
        g[1] = max_norm;
        g[2] = (float)n_clipped;
        g[3] = (float)n_nonfinite;
        g[4] = lr;
        *step_out = step;
    }
}

}  // namespace

extern "C" int mpsr_train_log_append(mpsr_train_log_terms terms, int n_terms, const float *sumsq, int n_segments,
                                     float clip_norm, float lr, long long step, float *rows, long long *steps,
                                     int n_rows, int n_cols, int row, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_terms >= 1 && n_terms <= MPSR_TRAIN_LOG_MAX_TERMS, "train_log_append: n_terms %d is outside [1, %d]",
                 n_terms, MPSR_TRAIN_LOG_MAX_TERMS);
    MPSR_REQUIRE(n_cols == n_terms + MPSR_TRAIN_LOG_STAT_COLS, "train_log_append: n_cols %d != n_terms + %d = %d", n_cols,
                 MPSR_TRAIN_LOG_STAT_COLS, n_terms + MPSR_TRAIN_LOG_STAT_COLS);
    MPSR_REQUIRE(row >= 0 && row < n_rows, "train_log_append: row %d is outside [0, %d)", row, n_rows);
    MPSR_REQUIRE(rows && steps, "train_log_append: rows / steps is null");
    MPSR_REQUIRE(n_segments >= 0, "train_log_append: negative n_segments %d", n_segments);
    if (!sumsq) n_segments = 0;
    hipLaunchKernelGGL(train_log_append_kernel, dim3(1), dim3(kThreads), 0, mpsr::as_stream(stream), terms, n_terms,
                       sumsq, n_segments, clip_norm, lr, step, rows + (long long)row * n_cols, steps + row);
    MPSR_CHECK_LAUNCH("train_log_append_kernel");
    return MPSR_OK;
}

// The evaluator's per-object error statistics (the reference's save_metrics, core/evaluator_utils.py:294-403, over the
// lists core/evaluator.py:270-281 gathers): count, mean, population std, and the same of |x|, per metric, from a
// device-resident table of one row per object.  fp64, two passes (the mean, then the centred squares), a fixed order of
// summation and no atomics: two calls on one table give the same bits.  DESIGN.md section 7.5.
// Built with -ffp-contract=off: the centred square (x - mean) * (x - mean) is rounded before it is added.
#include "common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;

struct MetricColumns {
    int metric[MPSR_METRIC_STATS_MAX_COLS];  // column -> metric
};

// the sum of every thread's v, to every thread: a tree over LDS, the same pairs in the same order on every call
__device__ __forceinline__ double block_sum(double v, double *lds)
{
    const int t = threadIdx.x;
    __syncthreads();  // (the previous sum's readers are done with lds)
    lds[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// One workgroup per metric.  Element e of the metric is (row e / k, the metric's (e % k)-th column), k = the number
// of its columns; thread t owns the elements t, t + 256, ...
__global__ void __launch_bounds__(kThreads) metric_stats_kernel(
    const float *__restrict__ values, const int *__restrict__ frame, int n_rows, int n_cols, MetricColumns cm,
    int n_frames, int nan_rule, int *frame_flags, double *__restrict__ stats)
{
    __shared__ double lds[kThreads];
    __shared__ int cols[MPSR_METRIC_STATS_MAX_COLS];
    __shared__ int n_own;
    const int m = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        int k = 0;
        for (int c = 0; c < n_cols; ++c)
            if (cm.metric[c] == m) cols[k++] = c;
        n_own = k;
    }
    __syncthreads();
    const int k = n_own;
    const long long n_elem = (long long)n_rows * k;
    int *flags = nullptr;
    if (nan_rule == 1) {
        flags = frame_flags + (long long)m * n_frames;  // this workgroup's own slice: no other one touches it
        for (int f = t; f < n_frames; f += kThreads) flags[f] = 0;
        __threadfence_block();
        __syncthreads();
        for (long long e = t; e < n_elem; e += kThreads) {
            const int r = (int)(e / k), c = cols[(int)(e % k)];
            const float v = values[(long long)r * n_cols + c];
            const int f = frame[r];
            if (v != v && f >= 0 && f < n_frames) flags[f] = 1;  // (every writer stores the same value)
        }
        __threadfence_block();
        __syncthreads();
    }
    // pass 1: which elements count, their sum and the sum of their magnitudes
    double cnt = 0.0, drop = 0.0, sum = 0.0, sum_abs = 0.0;
    for (long long e = t; e < n_elem; e += kThreads) {
        const int r = (int)(e / k), c = cols[(int)(e % k)];
        const float v = values[(long long)r * n_cols + c];
        bool out = v != v;
        if (nan_rule == 1) {
            const int f = frame[r];
            out = out || f < 0 || f >= n_frames || flags[f] != 0;
        }
        if (out) {
            drop += 1.0;
        } else {
            cnt += 1.0;
            sum += (double)v;
            sum_abs += fabs((double)v);
        }
    }
    cnt = block_sum(cnt, lds);
    drop = block_sum(drop, lds);
    sum = block_sum(sum, lds);
    sum_abs = block_sum(sum_abs, lds);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const double mean = cnt > 0.0 ? sum / cnt : nan, mean_abs = cnt > 0.0 ? sum_abs / cnt : nan;
    // pass 2: the centred squares
    double sq = 0.0, sq_abs = 0.0;
    for (long long e = t; e < n_elem && cnt > 0.0; e += kThreads) {
        const int r = (int)(e / k), c = cols[(int)(e % k)];
        const float v = values[(long long)r * n_cols + c];
        bool out = v != v;
        if (nan_rule == 1) {
            const int f = frame[r];
            out = out || f < 0 || f >= n_frames || flags[f] != 0;
        }
        if (!out) {
            const double d = (double)v - mean, da = fabs((double)v) - mean_abs;
            sq += d * d;
            sq_abs += da * da;
        }
    }
    sq = block_sum(sq, lds);
    sq_abs = block_sum(sq_abs, lds);
    if (t == 0) {
        double *o = stats + 6 * (long long)m;
        o[0] = cnt;
        o[1] = mean;
        o[2] = cnt > 0.0 ? sqrt(sq / cnt) : nan;
        o[3] = mean_abs;
        o[4] = cnt > 0.0 ? sqrt(sq_abs / cnt) : nan;
        o[5] = drop;
    }
}

}  // namespace

extern "C" int mpsr_metric_stats(const float *values, const int *frame, int n_rows, int n_cols,
                                 const int *column_metric, int n_metrics, int n_frames, int nan_rule,
                                 int *frame_flags, double *stats, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_metrics >= 0 && n_frames >= 0,
                 "metric_stats: negative size: n_rows %d, n_cols %d, n_metrics %d, n_frames %d", n_rows, n_cols,
                 n_metrics, n_frames);
    MPSR_REQUIRE(n_cols <= MPSR_METRIC_STATS_MAX_COLS, "metric_stats: n_cols %d above the limit of %d", n_cols,
                 MPSR_METRIC_STATS_MAX_COLS);
    MPSR_REQUIRE(n_metrics <= n_cols, "metric_stats: n_metrics %d > n_cols %d", n_metrics, n_cols);
    MPSR_REQUIRE(nan_rule == MPSR_NAN_RULE_ENTRY || nan_rule == MPSR_NAN_RULE_FRAME,
                 "metric_stats: unknown nan_rule %d", nan_rule);
    MPSR_REQUIRE(n_cols == 0 || column_metric, "metric_stats: column_metric is null");
    MetricColumns cm;
    for (int c = 0; c < MPSR_METRIC_STATS_MAX_COLS; ++c) cm.metric[c] = -1;
    for (int c = 0; c < n_cols; ++c) {
        MPSR_REQUIRE(column_metric[c] >= 0 && column_metric[c] < n_metrics,
                     "metric_stats: column_metric[%d] = %d is outside [0, %d)", c, column_metric[c], n_metrics);
        cm.metric[c] = column_metric[c];
    }
    if (n_metrics == 0) return MPSR_OK;  // no output element
    MPSR_REQUIRE(stats, "metric_stats: stats is null");
    const bool by_frame = nan_rule == MPSR_NAN_RULE_FRAME;
    MPSR_REQUIRE(n_rows == 0 || (values && (!by_frame || frame)), "metric_stats: a table pointer is null");
    MPSR_REQUIRE(!by_frame || n_frames == 0 || frame_flags, "metric_stats: frame_flags is null");
    metric_stats_kernel<<<(unsigned)n_metrics, kThreads, 0, mpsr::as_stream(stream)>>>(
        values, frame, n_rows, n_cols, cm, n_frames, nan_rule, frame_flags, stats);
    MPSR_CHECK_LAUNCH("metric_stats_kernel");
    return MPSR_OK;
}

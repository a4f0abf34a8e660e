// The evaluator's per-object error statistics (the reference's save_metrics, core/evaluator_utils.py:294-403, over the
// lists core/evaluator.py:270-281 gathers): count, mean, population std, and the same of |x|, per metric, from a
// device-resident table of one row per object.  fp64, two passes (the mean, then the centred squares), a fixed order of
// summation and no atomics: two calls on one table give the same bits.  DESIGN.md section 7.5.
// Built with -ffp-contract=off: the centred square (x - mean) * (x - mean) is rounded before it is added.
#include "common.h"
#include "metric_stats_core.h"

#include <cmath>

namespace {

using namespace mpsr_stats;  // the statistics' body, shared with object_pairs.hip's binned form

// One workgroup per metric (metric_stats_core.h: the element-to-thread assignment and the sums).
__global__ void __launch_bounds__(kThreads) metric_stats_kernel(
    const float *__restrict__ values, const int *__restrict__ frame, int n_rows, int n_cols, MetricColumns cm,
    int n_frames, int nan_rule, int *frame_flags, double *__restrict__ stats)
{
    __shared__ double lds[kThreads];
    __shared__ int cols[MPSR_METRIC_STATS_MAX_COLS];
    __shared__ int n_own;
    const int m = blockIdx.x, t = threadIdx.x;
    const int k = own_columns(cm, n_cols, m, cols, &n_own);
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
    // under the frame rule a row is dropped with its frame: a NaN among the frame's values, or no such frame
    const auto row_state = [=](int r) {
        if (nan_rule != 1) return (int)kRowIn;
        const int f = frame[r];
        return (int)(f < 0 || f >= n_frames || flags[f] != 0 ? kRowDropped : kRowIn);
    };
    metric_stats_body(values, n_rows, n_cols, cols, k, row_state, lds, stats + 6 * (long long)m);
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

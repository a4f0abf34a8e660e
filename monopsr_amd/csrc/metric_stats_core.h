// The two-pass fp64 statistics of one metric over a table's rows, by one workgroup of 256 threads: the body of
// metric_stats_kernel (metric_stats.hip: every row, either NaN rule) and of metric_stats_binned_kernel
// (object_pairs.hip: the rows of one slot).  The element-to-thread assignment, the order of each thread's sums and the
// LDS tree are the same for every caller, so a caller that leaves no row out gets the bits of one that leaves none out.
// Built with -ffp-contract=off: the centred square (x - mean) * (x - mean) is rounded before it is added.
#pragma once
#include "common.h"

#include <cmath>

namespace mpsr_stats {

constexpr int kThreads = 256;

struct MetricColumns {
    int metric[MPSR_METRIC_STATS_MAX_COLS];  // column -> metric
};

// what a row is to the statistics: its values count (unless NaN), are dropped, or are not there at all
enum RowState { kRowIn = 0, kRowDropped = 1, kRowAbsent = 2 };

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

// the columns of metric m into cols[] (LDS), their number as the result, to every thread
__device__ __forceinline__ int own_columns(const MetricColumns &cm, int n_cols, int m, int *cols, int *n_own)
{
    if (threadIdx.x == 0) {
        int k = 0;
        for (int c = 0; c < n_cols; ++c)
            if (cm.metric[c] == m) cols[k++] = c;
        *n_own = k;
    }
    __syncthreads();
    return *n_own;
}

// Element e of the metric is (row e / k, the metric's (e % k)-th column), k = the number of its columns; thread t owns
// the elements t, t + 256, ...  row_state(r) -> RowState.  o[6]: count, mean, std, mean |x|, std |x|, dropped.
template <typename RowStateFn>
__device__ __forceinline__ void metric_stats_body(const float *__restrict__ values, int n_rows, int n_cols,
                                                  const int *cols, int k, RowStateFn row_state, double *lds,
                                                  double *__restrict__ o)
{
    const int t = threadIdx.x;
    const long long n_elem = (long long)n_rows * k;
    // pass 1: which elements count, their sum and the sum of their magnitudes
    double cnt = 0.0, drop = 0.0, sum = 0.0, sum_abs = 0.0;
    for (long long e = t; e < n_elem; e += kThreads) {
        const int r = (int)(e / k), c = cols[(int)(e % k)];
        const int state = row_state(r);
        if (state == kRowAbsent) continue;
        const float v = values[(long long)r * n_cols + c];
        if (v != v || state == kRowDropped) {
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
        if (row_state(r) != kRowIn) continue;
        const float v = values[(long long)r * n_cols + c];
        if (v == v) {
            const double d = (double)v - mean, da = fabs((double)v) - mean_abs;
            sq += d * d;
            sq_abs += da * da;
        }
    }
    sq = block_sum(sq, lds);
    sq_abs = block_sum(sq_abs, lds);
    if (t == 0) {
        o[0] = cnt;
        o[1] = mean;
        o[2] = cnt > 0.0 ? sqrt(sq / cnt) : nan;
        o[3] = mean_abs;
        o[4] = cnt > 0.0 ? sqrt(sq_abs / cnt) : nan;
        o[5] = drop;
    }
}

}  // namespace mpsr_stats

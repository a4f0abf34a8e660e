// Each predicted box against its own label, and the evaluator's statistics split by where the label is (DESIGN.md
// section 7.11).
//   mpsr_object_pairs: per object the image IoU of the box the network was fed against the label's own 2-D box, the
//     BEV and 3-D IoU of the predicted box against the label's (the KITTI program's arithmetic, kitti_geometry.h) and
//     the distance of the box centres; the IoUs against 0.7 / 0.5 / 0.25; and the bins a breakdown is taken over: the
//     label's depth, its KITTI difficulty and the fed box's IoU.  One thread per object, fp64 from float32 inputs.
//   mpsr_metric_stats_binned: metric_stats_kernel's statistics (metric_stats_core.h) under MPSR_NAN_RULE_ENTRY for every
//     row and for every bin of up to four axes in one launch, one workgroup per (slot, metric).  No atomics: two calls
//     return the same bits, and slot 0 the bits of mpsr_metric_stats.
// Built with -ffp-contract=off, as kitti_eval.hip and metric_stats.hip are: their arithmetic is this file's.
#include "common.h"
#include "kitti_geometry.h"
#include "metric_stats_core.h"

#include <cmath>

namespace {

using namespace mpsr_kitti;
using namespace mpsr_stats;

constexpr int kPairThreads = 64;

struct Edges {
    double v[MPSR_OBJECT_PAIRS_MAX_EDGES];
    int n;
};

// the number of edges <= x: a value on an edge goes to the upper bin
__device__ __forceinline__ int bin_of(const Edges &e, double x)
{
    int b = 0;
    for (int i = 0; i < e.n; ++i) b += e.v[i] <= x ? 1 : 0;
    return b;
}

__device__ __forceinline__ double hit(double iou, double threshold)
{
    return iou != iou ? iou : (iou >= threshold ? 1.0 : 0.0);
}

__global__ void __launch_bounds__(kPairThreads) object_pairs_kernel(
    const float *__restrict__ pred, const float *__restrict__ gt, const float *__restrict__ fed,
    const float *__restrict__ info, int n, Edges depth_edges, Edges iou_edges, double *__restrict__ overlaps,
    float *__restrict__ table, int *__restrict__ bins)
{
    const int i = blockIdx.x * kPairThreads + threadIdx.x;
    if (i >= n) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // [x y z l w h ry] -> rows in the evaluator's column order
    double d[MPSR_KITTI_FIELDS] = {}, g[MPSR_KITTI_FIELDS] = {};
    const int field[7] = {MPSR_KITTI_TX, MPSR_KITTI_TY, MPSR_KITTI_TZ, MPSR_KITTI_L,
                          MPSR_KITTI_W,  MPSR_KITTI_H,  MPSR_KITTI_RY};
    bool finite = true;
    for (int k = 0; k < 7; ++k) {
        d[field[k]] = (double)pred[(long long)i * 7 + k];
        g[field[k]] = (double)gt[(long long)i * 7 + k];
        finite = finite && isfinite(d[field[k]]) && isfinite(g[field[k]]);
    }
    double o[6] = {nan, nan, nan, nan, nan, nan}, centre_dist = nan;
    if (finite) {
        ground_and_box_overlaps(d, g, o);
        const double dx = d[MPSR_KITTI_TX] - g[MPSR_KITTI_TX], dz = d[MPSR_KITTI_TZ] - g[MPSR_KITTI_TZ];
        const double dy = (d[MPSR_KITTI_TY] - d[MPSR_KITTI_H] / 2) - (g[MPSR_KITTI_TY] - g[MPSR_KITTI_H] / 2);
        centre_dist = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    // the fed box [y1 x1 y2 x2] against the label's own [x1 y1 x2 y2] (label_info's columns 2..5)
    double iou_fed = nan;
    int difficulty = -1;
    if (info) {
        double v[6];
        bool info_finite = true, box_finite = true;
        for (int k = 0; k < 6; ++k) {
            v[k] = (double)info[(long long)i * 6 + k];
            info_finite = info_finite && isfinite(v[k]);
            if (k >= 2) box_finite = box_finite && isfinite(v[k]);
        }
        if (fed) {
            const float *f = fed + (long long)i * 4;
            d[MPSR_KITTI_Y1] = (double)f[0];
            d[MPSR_KITTI_X1] = (double)f[1];
            d[MPSR_KITTI_Y2] = (double)f[2];
            d[MPSR_KITTI_X2] = (double)f[3];
            g[MPSR_KITTI_X1] = v[2];
            g[MPSR_KITTI_Y1] = v[3];
            g[MPSR_KITTI_X2] = v[4];
            g[MPSR_KITTI_Y2] = v[5];
            if (box_finite && isfinite(d[MPSR_KITTI_X1]) && isfinite(d[MPSR_KITTI_Y1]) && isfinite(d[MPSR_KITTI_X2]) &&
                isfinite(d[MPSR_KITTI_Y2]))
                iou_fed = image_overlap(d, g, false);
        }
        if (info_finite) {
            // cleanData's test (:411-413) on the label's own box: the first level that does not ignore it.  The
            // truncation arrives as float32, so its limits are rounded the same way: a label file's 0.15 or 0.3 is
            // on the limit here as it is in the KITTI program, not a float32 rounding above it.
            const double height = v[5] - v[3];
            difficulty = 3;
            for (int level = 2; level >= 0; --level)
                if (height > c_min_height[level] && v[1] <= c_max_occlusion[level] &&
                    v[0] <= (double)(float)c_max_truncation[level])
                    difficulty = level;
        }
    }
    const double iou_bev = o[1], iou_3d = o[2];
    const double row[9] = {iou_fed,           iou_bev,           iou_3d,           centre_dist,      hit(iou_3d, 0.7),
                           hit(iou_3d, 0.5),  hit(iou_3d, 0.25), hit(iou_bev, 0.7), hit(iou_bev, 0.5)};
    for (int k = 0; k < 4; ++k) overlaps[(long long)i * 4 + k] = row[k];
    for (int k = 0; k < 9; ++k) table[(long long)i * 9 + k] = (float)row[k];
    const double z = g[MPSR_KITTI_TZ];
    bins[(long long)i * 3 + 0] = isfinite(z) ? bin_of(depth_edges, z) : -1;
    bins[(long long)i * 3 + 1] = difficulty;
    bins[(long long)i * 3 + 2] = iou_fed != iou_fed ? -1 : bin_of(iou_edges, iou_fed);
}

struct BinAxes {
    int n_axes;
    int bins[MPSR_METRIC_STATS_MAX_AXES];
};

// One workgroup per (metric, slot).  Slot 0 is every row; slot 1 + (the bins of the axes before a) + b is bin b of
// axis a.  A row outside the slot is absent: neither counted nor dropped.
__global__ void __launch_bounds__(kThreads) metric_stats_binned_kernel(
    const float *__restrict__ values, const int *__restrict__ bins, int n_rows, int n_cols, MetricColumns cm,
    BinAxes axes, int n_metrics, double *__restrict__ stats)
{
    __shared__ double lds[kThreads];
    __shared__ int cols[MPSR_METRIC_STATS_MAX_COLS];
    __shared__ int n_own;
    const int m = blockIdx.x, slot = blockIdx.y;
    const int k = own_columns(cm, n_cols, m, cols, &n_own);
    int axis = -1, bin = slot - 1;
    if (slot > 0) {
        axis = 0;
        while (bin >= axes.bins[axis]) bin -= axes.bins[axis++];  // (slot < 1 + the sum of axes.bins: the grid's size)
    }
    const int n_axes = axes.n_axes;
    const auto row_state = [=](int r) {
        return (int)(axis < 0 || bins[(long long)r * n_axes + axis] == bin ? kRowIn : kRowAbsent);
    };
    metric_stats_body(values, n_rows, n_cols, cols, k, row_state, lds,
                      stats + 6 * ((long long)slot * n_metrics + m));
}

int fill_edges(const char *name, const double *edges, int n_edges, Edges *out)
{
    MPSR_REQUIRE(n_edges >= 0 && n_edges <= MPSR_OBJECT_PAIRS_MAX_EDGES,
                 "object_pairs: %d %s, outside 0..%d (too many)", n_edges, name, MPSR_OBJECT_PAIRS_MAX_EDGES);
    MPSR_REQUIRE(n_edges == 0 || edges, "object_pairs: %s is null", name);
    for (int i = 0; i < MPSR_OBJECT_PAIRS_MAX_EDGES; ++i) out->v[i] = 0.0;
    for (int i = 0; i < n_edges; ++i) {
        MPSR_REQUIRE(std::isfinite(edges[i]), "object_pairs: %s[%d] is not finite", name, i);
        MPSR_REQUIRE(i == 0 || edges[i] > edges[i - 1], "object_pairs: %s[%d] = %g is not increasing (after %g)",
                     name, i, edges[i], edges[i - 1]);
        out->v[i] = edges[i];
    }
    out->n = n_edges;
    return MPSR_OK;
}

}  // namespace

extern "C" int mpsr_object_pairs(const float *pred_box_3d, const float *gt_box_3d, const float *fed_box_2d,
                                 const float *label_info, int n, const double *depth_edges, int n_depth_edges,
                                 const double *box_iou_edges, int n_box_iou_edges, double *overlaps, float *table,
                                 int *bins, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0, "object_pairs: negative size: n %d", n);
    Edges de, ie;
    int st = fill_edges("depth_edges", depth_edges, n_depth_edges, &de);
    if (!st) st = fill_edges("box_iou_edges", box_iou_edges, n_box_iou_edges, &ie);
    if (st) return st;
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(pred_box_3d && gt_box_3d, "object_pairs: a box pointer is null with n = %d", n);
    MPSR_REQUIRE(overlaps && table && bins, "object_pairs: an output pointer is null with n = %d", n);
    object_pairs_kernel<<<(unsigned)mpsr::ceil_div(n, kPairThreads), kPairThreads, 0, mpsr::as_stream(stream)>>>(
        pred_box_3d, gt_box_3d, fed_box_2d, label_info, n, de, ie, overlaps, table, bins);
    MPSR_CHECK_LAUNCH("object_pairs_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_metric_stats_binned(const float *values, const int *bins, int n_rows, int n_cols,
                                        const int *column_metric, int n_metrics, int n_axes, const int *axis_bins,
                                        double *stats, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_metrics >= 0 && n_axes >= 0,
                 "metric_stats_binned: negative size: n_rows %d, n_cols %d, n_metrics %d, n_axes %d", n_rows, n_cols,
                 n_metrics, n_axes);
    MPSR_REQUIRE(n_cols <= MPSR_METRIC_STATS_MAX_COLS, "metric_stats_binned: n_cols %d above the limit of %d", n_cols,
                 MPSR_METRIC_STATS_MAX_COLS);
    MPSR_REQUIRE(n_metrics <= n_cols, "metric_stats_binned: n_metrics %d > n_cols %d", n_metrics, n_cols);
    MPSR_REQUIRE(n_axes <= MPSR_METRIC_STATS_MAX_AXES, "metric_stats_binned: n_axes %d above the limit of %d", n_axes,
                 MPSR_METRIC_STATS_MAX_AXES);
    MPSR_REQUIRE(n_axes == 0 || axis_bins, "metric_stats_binned: axis_bins is null");
    BinAxes axes{n_axes, {0, 0, 0, 0}};
    int n_bins = 0;
    for (int a = 0; a < n_axes; ++a) {
        MPSR_REQUIRE(axis_bins[a] >= 0 && axis_bins[a] <= MPSR_METRIC_STATS_MAX_BINS,
                     "metric_stats_binned: axis_bins[%d] = %d is outside [0, %d]", a, axis_bins[a],
                     MPSR_METRIC_STATS_MAX_BINS);
        axes.bins[a] = axis_bins[a];
        n_bins += axis_bins[a];
    }
    MPSR_REQUIRE(n_bins <= MPSR_METRIC_STATS_MAX_BINS, "metric_stats_binned: %d bins over all axes, above the limit of %d",
                 n_bins, MPSR_METRIC_STATS_MAX_BINS);
    MPSR_REQUIRE(n_cols == 0 || column_metric, "metric_stats_binned: column_metric is null");
    MetricColumns cm;
    for (int c = 0; c < MPSR_METRIC_STATS_MAX_COLS; ++c) cm.metric[c] = -1;
    for (int c = 0; c < n_cols; ++c) {
        MPSR_REQUIRE(column_metric[c] >= 0 && column_metric[c] < n_metrics,
                     "metric_stats_binned: column_metric[%d] = %d is outside [0, %d)", c, column_metric[c], n_metrics);
        cm.metric[c] = column_metric[c];
    }
    if (n_metrics == 0) return MPSR_OK;  // no output element
    MPSR_REQUIRE(stats, "metric_stats_binned: stats is null");
    MPSR_REQUIRE(n_rows == 0 || (values && (n_bins == 0 || bins)), "metric_stats_binned: a table pointer is null");
    metric_stats_binned_kernel<<<dim3((unsigned)n_metrics, (unsigned)(1 + n_bins)), kThreads, 0,
                                 mpsr::as_stream(stream)>>>(values, bins, n_rows, n_cols, cm, axes, n_metrics, stats);
    MPSR_CHECK_LAUNCH("metric_stats_binned_kernel");
    return MPSR_OK;
}

// Shape scores over valid points (mpsr_shape_scores): the masked Chamfer search of two clouds
// per box with its statistics -- accuracy, completeness, Chamfer-L1, squared Chamfer, Hausdorff and precision / recall
// / F-score at distance thresholds.
//
// Everything it has in common with mpsr_surface_scores lives in shape_score_core.h: the validity rule, the thresholds,
// the work items, the point minimum, the slab statistics, the combine and the workspace, here with D = float.  This
// file holds what is left:
//   * shape_search_kernel, one workgroup per (box, direction, slab of kSlab queries): each thread carries kQPT
//     queries, one in every quarter of the slab, and tracks only the running minimum (there is no index to recover):
//     load the queries, the point minimum over the other cloud through the kernel's own LDS tile, the statistics;
//   * shape_combine_kernel: the core's combine under its name;
//   * the size check and the entry point.
#include "common.h"
#include "shape_score_core.h"

#pragma clang fp contract(off)

namespace {

using namespace shape_core;

constexpr int kQPT = 4;                 // queries per thread
constexpr int kSlab = kThreads * kQPT;  // queries per workgroup

using Ws = Workspace<float, 0>;

__global__ __launch_bounds__(kThreads) void shape_search_kernel(
    const float *__restrict__ a, const float *__restrict__ mask_a, int P, const float *__restrict__ b,
    const float *__restrict__ mask_b, int Q, int slabs, long long items, Thresholds thr,
    char *__restrict__ workspace, float *__restrict__ dist_a, float *__restrict__ dist_b)
{
    __shared__ float4 tile[kTile];
    __shared__ StatsLds<float> stats;
    const int n_thr = stage_thresholds(thr, stats);

    for (unsigned w = blockIdx.x; w < (unsigned)items; w += gridDim.x) {
        const WorkItem<float> it(w, slabs, a, mask_a, P, b, mask_b, Q, dist_a, dist_b);
        const int qbase = it.slab * kSlab;
        float q[kQPT][3], best[kQPT];
        bool ok[kQPT];
        load_queries<kQPT>(it.q, it.qmask, it.q0, it.nq, qbase, q, ok);
        // a slab without a query (the shorter cloud's tail) searches nothing and leaves zeros
        point_minimum<kQPT>(tile, it.r, it.rmask, it.r0, qbase < it.nq ? it.nr : 0, q, best);
        slab_statistics<float, kQPT, 0>(stats, ok, best, it.dist != nullptr ? it.dist + it.q0 : nullptr, it.nq, qbase,
                                        n_thr, workspace, items, w, 0);
        if (last_pass(w, items)) break;
    }
}

__global__ __launch_bounds__(kCombineThreads) void shape_combine_kernel(
    int n, int P, int Q, int slabs, int T, const char *__restrict__ workspace, int *__restrict__ counts,
    double *__restrict__ sums, float *__restrict__ table, float *__restrict__ dist_a, float *__restrict__ dist_b)
{
    combine_boxes<float, 0>(n, P, Q, slabs, T, workspace, counts, sums, table, dist_a, dist_b, nullptr);
}

bool sizes_fit(int n, int P, int Q)
{
    const long long big = P > Q ? P : Q;
    return (long long)n * big < (1LL << 31);
}

}  // namespace

extern "C" size_t mpsr_shape_scores_workspace_bytes(int n, int P, int Q, int T)
{
    if (n <= 0 || P < 0 || Q < 0 || T < 0 || T > kMaxT || !sizes_fit(n, P, Q)) return 0;
    return Ws(n, P > Q ? P : Q, kSlab, T).bytes;
}

extern "C" int mpsr_shape_scores(const float *a, const float *mask_a, int P, const float *b, const float *mask_b,
                                 int Q, int n, const double *thresholds, int T, void *workspace,
                                 size_t workspace_bytes, int *counts, double *sums, float *table, float *dist_a,
                                 float *dist_b, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0 && P >= 0 && Q >= 0, "shape_scores: negative size (n=%d P=%d Q=%d)", n, P, Q);
    Thresholds thr;
    if (const int status = fill_thresholds("shape_scores", thresholds, T, &thr)) return status;
    MPSR_REQUIRE(sizes_fit(n, P, Q), "shape_scores: n max(P, Q) = %d x %d does not fit 31 bits", n, P > Q ? P : Q);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE((P == 0 || a) && (Q == 0 || b), "shape_scores: a cloud pointer is null (P=%d Q=%d)", P, Q);
    MPSR_REQUIRE(counts && sums && table, "shape_scores: an output pointer is null with n = %d", n);
    const Ws ws(n, P > Q ? P : Q, kSlab, T);
    if (const int status = ws.check("shape_scores", workspace, workspace_bytes)) return status;
    hipStream_t s = mpsr::as_stream(stream);
    hipLaunchKernelGGL(shape_search_kernel, ws.search_grid(), dim3(kThreads), 0, s, a, mask_a, P, b, mask_b, Q,
                       ws.slabs, ws.items, thr, static_cast<char *>(workspace), dist_a, dist_b);
    MPSR_CHECK_LAUNCH("shape_search_kernel");
    hipLaunchKernelGGL(shape_combine_kernel, Ws::combine_grid(n), dim3(kCombineThreads), 0, s, n, P, Q, ws.slabs, T,
                       static_cast<const char *>(workspace), counts, sums, table, dist_a, dist_b);
    MPSR_CHECK_LAUNCH("shape_combine_kernel");
    return MPSR_OK;
}

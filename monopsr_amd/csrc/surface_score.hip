// Shape scores against surfaces (mpsr_surface_scores): mpsr_shape_scores' statistics, but the
// distance of a valid point is taken to the other grid's triangulated surface -- its valid points and the kept
// triangles of section 7.9's indexing -- instead of to its nearest valid point alone.
//
// Everything it has in common with mpsr_shape_scores lives in shape_score_core.h: the validity rule, the thresholds,
// the work items, the point minimum (so the point term IS mpsr_shape_scores' d), the slab statistics, the combine and
// the workspace, here with D = double and one more count per work item.  This file holds the triangles.  The edge and
// face terms are fp64 on the coordinates converted exactly, every dot product (x x + y y) + z z.  Nothing is contracted
// (the file is compiled with -ffp-contract=off and repeats that as a pragma) and a minimum does not depend on its
// order, so every d is the header's definition bit for bit.
//
// surface_search_kernel, one workgroup per (box, direction, slab of kSlab queries):
//   * the point minimum first, its tile in the records' LDS;
//   * then the triangles, kThreads ids to a pass: thread i decides whether triangle t0 + i is KEPT (three valid
//     vertices, three float32 squared edge lengths within max_edge^2) and, if so, works out its record -- the corners
//     and the quantities that do not depend on the query: e0, eBC, e1, d00, eeBC, d11, d01, den, n, nn.  The kept
//     records are compacted into LDS in id order by ranks from wave ballots (no atomics) and read back at wave-uniform
//     addresses; each thread carries kQPT queries and only their running minima.  The divisions sit under their
//     predicates.  There is no setup kernel and no table of records in memory: a record costs about as much as one
//     (query, triangle) pair, so working it out again in each of the box's slabs is 1 / kSlab of the search, and a
//     table would take 2 (h - 1)(w - 1) 2 n records of 216 bytes, 0.5 GB for 256 boxes of 48 x 48;
//   * the statistics, with the number of kept triangles of the grid it searched as the work item's last count (the
//     combine reads slab 0's).
// surface_combine_kernel: the core's combine under its name, with tri_counts.
#include "common.h"
#include "shape_score_core.h"

#pragma clang fp contract(off)

namespace {

using namespace shape_core;

constexpr int kQPT = 2;                  // queries per thread
constexpr int kSlab = kThreads * kQPT;   // queries per workgroup
constexpr int kTriTile = kThreads;       // triangle ids per pass, one per thread
constexpr int kRec = 28;                 // doubles per triangle record (27 used; 16-byte aligned records)

// the record's slots
enum { kA = 0, kB = 3, kC = 6, kE0 = 9, kEBC = 12, kE1 = 15, kD00 = 18, kEEBC = 19, kD11 = 20, kD01 = 21, kDen = 22,
       kN = 23, kNN = 26 };

static_assert(kTile * sizeof(float4) <= kTriTile * kRec * sizeof(double), "the point tile shares the records' LDS");

using Ws = Workspace<double, 1>;

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

// the float32 squared length of the edge u -> v, nn_distance's arithmetic
__device__ __forceinline__ float edge_len2(const float *u, const float *v)
{
    const float dx = v[0] - u[0], dy = v[1] - u[1], dz = v[2] - u[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// The edge term of the query with w = q - U against the edge e = V - U, ee = e.e, t = w.e: -> the lower of it and best.
__device__ __forceinline__ double edge_term(double best, double wx, double wy, double wz, double ex, double ey,
                                            double ez, double ee, double t)
{
    if (ee > 0.0 && t > 0.0 && t < ee) {
        const double s = t / ee;
        const double rx = wx - s * ex, ry = wy - s * ey, rz = wz - s * ez;
        const double term = dot3(rx, ry, rz, rx, ry, rz);
        best = term < best ? term : best;
    }
    return best;
}

// The three edge terms and the face term of one kept triangle (its record R, read at a wave-uniform address).
__device__ __forceinline__ double triangle_terms(const double *__restrict__ R, double qx, double qy, double qz,
                                                 double best)
{
    const double e0x = R[kE0], e0y = R[kE0 + 1], e0z = R[kE0 + 2];
    const double e1x = R[kE1], e1y = R[kE1 + 1], e1z = R[kE1 + 2];
    const double d00 = R[kD00], d11 = R[kD11];
    // (A, B): U = A, e = e0, ee = d00
    const double wax = qx - R[kA], way = qy - R[kA + 1], waz = qz - R[kA + 2];
    const double d20 = dot3(wax, way, waz, e0x, e0y, e0z);
    best = edge_term(best, wax, way, waz, e0x, e0y, e0z, d00, d20);
    // (B, C)
    {
        const double ex = R[kEBC], ey = R[kEBC + 1], ez = R[kEBC + 2];
        const double wx = qx - R[kB], wy = qy - R[kB + 1], wz = qz - R[kB + 2];
        best = edge_term(best, wx, wy, wz, ex, ey, ez, R[kEEBC], dot3(wx, wy, wz, ex, ey, ez));
    }
    // (C, A): e = A - C = -e1 and e.e = d11, both exactly
    {
        const double ex = -e1x, ey = -e1y, ez = -e1z;
        const double wx = qx - R[kC], wy = qy - R[kC + 1], wz = qz - R[kC + 2];
        best = edge_term(best, wx, wy, wz, ex, ey, ez, d11, dot3(wx, wy, wz, ex, ey, ez));
    }
    // the face
    const double nn = R[kNN], den = R[kDen];
    if (nn > 0.0 && den > 0.0) {  // (the same for every lane)
        const double d01 = R[kD01];
        const double d21 = dot3(wax, way, waz, e1x, e1y, e1z);
        const double v = d11 * d20 - d01 * d21, u = d00 * d21 - d01 * d20;
        if (v > 0.0 && u > 0.0 && v + u < den) {
            const double hq = dot3(wax, way, waz, R[kN], R[kN + 1], R[kN + 2]);
            const double term = hq * hq / nn;
            best = term < best ? term : best;
        }
    }
    return best;
}

__global__ __launch_bounds__(kThreads) void surface_search_kernel(
    const float *__restrict__ a, const float *__restrict__ mask_a, const float *__restrict__ b,
    const float *__restrict__ mask_b, int map_h, int map_w, int slabs, long long items, double max_edge_sq,
    Thresholds thr, char *__restrict__ workspace, double *__restrict__ dist_a, double *__restrict__ dist_b)
{
    __shared__ __attribute__((aligned(16))) double rec[kTriTile * kRec];
    __shared__ int wkept[kWaves];
    __shared__ StatsLds<double> stats;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int n_thr = stage_thresholds(thr, stats);
    const int P = map_h * map_w;
    const int cells_w = map_w - 1;
    const int n_tri = 2 * (map_h - 1) * cells_w;

    for (unsigned w = blockIdx.x; w < (unsigned)items; w += gridDim.x) {
        const WorkItem<double> it(w, slabs, a, mask_a, P, b, mask_b, P, dist_a, dist_b);
        const float *r = it.r, *rmask = it.rmask;
        const long long p0 = it.r0;
        const int qbase = it.slab * kSlab;

        float qf[kQPT][3], best[kQPT];
        bool ok[kQPT];
        load_queries<kQPT>(it.q, it.qmask, p0, P, qbase, qf, ok);
#pragma unroll
        for (int u = 0; u < kQPT; ++u)
            if (!ok[u]) qf[u][0] = qf[u][1] = qf[u][2] = 0.f;

        // the point minimum: mpsr_shape_scores' d
        point_minimum<kQPT>(reinterpret_cast<float4 *>(rec), r, rmask, p0, P, qf, best);

        double d[kQPT], qd[kQPT][3];
#pragma unroll
        for (int u = 0; u < kQPT; ++u) {
            d[u] = (double)best[u];
            qd[u][0] = (double)qf[u][0];
            qd[u][1] = (double)qf[u][1];
            qd[u][2] = (double)qf[u][2];
        }

        // the kept triangles of the searched grid, kTriTile ids to a pass
        int kept_total = 0;
        for (int t0 = 0; t0 < n_tri; t0 += kTriTile) {
            const int t = t0 + tid;
            bool kept = false;
            float A[3], B[3], C[3];
            if (t < n_tri) {
                // triangle_corners' indexing (scene.hip): k = 0: (v00, v01, v10); k = 1: (v11, v10, v01)
                const int cell = t >> 1;
                const int v00 = (cell / cells_w) * map_w + cell % cells_w;
                const bool k = t & 1;
                const int ia = k ? v00 + map_w + 1 : v00;
                const int ib = k ? v00 + map_w : v00 + 1;
                const int ic = k ? v00 + 1 : v00 + map_w;
                const bool va = load_point(r, rmask, p0 + ia, true, A);
                const bool vb = load_point(r, rmask, p0 + ib, true, B);
                const bool vc = load_point(r, rmask, p0 + ic, true, C);
                kept = va && vb && vc && (double)edge_len2(A, B) <= max_edge_sq &&
                       (double)edge_len2(B, C) <= max_edge_sq && (double)edge_len2(C, A) <= max_edge_sq;
            }
            const unsigned long long votes = __ballot(kept);
            __syncthreads();  // the previous pass has read the records and wkept (the first: the point tile)
            if (lane == 0) wkept[wave] = __popcll(votes);
            __syncthreads();
            int at = __popcll(votes & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int v = 0; v < kWaves; ++v) {
                at += v < wave ? wkept[v] : 0;
                total += wkept[v];
            }
            if (kept) {
                double *R = rec + at * kRec;
                const double ax = A[0], ay = A[1], az = A[2], bx = B[0], by = B[1], bz = B[2];
                const double cx = C[0], cy = C[1], cz = C[2];
                const double e0x = bx - ax, e0y = by - ay, e0z = bz - az;
                const double e1x = cx - ax, e1y = cy - ay, e1z = cz - az;
                const double ebx = cx - bx, eby = cy - by, ebz = cz - bz;
                const double nx = e0y * e1z - e0z * e1y, ny = e0z * e1x - e0x * e1z, nz = e0x * e1y - e0y * e1x;
                const double d00 = dot3(e0x, e0y, e0z, e0x, e0y, e0z), d01 = dot3(e0x, e0y, e0z, e1x, e1y, e1z);
                const double d11 = dot3(e1x, e1y, e1z, e1x, e1y, e1z);
                R[kA] = ax, R[kA + 1] = ay, R[kA + 2] = az;
                R[kB] = bx, R[kB + 1] = by, R[kB + 2] = bz;
                R[kC] = cx, R[kC + 1] = cy, R[kC + 2] = cz;
                R[kE0] = e0x, R[kE0 + 1] = e0y, R[kE0 + 2] = e0z;
                R[kEBC] = ebx, R[kEBC + 1] = eby, R[kEBC + 2] = ebz;
                R[kE1] = e1x, R[kE1 + 1] = e1y, R[kE1 + 2] = e1z;
                R[kD00] = d00;
                R[kEEBC] = dot3(ebx, eby, ebz, ebx, eby, ebz);
                R[kD11] = d11;
                R[kD01] = d01;
                R[kDen] = d00 * d11 - d01 * d01;
                R[kN] = nx, R[kN + 1] = ny, R[kN + 2] = nz;
                R[kNN] = dot3(nx, ny, nz, nx, ny, nz);
            }
            __syncthreads();
            kept_total += total;
            for (int k = 0; k < total; ++k) {
                const double *R = rec + k * kRec;
#pragma unroll
                for (int u = 0; u < kQPT; ++u) d[u] = triangle_terms(R, qd[u][0], qd[u][1], qd[u][2], d[u]);
            }
        }

        slab_statistics<double, kQPT, 1>(stats, ok, d, it.dist != nullptr ? it.dist + p0 : nullptr, P, qbase, n_thr,
                                         workspace, items, w, kept_total);
        if (last_pass(w, items)) break;
    }
}

__global__ __launch_bounds__(kCombineThreads) void surface_combine_kernel(
    int n, int P, int slabs, int T, const char *__restrict__ workspace, int *__restrict__ counts,
    double *__restrict__ sums, float *__restrict__ table, double *__restrict__ dist_a, double *__restrict__ dist_b,
    int *__restrict__ tri_counts)
{
    combine_boxes<double, 1>(n, P, P, slabs, T, workspace, counts, sums, table, dist_a, dist_b, tri_counts);
}

// n h w < 2^31 (the point indices are ints) and h w <= 2^30 (so are the triangle ids)
bool sizes_fit(int n, int h, int w)
{
    const long long P = (long long)h * w;
    return P <= (1LL << 30) && (long long)n * P < (1LL << 31);
}

}  // namespace

extern "C" size_t mpsr_surface_scores_workspace_bytes(int n, int h, int w, int T)
{
    if (n <= 0 || h < 1 || w < 1 || T < 0 || T > kMaxT || !sizes_fit(n, h, w)) return 0;
    return Ws(n, h * w, kSlab, T).bytes;
}

extern "C" int mpsr_surface_scores(const float *a, const float *mask_a, const float *b, const float *mask_b, int n,
                                   int h, int w, const double *thresholds, int T, double max_edge, void *workspace,
                                   size_t workspace_bytes, int *counts, double *sums, float *table, double *dist_a,
                                   double *dist_b, int *tri_counts, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0, "surface_scores: negative size (n=%d)", n);
    MPSR_REQUIRE(h >= 1 && w >= 1, "surface_scores: a grid of %d x %d has no point", h, w);
    Thresholds thr;
    if (const int status = fill_thresholds("surface_scores", thresholds, T, &thr)) return status;
    // (NaN fails the comparison)
    MPSR_REQUIRE(max_edge >= 0.0, "surface_scores: max_edge = %g is not a length >= 0", max_edge);
    MPSR_REQUIRE(sizes_fit(n, h, w), "surface_scores: n h w = %d x %d x %d does not fit 31 bits", n, h, w);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(a && b, "surface_scores: a grid pointer is null");
    MPSR_REQUIRE(counts && sums && table && tri_counts, "surface_scores: an output pointer is null with n = %d", n);
    const int P = h * w;
    const Ws ws(n, P, kSlab, T);
    if (const int status = ws.check("surface_scores", workspace, workspace_bytes)) return status;
    hipStream_t s = mpsr::as_stream(stream);
    hipLaunchKernelGGL(surface_search_kernel, ws.search_grid(), dim3(kThreads), 0, s, a, mask_a, b, mask_b, h, w,
                       ws.slabs, ws.items, max_edge * max_edge, thr, static_cast<char *>(workspace), dist_a, dist_b);
    MPSR_CHECK_LAUNCH("surface_search_kernel");
    hipLaunchKernelGGL(surface_combine_kernel, Ws::combine_grid(n), dim3(kCombineThreads), 0, s, n, P, ws.slabs, T,
                       static_cast<const char *>(workspace), counts, sums, table, dist_a, dist_b, tri_counts);
    MPSR_CHECK_LAUNCH("surface_combine_kernel");
    return MPSR_OK;
}

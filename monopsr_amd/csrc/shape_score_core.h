// The shape scores' single body (DESIGN.md sections 7.14 and 7.15): what mpsr_shape_scores (shape_score.hip, distances
// to the nearest valid point, D = float) and mpsr_surface_scores (surface_score.hip, distances to the triangulated
// surface, D = double) must agree on to be comparable.  D is at once the type of a query's d, of the dist rows and of
// the stored maximum.
//
//   * load_point: a point is valid when its mask entry is > 0 and its three coordinates are finite;
//   * Thresholds: the host checks of (thresholds, T) and the staging of their squares into LDS;
//   * the work items w = (box * 2 + direction) * slabs + slab, one workgroup each: their decode, the grid's clamp and
//     the exit test of the grid-stride loop;
//   * point_minimum: the searched cloud staged through LDS as float4 tiles and read back with wave-uniform
//     ds_read_b128, as in nn_search_kernel; a searched point that is not valid is staged as a +inf point, never wins.
//     The distances are nn_distance.hip's: float differences, float products, (dx*dx + dy*dy) + dz*dz, two queries to a
//     packed pair; nothing is contracted (both files are compiled with -ffp-contract=off and this header repeats that
//     as a pragma), so with null masks and finite clouds every d equals mpsr_nn_distance_fwd's bit for bit;
//   * slab_statistics: the valid queries' d go to the dist row (NaN at the others); the counts come from ballots; each
//     thread adds sqrt((double) d) and (double) d of its queries in slice order, and the workgroup reduces them as
//     scene.hip's block_tally does: a lane-ordered wave tree, wave partials through LDS, a combine in wave order;
//     thread 0 leaves the slab's partials in the workspace;
//   * combine_boxes, one thread per box: adds the partials in slab order and writes counts, sums and table; a box with
//     an empty side gets its NaN rows there, and its dist rows are overwritten with NaN: by that one thread, element by
//     element, after the search has run for the box.  That is the price of a search that need not know an empty side
//     beforehand (it would take a counting pass over both masks in front of it); it is paid only where dist rows are
//     asked for and a box has an empty side, which the evaluator never does;
//   * Workspace: where the partials lie, for the kernels, the *_workspace_bytes functions and the entry points' checks.
// No floating-point atomics and no order that depends on scheduling: two calls return the same bytes.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace shape_core {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 1024;              // searched points per LDS tile (16 KiB as float4)
constexpr int kChunk = 8;                // the point loop's unrolled run; tiles are padded to it with +inf points
constexpr int kMaxT = MPSR_SHAPE_MAX_THRESHOLDS;
constexpr int kCombineThreads = 64;
constexpr unsigned kMaxGrid = 1u << 20;  // work items beyond it are reached by the grid's stride

using f32x2 = __attribute__((ext_vector_type(2))) float;

__device__ __forceinline__ float max_of(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double max_of(double a, double b) { return fmax(a, b); }

struct Thresholds {
    double sq[kMaxT];  // thresholds[t] * thresholds[t]
    int n;
};

// (thresholds, T) -> thr, or the status of what is wrong with them; `who` is the entry point's name in the message
inline int fill_thresholds(const char *who, const double *thresholds, int T, Thresholds *thr)
{
    MPSR_REQUIRE(T >= 0 && T <= kMaxT, "%s: %d thresholds, outside 0..%d", who, T, kMaxT);
    MPSR_REQUIRE(T == 0 || thresholds, "%s: thresholds is null", who);
    thr->n = T;
    for (int t = 0; t < kMaxT; ++t) thr->sq[t] = 0.0;
    for (int t = 0; t < T; ++t) {
        MPSR_REQUIRE(std::isfinite(thresholds[t]) && thresholds[t] > 0.0,
                     "%s: thresholds[%d] = %g is not a finite distance > 0", who, t, thresholds[t]);
        MPSR_REQUIRE(t == 0 || thresholds[t] > thresholds[t - 1],
                     "%s: thresholds[%d] = %g is not increasing (after %g)", who, t, thresholds[t], thresholds[t - 1]);
        thr->sq[t] = thresholds[t] * thresholds[t];
    }
    return MPSR_OK;
}

// The workspace, three arrays over the work items: two fp64 sums each (of the roots, of d), then one maximum of type D
// each, then 1 + T + kExtra int32 counts each (the valid queries, the queries within each threshold, and for the
// surfaces the kept triangles of the searched grid: slab 0 only).  The total is rounded up to 8 bytes.
template <typename D, int kExtra>
struct Workspace {
    static constexpr long long kSumBytes = 2 * sizeof(double), kMaxBytes = sizeof(D);

    long long items;  // n * 2 * slabs
    int slabs;        // per (box, direction): the slabs of the longer side, one where it has no point
    size_t bytes;

    Workspace(int n, int longer, int slab_queries, int T)
    {
        slabs = longer > 0 ? (int)(((long long)longer + slab_queries - 1) / slab_queries) : 1;
        items = (long long)n * 2 * slabs;
        const long long per_item = kSumBytes + kMaxBytes + (long long)sizeof(int) * counts_per_item(T);
        bytes = mpsr::align_up((size_t)per_item * (size_t)items, 8);
    }

    __host__ __device__ static int counts_per_item(int T) { return 1 + T + kExtra; }
    // the byte offsets of the maxima and of the counts (the sums come first)
    __host__ __device__ static long long maxima_at(long long items) { return kSumBytes * items; }
    __host__ __device__ static long long counts_at(long long items) { return (kSumBytes + kMaxBytes) * items; }

    // the entry point's checks of the caller's workspace
    int check(const char *who, const void *workspace, size_t workspace_bytes) const
    {
        MPSR_REQUIRE(workspace, "%s: workspace is null", who);
        MPSR_REQUIRE((uintptr_t)workspace % sizeof(double) == 0, "%s: workspace is not 8-byte aligned", who);
        if (workspace_bytes < bytes)
            return mpsr::fail(MPSR_ERR_WORKSPACE, "%s: workspace %zu bytes < %zu", who, workspace_bytes, bytes);
        return MPSR_OK;
    }
    dim3 search_grid() const { return dim3((unsigned)(items < (long long)kMaxGrid ? items : (long long)kMaxGrid)); }
    static dim3 combine_grid(int n) { return dim3((unsigned)mpsr::ceil_div(n, kCombineThreads)); }
};

// what a workgroup shares for the statistics
template <typename D>
struct alignas(16) StatsLds {  // (16 bytes: thread 0 reads a row of wave partials at once)
    int cpart[1 + kMaxT][kWaves];
    double dpart[2][kWaves];
    D mpart[kWaves];
    double thr_sq[kMaxT];  // (read back in a loop over t: sixteen scalar registers less than the argument)
};

// thr's squares into LDS, once per workgroup: -> the number of thresholds
template <typename D>
__device__ __forceinline__ int stage_thresholds(const Thresholds &thr, StatsLds<D> &lds)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int t = 0; t < kMaxT; ++t)
        if (tid == t) lds.thr_sq[t] = thr.sq[t];
    __syncthreads();
    return thr.n;
}

// Point i of cloud p where `live`, else nothing: -> is it valid, its coordinates in v.  Without short-circuits: one
// run of loads and one combined test.
__device__ __forceinline__ bool load_point(const float *p, const float *mask, long long i, bool live, float *v)
{
    float m = 0.f;
    v[0] = v[1] = v[2] = 0.f;
    if (live) {
        v[0] = p[3 * i];
        v[1] = p[3 * i + 1];
        v[2] = p[3 * i + 2];
        m = mask != nullptr ? mask[i] : 1.f;
    }
    // (a NaN mask fails the comparison)
    return ((int)(m > 0.0f) & (int)isfinite(v[0]) & (int)isfinite(v[1]) & (int)isfinite(v[2])) != 0;
}

// Work item w: direction 0 takes its queries from a and searches b, direction 1 the other way round.
template <typename D>
struct WorkItem {
    const float *q, *qmask, *r, *rmask;  // the queries' cloud and the searched one, with their masks
    D *dist;                             // the queries' dist rows, or null
    long long box, q0, r0;               // the box's first query and first searched point
    int dir, slab, nq, nr;

    __device__ __forceinline__ WorkItem(unsigned w, int slabs, const float *a, const float *mask_a, int P,
                                        const float *b, const float *mask_b, int Q, D *dist_a, D *dist_b)
    {
        const unsigned pair = w / (unsigned)slabs;
        slab = (int)(w - pair * (unsigned)slabs);
        dir = (int)(pair & 1u);
        box = pair >> 1;
        nq = dir ? Q : P;
        nr = dir ? P : Q;
        q = dir ? b : a;
        qmask = dir ? mask_b : mask_a;
        r = dir ? a : b;
        rmask = dir ? mask_a : mask_b;
        dist = dir ? dist_b : dist_a;
        q0 = box * nq, r0 = box * nr;  // (box * max(P, Q) < 2^31: the entry points' checks)
    }
};

// The search kernels' loop is `for (unsigned w = blockIdx.x; w < (unsigned)items; w += gridDim.x)` (items < 2^32), left
// behind its last pass by this test in front of the step, which keeps w from wrapping.
__device__ __forceinline__ bool last_pass(unsigned w, long long items) { return (unsigned)items - w <= gridDim.x; }

// The thread's kQ queries of the slab that starts at query qbase, one in every kThreads-th part of it: -> q, ok.
template <int kQ>
__device__ __forceinline__ void load_queries(const float *p, const float *mask, long long q0, int nq, int qbase,
                                             float (*q)[3], bool *ok)
{
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
        const int j = qbase + u * kThreads + (int)threadIdx.x;
        ok[u] = load_point(p, mask, q0 + j, j < nq, q[u]);
    }
}

// best[u] = the least float (dx*dx + dy*dy) + dz*dz of query u over the valid points r0 .. r0 + nr of r, +inf over
// none.  tile: kTile float4 of LDS that the workgroup may overwrite (a barrier stands in front of the first write).
template <int kQ>
__device__ __forceinline__ void point_minimum(float4 *tile, const float *r, const float *rmask, long long r0, int nr,
                                              const float (*q)[3], float *best)
{
    // two queries to a 2-wide vector, as in nn_search_kernel: packed fp32 subtract / multiply / add are IEEE-exact and
    // nothing is contracted, so every distance keeps the bits of (dx*dx + dy*dy) + dz*dz
    static_assert(kQ % 2 == 0, "packed search arithmetic pairs the queries of a thread");
    const int tid = threadIdx.x;
    const float inf = __builtin_inff();
    f32x2 vqx[kQ / 2], vqy[kQ / 2], vqz[kQ / 2], vbest[kQ / 2];
#pragma unroll
    for (int v = 0; v < kQ / 2; ++v) {
        vqx[v] = f32x2{q[2 * v][0], q[2 * v + 1][0]};
        vqy[v] = f32x2{q[2 * v][1], q[2 * v + 1][1]};
        vqz[v] = f32x2{q[2 * v][2], q[2 * v + 1][2]};
        vbest[v] = f32x2{inf, inf};
    }
    for (int t0 = 0; t0 < nr; t0 += kTile) {
        const int cnt = min(kTile, nr - t0);
        const int cntp = (cnt + kChunk - 1) / kChunk * kChunk;
        __syncthreads();
        for (int p = tid; p < cntp; p += kThreads) {
            float v[3];
            const bool valid = load_point(r, rmask, r0 + t0 + p, p < cnt, v);
            tile[p] = valid ? make_float4(v[0], v[1], v[2], 0.f) : make_float4(inf, inf, inf, 0.f);
        }
        __syncthreads();
        // A run in three steps -- its points, every distance, then the minima -- so that the schedule is the source's:
        // the eight LDS reads in flight together and the distances' independent chains interleaved.  With the minimum
        // taken inside the distance loop the compiler's choice between that and a serial, register-saving order hung
        // on code far from the loop, and the serial one costs a 32-box call a third more time.
        for (int k0 = 0; k0 < cntp; k0 += kChunk) {
            float4 rp[kChunk];
#pragma unroll
            for (int s = 0; s < kChunk; ++s) rp[s] = tile[k0 + s];
            f32x2 dd[kChunk][kQ / 2];
#pragma unroll
            for (int s = 0; s < kChunk; ++s) {
#pragma unroll
                for (int v = 0; v < kQ / 2; ++v) {
                    const f32x2 dx = rp[s].x - vqx[v], dy = rp[s].y - vqy[v], dz = rp[s].z - vqz[v];
                    dd[s][v] = (dx * dx + dy * dy) + dz * dz;
                }
            }
#pragma unroll
            for (int s = 0; s < kChunk; ++s) {
#pragma unroll
                for (int v = 0; v < kQ / 2; ++v) vbest[v] = __builtin_elementwise_min(vbest[v], dd[s][v]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < kQ / 2; ++v) {
        best[2 * v] = vbest[v][0];
        best[2 * v + 1] = vbest[v][1];
    }
}

// The statistics of work item w over the slab's queries (ok[u], d[u]: load_queries' order), left in the workspace by
// thread 0: counts per wave from ballots, sums per thread in slice order.  dist_row: the box's dist row, or null.
// extra: the item's last count where kExtra is 1.
template <typename D, int kQ, int kExtra>
__device__ __forceinline__ void slab_statistics(StatsLds<D> &lds, const bool *ok, const D *d, D *dist_row, int nq,
                                                int qbase, int n_thr, char *workspace, long long items, unsigned w,
                                                int extra)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();  // the previous work item's combine has read the partials
    double s_root = 0.0, s_sq = 0.0;
    D mx = 0;  // (d >= 0: the maximum over no query is never read, an empty side's row is NaN)
    int n_ok = 0;
#pragma unroll
    for (int u = 0; u < kQ; ++u) {
        const int j = qbase + u * kThreads + tid;
        if (ok[u]) {
            s_root += sqrt((double)d[u]);
            s_sq += (double)d[u];
            mx = max_of(mx, d[u]);
        }
        n_ok += __popcll(__ballot(ok[u]));
        if (dist_row != nullptr && j < nq) dist_row[j] = ok[u] ? d[u] : (D)__builtin_nan("");
    }
    for (int t = 0; t < n_thr; ++t) {
        const double limit = lds.thr_sq[t];
        int within = 0;
#pragma unroll
        for (int u = 0; u < kQ; ++u) within += __popcll(__ballot(ok[u] && (double)d[u] <= limit));
        if (lane == 0) lds.cpart[1 + t][wave] = within;
    }
    for (int o = 32; o > 0; o >>= 1) {
        s_root += __shfl_down(s_root, o);
        s_sq += __shfl_down(s_sq, o);
        mx = max_of(mx, __shfl_down(mx, o));
    }
    if (lane == 0) {
        lds.cpart[0][wave] = n_ok;
        lds.dpart[0][wave] = s_root;
        lds.dpart[1][wave] = s_sq;
        lds.mpart[wave] = mx;
    }
    __syncthreads();
    if (tid == 0) {
        using Ws = Workspace<D, kExtra>;
        double t_root = 0.0, t_sq = 0.0;
        D t_max = 0;
        for (int v = 0; v < kWaves; ++v) {  // in wave order
            t_root += lds.dpart[0][v];
            t_sq += lds.dpart[1][v];
            t_max = max_of(t_max, lds.mpart[v]);
        }
        double *part_sums = reinterpret_cast<double *>(workspace);
        part_sums[2 * (long long)w] = t_root;
        part_sums[2 * (long long)w + 1] = t_sq;
        reinterpret_cast<D *>(workspace + Ws::maxima_at(items))[w] = t_max;
        int *pc = reinterpret_cast<int *>(workspace + Ws::counts_at(items)) + (long long)w * Ws::counts_per_item(n_thr);
        for (int k = 0; k < 1 + n_thr; ++k) {
            int total = 0;
            for (int v = 0; v < kWaves; ++v) total += lds.cpart[k][v];
            pc[k] = total;
        }
        if (kExtra) pc[1 + n_thr] = extra;
    }
}

// One thread per box: adds the slabs' partials in slab order and writes the box's rows.  tri_counts (kExtra = 1): the
// kept triangles of a and of b, from the first slab of the direction that searched each.
template <typename D, int kExtra>
__device__ __forceinline__ void combine_boxes(int n, int P, int Q, int slabs, int T, const char *workspace, int *counts,
                                              double *sums, float *table, D *dist_a, D *dist_b, int *tri_counts)
{
    using Ws = Workspace<D, kExtra>;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long long items = (long long)n * 2 * slabs;
    const int per = Ws::counts_per_item(T);
    const double *part_sums = reinterpret_cast<const double *>(workspace);
    const D *part_max = reinterpret_cast<const D *>(workspace + Ws::maxima_at(items));
    const int *part_counts = reinterpret_cast<const int *>(workspace + Ws::counts_at(items));
    const long long box = (long long)blockIdx.x * kCombineThreads + threadIdx.x;
    if (box >= n) return;
    int nv[2] = {0, 0};
    double s[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    D mx[2] = {0, 0};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const long long w0 = (box * 2 + dir) * slabs;
        for (int k = 0; k < slabs; ++k) {  // in slab order
            nv[dir] += part_counts[(w0 + k) * per];
            s[dir][0] += part_sums[2 * (w0 + k)];
            s[dir][1] += part_sums[2 * (w0 + k) + 1];
            mx[dir] = max_of(mx[dir], part_max[w0 + k]);
        }
    }
    if (kExtra) {  // direction 0 searched b, direction 1 searched a
        tri_counts[2 * box] = part_counts[((box * 2 + 1) * slabs) * per + 1 + T];
        tri_counts[2 * box + 1] = part_counts[((box * 2) * slabs) * per + 1 + T];
    }
    const bool empty = nv[0] == 0 || nv[1] == 0;
    int *c = counts + box * (2 + 2 * T);
    double *so = sums + box * 6;
    float *row = table + box * (5 + 3 * T);
    c[0] = nv[0];
    c[1] = nv[1];
    if (empty) {
        for (int k = 0; k < 2 * T; ++k) c[2 + k] = 0;
        for (int k = 0; k < 6; ++k) so[k] = nan;
        for (int k = 0; k < 5 + 3 * T; ++k) row[k] = __builtin_nanf("");
        // the search left +inf at the valid points of the side that is not empty
        if (dist_a != nullptr)
            for (int j = 0; j < P; ++j) dist_a[box * P + j] = (D)__builtin_nan("");
        if (dist_b != nullptr)
            for (int j = 0; j < Q; ++j) dist_b[box * Q + j] = (D)__builtin_nan("");
        return;
    }
    const double na = (double)nv[0], nb = (double)nv[1];
    so[0] = s[0][0];
    so[1] = s[0][1];
    so[2] = s[1][0];
    so[3] = s[1][1];
    so[4] = (double)mx[0];
    so[5] = (double)mx[1];
    const double accuracy = s[0][0] / na, completeness = s[1][0] / nb;
    row[0] = (float)accuracy;
    row[1] = (float)completeness;
    row[2] = (float)((accuracy + completeness) / 2);
    row[3] = (float)(s[0][1] / na + s[1][1] / nb);
    row[4] = (float)sqrt((double)max_of(mx[0], mx[1]));
    for (int t = 0; t < T; ++t) {
        int within[2] = {0, 0};
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const long long w0 = (box * 2 + dir) * slabs;
            for (int k = 0; k < slabs; ++k) within[dir] += part_counts[(w0 + k) * per + 1 + t];
        }
        c[2 + t] = within[0];
        c[2 + T + t] = within[1];
        const double p = (double)within[0] / na, r = (double)within[1] / nb;
        row[5 + 3 * t] = (float)p;
        row[5 + 3 * t + 1] = (float)r;
        row[5 + 3 * t + 2] = (float)(p + r == 0.0 ? 0.0 : 2 * p * r / (p + r));
    }
}

}  // namespace shape_core

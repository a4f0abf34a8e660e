// Shape scores over valid points (mpsr_shape_scores): the masked Chamfer search of two clouds
// per box with its statistics -- accuracy, completeness, Chamfer-L1, squared Chamfer, Hausdorff and precision / recall
// / F-score at distance thresholds.
//
// The distances are nn_distance.hip's: float differences, float products, (dx*dx + dy*dy) + dz*dz, nothing contracted
// (the file is compiled with -ffp-contract=off and repeats that as a pragma), so with null masks and finite clouds
// every d equals mpsr_nn_distance_fwd's bit for bit.
//
// shape_search_kernel, one workgroup per (box, direction, slab of kSlab queries):
//   * the searched cloud is staged through LDS as float4 tiles and read back with wave-uniform ds_read_b128, as in
//     nn_search_kernel; a searched point that is not valid is staged as a +inf point and never wins;
//   * each thread carries kQPT queries, one in every quarter of the slab, and tracks only the running minimum: there
//     is no index to recover;
//   * the valid queries' d go to dist_a / dist_b (NaN at the others); the counts come from ballots; each thread adds
//     sqrt((double) d) and (double) d of its queries in slice order, and the workgroup reduces them as scene.hip's
//     block_tally does: a lane-ordered wave tree, wave partials through LDS, a combine in wave order;
//   * thread 0 leaves the slab's counts, two fp64 sums and the float maximum in the workspace.
// shape_combine_kernel, one thread per box, adds the partials in slab order and writes counts, sums and table; a box
//   with an empty side gets its NaN row there, and its dist rows are overwritten with NaN: by that one thread, element
//   by element, after the search has run for the box.  That is the price of a search that need not know an empty side
//   beforehand (it would take a counting pass over both masks in front of it); it is paid only where dist rows are
//   asked for and a box has an empty side, which the evaluator never does.
// No floating-point atomics and no order that depends on scheduling: two calls return the same bytes.
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQPT = 4;                  // queries per thread
constexpr int kSlab = kThreads * kQPT;   // queries per workgroup
constexpr int kTile = 1024;              // searched points per LDS tile (16 KiB as float4)
constexpr int kChunk = 8;                // the inner loop's unrolled run; tiles are padded to it with +inf points
constexpr int kMaxT = MPSR_SHAPE_MAX_THRESHOLDS;
constexpr int kCombineThreads = 64;
constexpr unsigned kMaxGrid = 1u << 20;  // work items beyond it are reached by the grid's stride

using f32x2 = __attribute__((ext_vector_type(2))) float;

struct Thresholds {
    double sq[kMaxT];  // thresholds[t] * thresholds[t]
    int n;
};

// The workspace, three arrays over the work items w = (box * 2 + direction) * slabs + slab: two fp64 sums each, then
// one float maximum each, then 1 + T int32 counts each (the valid queries, then the queries within each threshold).
constexpr long long kSumBytes = 2 * sizeof(double), kMaxBytes = sizeof(float);

struct Layout {
    long long items;
    size_t bytes;
};

Layout layout_of(int n, int P, int Q, int T)
{
    Layout l;
    const int big = P > Q ? P : Q;
    const long long slabs = big > 0 ? ((long long)big + kSlab - 1) / kSlab : 1;
    l.items = (long long)n * 2 * slabs;
    l.bytes = (size_t)(kSumBytes + kMaxBytes + (long long)sizeof(int) * (1 + T)) * (size_t)l.items;
    return l;
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

__global__ __launch_bounds__(kThreads) void shape_search_kernel(
    const float *__restrict__ a, const float *__restrict__ mask_a, int P, const float *__restrict__ b,
    const float *__restrict__ mask_b, int Q, int slabs, long long items, Thresholds thr,
    char *__restrict__ workspace, float *__restrict__ dist_a, float *__restrict__ dist_b)
{
    __shared__ float4 tile[kTile];
    __shared__ int cpart[1 + kMaxT][kWaves];
    __shared__ double dpart[2][kWaves];
    __shared__ float mpart[kWaves];
    __shared__ double thr_sq[kMaxT];  // (read back in a loop over t: sixteen scalar registers less than the argument)
    const int tid = threadIdx.x;
    const float inf = __builtin_inff();
#pragma unroll
    for (int t = 0; t < kMaxT; ++t)
        if (tid == t) thr_sq[t] = thr.sq[t];
    const int n_thr = thr.n;
    __syncthreads();

    // (items < 2^32; the test in front of the step keeps w from wrapping)
    for (unsigned w = blockIdx.x; w < (unsigned)items; w += gridDim.x) {
        const unsigned pair = w / (unsigned)slabs;
        const int slab = (int)(w - pair * (unsigned)slabs);
        const int dir = (int)(pair & 1u);
        const long long box = pair >> 1;
        const int nq = dir ? Q : P;
        const int nr = dir ? P : Q;
        const float *q = dir ? b : a;
        const float *qmask = dir ? mask_b : mask_a;
        const float *r = dir ? a : b;
        const float *rmask = dir ? mask_a : mask_b;
        float *dist = dir ? dist_b : dist_a;
        const long long q0 = box * nq, r0 = box * nr;  // (box * max(P, Q) < 2^31: the entry point's check)
        const int qbase = slab * kSlab;

        float qx[kQPT], qy[kQPT], qz[kQPT], best[kQPT];
        bool ok[kQPT];
#pragma unroll
        for (int u = 0; u < kQPT; ++u) {
            const int j = qbase + u * kThreads + tid;
            float v[3];
            ok[u] = load_point(q, qmask, q0 + j, j < nq, v);
            qx[u] = v[0];
            qy[u] = v[1];
            qz[u] = v[2];
            best[u] = inf;
        }

        // a slab without a query (the shorter cloud's tail) searches nothing and leaves zeros
        const int n_search = qbase < nq ? nr : 0;
        for (int t0 = 0; t0 < n_search; t0 += kTile) {
            const int cnt = min(kTile, nr - t0);
            const int cntp = (cnt + kChunk - 1) / kChunk * kChunk;
            __syncthreads();
            for (int p = tid; p < cntp; p += kThreads) {
                float v[3];
                const bool valid = load_point(r, rmask, r0 + t0 + p, p < cnt, v);
                tile[p] = valid ? make_float4(v[0], v[1], v[2], 0.f) : make_float4(inf, inf, inf, 0.f);
            }
            __syncthreads();
            // two queries to a 2-wide vector, as in nn_search_kernel: packed fp32 subtract / multiply / add are
            // IEEE-exact and nothing is contracted, so every distance keeps the bits of (dx*dx + dy*dy) + dz*dz
            static_assert(kQPT % 2 == 0, "packed search arithmetic pairs the queries of a thread");
            f32x2 vqx[kQPT / 2], vqy[kQPT / 2], vqz[kQPT / 2], vbest[kQPT / 2];
#pragma unroll
            for (int v = 0; v < kQPT / 2; ++v) {
                vqx[v] = f32x2{qx[2 * v], qx[2 * v + 1]};
                vqy[v] = f32x2{qy[2 * v], qy[2 * v + 1]};
                vqz[v] = f32x2{qz[2 * v], qz[2 * v + 1]};
                vbest[v] = f32x2{best[2 * v], best[2 * v + 1]};
            }
            for (int k0 = 0; k0 < cntp; k0 += kChunk) {
#pragma unroll
                for (int s = 0; s < kChunk; ++s) {
                    const float4 rp = tile[k0 + s];
#pragma unroll
                    for (int v = 0; v < kQPT / 2; ++v) {
                        const f32x2 dx = rp.x - vqx[v], dy = rp.y - vqy[v], dz = rp.z - vqz[v];
                        vbest[v] = __builtin_elementwise_min(vbest[v], (dx * dx + dy * dy) + dz * dz);
                    }
                }
            }
#pragma unroll
            for (int v = 0; v < kQPT / 2; ++v) {
                best[2 * v] = vbest[v][0];
                best[2 * v + 1] = vbest[v][1];
            }
        }

        // the slab's statistics: counts per wave from ballots, sums per thread in slice order
        __syncthreads();  // the previous work item's combine has read the partials
        double d[kQPT], s_root = 0.0, s_sq = 0.0;
        float mx = 0.f;  // (d >= 0: the maximum over no query is never read, an empty side's row is NaN)
        int n_ok = 0;
#pragma unroll
        for (int u = 0; u < kQPT; ++u) {
            const int j = qbase + u * kThreads + tid;
            d[u] = (double)best[u];
            if (ok[u]) {
                s_root += sqrt(d[u]);
                s_sq += d[u];
                mx = fmaxf(mx, best[u]);
            }
            n_ok += __popcll(__ballot(ok[u]));
            if (dist != nullptr && j < nq) dist[q0 + j] = ok[u] ? best[u] : __builtin_nanf("");
        }
        for (int t = 0; t < n_thr; ++t) {
            const double limit = thr_sq[t];
            int within = 0;
#pragma unroll
            for (int u = 0; u < kQPT; ++u) within += __popcll(__ballot(ok[u] && d[u] <= limit));
            if ((tid & 63) == 0) cpart[1 + t][tid >> 6] = within;
        }
        for (int o = 32; o > 0; o >>= 1) {
            s_root += __shfl_down(s_root, o);
            s_sq += __shfl_down(s_sq, o);
            mx = fmaxf(mx, __shfl_down(mx, o));
        }
        if ((tid & 63) == 0) {
            cpart[0][tid >> 6] = n_ok;
            dpart[0][tid >> 6] = s_root;
            dpart[1][tid >> 6] = s_sq;
            mpart[tid >> 6] = mx;
        }
        __syncthreads();
        if (tid == 0) {
            double t_root = 0.0, t_sq = 0.0;
            float t_max = 0.f;
            for (int v = 0; v < kWaves; ++v) {  // in wave order
                t_root += dpart[0][v];
                t_sq += dpart[1][v];
                t_max = fmaxf(t_max, mpart[v]);
            }
            double *part_sums = reinterpret_cast<double *>(workspace);
            float *part_max = reinterpret_cast<float *>(workspace + kSumBytes * items);
            int *part_counts = reinterpret_cast<int *>(workspace + (kSumBytes + kMaxBytes) * items);
            part_sums[2 * (long long)w] = t_root;
            part_sums[2 * (long long)w + 1] = t_sq;
            part_max[w] = t_max;
            int *pc = part_counts + (long long)w * (1 + n_thr);
            for (int k = 0; k < 1 + n_thr; ++k) {
                int total = 0;
                for (int v = 0; v < kWaves; ++v) total += cpart[k][v];
                pc[k] = total;
            }
        }
        if ((unsigned)items - w <= gridDim.x) break;
    }
}

// One thread per box: adds the slabs' partials in slab order and writes the box's rows.
__global__ __launch_bounds__(kCombineThreads) void shape_combine_kernel(
    int n, int P, int Q, int slabs, int T, const char *__restrict__ workspace, int *__restrict__ counts,
    double *__restrict__ sums, float *__restrict__ table, float *__restrict__ dist_a, float *__restrict__ dist_b)
{
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long long items = (long long)n * 2 * slabs;
    const double *part_sums = reinterpret_cast<const double *>(workspace);
    const float *part_max = reinterpret_cast<const float *>(workspace + kSumBytes * items);
    const int *part_counts = reinterpret_cast<const int *>(workspace + (kSumBytes + kMaxBytes) * items);
    const long long box = (long long)blockIdx.x * kCombineThreads + threadIdx.x;
    if (box >= n) return;
    int nv[2] = {0, 0};
    double s[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    float mx[2] = {0.f, 0.f};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const long long w0 = (box * 2 + dir) * slabs;
        for (int k = 0; k < slabs; ++k) {  // in slab order
            nv[dir] += part_counts[(w0 + k) * (1 + T)];
            s[dir][0] += part_sums[2 * (w0 + k)];
            s[dir][1] += part_sums[2 * (w0 + k) + 1];
            mx[dir] = fmaxf(mx[dir], part_max[w0 + k]);
        }
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
            for (int j = 0; j < P; ++j) dist_a[box * P + j] = __builtin_nanf("");
        if (dist_b != nullptr)
            for (int j = 0; j < Q; ++j) dist_b[box * Q + j] = __builtin_nanf("");
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
    row[4] = (float)sqrt((double)fmaxf(mx[0], mx[1]));
    for (int t = 0; t < T; ++t) {
        int within[2] = {0, 0};
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const long long w0 = (box * 2 + dir) * slabs;
            for (int k = 0; k < slabs; ++k) within[dir] += part_counts[(w0 + k) * (1 + T) + 1 + t];
        }
        c[2 + t] = within[0];
        c[2 + T + t] = within[1];
        const double p = (double)within[0] / na, r = (double)within[1] / nb;
        row[5 + 3 * t] = (float)p;
        row[5 + 3 * t + 1] = (float)r;
        row[5 + 3 * t + 2] = (float)(p + r == 0.0 ? 0.0 : 2 * p * r / (p + r));
    }
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
    return layout_of(n, P, Q, T).bytes;
}

extern "C" int mpsr_shape_scores(const float *a, const float *mask_a, int P, const float *b, const float *mask_b,
                                 int Q, int n, const double *thresholds, int T, void *workspace,
                                 size_t workspace_bytes, int *counts, double *sums, float *table, float *dist_a,
                                 float *dist_b, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0 && P >= 0 && Q >= 0, "shape_scores: negative size (n=%d P=%d Q=%d)", n, P, Q);
    MPSR_REQUIRE(T >= 0 && T <= kMaxT, "shape_scores: %d thresholds, outside 0..%d", T, kMaxT);
    MPSR_REQUIRE(T == 0 || thresholds, "shape_scores: thresholds is null");
    Thresholds thr;
    thr.n = T;
    for (int t = 0; t < kMaxT; ++t) thr.sq[t] = 0.0;
    for (int t = 0; t < T; ++t) {
        MPSR_REQUIRE(std::isfinite(thresholds[t]) && thresholds[t] > 0.0,
                     "shape_scores: thresholds[%d] = %g is not a finite distance > 0", t, thresholds[t]);
        MPSR_REQUIRE(t == 0 || thresholds[t] > thresholds[t - 1],
                     "shape_scores: thresholds[%d] = %g is not increasing (after %g)", t, thresholds[t],
                     thresholds[t - 1]);
        thr.sq[t] = thresholds[t] * thresholds[t];
    }
    MPSR_REQUIRE(sizes_fit(n, P, Q), "shape_scores: n max(P, Q) = %d x %d does not fit 31 bits", n, P > Q ? P : Q);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE((P == 0 || a) && (Q == 0 || b), "shape_scores: a cloud pointer is null (P=%d Q=%d)", P, Q);
    MPSR_REQUIRE(counts && sums && table, "shape_scores: an output pointer is null with n = %d", n);
    const Layout l = layout_of(n, P, Q, T);
    MPSR_REQUIRE(workspace, "shape_scores: workspace is null");
    MPSR_REQUIRE((uintptr_t)workspace % sizeof(double) == 0, "shape_scores: workspace is not 8-byte aligned");
    if (workspace_bytes < l.bytes)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "shape_scores: workspace %zu bytes < %zu", workspace_bytes, l.bytes);
    char *ws = static_cast<char *>(workspace);
    const int slabs = (int)(l.items / n / 2);
    hipStream_t s = mpsr::as_stream(stream);
    const unsigned grid = (unsigned)(l.items < (long long)kMaxGrid ? l.items : (long long)kMaxGrid);
    hipLaunchKernelGGL(shape_search_kernel, dim3(grid), dim3(kThreads), 0, s, a, mask_a, P, b, mask_b, Q, slabs,
                       l.items, thr, ws, dist_a, dist_b);
    MPSR_CHECK_LAUNCH("shape_search_kernel");
    hipLaunchKernelGGL(shape_combine_kernel, dim3((unsigned)mpsr::ceil_div(n, kCombineThreads)),
                       dim3(kCombineThreads), 0, s, n, P, Q, slabs, T, ws, counts, sums, table, dist_a, dist_b);
    MPSR_CHECK_LAUNCH("shape_combine_kernel");
    return MPSR_OK;
}

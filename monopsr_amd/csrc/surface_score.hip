// Shape scores against surfaces (mpsr_surface_scores): mpsr_shape_scores' statistics, but the
// distance of a valid point is taken to the other grid's triangulated surface -- its valid points and the kept
// triangles of section 7.9's indexing -- instead of to its nearest valid point alone.
//
// The point term is shape_score.hip's, restated: float differences, float products, (dx*dx + dy*dy) + dz*dz, a float
// minimum.  The edge and face terms are fp64 on the coordinates converted exactly, every dot product (x x + y y) + z z.
// Nothing is contracted (the file is compiled with -ffp-contract=off and repeats that as a pragma) and a minimum does
// not depend on its order, so every d is the header's definition bit for bit.
//
// surface_search_kernel, one workgroup per (box, direction, slab of kSlab queries):
//   * the point minimum first, laid out as shape_search_kernel: the searched grid staged through LDS as float4 tiles,
//     a point that is not valid as a +inf point;
//   * then the triangles, kThreads ids to a pass: thread i decides whether triangle t0 + i is KEPT (three valid
//     vertices, three float32 squared edge lengths within max_edge^2) and, if so, works out its record -- the corners
//     and the quantities that do not depend on the query: e0, eBC, e1, d00, eeBC, d11, d01, den, n, nn.  The kept
//     records are compacted into LDS in id order by ranks from wave ballots (no atomics) and read back at wave-uniform
//     addresses; each thread carries kQPT queries and only their running minima.  The divisions sit under their
//     predicates.  There is no setup kernel and no table of records in memory: a record costs about as much as one
//     (query, triangle) pair, so working it out again in each of the box's slabs is 1 / kSlab of the search, and a
//     table would take 2 (h - 1)(w - 1) 2 n records of 216 bytes, 0.5 GB for 256 boxes of 48 x 48;
//   * the statistics as shape_search_kernel leaves them, the maximum in fp64; the workgroup of a side's slab 0 also
//     leaves the number of kept triangles of the grid it searched.
// surface_combine_kernel, one thread per box, adds the partials in slab order and writes counts, sums, table and
//   tri_counts; a box with an empty side gets its NaN rows there, as in shape_combine_kernel.
// No floating-point atomics and no order that depends on scheduling: two calls return the same bytes.
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQPT = 2;                  // queries per thread
constexpr int kSlab = kThreads * kQPT;   // queries per workgroup
constexpr int kTile = 1024;              // searched points per LDS tile (16 KiB as float4)
constexpr int kChunk = 8;                // the point loop's unrolled run; tiles are padded to it with +inf points
constexpr int kTriTile = kThreads;       // triangle ids per pass, one per thread
constexpr int kRec = 28;                 // doubles per triangle record (27 used; 16-byte aligned records)
constexpr int kMaxT = MPSR_SHAPE_MAX_THRESHOLDS;
constexpr int kCombineThreads = 64;
constexpr unsigned kMaxGrid = 1u << 20;  // work items beyond it are reached by the grid's stride

// the record's slots
enum { kA = 0, kB = 3, kC = 6, kE0 = 9, kEBC = 12, kE1 = 15, kD00 = 18, kEEBC = 19, kD11 = 20, kD01 = 21, kDen = 22,
       kN = 23, kNN = 26 };

static_assert(kTile * sizeof(float4) <= kTriTile * kRec * sizeof(double), "the point tile shares the records' LDS");

struct Thresholds {
    double sq[kMaxT];  // thresholds[t] * thresholds[t]
    int n;
};

// The workspace, two arrays over the work items w = (box * 2 + direction) * slabs + slab: three doubles each (the sum
// of the roots, the sum of d, the maximum of d), then 2 + T int32 each (the valid queries, the queries within each
// threshold, the kept triangles of the searched grid: slab 0 only).
constexpr long long kDoubleBytes = 3 * sizeof(double);

struct Layout {
    long long items;
    int slabs;
    size_t bytes;
};

Layout layout_of(int n, int P, int T)
{
    Layout l;
    l.slabs = (P + kSlab - 1) / kSlab;
    l.items = (long long)n * 2 * l.slabs;
    const size_t raw = (size_t)(kDoubleBytes + (long long)sizeof(int) * (2 + T)) * (size_t)l.items;
    l.bytes = (raw + 7) / 8 * 8;
    return l;
}

// Point i of grid p where `live`, else nothing: -> is it valid, its coordinates in v.
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
    __shared__ int cpart[1 + kMaxT][kWaves];
    __shared__ double dpart[3][kWaves];
    __shared__ double thr_sq[kMaxT];
    float4 *tile = reinterpret_cast<float4 *>(rec);
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const float inf = __builtin_inff();
#pragma unroll
    for (int t = 0; t < kMaxT; ++t)
        if (tid == t) thr_sq[t] = thr.sq[t];
    const int n_thr = thr.n;
    const int P = map_h * map_w;
    const int cells_w = map_w - 1;
    const int n_tri = 2 * (map_h - 1) * cells_w;
    __syncthreads();

    // (items < 2^32; the test in front of the step keeps w from wrapping)
    for (unsigned w = blockIdx.x; w < (unsigned)items; w += gridDim.x) {
        const unsigned pair = w / (unsigned)slabs;
        const int slab = (int)(w - pair * (unsigned)slabs);
        const int dir = (int)(pair & 1u);
        const long long box = pair >> 1;
        const float *q = dir ? b : a;
        const float *qmask = dir ? mask_b : mask_a;
        const float *r = dir ? a : b;
        const float *rmask = dir ? mask_a : mask_b;
        double *dist = dir ? dist_b : dist_a;
        const long long p0 = box * P;  // (box * P < 2^31: the entry point's check)
        const int qbase = slab * kSlab;

        float qf[kQPT][3], best[kQPT];
        bool ok[kQPT];
#pragma unroll
        for (int u = 0; u < kQPT; ++u) {
            const int j = qbase + u * kThreads + tid;
            ok[u] = load_point(q, qmask, p0 + j, j < P, qf[u]);
            if (!ok[u]) qf[u][0] = qf[u][1] = qf[u][2] = 0.f;
            best[u] = inf;
        }

        // the point minimum: mpsr_shape_scores' d
        for (int t0 = 0; t0 < P; t0 += kTile) {
            const int cnt = min(kTile, P - t0);
            const int cntp = (cnt + kChunk - 1) / kChunk * kChunk;
            __syncthreads();
            for (int p = tid; p < cntp; p += kThreads) {
                float v[3];
                const bool valid = load_point(r, rmask, p0 + t0 + p, p < cnt, v);
                tile[p] = valid ? make_float4(v[0], v[1], v[2], 0.f) : make_float4(inf, inf, inf, 0.f);
            }
            __syncthreads();
            for (int k0 = 0; k0 < cntp; k0 += kChunk) {
#pragma unroll
                for (int s = 0; s < kChunk; ++s) {
                    const float4 rp = tile[k0 + s];
#pragma unroll
                    for (int u = 0; u < kQPT; ++u) {
                        const float dx = rp.x - qf[u][0], dy = rp.y - qf[u][1], dz = rp.z - qf[u][2];
                        best[u] = fminf(best[u], (dx * dx + dy * dy) + dz * dz);
                    }
                }
            }
        }

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

        // the slab's statistics: counts per wave from ballots, sums per thread in slice order
        __syncthreads();  // the previous work item's combine has read the partials
        double s_root = 0.0, s_sq = 0.0, mx = 0.0;  // (d >= 0: the maximum over no query is never read)
        int n_ok = 0;
#pragma unroll
        for (int u = 0; u < kQPT; ++u) {
            const int j = qbase + u * kThreads + tid;
            if (ok[u]) {
                s_root += sqrt(d[u]);
                s_sq += d[u];
                mx = fmax(mx, d[u]);
            }
            n_ok += __popcll(__ballot(ok[u]));
            if (dist != nullptr && j < P) dist[p0 + j] = ok[u] ? d[u] : __longlong_as_double(0x7ff8000000000000LL);
        }
        for (int t = 0; t < n_thr; ++t) {
            const double limit = thr_sq[t];
            int within = 0;
#pragma unroll
            for (int u = 0; u < kQPT; ++u) within += __popcll(__ballot(ok[u] && d[u] <= limit));
            if (lane == 0) cpart[1 + t][wave] = within;
        }
        for (int o = 32; o > 0; o >>= 1) {
            s_root += __shfl_down(s_root, o);
            s_sq += __shfl_down(s_sq, o);
            mx = fmax(mx, __shfl_down(mx, o));
        }
        if (lane == 0) {
            cpart[0][wave] = n_ok;
            dpart[0][wave] = s_root;
            dpart[1][wave] = s_sq;
            dpart[2][wave] = mx;
        }
        __syncthreads();
        if (tid == 0) {
            double t_root = 0.0, t_sq = 0.0, t_max = 0.0;
            for (int v = 0; v < kWaves; ++v) {  // in wave order
                t_root += dpart[0][v];
                t_sq += dpart[1][v];
                t_max = fmax(t_max, dpart[2][v]);
            }
            double *part_d = reinterpret_cast<double *>(workspace) + 3 * (long long)w;
            int *pc = reinterpret_cast<int *>(workspace + kDoubleBytes * items) + (long long)w * (2 + n_thr);
            part_d[0] = t_root;
            part_d[1] = t_sq;
            part_d[2] = t_max;
            for (int k = 0; k < 1 + n_thr; ++k) {
                int total = 0;
                for (int v = 0; v < kWaves; ++v) total += cpart[k][v];
                pc[k] = total;
            }
            pc[1 + n_thr] = kept_total;
        }
        if ((unsigned)items - w <= gridDim.x) break;
    }
}

// One thread per box: adds the slabs' partials in slab order and writes the box's rows.
__global__ __launch_bounds__(kCombineThreads) void surface_combine_kernel(
    int n, int P, int slabs, int T, const char *__restrict__ workspace, int *__restrict__ counts,
    double *__restrict__ sums, float *__restrict__ table, double *__restrict__ dist_a, double *__restrict__ dist_b,
    int *__restrict__ tri_counts)
{
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const long long items = (long long)n * 2 * slabs;
    const double *part_d = reinterpret_cast<const double *>(workspace);
    const int *part_counts = reinterpret_cast<const int *>(workspace + kDoubleBytes * items);
    const long long box = (long long)blockIdx.x * kCombineThreads + threadIdx.x;
    if (box >= n) return;
    int nv[2] = {0, 0};
    double s[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    double mx[2] = {0.0, 0.0};
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
        const long long w0 = (box * 2 + dir) * slabs;
        for (int k = 0; k < slabs; ++k) {  // in slab order
            nv[dir] += part_counts[(w0 + k) * (2 + T)];
            s[dir][0] += part_d[3 * (w0 + k)];
            s[dir][1] += part_d[3 * (w0 + k) + 1];
            mx[dir] = fmax(mx[dir], part_d[3 * (w0 + k) + 2]);
        }
    }
    // direction 0 searched b, direction 1 searched a
    tri_counts[2 * box] = part_counts[((box * 2 + 1) * slabs) * (2 + T) + 1 + T];
    tri_counts[2 * box + 1] = part_counts[((box * 2) * slabs) * (2 + T) + 1 + T];
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
            for (int j = 0; j < P; ++j) dist_a[box * P + j] = nan;
        if (dist_b != nullptr)
            for (int j = 0; j < P; ++j) dist_b[box * P + j] = nan;
        return;
    }
    const double na = (double)nv[0], nb = (double)nv[1];
    so[0] = s[0][0];
    so[1] = s[0][1];
    so[2] = s[1][0];
    so[3] = s[1][1];
    so[4] = mx[0];
    so[5] = mx[1];
    const double accuracy = s[0][0] / na, completeness = s[1][0] / nb;
    row[0] = (float)accuracy;
    row[1] = (float)completeness;
    row[2] = (float)((accuracy + completeness) / 2);
    row[3] = (float)(s[0][1] / na + s[1][1] / nb);
    row[4] = (float)sqrt(fmax(mx[0], mx[1]));
    for (int t = 0; t < T; ++t) {
        int within[2] = {0, 0};
#pragma unroll
        for (int dir = 0; dir < 2; ++dir) {
            const long long w0 = (box * 2 + dir) * slabs;
            for (int k = 0; k < slabs; ++k) within[dir] += part_counts[(w0 + k) * (2 + T) + 1 + t];
        }
        c[2 + t] = within[0];
        c[2 + T + t] = within[1];
        const double p = (double)within[0] / na, r = (double)within[1] / nb;
        row[5 + 3 * t] = (float)p;
        row[5 + 3 * t + 1] = (float)r;
        row[5 + 3 * t + 2] = (float)(p + r == 0.0 ? 0.0 : 2 * p * r / (p + r));
    }
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
    return layout_of(n, h * w, T).bytes;
}

extern "C" int mpsr_surface_scores(const float *a, const float *mask_a, const float *b, const float *mask_b, int n,
                                   int h, int w, const double *thresholds, int T, double max_edge, void *workspace,
                                   size_t workspace_bytes, int *counts, double *sums, float *table, double *dist_a,
                                   double *dist_b, int *tri_counts, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0, "surface_scores: negative size (n=%d)", n);
    MPSR_REQUIRE(h >= 1 && w >= 1, "surface_scores: a grid of %d x %d has no point", h, w);
    MPSR_REQUIRE(T >= 0 && T <= kMaxT, "surface_scores: %d thresholds, outside 0..%d", T, kMaxT);
    MPSR_REQUIRE(T == 0 || thresholds, "surface_scores: thresholds is null");
    Thresholds thr;
    thr.n = T;
    for (int t = 0; t < kMaxT; ++t) thr.sq[t] = 0.0;
    for (int t = 0; t < T; ++t) {
        MPSR_REQUIRE(std::isfinite(thresholds[t]) && thresholds[t] > 0.0,
                     "surface_scores: thresholds[%d] = %g is not a finite distance > 0", t, thresholds[t]);
        MPSR_REQUIRE(t == 0 || thresholds[t] > thresholds[t - 1],
                     "surface_scores: thresholds[%d] = %g is not increasing (after %g)", t, thresholds[t],
                     thresholds[t - 1]);
        thr.sq[t] = thresholds[t] * thresholds[t];
    }
    // (NaN fails the comparison)
    MPSR_REQUIRE(max_edge >= 0.0, "surface_scores: max_edge = %g is not a length >= 0", max_edge);
    MPSR_REQUIRE(sizes_fit(n, h, w), "surface_scores: n h w = %d x %d x %d does not fit 31 bits", n, h, w);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(a && b, "surface_scores: a grid pointer is null");
    MPSR_REQUIRE(counts && sums && table && tri_counts, "surface_scores: an output pointer is null with n = %d", n);
    const int P = h * w;
    const Layout l = layout_of(n, P, T);
    MPSR_REQUIRE(workspace, "surface_scores: workspace is null");
    MPSR_REQUIRE((uintptr_t)workspace % sizeof(double) == 0, "surface_scores: workspace is not 8-byte aligned");
    if (workspace_bytes < l.bytes)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "surface_scores: workspace %zu bytes < %zu", workspace_bytes, l.bytes);
    char *ws = static_cast<char *>(workspace);
    hipStream_t s = mpsr::as_stream(stream);
    const unsigned grid = (unsigned)(l.items < (long long)kMaxGrid ? l.items : (long long)kMaxGrid);
    hipLaunchKernelGGL(surface_search_kernel, dim3(grid), dim3(kThreads), 0, s, a, mask_a, b, mask_b, h, w, l.slabs,
                       l.items, max_edge * max_edge, thr, ws, dist_a, dist_b);
    MPSR_CHECK_LAUNCH("surface_search_kernel");
    hipLaunchKernelGGL(surface_combine_kernel, dim3((unsigned)mpsr::ceil_div(n, kCombineThreads)),
                       dim3(kCombineThreads), 0, s, n, P, l.slabs, T, ws, counts, sums, table, dist_a, dist_b,
                       tri_counts);
    MPSR_CHECK_LAUNCH("surface_combine_kernel");
    return MPSR_OK;
}

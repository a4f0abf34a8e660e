// Projection error of a placed instance cloud against its 2-D box, and its minimiser.
//   A box's predicted local cloud is put at distance xz_dist along its viewing ray and at height centroid_y, projected,
//   and compared with the regular grid of the 2-D box: err = mean over valid points of |u - eu| + |v - ev|.
//   mpsr_proj_points evaluates that once per box; mpsr_proj_fit runs Nelder-Mead on it, one workgroup per box, with the
//   cloud and the expected grid held in registers and one block reduction per evaluation.
// Reference: core/instances/instance_metrics.py:13-107 (np_proj_error, scipy_proj_error*),
// datasets/kitti/instance_utils.py:684-735 (get_exp_proj_uv_map), 791-838 (proj_points).
// Products are fp32 and every one is rounded (the Makefile builds this unit without contraction); the per-box sum is
// fp64, taken in a fixed order: each thread adds its points in index order, the lanes of a wave are folded 32, 16, ..., 1
// and the waves are added in wave order.  No atomics: two runs give the same bits, and the fit's err is the bits that
// mpsr_proj_points returns at the fitted x.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSlots = 9;  // points a thread of the fit holds in registers: 48 x 48 = 9 * 256
constexpr int kFitMaxPoints = kSlots * kThreads;

using mpsr::cam_of;

struct Flags {
    int rotate_view, cam0_shift, round_box_2d, use_pixel_centres;
};

// get_exp_proj_uv_map's np.linspace(start, stop, n) as start + i * step, in both of its forms
struct Grid {
    float u0, du, v0, dv;
};

__device__ __forceinline__ Grid exp_grid(const float *box, int H, int W, const Flags &f)
{
    float v1 = box[0], u1 = box[1], v2 = box[2], u2 = box[3];
    if (f.round_box_2d) {  // np.round: half to even
        v1 = rintf(v1);
        u1 = rintf(u1);
        v2 = rintf(v2);
        u2 = rintf(u2);
    }
    const float su = (u2 - u1) / (float)W, sv = (v2 - v1) / (float)H;
    float ue, ve;
    Grid g;
    if (f.use_pixel_centres) {
        const float hu = su / 2.0f, hv = sv / 2.0f;
        g.u0 = u1 + hu;
        ue = u2 - hu;
        g.v0 = v1 + hv;
        ve = v2 - hv;
    } else {
        g.u0 = u1;
        ue = u2 - su;
        g.v0 = v1;
        ve = v2 - sv;
    }
    g.du = W > 1 ? (ue - g.u0) / (float)(W - 1) : 0.f;
    g.dv = H > 1 ? (ve - g.v0) / (float)(H - 1) : 0.f;
    return g;
}

// R_y(va) of local_to_global_kernel (geometry.hip)
__device__ __forceinline__ void rotate_y(float c, float s, float x, float y, float z, float &rx, float &ry, float &rz)
{
    rx = c * x + s * z;
    ry = y;
    rz = -s * x + c * z;
}

__device__ __forceinline__ bool point_valid(float rx, float ry, float rz)
{
    return (fabsf(rx) + fabsf(ry)) + fabsf(rz) > 0.1f;  // false for NaN
}

// A rotated point, translated, shifted to cam0 and projected.  wc is the projective depth.
__device__ __forceinline__ void project(float rx, float ry, float rz, float tx, float ty, float tz, float xoff,
                                        const float *pm, float &u, float &v, float &wc)
{
    const float gx = (rx + tx) + xoff, gy = ry + ty, gz = rz + tz;
    const float U = pm[0] * gx + pm[1] * gy + pm[2] * gz + pm[3];
    const float V = pm[4] * gx + pm[5] * gy + pm[6] * gz + pm[7];
    wc = pm[8] * gx + pm[9] * gy + pm[10] * gz + pm[11];
    u = U / wc;
    v = V / wc;
}

// |u - eu| + |v - ev| of a valid point; +inf when it is not in front of the camera
__device__ __forceinline__ float point_term(float u, float v, float wc, float eu, float ev)
{
    const float t = fabsf(u - eu) + fabsf(v - ev);
    return wc > 0.f ? t : __builtin_inff();
}

// The workgroup's sum and count in a fixed order, returned to every thread.  The LDS words are read by all threads
// after the second barrier and rewritten only after the next call's first one.
__device__ __forceinline__ double block_mean(double s, int n, double *red, int *redn)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        n += __shfl_down(n, o, 64);
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        red[tid >> 6] = s;
        redn[tid >> 6] = n;
    }
    __syncthreads();
    double rs = 0.0;
    int rn = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        rs += red[i];
        rn += redn[i];
    }
    return rn > 0 ? rs / (double)rn : __builtin_nan("");
}

// ------------------------------------------------------------------------------------------ the objective, once

__global__ __launch_bounds__(kThreads) void proj_points_kernel(const float *__restrict__ local,
                                                               const float *__restrict__ x,
                                                               const float *__restrict__ boxes,
                                                               const float *__restrict__ cam_p,
                                                               const int *__restrict__ cam_index, int n_cams,
                                                               const float *__restrict__ mask, float *__restrict__ uv,
                                                               unsigned char *__restrict__ valid,
                                                               double *__restrict__ err, int H, int W, Flags f)
{
    __shared__ double red[kWaves];
    __shared__ int redn[kWaves];
    const int b = blockIdx.x, P = H * W;
    const float *cam = cam_of(cam_p, cam_index, n_cams, b);
    if (!cam) {  // uniform over the workgroup
        const float nan = __builtin_nanf("");
        for (int i = threadIdx.x; i < P; i += kThreads) {
            if (uv) uv[(size_t)b * 2 * P + i] = uv[(size_t)b * 2 * P + P + i] = nan;
            if (valid) valid[(size_t)b * P + i] = 0;
        }
        if (threadIdx.x == 0) err[b] = __builtin_nan("");
        return;
    }
    float pm[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pm[i] = cam[i];
    const Grid g = exp_grid(boxes + b * 4, H, W, f);
    const float d = x[b * 3 + 0], cy = x[b * 3 + 1], va = x[b * 3 + 2];
    const float c = cosf(va), s = sinf(va);
    const float tx = d * s, tz = d * c;
    const float xoff = f.cam0_shift ? -pm[3] / pm[0] : 0.f;
    double sum = 0.0;
    int n = 0;
    for (int i = threadIdx.x; i < P; i += kThreads) {
        const float *p = local + ((size_t)b * P + i) * 3;
        float rx = p[0], ry = p[1], rz = p[2];
        if (f.rotate_view) rotate_y(c, s, p[0], p[1], p[2], rx, ry, rz);
        const bool ok = point_valid(rx, ry, rz) && (!mask || mask[(size_t)b * P + i] != 0.f);
        float u, v, wc;
        project(rx, ry, rz, tx, cy, tz, xoff, pm, u, v, wc);
        if (ok) {
            const int r = i / W, col = i - r * W;
            sum += (double)point_term(u, v, wc, g.u0 + g.du * (float)col, g.v0 + g.dv * (float)r);
            ++n;
        }
        if (uv) {
            uv[(size_t)b * 2 * P + i] = ok ? u : 0.f;
            uv[(size_t)b * 2 * P + P + i] = ok ? v : 0.f;
        }
        if (valid) valid[(size_t)b * P + i] = ok ? 1 : 0;
    }
    const double e = block_mean(sum, n, red, redn);
    if (threadIdx.x == 0) err[b] = e;
}

// ------------------------------------------------------------------------------------------------ the minimiser

struct FitParams {
    const float *local, *x0, *boxes, *cam_p, *mask;
    const int *cam_index;
    float *x;
    double *err, *err0;
    int *iters, *evals, *status;
    int n_cams, H, W, max_iter;
    double xatol, fatol;
    Flags f;
};

// A thread's points.  With N == 2 the viewing angle is fixed: the points are kept rotated and their validity is a bit
// each.  With N == 3 they are kept raw, and `ok` holds the mask alone: validity follows the rotation.
struct Slots {
    float px[kSlots], py[kSlots], pz[kSlots], eu[kSlots], ev[kSlots];
    unsigned ok;
};

template <int N>
__device__ __forceinline__ double objective(const Slots &sl, const float *pm, float xoff, int rotate_view, float d,
                                            float cy, float c, float s, double *red, int *redn)
{
    const float tx = d * s, tz = d * c;
    double sum = 0.0;
    int n = 0;
#pragma unroll
    for (int k = 0; k < kSlots; ++k) {
        float rx = sl.px[k], ry = sl.py[k], rz = sl.pz[k];
        bool ok = (sl.ok >> k) & 1u;
        if (N == 3) {
            if (rotate_view) rotate_y(c, s, sl.px[k], sl.py[k], sl.pz[k], rx, ry, rz);
            ok = ok && point_valid(rx, ry, rz);
        }
        float u, v, wc;
        project(rx, ry, rz, tx, cy, tz, xoff, pm, u, v, wc);
        if (ok) {
            sum += (double)point_term(u, v, wc, sl.eu[k], sl.ev[k]);
            ++n;
        }
    }
    return block_mean(sum, n, red, redn);
}

// SciPy's Nelder-Mead (reflection 1, expansion 2, contractions 0.5, shrink 0.5), every thread carrying the same simplex
// in fp64.  An evaluation past the cap ends the iteration where it stands, as SciPy's wrapped objective does.
template <int N>
__global__ __launch_bounds__(kThreads) void proj_fit_kernel(const FitParams p)
{
    __shared__ double red[kWaves];
    __shared__ int redn[kWaves];
    const int b = blockIdx.x, P = p.H * p.W, tid = threadIdx.x;
    const float d0 = p.x0[b * 3 + 0], cy0 = p.x0[b * 3 + 1], va0 = p.x0[b * 3 + 2];
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const float *cam = cam_of(p.cam_p, p.cam_index, p.n_cams, b);
    int evals = 0;
    double e0 = nan;
    float pm[12];
    Slots sl;
    float c0 = 0.f, s0 = 0.f, xoff = 0.f;
    if (cam) {  // uniform over the workgroup
#pragma unroll
        for (int i = 0; i < 12; ++i) pm[i] = cam[i];
        xoff = p.f.cam0_shift ? -pm[3] / pm[0] : 0.f;
        const Grid g = exp_grid(p.boxes + b * 4, p.H, p.W, p.f);
        c0 = cosf(va0);
        s0 = sinf(va0);
        sl.ok = 0u;
#pragma unroll
        for (int k = 0; k < kSlots; ++k) {
            const int i = tid + k * kThreads;
            float x = 0.f, y = 0.f, z = 0.f;
            bool ok = false;
            int r = 0, col = 0;
            if (i < P) {
                const float *q = p.local + ((size_t)b * P + i) * 3;
                x = q[0];
                y = q[1];
                z = q[2];
                ok = !p.mask || p.mask[(size_t)b * P + i] != 0.f;
                r = i / p.W;
                col = i - r * p.W;
            }
            if (N == 2) {
                float rx = x, ry = y, rz = z;
                if (p.f.rotate_view) rotate_y(c0, s0, x, y, z, rx, ry, rz);
                ok = ok && point_valid(rx, ry, rz);
                x = rx;
                y = ry;
                z = rz;
            }
            sl.px[k] = x;
            sl.py[k] = y;
            sl.pz[k] = z;
            sl.eu[k] = g.u0 + g.du * (float)col;
            sl.ev[k] = g.v0 + g.dv * (float)r;
            if (ok) sl.ok |= 1u << k;
        }
        e0 = objective<N>(sl, pm, xoff, p.f.rotate_view, d0, cy0, c0, s0, red, redn);
        evals = 1;
    }
    if (e0 != e0) {  // bad camera, or no valid point at x0
        if (tid == 0) {
            p.x[b * 3 + 0] = d0;
            p.x[b * 3 + 1] = cy0;
            p.x[b * 3 + 2] = va0;
            p.err[b] = nan;
            p.err0[b] = nan;
            p.iters[b] = 0;
            p.evals[b] = evals;
            p.status[b] = 2;
        }
        return;
    }

    // an evaluation with no valid point (N == 3 only) ranks last
    auto eval = [&](const double *v) -> double {
        const float d = (float)v[0], cy = (float)v[1];
        float c = c0, s = s0;
        if (N == 3) {
            const float va = (float)v[2];
            c = cosf(va);
            s = sinf(va);
        }
        const double e = objective<N>(sl, pm, xoff, p.f.rotate_view, d, cy, c, s, red, redn);
        ++evals;
        return e != e ? inf : e;
    };

    double sim[N + 1][N], fs[N + 1];
    const double x0[3] = {(double)d0, (double)cy0, (double)va0};
#pragma unroll
    for (int j = 0; j <= N; ++j) {
#pragma unroll
        for (int k = 0; k < N; ++k) sim[j][k] = x0[k];
        if (j > 0) sim[j][j - 1] = x0[j - 1] != 0.0 ? (1 + 0.05) * x0[j - 1] : 0.00025;
        fs[j] = inf;
    }
    const int max_it = p.max_iter;
    fs[0] = e0;
#pragma unroll
    for (int j = 1; j <= N; ++j)
        if (evals < max_it) fs[j] = eval(sim[j]);

    auto sort = [&]() {  // stable: adjacent swaps on a strict >
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = 0; j < N - i; ++j)
                if (fs[j] > fs[j + 1]) {
                    const double t = fs[j];
                    fs[j] = fs[j + 1];
                    fs[j + 1] = t;
#pragma unroll
                    for (int k = 0; k < N; ++k) {
                        const double u = sim[j][k];
                        sim[j][k] = sim[j + 1][k];
                        sim[j + 1][k] = u;
                    }
                }
    };
    sort();

    int iterations = 1;
    while (evals < max_it && iterations < max_it) {
        double dx = 0.0, df = 0.0;
#pragma unroll
        for (int j = 1; j <= N; ++j) {
#pragma unroll
            for (int k = 0; k < N; ++k) dx = fmax(dx, fabs(sim[j][k] - sim[0][k]));
            const double t = fabs(fs[0] - fs[j]);
            df = (t != t || df != df) ? nan : fmax(df, t);  // np.max keeps a NaN (inf - inf): not converged
        }
        if (dx <= p.xatol && df <= p.fatol) break;

        double xbar[N], xt[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double a = sim[0][k];
#pragma unroll
            for (int j = 1; j < N; ++j) a += sim[j][k];
            xbar[k] = a / (double)N;
        }
        bool capped = false;  // set where SciPy's objective would raise: the iteration ends as it stands
#pragma unroll
        for (int k = 0; k < N; ++k) xt[k] = 2.0 * xbar[k] - 1.0 * sim[N][k];
        double xr[N];
#pragma unroll
        for (int k = 0; k < N; ++k) xr[k] = xt[k];
        const double fxr = eval(xr);  // (evals < max_it holds here)
        bool shrink = false;
        if (fxr < fs[0]) {
            if (evals < max_it) {
#pragma unroll
                for (int k = 0; k < N; ++k) xt[k] = 3.0 * xbar[k] - 2.0 * sim[N][k];
                const double fxe = eval(xt);
                if (fxe < fxr) {
#pragma unroll
                    for (int k = 0; k < N; ++k) sim[N][k] = xt[k];
                    fs[N] = fxe;
                } else {
#pragma unroll
                    for (int k = 0; k < N; ++k) sim[N][k] = xr[k];
                    fs[N] = fxr;
                }
            } else {
                capped = true;
            }
        } else if (fxr < fs[N - 1]) {
#pragma unroll
            for (int k = 0; k < N; ++k) sim[N][k] = xr[k];
            fs[N] = fxr;
        } else if (evals >= max_it) {
            capped = true;
        } else if (fxr < fs[N]) {
#pragma unroll
            for (int k = 0; k < N; ++k) xt[k] = 1.5 * xbar[k] - 0.5 * sim[N][k];
            const double fxc = eval(xt);
            if (fxc <= fxr) {
#pragma unroll
                for (int k = 0; k < N; ++k) sim[N][k] = xt[k];
                fs[N] = fxc;
            } else {
                shrink = true;
            }
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) xt[k] = 0.5 * xbar[k] + 0.5 * sim[N][k];
            const double fxcc = eval(xt);
            if (fxcc < fs[N]) {
#pragma unroll
                for (int k = 0; k < N; ++k) sim[N][k] = xt[k];
                fs[N] = fxcc;
            } else {
                shrink = true;
            }
        }
        if (shrink) {
#pragma unroll
            for (int j = 1; j <= N; ++j) {
                if (capped) continue;
#pragma unroll
                for (int k = 0; k < N; ++k) sim[j][k] = sim[0][k] + 0.5 * (sim[j][k] - sim[0][k]);
                if (evals < max_it)
                    fs[j] = eval(sim[j]);
                else
                    capped = true;  // (the vertex has moved and keeps its old value, as in SciPy)
            }
        }
        if (!capped) ++iterations;
        sort();
    }

    if (tid == 0) {
        p.x[b * 3 + 0] = (float)sim[0][0];
        p.x[b * 3 + 1] = (float)sim[0][1];
        p.x[b * 3 + 2] = N == 3 ? (float)sim[0][2] : va0;
        p.err[b] = fs[0];
        p.err0[b] = e0;
        p.iters[b] = iterations;
        p.evals[b] = evals;
        p.status[b] = (evals >= max_it || iterations >= max_it) ? 1 : 0;
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------- C ABI

extern "C" {

int mpsr_proj_points(const float *local, const float *x, const float *boxes_2d, const float *cam_p, int n_cams,
                     const int *cam_index, const float *mask, float *uv, unsigned char *valid, double *err, int b,
                     int h, int w, int rotate_view, int cam0_shift, int round_box_2d, int use_pixel_centres,
                     mpsr_stream_t stream)
{
    MPSR_REQUIRE(b >= 0 && h > 0 && w > 0 && n_cams >= 1 && (long long)h * w < (1LL << 24),
                 "proj_points: bad size b=%d h=%d w=%d n_cams=%d", b, h, w, n_cams);
    if (b == 0) return MPSR_OK;
    MPSR_REQUIRE(local && x && boxes_2d && cam_p && err, "proj_points: null pointer");
    const Flags f{rotate_view, cam0_shift, round_box_2d, use_pixel_centres};
    hipLaunchKernelGGL(proj_points_kernel, dim3(b), dim3(kThreads), 0, mpsr::as_stream(stream), local, x, boxes_2d,
                       cam_p, cam_index, n_cams, mask, uv, valid, err, h, w, f);
    MPSR_CHECK_LAUNCH("proj_points");
    return MPSR_OK;
}

int mpsr_proj_fit(const float *local, const float *x0, const float *boxes_2d, const float *cam_p, int n_cams,
                  const int *cam_index, const float *mask, int b, int h, int w, int n_fit, int rotate_view,
                  int cam0_shift, int round_box_2d, int use_pixel_centres, double xatol, double fatol, int max_iter,
                  float *x, double *err, double *err0, int *iters, int *evals, int *status, mpsr_stream_t stream)
{
    MPSR_REQUIRE(b >= 0 && h > 0 && w > 0 && n_cams >= 1, "proj_fit: bad size b=%d h=%d w=%d n_cams=%d", b, h, w,
                 n_cams);
    MPSR_REQUIRE((long long)h * w <= kFitMaxPoints, "proj_fit: %d x %d points, at most %d fit a workgroup's registers",
                 h, w, kFitMaxPoints);
    MPSR_REQUIRE(n_fit == 2 || n_fit == 3, "proj_fit: n_fit = %d (2 or 3)", n_fit);
    MPSR_REQUIRE(xatol >= 0.0 && fatol >= 0.0, "proj_fit: negative tolerance");  // (false for NaN)
    if (b == 0) return MPSR_OK;
    MPSR_REQUIRE(local && x0 && boxes_2d && cam_p && x && err && err0 && iters && evals && status,
                 "proj_fit: null pointer");
    FitParams p;
    p.local = local;
    p.x0 = x0;
    p.boxes = boxes_2d;
    p.cam_p = cam_p;
    p.mask = mask;
    p.cam_index = cam_index;
    p.x = x;
    p.err = err;
    p.err0 = err0;
    p.iters = iters;
    p.evals = evals;
    p.status = status;
    p.n_cams = n_cams;
    p.H = h;
    p.W = w;
    p.max_iter = max_iter > 0 ? max_iter : 200 * n_fit;
    p.xatol = xatol;
    p.fatol = fatol;
    p.f = Flags{rotate_view, cam0_shift, round_box_2d, use_pixel_centres};
    if (n_fit == 2)
        hipLaunchKernelGGL(proj_fit_kernel<2>, dim3(b), dim3(kThreads), 0, mpsr::as_stream(stream), p);
    else
        hipLaunchKernelGGL(proj_fit_kernel<3>, dim3(b), dim3(kThreads), 0, mpsr::as_stream(stream), p);
    MPSR_CHECK_LAUNCH("proj_fit");
    return MPSR_OK;
}

}  // extern "C"

// Scene reconstruction on the device: the predicted instance clouds of a chunk of frames (B boxes of P points each, in
// the camera frame: what instance_utils.tf_inst_xyz_map_local_to_global returns) projected into their images, rendered
// as a depth map and an instance image per frame, and compacted into one coloured cloud.
//
// mpsr_scene_project: one thread per point computes, in fp64 without contraction (rows3 and rint as in depth_fill.hip),
//   pixel = rint(u0 / u2), rint(u1 / u2) of cam_p . [x y z 1], stores the pixel index of a kept point (-1 of a dropped
//   one) and lowers the pixel's 64-bit key ((uint64) float_bits(z) << 32 | point index) with an unsigned atomicMin: the
//   one atomic of the point rendering.  A kept point has z > 0, so its float bits order as its value: the NEARER point
//   wins, and on equal float32 depth the LOWER point index, in whatever order the waves run.  A true z-buffer.  The LiDAR
//   projection of depth_fill.hip is not: it keeps the LAST duplicate of a pixel, near or far, because that is what the
//   reference's fancy assignment does with a LiDAR cloud.
//   alive() is the one rule for which point takes part; the surfaces' vertex pass calls it too.
// mpsr_scene_resolve: one thread per pixel turns the key into depth (the key's upper half, the winner's z bit for bit;
//   0 where no point fell) and instance (the winner box's ordinal within its frame; 255 where no point fell).
//   resolve_kernel serves the surfaces' z-buffer as well: there the key's lower half is a triangle id.
// mpsr_scene_compact: per-box counts of kept and of visible points (a visible point is its pixel's winner), a one-block
//   exclusive scan over the boxes, and a write pass of one workgroup per box that places a point at its box's offset
//   plus its rank within the box: __ballot / __popcll prefix counts within a wave, wave offsets through LDS, a running
//   base from one 256-point slice of the box to the next.  No atomics: the write position does not depend on scheduling.
// mpsr_scene_score: the reconstruction against ground truth, after project, independent of
//   resolve and compact.  hist_kernel counts the values of every ground-truth instance image into a (n_frames, 256)
//   int32 table: a 256-bin histogram per workgroup in LDS, flushed with integer atomics, whose result does not depend
//   on order.  The frame pointers are NOT aligned (frame k of a stack of 5 x 7 images starts at byte 35 k): the pass
//   PEELS to alignment -- the bytes in front of the first 16-byte boundary and behind the last one are read one by
//   one, the body in 16-byte loads.  score_kernel, one workgroup per box, walks the box's points in slices of 256 as
//   count_kernel does: the six counts from ballots and popcounts, the three fp64 sums per thread in slice order
//   (add_depth_error), then block_tally, the end of every per-box pass here: a lane-ordered wave reduction, wave
//   partials through LDS and a combine in wave order.  No floating-point atomics: two calls return the same bytes.
// The host side of both z-buffers is shared too: ZLayout (the front of either workspace), check_render_args,
//   start_zbuffer, resolve and launch_hist.
#include "common.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned long long kEmptyKey = ~0ULL;  // the memset's 0xff bytes; no kept point has it (its z is finite)

__device__ __forceinline__ void rows3(const double *m, double x, double y, double z, double *o)
{
    for (int r = 0; r < 3; ++r) o[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// Is point i, of box b, alive: its box kept, its mask > 0, x, y and z finite and z > 0?  u = cam_p of its frame .
// [x y z 1]; what becomes of u is the caller's.  u is written for a dead point too, where nobody reads it: filled
// under `on`, u would join the two paths behind the call, and the caller's `if` would be a second branch on the same
// condition; written like this the products sink into that `if`.
__device__ __forceinline__ bool alive(const float *xyz, const float *valid_mask, const int *box_frame,
                                      const int *box_keep, const double *cam_p, long long i, int b, double *u)
{
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const bool on = (box_keep == nullptr || box_keep[b] != 0) && (valid_mask == nullptr || valid_mask[i] > 0.0f) &&
                    isfinite(x) && isfinite(y) && isfinite(z) && z > 0.0f;
    rows3(cam_p + 12 * box_frame[b], (double)x, (double)y, (double)z, u);
    return on;
}

// frame_box[f] = the first box of frame f (box_frame is sorted), frame_box[n_frames] = n_boxes
__global__ void __launch_bounds__(kThreads) frame_box_kernel(const int *__restrict__ box_frame, int n_boxes,
                                                             int n_frames, int *__restrict__ frame_box)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f > n_frames) return;
    int lo = 0, hi = n_boxes;  // lower bound of f
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (box_frame[mid] < f)
            lo = mid + 1;
        else
            hi = mid;
    }
    frame_box[f] = lo;
}

__global__ void __launch_bounds__(kThreads) project_kernel(const float *__restrict__ xyz,
                                                           const float *__restrict__ valid_mask,
                                                           const int *__restrict__ box_frame,
                                                           const int *__restrict__ box_keep,
                                                           const double *__restrict__ cam_p,
                                                           const int *__restrict__ frame_hw,
                                                           const long long *__restrict__ pixel_offset, long long n,
                                                           int points_per_box, unsigned long long *__restrict__ keys,
                                                           int *__restrict__ pix)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / points_per_box);
        int at = -1;
        double u[3];
        if (alive(xyz, valid_mask, box_frame, box_keep, cam_p, i, b, u)) {
            const int f = box_frame[b];
            const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
            const double col = rint(u[0] / u[2]), row = rint(u[1] / u[2]);
            // NaN fails every comparison; +-inf fails the range test; -0.0 is inside
            if (u[2] > 0.0 && col >= 0.0 && col < (double)w && row >= 0.0 && row < (double)h) {
                at = (int)row * w + (int)col;
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(xyz[3 * i + 2]) << 32) | (unsigned long long)(unsigned)i;
                atomicMin(keys + pixel_offset[f] + at, key);
            }
        }
        pix[i] = at;
    }
}

// one thread per pixel of either z-buffer: a key's lower half is the id of a point or of a triangle, ids_per_box of
// them to a box; ids (may be null) takes it, -1 where nothing fell
__global__ void __launch_bounds__(kThreads) resolve_kernel(const unsigned long long *__restrict__ keys,
                                                           long long total_pixels, const int *__restrict__ box_frame,
                                                           const int *__restrict__ frame_box, unsigned ids_per_box,
                                                           float *__restrict__ depth,
                                                           unsigned char *__restrict__ instance, int *__restrict__ ids)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total_pixels;
         i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        float d = 0.0f;
        unsigned char inst = 255;
        int id = -1;
        if (key != kEmptyKey) {
            d = __uint_as_float((unsigned)(key >> 32));
            id = (int)(unsigned)key;
            const int b = (int)((unsigned)key / ids_per_box);
            inst = (unsigned char)(b - frame_box[box_frame[b]]);
        }
        depth[i] = d;
        instance[i] = inst;
        if (ids) ids[i] = id;
    }
}

// is point i its pixel's winner, key being that pixel's?
__device__ __forceinline__ bool wins(unsigned long long key, long long i) { return (unsigned)key == (unsigned)i; }

// Adds the depth error of an element whose key won its pixel, against the ground-truth depth d there, to s = the sums
// of e, |e| and e * e, e = (double) the key's depth - (double) d; false, and nothing added, where d is no measurement.
__device__ __forceinline__ bool add_depth_error(unsigned long long key, float d, double *s)
{
    if (!(isfinite(d) && d > 0.0f)) return false;
    const double e = (double)__uint_as_float((unsigned)(key >> 32)) - (double)d;
    s[0] += e;
    s[1] += fabs(e);
    s[2] += e * e;
    return true;
}

// The end of a one-workgroup-per-box pass.  n: N counts per wave (every lane holds its wave's); s: S fp64 sums per
// thread.  On return thread 0 holds the workgroup's totals in both: s reduced within a wave by a fixed tree (lane l +=
// lane l + o, o = 32 .. 1), then both combined in wave order through LDS.  The order does not depend on scheduling.
template <int N, int S>
__device__ __forceinline__ void block_tally(int *n, double *s)
{
    __shared__ int part[N][kWaves];
    __shared__ double dpart[S ? S : 1][kWaves];  // (S = 0: never touched, and dropped)
    for (int k = 0; k < S; ++k)
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o);
    if ((threadIdx.x & 63) == 0) {
        for (int k = 0; k < N; ++k) part[k][threadIdx.x >> 6] = n[k];
        for (int k = 0; k < S; ++k) dpart[k][threadIdx.x >> 6] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < N; ++k) n[k] = 0;
        for (int k = 0; k < S; ++k) s[k] = 0.0;
        for (int v = 0; v < kWaves; ++v) {  // in wave order
            for (int k = 0; k < N; ++k) n[k] += part[k][v];
            for (int k = 0; k < S; ++k) s[k] += dpart[k][v];
        }
    }
}

// one workgroup per box: kept[b] and visible[b]
__global__ void __launch_bounds__(kThreads) count_kernel(const unsigned long long *__restrict__ keys,
                                                         const int *__restrict__ pix,
                                                         const int *__restrict__ box_frame,
                                                         const long long *__restrict__ pixel_offset,
                                                         int points_per_box, int *__restrict__ kept,
                                                         int *__restrict__ visible)
{
    const int b = blockIdx.x;
    const unsigned long long *fkeys = keys + pixel_offset[box_frame[b]];
    const long long i0 = (long long)b * points_per_box;
    int n[2] = {0, 0};  // kept, visible
    for (int p0 = 0; p0 < points_per_box; p0 += kThreads) {
        const int p = p0 + threadIdx.x;
        const int at = p < points_per_box ? pix[i0 + p] : -1;
        n[0] += __popcll(__ballot(at >= 0));
        n[1] += __popcll(__ballot(at >= 0 && wins(fkeys[at], i0 + p)));
    }
    block_tally<2, 0>(n, nullptr);
    if (threadIdx.x == 0) {
        kept[b] = n[0];
        visible[b] = n[1];
    }
}

// One workgroup: box_offset (n_boxes + 1) = the exclusive scan of the boxes' counts (int64), and frame_offset
// (n_frames + 1) = box_offset at each frame's first box (n_boxes past the last box): the thread of box b writes the
// entries of the frames that start at b, i.e. box_frame[b] and the frames without a box in front of it.
__global__ void __launch_bounds__(kThreads) scan_kernel(const int *__restrict__ counts, int n_boxes,
                                                        const int *__restrict__ box_frame, int n_frames,
                                                        long long *__restrict__ box_offset,
                                                        long long *__restrict__ frame_offset)
{
    __shared__ long long wave_sum[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long base = 0;
    for (int b0 = 0; b0 < n_boxes; b0 += kThreads) {
        const int b = b0 + threadIdx.x;
        const long long c = b < n_boxes ? counts[b] : 0;
        long long incl = c;  // inclusive scan within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
        for (int v = 0; v < kWaves; ++v) {
            before += v < wave ? wave_sum[v] : 0;
            all += wave_sum[v];
        }
        if (b < n_boxes) {
            const long long excl = base + before + incl - c;
            box_offset[b] = excl;
            for (int f = b ? box_frame[b - 1] + 1 : 0; f <= box_frame[b]; ++f) frame_offset[f] = excl;
        }
        base += all;
        __syncthreads();  // wave_sum is rewritten by the next slice
    }
    if (threadIdx.x == 0) {
        box_offset[n_boxes] = base;
        for (int f = box_frame[n_boxes - 1] + 1; f <= n_frames; ++f) frame_offset[f] = base;
    }
}

// one workgroup per box: its selected points, in point order, to box_offset[b] + rank
__global__ void __launch_bounds__(kThreads) write_kernel(const float *__restrict__ xyz_in,
                                                         const unsigned long long *__restrict__ keys,
                                                         const int *__restrict__ pix,
                                                         const int *__restrict__ box_frame,
                                                         const long long *__restrict__ pixel_offset,
                                                         const float *const *__restrict__ images,
                                                         const long long *__restrict__ box_offset,
                                                         int points_per_box, int visible_only,
                                                         float *__restrict__ xyz, float *__restrict__ rgb,
                                                         int *__restrict__ box, int *__restrict__ pixel)
{
    __shared__ int wave_n[kWaves];
    const int b = blockIdx.x, f = box_frame[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long *fkeys = keys + pixel_offset[f];
    const float *image = images ? images[f] : nullptr;
    const long long i0 = (long long)b * points_per_box;
    long long base = box_offset[b];
    for (int p0 = 0; p0 < points_per_box; p0 += kThreads) {
        const int p = p0 + threadIdx.x;
        const int at = p < points_per_box ? pix[i0 + p] : -1;
        const bool take = at >= 0 && (!visible_only || wins(fkeys[at], i0 + p));
        const unsigned long long mask = __ballot(take);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < kWaves; ++v) {
            before += v < wave ? wave_n[v] : 0;
            all += wave_n[v];
        }
        if (take) {
            const long long o = base + before + __popcll(mask & ((1ULL << lane) - 1ULL));
            const float *q = xyz_in + 3 * (i0 + p);
            xyz[3 * o] = q[0];
            xyz[3 * o + 1] = q[1];
            xyz[3 * o + 2] = q[2];
            if (image) {
                const float *c = image + 3 * (long long)at;
                rgb[3 * o] = c[0];
                rgb[3 * o + 1] = c[1];
                rgb[3 * o + 2] = c[2];
            }
            box[o] = b;
            pixel[o] = at;
        }
        base += all;
        __syncthreads();  // wave_n is rewritten by the next slice
    }
}

// value counts of frame blockIdx.y's ground-truth instance image, added into hist[frame][256] (zeroed by the caller).
// 255, the background, is most of an image: it is counted in a register, not in LDS.
__global__ void __launch_bounds__(kThreads) hist_kernel(const unsigned char *const *__restrict__ gt_instance,
                                                        const long long *__restrict__ pixel_offset,
                                                        int *__restrict__ hist)
{
    __shared__ int bins[256];
    const int f = blockIdx.y;
    const unsigned char *img = gt_instance[f];
    const long long n = pixel_offset[f + 1] - pixel_offset[f];
    bins[threadIdx.x] = 0;
    __syncthreads();
    int background = 0;
    auto count = [&](unsigned v) {
        if (v == 255u)
            ++background;
        else
            atomicAdd(&bins[v], 1);
    };
    // [0, head): bytes in front of the first 16-byte boundary; [head, head + 16 body): aligned vectors; the rest: bytes
    const long long to_boundary = (long long)((16 - ((unsigned long long)img & 15)) & 15);
    const long long head = to_boundary < n ? to_boundary : n;
    const long long body = (n - head) / 16;
    const uint4 *vec = reinterpret_cast<const uint4 *>(img + head);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < body; i += (long long)gridDim.x * kThreads) {
        const uint4 q = vec[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        for (int k = 0; k < 4; ++k)
            for (int s = 0; s < 32; s += 8) count((w[k] >> s) & 255u);
    }
    if (blockIdx.x == 0) {
        const long long tail = head + 16 * body;  // n - tail < 16, head < 16: one thread each
        if (threadIdx.x < head) count(img[threadIdx.x]);
        if (tail + threadIdx.x < n) count(img[tail + threadIdx.x]);
    }
    for (int o = 32; o > 0; o >>= 1) background += __shfl_down(background, o);
    if ((threadIdx.x & 63) == 0 && background) atomicAdd(&bins[255], background);
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(hist + 256 * (long long)f + threadIdx.x, bins[threadIdx.x]);
}

// one workgroup per box: counts[b][6] = kept, on_points, pred_px, inter_px, gt_px, depth_n and sums[b][3] = the sums of
// e, |e| and e * e over the depth_n points, e = (double)z - (double)gt depth
__global__ void __launch_bounds__(kThreads) score_kernel(const unsigned long long *__restrict__ keys,
                                                         const int *__restrict__ pix,
                                                         const int *__restrict__ box_frame,
                                                         const int *__restrict__ box_gt_id,
                                                         const float *const *__restrict__ gt_depth,
                                                         const unsigned char *const *__restrict__ gt_instance,
                                                         const long long *__restrict__ pixel_offset,
                                                         const int *__restrict__ hist, int points_per_box,
                                                         int *__restrict__ counts, double *__restrict__ sums)
{
    const int b = blockIdx.x, f = box_frame[b], g = box_gt_id[b];
    const bool has_gt = g >= 0 && g <= 254;
    const unsigned long long *fkeys = keys + pixel_offset[f];
    const unsigned char *inst = gt_instance[f];
    const float *depth = gt_depth[f];
    const long long i0 = (long long)b * points_per_box;
    int n[5] = {0, 0, 0, 0, 0};     // kept, on_points, pred_px, inter_px, depth_n
    double s[3] = {0.0, 0.0, 0.0};  // in slice order
    for (int p0 = 0; p0 < points_per_box; p0 += kThreads) {
        const int p = p0 + threadIdx.x;
        const int at = p < points_per_box ? pix[i0 + p] : -1;
        const bool kept = at >= 0;
        const bool on = kept && has_gt && (int)inst[at] == g;
        const unsigned long long key = kept ? fkeys[at] : kEmptyKey;
        const bool visible = kept && wins(key, i0 + p);
        const bool inter = visible && on;
        const bool measured = inter && add_depth_error(key, depth[at], s);
        n[0] += __popcll(__ballot(kept));
        n[1] += __popcll(__ballot(on));
        n[2] += __popcll(__ballot(visible));
        n[3] += __popcll(__ballot(inter));
        n[4] += __popcll(__ballot(measured));
    }
    block_tally<5, 3>(n, s);
    if (threadIdx.x == 0) {
        int *out = counts + 6 * (long long)b;
        out[0] = n[0];
        out[1] = n[1];
        out[2] = n[2];
        out[3] = n[3];
        out[4] = has_gt ? hist[256 * (long long)f + g] : 0;
        out[5] = n[4];
        for (int k = 0; k < 3; ++k) sums[3 * (long long)b + k] = s[k];
    }
}

// A workspace is a row of regions, each aligned to 256 bytes: take() lays the next one behind the others.
struct Regions {
    size_t total = 0;

    size_t take(size_t bytes)
    {
        const size_t at = total;
        total += mpsr::align_up(bytes, 256);
        return at;
    }
};

// A z-buffer's workspace begins [keys: one uint64 per pixel] [frame_box: n_frames + 1 ints], whatever is drawn into it.
struct ZLayout : Regions {
    size_t keys, frame_box;

    ZLayout(int n_frames, long long total_pixels)
    {
        keys = take((size_t)total_pixels * sizeof(unsigned long long));
        frame_box = take(((size_t)n_frames + 1) * sizeof(int));
    }
};

// the points' workspace: ... [pix: one int per point] [box_offset: n_boxes + 1 int64]
struct SceneLayout : ZLayout {
    size_t pix, box_offset;

    SceneLayout(int n_frames, long long total_pixels, int n_boxes, int points_per_box) : ZLayout(n_frames, total_pixels)
    {
        pix = take((size_t)n_boxes * points_per_box * sizeof(int));
        box_offset = take(((size_t)n_boxes + 1) * sizeof(long long));
    }
};

// the sizes every entry point takes; *empty: nothing to do
int check_sizes(const char *who, int n_frames, long long total_pixels, int n_boxes, int points_per_box, bool *empty)
{
    MPSR_REQUIRE(n_frames >= 0 && total_pixels >= 0 && n_boxes >= 0 && points_per_box >= 0,
                 "%s: negative size (n_frames %d, total_pixels %lld, n_boxes %d, points_per_box %d)", who, n_frames,
                 total_pixels, n_boxes, points_per_box);
    MPSR_REQUIRE((long long)n_boxes * points_per_box < (1LL << 32),
                 "%s: %d boxes of %d points: the point index does not fit the key's 32 bits", who, n_boxes,
                 points_per_box);
    MPSR_REQUIRE(total_pixels <= (1LL << 40), "%s: %lld pixels are too many", who, total_pixels);
    *empty = n_frames == 0 || n_boxes == 0 || points_per_box == 0;
    return MPSR_OK;
}

int check_workspace(const char *who, const void *workspace, size_t workspace_bytes, size_t need)
{
    if (!workspace || workspace_bytes < need)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "%s: workspace %zu bytes < %zu", who, workspace_bytes, need);
    return MPSR_OK;
}

// box_frame (host): in [0, n_frames) and never decreasing; at most max_per_frame boxes in a frame (0: any number)
int check_box_frames(const char *who, const int *box_frame_host, int n_boxes, int n_frames, int max_per_frame)
{
    int run = 0;
    for (int b = 0; b < n_boxes; ++b) {
        const int f = box_frame_host[b];
        MPSR_REQUIRE(f >= 0 && f < n_frames, "%s: box %d is of frame %d (0..%d)", who, b, f, n_frames - 1);
        MPSR_REQUIRE(b == 0 || f >= box_frame_host[b - 1], "%s: box_frame decreases at box %d (%d after %d)", who, b,
                     f, b ? box_frame_host[b - 1] : 0);
        run = (b > 0 && f == box_frame_host[b - 1]) ? run + 1 : 1;
        MPSR_REQUIRE(max_per_frame == 0 || run <= max_per_frame,
                     "%s: frame %d has more than %d boxes (255 of an instance image is the background)", who, f,
                     max_per_frame);
    }
    return MPSR_OK;
}

// frame_hw and pixel_offset (host): positive sizes of at most 2^30 pixels, offsets that start at 0 and agree with them
int check_frame_tables(const char *who, const int *frame_hw_host, const long long *pixel_offset_host, int n_frames)
{
    MPSR_REQUIRE(pixel_offset_host[0] == 0, "%s: pixel_offset[0] = %lld, expected 0", who, pixel_offset_host[0]);
    for (int f = 0; f < n_frames; ++f) {
        const int h = frame_hw_host[2 * f], w = frame_hw_host[2 * f + 1];
        MPSR_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "%s: frame %d is %d x %d", who, f, h, w);
        MPSR_REQUIRE(pixel_offset_host[f + 1] - pixel_offset_host[f] == (long long)h * w,
                     "%s: pixel_offset of frame %d spans %lld pixels, its image has %lld", who, f,
                     pixel_offset_host[f + 1] - pixel_offset_host[f], (long long)h * w);
    }
    return MPSR_OK;
}

// scratch, checked = hist (n_frames, 256) int32 = the value counts of the ground-truth instance images: zeroed, then
// hist_kernel
int launch_hist(const char *who, const unsigned char *const *gt_instance, const long long *pixel_offset, int n_frames,
                long long total_pixels, void *scratch, size_t scratch_bytes, hipStream_t s)
{
    const size_t need = mpsr_scene_score_scratch_bytes(n_frames);
    if (!scratch || scratch_bytes < need)
        return mpsr::fail(MPSR_ERR_WORKSPACE, "%s: scratch %zu bytes < %zu", who, scratch_bytes, need);
    int *hist = static_cast<int *>(scratch);
    MPSR_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n_frames * 256 * sizeof(int), s));
    // workgroups per frame: one per 64 KiB of an average frame (a frame of any size is walked with the grid's stride)
    const long long per_frame = (total_pixels + n_frames - 1) / n_frames;
    const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((per_frame + 65535) / 65536, 1), 64);
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {  // (gridDim.y holds 65535)
        const int nf = std::min(n_frames - f0, 65535);
        hipLaunchKernelGGL(hist_kernel, dim3(gx, nf), dim3(kThreads), 0, s, gt_instance + f0, pixel_offset + f0,
                           hist + 256 * (size_t)f0);
    }
    return MPSR_OK;
}

unsigned grid_for(long long n) { return (unsigned)std::min<long long>((n + kThreads - 1) / kThreads, 1 << 16); }

// What mpsr_scene_project and mpsr_scene_surface_render check alike once their own sizes are known good: the pointers,
// the frame tables, the *total_pixels these give (read once the pointer is known to be there) and box_frame.
int check_render_args(const char *who, const float *xyz_global, const int *box_frame, const int *box_frame_host,
                      const double *cam_p, const int *frame_hw, const int *frame_hw_host,
                      const long long *pixel_offset, const long long *pixel_offset_host, int n_frames, int n_boxes,
                      long long *total_pixels)
{
    MPSR_REQUIRE(xyz_global && box_frame && box_frame_host, "%s: points or box_frame is null", who);
    MPSR_REQUIRE(cam_p && frame_hw && frame_hw_host && pixel_offset && pixel_offset_host,
                 "%s: cameras, frame sizes or pixel offsets are null", who);
    int st = check_frame_tables(who, frame_hw_host, pixel_offset_host, n_frames);
    if (st) return st;
    *total_pixels = pixel_offset_host[n_frames];
    bool empty;
    st = check_sizes(who, n_frames, *total_pixels, n_boxes, 1, &empty);  // (the caller has checked what a box holds)
    if (st) return st;
    return check_box_frames(who, box_frame_host, n_boxes, n_frames, 0);
}

// starts a z-buffer in a checked workspace: every key empty, frame_box filled
int start_zbuffer(const char *who, void *workspace, size_t workspace_bytes, const ZLayout &L, long long total_pixels,
                  const int *box_frame, int n_boxes, int n_frames, hipStream_t s)
{
    int st = check_workspace(who, workspace, workspace_bytes, L.total);
    if (st) return st;
    char *ws = static_cast<char *>(workspace);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + L.keys);
    MPSR_CHECK_HIP(hipMemsetAsync(keys, 0xff, (size_t)total_pixels * sizeof(unsigned long long), s));  // kEmptyKey
    hipLaunchKernelGGL(frame_box_kernel, dim3((n_frames + 1 + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                       box_frame, n_boxes, n_frames, reinterpret_cast<int *>(ws + L.frame_box));
    return MPSR_OK;
}

// a non-empty z-buffer's keys -> depth, instance and (ids not null) id maps; ids_per_box: the points or triangles of a box
int resolve(const char *who, const int *box_frame, const int *box_frame_host, int n_frames, long long total_pixels,
            int n_boxes, unsigned ids_per_box, const void *workspace, size_t workspace_bytes, const ZLayout &L,
            float *depth, unsigned char *instance, int *ids, mpsr_stream_t stream)
{
    MPSR_REQUIRE(box_frame && box_frame_host && depth && instance, "%s: box_frame or an output is null", who);
    int st = check_box_frames(who, box_frame_host, n_boxes, n_frames, MPSR_INSTANCE_MAX_BOXES);
    if (st) return st;
    st = check_workspace(who, workspace, workspace_bytes, L.total);
    if (st) return st;
    const char *ws = static_cast<const char *>(workspace);
    hipLaunchKernelGGL(resolve_kernel, dim3(grid_for(total_pixels)), dim3(kThreads), 0, mpsr::as_stream(stream),
                       reinterpret_cast<const unsigned long long *>(ws + L.keys), total_pixels, box_frame,
                       reinterpret_cast<const int *>(ws + L.frame_box), ids_per_box, depth, instance, ids);
    MPSR_CHECK_LAUNCH(who);
    return MPSR_OK;
}

}  // namespace

extern "C" size_t mpsr_scene_workspace_bytes(int n_frames, long long total_pixels, int n_boxes, int points_per_box)
{
    if (n_frames <= 0 || total_pixels <= 0 || n_boxes <= 0 || points_per_box <= 0) return 0;
    if ((long long)n_boxes * points_per_box >= (1LL << 32) || total_pixels > (1LL << 40)) return 0;
    return SceneLayout(n_frames, total_pixels, n_boxes, points_per_box).total;
}

extern "C" int mpsr_scene_project(const float *xyz_global, const float *valid_mask, const int *box_frame,
                                  const int *box_frame_host, const int *box_keep, const double *cam_p,
                                  const int *frame_hw, const int *frame_hw_host, const long long *pixel_offset,
                                  const long long *pixel_offset_host, int n_frames, int n_boxes, int points_per_box,
                                  void *workspace, size_t workspace_bytes, mpsr_stream_t stream)
{
    const char *who = "scene_project";
    bool empty;
    int st = check_sizes(who, n_frames, 0, n_boxes, points_per_box, &empty);
    if (st) return st;
    if (empty) return MPSR_OK;
    long long total_pixels;
    st = check_render_args(who, xyz_global, box_frame, box_frame_host, cam_p, frame_hw, frame_hw_host, pixel_offset,
                           pixel_offset_host, n_frames, n_boxes, &total_pixels);
    if (st) return st;
    const SceneLayout L(n_frames, total_pixels, n_boxes, points_per_box);
    hipStream_t s = mpsr::as_stream(stream);
    st = start_zbuffer(who, workspace, workspace_bytes, L, total_pixels, box_frame, n_boxes, n_frames, s);
    if (st) return st;
    char *ws = static_cast<char *>(workspace);
    const long long n = (long long)n_boxes * points_per_box;
    hipLaunchKernelGGL(project_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, xyz_global, valid_mask, box_frame,
                       box_keep, cam_p, frame_hw, pixel_offset, n, points_per_box,
                       reinterpret_cast<unsigned long long *>(ws + L.keys), reinterpret_cast<int *>(ws + L.pix));
    MPSR_CHECK_LAUNCH(who);
    return MPSR_OK;
}

extern "C" int mpsr_scene_resolve(const int *box_frame, const int *box_frame_host, int n_frames,
                                  long long total_pixels, int n_boxes, int points_per_box, const void *workspace,
                                  size_t workspace_bytes, float *depth, unsigned char *instance, mpsr_stream_t stream)
{
    bool empty;
    int st = check_sizes("scene_resolve", n_frames, total_pixels, n_boxes, points_per_box, &empty);
    if (st) return st;
    if (empty || total_pixels == 0) return MPSR_OK;
    return resolve("scene_resolve", box_frame, box_frame_host, n_frames, total_pixels, n_boxes,
                   (unsigned)points_per_box, workspace, workspace_bytes,
                   SceneLayout(n_frames, total_pixels, n_boxes, points_per_box), depth, instance, nullptr, stream);
}

extern "C" int mpsr_scene_compact(const float *xyz_global, const int *box_frame, const float *const *images,
                                  const long long *pixel_offset, int n_frames, long long total_pixels, int n_boxes,
                                  int points_per_box, int visible_only, void *workspace, size_t workspace_bytes,
                                  float *xyz, float *rgb, int *box, int *pixel, long long *frame_offset,
                                  int *kept_per_box, int *visible_per_box, mpsr_stream_t stream)
{
    bool empty;
    int st = check_sizes("scene_compact", n_frames, total_pixels, n_boxes, points_per_box, &empty);
    if (st) return st;
    if (empty || total_pixels == 0) return MPSR_OK;
    MPSR_REQUIRE(xyz_global && box_frame && pixel_offset, "scene_compact: points, box_frame or pixel_offset is null");
    MPSR_REQUIRE(xyz && box && pixel && frame_offset && kept_per_box && visible_per_box,
                 "scene_compact: an output is null");
    MPSR_REQUIRE((images == nullptr) == (rgb == nullptr), "scene_compact: images and rgb go together (both or neither)");
    const SceneLayout L(n_frames, total_pixels, n_boxes, points_per_box);
    st = check_workspace("scene_compact", workspace, workspace_bytes, L.total);
    if (st) return st;
    char *ws = static_cast<char *>(workspace);
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(ws + L.keys);
    const int *pix = reinterpret_cast<const int *>(ws + L.pix);
    long long *box_offset = reinterpret_cast<long long *>(ws + L.box_offset);
    hipStream_t s = mpsr::as_stream(stream);
    hipLaunchKernelGGL(count_kernel, dim3(n_boxes), dim3(kThreads), 0, s, keys, pix, box_frame, pixel_offset,
                       points_per_box, kept_per_box, visible_per_box);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, s, visible_only ? visible_per_box : kept_per_box,
                       n_boxes, box_frame, n_frames, box_offset, frame_offset);
    hipLaunchKernelGGL(write_kernel, dim3(n_boxes), dim3(kThreads), 0, s, xyz_global, keys, pix, box_frame,
                       pixel_offset, images, box_offset, points_per_box, visible_only, xyz, rgb, box, pixel);
    MPSR_CHECK_LAUNCH("scene_compact");
    return MPSR_OK;
}

extern "C" size_t mpsr_scene_score_scratch_bytes(int n_frames)
{
    return n_frames <= 0 ? 0 : (size_t)n_frames * 256 * sizeof(int);
}

extern "C" int mpsr_scene_score(const float *xyz_global, const int *box_frame, const int *box_frame_host,
                                const int *box_gt_id, const float *const *gt_depth,
                                const unsigned char *const *gt_instance, const long long *pixel_offset, int n_frames,
                                long long total_pixels, int n_boxes, int points_per_box, const void *workspace,
                                size_t workspace_bytes, void *scratch, size_t scratch_bytes, int *counts, double *sums,
                                mpsr_stream_t stream)
{
    bool empty;
    int st = check_sizes("scene_score", n_frames, total_pixels, n_boxes, points_per_box, &empty);
    if (st) return st;
    if (empty || total_pixels == 0) return MPSR_OK;
    MPSR_REQUIRE(xyz_global && box_frame && box_frame_host && box_gt_id && pixel_offset,
                 "scene_score: points, box_frame, box_gt_id or pixel_offset is null");
    MPSR_REQUIRE(gt_depth && gt_instance, "scene_score: a ground-truth table is null");
    MPSR_REQUIRE(counts && sums, "scene_score: an output is null");
    st = check_box_frames("scene_score", box_frame_host, n_boxes, n_frames, 0);
    if (st) return st;
    const SceneLayout L(n_frames, total_pixels, n_boxes, points_per_box);
    st = check_workspace("scene_score", workspace, workspace_bytes, L.total);
    if (st) return st;
    hipStream_t s = mpsr::as_stream(stream);
    st = launch_hist("scene_score", gt_instance, pixel_offset, n_frames, total_pixels, scratch, scratch_bytes, s);
    if (st) return st;
    const char *ws = static_cast<const char *>(workspace);
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(ws + L.keys);
    const int *pix = reinterpret_cast<const int *>(ws + L.pix);
    hipLaunchKernelGGL(score_kernel, dim3(n_boxes), dim3(kThreads), 0, s, keys, pix, box_frame, box_gt_id, gt_depth,
                       gt_instance, pixel_offset, static_cast<const int *>(scratch), points_per_box, counts, sums);
    MPSR_CHECK_LAUNCH("scene_score");
    return MPSR_OK;
}

// ---- Surfaces: a box's (map_h, map_w) xyz map rendered as the triangles of its grid cells
// through the same 64-bit z-buffer, next to the point rendering above and in a workspace of its own.
// mpsr_scene_surface_render: surface_vertex_kernel, one thread per map point, snaps a valid vertex to fixed-point
//   screen coordinates with 8 sub-pixel bits (the centre of pixel (col, row) is (256 col, 256 row), as a point's pixel
//   is rint(u)); surface_triangle_kernel, one thread per triangle, walks the pixel centres of the triangle's extent
//   with exact int64 edge functions and an ownership rule for centres on an edge, computes the perspective-correct
//   depth in fp64 and lowers the pixel's key ((uint64) float_bits(depth) << 32 | triangle id) with the unsigned
//   atomicMin.  Per box it counts the drawn triangles and takes the bounding rectangle of their clamped extents:
//   integer atomics, one set per wave where the wave's triangles are of one box.
// mpsr_scene_surface_resolve: keys -> depth, instance and (optionally) triangle id maps, by the points' resolve_kernel.
// mpsr_scene_surface_score: hist_kernel, then one workgroup per box over the box's rectangle, row-major in slices of
//   256 pixels, summed and reduced by score_kernel's add_depth_error and block_tally.

namespace {

constexpr int kSubPixel = 256;             // fixed-point units per pixel
constexpr int kNoVertex = INT_MIN;         // X of an invalid vertex
constexpr double kMaxScreen = 1048576.0;   // 2^20 pixels: |u / u2| of a valid vertex is below it
constexpr int kMaxSpan = 1024;

__device__ __forceinline__ int floor_div256(int v) { return v >> 8; }  // arithmetic shift: floor for v < 0 too
__device__ __forceinline__ int ceil_div256(int v) { return -((-v) >> 8); }

// does the directed edge with direction (dx, dy) own the pixel centres that lie exactly on it?
__device__ __forceinline__ bool owns(long long dx, long long dy) { return dy > 0 || (dy == 0 && dx < 0); }

// one thread per map point: vert[i] = (X, Y), X = kNoVertex for an invalid vertex; the first n_boxes threads also
// reset the per-box tables (tris 0, an empty rectangle)
__global__ void __launch_bounds__(kThreads) surface_vertex_kernel(const float *__restrict__ xyz,
                                                                  const float *__restrict__ valid_mask,
                                                                  const int *__restrict__ box_frame,
                                                                  const int *__restrict__ box_keep,
                                                                  const double *__restrict__ cam_p, long long n,
                                                                  int points_per_box, int n_boxes,
                                                                  int2 *__restrict__ vert, int *__restrict__ box_tris,
                                                                  int *__restrict__ box_rect)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        if (i < n_boxes) {
            box_tris[i] = 0;
            box_rect[4 * i] = box_rect[4 * i + 1] = INT_MAX;      // min col, min row
            box_rect[4 * i + 2] = box_rect[4 * i + 3] = INT_MIN;  // max col, max row
        }
        int2 v = make_int2(kNoVertex, 0);
        double u[3];
        if (alive(xyz, valid_mask, box_frame, box_keep, cam_p, i, (int)(i / points_per_box), u)) {
            const double c = u[0] / u[2], r = u[1] / u[2];
            // NaN fails both range tests
            if (u[2] > 0.0 && fabs(c) < kMaxScreen && fabs(r) < kMaxScreen)
                v = make_int2((int)rint(c * (double)kSubPixel), (int)rint(r * (double)kSubPixel));
        }
        vert[i] = v;
    }
}

// Triangle n of a box (n = 2 (i cells_w + j) + k): its corners (a, b, c) as map points of the box.
// k = 0: (v00, v01, v10); k = 1: (v11, v10, v01)
__device__ __forceinline__ void triangle_corners(long long n, int cells_w, int map_w, long long *ia, long long *ib,
                                                 long long *ic)
{
    const long long cell = n >> 1;
    const long long v00 = (cell / cells_w) * map_w + cell % cells_w;
    const bool k = n & 1;
    *ia = k ? v00 + map_w + 1 : v00;
    *ib = k ? v00 + map_w : v00 + 1;
    *ic = k ? v00 + 1 : v00 + map_w;
}

// The one rule for which triangle is DRAWN; the renderer and the mesh's selection both ask it.
// (ia, ib, ic): the corners as indices into vert and xyz.  p: their screen coordinates, z: their float32 depths, *A:
// the doubled screen area, ext = c0, c1, r0, r1: the unclamped pixel extent; z, A and ext only where all three
// vertices are valid.
__device__ __forceinline__ bool triangle_drawn(const float *xyz, const int2 *vert, long long ia, long long ib,
                                               long long ic, float max_edge_dz, int max_span_px, int2 *p, float *z,
                                               long long *A, int *ext)
{
    const int2 pa = vert[ia], pb = vert[ib], pc = vert[ic];
    p[0] = pa, p[1] = pb, p[2] = pc;
    if (pa.x == kNoVertex || pb.x == kNoVertex || pc.x == kNoVertex) return false;
    const float za = xyz[3 * ia + 2], zb = xyz[3 * ib + 2], zc = xyz[3 * ic + 2];
    z[0] = za, z[1] = zb, z[2] = zc;
    const float dz = fmaxf(fmaxf(za, zb), zc) - fminf(fminf(za, zb), zc);
    *A = (long long)(pb.x - pa.x) * (pc.y - pa.y) - (long long)(pb.y - pa.y) * (pc.x - pa.x);
    const int c0 = ceil_div256(min(min(pa.x, pb.x), pc.x)), c1 = floor_div256(max(max(pa.x, pb.x), pc.x));
    const int r0 = ceil_div256(min(min(pa.y, pb.y), pc.y)), r1 = floor_div256(max(max(pa.y, pb.y), pc.y));
    ext[0] = c0, ext[1] = c1, ext[2] = r0, ext[3] = r1;
    return !(dz > max_edge_dz) && *A != 0 && c1 - c0 + 1 <= max_span_px && r1 - r0 + 1 <= max_span_px;
}

__global__ void __launch_bounds__(kThreads) surface_triangle_kernel(const float *__restrict__ xyz,
                                                                    const int2 *__restrict__ vert,
                                                                    const int *__restrict__ box_frame,
                                                                    const int *__restrict__ frame_hw,
                                                                    const long long *__restrict__ pixel_offset,
                                                                    long long n_tris, int map_h, int map_w,
                                                                    float max_edge_dz, int max_span_px,
                                                                    unsigned long long *__restrict__ keys,
                                                                    int *__restrict__ box_tris,
                                                                    int *__restrict__ box_rect)
{
    const int cells_w = map_w - 1;
    const long long points_per_box = (long long)map_h * map_w, per_box = 2LL * (map_h - 1) * cells_w;
    // every lane of a wave makes the same number of rounds, so that the wave can combine its per-box bookkeeping
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long first = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63);
    for (long long t0 = first; t0 < n_tris; t0 += stride) {
        const long long t = t0 + (threadIdx.x & 63);
        const bool live = t < n_tris;
        int b = -1, drawn = 0;
        int lo_c = INT_MAX, lo_r = INT_MAX, hi_c = INT_MIN, hi_r = INT_MIN;  // the clamped extent, empty
        if (live) {
            b = (int)(t / per_box);
            long long ia, ib, ic, A;
            triangle_corners(t - b * per_box, cells_w, map_w, &ia, &ib, &ic);
            const long long i0 = (long long)b * points_per_box;
            int2 p[3];
            float z[3];
            int ext[4];
            if (triangle_drawn(xyz, vert, i0 + ia, i0 + ib, i0 + ic, max_edge_dz, max_span_px, p, z, &A, ext)) {
                const int2 pa = p[0];
                int2 pb = p[1], pc = p[2];
                const float za = z[0];
                float zb = z[1], zc = z[2];
                const int c0 = ext[0], c1 = ext[1], r0 = ext[2], r1 = ext[3];
                drawn = 1;
                if (A < 0) {  // the other facing: swap the second and the third vertex
                    const int2 pp = pb;
                    pb = pc;
                    pc = pp;
                    const float zz = zb;
                    zb = zc;
                    zc = zz;
                    A = -A;
                }
                const int f = box_frame[b];
                const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
                const int cc0 = max(c0, 0), cc1 = min(c1, w - 1), rr0 = max(r0, 0), rr1 = min(r1, h - 1);
                if (cc0 <= cc1 && rr0 <= rr1) {
                    lo_c = cc0, hi_c = cc1, lo_r = rr0, hi_r = rr1;
                    unsigned long long *fkeys = keys + pixel_offset[f];
                    const long long bcx = pc.x - pb.x, bcy = pc.y - pb.y, cax = pa.x - pc.x, cay = pa.y - pc.y;
                    const long long abx = pb.x - pa.x, aby = pb.y - pa.y;
                    const bool own0 = owns(bcx, bcy), own1 = owns(cax, cay), own2 = owns(abx, aby);
                    const double wa = 1.0 / (double)za, wb = 1.0 / (double)zb, wc = 1.0 / (double)zc;
                    for (int row = rr0; row <= rr1; ++row) {
                        const long long sy = (long long)row * kSubPixel;
                        for (int col = cc0; col <= cc1; ++col) {
                            const long long sx = (long long)col * kSubPixel;
                            const long long e0 = bcx * (sy - pb.y) - bcy * (sx - pb.x);
                            const long long e1 = cax * (sy - pc.y) - cay * (sx - pc.x);
                            const long long e2 = abx * (sy - pa.y) - aby * (sx - pa.x);
                            if ((e0 > 0 || (e0 == 0 && own0)) && (e1 > 0 || (e1 == 0 && own1)) &&
                                (e2 > 0 || (e2 == 0 && own2))) {
                                const double q = ((double)e0 * wa + (double)e1 * wb) + (double)e2 * wc;
                                const float zf = (float)((double)A / q);
                                atomicMin(fkeys + (long long)row * w + col,
                                          ((unsigned long long)__float_as_uint(zf) << 32) |
                                              (unsigned long long)(unsigned)t);
                            }
                        }
                    }
                }
            }
        }
        // bookkeeping: the wave's triangles are of one box almost always (a box has thousands)
        const int b_first = __shfl(b, 0);  // (lane 0 is live whenever any lane is)
        if (__all(!live || b == b_first)) {
            for (int o = 32; o > 0; o >>= 1) {
                drawn += __shfl_down(drawn, o);
                lo_c = min(lo_c, __shfl_down(lo_c, o));
                lo_r = min(lo_r, __shfl_down(lo_r, o));
                hi_c = max(hi_c, __shfl_down(hi_c, o));
                hi_r = max(hi_r, __shfl_down(hi_r, o));
            }
            if ((threadIdx.x & 63) != 0) drawn = 0;  // lane 0 speaks for the wave
        }
        if (drawn) {
            atomicAdd(box_tris + b, drawn);
            if (lo_c <= hi_c) {
                atomicMin(box_rect + 4 * (long long)b, lo_c);
                atomicMin(box_rect + 4 * (long long)b + 1, lo_r);
                atomicMax(box_rect + 4 * (long long)b + 2, hi_c);
                atomicMax(box_rect + 4 * (long long)b + 3, hi_r);
            }
        }
    }
}

// one workgroup per box: counts[b][5] = tris, pred_px, inter_px, gt_px, depth_n and sums[b][3] = the sums of e, |e| and
// e * e over the depth_n pixels, e = (double) rendered depth - (double) ground-truth depth.  The box's rectangle is
// walked row-major in slices of 256 pixels.
__global__ void __launch_bounds__(kThreads) surface_score_kernel(const unsigned long long *__restrict__ keys,
                                                                 const int *__restrict__ box_tris,
                                                                 const int *__restrict__ box_rect,
                                                                 const int *__restrict__ box_frame,
                                                                 const int *__restrict__ box_gt_id,
                                                                 const float *const *__restrict__ gt_depth,
                                                                 const unsigned char *const *__restrict__ gt_instance,
                                                                 const int *__restrict__ frame_hw,
                                                                 const long long *__restrict__ pixel_offset,
                                                                 const int *__restrict__ hist, unsigned tris_per_box,
                                                                 int *__restrict__ counts, double *__restrict__ sums)
{
    const int b = blockIdx.x, f = box_frame[b], g = box_gt_id ? box_gt_id[b] : -1;  // (null: no ground truth at all)
    const bool has_gt = g >= 0 && g <= 254;
    const unsigned long long *fkeys = keys + pixel_offset[f];
    const unsigned char *inst = has_gt ? gt_instance[f] : nullptr;
    const float *depth = has_gt ? gt_depth[f] : nullptr;
    const int w = frame_hw[2 * f + 1];
    const int c0 = box_rect[4 * (long long)b], r0 = box_rect[4 * (long long)b + 1];
    const int c1 = box_rect[4 * (long long)b + 2], r1 = box_rect[4 * (long long)b + 3];
    const long long rw = c0 <= c1 ? (long long)c1 - c0 + 1 : 0;
    const long long area = r0 <= r1 ? rw * ((long long)r1 - r0 + 1) : 0;
    int n[3] = {0, 0, 0};           // pred_px, inter_px, depth_n
    double s[3] = {0.0, 0.0, 0.0};  // in slice order
    for (long long q0 = 0; q0 < area; q0 += kThreads) {
        const long long q = q0 + threadIdx.x;
        bool mine = false, inter = false, measured = false;
        if (q < area) {
            const long long at = (r0 + q / rw) * w + (c0 + q % rw);
            const unsigned long long key = fkeys[at];
            mine = key != kEmptyKey && (unsigned)key / tris_per_box == (unsigned)b;
            inter = mine && has_gt && (int)inst[at] == g;
            measured = inter && add_depth_error(key, depth[at], s);
        }
        n[0] += __popcll(__ballot(mine));
        n[1] += __popcll(__ballot(inter));
        n[2] += __popcll(__ballot(measured));
    }
    block_tally<3, 3>(n, s);
    if (threadIdx.x == 0) {
        int *out = counts + 5 * (long long)b;
        out[0] = box_tris[b];
        out[1] = n[0];
        out[2] = n[1];
        out[3] = has_gt ? hist[256 * (long long)f + g] : 0;
        out[4] = n[2];
        for (int k = 0; k < 3; ++k) sums[3 * (long long)b + k] = s[k];
    }
}

// the surfaces' workspace: ... [vert: one int2 per map point] [box_tris: n_boxes ints] [box_rect: n_boxes x 4 ints]
struct SurfaceLayout : ZLayout {
    size_t vert, box_tris, box_rect;

    SurfaceLayout(int n_frames, long long total_pixels, int n_boxes, int map_h, int map_w)
        : ZLayout(n_frames, total_pixels)
    {
        vert = take((size_t)n_boxes * map_h * map_w * sizeof(int2));
        box_tris = take((size_t)n_boxes * sizeof(int));
        box_rect = take((size_t)n_boxes * 4 * sizeof(int));
    }
};

// the triangles of a box: two to a cell (below 2^32, as a map has at most INT_MAX points)
long long tris_per_box(int map_h, int map_w) { return 2LL * (map_h - 1) * (map_w - 1); }

// the sizes every surface entry point takes; *empty: nothing to do
int check_surface_sizes(const char *who, int n_frames, long long total_pixels, int n_boxes, int map_h, int map_w,
                        bool *empty)
{
    MPSR_REQUIRE(map_h >= 2 && map_w >= 2 && (long long)map_h * map_w <= INT_MAX,
                 "%s: a map of %d x %d has no cell (map_h and map_w must be 2 or more)", who, map_h, map_w);
    int st = check_sizes(who, n_frames, total_pixels, n_boxes, 1, empty);
    if (st) return st;
    MPSR_REQUIRE(n_boxes * tris_per_box(map_h, map_w) < (1LL << 32),
                 "%s: %d boxes of %d x %d cells: the triangle id does not fit the key's 32 bits", who, n_boxes,
                 map_h - 1, map_w - 1);
    return MPSR_OK;
}

}  // namespace

extern "C" size_t mpsr_scene_surface_workspace_bytes(int n_frames, long long total_pixels, int n_boxes, int map_h,
                                                     int map_w)
{
    if (n_frames <= 0 || total_pixels <= 0 || n_boxes <= 0 || map_h < 2 || map_w < 2) return 0;
    if ((long long)map_h * map_w > INT_MAX || total_pixels > (1LL << 40)) return 0;
    if (n_boxes * tris_per_box(map_h, map_w) >= (1LL << 32)) return 0;
    return SurfaceLayout(n_frames, total_pixels, n_boxes, map_h, map_w).total;
}

extern "C" int mpsr_scene_surface_render(const float *xyz_global, const float *valid_mask, const int *box_frame,
                                         const int *box_frame_host, const int *box_keep, const double *cam_p,
                                         const int *frame_hw, const int *frame_hw_host, const long long *pixel_offset,
                                         const long long *pixel_offset_host, int n_frames, int n_boxes, int map_h,
                                         int map_w, float max_edge_dz, int max_span_px, void *workspace,
                                         size_t workspace_bytes, mpsr_stream_t stream)
{
    const char *who = "scene_surface_render";
    bool empty;
    int st = check_surface_sizes(who, n_frames, 0, n_boxes, map_h, map_w, &empty);
    if (st) return st;
    MPSR_REQUIRE(max_span_px >= 1 && max_span_px <= kMaxSpan, "%s: max_span_px %d is outside 1..%d", who, max_span_px,
                 kMaxSpan);
    MPSR_REQUIRE(max_edge_dz > 0.0f, "%s: max_edge_dz %g must be greater than 0 (+inf: no limit)", who,
                 (double)max_edge_dz);  // NaN fails the comparison
    if (empty) return MPSR_OK;
    long long total_pixels;
    st = check_render_args(who, xyz_global, box_frame, box_frame_host, cam_p, frame_hw, frame_hw_host, pixel_offset,
                           pixel_offset_host, n_frames, n_boxes, &total_pixels);
    if (st) return st;
    const SurfaceLayout L(n_frames, total_pixels, n_boxes, map_h, map_w);
    hipStream_t s = mpsr::as_stream(stream);
    st = start_zbuffer(who, workspace, workspace_bytes, L, total_pixels, box_frame, n_boxes, n_frames, s);
    if (st) return st;
    char *ws = static_cast<char *>(workspace);
    int2 *vert = reinterpret_cast<int2 *>(ws + L.vert);
    int *box_tris = reinterpret_cast<int *>(ws + L.box_tris), *box_rect = reinterpret_cast<int *>(ws + L.box_rect);
    const int points_per_box = map_h * map_w;
    const long long n = (long long)n_boxes * points_per_box;  // n >= n_boxes: the vertex pass resets the box tables
    hipLaunchKernelGGL(surface_vertex_kernel, dim3(grid_for(n)), dim3(kThreads), 0, s, xyz_global, valid_mask,
                       box_frame, box_keep, cam_p, n, points_per_box, n_boxes, vert, box_tris, box_rect);
    const long long n_tris = n_boxes * tris_per_box(map_h, map_w);
    hipLaunchKernelGGL(surface_triangle_kernel, dim3(grid_for(n_tris)), dim3(kThreads), 0, s, xyz_global, vert,
                       box_frame, frame_hw, pixel_offset, n_tris, map_h, map_w, max_edge_dz, max_span_px,
                       reinterpret_cast<unsigned long long *>(ws + L.keys), box_tris, box_rect);
    MPSR_CHECK_LAUNCH(who);
    return MPSR_OK;
}

extern "C" int mpsr_scene_surface_resolve(const int *box_frame, const int *box_frame_host, int n_frames,
                                          long long total_pixels, int n_boxes, int map_h, int map_w,
                                          const void *workspace, size_t workspace_bytes, float *depth,
                                          unsigned char *instance, int *tri, mpsr_stream_t stream)
{
    const char *who = "scene_surface_resolve";
    bool empty;
    int st = check_surface_sizes(who, n_frames, total_pixels, n_boxes, map_h, map_w, &empty);
    if (st) return st;
    if (empty || total_pixels == 0) return MPSR_OK;
    return resolve(who, box_frame, box_frame_host, n_frames, total_pixels, n_boxes,
                   (unsigned)tris_per_box(map_h, map_w), workspace, workspace_bytes,
                   SurfaceLayout(n_frames, total_pixels, n_boxes, map_h, map_w), depth, instance, tri, stream);
}

extern "C" int mpsr_scene_surface_score(const int *box_frame, const int *box_frame_host, const int *box_gt_id,
                                        const float *const *gt_depth, const unsigned char *const *gt_instance,
                                        const int *frame_hw, const long long *pixel_offset, int n_frames,
                                        long long total_pixels, int n_boxes, int map_h, int map_w,
                                        const void *workspace, size_t workspace_bytes, void *scratch,
                                        size_t scratch_bytes, int *counts, double *sums, mpsr_stream_t stream)
{
    const char *who = "scene_surface_score";
    bool empty;
    int st = check_surface_sizes(who, n_frames, total_pixels, n_boxes, map_h, map_w, &empty);
    if (st) return st;
    if (empty || total_pixels == 0) return MPSR_OK;
    MPSR_REQUIRE(box_frame && box_frame_host && frame_hw && pixel_offset,
                 "%s: box_frame, frame_hw or pixel_offset is null", who);
    // without ground truth (all three null): tris and pred_px alone, every other count and sum 0, no scratch
    const bool with_gt = box_gt_id || gt_depth || gt_instance;
    MPSR_REQUIRE(!with_gt || (box_gt_id && gt_depth && gt_instance),
                 "%s: box_gt_id or a ground-truth table is null (all three, or none)", who);
    MPSR_REQUIRE(counts && sums, "%s: an output is null", who);
    st = check_box_frames(who, box_frame_host, n_boxes, n_frames, 0);
    if (st) return st;
    const SurfaceLayout L(n_frames, total_pixels, n_boxes, map_h, map_w);
    st = check_workspace(who, workspace, workspace_bytes, L.total);
    if (st) return st;
    hipStream_t s = mpsr::as_stream(stream);
    if (with_gt) {
        st = launch_hist(who, gt_instance, pixel_offset, n_frames, total_pixels, scratch, scratch_bytes, s);
        if (st) return st;
    }
    const char *ws = static_cast<const char *>(workspace);
    hipLaunchKernelGGL(surface_score_kernel, dim3(n_boxes), dim3(kThreads), 0, s,
                       reinterpret_cast<const unsigned long long *>(ws + L.keys),
                       reinterpret_cast<const int *>(ws + L.box_tris), reinterpret_cast<const int *>(ws + L.box_rect),
                       box_frame, box_gt_id, gt_depth, gt_instance, frame_hw, pixel_offset,
                       static_cast<const int *>(scratch), (unsigned)tris_per_box(map_h, map_w), counts, sums);
    MPSR_CHECK_LAUNCH(who);
    return MPSR_OK;
}

// ---- Meshes: the drawn triangles of the surfaces as indexed, coloured faces.  Runs after
// mpsr_scene_surface_render on the same inputs, reads its vertex table and keys, and has a workspace of its own.
// mesh_win_kernel, one thread per pixel, flags the triangle that won it (a byte per triangle; equal values race
// benignly); mesh_select_kernel, one thread per triangle, asks triangle_drawn and, with visible_only, the flag.  A map
// point is a vertex when one of its (up to six) triangles is selected: every point GATHERS over its own triangles.
// mesh_count_kernel, one workgroup per box, counts vertices and faces and sums the area (block_tally); scan_kernel
// gives the offsets of both streams; mesh_vertex_kernel and mesh_face_kernel, one workgroup per box each, write at
// ranks from wave ballots as write_kernel does.  No atomics at all: two calls return the same bytes.

namespace {

// the triangles of a box that have map point (i, j) as a corner, in increasing id; -1 where the cell is outside the map
__device__ __forceinline__ void incident_triangles(int i, int j, int cells_h, int cells_w, long long *n)
{
    auto cell = [&](int ci, int cj) -> long long {
        return ci >= 0 && ci < cells_h && cj >= 0 && cj < cells_w ? 2 * ((long long)ci * cells_w + cj) : -1;
    };
    const long long c00 = cell(i - 1, j - 1), c01 = cell(i - 1, j), c10 = cell(i, j - 1), c11 = cell(i, j);
    n[0] = c00 < 0 ? -1 : c00 + 1;  // its v11
    n[1] = c01;                     // its v10, twice
    n[2] = c01 < 0 ? -1 : c01 + 1;
    n[3] = c10;                     // its v01, twice
    n[4] = c10 < 0 ? -1 : c10 + 1;
    n[5] = c11;                     // its v00
}

__device__ __forceinline__ bool point_used(const unsigned char *sel, int p, int map_w, int cells_h, int cells_w)
{
    long long n[6];
    incident_triangles(p / map_w, p % map_w, cells_h, cells_w, n);
    bool used = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) used = used || (n[k] >= 0 && sel[n[k]] != 0);
    return used;
}

// o = (c - a) x (b - a) of triangle n of the box whose points start at q, fp64 from the float32 coordinates
__device__ __forceinline__ void face_cross(const float *q, long long n, int cells_w, int map_w, double *o)
{
    long long ia, ib, ic;
    triangle_corners(n, cells_w, map_w, &ia, &ib, &ic);
    const float *a = q + 3 * ia, *b = q + 3 * ib, *c = q + 3 * ic;
    const double ux = (double)c[0] - (double)a[0], uy = (double)c[1] - (double)a[1], uz = (double)c[2] - (double)a[2];
    const double vx = (double)b[0] - (double)a[0], vy = (double)b[1] - (double)a[1], vz = (double)b[2] - (double)a[2];
    o[0] = uy * vz - uz * vy;
    o[1] = uz * vx - ux * vz;
    o[2] = ux * vy - uy * vx;
}

__device__ __forceinline__ double length3(const double *o) { return sqrt((o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]); }

__global__ void __launch_bounds__(kThreads) mesh_win_kernel(const unsigned long long *__restrict__ keys,
                                                            long long total_pixels, long long n_tris,
                                                            unsigned char *__restrict__ sel)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total_pixels;
         i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        if (key != kEmptyKey && (long long)(unsigned)key < n_tris) sel[(unsigned)key] = 1;
    }
}

// sel[t] = is triangle t in the mesh; with visible_only sel comes in as mesh_win_kernel's flags
__global__ void __launch_bounds__(kThreads) mesh_select_kernel(const float *__restrict__ xyz,
                                                               const int2 *__restrict__ vert, long long n_tris,
                                                               int map_h, int map_w, float max_edge_dz,
                                                               int max_span_px, int visible_only, unsigned char *sel)
{
    const int cells_w = map_w - 1;
    const long long points_per_box = (long long)map_h * map_w, per_box = 2LL * (map_h - 1) * cells_w;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_tris;
         t += (long long)gridDim.x * blockDim.x) {
        const long long b = t / per_box, i0 = b * points_per_box;
        long long ia, ib, ic, A;
        triangle_corners(t - b * per_box, cells_w, map_w, &ia, &ib, &ic);
        int2 p[3];
        float z[3];
        int ext[4];
        bool in = triangle_drawn(xyz, vert, i0 + ia, i0 + ib, i0 + ic, max_edge_dz, max_span_px, p, z, &A, ext);
        if (visible_only) in = in && sel[t] != 0;
        sel[t] = in ? 1 : 0;
    }
}

// one workgroup per box: vertices[b], faces[b] and area[b] = the sum of 0.5 |(c - a) x (b - a)| over its faces, thread
// n % 256 adding triangle n in slice order, then block_tally
__global__ void __launch_bounds__(kThreads) mesh_count_kernel(const float *__restrict__ xyz,
                                                              const unsigned char *__restrict__ sel, int map_h,
                                                              int map_w, int *__restrict__ vertices,
                                                              int *__restrict__ faces, double *__restrict__ area)
{
    const int b = blockIdx.x, cells_h = map_h - 1, cells_w = map_w - 1;
    const int points_per_box = map_h * map_w;
    const long long per_box = 2LL * cells_h * cells_w;
    const unsigned char *bsel = sel + b * per_box;
    const float *q = xyz + 3 * (long long)b * points_per_box;
    int n[2] = {0, 0};  // vertices, faces
    double s[1] = {0.0};
    for (int p0 = 0; p0 < points_per_box; p0 += kThreads) {
        const int p = p0 + threadIdx.x;
        n[0] += __popcll(__ballot(p < points_per_box && point_used(bsel, p, map_w, cells_h, cells_w)));
    }
    for (long long t0 = 0; t0 < per_box; t0 += kThreads) {
        const long long t = t0 + threadIdx.x;
        const bool take = t < per_box && bsel[t] != 0;
        if (take) {
            double o[3];
            face_cross(q, t, cells_w, map_w, o);
            s[0] += 0.5 * length3(o);
        }
        n[1] += __popcll(__ballot(take));
    }
    block_tally<2, 1>(n, s);
    if (threadIdx.x == 0) {
        vertices[b] = n[0];
        faces[b] = n[1];
        area[b] = s[0];
    }
}

// one workgroup per box: its vertices, in map-point order, to box_offset[b] + rank; rank[point] = the vertex's rank
// within its FRAME (-1: no vertex), which the faces index
__global__ void __launch_bounds__(kThreads) mesh_vertex_kernel(const float *__restrict__ xyz_in,
                                                               const unsigned char *__restrict__ sel,
                                                               const int *__restrict__ box_frame,
                                                               const double *__restrict__ cam_p,
                                                               const int *__restrict__ frame_hw,
                                                               const float *const *__restrict__ images,
                                                               const long long *__restrict__ box_offset,
                                                               const long long *__restrict__ frame_offset, int map_h,
                                                               int map_w, int *__restrict__ rank,
                                                               float *__restrict__ xyz, float *__restrict__ rgb,
                                                               float *__restrict__ normal, int *__restrict__ box)
{
    __shared__ int wave_n[kWaves];
    const int b = blockIdx.x, f = box_frame[b], cells_h = map_h - 1, cells_w = map_w - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int points_per_box = map_h * map_w;
    const unsigned char *bsel = sel + b * (2LL * cells_h * cells_w);
    const long long i0 = (long long)b * points_per_box;
    const float *q0 = xyz_in + 3 * i0;
    const float *image = images ? images[f] : nullptr;
    const int h = frame_hw[2 * f], w = frame_hw[2 * f + 1];
    const long long in_frame = frame_offset[f];
    long long base = box_offset[b];
    for (int p0 = 0; p0 < points_per_box; p0 += kThreads) {
        const int p = p0 + threadIdx.x;
        long long n[6];
        bool on[6];
        bool take = false;
        if (p < points_per_box) {
            incident_triangles(p / map_w, p % map_w, cells_h, cells_w, n);
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                on[k] = n[k] >= 0 && bsel[n[k]] != 0;
                take = take || on[k];
            }
        }
        const unsigned long long mask = __ballot(take);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < kWaves; ++v) {
            before += v < wave ? wave_n[v] : 0;
            all += wave_n[v];
        }
        if (take) {
            const long long o = base + before + __popcll(mask & ((1ULL << lane) - 1ULL));
            rank[i0 + p] = (int)(o - in_frame);
            const float *q = q0 + 3 * (long long)p;
            xyz[3 * o] = q[0];
            xyz[3 * o + 1] = q[1];
            xyz[3 * o + 2] = q[2];
            // the colour: the image at the point's pixel, mpsr_scene_project's; 0 outside the frame
            float c[3] = {0.0f, 0.0f, 0.0f};
            if (image) {
                double u[3];
                rows3(cam_p + 12 * f, (double)q[0], (double)q[1], (double)q[2], u);
                const double col = rint(u[0] / u[2]), row = rint(u[1] / u[2]);
                if (u[2] > 0.0 && col >= 0.0 && col < (double)w && row >= 0.0 && row < (double)h) {
                    const float *px = image + 3 * ((long long)(int)row * w + (int)col);
                    c[0] = px[0], c[1] = px[1], c[2] = px[2];
                }
            }
            rgb[3 * o] = c[0];
            rgb[3 * o + 1] = c[1];
            rgb[3 * o + 2] = c[2];
            // the normal: the faces' cross products added in increasing triangle id
            double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (on[k]) {
                    double e[3];
                    face_cross(q0, n[k], cells_w, map_w, e);
                    s[0] += e[0];
                    s[1] += e[1];
                    s[2] += e[2];
                }
            const double len = length3(s);
            const bool unit = len > 0.0 && isfinite(len);  // (NaN fails the comparison)
            normal[3 * o] = unit ? (float)(s[0] / len) : 0.0f;
            normal[3 * o + 1] = unit ? (float)(s[1] / len) : 0.0f;
            normal[3 * o + 2] = unit ? (float)(s[2] / len) : 0.0f;
            box[o] = b;
        } else if (p < points_per_box) {
            rank[i0 + p] = -1;
        }
        base += all;
        __syncthreads();  // wave_n is rewritten by the next slice
    }
}

// one workgroup per box: its faces, in triangle-id order, to box_offset[b] + rank, as (a, c, b) of the vertices' ranks
__global__ void __launch_bounds__(kThreads) mesh_face_kernel(const unsigned char *__restrict__ sel,
                                                             const int *__restrict__ rank,
                                                             const long long *__restrict__ box_offset, int map_h,
                                                             int map_w, int *__restrict__ faces,
                                                             int *__restrict__ face_box)
{
    __shared__ int wave_n[kWaves];
    const int b = blockIdx.x, cells_w = map_w - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long per_box = 2LL * (map_h - 1) * cells_w;
    const unsigned char *bsel = sel + b * per_box;
    const int *brank = rank + (long long)b * map_h * map_w;
    long long base = box_offset[b];
    for (long long t0 = 0; t0 < per_box; t0 += kThreads) {
        const long long t = t0 + threadIdx.x;
        const bool take = t < per_box && bsel[t] != 0;
        const unsigned long long mask = __ballot(take);
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, all = 0;
        for (int v = 0; v < kWaves; ++v) {
            before += v < wave ? wave_n[v] : 0;
            all += wave_n[v];
        }
        if (take) {
            const long long o = base + before + __popcll(mask & ((1ULL << lane) - 1ULL));
            long long ia, ib, ic;
            triangle_corners(t, cells_w, map_w, &ia, &ib, &ic);
            faces[3 * o] = brank[ia];
            faces[3 * o + 1] = brank[ic];
            faces[3 * o + 2] = brank[ib];
            face_box[o] = b;
        }
        base += all;
        __syncthreads();  // wave_n is rewritten by the next slice
    }
}

// the mesh's workspace: [sel: one byte per triangle] [rank: one int per map point] [vertices, faces: n_boxes ints each]
struct MeshLayout : Regions {
    size_t sel, rank, vertices, faces;

    MeshLayout(int n_boxes, int map_h, int map_w)
    {
        sel = take((size_t)n_boxes * tris_per_box(map_h, map_w));
        rank = take((size_t)n_boxes * map_h * map_w * sizeof(int));
        vertices = take((size_t)n_boxes * sizeof(int));
        faces = take((size_t)n_boxes * sizeof(int));
    }
};

}  // namespace

extern "C" size_t mpsr_scene_surface_mesh_workspace_bytes(int n_boxes, int map_h, int map_w)
{
    if (n_boxes <= 0 || map_h < 2 || map_w < 2 || (long long)n_boxes * map_h * map_w > INT_MAX) return 0;
    if (n_boxes * tris_per_box(map_h, map_w) >= (1LL << 32)) return 0;
    return MeshLayout(n_boxes, map_h, map_w).total;
}

extern "C" int mpsr_scene_surface_mesh(const float *xyz_global, const int *box_frame, const int *box_frame_host,
                                       const double *cam_p, const int *frame_hw, const int *frame_hw_host,
                                       const long long *pixel_offset, const long long *pixel_offset_host,
                                       const float *const *images, int n_frames, int n_boxes, int map_h, int map_w,
                                       float max_edge_dz, int max_span_px, int visible_only,
                                       const void *render_workspace, size_t render_workspace_bytes,
                                       void *mesh_workspace, size_t mesh_workspace_bytes, float *xyz, float *rgb,
                                       float *normal, int *vertex_box, int *faces, int *face_box,
                                       double *area_per_box, long long *vertex_box_offset,
                                       long long *vertex_frame_offset, long long *face_box_offset,
                                       long long *face_frame_offset, mpsr_stream_t stream)
{
    const char *who = "scene_surface_mesh";
    bool empty;
    int st = check_surface_sizes(who, n_frames, 0, n_boxes, map_h, map_w, &empty);
    if (st) return st;
    MPSR_REQUIRE(max_span_px >= 1 && max_span_px <= kMaxSpan, "%s: max_span_px %d is outside 1..%d", who, max_span_px,
                 kMaxSpan);
    MPSR_REQUIRE(max_edge_dz > 0.0f, "%s: max_edge_dz %g must be greater than 0 (+inf: no limit)", who,
                 (double)max_edge_dz);  // NaN fails the comparison
    hipStream_t s = mpsr::as_stream(stream);
    if (empty) {  // no vertex and no face: zeroed offsets are all there is to write (a null table is left alone)
        long long *const tables[4] = {vertex_box_offset, face_box_offset, vertex_frame_offset, face_frame_offset};
        for (int k = 0; k < 4; ++k) {
            const size_t rows = (size_t)(k < 2 ? n_boxes : n_frames) + 1;
            if (tables[k]) MPSR_CHECK_HIP(hipMemsetAsync(tables[k], 0, rows * sizeof(long long), s));
        }
        return MPSR_OK;
    }
    MPSR_REQUIRE((long long)n_boxes * map_h * map_w <= INT_MAX,
                 "%s: %d boxes of %d x %d points: a vertex index does not fit 31 bits", who, n_boxes, map_h, map_w);
    long long total_pixels;
    st = check_render_args(who, xyz_global, box_frame, box_frame_host, cam_p, frame_hw, frame_hw_host, pixel_offset,
                           pixel_offset_host, n_frames, n_boxes, &total_pixels);
    if (st) return st;
    MPSR_REQUIRE(xyz && rgb && normal && vertex_box && faces && face_box && area_per_box, "%s: an output is null", who);
    MPSR_REQUIRE(vertex_box_offset && vertex_frame_offset && face_box_offset && face_frame_offset,
                 "%s: an offset table is null", who);
    const SurfaceLayout R(n_frames, total_pixels, n_boxes, map_h, map_w);
    st = check_workspace(who, render_workspace, render_workspace_bytes, R.total);
    if (st) return st;
    const MeshLayout L(n_boxes, map_h, map_w);
    st = check_workspace(who, mesh_workspace, mesh_workspace_bytes, L.total);
    if (st) return st;
    const char *rws = static_cast<const char *>(render_workspace);
    const unsigned long long *keys = reinterpret_cast<const unsigned long long *>(rws + R.keys);
    const int2 *vert = reinterpret_cast<const int2 *>(rws + R.vert);
    char *ws = static_cast<char *>(mesh_workspace);
    unsigned char *sel = reinterpret_cast<unsigned char *>(ws + L.sel);
    int *rank = reinterpret_cast<int *>(ws + L.rank);
    int *n_vertices = reinterpret_cast<int *>(ws + L.vertices), *n_faces = reinterpret_cast<int *>(ws + L.faces);
    const long long n_tris = n_boxes * tris_per_box(map_h, map_w);
    if (visible_only) {
        MPSR_CHECK_HIP(hipMemsetAsync(sel, 0, (size_t)n_tris, s));
        hipLaunchKernelGGL(mesh_win_kernel, dim3(grid_for(total_pixels)), dim3(kThreads), 0, s, keys, total_pixels,
                           n_tris, sel);
    }
    hipLaunchKernelGGL(mesh_select_kernel, dim3(grid_for(n_tris)), dim3(kThreads), 0, s, xyz_global, vert, n_tris,
                       map_h, map_w, max_edge_dz, max_span_px, visible_only, sel);
    hipLaunchKernelGGL(mesh_count_kernel, dim3(n_boxes), dim3(kThreads), 0, s, xyz_global, sel, map_h, map_w,
                       n_vertices, n_faces, area_per_box);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, s, n_vertices, n_boxes, box_frame, n_frames,
                       vertex_box_offset, vertex_frame_offset);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, s, n_faces, n_boxes, box_frame, n_frames,
                       face_box_offset, face_frame_offset);
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(n_boxes), dim3(kThreads), 0, s, xyz_global, sel, box_frame, cam_p,
                       frame_hw, images, vertex_box_offset, vertex_frame_offset, map_h, map_w, rank, xyz, rgb, normal,
                       vertex_box);
    hipLaunchKernelGGL(mesh_face_kernel, dim3(n_boxes), dim3(kThreads), 0, s, sel, rank, face_box_offset, map_h,
                       map_w, faces, face_box);
    MPSR_CHECK_LAUNCH(who);
    return MPSR_OK;
}

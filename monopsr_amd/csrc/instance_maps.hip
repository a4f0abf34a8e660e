// Training ground truth from depth maps: the instance images of demos/instances/gen_instance_masks.py:86-153 and the
// per-box crops of instance_utils.tf_instance_xyz_crop_from_depth_map (instance_utils.py:395-481), for batches of frames
// that share one image size.
//
// mpsr_instance_images: one thread per pixel; the frame's per-box constants (built on the host in the reference's
//   operation order) sit in LDS.  The pixel's point and its projection are computed once in fp64, then the boxes are
//   tested from the last to the first and the first hit wins (the reference's later box overwrites an earlier one).
// mpsr_instance_xyz_crops: one thread per (box, output pixel) gathers the nearest-neighbour source pixel of the
//   rounded crop, masks it by the box's instance id and writes the local map, the global map and the valid mask.
// Built with -ffp-contract=off: every product and sum is rounded as tests/instance_restatement.py rounds it.
#include "common.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kStride = MPSR_INSTANCE_BOX_STRIDE;

__global__ void __launch_bounds__(kThreads) instance_image_kernel(const float *__restrict__ depth,
                                                                  const double *__restrict__ p2,
                                                                  const double *__restrict__ boxes,
                                                                  const long long *__restrict__ box_offsets, int h,
                                                                  int w, unsigned char *__restrict__ out)
{
    __shared__ double table[MPSR_INSTANCE_MAX_BOXES * kStride];
    const int f = blockIdx.y;
    const long long b0 = box_offsets[f];
    const int nb = (int)(box_offsets[f + 1] - b0);
    for (int i = threadIdx.x; i < nb * kStride; i += blockDim.x) table[i] = boxes[b0 * kStride + i];
    __syncthreads();
    const long long npix = (long long)h * w;
    const long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const int v = (int)(pix / w), u = (int)(pix - (long long)v * w);
    const double *P = p2 + 12 * f;
    const float d = depth[f * npix + pix];
    // get_depth_point_cloud: ratio = d / f in float32 (numpy 1), then fp64, then the point rounded to float32
    const double ratio = (double)(d / (float)P[0]);
    const double x_offset = -P[3] / P[0];
    const double px = (double)(float)(((double)u - P[2]) * ratio + x_offset);
    const double py = (double)(float)(((double)v - P[6]) * ratio);
    const double pz = (double)d;
    double r[3];
    for (int k = 0; k < 3; ++k) r[k] = ((P[4 * k] * px + P[4 * k + 1] * py) + P[4 * k + 2] * pz) + P[4 * k + 3];
    const double pu = r[0] / r[2], pv = r[1] / r[2];
    int id = 255;
    for (int k = nb - 1; k >= 0; --k) {
        const double *t = table + k * kStride;
        bool in = true;
        for (int a = 0; a < 3 && in; ++a) {
            const double *ax = t + 5 * a;
            const double dot = (px * ax[0] + py * ax[1]) + pz * ax[2];
            in = dot <= ax[3] && dot >= ax[4];
        }
        if (in && pu >= t[16] && pu <= t[18] && pv >= t[15] && pv <= t[17]) {
            id = k;
            break;
        }
    }
    out[f * npix + pix] = (unsigned char)id;
}

// resize_nearest_neighbor(align_corners=True), TF 1.8: float32 scale, roundf (halves away from zero)
__device__ __forceinline__ int nn_source(int i, int in, int out)
{
    const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : (float)in / (float)out;
    const long long s = (long long)roundf((float)i * scale);
    return (int)(s < in - 1 ? s : in - 1);
}

// tf.linspace (TF's LinSpace kernel: start + step * i, the last element NOT forced to stop)
__device__ __forceinline__ float linspace_at(float start, float stop, int num, int i)
{
    if (num == 1) return start;
    const float step = (stop - start) / (float)(num - 1);
    return start + step * (float)i;
}

// kDeviceChecks: the argument checks mpsr_instance_xyz_crops makes on host copies are made here, per box, on the device
// arrays; a box that fails them is written as zeros, reads no image, and is reported in status[0] (the OR of the
// MPSR_CROP_BAD_* bits) and status[1] (the number of such boxes).
template <bool kDeviceChecks>
__global__ void __launch_bounds__(kThreads) instance_crop_kernel(
    const float *__restrict__ depth, const unsigned char *__restrict__ inst, const float *__restrict__ p2, int h,
    int w, const int *__restrict__ frame_index, const int *__restrict__ instance_id,
    const float *__restrict__ boxes_2d, const float *__restrict__ boxes_3d, const float *__restrict__ view_angs,
    int n_boxes, int roi, int middle, int rotate_view, float *__restrict__ xyz_local, float *__restrict__ xyz_global,
    float *__restrict__ valid, int n_frames, int *__restrict__ status)
{
    const long long per_box = (long long)roi * roi;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= per_box * n_boxes) return;
    const int b = (int)(idx / per_box);
    const int rem = (int)(idx - (long long)b * per_box);
    const int i = rem / roi, j = rem - i * roi;
    const int f = frame_index[b];
    const float y1 = boxes_2d[4 * b], x1 = boxes_2d[4 * b + 1], y2 = boxes_2d[4 * b + 2], x2 = boxes_2d[4 * b + 3];
    if (kDeviceChecks) {
        int bad = 0;
        if (f < 0 || f >= n_frames) bad |= MPSR_CROP_BAD_FRAME;
        if (instance_id[b] < 0 || instance_id[b] > 254) bad |= MPSR_CROP_BAD_ID;
        if (!(isfinite(y1) && isfinite(x1) && isfinite(y2) && isfinite(x2))) {
            bad |= MPSR_CROP_BAD_NOT_FINITE;
        } else {
            const float fr0 = rintf(y1), fc0 = rintf(x1), fr2 = rintf(y2), fc2 = rintf(x2);
            if (!(fr0 >= 0.0f && fc0 >= 0.0f && fr2 <= (float)h && fc2 <= (float)w && fr0 < fr2 && fc0 < fc2))
                bad |= MPSR_CROP_BAD_BOX;
        }
        if (bad) {
            if (rem == 0) {
                atomicOr(status, bad);
                atomicAdd(status + 1, 1);
            }
            for (int k = 0; k < 3; ++k) xyz_local[3 * idx + k] = xyz_global[3 * idx + k] = 0.0f;
            valid[idx] = 0.0f;
            return;
        }
    }
    const int r0 = (int)rintf(y1), c0 = (int)rintf(x1), r2 = (int)rintf(y2), c2 = (int)rintf(x2);
    const int sy = r0 + nn_source(i, r2 - r0, roi), sx = c0 + nn_source(j, c2 - c0, roi);
    const long long src = (long long)f * h * w + (long long)sy * w + sx;
    const float d = depth[src] * (inst[src] == instance_id[b] ? 1.0f : 0.0f);
    const float *P = p2 + 12 * f;
    // tf_depth_patch_to_pc_map with pixel centres of the UNROUNDED box
    const float pw = (x2 - x1) / (float)roi, ph = (y2 - y1) / (float)roi;
    const float hw = pw / 2.0f, hh = ph / 2.0f;
    const float xx = linspace_at(x1 + hw, x2 - hw, roi, j), yy = linspace_at(y1 + hh, y2 - hh, roi, i);
    const float ratio = d / P[0];
    const float x = (xx - P[2]) * ratio, y = (yy - P[6]) * ratio, z = d;
    const float m = fabsf(d) >= 0.1f ? 1.0f : 0.0f;
    float *g = xyz_global + 3 * idx, *l = xyz_local + 3 * idx;
    g[0] = x * m;
    g[1] = y * m;
    g[2] = z * m;
    valid[idx] = m;
    // local frame: rot_y(-view_ang) . translate(-centroid) (transform_utils.tf_get_tr_mat), the centroid in camera N
    const float *b3 = boxes_3d + 7 * b;
    const float x_offset = -P[3] / P[0];
    const float tx = -(b3[0] - x_offset);
    const float ty = -(middle ? b3[1] - b3[5] / 2.0f : b3[1]);
    const float tz = -b3[2];
    float lx, ly, lz;
    if (rotate_view) {
        // cos / sin in fp64, rounded once: float32 values within an ulp of TF's float32 cos / sin
        const double a = -(double)view_angs[b];
        const float c = (float)cos(a), s = (float)sin(a);
        const float t0 = c * tx + s * tz, t2 = -s * tx + c * tz;
        lx = (c * x + s * z) + t0;
        ly = y + ty;
        lz = (-s * x + c * z) + t2;
    } else {
        lx = x + tx;
        ly = y + ty;
        lz = z + tz;
    }
    l[0] = lx * m;
    l[1] = ly * m;
    l[2] = lz * m;
}

}  // namespace

extern "C" int mpsr_instance_images(const float *depth, int n_frames, int h, int w, const double *p2,
                                    const double *boxes, const long long *box_offsets,
                                    const long long *box_offsets_host, unsigned char *out, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_frames >= 0 && n_frames <= 65535, "instance_images: n_frames %d (0..65535)", n_frames);
    MPSR_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "instance_images: bad image size %d x %d", h, w);
    if (n_frames == 0) return MPSR_OK;
    MPSR_REQUIRE(depth && p2 && out && box_offsets && box_offsets_host, "instance_images: a pointer is null");
    MPSR_REQUIRE(box_offsets_host[0] == 0, "instance_images: box_offsets[0] = %lld, expected 0", box_offsets_host[0]);
    for (int f = 0; f < n_frames; ++f) {
        const long long n = box_offsets_host[f + 1] - box_offsets_host[f];
        MPSR_REQUIRE(n >= 0 && n <= MPSR_INSTANCE_MAX_BOXES,
                     "instance_images: frame %d has %lld boxes (0..%d: id 255 is the background)", f, n,
                     MPSR_INSTANCE_MAX_BOXES);
    }
    MPSR_REQUIRE(box_offsets_host[n_frames] == 0 || boxes, "instance_images: boxes is null");
    hipStream_t s = mpsr::as_stream(stream);
    const long long npix = (long long)h * w;
    dim3 grid((unsigned)((npix + kThreads - 1) / kThreads), (unsigned)n_frames);
    instance_image_kernel<<<grid, kThreads, 0, s>>>(depth, p2, boxes, box_offsets, h, w, out);
    MPSR_CHECK_LAUNCH("instance_image_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_instance_xyz_crops(const float *depth, const unsigned char *inst, const float *p2, int n_frames,
                                       int h, int w, const int *frame_index, const int *instance_id,
                                       const float *boxes_2d, const float *boxes_3d, const float *view_angs,
                                       const int *frame_index_host, const int *instance_id_host,
                                       const float *boxes_2d_host, int n_boxes, int roi_h, int roi_w,
                                       int centroid_type, int rotate_view, float *xyz_local, float *xyz_global,
                                       float *valid, mpsr_stream_t stream)
{
    MPSR_REQUIRE(roi_h == roi_w, "instance_crops: the ROI must be square (the reference's graph only builds for "
                                 "square ROIs), got %d x %d", roi_h, roi_w);
    MPSR_REQUIRE(roi_h >= 1 && roi_h <= 1024, "instance_crops: roi %d (1..1024)", roi_h);
    MPSR_REQUIRE(n_boxes >= 0 && n_frames >= 0, "instance_crops: n_boxes %d, n_frames %d", n_boxes, n_frames);
    MPSR_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "instance_crops: bad image size %d x %d", h, w);
    MPSR_REQUIRE(centroid_type == MPSR_CENTROID_BOTTOM || centroid_type == MPSR_CENTROID_MIDDLE,
                 "instance_crops: unknown centroid_type %d", centroid_type);
    if (n_boxes == 0) return MPSR_OK;
    MPSR_REQUIRE((long long)n_boxes * roi_h * roi_h <= INT_MAX, "instance_crops: %d boxes of %d x %d is too many",
                 n_boxes, roi_h, roi_h);
    MPSR_REQUIRE(depth && inst && p2 && frame_index && instance_id && boxes_2d && boxes_3d && view_angs && xyz_local &&
                     xyz_global && valid && frame_index_host && instance_id_host && boxes_2d_host,
                 "instance_crops: a pointer is null");
    for (int b = 0; b < n_boxes; ++b) {
        const int f = frame_index_host[b], id = instance_id_host[b];
        MPSR_REQUIRE(f >= 0 && f < n_frames, "instance_crops: box %d: frame %d not in [0, %d)", b, f, n_frames);
        MPSR_REQUIRE(id >= 0 && id <= 254, "instance_crops: box %d: instance id %d not in [0, 254]", b, id);
        const float *bx = boxes_2d_host + 4 * b;
        MPSR_REQUIRE(std::isfinite(bx[0]) && std::isfinite(bx[1]) && std::isfinite(bx[2]) && std::isfinite(bx[3]),
                     "instance_crops: box %d is not finite", b);
        const float r0 = rintf(bx[0]), c0 = rintf(bx[1]), r2 = rintf(bx[2]), c2 = rintf(bx[3]);
        MPSR_REQUIRE(r0 >= 0.0f && c0 >= 0.0f && r2 <= (float)h && c2 <= (float)w && r0 < r2 && c0 < c2,
                     "instance_crops: box %d rounds to rows [%g, %g) x columns [%g, %g): empty or outside the %d x %d "
                     "image", b, r0, r2, c0, c2, h, w);
    }
    hipStream_t s = mpsr::as_stream(stream);
    const long long total = (long long)n_boxes * roi_h * roi_h;
    instance_crop_kernel<false><<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        depth, inst, p2, h, w, frame_index, instance_id, boxes_2d, boxes_3d, view_angs, n_boxes, roi_h,
        centroid_type == MPSR_CENTROID_MIDDLE, rotate_view != 0, xyz_local, xyz_global, valid, n_frames, nullptr);
    MPSR_CHECK_LAUNCH("instance_crop_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_instance_xyz_crops_status(const float *depth, const unsigned char *inst, const float *p2,
                                              int n_frames, int h, int w, const int *frame_index,
                                              const int *instance_id, const float *boxes_2d, const float *boxes_3d,
                                              const float *view_angs, int n_boxes, int roi_h, int roi_w,
                                              int centroid_type, int rotate_view, float *xyz_local, float *xyz_global,
                                              float *valid, int *status, mpsr_stream_t stream)
{
    MPSR_REQUIRE(roi_h == roi_w, "instance_crops: the ROI must be square (the reference's graph only builds for "
                                 "square ROIs), got %d x %d", roi_h, roi_w);
    MPSR_REQUIRE(roi_h >= 1 && roi_h <= 1024, "instance_crops: roi %d (1..1024)", roi_h);
    MPSR_REQUIRE(n_boxes >= 0 && n_frames >= 0, "instance_crops: n_boxes %d, n_frames %d", n_boxes, n_frames);
    MPSR_REQUIRE(h > 0 && w > 0 && (long long)h * w <= (1LL << 30), "instance_crops: bad image size %d x %d", h, w);
    MPSR_REQUIRE(centroid_type == MPSR_CENTROID_BOTTOM || centroid_type == MPSR_CENTROID_MIDDLE,
                 "instance_crops: unknown centroid_type %d", centroid_type);
    if (n_boxes == 0) return MPSR_OK;
    MPSR_REQUIRE((long long)n_boxes * roi_h * roi_h <= INT_MAX, "instance_crops: %d boxes of %d x %d is too many",
                 n_boxes, roi_h, roi_h);
    MPSR_REQUIRE(depth && inst && p2 && frame_index && instance_id && boxes_2d && boxes_3d && view_angs && xyz_local &&
                     xyz_global && valid && status,
                 "instance_crops: a pointer is null");
    const long long total = (long long)n_boxes * roi_h * roi_h;
    instance_crop_kernel<true><<<(unsigned)((total + kThreads - 1) / kThreads), kThreads, 0, mpsr::as_stream(stream)>>>(
        depth, inst, p2, h, w, frame_index, instance_id, boxes_2d, boxes_3d, view_angs, n_boxes, roi_h,
        centroid_type == MPSR_CENTROID_MIDDLE, rotate_view != 0, xyz_local, xyz_global, valid, n_frames, status);
    MPSR_CHECK_LAUNCH("instance_crop_kernel");
    return MPSR_OK;
}

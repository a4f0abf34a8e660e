// Batch assembly of KITTI training samples on the device: the oversampling draw of kitti_dataset.py:301-308 and the 2-D
// box jitter of kitti_aug.jitter_obj_boxes_2d (kitti_aug.py:173-254), one lane per box slot.
//
// Random numbers are counter-based (Philox4x32-10): a slot's draws depend on (seed, epoch, frame, slot, draw) and on
// nothing else, so a frame's sample is the same in any batch, at any batch size and on any rank.
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (draw j, slot s, frame's index in the split file, (epoch << 4) | stream)   stream 0: oversampling, 1: jitter
//   uniform = ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53 from two words; a pair of normals by Box-Muller in fp64 from
//             (1 - u0, u1); one Philox call gives one pair.
// Built with -ffp-contract=off: every product and sum is rounded as tests/jitter_restatement.py rounds it.
//
// Image noise (kitti_aug.apply_image_noise, kitti_aug.py:124-170) of a batch's frames, fused with their gather and
// their conversion to float32: stream 2 holds a frame's own draws, stream 3 its per-element ones (mpsr_image_noise
// in include/monopsr_hip.h gives the counters; tests/image_noise_restatement.py restates the arithmetic).
#include "common.h"

#include <cmath>

namespace {

constexpr int kThreads = 64;
constexpr unsigned kStreamOversample = 0u, kStreamJitter = 1u, kStreamImageFrame = 2u, kStreamImageElement = 3u;

struct Words {
    unsigned w[4];
};

__device__ __forceinline__ Words philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                               unsigned k1)
{
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

__device__ __forceinline__ double uniform53(unsigned w0, unsigned w1)
{
    return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0;
}

// z0, z1 of draw j
__device__ __forceinline__ void normal_pair(unsigned j, unsigned s, unsigned i, unsigned e, unsigned k0, unsigned k1,
                                            double &z0, double &z1)
{
    const Words p = philox4x32_10(j, s, i, e, k0, k1);
    const double u0 = uniform53(p.w[0], p.w[1]), u1 = uniform53(p.w[2], p.w[3]);
    const double r = sqrt(-2.0 * log(1.0 - u0));
    const double a = 6.283185307179586 * u1;
    z0 = r * cos(a);
    z1 = r * sin(a);
}

// evaluation.two_d_iou (core/evaluation.py:23-61) of one pair
__device__ __forceinline__ double two_d_iou(double ax1, double ay1, double ax2, double ay2, double bx1, double by1,
                                            double bx2, double by2)
{
    const double w_int = fmin(ax2, bx2) - fmax(ax1, bx1);
    const double h_int = fmin(ay2, by2) - fmax(ay1, by1);
    if (!(w_int > 0.0 && h_int > 0.0)) return 0.0;
    const double inter = w_int * h_int;
    const double box_area = (ax2 - ax1) * (ay2 - ay1);
    const double boxes_area = (bx2 - bx1) * (by2 - by1);
    const double union_area = (box_area + boxes_area) - inter;
    return inter / union_area;
}

__global__ void __launch_bounds__(kThreads) sample_slots_kernel(
    const int *__restrict__ slot_frame, const int *__restrict__ slot_s, int n, const int *__restrict__ num_objs,
    const long long *__restrict__ label_offset, const int *__restrict__ split_index,
    const int *__restrict__ frame_local, const int *__restrict__ image_hw, const double *__restrict__ p00_p02,
    const double *__restrict__ label_boxes, int n_frames, unsigned k0, unsigned k1, unsigned epoch, int jitter_mode,
    long long *__restrict__ label_row, int *__restrict__ oversample_index, int *__restrict__ jitter_flag,
    double *__restrict__ boxes_xyxy, int *__restrict__ slot_hw, double *__restrict__ slot_p,
    int *__restrict__ slot_split_index, int *__restrict__ slot_frame_local)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int r = slot_frame[t], s = slot_s[t];
    // The caller guarantees both ranges (include/monopsr_hip.h); the arrays are on the device, so the entry point
    // cannot check them.  A value out of range is read as frame 0 / slot 0 so that no lane leaves the tables.
    if (r < 0 || r >= n_frames) r = 0;
    if (s < 0) s = 0;
    const int no = num_objs[r];
    const unsigned i = (unsigned)split_index[r];
    int idx = s;
    if (s >= no) {
        const Words p = philox4x32_10(0u, (unsigned)s, i, (epoch << 4) | kStreamOversample, k0, k1);
        idx = (int)floor(uniform53(p.w[0], p.w[1]) * (double)no);
        if (idx > no - 1) idx = no - 1;  // (u < 1, so u * no < no unless the product rounds up)
    }
    const long long row = label_offset[r] + idx;
    label_row[t] = row;
    oversample_index[t] = idx;
    jitter_flag[t] = jitter_mode == 2 || (jitter_mode == 1 && s >= no);
    for (int k = 0; k < 4; ++k) boxes_xyxy[4 * t + k] = label_boxes[4 * row + k];
    slot_hw[2 * t] = image_hw[2 * r];
    slot_hw[2 * t + 1] = image_hw[2 * r + 1];
    slot_p[2 * t] = p00_p02[2 * r];
    slot_p[2 * t + 1] = p00_p02[2 * r + 1];
    slot_split_index[t] = (int)i;
    slot_frame_local[t] = frame_local[r];
}

__global__ void __launch_bounds__(kThreads) jitter_boxes_kernel(
    const double *__restrict__ boxes_xyxy, const int *__restrict__ jitter_flag, const int *__restrict__ image_hw,
    const double *__restrict__ p00_p02, const int *__restrict__ frame_index, const int *__restrict__ slot, int n,
    unsigned k0, unsigned k1, unsigned epoch, double iou_threshold_min, int max_trials, int write_unjittered,
    double *__restrict__ out_xyxy, float *__restrict__ out_boxes_2d, float *__restrict__ out_norm,
    float *__restrict__ out_view, int *__restrict__ out_trials)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double x1 = boxes_xyxy[4 * t], y1 = boxes_xyxy[4 * t + 1], x2 = boxes_xyxy[4 * t + 2],
                 y2 = boxes_xyxy[4 * t + 3];
    const int img_h = image_hw[2 * t], img_w = image_hw[2 * t + 1];
    const double box_w = x2 - x1, box_h = y2 - y1;
    const double half_w = box_w / 2, half_h = box_h / 2;
    const double cx = (x2 + x1) / 2, cy = (y2 + y1) / 2;
    double nx1 = x1, ny1 = y1, nx2 = x2, ny2 = y2;
    int trials = 0;
    bool jittered = false;
    if (jitter_flag[t] && !(box_w < 10 || box_h < 10)) {
        const unsigned s = (unsigned)slot[t], i = (unsigned)frame_index[t], e = (epoch << 4) | kStreamJitter;
        const double sd_cx = half_w / 3, sd_cy = half_h / 3, sd_w = half_w / 6, sd_h = half_h / 6;
        const double x_max = (double)(img_w - 1), y_max = (double)(img_h - 1);
        while (trials < max_trials) {
            double za, zb, zc, zd;
            normal_pair(2u * (unsigned)trials, s, i, e, k0, k1, za, zb);
            normal_pair(2u * (unsigned)trials + 1u, s, i, e, k0, k1, zc, zd);
            ++trials;
            const double ncx = cx + sd_cx * za, ncy = cy + sd_cy * zb;
            const double nhw = half_w + sd_w * zc, nhh = half_h + sd_h * zd;
            const double tx1 = fmax(0.0, ncx - nhw), tx2 = fmin(x_max, ncx + nhw);
            const double ty1 = fmax(0.0, ncy - nhh), ty2 = fmin(y_max, ncy + nhh);
            if (two_d_iou(tx1, ty1, tx2, ty2, x1, y1, x2, y2) >= iou_threshold_min) {
                nx1 = tx1;
                ny1 = ty1;
                nx2 = tx2;
                ny2 = ty2;
                jittered = true;
                break;
            }
        }
        if (!jittered) trials = max_trials + 1;  // the cap: the label's box is kept
    }
    out_xyxy[4 * t] = nx1;
    out_xyxy[4 * t + 1] = ny1;
    out_xyxy[4 * t + 2] = nx2;
    out_xyxy[4 * t + 3] = ny2;
    out_trials[t] = trials;
    if (!jittered && !write_unjittered) return;  // the caller's rows stay as they are
    const float fy1 = (float)ny1, fx1 = (float)nx1, fy2 = (float)ny2, fx2 = (float)nx2;
    out_boxes_2d[4 * t] = fy1;
    out_boxes_2d[4 * t + 1] = fx1;
    out_boxes_2d[4 * t + 2] = fy2;
    out_boxes_2d[4 * t + 3] = fx2;
    out_norm[4 * t] = (float)((double)fy1 / (double)img_h);
    out_norm[4 * t + 1] = (float)((double)fx1 / (double)img_w);
    out_norm[4 * t + 2] = (float)((double)fy2 / (double)img_h);
    out_norm[4 * t + 3] = (float)((double)fx2 / (double)img_w);
    // get_viewing_angle_box_2d: np.mean of the two float32 columns, then fp64
    const float centre = (fx1 + fx2) / 2.0f;
    out_view[t] = (float)atan2(((double)centre - p00_p02[2 * t + 1]) / p00_p02[2 * t], 1.0);
}

// ---- image noise

constexpr int kNoiseThreads = 256;  // lanes of a block
constexpr int kNoiseQuads = 8;      // quads (4 consecutive elements) per lane: a wave makes the frame's own draws once
enum { kBitSwap = 0, kBitGaussian = 1, kBitChannel = 2, kBitBrightness = 3, kBitUniform = 4 };

// np.uint8(np.clip(value + noise, 0.0, 255.0)): fp64 sum, clip, truncation toward zero
__device__ __forceinline__ int add_clip_truncate(int value, double noise)
{
    return (int)fmin(fmax((double)value + noise, 0.0), 255.0);
}

// One block handles kNoiseThreads * kNoiseQuads quads of one gathered frame.  A quad starts at the frame's element
// 4 t - shift, shift = 0 or 2 chosen per frame so that the quad's 16 output bytes are aligned whenever the frame's
// output base is even (in elements); a quad therefore always covers two whole Philox pairs (2q, 2q + 1).  Quads that
// hang over either end of the frame, frames whose output base is odd, and frames that exchange channels go element by
// element.  Everything that selects a path is the same for all lanes of a frame.
__global__ void __launch_bounds__(kNoiseThreads) image_noise_kernel(
    const unsigned char *__restrict__ frames, int n_frames, int n, const int *__restrict__ gather,
    const int *__restrict__ frame_index, int blocks_per_frame, unsigned k0, unsigned k1, unsigned epoch, int mode,
    float *__restrict__ out, int *__restrict__ stages, double *__restrict__ params)
{
    const int k = (int)(blockIdx.x / (unsigned)blocks_per_frame);
    const int chunk = (int)(blockIdx.x - (unsigned)k * (unsigned)blocks_per_frame);
    int f = gather[k];
    // (as in sample_slots_kernel: the indices are on the device; one out of range is read as frame 0)
    if (f < 0 || f >= n_frames) f = 0;
    const unsigned i = (unsigned)frame_index[k];

    // the frame's own draws
    const unsigned ef = (epoch << 4) | kStreamImageFrame, ee = (epoch << 4) | kStreamImageElement;
    Words p = philox4x32_10(0u, 0u, i, ef, k0, k1);
    int fired = (uniform53(p.w[0], p.w[1]) < 0.10) << kBitSwap | (uniform53(p.w[2], p.w[3]) < 0.40) << kBitGaussian;
    p = philox4x32_10(1u, 0u, i, ef, k0, k1);
    fired |= (uniform53(p.w[0], p.w[1]) < 0.40) << kBitChannel | (uniform53(p.w[2], p.w[3]) < 0.40) << kBitBrightness;
    p = philox4x32_10(2u, 0u, i, ef, k0, k1);
    fired |= (uniform53(p.w[0], p.w[1]) < 0.40) << kBitUniform;
    const double amount = 10.0 * uniform53(p.w[2], p.w[3]);
    double ch_r = 0.0, ch_g = 0.0, ch_b = 0.0, brightness = 0.0;
    const bool reports = chunk == 0;
    if (reports || (fired & (1 << kBitChannel | 1 << kBitBrightness))) {
        double za, zb, zc, zd;
        normal_pair(3u, 0u, i, ef, k0, k1, za, zb);
        normal_pair(4u, 0u, i, ef, k0, k1, zc, zd);
        ch_r = za * 8.0;
        ch_g = zb * 8.0;
        ch_b = zc * 8.0;
        brightness = zd * 15.0;
    }
    if (reports && threadIdx.x == 0) {
        stages[k] = fired;
        params[5 * k] = amount;
        params[5 * k + 1] = ch_r;
        params[5 * k + 2] = ch_g;
        params[5 * k + 3] = ch_b;
        params[5 * k + 4] = brightness;
    }

    // the stages whose result is seen: in the reference's arithmetic the last noise stage alone (or none)
    const int noise_bits = fired >> 1;
    int first_stage = 1, last_stage = noise_bits ? 32 - __clz(noise_bits) : 0;
    if (mode == MPSR_IMAGE_NOISE_REFERENCE) first_stage = last_stage;
    // the exchange as a source offset per channel: G := B alone (what the tuple assignment on views does) or G <-> B
    int from_g = 0, from_b = 0;
    if (mode == MPSR_IMAGE_NOISE_REFERENCE) {
        if (fired == 1 << kBitSwap) from_g = 1;
    } else if (fired & (1 << kBitSwap)) {
        from_g = 1;
        from_b = -1;
    }
    const bool exchanges = from_g != 0;

    const long long in_base = (long long)f * n, out_base = (long long)k * n;
    const unsigned char *__restrict__ src = frames + in_base;
    float *__restrict__ dst = out + out_base;
    // (the pointers' own alignment counts too: a caller may pass a view that starts inside an allocation)
    const int out_mis = (int)(((long long)(reinterpret_cast<size_t>(out) >> 2) + out_base) & 3);
    const int shift = out_mis == 2 ? 2 : 0;
    const bool wide_store = !(out_mis & 1);
    const int in_mis = (int)(((long long)(reinterpret_cast<size_t>(frames) & 3) + in_base - shift) & 3);
    const long long n_quads = ((long long)n + shift + 3) >> 2;

    for (int u = 0; u < kNoiseQuads; ++u) {
        const long long t = ((long long)chunk * kNoiseQuads + u) * kNoiseThreads + threadIdx.x;
        if (t >= n_quads) break;
        const long long e0 = 4 * t - shift;  // even; -2 for the first quad of a shifted frame
        const bool whole = e0 >= 0 && e0 + 3 < n;
        const int c0 = (int)((e0 + 3) % 3);  // the channel of element e0
        int v[4] = {0, 0, 0, 0};
        if (whole && !exchanges) {
            if (in_mis == 0) {
                const unsigned x = *reinterpret_cast<const unsigned *>(src + e0);
                v[0] = x & 255u;
                v[1] = (x >> 8) & 255u;
                v[2] = (x >> 16) & 255u;
                v[3] = x >> 24;
            } else if (in_mis == 2) {
                const unsigned lo = *reinterpret_cast<const unsigned short *>(src + e0);
                const unsigned hi = *reinterpret_cast<const unsigned short *>(src + e0 + 2);
                v[0] = lo & 255u;
                v[1] = lo >> 8;
                v[2] = hi & 255u;
                v[3] = hi >> 8;
            } else {
                for (int j = 0; j < 4; ++j) v[j] = src[e0 + j];
            }
        } else {
            for (int j = 0; j < 4; ++j) {
                const long long e = e0 + j;
                int c = c0 + j;
                if (c >= 3) c -= 3;
                // (a G or B element always has its partner inside the frame: n is a multiple of 3)
                if (e >= 0 && e < n) v[j] = src[e + (c == 1 ? from_g : c == 2 ? from_b : 0)];
            }
        }
        for (int s = first_stage; s >= 1 && s <= last_stage; ++s) {
            if (!((fired >> s) & 1)) continue;
            double nz[4];
            if (s == kBitGaussian) {
                for (int h = 0; h < 2; ++h) {
                    double za, zb;
                    normal_pair((unsigned)(e0 >> 1) + (unsigned)h, (unsigned)kBitGaussian, i, ee, k0, k1, za, zb);
                    nz[2 * h] = za * 10.0;
                    nz[2 * h + 1] = zb * 10.0;
                }
            } else if (s == kBitChannel) {
                for (int j = 0; j < 4; ++j) {
                    int c = c0 + j;
                    if (c >= 3) c -= 3;
                    nz[j] = c == 0 ? ch_r : c == 1 ? ch_g : ch_b;
                }
            } else if (s == kBitBrightness) {
                for (int j = 0; j < 4; ++j) nz[j] = brightness;
            } else {
                for (int h = 0; h < 2; ++h) {
                    const Words d = philox4x32_10((unsigned)(e0 >> 1) + (unsigned)h, (unsigned)kBitUniform, i, ee, k0,
                                                  k1);
                    nz[2 * h] = -amount + (2.0 * amount) * uniform53(d.w[0], d.w[1]);
                    nz[2 * h + 1] = -amount + (2.0 * amount) * uniform53(d.w[2], d.w[3]);
                }
            }
            for (int j = 0; j < 4; ++j) v[j] = add_clip_truncate(v[j], nz[j]);
        }
        if (whole && wide_store) {
            *reinterpret_cast<float4 *>(dst + e0) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
        } else {
            for (int j = 0; j < 4; ++j)
                if (e0 + j >= 0 && e0 + j < n) dst[e0 + j] = (float)v[j];
        }
    }
}

}  // namespace

extern "C" int mpsr_sample_slots(const int *slot_frame, const int *slot_s, int n, const int *num_objs,
                                 const long long *label_offset, const int *split_index, const int *frame_local,
                                 const int *image_hw, const double *p00_p02, const double *label_boxes, int n_frames,
                                 unsigned long long seed, int epoch, int jitter_mode, long long *label_row,
                                 int *oversample_index, int *jitter_flag, double *boxes_xyxy, int *slot_hw,
                                 double *slot_p, int *slot_split_index, int *slot_frame_local, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0 && n_frames >= 0, "sample_slots: n %d, n_frames %d", n, n_frames);
    MPSR_REQUIRE(epoch >= 0 && epoch < (1 << 28), "sample_slots: epoch %d not in [0, 2^28)", epoch);
    MPSR_REQUIRE(jitter_mode >= MPSR_JITTER_NONE && jitter_mode <= MPSR_JITTER_ALL,
                 "sample_slots: unknown jitter_mode %d", jitter_mode);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(n_frames >= 1, "sample_slots: %d slots but no frame", n);
    MPSR_REQUIRE(slot_frame && slot_s && num_objs && label_offset && split_index && frame_local && image_hw &&
                     p00_p02 && label_boxes && label_row && oversample_index && jitter_flag && boxes_xyxy && slot_hw &&
                     slot_p && slot_split_index && slot_frame_local,
                 "sample_slots: a pointer is null");
    sample_slots_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, mpsr::as_stream(stream)>>>(
        slot_frame, slot_s, n, num_objs, label_offset, split_index, frame_local, image_hw, p00_p02, label_boxes,
        n_frames, (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)epoch, jitter_mode, label_row,
        oversample_index, jitter_flag, boxes_xyxy, slot_hw, slot_p, slot_split_index, slot_frame_local);
    MPSR_CHECK_LAUNCH("sample_slots_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_jitter_boxes_2d(const double *boxes_xyxy, const int *jitter_flag, const int *image_hw,
                                    const double *p00_p02, const int *frame_index, const int *slot, int n,
                                    unsigned long long seed, int epoch, double iou_threshold_min, int max_trials,
                                    int write_unjittered, double *out_xyxy, float *out_boxes_2d,
                                    float *out_boxes_2d_norm, float *out_view_angs, int *out_trials,
                                    mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0, "jitter_boxes_2d: n %d", n);
    MPSR_REQUIRE(epoch >= 0 && epoch < (1 << 28), "jitter_boxes_2d: epoch %d not in [0, 2^28)", epoch);
    // (the reference never enters its loop for a threshold <= 0 and never leaves it for one above 1)
    MPSR_REQUIRE(iou_threshold_min > 0.0 && iou_threshold_min <= 1.0,
                 "jitter_boxes_2d: iou_threshold_min %g not in (0, 1]", iou_threshold_min);
    MPSR_REQUIRE(max_trials >= 1 && max_trials <= (1 << 30), "jitter_boxes_2d: max_trials %d (1..2^30)", max_trials);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(boxes_xyxy && jitter_flag && image_hw && p00_p02 && frame_index && slot && out_xyxy && out_boxes_2d &&
                     out_boxes_2d_norm && out_view_angs && out_trials,
                 "jitter_boxes_2d: a pointer is null");
    jitter_boxes_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, mpsr::as_stream(stream)>>>(
        boxes_xyxy, jitter_flag, image_hw, p00_p02, frame_index, slot, n, (unsigned)(seed & 0xffffffffull),
        (unsigned)(seed >> 32), (unsigned)epoch, iou_threshold_min, max_trials, write_unjittered != 0, out_xyxy,
        out_boxes_2d, out_boxes_2d_norm, out_view_angs, out_trials);
    MPSR_CHECK_LAUNCH("jitter_boxes_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_image_noise(const unsigned char *frames, int n_frames, int h, int w, const int *gather,
                                const int *frame_index, int nb, unsigned long long seed, int epoch, int mode,
                                float *out, int *stages, double *params, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_frames >= 1 && h >= 1 && w >= 1 && nb >= 1, "image_noise: n_frames %d, h %d, w %d, nb %d (all >= 1)",
                 n_frames, h, w, nb);
    MPSR_REQUIRE((long long)h * w * 3 < (1LL << 31) - 8, "image_noise: a frame of %d x %d x 3 elements (< 2^31)", h, w);
    MPSR_REQUIRE(epoch >= 0 && epoch < (1 << 28), "image_noise: epoch %d not in [0, 2^28)", epoch);
    MPSR_REQUIRE(mode == MPSR_IMAGE_NOISE_REFERENCE || mode == MPSR_IMAGE_NOISE_COMPOSED,
                 "image_noise: unknown mode %d", mode);
    MPSR_REQUIRE(frames && gather && frame_index && out && stages && params, "image_noise: a pointer is null");
    const int n = h * w * 3;
    const long long per_block = (long long)kNoiseThreads * kNoiseQuads;
    // (n + 2 + 3) / 4 quads at most: a frame whose output base is 2 mod 4 starts two elements early
    const long long blocks_per_frame = ((((long long)n + 5) >> 2) + per_block - 1) / per_block;
    MPSR_REQUIRE(blocks_per_frame * nb < (1LL << 31), "image_noise: %d frames of %d x %d need too many blocks", nb, h,
                 w);
    image_noise_kernel<<<(unsigned)(blocks_per_frame * nb), kNoiseThreads, 0, mpsr::as_stream(stream)>>>(
        frames, n_frames, n, gather, frame_index, (int)blocks_per_frame, (unsigned)(seed & 0xffffffffull),
        (unsigned)(seed >> 32), (unsigned)epoch, mode, out, stages, params);
    MPSR_CHECK_LAUNCH("image_noise_kernel");
    return MPSR_OK;
}

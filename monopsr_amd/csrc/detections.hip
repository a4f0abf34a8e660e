// Evaluation on 2-D detections: obj_utils.merge_kitti_and_mscnn_obj_labels (obj_utils.py:1037-1089) for every frame
// of a split in one launch, and evaluator_utils.kitti_label_array (with or without project_boxes_3d) for every
// prediction of an epoch in one launch.
//
// The merge forms its IoU in float32: boxes_2d_from_obj_labels returns float32 arrays and two_d_iou of
// datasets/kitti/evaluation.py (:6-44, the one obj_utils imports) multiplies, adds and divides them as float32, stores
// the quotient in a float64 array and returns that array ROUNDED TO 3 DECIMALS (np.round: rint(x * 1000) / 1000).  The
// arg-max and `matching_iou >= min_iou` are taken in fp64 on the rounded values.  DESIGN.md section 7.5.
// Built with -ffp-contract=off: every product and sum is rounded as tests/merge_restatement.py rounds it.
#include "common.h"

#include <cmath>

namespace {

constexpr int kWave = 64;

// two_d_iou of one pair: float32 up to the quotient, then fp64 and rounded to 3 decimals (boxes [y1, x1, y2, x2])
__device__ __forceinline__ double two_d_iou_r3(const float d0, const float d1, const float d2, const float d3,
                                               const float *__restrict__ b)
{
    const float x1_int = fmaxf(d0, b[0]), y1_int = fmaxf(d1, b[1]);
    const float x2_int = fminf(d2, b[2]), y2_int = fminf(d3, b[3]);
    const float w_int = x2_int - x1_int, h_int = y2_int - y1_int;
    if (!(w_int > 0.0f && h_int > 0.0f)) return 0.0;
    const float inter = w_int * h_int;
    const float box_area = (d2 - d0) * (d3 - d1);
    const float boxes_area = (b[2] - b[0]) * (b[3] - b[1]);
    const float union_area = (box_area + boxes_area) - inter;
    const float iou = inter / union_area;
    return rint((double)iou * 1000.0) / 1000.0;
}

// One wave per frame.  Detections in file order; the lanes stride the frame's labels, each keeps its best
// (IoU, lowest index), and a butterfly gives every lane the frame's arg-max with np.argmax's tie rule.  The lane that
// owns a label (index % 64) is the only one that ever writes its outputs, so a later detection overwrites an earlier
// one in program order.
__global__ void __launch_bounds__(kWave) merge_detections_kernel(
    const float *__restrict__ label_boxes, const float *__restrict__ label_z, const long long *__restrict__ label_off,
    long long n_labels, const float *__restrict__ det_boxes, const double *__restrict__ det_scores,
    const long long *__restrict__ det_off, long long n_dets, int n_frames, double min_iou, int score_type,
    float *__restrict__ out_boxes, double *__restrict__ out_scores, int *__restrict__ out_match)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n_frames) return;
    const long long l0 = label_off[f], l1 = label_off[f + 1];
    long long d0 = det_off[f], d1 = det_off[f + 1];
    // offsets that leave the tables are the caller's error (include/monopsr_hip.h); such a frame is not touched
    if (l0 < 0 || l1 < l0 || l1 > n_labels || l1 - l0 > 0x7fffffffLL) return;
    if (d0 < 0 || d1 < d0 || d1 > n_dets || d1 - d0 > 0x7fffffffLL) d1 = d0;
    const int nl = (int)(l1 - l0), nd = (int)(d1 - d0);
    const float *kitti = label_boxes + 4 * l0;
    float *ob = out_boxes + 4 * l0;
    double *os = out_scores + l0;
    int *om = out_match + l0;
    for (int i = lane; i < nl; i += kWave) {
        for (int k = 0; k < 4; ++k) ob[4 * i + k] = kitti[4 * i + k];
        os[i] = 0.0;
        om[i] = -1;
    }
    for (int d = 0; d < nd && nl > 0; ++d) {
        const float *db = det_boxes + 4 * (d0 + d);
        const float b0 = db[0], b1 = db[1], b2 = db[2], b3 = db[3];
        double best = -1.0;
        int best_i = 0x7fffffff;
        for (int i = lane; i < nl; i += kWave) {
            const double iou = two_d_iou_r3(b0, b1, b2, b3, kitti + 4 * i);  // against the ORIGINAL box
            if (iou > best) {
                best = iou;
                best_i = i;
            }
        }
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            const double o = __shfl_xor(best, m, kWave);
            const int oi = __shfl_xor(best_i, m, kWave);
            if (o > best || (o == best && oi < best_i)) {
                best = o;
                best_i = oi;
            }
        }
        if (best_i < nl && best >= min_iou && (best_i % kWave) == lane) {
            ob[4 * best_i] = b0;
            ob[4 * best_i + 1] = b1;
            ob[4 * best_i + 2] = b2;
            ob[4 * best_i + 3] = b3;
            os[best_i] = det_scores[d0 + d];
            om[best_i] = d;
        }
    }
    if (score_type == MPSR_MERGE_SCORE_MIN) return;
    for (int i = lane; i < nl; i += kWave) {
        if (os[i] == 0.0) {
            float s = 1.0f;
            if (score_type == MPSR_MERGE_SCORE_DISTANCE) {
                s = 1.0f - label_z[l0 + i] / 45.0f;
                s = fminf(fmaxf(s, 0.1f), 1.0f);
            }
            os[i] = (double)s;
        }
    }
}

__device__ __forceinline__ double round3(double x) { return rint(x * 1000.0) / 1000.0; }

// One lane per prediction row.  rows: MPSR_KITTI_FIELDS columns in kitti_eval's order.
__global__ void __launch_bounds__(256) detection_rows_kernel(
    const float *__restrict__ box_3d, const float *__restrict__ box_2d, const int *__restrict__ frame,
    const double *__restrict__ p2, const int *__restrict__ image_wh, int n, int n_frames, double score_threshold,
    int project, double *__restrict__ rows, int *__restrict__ cls, int *__restrict__ keep)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const float *b3 = box_3d + 9 * (long long)t, *b2 = box_2d + 7 * (long long)t;
    const double x = b3[0], y = b3[1], z = b3[2], l = b3[3], w = b3[4], h = b3[5], ry = b3[6], score = b3[7];
    bool kept = score >= score_threshold;
    double x1 = b2[1], y1 = b2[0], x2 = b2[3], y2 = b2[2];
    if (project) {
        const int f = frame[t];
        if (f < 0 || f >= n_frames) {
            kept = false;  // (the caller's error: no frame to project with)
        } else {
            const double *p = p2 + 12 * (long long)f;
            const double w_img = (double)image_wh[2 * f], h_img = (double)image_wh[2 * f + 1];
            const double c = cos(ry), s = sin(ry);
            double u_min = 0, v_min = 0, u_max = 0, v_max = 0;
            for (int k = 0; k < 8; ++k) {
                // corner signs of evaluator_utils.project_boxes_3d: sx, sz, sy
                const double sx = (k & 2) ? -0.5 : 0.5;
                const double sz = ((k + 1) & 2) ? -0.5 : 0.5;
                const double sy = (k & 4) ? -1.0 : 0.0;
                const double cx = l * sx, cy = h * sy, cz = w * sz;
                const double px = c * cx + s * cz + x, py = cy + y, pz = -s * cx + c * cz + z;
                const double uu = p[0] * px + p[1] * py + p[2] * pz + p[3];
                const double vv = p[4] * px + p[5] * py + p[6] * pz + p[7];
                const double ww = p[8] * px + p[9] * py + p[10] * pz + p[11];
                const double u = uu / ww, v = vv / ww;
                // np.min / np.max propagate a NaN
                if (k == 0) {
                    u_min = u_max = u;
                    v_min = v_max = v;
                } else {
                    u_min = (u < u_min || u != u) ? u : u_min;
                    u_max = (u > u_max || u != u) ? u : u_max;
                    v_min = (v < v_min || v != v) ? v : v_min;
                    v_max = (v > v_max || v != v) ? v : v_max;
                }
            }
            const bool inside = u_min <= w_img && v_min <= h_img && u_max >= 0.0 && v_max >= 0.0;
            const bool small = (u_max - u_min) <= 0.8 * w_img && (v_max - v_min) <= 0.8 * h_img;
            kept = kept && inside && small;
            x1 = u_min < 0.0 ? 0.0 : u_min;
            y1 = v_min < 0.0 ? 0.0 : v_min;
            x2 = u_max > w_img ? w_img : u_max;
            y2 = v_max > h_img ? h_img : v_max;
        }
    }
    double *r = rows + MPSR_KITTI_FIELDS * (long long)t;
    r[0] = round3(x1);
    r[1] = round3(y1);
    r[2] = round3(x2);
    r[3] = round3(y2);
    r[4] = round3((double)b2[4]);
    r[5] = round3(h);
    r[6] = round3(w);
    r[7] = round3(l);
    r[8] = round3(x);
    r[9] = round3(y);
    r[10] = round3(z);
    r[11] = round3(ry);
    r[12] = round3(score);
    r[13] = 0.0;
    const float c8 = b3[8];
    cls[t] = (c8 >= -2147483648.0f && c8 < 2147483648.0f) ? (int)c8 : -1;
    keep[t] = kept ? 1 : 0;
}

}  // namespace

extern "C" int mpsr_merge_detections(const float *label_boxes, const float *label_z, const long long *label_off,
                                     long long n_labels, const float *det_boxes, const double *det_scores,
                                     const long long *det_off, long long n_dets, int n_frames, double min_iou,
                                     int score_type, float *out_boxes, double *out_scores, int *out_match,
                                     mpsr_stream_t stream)
{
    MPSR_REQUIRE(n_frames >= 0 && n_labels >= 0 && n_dets >= 0, "merge_detections: n_frames %d, n_labels %lld, n_dets %lld",
                 n_frames, n_labels, n_dets);
    MPSR_REQUIRE(score_type >= MPSR_MERGE_SCORE_DISTANCE && score_type <= MPSR_MERGE_SCORE_MIN,
                 "merge_detections: unknown score_type %d", score_type);
    MPSR_REQUIRE(min_iou == min_iou, "merge_detections: min_iou is not a number");
    if (n_frames == 0 || n_labels == 0) return MPSR_OK;
    MPSR_REQUIRE(label_boxes && label_z && label_off && det_off && out_boxes && out_scores && out_match,
                 "merge_detections: a pointer is null");
    MPSR_REQUIRE(n_dets == 0 || (det_boxes && det_scores), "merge_detections: a detection pointer is null");
    merge_detections_kernel<<<(unsigned)n_frames, kWave, 0, mpsr::as_stream(stream)>>>(
        label_boxes, label_z, label_off, n_labels, det_boxes, det_scores, det_off, n_dets, n_frames, min_iou,
        score_type, out_boxes, out_scores, out_match);
    MPSR_CHECK_LAUNCH("merge_detections_kernel");
    return MPSR_OK;
}

extern "C" int mpsr_kitti_detection_rows(const float *box_3d, const float *box_2d, const int *frame, const double *p2,
                                         const int *image_wh, int n, int n_frames, double score_threshold, int project,
                                         double *rows, int *cls, int *keep, mpsr_stream_t stream)
{
    MPSR_REQUIRE(n >= 0 && n_frames >= 0, "kitti_detection_rows: n %d, n_frames %d", n, n_frames);
    if (n == 0) return MPSR_OK;
    MPSR_REQUIRE(box_3d && box_2d && rows && cls && keep, "kitti_detection_rows: a pointer is null");
    MPSR_REQUIRE(!project || (frame && p2 && image_wh && n_frames >= 1),
                 "kitti_detection_rows: projection needs frame, p2 and image_wh of at least one frame");
    detection_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, mpsr::as_stream(stream)>>>(
        box_3d, box_2d, frame, p2, image_wh, n, n_frames, score_threshold, project != 0, rows, cls, keep);
    MPSR_CHECK_LAUNCH("detection_rows_kernel");
    return MPSR_OK;
}

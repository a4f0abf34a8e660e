// KITTI object evaluation (scripts/offline_eval/kitti_native_eval/evaluate_object_3d_offline.cpp) on the device, fp64.
//
// One ragged batch of frames (mpsr_kitti_batch): detection and ground-truth rows of MPSR_KITTI_FIELDS doubles, a class
// code per row, per-frame row offsets and per-frame (detection, ground truth) pair offsets.
//   mpsr_kitti_overlaps: the six overlaps of every pair, computed once (the C++ program recomputes them for every
//     score threshold): image / BEV / 3D IoU (criterion -1) and the same three over the detection's own area or
//     volume (criterion 0, the DontCare test).  One block per frame, threads striding over its pairs.
//   mpsr_kitti_match: computeStatistics with compute_fp = false (:457-636) for every (metric, class, difficulty) --
//     one lane per configuration, one block per frame.  Writes the score of each true positive into the slot of its
//     ground truth and the number of ground truths that count (n_gt of eval_class).
//   mpsr_kitti_stats: computeStatistics with compute_fp = true for every (configuration, frame, threshold) -- one
//     block per (frame, configuration), one lane per threshold; every lane reads the same overlap (a broadcast).
//     The per-frame results land in the workspace and a second kernel sums them over frames in frame order, one
//     thread per (configuration, threshold), as eval_class does (:686-705): no float atomics, the same order on
//     every run.
//   mpsr_kitti_match_slices / mpsr_kitti_stats_slices: the same two passes for n_slices slices at once.  A slice is an
//     IoU set (its nine min_overlap) and, when depth-tested, a depth bin lo <= z < hi: a ground truth outside it is
//     ignored (as if occluded beyond every level), a detection outside it is of another class.  A configuration is
//     then (slice, one of the 27), index slice * 27 + configuration: the matching pass runs one block per (frame,
//     group of 64 configurations), the statistics pass one block per (frame, launched configuration).  The slice
//     table, the thresholds' counts and the launched-configuration list are read from device memory (32 slices are
//     864 configurations: more than a launch's arguments should carry); the configuration -> slice map is the
//     division by 27.  The three old entry points are the one-slice, untested-depth case of the same kernels, with
//     their small tables still in the launch's arguments.
//     tp_scores is (n_slices * 27, n_gt) doubles, written whole (a row of another class holds NaN): at KITTI val's
//     37 540 ground truths and 14 slices that is 113 MB on the card and one copy of as much to the host.
// cleanData (:382-455) is applied inside the kernels, per (configuration, row).  Which detections a lane has assigned
// is a bitset in LDS, [word][lane] (lanes of one word hit distinct banks), sized at launch from the largest frame.
#include "common.h"
#include "kitti_geometry.h"

#include <cmath>

namespace {

using namespace mpsr_kitti;  // the geometry (:228-345) and the difficulty levels (:44-46)

constexpr int F = MPSR_KITTI_FIELDS;
constexpr int kCfg = MPSR_KITTI_CONFIGS;
constexpr int kPts = MPSR_KITTI_POINTS;
constexpr int kLanes = 64;

struct Batch {
    const double *det, *gt;
    const int *det_cls, *gt_cls, *det_off, *gt_off;
    const long long *pair_off;
    long long n_pairs;
};

// The one-slice entry points' tables, by value.
struct EvalArgs {
    double min_overlap[9];  // [metric][class] (:55)
    int n_thr[kCfg];        // thresholds per configuration (stats pass)
    int cfg[kCfg];          // configurations launched (stats pass): blockIdx.y -> configuration
    int compute_aos;        // no detection has alpha == -10 (:157)
};

// The sliced entry points' tables, in device memory; slices == nullptr: one slice, read from EvalArgs.
struct Tables {
    const mpsr_kitti_slice *slices;  // (n_slices)
    const int *n_thr;                // (n_slices * kCfg)
    const int *launched;             // (n_launched): blockIdx.y -> slice * kCfg + configuration
    int n_total;                     // n_slices * kCfg
};

// What compute_statistics needs of a slice.
struct Cut {
    double min_overlap;
    bool tested;  // false: no depth test whatever (a NaN z is in the slice too)
    double lo, hi;
};

__device__ inline bool in_cut(const Cut &c, double z) { return !c.tested || (c.lo <= z && z < c.hi); }

// global configuration gc = slice * kCfg + (metric * 3 + class) * 3 + difficulty
__device__ inline Cut cut_of(const EvalArgs &a, const Tables &t, int gc)
{
    const int mc = (gc % kCfg) / 3;  // metric * 3 + class
    if (!t.slices) return Cut{a.min_overlap[mc], false, 0.0, 0.0};
    const mpsr_kitti_slice &s = t.slices[gc / kCfg];
    return Cut{s.min_overlap[mc], s.depth_tested != 0, s.lo, s.hi};
}

// ---------------------------------------------------------------- overlaps

__global__ void __launch_bounds__(256) overlaps_kernel(Batch b, double *__restrict__ out)
{
    const int f = blockIdx.x;
    const int d0 = b.det_off[f], g0 = b.gt_off[f];
    const int ng = b.gt_off[f + 1] - g0;
    const long long p0 = b.pair_off[f], np = b.pair_off[f + 1] - p0;
    for (long long p = threadIdx.x; p < np; p += blockDim.x) {
        const int j = (int)(p / ng), i = (int)(p - (long long)j * ng);
        const double *d = b.det + (long long)(d0 + j) * F, *g = b.gt + (long long)(g0 + i) * F;
        double o[6];
        o[0] = image_overlap(d, g, false);
        o[3] = image_overlap(d, g, true);
        ground_and_box_overlaps(d, g, o);
        for (int k = 0; k < 6; ++k) out[k * b.n_pairs + p0 + p] = o[k];
    }
}

// ---------------------------------------------------------------- computeStatistics

// cleanData (:382-455) for one row
// A ground truth outside the slice's depth bin is ignored, as one occluded beyond every level.
__device__ inline int ignored_gt(const Batch &b, int row, int cls, int diff, const Cut &cut)
{
    const int code = b.gt_cls[row];
    const double *g = b.gt + (long long)row * F;
    int valid;
    if (code == cls) valid = 1;
    else if ((cls == MPSR_KITTI_PEDESTRIAN && code == MPSR_KITTI_PERSON_SITTING) ||
             (cls == MPSR_KITTI_CAR && code == MPSR_KITTI_VAN))
        valid = 0;
    else valid = -1;
    const double height = g[MPSR_KITTI_Y2] - g[MPSR_KITTI_Y1];  // double, compared with <= (:411)
    const bool ignore = g[MPSR_KITTI_OCCLUSION] > c_max_occlusion[diff] ||
                        g[MPSR_KITTI_TRUNCATION] > c_max_truncation[diff] || height <= c_min_height[diff] ||
                        !in_cut(cut, g[MPSR_KITTI_TZ]);
    if (valid == 1 && !ignore) return 0;
    if (valid == 0 || (ignore && valid == 1)) return 1;
    return -1;
}

// A detection outside the slice's depth bin is of another class.
__device__ inline int ignored_det(const Batch &b, int row, int cls, int diff, const Cut &cut)
{
    const double *d = b.det + (long long)row * F;
    const int height = (int)fabs(d[MPSR_KITTI_Y1] - d[MPSR_KITTI_Y2]);  // int32_t height = fabs(...) (:445)
    if (height < c_min_height[diff]) return 1;  // whatever the class (:448)
    return b.det_cls[row] == cls && in_cut(cut, d[MPSR_KITTI_TZ]) ? 0 : -1;
}

struct Stat {
    int tp, fp, fn;
    double sim, sim_ground;
};

// One lane's computeStatistics for frame f, configuration cfg (one of the 27) and slice `cut`.  `assigned` is this
// lane's bitset (stride kLanes).
// compute_fp = false: tp_slot (when non-null) receives each true positive's score at its ground truth's row.
template <bool kComputeFp>
__device__ Stat compute_statistics(const Batch &b, const double *__restrict__ ov, int f, int cfg, const Cut &cut,
                                   double thresh, bool aos, unsigned *assigned, double *tp_slot)
{
    const double min_overlap = cut.min_overlap;
    const int metric = cfg / 9, cls = (cfg / 3) % 3, diff = cfg % 3;
    const double NO_DETECTION = -10000000;
    const int d0 = b.det_off[f], nd = b.det_off[f + 1] - d0;
    const int g0 = b.gt_off[f], ng = b.gt_off[f + 1] - g0;
    const long long p0 = b.pair_off[f];
    const double *ov_union = ov + metric * b.n_pairs + p0, *ov_own = ov + (metric + 3) * b.n_pairs + p0;
    const bool heading = metric != 0;  // compute_aos_ground: BEV and 3D (:932)
    for (int w = 0; w < (nd + 31) / 32; ++w) assigned[w * kLanes] = 0u;
#define ASSIGNED(j) ((assigned[((j) >> 5) * kLanes] >> ((j) & 31)) & 1u)
#define ASSIGN(j) (assigned[((j) >> 5) * kLanes] |= 1u << ((j) & 31))
#define IGN_THR(j) (kComputeFp && b.det[(long long)(d0 + (j)) * F + MPSR_KITTI_SCORE] < thresh)

    Stat st{0, 0, 0, 0.0, 0.0};
    for (int i = 0; i < ng; ++i) {
        const int ig = ignored_gt(b, g0 + i, cls, diff, cut);
        if (ig == -1) continue;
        int det_idx = -1;
        double valid_detection = NO_DETECTION, max_overlap = 0;
        bool assigned_ignored_det = false;
        for (int j = 0; j < nd; ++j) {
            const int id = ignored_det(b, d0 + j, cls, diff, cut);
            if (id == -1 || ASSIGNED(j) || IGN_THR(j)) continue;
            const double overlap = ov_union[(long long)j * ng + i];
            const double score = b.det[(long long)(d0 + j) * F + MPSR_KITTI_SCORE];
            if (!kComputeFp && overlap > min_overlap && score > valid_detection) {
                det_idx = j;
                valid_detection = score;
            } else if (kComputeFp && overlap > min_overlap && (overlap > max_overlap || assigned_ignored_det) &&
                       id == 0) {
                max_overlap = overlap;
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = false;
            } else if (kComputeFp && overlap > min_overlap && valid_detection == NO_DETECTION && id == 1) {
                det_idx = j;
                valid_detection = 1;
                assigned_ignored_det = true;
            }
        }
        if (valid_detection == NO_DETECTION && ig == 0) {
            st.fn++;
        } else if (valid_detection != NO_DETECTION &&
                   (ig == 1 || ignored_det(b, d0 + det_idx, cls, diff, cut) == 1)) {
            ASSIGN(det_idx);
        } else if (valid_detection != NO_DETECTION) {
            st.tp++;
            const double *g = b.gt + (long long)(g0 + i) * F, *d = b.det + (long long)(d0 + det_idx) * F;
            if (tp_slot) tp_slot[g0 + i] = d[MPSR_KITTI_SCORE];
            // tmp = fp zeros then the TPs in ground-truth order, summed from 0.0 (:600-612): the zeros add nothing
            if (aos) st.sim += (1.0 + cos(g[MPSR_KITTI_ALPHA] - d[MPSR_KITTI_ALPHA])) / 2.0;
            // abs(double) (:554): with `using namespace std` and <math.h>, std::abs(double) is the overload chosen
            // (checked with g++ 11 / libstdc++ on the reference's includes), not the int one.
            if (heading) st.sim_ground += (1.0 + cos(fabs(g[MPSR_KITTI_RY] - d[MPSR_KITTI_RY]))) / 2.0;
            ASSIGN(det_idx);
        }
    }
    if (kComputeFp) {
        for (int j = 0; j < nd; ++j) {
            const int id = ignored_det(b, d0 + j, cls, diff, cut);
            if (!(ASSIGNED(j) || id == -1 || id == 1 || IGN_THR(j))) st.fp++;
        }
        // detections in DontCare regions: the metric's own overlap with criterion 0 (:572-595)
        int nstuff = 0;
        for (int i = 0; i < ng; ++i) {
            if (b.gt_cls[g0 + i] != MPSR_KITTI_DONTCARE) continue;
            for (int j = 0; j < nd; ++j) {
                if (ASSIGNED(j)) continue;
                const int id = ignored_det(b, d0 + j, cls, diff, cut);
                if (id == -1 || id == 1 || IGN_THR(j)) continue;
                if (ov_own[(long long)j * ng + i] > min_overlap) {
                    ASSIGN(j);
                    nstuff++;
                }
            }
        }
        st.fp -= nstuff;
        // neither a FP nor a TP: the similarity is ignored in the evaluation (-1, :614-616)
        if (aos && !(st.tp > 0 || st.fp > 0)) st.sim = -1;
        if (heading && !(st.tp > 0 || st.fp > 0)) st.sim_ground = -1;
    }
#undef ASSIGNED
#undef ASSIGN
#undef IGN_THR
    return st;
}

// grid (frames, groups of kLanes configurations); tp_scores (n_total, n_gt), n_care (n_total, n_frames)
__global__ void __launch_bounds__(kLanes) match_kernel(Batch b, const double *__restrict__ ov, EvalArgs a, Tables tb,
                                                       double *__restrict__ tp_scores, int *__restrict__ n_care,
                                                       int n_gt, int n_frames)
{
    extern __shared__ unsigned bits[];
    const int f = blockIdx.x, gc = blockIdx.y * kLanes + threadIdx.x;
    if (gc >= tb.n_total) return;
    const int cfg = gc % kCfg, cls = (cfg / 3) % 3, diff = cfg % 3;
    const Cut cut = cut_of(a, tb, gc);
    double *slot = tp_scores + (long long)gc * n_gt;
    const int g0 = b.gt_off[f], g1 = b.gt_off[f + 1];
    int care = 0;
    for (int r = g0; r < g1; ++r) {
        slot[r] = NAN;  // no true positive
        care += ignored_gt(b, r, cls, diff, cut) == 0;
    }
    compute_statistics<false>(b, ov, f, cfg, cut, 0.0, false, bits + threadIdx.x, slot);
    n_care[(long long)gc * n_frames + f] = care;
}

// per-frame partials, [launched configuration][frame][threshold]
struct Partials {
    int *tp, *fp, *fn;
    double *sim, *sim_ground;
};

// blockIdx.y -> global configuration, and its number of thresholds
__device__ inline int launched_config(const EvalArgs &a, const Tables &tb, int k, int *n_thr)
{
    const int gc = tb.slices ? tb.launched[k] : a.cfg[k];
    const int n = gc < 0 ? 0 : tb.slices ? tb.n_thr[gc] : a.n_thr[gc];
    *n_thr = n < kPts ? n : kPts;
    return gc;
}

__global__ void __launch_bounds__(kLanes) stats_kernel(Batch b, const double *__restrict__ ov, EvalArgs a, Tables tb,
                                                       const double *__restrict__ thresholds, Partials part,
                                                       int n_frames)
{
    extern __shared__ unsigned bits[];
    const int f = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    int n_thr;
    const int gc = launched_config(a, tb, k, &n_thr);
    if (t >= n_thr) return;
    const int cfg = gc % kCfg, metric = cfg / 9;
    const Stat s = compute_statistics<true>(b, ov, f, cfg, cut_of(a, tb, gc), thresholds[(long long)gc * kPts + t],
                                            metric == 0 && a.compute_aos, bits + t, nullptr);
    const long long o = ((long long)k * n_frames + f) * kPts + t;
    part.tp[o] = s.tp;
    part.fp[o] = s.fp;
    part.fn[o] = s.fn;
    part.sim[o] = s.sim;
    part.sim_ground[o] = s.sim_ground;
}

// the sum over frames of eval_class (:695-704), in frame order
__global__ void __launch_bounds__(kLanes) reduce_kernel(EvalArgs a, Tables tb, Partials part, int n_frames,
                                                        int *__restrict__ counts, double *__restrict__ similarity)
{
    const int k = blockIdx.x, t = threadIdx.x;
    int n_thr;
    const int gc = launched_config(a, tb, k, &n_thr);
    if (t >= kPts || gc < 0) return;
    int tp = 0, fp = 0, fn = 0;
    double sim = 0, sim_ground = 0;
    if (t < n_thr) {
        for (int f = 0; f < n_frames; ++f) {
            const long long o = ((long long)k * n_frames + f) * kPts + t;
            tp += part.tp[o];
            fp += part.fp[o];
            fn += part.fn[o];
            const double s = part.sim[o], sg = part.sim_ground[o];
            if (s != -1) sim += s;
            if (sg != -1) sim_ground += sg;
        }
    }
    const int o = gc * kPts + t;
    counts[o * 3 + 0] = tp;
    counts[o * 3 + 1] = fp;
    counts[o * 3 + 2] = fn;
    similarity[o * 2 + 0] = sim;
    similarity[o * 2 + 1] = sim_ground;
}

// The launched-configuration list of the sliced statistics pass: the configurations with thresholds, in order.  One
// thread; at most 32 * 27 entries.  Exactly n_launched entries are written, the host's count: were the device's copy of
// the counts another, the rest would be -1, which the kernels skip.
__global__ void launched_kernel(const int *__restrict__ n_thr, int n_total, int n_launched,
                                int *__restrict__ launched)
{
    if (blockIdx.x || threadIdx.x) return;
    int k = 0;
    for (int gc = 0; gc < n_total && k < n_launched; ++gc)
        if (n_thr[gc] > 0) launched[k++] = gc;
    for (; k < n_launched; ++k) launched[k] = -1;
}

// ---------------------------------------------------------------- host side

constexpr size_t kLdsLimit = 64 * 1024;

int check_batch(const mpsr_kitti_batch *kb, Batch *b, int *max_det)
{
    MPSR_REQUIRE(kb, "kitti: batch is null");
    MPSR_REQUIRE(kb->n_frames >= 0 && kb->n_det >= 0 && kb->n_gt >= 0,
                 "kitti: negative count (frames %d, detections %d, ground truths %d)", kb->n_frames, kb->n_det,
                 kb->n_gt);
    MPSR_REQUIRE(kb->det_off_host && kb->gt_off_host && kb->pair_off_host,
                 "kitti: host offsets are null (they are read on the host)");
    MPSR_REQUIRE(kb->n_frames == 0 || (kb->det_off && kb->gt_off && kb->pair_off),
                 "kitti: device offsets are null with %d frames", kb->n_frames);
    MPSR_REQUIRE(kb->n_det == 0 || (kb->det && kb->det_cls), "kitti: detection rows are null with n_det = %d",
                 kb->n_det);
    MPSR_REQUIRE(kb->n_gt == 0 || (kb->gt && kb->gt_cls), "kitti: ground-truth rows are null with n_gt = %d",
                 kb->n_gt);
    const int *dof = kb->det_off_host, *gof = kb->gt_off_host;
    const long long *pof = kb->pair_off_host;
    MPSR_REQUIRE(dof[0] == 0 && gof[0] == 0 && pof[0] == 0, "kitti: offsets must start at 0");
    int md = 0;
    for (int f = 0; f < kb->n_frames; ++f) {
        MPSR_REQUIRE(dof[f + 1] >= dof[f] && gof[f + 1] >= gof[f] && pof[f + 1] >= pof[f],
                     "kitti: offsets decrease at frame %d", f);
        const long long nd = dof[f + 1] - dof[f], ng = gof[f + 1] - gof[f];
        MPSR_REQUIRE(pof[f + 1] - pof[f] == nd * ng,
                     "kitti: frame %d has %lld pairs, expected %lld detections x %lld ground truths", f,
                     pof[f + 1] - pof[f], nd, ng);
        if (nd > md) md = (int)nd;
    }
    MPSR_REQUIRE(dof[kb->n_frames] == kb->n_det && gof[kb->n_frames] == kb->n_gt,
                 "kitti: last offsets (%d, %d) != row counts (%d, %d)", dof[kb->n_frames], gof[kb->n_frames],
                 kb->n_det, kb->n_gt);
    *b = Batch{kb->det, kb->gt, kb->det_cls, kb->gt_cls, kb->det_off, kb->gt_off, kb->pair_off,
               pof[kb->n_frames]};
    *max_det = md;
    return MPSR_OK;
}

int check_limits(int max_det, size_t *lds)
{
    MPSR_REQUIRE(max_det <= MPSR_KITTI_MAX_FRAME_DETECTIONS,
                 "kitti: a frame holds %d detections, more than the %d the statistics kernels support", max_det,
                 MPSR_KITTI_MAX_FRAME_DETECTIONS);
    *lds = (size_t)((max_det + 31) / 32) * kLanes * sizeof(unsigned);
    if (*lds == 0) *lds = sizeof(unsigned);
    return MPSR_OK;
}

int fill_overlap_table(const double *min_overlap, EvalArgs *a)
{
    MPSR_REQUIRE(min_overlap, "kitti: min_overlap is null");
    for (int k = 0; k < 9; ++k) a->min_overlap[k] = min_overlap[k];
    return MPSR_OK;
}

}  // namespace

static_assert(kLdsLimit == (size_t)MPSR_KITTI_MAX_FRAME_DETECTIONS / 32 * kLanes * sizeof(unsigned),
              "the detection limit is what one block's bitsets fit in 64 KB of LDS");

extern "C" int mpsr_kitti_overlaps(const mpsr_kitti_batch *batch, double *overlaps, mpsr_stream_t stream)
{
    Batch b;
    int max_det;
    int st = check_batch(batch, &b, &max_det);
    if (st) return st;
    MPSR_REQUIRE(b.n_pairs == 0 || overlaps, "kitti: overlaps is null with %lld pairs", b.n_pairs);
    if (b.n_pairs == 0) return MPSR_OK;
    hipLaunchKernelGGL(overlaps_kernel, dim3(batch->n_frames), dim3(256), 0, mpsr::as_stream(stream), b, overlaps);
    MPSR_CHECK_LAUNCH("kitti overlaps");
    return MPSR_OK;
}


namespace {

// The slice table as the host sees it: 1 .. MPSR_KITTI_MAX_SLICES slices, a depth-tested one with lo <= hi.
int check_slices(const mpsr_kitti_slice *slices, const mpsr_kitti_slice *slices_host, int n_slices)
{
    MPSR_REQUIRE(n_slices >= 1 && n_slices <= MPSR_KITTI_MAX_SLICES, "kitti: %d slices (1..%d)", n_slices,
                 MPSR_KITTI_MAX_SLICES);
    MPSR_REQUIRE(slices && slices_host, "kitti: the slice table is null (it is read on the device and on the host)");
    for (int s = 0; s < n_slices; ++s) {
        const mpsr_kitti_slice &c = slices_host[s];
        MPSR_REQUIRE(!c.depth_tested || c.lo <= c.hi, "kitti: slice %d has the depth bin [%g, %g): hi < lo or a NaN",
                     s, c.lo, c.hi);
    }
    return MPSR_OK;
}

int launch_match(const mpsr_kitti_batch *batch, const double *overlaps, const EvalArgs &a, const Tables &tb,
                 double *tp_scores, int *n_care, mpsr_stream_t stream)
{
    Batch b;
    int max_det;
    size_t lds;
    int st = check_batch(batch, &b, &max_det);
    if (!st) st = check_limits(max_det, &lds);
    if (st) return st;
    MPSR_REQUIRE(b.n_pairs == 0 || overlaps, "kitti: overlaps is null with %lld pairs", b.n_pairs);
    MPSR_REQUIRE(batch->n_frames == 0 || ((tp_scores || batch->n_gt == 0) && n_care),
                 "kitti: match outputs are null with %d frames", batch->n_frames);
    if (batch->n_frames == 0) return MPSR_OK;
    hipLaunchKernelGGL(match_kernel, dim3(batch->n_frames, (tb.n_total + kLanes - 1) / kLanes), dim3(kLanes), lds,
                       mpsr::as_stream(stream), b, overlaps, a, tb, tp_scores, n_care, batch->n_gt, batch->n_frames);
    MPSR_CHECK_LAUNCH("kitti match");
    return MPSR_OK;
}

size_t partials_bytes(int n_frames, int n_configs)
{
    if (n_frames <= 0 || n_configs <= 0) return 0;
    const size_t n = (size_t)n_configs * n_frames * kPts;
    return mpsr::align_up(3 * n * sizeof(int), 256) + 2 * n * sizeof(double);
}

// the list of launched configurations sits in front of the sliced pass's partials
constexpr size_t kLaunchedBytes = ((size_t)MPSR_KITTI_MAX_SLICES * kCfg * sizeof(int) + 255) / 256 * 256;
static_assert(kLaunchedBytes % 256 == 0, "the partials behind the list stay aligned");

// The statistics pass and the frame-order sum of n_launched configurations (the host's count of those with
// thresholds).  The workspace: partials_bytes, behind kLaunchedBytes of list when the tables are in device memory.
int launch_stats(const mpsr_kitti_batch *batch, const double *overlaps, const EvalArgs &a, Tables tb, int n_launched,
                 const double *thresholds, int *counts, double *similarity, void *workspace, size_t workspace_bytes,
                 mpsr_stream_t stream)
{
    Batch b;
    int max_det;
    size_t lds;
    int st = check_batch(batch, &b, &max_det);
    if (!st) st = check_limits(max_det, &lds);
    if (st) return st;
    MPSR_REQUIRE(counts && similarity, "kitti: stats outputs are null");
    MPSR_REQUIRE(n_launched == 0 || thresholds, "kitti: thresholds is null");
    const int nf = batch->n_frames;
    const size_t lead = tb.slices ? kLaunchedBytes : 0;
    const size_t need = partials_bytes(nf, n_launched) ? lead + partials_bytes(nf, n_launched) : 0;
    if (workspace_bytes < need || (need && !workspace))
        return mpsr::fail(MPSR_ERR_WORKSPACE, "kitti stats: workspace %zu bytes < %zu", workspace_bytes, need);
    MPSR_REQUIRE(b.n_pairs == 0 || overlaps, "kitti: overlaps is null with %lld pairs", b.n_pairs);
    MPSR_CHECK_HIP(hipMemsetAsync(counts, 0, sizeof(int) * tb.n_total * kPts * 3, mpsr::as_stream(stream)));
    MPSR_CHECK_HIP(hipMemsetAsync(similarity, 0, sizeof(double) * tb.n_total * kPts * 2, mpsr::as_stream(stream)));
    if (n_launched == 0 || nf == 0) return MPSR_OK;
    const size_t n = (size_t)n_launched * nf * kPts;
    char *partials = static_cast<char *>(workspace) + lead;
    if (tb.slices) {
        int *launched = static_cast<int *>(workspace);
        hipLaunchKernelGGL(launched_kernel, dim3(1), dim3(1), 0, mpsr::as_stream(stream), tb.n_thr, tb.n_total,
                           n_launched, launched);
        MPSR_CHECK_LAUNCH("kitti launched configurations");
        tb.launched = launched;
    }
    Partials part;
    part.tp = reinterpret_cast<int *>(partials);
    part.fp = part.tp + n;
    part.fn = part.fp + n;
    part.sim = reinterpret_cast<double *>(partials + mpsr::align_up(3 * n * sizeof(int), 256));
    part.sim_ground = part.sim + n;
    hipLaunchKernelGGL(stats_kernel, dim3(nf, n_launched), dim3(kLanes), lds, mpsr::as_stream(stream), b, overlaps, a,
                       tb, thresholds, part, nf);
    MPSR_CHECK_LAUNCH("kitti stats");
    hipLaunchKernelGGL(reduce_kernel, dim3(n_launched), dim3(kLanes), 0, mpsr::as_stream(stream), a, tb, part, nf,
                       counts, similarity);
    MPSR_CHECK_LAUNCH("kitti stats reduce");
    return MPSR_OK;
}

}  // namespace

extern "C" int mpsr_kitti_match(const mpsr_kitti_batch *batch, const double *overlaps, const double *min_overlap,
                                double *tp_scores, int *n_care, mpsr_stream_t stream)
{
    EvalArgs a{};
    const int st = fill_overlap_table(min_overlap, &a);
    if (st) return st;
    return launch_match(batch, overlaps, a, Tables{nullptr, nullptr, nullptr, kCfg}, tp_scores, n_care, stream);
}

extern "C" int mpsr_kitti_match_slices(const mpsr_kitti_batch *batch, const double *overlaps,
                                       const mpsr_kitti_slice *slices, const mpsr_kitti_slice *slices_host,
                                       int n_slices, double *tp_scores, int *n_care, mpsr_stream_t stream)
{
    const int st = check_slices(slices, slices_host, n_slices);
    if (st) return st;
    return launch_match(batch, overlaps, EvalArgs{}, Tables{slices, nullptr, nullptr, n_slices * kCfg}, tp_scores,
                        n_care, stream);
}

extern "C" size_t mpsr_kitti_stats_workspace_bytes(int n_frames, int n_configs)
{
    return partials_bytes(n_frames, n_configs);
}

extern "C" size_t mpsr_kitti_stats_slices_workspace_bytes(int n_frames, int n_configs)
{
    const size_t p = partials_bytes(n_frames, n_configs);
    return p ? kLaunchedBytes + p : 0;
}

extern "C" int mpsr_kitti_stats(const mpsr_kitti_batch *batch, const double *overlaps, const double *min_overlap,
                                const double *thresholds, const int *n_thresholds, int compute_aos, int *counts,
                                double *similarity, void *workspace, size_t workspace_bytes, mpsr_stream_t stream)
{
    EvalArgs a{};
    const int st = fill_overlap_table(min_overlap, &a);
    if (st) return st;
    MPSR_REQUIRE(n_thresholds, "kitti: n_thresholds is null");
    int n_cfg = 0;
    for (int c = 0; c < kCfg; ++c) {
        MPSR_REQUIRE(n_thresholds[c] >= 0 && n_thresholds[c] <= kPts,
                     "kitti: configuration %d has %d thresholds (0..%d)", c, n_thresholds[c], kPts);
        a.n_thr[c] = n_thresholds[c];
        if (n_thresholds[c] > 0) a.cfg[n_cfg++] = c;
    }
    a.compute_aos = compute_aos ? 1 : 0;
    return launch_stats(batch, overlaps, a, Tables{nullptr, nullptr, nullptr, kCfg}, n_cfg, thresholds, counts,
                        similarity, workspace, workspace_bytes, stream);
}

extern "C" int mpsr_kitti_stats_slices(const mpsr_kitti_batch *batch, const double *overlaps,
                                       const mpsr_kitti_slice *slices, const mpsr_kitti_slice *slices_host,
                                       int n_slices, const double *thresholds, const int *n_thresholds,
                                       const int *n_thresholds_host, int compute_aos, int *counts, double *similarity,
                                       void *workspace, size_t workspace_bytes, mpsr_stream_t stream)
{
    const int st = check_slices(slices, slices_host, n_slices);
    if (st) return st;
    MPSR_REQUIRE(n_thresholds && n_thresholds_host,
                 "kitti: n_thresholds is null (it is read on the device and on the host)");
    const int n_total = n_slices * kCfg;
    int n_launched = 0;
    for (int c = 0; c < n_total; ++c) {
        MPSR_REQUIRE(n_thresholds_host[c] >= 0 && n_thresholds_host[c] <= kPts,
                     "kitti: configuration %d of slice %d has %d thresholds (0..%d)", c % kCfg, c / kCfg,
                     n_thresholds_host[c], kPts);
        n_launched += n_thresholds_host[c] > 0;
    }
    EvalArgs a{};
    a.compute_aos = compute_aos ? 1 : 0;
    return launch_stats(batch, overlaps, a, Tables{slices, n_thresholds, nullptr, n_total}, n_launched, thresholds,
                        counts, similarity, workspace, workspace_bytes, stream);
}

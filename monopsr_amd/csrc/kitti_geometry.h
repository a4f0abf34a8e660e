// The box geometry of KITTI's object evaluation (evaluate_object_3d_offline.cpp:228-345) and its difficulty levels
// (:44-46), fp64, on rows of MPSR_KITTI_FIELDS doubles: one body for kitti_eval.hip (all pairs of a frame) and
// object_pairs.hip (each prediction against its own label).  Both are built with -ffp-contract=off.
#pragma once
#include "common.h"

#include <cmath>

namespace mpsr_kitti {

// evaluation parameters (:44-46)
__constant__ static int c_min_height[3] = {40, 25, 25};
__constant__ static int c_max_occlusion[3] = {0, 1, 2};
__constant__ static double c_max_truncation[3] = {0.15, 0.3, 0.5};

__device__ inline double image_overlap(const double *d, const double *g, bool own)
{
    double x1 = fmax(d[MPSR_KITTI_X1], g[MPSR_KITTI_X1]), y1 = fmax(d[MPSR_KITTI_Y1], g[MPSR_KITTI_Y1]);
    double x2 = fmin(d[MPSR_KITTI_X2], g[MPSR_KITTI_X2]), y2 = fmin(d[MPSR_KITTI_Y2], g[MPSR_KITTI_Y2]);
    double w = x2 - x1, h = y2 - y1;
    if (w <= 0 || h <= 0) return 0;
    double inter = w * h;
    double a_area = (d[MPSR_KITTI_X2] - d[MPSR_KITTI_X1]) * (d[MPSR_KITTI_Y2] - d[MPSR_KITTI_Y1]);
    double b_area = (g[MPSR_KITTI_X2] - g[MPSR_KITTI_X1]) * (g[MPSR_KITTI_Y2] - g[MPSR_KITTI_Y1]);
    return own ? inter / a_area : inter / (a_area + b_area - inter);
}

// toPolygon (:266-292): rotation [[c, s], [-s, c]] applied to corners (+-l/2, +-w/2) on (x, z), clockwise order
__device__ inline void bev_corners(const double *b, double *px, double *pz)
{
    const double c = cos(b[MPSR_KITTI_RY]), s = sin(b[MPSR_KITTI_RY]);
    const double l2 = b[MPSR_KITTI_L] / 2, w2 = b[MPSR_KITTI_W] / 2;
    const double cx[4] = {l2, l2, -l2, -l2}, cz[4] = {w2, -w2, -w2, w2};
    for (int i = 0; i < 4; ++i) {
        px[i] = c * cx[i] + s * cz[i] + b[MPSR_KITTI_TX];
        pz[i] = -s * cx[i] + c * cz[i] + b[MPSR_KITTI_TZ];
    }
}

__device__ inline double shoelace(const double *px, const double *pz, int n)
{
    double a = 0;
    for (int i = 0; i < n; ++i) {
        int j = i + 1 == n ? 0 : i + 1;
        a += px[i] * pz[j] - px[j] * pz[i];
    }
    return fabs(a) / 2;
}

// Exact intersection of two convex quadrilaterals: the subject (detection) clipped by each edge's half-plane of the
// clip polygon (ground truth), then the shoelace formula.  A convex quad clipped by four half-planes has at most 8
// vertices.  Returns the intersection area; areas of both polygons through *area_d / *area_g.
__device__ inline double bev_intersection(const double *d, const double *g, double *area_d, double *area_g)
{
    double sx[8], sz[8], tx[8], tz[8], gx[4], gz[4];
    bev_corners(d, sx, sz);
    bev_corners(g, gx, gz);
    *area_d = shoelace(sx, sz, 4);
    *area_g = shoelace(gx, gz, 4);
    // orientation of the clip polygon: inside = the side of its interior
    double orient = 0;
    for (int i = 0; i < 4; ++i) orient += gx[i] * gz[(i + 1) & 3] - gx[(i + 1) & 3] * gz[i];
    const double sgn = orient < 0 ? -1.0 : 1.0;
    int n = 4;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double ax = gx[e], az = gz[e], ex = gx[(e + 1) & 3] - ax, ez = gz[(e + 1) & 3] - az;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int j = i + 1 == n ? 0 : i + 1;
            const double si = sgn * (ex * (sz[i] - az) - ez * (sx[i] - ax));
            const double sj = sgn * (ex * (sz[j] - az) - ez * (sx[j] - ax));
            if (si >= 0) {
                tx[m] = sx[i];
                tz[m] = sz[i];
                ++m;
            }
            if ((si >= 0) != (sj >= 0)) {
                const double t = si / (si - sj);
                tx[m] = sx[i] + t * (sx[j] - sx[i]);
                tz[m] = sz[i] + t * (sz[j] - sz[i]);
                ++m;
            }
        }
        n = m < 8 ? m : 8;
        for (int i = 0; i < n; ++i) {
            sx[i] = tx[i];
            sz[i] = tz[i];
        }
    }
    return n >= 3 ? shoelace(sx, sz, n) : 0.0;
}

// groundBoxOverlap and box3DOverlap (:294-345) of detection d against ground truth g, both criteria, into their places
// among mpsr_kitti_overlaps' six: o[1] = BEV IoU, o[2] = 3D IoU (criterion -1); o[4], o[5] = the same over the
// detection's own area / volume (criterion 0).  o[0] and o[3], the image overlaps, are not touched.
__device__ inline void ground_and_box_overlaps(const double *d, const double *g, double *o)
{
    // boxes with non-positive l / w (BEV) or l / w / h (3D) overlap nothing (boost's result is undefined there)
    const bool bev_ok = d[MPSR_KITTI_L] > 0 && d[MPSR_KITTI_W] > 0 && g[MPSR_KITTI_L] > 0 && g[MPSR_KITTI_W] > 0;
    const bool box_ok = bev_ok && d[MPSR_KITTI_H] > 0 && g[MPSR_KITTI_H] > 0;
    double inter = 0, area_d = 1, area_g = 1;
    if (bev_ok) inter = bev_intersection(d, g, &area_d, &area_g);
    o[1] = bev_ok ? inter / (area_d + area_g - inter) : 0.0;
    o[4] = bev_ok ? inter / area_d : 0.0;
    // box3DOverlap (:318-345): y is the bottom face, the box extends up by h
    const double ymax = fmin(d[MPSR_KITTI_TY], g[MPSR_KITTI_TY]);
    const double ymin = fmax(d[MPSR_KITTI_TY] - d[MPSR_KITTI_H], g[MPSR_KITTI_TY] - g[MPSR_KITTI_H]);
    const double inter_vol = inter * fmax(0.0, ymax - ymin);
    const double det_vol = d[MPSR_KITTI_H] * d[MPSR_KITTI_L] * d[MPSR_KITTI_W];
    const double gt_vol = g[MPSR_KITTI_H] * g[MPSR_KITTI_L] * g[MPSR_KITTI_W];
    o[2] = box_ok ? inter_vol / (det_vol + gt_vol - inter_vol) : 0.0;
    o[5] = box_ok ? inter_vol / det_vol : 0.0;
}

}  // namespace mpsr_kitti

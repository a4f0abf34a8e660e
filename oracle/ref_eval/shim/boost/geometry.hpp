// A boost-free stand-in for the four boost::geometry calls KITTI's evaluate_object_3d_offline.cpp makes on the
// bird's-eye-view rectangles of two boxes: append, intersection, union_ and area.  Test infrastructure only, written
// for this project (see oracle/ref_eval/README.md); it lets the unmodified program be compiled as a second oracle.
//
// What it claims to reproduce: the area of the intersection of two convex, clockwise, non-degenerate quadrilaterals,
// to within a few ulps of the exact value (long double throughout), and an empty result when they share no area
// (disjoint, or touching along an edge or at a corner).  It does not follow boost's own operation order, so an
// overlap that lies within rounding of a threshold may compare differently than under boost.
//
// The shim's one shortcut: union_ does not build the union's outline.  It returns one polygon that carries
// area(a) + area(b) - area(intersection), which is all the evaluator reads from it (area(un.front())).
//
// Outside what it claims: a counter-clockwise or zero-area input polygon.  Those abort() with a message instead of
// guessing what boost would do.
#ifndef REF_EVAL_SHIM_GEOMETRY_HPP
#define REF_EVAL_SHIM_GEOMETRY_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include <boost/geometry/geometries/point_xy.hpp>
#include <boost/geometry/geometries/polygon.hpp>

namespace boost {
namespace geometry {

namespace cs {
struct cartesian {};
}  // namespace cs

namespace shim_detail {

typedef long double real;

struct pt {
    real x, y;
};

// The open ring of a polygon (the closing repeat of the first point dropped).
template <typename P>
std::vector<pt> ring(const model::polygon<P>& poly) {
    std::vector<pt> r;
    const std::vector<P>& o = poly.outer();
    for (std::size_t i = 0; i < o.size(); ++i) {
        pt p = {o[i].x(), o[i].y()};
        r.push_back(p);
    }
    if (r.size() > 1 && r.front().x == r.back().x && r.front().y == r.back().y) r.pop_back();
    return r;
}

// Shoelace sum: twice the signed area, negative for a clockwise ring (x right, y up).
inline real twice_signed_area(const std::vector<pt>& r) {
    real s = 0;
    for (std::size_t i = 0; i < r.size(); ++i) {
        const pt& a = r[i];
        const pt& b = r[(i + 1) % r.size()];
        s += a.x * b.y - b.x * a.y;
    }
    return s;
}

// An input polygon must be a closed, clockwise ring with positive area; anything else is outside the shim.
template <typename P>
std::vector<pt> checked_ring(const model::polygon<P>& poly, const char* what) {
    const std::vector<P>& o = poly.outer();
    if (o.size() < 4 || o.front().x() != o.back().x() || o.front().y() != o.back().y()) {
        std::fprintf(stderr, "boost::geometry shim: %s: the polygon is not a closed ring of >= 3 points\n", what);
        std::abort();
    }
    std::vector<pt> r = ring(poly);
    real s = twice_signed_area(r);
    if (!(s < 0)) {
        std::fprintf(stderr, "boost::geometry shim: %s: the polygon is %s (twice its signed area: %Lg); the shim only "
                     "handles clockwise polygons with positive area\n", what, s > 0 ? "counter-clockwise" : "degenerate",
                     s);
        std::abort();
    }
    return r;
}

inline real cross(real ax, real ay, real bx, real by) { return ax * by - ay * bx; }

// Is p inside or on the boundary of the convex clockwise ring r?  tol: a length scale for "on the boundary".
inline bool inside(const std::vector<pt>& r, const pt& p, real tol) {
    for (std::size_t i = 0; i < r.size(); ++i) {
        const pt& a = r[i];
        const pt& b = r[(i + 1) % r.size()];
        real ex = b.x - a.x, ey = b.y - a.y;
        real len = std::sqrt(ex * ex + ey * ey);
        // clockwise: the interior is to the right of every edge, where the cross product is negative
        if (cross(ex, ey, p.x - a.x, p.y - a.y) > tol * len) return false;
    }
    return true;
}

// The intersection of two convex rings: the vertices of each inside the other plus every crossing of two edges,
// merged where they coincide, ordered clockwise around their centroid.  Fewer than three distinct points, or no
// area, is an empty intersection.
inline std::vector<pt> convex_intersection(const std::vector<pt>& a, const std::vector<pt>& b) {
    real scale = 0;
    for (std::size_t i = 0; i < a.size(); ++i) scale = std::max(scale, std::max(std::fabs(a[i].x), std::fabs(a[i].y)));
    for (std::size_t i = 0; i < b.size(); ++i) scale = std::max(scale, std::max(std::fabs(b[i].x), std::fabs(b[i].y)));
    const real tol = (scale > 1 ? scale : real(1)) * 1e-13L;

    std::vector<pt> pts;
    for (std::size_t i = 0; i < a.size(); ++i)
        if (inside(b, a[i], tol)) pts.push_back(a[i]);
    for (std::size_t i = 0; i < b.size(); ++i)
        if (inside(a, b[i], tol)) pts.push_back(b[i]);
    for (std::size_t i = 0; i < a.size(); ++i) {
        const pt& p = a[i];
        const pt& p2 = a[(i + 1) % a.size()];
        real rx = p2.x - p.x, ry = p2.y - p.y;
        for (std::size_t j = 0; j < b.size(); ++j) {
            const pt& q = b[j];
            const pt& q2 = b[(j + 1) % b.size()];
            real sx = q2.x - q.x, sy = q2.y - q.y;
            real d = cross(rx, ry, sx, sy);
            real lr = std::sqrt(rx * rx + ry * ry), ls = std::sqrt(sx * sx + sy * sy);
            if (std::fabs(d) <= 1e-15L * lr * ls) continue;  // parallel: shared stretches come from the vertex tests
            real t = cross(q.x - p.x, q.y - p.y, sx, sy) / d;
            real u = cross(q.x - p.x, q.y - p.y, rx, ry) / d;
            const real et = tol / lr, eu = tol / ls;
            if (t < -et || t > 1 + et || u < -eu || u > 1 + eu) continue;
            pt c = {p.x + t * rx, p.y + t * ry};
            pts.push_back(c);
        }
    }

    std::vector<pt> uniq;
    for (std::size_t i = 0; i < pts.size(); ++i) {
        bool dup = false;
        for (std::size_t k = 0; k < uniq.size() && !dup; ++k)
            dup = std::fabs(uniq[k].x - pts[i].x) <= tol && std::fabs(uniq[k].y - pts[i].y) <= tol;
        if (!dup) uniq.push_back(pts[i]);
    }
    if (uniq.size() < 3) return std::vector<pt>();

    real cx = 0, cy = 0;
    for (std::size_t i = 0; i < uniq.size(); ++i) {
        cx += uniq[i].x;
        cy += uniq[i].y;
    }
    cx /= uniq.size();
    cy /= uniq.size();
    std::vector<std::pair<real, pt> > by_angle;
    for (std::size_t i = 0; i < uniq.size(); ++i)
        by_angle.push_back(std::make_pair(std::atan2(uniq[i].y - cy, uniq[i].x - cx), uniq[i]));
    // descending angle = clockwise
    std::sort(by_angle.begin(), by_angle.end(),
              [](const std::pair<real, pt>& l, const std::pair<real, pt>& r) { return l.first > r.first; });
    std::vector<pt> out;
    for (std::size_t i = 0; i < by_angle.size(); ++i) out.push_back(by_angle[i].second);
    // a sliver thinner than tol (boxes touching along an edge, in rounding) has no area
    if (!(-twice_signed_area(out) > tol * (scale > 1 ? scale : real(1)))) return std::vector<pt>();
    return out;
}

template <typename P>
model::polygon<P> to_polygon(const std::vector<pt>& r) {
    model::polygon<P> poly;
    for (std::size_t i = 0; i <= r.size(); ++i) {
        const pt& p = r[i % r.size()];
        poly.outer().push_back(P((double)p.x, (double)p.y));
    }
    return poly;
}

}  // namespace shim_detail

// append(poly, double[N][2]): the points become the polygon's outer ring as given.
template <typename P, std::size_t N>
void append(model::polygon<P>& poly, const double (&points)[N][2]) {
    for (std::size_t i = 0; i < N; ++i) poly.outer().push_back(P(points[i][0], points[i][1]));
    poly.has_area_ = false;
}

template <typename P>
double area(const model::polygon<P>& poly) {
    if (poly.has_area_) return poly.area_;
    return (double)(-shim_detail::twice_signed_area(shim_detail::checked_ring(poly, "area")) / 2);
}

// out receives the intersection polygon, or nothing when the two share no area.
template <typename P>
void intersection(const model::polygon<P>& a, const model::polygon<P>& b, std::vector<model::polygon<P> >& out) {
    std::vector<shim_detail::pt> r = shim_detail::convex_intersection(shim_detail::checked_ring(a, "intersection"),
                                                                      shim_detail::checked_ring(b, "intersection"));
    if (r.empty()) return;
    model::polygon<P> poly = shim_detail::to_polygon<P>(r);
    poly.has_area_ = true;  // the area of the long double outline, rounded once
    poly.area_ = (double)(-shim_detail::twice_signed_area(r) / 2);
    out.push_back(poly);
}

// The shortcut (see the top of this file): one polygon carrying area(a) + area(b) - area(a intersection b).
template <typename P>
void union_(const model::polygon<P>& a, const model::polygon<P>& b, std::vector<model::polygon<P> >& out) {
    std::vector<shim_detail::pt> ra = shim_detail::checked_ring(a, "union_");
    std::vector<shim_detail::pt> rb = shim_detail::checked_ring(b, "union_");
    std::vector<shim_detail::pt> ri = shim_detail::convex_intersection(ra, rb);
    shim_detail::real inter = ri.empty() ? 0 : -shim_detail::twice_signed_area(ri) / 2;
    model::polygon<P> u = a;
    u.has_area_ = true;
    u.area_ = (double)(-shim_detail::twice_signed_area(ra) / 2 - shim_detail::twice_signed_area(rb) / 2 - inter);
    out.push_back(u);
}

}  // namespace geometry
}  // namespace boost

#endif

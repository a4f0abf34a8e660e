// Reads pairs of boxes and prints the bird's-eye-view and 3D IoU the shim's geometry gives them, computed the way
// KITTI's evaluator does (rotated l x w rectangle in the x-z plane; volume overlap over the y extent [ty - h, ty]).
// Each stdin line: l w h tx ty tz ry of box a, then of box b.  Each stdout line: "<bev iou> <3d iou>" as %.17g.
// Test infrastructure for tests/test_kitti_eval_shim.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include <boost/geometry.hpp>

typedef boost::geometry::model::d2::point_xy<double> Point;
typedef boost::geometry::model::polygon<Point> Polygon;

struct Box {
    double l, w, h, tx, ty, tz, ry;
};

static Polygon footprint(const Box& b) {
    const double c = std::cos(b.ry), s = std::sin(b.ry);
    const double x[4] = {b.l / 2, b.l / 2, -b.l / 2, -b.l / 2};
    const double z[4] = {b.w / 2, -b.w / 2, -b.w / 2, b.w / 2};
    double pts[5][2];
    for (int i = 0; i < 5; ++i) {
        pts[i][0] = c * x[i % 4] + s * z[i % 4] + b.tx;
        pts[i][1] = -s * x[i % 4] + c * z[i % 4] + b.tz;
    }
    Polygon p;
    boost::geometry::append(p, pts);
    return p;
}

int main() {
    Box a, b;
    while (std::scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf", &a.l, &a.w, &a.h, &a.tx, &a.ty, &a.tz,
                      &a.ry, &b.l, &b.w, &b.h, &b.tx, &b.ty, &b.tz, &b.ry) == 14) {
        Polygon pa = footprint(a), pb = footprint(b);
        std::vector<Polygon> in, un;
        boost::geometry::intersection(pa, pb, in);
        boost::geometry::union_(pa, pb, un);
        const double inter = in.empty() ? 0 : boost::geometry::area(in.front());
        const double bev = inter / boost::geometry::area(un.front());
        const double dy = std::max(0.0, std::min(a.ty, b.ty) - std::max(a.ty - a.h, b.ty - b.h));
        const double iv = inter * dy;
        const double iou3d = iv / (a.h * a.l * a.w + b.h * b.l * b.w - iv);
        std::printf("%.17g %.17g\n", bev, iou3d);
    }
    return 0;
}

// boost-free stand-in for boost::geometry::model::d2::point_xy (see boost/geometry.hpp of this shim).
#ifndef REF_EVAL_SHIM_GEOMETRY_POINT_XY_HPP
#define REF_EVAL_SHIM_GEOMETRY_POINT_XY_HPP

namespace boost {
namespace geometry {
namespace model {
namespace d2 {

template <typename T>
class point_xy {
public:
    point_xy() : x_(T()), y_(T()) {}
    point_xy(T x, T y) : x_(x), y_(y) {}
    T x() const { return x_; }
    T y() const { return y_; }
    void x(T v) { x_ = v; }
    void y(T v) { y_ = v; }

private:
    T x_, y_;
};

}  // namespace d2
}  // namespace model
}  // namespace geometry
}  // namespace boost

#endif

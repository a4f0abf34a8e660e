// boost-free stand-in for boost::geometry::model::polygon (see boost/geometry.hpp of this shim).
#ifndef REF_EVAL_SHIM_GEOMETRY_POLYGON_HPP
#define REF_EVAL_SHIM_GEOMETRY_POLYGON_HPP

#include <vector>

namespace boost {
namespace geometry {
namespace model {

// One outer ring, clockwise and closed (the first point repeated at the end), boost's default polygon type.
// No inner rings: the evaluator never makes any.
template <typename P>
class polygon {
public:
    typedef P point_type;
    polygon() : has_area_(false), area_(0) {}
    std::vector<P>& outer() { return outer_; }
    const std::vector<P>& outer() const { return outer_; }
    void clear() { outer_.clear(); has_area_ = false; }

    // Set by the shim's intersection and union_ (boost/geometry.hpp): the area the result carries.
    bool has_area_;
    double area_;

private:
    std::vector<P> outer_;
};

}  // namespace model
}  // namespace geometry
}  // namespace boost

#endif

// A boost-free stand-in for the part of boost::numeric::ublas that KITTI's evaluate_object_3d_offline.cpp uses
// (toPolygon: a 2x2 rotation times the 2x4 corner matrix).  Test infrastructure only; see oracle/ref_eval/README.md.
#ifndef REF_EVAL_SHIM_UBLAS_MATRIX_HPP
#define REF_EVAL_SHIM_UBLAS_MATRIX_HPP

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace boost {
namespace numeric {
namespace ublas {

// Dense row-major matrix: data() holds element (i, j) at i * cols + j, as ublas's default row_major layout does.
template <typename T>
class matrix {
public:
    matrix() : rows_(0), cols_(0) {}
    matrix(std::size_t rows, std::size_t cols) : rows_(rows), cols_(cols), data_(rows * cols, T()) {}
    std::size_t size1() const { return rows_; }
    std::size_t size2() const { return cols_; }
    T& operator()(std::size_t i, std::size_t j) { return data_[i * cols_ + j]; }
    const T& operator()(std::size_t i, std::size_t j) const { return data_[i * cols_ + j]; }
    std::vector<T>& data() { return data_; }
    const std::vector<T>& data() const { return data_; }

private:
    std::size_t rows_, cols_;
    std::vector<T> data_;
};

// ublas's matrix_matrix_prod: t = 0; for k: t += a(i, k) * b(k, j) -- every product rounded, summed in k order.
template <typename T>
matrix<T> prod(const matrix<T>& a, const matrix<T>& b) {
    if (a.size2() != b.size1()) {
        std::fprintf(stderr, "ublas shim: prod of %zux%zu and %zux%zu\n", a.size1(), a.size2(), b.size1(), b.size2());
        std::abort();
    }
    matrix<T> out(a.size1(), b.size2());
    for (std::size_t i = 0; i < a.size1(); ++i)
        for (std::size_t j = 0; j < b.size2(); ++j) {
            T t = T(0);
            for (std::size_t k = 0; k < a.size2(); ++k) t += a(i, k) * b(k, j);
            out(i, j) = t;
        }
    return out;
}

}  // namespace ublas
}  // namespace numeric
}  // namespace boost

#endif

// boost-free stand-in: the evaluator includes ublas's stream operators but never uses them.
#ifndef REF_EVAL_SHIM_UBLAS_IO_HPP
#define REF_EVAL_SHIM_UBLAS_IO_HPP
#include <boost/numeric/ublas/matrix.hpp>
#endif

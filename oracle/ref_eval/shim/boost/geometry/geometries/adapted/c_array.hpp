// boost-free stand-in: the shim's append() takes double[N][2] directly, so registering C arrays as points is a no-op.
#ifndef REF_EVAL_SHIM_GEOMETRY_C_ARRAY_HPP
#define REF_EVAL_SHIM_GEOMETRY_C_ARRAY_HPP
#define BOOST_GEOMETRY_REGISTER_C_ARRAY_CS(cs)
#endif

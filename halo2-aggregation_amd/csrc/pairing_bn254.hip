// pairing_bn254.hip -- the BN254 pairing decider's kernels and their driver
// (DESIGN §10g).  A translation unit of its own: nothing here goes through
// make_curve_ops or the per-curve instantiations.
#define PM_PAIRING_IMPL
#include "pairing_engine.hpp"

// pairing_batch_bn254.hip -- the batch decider's kernels and their driver
// (DESIGN §10h).  A translation unit of its own: the code objects of the
// per-curve instantiations and of pairing_bn254.hip do not change with it.
#define PM_PAIRING_BATCH_IMPL
#include "pairing_batch_engine.hpp"

// pairing_fq.hpp -- the BN254 base field in the kernels' radix-2^29 form, as the
// pairing decider's kernels name it (pairing_kernels.hpp, pairing_g1.hpp).
#pragma once
#include "fp29.hpp"
#include "pairing_plan.hpp"

namespace pm {
namespace pairing {

using Fq = Bn254Fq;
using F = F29<Fq>;
using KQ = F29Consts<Fq>;

__device__ __forceinline__ F fq_one() { return f29_const<Fq>(KQ::ONE); }

}  // namespace pairing
}  // namespace pm

// quotient_kernels.hpp -- the quotient numerator on the extended domain
// (pm_quotient_device): halo2's evaluate_h, the input of
// vanishing::Argument::construct [3P plonk/prover.rs], between
// pm_coeff_to_extended_device and pm_extended_to_coeff_device.
//
// k_quot_eval runs the program of quotient_plan.hpp once per extended row j,
// one row per lane, blocks of one wave.  The program, the leaf table, the
// pointer table and the constants are read at wave-uniform addresses and every
// branch is on a program word, so no lane diverges; only the lanes of a last,
// partial wave (N < 64) leave at the top.  Value slots live in LDS laid out
// [slot][limb][lane]: a wave's 64 lanes read 64 consecutive words, one per
// bank.  The fold register h stays in VGPRs.
//
// Arithmetic (as gp_kernels.hpp).  f29_mul_c(a, b) = a b 2^-261; the forms of
// the operands are the compiler's business (the deficits of quotient_plan.hpp),
// the kernel only multiplies.  Bounds: every slot and h hold Norm values < 3p.
//   * a leaf is a packed column word < 2^256 (< 5.4p; canonical by contract),
//     reduced once (f29_reduce3: < 16p -> < 3p); a constant is canonical;
//   * a product takes two Norm operands < 3p and is Norm, < 2p;
//   * a sum is < 6p with limbs < 2^30, a difference a + 6p - b < 9p with limbs
//     < 2^29 + 2^30 (K6 dominates the limbs of any Norm b < 3p), the fold
//     h y + e < 5p: each is normalised and reduced (f29_nr) to Norm, < 3p
//     before it is stored.
// Every f29_mul_c therefore takes two Norm operands below 6p, an operand shape
// tests/test_fp29_asm.py pins.  The row's h is canonicalised and stored once.
#pragma once
#include "domain_kernels.hpp"
#include "quotient_plan.hpp"

namespace pm {

constexpr int kQuotThreads = 64;
constexpr size_t kQuotSlotBytes = 9 * 4 * kQuotThreads;  // LDS per value slot and block

struct QuotArgs {
  const uint32_t* prog;
  const uint32_t* leaves;          // per leaf: pointer slot, row offset
  const uint32_t* const* ptrs;     // the call's column pointers, then the quotient's own columns
  const uint32_t* consts;          // 8 words each, canonical
  const uint32_t* t;               // t[j mod 2^e], R = 2^261 canonical (pm_domain's table)
  uint32_t* out;
  uint32_t nops, n, tmask, y_const;
  uint32_t divide, accumulate;
};

template <class Fs>
__device__ __forceinline__ F29<Fs> quot_lds_ld(const uint32_t* sm, uint32_t slot) {
  F29<Fs> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = sm[(slot * 9 + k) * kQuotThreads + threadIdx.x];
  return r;
}
template <class Fs>
__device__ __forceinline__ void quot_lds_st(uint32_t* sm, uint32_t slot, const F29<Fs>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) sm[(slot * 9 + k) * kQuotThreads + threadIdx.x] = v.l[k];
}

template <class Fs>
__global__ void __launch_bounds__(kQuotThreads) k_quot_eval(QuotArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  using K = F29Consts<Fs>;
  const uint32_t j = blockIdx.x * kQuotThreads + threadIdx.x;
  if (j >= a.n) return;
  const uint32_t mask = a.n - 1;
  const F29<Fs> y = g_ld29<Fs>(a.consts, a.y_const);
  F29<Fs> h = a.accumulate ? f29_reduce3<Fs>(g_ld29<Fs>(a.out, j)) : f29_zero<Fs>();
  for (uint32_t pc = 0; pc < a.nops; pc++) {
    const uint32_t w = a.prog[pc];
    const uint32_t op = w & 7u, cb = w & kQConstB, dst = (w >> 4) & 63u, sa = (w >> 10) & 63u, b = w >> 16;
    if (op == kQLoad) {
      const uint32_t* col = a.ptrs[a.leaves[2 * b]];
      const uint32_t row = (j + a.leaves[2 * b + 1]) & mask;  // < n <= 2^28
      quot_lds_st<Fs>(sm, dst, f29_reduce3<Fs>(g_ld29<Fs>(col, row)));
      continue;
    }
    if (op == kQConst) {
      quot_lds_st<Fs>(sm, dst, g_ld29<Fs>(a.consts, b));
      continue;
    }
    const F29<Fs> x = quot_lds_ld<Fs>(sm, sa);
    if (op == kQFold && b && !a.accumulate) {
      h = x;
      continue;
    }
    F29<Fs> z = y;  // the second operand
    if (op != kQFold && op != kQNeg) z = cb ? g_ld29<Fs>(a.consts, b) : quot_lds_ld<Fs>(sm, b & 63u);
    F29<Fs> r;
    if (op == kQMul || op == kQFold) {
      r = f29_mul_c<Fs>(op == kQFold ? h : x, z);
      if (op == kQFold) {
        h = f29_nr<Fs>(f29_add<Fs>(r, x));
        continue;
      }
    } else if (op == kQAdd) {
      r = f29_nr<Fs>(f29_add<Fs>(x, z));
    } else if (op == kQSub) {
      r = cb ? f29_nr<Fs>(f29_sub<Fs>(z, x, K::K6)) : f29_nr<Fs>(f29_sub<Fs>(x, z, K::K6));
    } else {  // kQNeg
      r = f29_nr<Fs>(f29_sub<Fs>(f29_zero<Fs>(), x, K::K6));
    }
    quot_lds_st<Fs>(sm, dst, r);
  }
  if (a.divide) h = f29_mul_c<Fs>(h, g_ld29<Fs>(a.t, j & a.tmask));
  g_st29<Fs>(a.out, j, f29_canon<Fs>(h));
}

}  // namespace pm

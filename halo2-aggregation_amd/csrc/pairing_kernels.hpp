// pairing_kernels.hpp -- BN254 pairing decider on the device.
//
//   k_pairing_prep   one lane per item: the points R256 -> F29, the curve check,
//                    for an accumulator quad C = -(zw + f + e) with the complete
//                    affine group law (one f29_inv per addition);
//   k_pairing_run    pairing_plan.hpp's program: Miller loop of the product
//                    e(A, s_g2) e(C, g2) and the final exponentiation.
//
// k_pairing_run holds an Fp12 value as six Fp2 coefficients of
// Fp2[w] / (w^6 - xi), coefficient k in lane k of a group of 6 lanes, and the
// program's registers in LDS, limb-major.  A lane computes ITS coefficient of
// every result: six independent Fp2 products for a product, two and a scaling
// for a line, one for a Frobenius.  Operands of other lanes are read from LDS
// (a group reading one coefficient is a broadcast); between an operation's reads
// and its write, and after the write, the block (one wave) meets at a barrier.
// Line coefficients and the program are uniform: scalar loads.
//
// Lazy bounds (fp29.hpp; for BN254 R = 2^261 > 169 p).  Every value kept in LDS
// is Norm and < 3p.  An Fp2 product is two f29_mul2 (a b + u v < 99 p^2, all
// four Norm) with the subtraction folded in as a product by K6 - b1 < 6p:
// 3p 3p + 3p 6p = 27 p^2; with a conjugated first operand (< 6p) and a constant
// (< p) second one 6p p + 6p 6p = 42 p^2.  Sums of products are limb-wise
// (at most 7 terms below 2^29: no limb overflow) and go through
// f29_norm + f29_reduce3 (< 16p -> < 3p) before they enter the next product.
#pragma once
#include "fp29.hpp"
#include "pairing_fq.hpp"
#include "pairing_plan.hpp"

namespace pm {
namespace pairing {

struct F2 {
  F c0, c1;
};

// limbs < 2^32 - 8, value < 16p -> Norm, < 3p
__device__ __forceinline__ F fq_red(const F& a) { return f29_reduce3<Fq>(f29_norm<Fq>(a)); }
// a Norm, < 6p -> 6p - a: Norm, in (0, 6p] (K6's limbs dominate a's)
__device__ __forceinline__ F fq_negn(const F& a) {
  F r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = KQ::K6[i] - a.l[i];
  return f29_norm<Fq>(r);
}

// a, b Norm with a0 b0 + a1 (6p) < 99 p^2 (see the header) -> both parts Norm, < 2p
__device__ __forceinline__ F2 fq2_mul(const F2& a, const F2& b) {
  const F nb1 = fq_negn(b.c1);
  F2 r;
  r.c0 = f29_mul2_c<Fq>(a.c0, b.c0, a.c1, nb1);
  r.c1 = f29_mul2_c<Fq>(a.c0, b.c1, a.c1, b.c0);
  return r;
}

// lo + xi hi, xi = 9 + u.  lo: limb-wise sums of at most 6 values < 2p plus
// nothing else (< 12p); hi: of at most 5 (< 10p).  -> Norm, < 3p.
// xi (h0 + h1 u) = (9 h0 - h1) + (9 h1 + h0) u, with 9 h as 2 (4 h reduced) + h.
__device__ __forceinline__ F2 fq2_fold_xi(const F2& lo, const F2& hi) {
  const F h0 = fq_red(hi.c0), h1 = fq_red(hi.c1);  // < 3p
  F t0, t1;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    t0.l[i] = h0.l[i] << 2;  // < 12p, limbs < 2^31
    t1.l[i] = h1.l[i] << 2;
  }
  const F q0 = fq_red(t0), q1 = fq_red(t1);  // 4 h, < 3p
  F n0, n1;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    n0.l[i] = 2u * q0.l[i] + h0.l[i] + (KQ::K6[i] - h1.l[i]);  // 9 h0 - h1 + 6p: < 15p, limbs < 2^32 - 8
    n1.l[i] = 2u * q1.l[i] + h1.l[i] + h0.l[i];                // 9 h1 + h0: < 12p
  }
  const F x0 = fq_red(n0), x1 = fq_red(n1);  // < 3p
  F2 r;
  r.c0 = fq_red(f29_add<Fq>(lo.c0, x0));  // < 12p + 3p
  r.c1 = fq_red(f29_add<Fq>(lo.c1, x1));
  return r;
}

// ---- LDS registers: value v, limb i, lane l at [(v * 9 + i) * 64 + l]
__device__ __forceinline__ F lds_get(const uint32_t* s, int lane) {
  F r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = s[i * kPairWave + lane];
  return r;
}
__device__ __forceinline__ void lds_put(uint32_t* s, int lane, const F& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) s[i * kPairWave + lane] = a.l[i];
}
__device__ __forceinline__ F2 slot_get(const uint32_t* lds, uint32_t slot, int lane) {
  const uint32_t* s = lds + slot * kSlotWords;
  F2 r;
  r.c0 = lds_get(s, lane);
  r.c1 = lds_get(s + 9 * kPairWave, lane);
  return r;
}
__device__ __forceinline__ void slot_put(uint32_t* lds, uint32_t slot, int lane, const F2& a) {
  uint32_t* s = lds + slot * kSlotWords;
  lds_put(s, lane, a.c0);
  lds_put(s + 9 * kPairWave, lane, a.c1);
}
__device__ __forceinline__ F glb_get(const uint32_t* p) {
  F r;
#pragma unroll
  for (int i = 0; i < 9; i++) r.l[i] = p[i];
  return r;
}
// r += t where m is all ones, limb-wise
__device__ __forceinline__ void acc_masked(F2& r, const F2& t, uint32_t m) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    r.c0.l[i] += t.c0.l[i] & m;
    r.c1.l[i] += t.c1.l[i] & m;
  }
}
__device__ __forceinline__ F2 f2_zero() {
  F2 r;
  r.c0 = f29_zero<Fq>();
  r.c1 = f29_zero<Fq>();
  return r;
}

// tab: pm_pairing's device words (lines, Frobenius constants, program);
// items: k_pairing_prep's output; out_ok: B x u32; out_gt: B x 48 x u64 or null
__global__ __launch_bounds__(kPairBlock) void k_pairing_run(uint32_t B, const uint32_t* __restrict__ tab,
                                                            const uint32_t* __restrict__ items,
                                                            uint32_t* __restrict__ out_ok,
                                                            uint64_t* __restrict__ out_gt) {
  __shared__ uint32_t lds[kLdsWords];
  uint32_t* const pts = lds + kSlots * kSlotWords;
  uint32_t* const flg = pts + kPointWords;
  const int lane = (int)threadIdx.x;
  // lanes 60..63 repeat coefficients 0..3 of the wave's last group: every lane
  // holds valid field values at every barrier; they write their own LDS columns,
  // which no lane reads, and store nothing to global memory
  const int grp = lane < kPairG * kPairPerWave ? lane / kPairG : kPairPerWave - 1;
  const int base = grp * kPairG;
  const int k = lane < kPairG * kPairPerWave ? lane - base : lane - kPairG * kPairPerWave;
  const size_t item = (size_t)blockIdx.x * kPairPerBlock + (size_t)grp;
  const bool live = lane < kPairG * kPairPerWave && item < B;
  const uint32_t* it = items + (item < B ? item : (size_t)B - 1) * kItemWords;  // B >= 1
  const uint32_t flags = it[4 * 9];
#pragma unroll
  for (int v = 0; v < 4; v++) lds_put(pts + v * 9 * kPairWave, lane, glb_get(it + v * 9));
  {
    F2 one = f2_zero();
    if (k == 0) one.c0 = fq_one();
    slot_put(lds, 0, lane, one);
  }
  __syncthreads();

  const uint32_t* const frob = tab + kTableWords29;
  const uint32_t* const prog = frob + kFrobWords29;
  for (int pc = 0; pc < kProgOps; pc++) {
    const uint32_t w = prog[pc], d = op_d(w), a = op_a(w), b = op_b(w);
    F2 r;
    uint32_t dst = d;
    switch (op_code(w)) {
      case kOpMul: {
        F2 lo = f2_zero(), hi = f2_zero();
#pragma unroll 2
        for (int i = 0; i < 6; i++) {
          const bool wrap = i > k;
          const int j = k - i + (wrap ? 6 : 0);
          const F2 t = fq2_mul(slot_get(lds, a, base + i), slot_get(lds, b, base + j));  // 27 p^2
          const uint32_t m = wrap ? ~0u : 0u;
          acc_masked(hi, t, m);
          acc_masked(lo, t, ~m);
        }
        r = fq2_fold_xi(lo, hi);
        break;
      }
      case kOpLine: {
        dst = 0;
        const uint32_t* lc = tab + a * kStepWords29 + b * (kLineFp * 9);
        const bool inf = (flags >> b) & 1u;  // kFlagAInf, kFlagCInf: x = 0, y = 1 and no w^3 term: the line is 1
        const F xp = lds_get(pts + (2 * b) * 9 * kPairWave, lane), yp = lds_get(pts + (2 * b + 1) * 9 * kPairWave, lane);
        const F nx = fq_negn(xp);  // -x_P, < 6p
        F2 l1, l3;
        l1.c0 = f29_mul_c<Fq>(glb_get(lc), nx);  // lambda < p: 6 p^2
        l1.c1 = f29_mul_c<Fq>(glb_get(lc + 9), nx);
        l3.c0 = glb_get(lc + 18);
        l3.c1 = glb_get(lc + 27);
        const uint32_t keep = inf ? 0u : ~0u;
#pragma unroll
        for (int i = 0; i < 9; i++) {
          l3.c0.l[i] &= keep;
          l3.c1.l[i] &= keep;
        }
        const F2 ak = slot_get(lds, 0, lane);
        const F2 t1 = fq2_mul(slot_get(lds, 0, base + (k + 5) % 6), l1);
        const F2 t3 = fq2_mul(slot_get(lds, 0, base + (k + 3) % 6), l3);
        F2 lo, hi = f2_zero();
        lo.c0 = f29_mul_c<Fq>(ak.c0, yp);  // y_P < p
        lo.c1 = f29_mul_c<Fq>(ak.c1, yp);
        const uint32_t m1 = k < 1 ? ~0u : 0u, m3 = k < 3 ? ~0u : 0u;
        acc_masked(hi, t1, m1);
        acc_masked(lo, t1, ~m1);
        acc_masked(hi, t3, m3);
        acc_masked(lo, t3, ~m3);
        r = fq2_fold_xi(lo, hi);
        break;
      }
      case kOpFrob: {
        F2 x = slot_get(lds, a, lane);
        if (b & 1u) x.c1 = fq_negn(x.c1);  // conjugate: < 6p
        const uint32_t* g = frob + ((b - 1) * 6 + k) * 18;
        F2 c;
        c.c0 = glb_get(g);
        c.c1 = glb_get(g + 9);
        r = fq2_mul(x, c);  // 42 p^2
        break;
      }
      case kOpConj: {
        r = slot_get(lds, a, lane);
        if (k & 1) {
          r.c0 = f29_reduce3<Fq>(fq_negn(r.c0));
          r.c1 = f29_reduce3<Fq>(fq_negn(r.c1));
        }
        break;
      }
      default: {  // kOpScaleInv: 1 / (n0 + n1 u) = (n0 - n1 u) / (n0^2 + n1^2)
        const F2 n = slot_get(lds, b, base);
        const F di = f29_inv<Fq>(f29_mul2_c<Fq>(n.c0, n.c0, n.c1, n.c1));  // 18 p^2; < 2p
        F2 ni;
        ni.c0 = f29_mul_c<Fq>(n.c0, di);
        ni.c1 = f29_mul_c<Fq>(fq_negn(n.c1), di);  // 12 p^2
        r = fq2_mul(slot_get(lds, a, lane), ni);
        break;
      }
    }
    __syncthreads();  // every lane has read its operands
    slot_put(lds, dst, lane, r);
    __syncthreads();
  }

  // canonical R = 2^256 words of this lane's coefficient; the group's decision
  const F2 g = slot_get(lds, 0, lane);
  uint32_t w0[8], w1[8];
  f29_to_r256<Fq>(g.c0, w0);
  f29_to_r256<Fq>(g.c1, w1);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) diff |= (w0[i] ^ (k == 0 ? Fq::ONE[i] : 0u)) | w1[i];
  flg[lane] = diff;
  __syncthreads();
  const bool skip = flags & kFlagSkip;
  if (live && k == 0) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < kPairG; i++) any |= flg[base + i];
    out_ok[item] = (!skip && any == 0) ? 1u : 0u;
  }
  if (live && out_gt) {
    // the ABI's order c0.c0.c0 .. c1.c2.c1: tower c_i.c_j is w^(2 j + i)
    uint64_t* o = out_gt + item * 48 + (size_t)(((k & 1) * 3 + (k >> 1)) * 8);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      o[i] = skip ? 0ull : ((uint64_t)w0[2 * i] | ((uint64_t)w0[2 * i + 1] << 32));
      o[4 + i] = skip ? 0ull : ((uint64_t)w1[2 * i] | ((uint64_t)w1[2 * i + 1] << 32));
    }
  }
}

}  // namespace pairing
}  // namespace pm

// ---- k_pairing_prep.  G1 in affine form is shared with the batch decider's prep
// kernel; it is included here, after k_pairing_run, so that this unit's code
// object keeps its order of functions.
#include "pairing_g1.hpp"

namespace pm {
namespace pairing {

// in: B x NP x 8 u64 (NP = 4: quads w, zw, f, e; NP = 2: pairs A, C);
// items: B x kItemWords; status_in / status_out may be null, and may be one buffer
template <bool QUAD>
__global__ __launch_bounds__(kPrepBlock) void k_pairing_prep(uint32_t B, const uint64_t* __restrict__ in,
                                                             const uint32_t* status_in,
                                                             uint32_t* __restrict__ items, uint32_t* status_out) {
  const size_t i = (size_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (i >= B) return;
  constexpr int NP = QUAD ? 4 : 2;
  uint32_t st = status_in ? status_in[i] : 0u;
  G1a A, C;
  A.x = C.x = f29_zero<Fq>();
  A.y = C.y = fq_one();
  A.inf = C.inf = true;
  if (st == 0) {  // a non-zero word is passed through and nothing is evaluated
    const uint64_t* p = in + i * (NP * 8);
    A = g1_load(p);
    if (!g1_on_curve(A)) st |= kNotOnCurveBit;
    C = g1_load(p + 8);
    if (!g1_on_curve(C)) st |= kNotOnCurveBit;
    if (QUAD) {
#pragma unroll 1
      for (int t = 2; t < 4; t++) {
        const G1a q = g1_load(p + 8 * t);
        if (!g1_on_curve(q)) st |= kNotOnCurveBit;
        if (st == 0) C = g1_add(C, q);
      }
      if (!C.inf) C.y = fq_subc(f29_zero<Fq>(), C.y);
    }
  }
  uint32_t flags = (A.inf ? kFlagAInf : 0u) | (C.inf ? kFlagCInf : 0u);
  if (st) flags = kFlagAInf | kFlagCInf | kFlagSkip;
  if (flags & kFlagAInf) A.x = f29_zero<Fq>(), A.y = fq_one();
  if (flags & kFlagCInf) C.x = f29_zero<Fq>(), C.y = fq_one();
  uint32_t* o = items + i * kItemWords;
#pragma unroll
  for (int l = 0; l < 9; l++) {
    o[l] = A.x.l[l];
    o[9 + l] = A.y.l[l];
    o[18 + l] = C.x.l[l];
    o[27 + l] = C.y.l[l];
  }
  o[36] = flags;
  if (status_out) status_out[i] = st;
}

}  // namespace pairing
}  // namespace pm

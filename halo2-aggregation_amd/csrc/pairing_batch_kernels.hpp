// pairing_batch_kernels.hpp -- the batch decider's fold on the device.
//
//   k_batch_prep    one lane per item: the four points R256 -> F29 and the curve
//                   checks, C = -(zw + f + e) by the complete affine law
//                   (pairing_g1.hpp, as k_pairing_prep), the coefficient r_i by
//                   one Blake2b compression and its 33 signed 4-bit digits.
//                   Writes the bases (w_i, C_i) in the packed R = 2^261 form
//                   (all-zero words: the identity), the digits and the status.
//   k_small_table   msm_small.hpp's, over the 2n bases: the multiples [1..8]P.
//   k_batch_sum     block (s, j, o): slice s of window j of output o (0: L over
//                   the w_i, 1: R over the C_i).  Base 2i + o of item i takes
//                   digit j of r_i: both outputs read one digit array.  Quad v
//                   adds kq table entries (quad-cooperative XYZZ additions), an
//                   LDS tree folds the 64 quads, and with ns > 1 the last block
//                   of (j, o) (atomic ticket) folds the ns partials.  The
//                   window sums go out Jacobian, R = 2^256, into mapped host
//                   memory; the host runs the Horner tail.
// No GLV split: a 128-bit coefficient already has half length.
//
// Lazy bounds.  k_batch_prep keeps every coordinate canonical (pairing_g1.hpp).
// k_batch_sum keeps curve29.hpp's: table entries and sums are Norm with
// X, Y < 3p and ZZ, ZZZ < 2p; a negated entry is 6p - Y in (3p, 6p], Norm, and
// f29_reduce3 brings it below 3p before it enters xyzz29_add_q.
#pragma once
#include "msm_small.hpp"
#include "pairing_batch_plan.hpp"
#include "pairing_g1.hpp"

namespace pm {
namespace pairing {

struct BatchSeed {
  uint64_t w[4];
};
struct BatchGeom {
  uint32_t n;   // items of this chunk
  uint32_t kq;  // terms per quad and slice
  uint32_t ns;  // slices per (window, output)
};

// quads: n x 4 x 8 u64 of this chunk; i0: the chunk's first item (r_i is derived
// from the item's index in the whole batch); bases: n x 2 x 16 u32; digits:
// [window][n]; status_in / status_out may be null, and may be one buffer;
// any_bad: one word in mapped host memory, set when an item has a status
__global__ __launch_bounds__(kPrepBlock) void k_batch_prep(uint32_t n, uint64_t i0, BatchSeed seed,
                                                           const uint64_t* __restrict__ quads,
                                                           const uint32_t* status_in, uint32_t* __restrict__ bases,
                                                           int8_t* __restrict__ digits, uint32_t* status_out,
                                                           uint32_t* __restrict__ any_bad) {
  const size_t i = (size_t)blockIdx.x * kPrepBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t st = status_in ? status_in[i] : 0u;
  G1a A, C;
  A.x = C.x = A.y = C.y = f29_zero<Fq>();
  A.inf = C.inf = true;
  if (st == 0) {  // a non-zero word is passed through and nothing is evaluated
    const uint64_t* p = quads + i * 32;
    A = g1_load(p);
    if (!g1_on_curve(A)) st |= kNotOnCurveBit;
    C = g1_load(p + 8);
    if (!g1_on_curve(C)) st |= kNotOnCurveBit;
#pragma unroll 1
    for (int t = 2; t < 4; t++) {
      const G1a q = g1_load(p + 8 * t);
      if (!g1_on_curve(q)) st |= kNotOnCurveBit;
      if (st == 0) C = g1_add(C, q);
    }
    if (!C.inf) C.y = fq_subc(f29_zero<Fq>(), C.y);
  }
  if (st) A.inf = C.inf = true;  // contributes nothing
  if (A.inf) A.x = A.y = f29_zero<Fq>();
  if (C.inf) C.x = C.y = f29_zero<Fq>();
  uint4* o = reinterpret_cast<uint4*>(bases + i * 32);
  st29<Fq>(o, A.x);  // canonical: packs into 8 words; zero packs to zero words
  st29<Fq>(o + 2, A.y);
  st29<Fq>(o + 4, C.x);
  st29<Fq>(o + 6, C.y);
  uint64_t r[2] = {0, 0};
  if (st == 0) batch_coef(seed.w, i0 + i, r);
  batch_recode(r, digits + i, n);
  if (status_out) status_out[i] = st;
  if (st) *(volatile uint32_t*)any_bad = 1u;  // every writer stores the same word
}

// table entry of base t with digit d != 0: [|d|] P_t, negated for d < 0
__device__ __forceinline__ Xyzz29<Fq> batch_term(const Xyzz<Fq>* __restrict__ tab, uint32_t t, int d) {
  Xyzz29<Fq> P = load_xyzz29<Fq>(&tab[(size_t)t * kSmallMults + (uint32_t)(d < 0 ? -d : d) - 1u]);
  if (d < 0) P.Y = f29_reduce3<Fq>(f29_norm<Fq>(f29_sub<Fq>(f29_zero<Fq>(), P.Y, KQ::K6)));  // < 3p
  return P;
}

// tab: k_small_table's rows over the 2n bases; digits: [window][n]; part:
// kBatchSlots x ns partials; tickets: kBatchSlots words, zero on entry; out:
// kBatchSlots window sums, slot o * kBatchWin + j
__global__ __launch_bounds__(256) void k_batch_sum(BatchGeom g, const Xyzz<Fq>* __restrict__ tab,
                                                   const int8_t* __restrict__ digits, Xyzz<Fq>* __restrict__ part,
                                                   uint32_t* __restrict__ tickets, Xyzz<Fq>* __restrict__ out) {
  static_assert(kBatchQuads == kSmallQuads, "small_tree folds kSmallQuads quads");
  __shared__ uint32_t s_p[kBatchQuads][kSmallPt];
  __shared__ uint32_t last;
  const uint32_t s = blockIdx.x, j = blockIdx.y, o = blockIdx.z, v = threadIdx.x >> 2, q = threadIdx.x & 3u;
  const uint32_t slot = o * kBatchWin + j;
  const uint32_t t0 = s * g.kq * kBatchQuads;  // < n: batch_plan leaves no empty slice
  const int8_t* dj = digits + (size_t)j * g.n;
  Xyzz29<Fq> acc = xyzz29_inf<Fq>();
  for (uint32_t r = 0; r < g.kq; r++) {
    const uint32_t i = t0 + r * kBatchQuads + v;
    if (i >= g.n) break;  // quad-uniform
    const int d = dj[i];
    if (d != 0) acc = xyzz29_add_q<Fq>(acc, batch_term(tab, 2u * i + o, d));
  }
  // quads holding at least one item
  const uint32_t active = g.n - t0 >= (uint32_t)kBatchQuads ? (uint32_t)kBatchQuads : g.n - t0;
  acc = small_tree<Fq>(s_p, acc, v, q, small_pow2(active));
  if (g.ns > 1) {
    // park the slice's partial; the last block of this slot folds the ns of them
    if (v == 0) {
      store_xyzz29_q<Fq>(&part[(size_t)slot * g.ns + s], acc, q);
      __threadfence();
      if (q == 0) last = atomicAdd(&tickets[slot], 1u) == g.ns - 1u;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    acc = xyzz29_inf<Fq>();
    for (uint32_t u = v; u < g.ns; u += kBatchQuads)
      acc = xyzz29_add_q<Fq>(acc, load_xyzz29<Fq>(&part[(size_t)slot * g.ns + u]));
    acc = small_tree<Fq>(s_p, acc, v, q, small_pow2(g.ns < (uint32_t)kBatchQuads ? g.ns : (uint32_t)kBatchQuads));
  }
  if (v == 0) store_jac_r256_q<Fq>(&out[slot], acc, q);
}

}  // namespace pairing
}  // namespace pm

// pairing_batch_host.hpp -- host side of the batch decider: the
// Horner tail over the device's window sums, the fold on the CPU
// (pm_accum_decide_batch_host: the parity form and the CPU baseline) and the one
// pairing product of the decision.  HIP-free.  Field values are Montgomery
// R = 2^256 and canonical, as in pairing_host.hpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "pairing_batch_plan.hpp"
#include "pairing_host.hpp"

namespace pm {
namespace pairing {

using J1 = host::Jac<Fq>;

inline J1 j1_inf() {
  J1 r;
  memset(&r, 0, sizeof(r));
  return r;
}
inline J1 j1_from(const G1& p) {
  if (p.inf) return j1_inf();
  J1 r;
  r.X = p.x, r.Y = p.y, r.Z = e1_one();
  return r;
}
inline J1 j1_neg(const J1& p) {
  J1 r = p;
  r.Y = e1_neg(p.Y);
  return r;
}
// Jacobian -> affine; the identity (Z = 0) -> inf
inline G1 j1_affine(const J1& p) {
  if (host::is_zero(p.Z)) return G1{e1_zero(), e1_zero(), true};
  const E1 zi = e1_inv(p.Z), zi2 = e1_mul(zi, zi);
  return G1{e1_mul(p.X, zi2), e1_mul(p.Y, e1_mul(zi2, zi)), false};
}
// the ABI's 8 words, (0, 0) for the identity
inline void g1_to_words(const G1& p, uint64_t out[8]) {
  memset(out, 0, 64);
  if (p.inf) return;
  memcpy(out, p.x.v, 32);
  memcpy(out + 4, p.y.v, 32);
}

// sum_j 16^j W[j] over kBatchWin window sums, from the top window down: 32 x 4
// doublings and 32 additions
inline J1 batch_horner(const J1* W) {
  J1 acc = W[kBatchWin - 1];
  for (int j = kBatchWin - 2; j >= 0; j--) {
    for (int k = 0; k < 4; k++) acc = host::jdbl<Fq>(acc);
    acc = host::jadd<Fq>(acc, W[j]);
  }
  return acc;
}

// The status word of one item and, for a status of 0, its two bases: w and
// C = -(zw + f + e) by the complete group law (Jacobian: no inversion).
inline uint32_t batch_item(const uint64_t* quad, uint32_t status_in, J1* w, J1* c) {
  *w = *c = j1_inf();
  if (status_in) return status_in;
  G1 p[4];
  uint32_t st = 0;
  for (int i = 0; i < 4; i++) {
    p[i] = g1_from_words(quad + 8 * i);
    if (!g1_on_curve(p[i])) st |= kNotOnCurveBit;
  }
  if (st) return st;
  *w = j1_from(p[0]);
  *c = j1_neg(host::jadd<Fq>(host::jadd<Fq>(j1_from(p[1]), j1_from(p[2])), j1_from(p[3])));
  return 0;
}

// L and R over the items with status 0 (Jacobian), with the device's structure:
// signed 4-bit windows, per window the buckets [1..8] filled item by item and
// summed by running sums, then the Horner tail.  status (may be null) receives
// the words.  Returns true when every status is 0.
inline bool batch_fold(size_t B, const uint64_t* quads, const uint32_t* status_in, const uint64_t seed[4],
                       uint32_t* status, J1* L, J1* R) {
  std::vector<J1> bk((size_t)kBatchSlots * 8, j1_inf());
  bool clean = true;
  for (size_t i = 0; i < B; i++) {
    J1 base[2];
    const uint32_t st = batch_item(quads + 32 * i, status_in ? status_in[i] : 0u, &base[0], &base[1]);
    if (status) status[i] = st;
    if (st) {
      clean = false;
      continue;
    }
    uint64_t r[2];
    int8_t dig[kBatchWin];
    batch_coef(seed, (uint64_t)i, r);
    batch_recode(r, dig, 1);
    for (int o = 0; o < kBatchOutputs; o++) {
      if (host::is_zero(base[o].Z)) continue;  // an identity base contributes nothing
      const J1 neg = j1_neg(base[o]);
      for (int j = 0; j < kBatchWin; j++) {
        const int d = dig[j];
        if (d == 0) continue;
        J1& b = bk[((size_t)o * kBatchWin + j) * 8 + (size_t)(d < 0 ? -d : d) - 1];
        b = host::jadd<Fq>(b, d < 0 ? neg : base[o]);
      }
    }
  }
  J1 out[kBatchOutputs];
  for (int o = 0; o < kBatchOutputs; o++) {
    J1 W[kBatchWin];
    for (int j = 0; j < kBatchWin; j++) {
      // sum_k k bucket[k]: the running sum of the buckets from 8 down, summed
      const J1* b = &bk[((size_t)o * kBatchWin + j) * 8];
      J1 run = j1_inf(), sum = j1_inf();
      for (int k = 7; k >= 0; k--) {
        run = host::jadd<Fq>(run, b[k]);
        sum = host::jadd<Fq>(sum, run);
      }
      W[j] = sum;
    }
    out[o] = batch_horner(W);
  }
  *L = out[0];
  *R = out[1];
  return clean;
}

// the decision on the folded pair: one pairing product (pairing_host.hpp run_program)
inline uint32_t batch_decide(const HostTables& t, bool clean, const G1& L, const G1& R) {
  if (!clean) return 0u;
  if (L.inf && R.inf) return 1u;
  return e12_is_one(run_program(t, L, R)) ? 1u : 0u;
}

}  // namespace pairing
}  // namespace pm

// pairing_batch_plan.hpp -- host plan of the batch decider: one
// pairing check for B accumulator quads by a random linear combination,
//   L = sum r_i w_i,  R = sum r_i C_i,  C_i = -(zw_i + f_i + e_i),
//   ok = [ e(L, s_g2) e(R, g2) == 1 ].
// Here: the coefficient derivation, the recoding of a 128-bit coefficient into
// signed 4-bit windows, and the geometry of the sum kernel.  HIP-free apart
// from the PM_HD functions the prep kernel shares with the host form; read by
// pairing_batch_host.hpp, the kernels and tests/native/decide_batch_host.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "blake2b.hpp"
#include "pairing_plan.hpp"

namespace pm {
namespace pairing {

constexpr uint32_t kDecideLocate = 1u;  // PM_DECIDE_LOCATE

// ---- coefficients.  r_i = the first 16 bytes, little-endian, of BLAKE2b-512
// with the personalisation "pm-batch-decide" (zero-padded to 16 bytes) over
// seed[32] || le64(i): 40 bytes, one compression.  Used as it comes: a zero
// (probability 2^-128) is not special-cased.
constexpr uint64_t le64_of(const char* s, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)(uint8_t)s[i] << (8 * i);
  return v;
}
constexpr uint64_t kBatchPersonal0 = le64_of("pm-batch", 8);
constexpr uint64_t kBatchPersonal1 = le64_of("-decide", 7);  // the 16th byte is the padding zero

// seed: the 32 bytes as four little-endian words
PM_HD void batch_coef(const uint64_t seed[4], uint64_t i, uint64_t r[2]) {
  uint64_t h[8], m[16];
  for (int k = 0; k < 8; k++) h[k] = Blake2bIV::v[k];
  h[0] ^= 0x01010040ull;  // digest_length 64, key_length 0, fanout 1, depth 1
  h[6] ^= kBatchPersonal0;
  h[7] ^= kBatchPersonal1;
  for (int k = 0; k < 16; k++) m[k] = 0;
  for (int k = 0; k < 4; k++) m[k] = seed[k];
  m[4] = i;
  blake2b_compress(h, m, 40, true);
  r[0] = h[0];
  r[1] = h[1];
}

// ---- recoding.  r < 2^128 -> kBatchWin signed digits d_w in [-8, 7],
// sum_w d_w 16^w = r, stored at dst[w * stride].  A nibble plus the carry is at
// most 16; from 8 on it becomes (v - 16) and carries.  Window 32 holds the carry
// out of the top nibble alone (0 or 1), so nothing is carried out of it.
constexpr int kBatchWin = 33;
PM_HD void batch_recode(const uint64_t r[2], int8_t* dst, size_t stride) {
  uint32_t carry = 0;
  for (int w = 0; w < kBatchWin; w++) {
    const uint32_t nib = w < 32 ? (uint32_t)(r[w >> 4] >> ((w & 15) * 4)) & 15u : 0u;
    const uint32_t v = nib + carry;  // <= 16
    carry = v >= 8u ? 1u : 0u;
    dst[(size_t)w * stride] = (int8_t)((int)v - (carry ? 16 : 0));
  }
}

// ---- geometry of k_batch_sum.  Block (s, j, o): slice s of window j of output
// o (0: L over the w_i, 1: R over the C_i).  A block is kBatchQuads quads; quad
// v adds the items s kq 64 + r 64 + v, r < kq, then an LDS tree folds the quads
// and the last block of (j, o) folds the ns slices by ticket.
constexpr int kBatchQuads = 64;
constexpr int kBatchOutputs = 2;
constexpr int kBatchSlots = kBatchOutputs * kBatchWin;  // window sums of one chunk
// At most kBatchKq terms per quad and slice: up to 512 items a (window, output)
// is one block and needs no ticket fold; at 4096 items the geometry is the small
// path's measured best for that many terms (8 slices of 8 terms per quad,
// msm_plan.hpp small_plan); beyond, the slices grow and the chain of additions
// (~3.2 us each, msm_small.hpp) does not.  Not tuned by measurement of its own.
constexpr uint32_t kBatchKq = 8;
// one chunk of items: its [1..8]P table is 2 KiB per item (128 MiB here); a
// larger batch runs chunk after chunk and the host adds the chunks' sums
constexpr size_t kBatchChunk = size_t(1) << 16;
struct BatchPlan {
  uint32_t kq;  // terms per quad and slice
  uint32_t ns;  // slices per (window, output)
};
inline BatchPlan batch_plan(size_t n) {  // 1 <= n <= kBatchChunk
  BatchPlan p;
  const size_t per = (n + kBatchQuads - 1) / kBatchQuads;
  p.kq = (uint32_t)(per < kBatchKq ? per : kBatchKq);
  p.ns = (uint32_t)((n + (size_t)p.kq * kBatchQuads - 1) / ((size_t)p.kq * kBatchQuads));
  return p;
}
// scratch of one chunk: the prepared bases (w_i, C_i: 2 x 64 B), then the tickets
inline size_t batch_bases_bytes(size_t n) { return n * 128; }
inline size_t batch_digits_bytes(size_t n) { return (size_t)kBatchWin * n; }

}  // namespace pairing
}  // namespace pm

// decide_batch_host.cpp -- stand-alone host program over pairing_batch_plan.hpp
// and pairing_batch_host.hpp (`make -C halo2-aggregation_amd decide_batch_asan`:
// g++ with ASan + UBSan; tests/test_decide_batch_native.py).  It checks the batch
// decider's host pieces against values it recomputes naively here:
//   * the coefficient derivation (one hand-built compression) against the
//     streaming Blake2b hasher and two pinned values;
//   * the 128-bit recoding: sum digit 16^k == r, digits in [-8, 7], for zero,
//     all-ones (the carry out of the top nibble lands in window 32), the
//     carry-chain extremes and random values;
//   * the Horner tail over 33 window sums against a bitwise double-and-add of
//     the combined scalar;
//   * the host fold (buckets, running sums, Horner) against r_i-by-r_i
//     double-and-add over the affine complete law, with a status item, an
//     identity w, an identity sum and equal points among the items.
// Exit status 0 and "decide_batch_host: all checks passed", or 1 at the first mismatch.
#include <stdio.h>
#include <stdlib.h>

#include "../../halo2-aggregation_amd/csrc/pairing_batch_host.hpp"

using namespace pm::pairing;
namespace host = pm::host;
typedef unsigned __int128 u128;

static int g_checks = 0;
#define CHECK(c)                                                                          \
  do {                                                                                    \
    g_checks++;                                                                           \
    if (!(c)) {                                                                           \
      fprintf(stderr, "decide_batch_host: FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

// ---- naive group arithmetic: bitwise double-and-add from the top bit
static J1 gen() { return j1_from(G1{e1_small(1), e1_small(2), false}); }
static J1 smul(const uint64_t* k, int limbs, const J1& p) {
  J1 acc = j1_inf();
  for (int bit = 64 * limbs - 1; bit >= 0; bit--) {
    acc = host::jdbl<Fq>(acc);
    if ((k[bit >> 6] >> (bit & 63)) & 1) acc = host::jadd<Fq>(acc, p);
  }
  return acc;
}
static bool same_point(const J1& a, const J1& b) {
  const G1 x = j1_affine(a), y = j1_affine(b);
  if (x.inf || y.inf) return x.inf == y.inf;
  return e1_eq(x.x, y.x) && e1_eq(x.y, y.y);
}
static void put_point(uint64_t* out, const J1& p) { g1_to_words(j1_affine(p), out); }

static void test_coefficients() {
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)i;
  uint64_t sw[4];
  memcpy(sw, seed, 32);
  const char personal[16] = {'p', 'm', '-', 'b', 'a', 't', 'c', 'h', '-', 'd', 'e', 'c', 'i', 'd', 'e', 0};
  const uint64_t idx[] = {0, 1, 7, 0x100000005ull, ~0ull};
  for (uint64_t i : idx) {
    uint64_t r[2];
    batch_coef(sw, i, r);
    pm::Blake2bHost h(personal);
    h.update(seed, 32);
    h.update(&i, 8);  // little-endian host
    uint8_t d[64];
    h.finalize(d);
    uint64_t want[2];
    memcpy(want, d, 16);
    CHECK(r[0] == want[0] && r[1] == want[1]);
  }
  uint64_t r[2];
  batch_coef(sw, 0, r);  // tests/test_decide_batch_ref.py pins the same values against hashlib
  CHECK(r[1] == 0x8c0afa9d4fcc8a90ull && r[0] == 0xa5edaa4407bee311ull);
  batch_coef(sw, 7, r);
  CHECK(r[1] == 0x7f20c890bca58ae4ull && r[0] == 0x5a221eef282d2c2dull);
}

static void check_recode(uint64_t lo, uint64_t hi) {
  const uint64_t r[2] = {lo, hi};
  int8_t d[kBatchWin + 2];
  d[0] = d[kBatchWin + 1] = 0x55;  // guards: the recoding writes kBatchWin digits and no more
  batch_recode(r, d + 1, 1);
  CHECK(d[0] == 0x55 && d[kBatchWin + 1] == 0x55);
  // Horner from the top window: exact modulo 2^128 (unsigned wrap) and modulo 2^61 - 1
  const uint64_t M = (1ull << 61) - 1;
  u128 acc = 0;
  uint64_t accm = 0;
  for (int w = kBatchWin - 1; w >= 0; w--) {
    const int dw = d[1 + w];
    CHECK(dw >= -8 && dw <= 7);
    acc = acc * 16 + (u128)(int64_t)dw;  // a negative digit wraps: the sum is taken mod 2^128
    accm = (uint64_t)(((u128)accm * 16 + (uint64_t)(dw + 16)) % M);
    accm = (accm + M - 16) % M;
  }
  CHECK(d[kBatchWin] == 0 || d[kBatchWin] == 1);
  const u128 want = ((u128)hi << 64) | lo;
  CHECK(acc == want);
  CHECK(accm == (uint64_t)(want % M));
}
static void test_recoding() {
  check_recode(0, 0);
  check_recode(1, 0);
  check_recode(7, 0);
  check_recode(8, 0);
  check_recode(~0ull, ~0ull);  // all ones: -1, 0, ..., 0, and 1 in window 32
  check_recode(0, 1ull << 63);
  check_recode(0x8888888888888888ull, 0x8888888888888888ull);  // every nibble carries
  check_recode(0x7777777777777777ull, 0x7777777777777777ull);  // none does
  check_recode(0xfffffffffffffff8ull, ~0ull);
  check_recode(0x7fffffffffffffffull, 0xf000000000000000ull);
  {
    const uint64_t r[2] = {~0ull, ~0ull};
    int8_t d[kBatchWin];
    batch_recode(r, d, 1);
    CHECK(d[0] == -1 && d[kBatchWin - 1] == 1);
    for (int w = 1; w < kBatchWin - 1; w++) CHECK(d[w] == 0);
  }
  for (int t = 0; t < 200; t++) check_recode(rnd(), rnd());
  // strided store (the device layout [window][n])
  const uint64_t r[2] = {rnd(), rnd()};
  int8_t a[kBatchWin], b[kBatchWin * 3];
  memset(b, 0x55, sizeof(b));
  batch_recode(r, a, 1);
  batch_recode(r, b + 1, 3);
  for (int w = 0; w < kBatchWin; w++) CHECK(b[3 * w + 1] == a[w] && b[3 * w] == 0x55 && b[3 * w + 2] == 0x55);
}

static void test_horner() {
  const J1 G = gen();
  for (int round = 0; round < 3; round++) {
    // W[j] = [k_j]G with k_j < 2^60; K = sum k_j 16^j < 2^(60 + 132) in four limbs
    uint64_t K[4] = {0, 0, 0, 0};
    J1 W[kBatchWin];
    for (int j = 0; j < kBatchWin; j++) {
      uint64_t k = rnd() >> 4;
      if (round == 1 && j % 3 == 0) k = 0;        // identity windows, the top one included
      if (round == 2) k = j < 32 ? 5 : 0;          // equal windows: additions that double
      W[j] = smul(&k, 1, G);
      // K += k << (4 j)
      const int sh = 4 * j, limb = sh >> 6, off = sh & 63;
      u128 carry = (u128)k << off;
      for (int l = limb; l < 4 && carry; l++) {
        const u128 s = (u128)K[l] + (uint64_t)carry;
        K[l] = (uint64_t)s;
        carry = (carry >> 64) + (s >> 64);
      }
    }
    CHECK(same_point(batch_horner(W), smul(K, 4, G)));
  }
  J1 Z[kBatchWin];
  for (int j = 0; j < kBatchWin; j++) Z[j] = j1_inf();
  CHECK(host::is_zero(batch_horner(Z).Z));
}

static void test_fold() {
  const J1 G = gen();
  const int B = 9;
  uint64_t quads[B * 32];
  uint32_t status_in[B] = {0, 0, 0, 0x13, 0, 0, 0, 0, 0};
  // logs (a, b, c, d); 0 = the identity
  const uint64_t logs[B][4] = {{5, 6, 7, 8},    {11, 12, 13, 14}, {5, 6, 7, 8},  // items 0 and 2: equal points
                               {21, 22, 23, 24}, {0, 31, 32, 33},                // a status; an identity w
                               {41, 42, 43, 0},  {51, 52, 52, 53},               // an identity e; zw = f
                               {61, 0, 0, 0},    {71, 72, 73, 74}};
  for (int i = 0; i < B; i++)
    for (int t = 0; t < 4; t++) put_point(quads + 32 * i + 8 * t, smul(&logs[i][t], 1, G));
  // item 7: the three-point sum is the identity.  Item 8: off the curve
  quads[32 * 8 + 16 + 4] ^= 2;
  uint8_t seed[32];
  for (int i = 0; i < 32; i++) seed[i] = (uint8_t)(3 * i + 1);
  uint64_t sw[4];
  memcpy(sw, seed, 32);
  uint32_t status[B];
  J1 L, R;
  const bool clean = batch_fold(B, quads, status_in, sw, status, &L, &R);
  CHECK(!clean);
  J1 wantL = j1_inf(), wantR = j1_inf();
  for (int i = 0; i < B; i++) {
    const uint32_t want_st = i == 3 ? 0x13u : i == 8 ? kNotOnCurveBit : 0u;
    CHECK(status[i] == want_st);
    if (want_st) continue;
    G1 p[4];
    for (int t = 0; t < 4; t++) p[t] = g1_from_words(quads + 32 * i + 8 * t);
    G1 c = g1_add(g1_add(p[1], p[2]), p[3]);  // the affine complete law of the per-proof decider
    if (!c.inf) c.y = e1_neg(c.y);
    uint64_t r[2];
    batch_coef(sw, (uint64_t)i, r);
    wantL = host::jadd<Fq>(wantL, smul(r, 2, j1_from(p[0])));
    wantR = host::jadd<Fq>(wantR, smul(r, 2, j1_from(c)));
  }
  CHECK(same_point(L, wantL) && same_point(R, wantR));
  CHECK(!host::is_zero(L.Z) && !host::is_zero(R.Z));
  // without the two bad items the batch is clean; null status pointers are fine
  uint64_t q2[7 * 32];
  int n = 0;
  for (int i = 0; i < B; i++)
    if (i != 3 && i != 8) memcpy(q2 + 32 * n++, quads + 32 * i, 256);
  CHECK(batch_fold(7, q2, nullptr, sw, nullptr, &L, &R));
  // the empty batch: both sums the identity
  CHECK(batch_fold(0, nullptr, nullptr, sw, nullptr, &L, &R) && host::is_zero(L.Z) && host::is_zero(R.Z));
}

static void test_plan() {
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)512, (size_t)513, (size_t)4096, kBatchChunk}) {
    const BatchPlan p = batch_plan(n);
    CHECK(p.kq >= 1 && p.kq <= kBatchKq && p.ns >= 1);
    CHECK((size_t)p.ns * p.kq * kBatchQuads >= n);            // every item has a slot
    CHECK((size_t)(p.ns - 1) * p.kq * kBatchQuads < n);       // and no slice is empty
  }
  CHECK(batch_plan(kBatchKq * kBatchQuads).ns == 1 && batch_plan(kBatchKq * kBatchQuads + 1).ns == 2);
}

int main() {
  test_coefficients();
  test_recoding();
  test_horner();
  test_fold();
  test_plan();
  printf("decide_batch_host: all checks passed (%d)\n", g_checks);
  return 0;
}

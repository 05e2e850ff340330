// pairing_host.hpp -- host side of the BN254 pairing decider:
// the Fp2 / Fp12 tower over host_ec.hpp's field, the G2 checks and the line
// tables of pm_pairing_create, and pairing_plan.hpp's program run on the CPU
// (pm_accum_decide_host: the parity form of the kernels and the CPU baseline).
// HIP-free.  Every field value is Montgomery R = 2^256 and canonical.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "host_ec.hpp"
#include "pairing_plan.hpp"

namespace pm {
namespace pairing {

using Fq = Bn254Fq;
using E1 = host::E<Fq>;

inline E1 e1_words(const uint64_t w[4]) {
  E1 r;
  memcpy(r.v, w, 32);
  return r;
}
inline E1 e1_zero() {
  E1 r;
  memset(r.v, 0, 32);
  return r;
}
inline E1 e1_one() {  // R mod p
  E1 r;
  memcpy(r.v, Fq::ONE, 32);
  return r;
}
// any 256-bit word -> its value mod p (a product with R mod p reduces it)
inline E1 e1_canon(const E1& a) { return host::mul<Fq>(e1_one(), a); }  // the first operand is the reduced one
// canonical integer (< p) -> Montgomery
inline E1 e1_to_mont(const uint64_t w[4]) {
  E1 r2;
  memcpy(r2.v, Fq::R2, 32);
  return host::mul<Fq>(e1_words(w), r2);
}
inline E1 e1_small(uint64_t k) {
  const uint64_t w[4] = {k, 0, 0, 0};
  return e1_to_mont(w);
}
inline E1 e1_add(const E1& a, const E1& b) { return host::add<Fq>(a, b); }
inline E1 e1_sub(const E1& a, const E1& b) { return host::sub<Fq>(a, b); }
inline E1 e1_mul(const E1& a, const E1& b) { return host::mul<Fq>(a, b); }
inline E1 e1_neg(const E1& a) { return host::sub<Fq>(e1_zero(), a); }
inline bool e1_eq(const E1& a, const E1& b) { return memcmp(a.v, b.v, 32) == 0; }
// a^(p - 2); 0 -> 0
inline E1 e1_inv(const E1& a) {
  uint64_t e[4];
  for (int i = 0; i < 4; i++) e[i] = host::F64<Fq>::mod(i);
  e[0] -= 2;  // p is odd and p_0 > 2: no borrow
  E1 r = e1_one();
  for (int bit = 253; bit >= 0; bit--) {
    r = e1_mul(r, r);
    if ((e[bit >> 6] >> (bit & 63)) & 1) r = e1_mul(r, a);
  }
  return r;
}

struct E2 {
  E1 c0, c1;
};
inline E2 e2_zero() { return E2{e1_zero(), e1_zero()}; }
inline E2 e2_one() { return E2{e1_one(), e1_zero()}; }
inline bool e2_is_zero(const E2& a) { return host::is_zero(a.c0) && host::is_zero(a.c1); }
inline bool e2_eq(const E2& a, const E2& b) { return e1_eq(a.c0, b.c0) && e1_eq(a.c1, b.c1); }
inline E2 e2_add(const E2& a, const E2& b) { return E2{e1_add(a.c0, b.c0), e1_add(a.c1, b.c1)}; }
inline E2 e2_sub(const E2& a, const E2& b) { return E2{e1_sub(a.c0, b.c0), e1_sub(a.c1, b.c1)}; }
inline E2 e2_neg(const E2& a) { return E2{e1_neg(a.c0), e1_neg(a.c1)}; }
inline E2 e2_conj(const E2& a) { return E2{a.c0, e1_neg(a.c1)}; }
inline E2 e2_scale(const E2& a, const E1& k) { return E2{e1_mul(a.c0, k), e1_mul(a.c1, k)}; }
inline E2 e2_mul(const E2& a, const E2& b) {  // u^2 = -1, three products
  const E1 t0 = e1_mul(a.c0, b.c0), t1 = e1_mul(a.c1, b.c1);
  const E1 m = e1_mul(e1_add(a.c0, a.c1), e1_add(b.c0, b.c1));
  return E2{e1_sub(t0, t1), e1_sub(e1_sub(m, t0), t1)};
}
// times xi = 9 + u: (9 a0 - a1) + (9 a1 + a0) u
inline E2 e2_mul_xi(const E2& a) {
  const E2 a2 = e2_add(a, a), a4 = e2_add(a2, a2), a9 = e2_add(e2_add(a4, a4), a);
  return E2{e1_sub(a9.c0, a.c1), e1_add(a9.c1, a.c0)};
}
inline E2 e2_inv(const E2& a) {
  const E1 n = e1_inv(e1_add(e1_mul(a.c0, a.c0), e1_mul(a.c1, a.c1)));
  return E2{e1_mul(a.c0, n), e1_neg(e1_mul(a.c1, n))};
}
inline E2 e2_frob_const(int j, int k) { return E2{e1_to_mont(kFrob[j - 1][k][0]), e1_to_mont(kFrob[j - 1][k][1])}; }

// sum a[k] w^k, w^6 = xi
struct E12 {
  E2 a[6];
};
inline E12 e12_one() {
  E12 r;
  for (int k = 0; k < 6; k++) r.a[k] = e2_zero();
  r.a[0] = e2_one();
  return r;
}
inline E12 e12_mul(const E12& x, const E12& y) {
  E12 r;
  for (int k = 0; k < 6; k++) {
    E2 lo = e2_zero(), hi = e2_zero();
    for (int i = 0; i < 6; i++) {
      if (i <= k) lo = e2_add(lo, e2_mul(x.a[i], y.a[k - i]));
      else hi = e2_add(hi, e2_mul(x.a[i], y.a[k - i + 6]));
    }
    r.a[k] = e2_add(lo, e2_mul_xi(hi));
  }
  return r;
}
// x * (l0 + l1 w + l3 w^3), l0 in Fp
inline E12 e12_mul_line(const E12& x, const E1& l0, const E2& l1, const E2& l3) {
  E12 r;
  for (int k = 0; k < 6; k++) {
    E2 t1 = e2_mul(x.a[(k + 5) % 6], l1), t3 = e2_mul(x.a[(k + 3) % 6], l3);
    if (k < 1) t1 = e2_mul_xi(t1);
    if (k < 3) t3 = e2_mul_xi(t3);
    r.a[k] = e2_add(e2_scale(x.a[k], l0), e2_add(t1, t3));
  }
  return r;
}
inline E12 e12_conj(const E12& x) {
  E12 r = x;
  for (int k = 1; k < 6; k += 2) r.a[k] = e2_neg(x.a[k]);
  return r;
}

// ---- G2 on the twist y^2 = x^3 + 3 / xi, affine; inf for the identity
struct G2 {
  E2 x, y;
  bool inf;
};
inline E2 twist_b() {
  const E2 xi{e1_small(9), e1_one()};
  return e2_scale(e2_inv(xi), e1_small(3));
}
inline bool g2_on_curve(const G2& q) {
  if (q.inf) return true;
  return e2_eq(e2_mul(q.y, q.y), e2_add(e2_mul(q.x, e2_mul(q.x, q.x)), twist_b()));
}
// the slope of the line through t and q (the tangent when they are equal);
// false: the line is vertical (t = -q, or a tangent at y = 0)
inline bool g2_slope(const G2& t, const G2& q, E2* lam) {
  if (e2_eq(t.x, q.x)) {
    if (e2_is_zero(e2_add(t.y, q.y))) return false;
    const E2 xx = e2_mul(t.x, t.x);
    *lam = e2_mul(e2_add(e2_add(xx, xx), xx), e2_inv(e2_add(t.y, t.y)));
  } else {
    *lam = e2_mul(e2_sub(q.y, t.y), e2_inv(e2_sub(q.x, t.x)));
  }
  return true;
}
inline G2 g2_add(const G2& t, const G2& q) {
  if (t.inf) return q;
  if (q.inf) return t;
  E2 lam;
  if (!g2_slope(t, q, &lam)) return G2{e2_zero(), e2_zero(), true};
  G2 r;
  r.x = e2_sub(e2_sub(e2_mul(lam, lam), t.x), q.x);
  r.y = e2_sub(e2_mul(lam, e2_sub(t.x, r.x)), t.y);
  r.inf = false;
  return r;
}
inline G2 g2_neg(const G2& q) { return G2{q.x, e2_neg(q.y), q.inf}; }
inline G2 g2_frobenius(const G2& q) {
  return G2{e2_mul(e2_conj(q.x), e2_frob_const(1, 2)), e2_mul(e2_conj(q.y), e2_frob_const(1, 3)), q.inf};
}
// [r] q == O ?
inline bool g2_order_r(const G2& q) {
  G2 acc{e2_zero(), e2_zero(), true};
  for (int bit = 253; bit >= 0; bit--) {
    acc = g2_add(acc, acc);
    const uint64_t w = host::F64<Bn254Fr>::mod(bit >> 6);
    if ((w >> (bit & 63)) & 1) acc = g2_add(acc, q);
  }
  return acc.inf;
}
// 16 x u64 (x.c0, x.c1, y.c0, y.c1), each canonical; false: a word >= p or the identity
inline bool g2_from_words(const uint64_t w[16], G2* out) {
  uint64_t any = 0;
  E1 c[4];
  for (int i = 0; i < 4; i++) {
    c[i] = e1_words(w + 4 * i);
    if (!e1_eq(c[i], e1_canon(c[i]))) return false;
    any |= c[i].v[0] | c[i].v[1] | c[i].v[2] | c[i].v[3];
  }
  if (!any) return false;
  *out = G2{E2{c[0], c[1]}, E2{c[2], c[3]}, false};
  return true;
}

// The line coefficients of one fixed G2 point, step by step in the program's
// order: out[step] = (lambda, lambda x_T - y_T).  false: a vertical line, which
// a point of order r never meets (6x + 2 < r).
struct LineCoef {
  E2 lam, c;
};
inline bool g2_line_table(const G2& q, std::vector<LineCoef>* out) {
  out->clear();
  G2 t = q;
  auto step = [&](const G2& other) {
    E2 lam;
    if (t.inf || !g2_slope(t, other, &lam)) return false;
    out->push_back(LineCoef{lam, e2_sub(e2_mul(lam, t.x), t.y)});
    t = g2_add(t, other);
    return true;
  };
  for (int bit = kLoopBits - 2; bit >= 0; bit--) {
    if (!step(t)) return false;
    if (((kLoopLow >> bit) & 1) && !step(q)) return false;
  }
  const G2 q1 = g2_frobenius(q), q2 = g2_neg(g2_frobenius(q1));
  if (!step(q1)) return false;
  E2 lam;  // the last line's sum T + (-pi^2 Q) is not needed
  if (t.inf || !g2_slope(t, q2, &lam)) return false;
  out->push_back(LineCoef{lam, e2_sub(e2_mul(lam, t.x), t.y)});
  return (int)out->size() == kSteps;
}

// Montgomery R = 2^256 -> the kernels' form: canonical x 2^261 mod p in 9 limbs of 29 bits
inline void e1_to_words29(const E1& a, uint32_t out[9]) {
  E1 v = a;
  for (int i = 0; i < 5; i++) v = e1_add(v, v);
  for (int i = 0; i < 9; i++) {
    const int bit = 29 * i, k = bit >> 6, s = bit & 63;
    uint64_t x = v.v[k] >> s;
    if (s > 35 && k + 1 < 4) x |= v.v[k + 1] << (64 - s);
    out[i] = (uint32_t)x & ((1u << 29) - 1u);
  }
}

// ---- G1 for the decider's three-point sum: affine, complete
struct G1 {
  E1 x, y;
  bool inf;
};
inline bool g1_on_curve(const G1& p) {
  if (p.inf) return true;
  return e1_eq(e1_mul(p.y, p.y), e1_add(e1_mul(p.x, e1_mul(p.x, p.x)), e1_small(3)));
}
inline G1 g1_add(const G1& p, const G1& q) {
  if (p.inf) return q;
  if (q.inf) return p;
  E1 lam;
  if (e1_eq(p.x, q.x)) {
    if (host::is_zero(e1_add(p.y, q.y))) return G1{e1_zero(), e1_zero(), true};
    const E1 xx = e1_mul(p.x, p.x);
    lam = e1_mul(e1_add(e1_add(xx, xx), xx), e1_inv(e1_add(p.y, p.y)));
  } else {
    lam = e1_mul(e1_sub(q.y, p.y), e1_inv(e1_sub(q.x, p.x)));
  }
  G1 r;
  r.x = e1_sub(e1_sub(e1_mul(lam, lam), p.x), q.x);
  r.y = e1_sub(e1_mul(lam, e1_sub(p.x, r.x)), p.y);
  r.inf = false;
  return r;
}
// 8 x u64 affine, (0, 0) the identity (all words zero); other words are taken mod p
inline G1 g1_from_words(const uint64_t w[8]) {
  uint64_t any = 0;
  for (int i = 0; i < 8; i++) any |= w[i];
  if (!any) return G1{e1_zero(), e1_zero(), true};
  return G1{e1_canon(e1_words(w)), e1_canon(e1_words(w + 4)), false};
}

// host tables of a pm_pairing: lines[step][pair], and the Frobenius constants in Montgomery form
struct HostTables {
  std::vector<LineCoef> lines[2];  // 0: s_g2 (with A), 1: g2 (with C)
  E2 frob[2][6];
};
inline void host_frob(HostTables* t) {
  for (int j = 1; j <= 2; j++)
    for (int k = 0; k < 6; k++) t->frob[j - 1][k] = e2_frob_const(j, k);
}

// pairing_plan.hpp's program on the CPU: the final-exponentiated e(A, s_g2) e(C, g2)
inline E12 run_program(const HostTables& t, const G1& A, const G1& C) {
  E12 s[kSlots];
  s[0] = e12_one();
  const G1* pt[2] = {&A, &C};
  for (int pc = 0; pc < kProgram.n; pc++) {
    const uint32_t w = kProgram.w[pc], d = op_d(w), a = op_a(w), b = op_b(w);
    switch (op_code(w)) {
      case kOpMul: s[d] = e12_mul(s[a], s[b]); break;
      case kOpLine: {
        const G1& p = *pt[b];
        if (p.inf) break;  // an identity point contributes 1
        const LineCoef& lc = t.lines[b][a];
        s[0] = e12_mul_line(s[0], p.y, e2_neg(e2_scale(lc.lam, p.x)), lc.c);
        break;
      }
      case kOpFrob:
        for (int k = 0; k < 6; k++) s[d].a[k] = e2_mul((b & 1) ? e2_conj(s[a].a[k]) : s[a].a[k], t.frob[b - 1][k]);
        break;
      case kOpConj: s[d] = e12_conj(s[a]); break;
      case kOpScaleInv: {
        const E2 ni = e2_inv(s[b].a[0]);
        for (int k = 0; k < 6; k++) s[d].a[k] = e2_mul(s[a].a[k], ni);
        break;
      }
    }
  }
  return s[0];
}

// the ABI's order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1: tower c_i.c_j is w^(2 j + i)
inline void e12_to_words(const E12& f, uint64_t out[48]) {
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      const E2& c = f.a[2 * j + i];
      memcpy(out + ((i * 3 + j) * 2 + 0) * 4, c.c0.v, 32);
      memcpy(out + ((i * 3 + j) * 2 + 1) * 4, c.c1.v, 32);
    }
}
inline bool e12_is_one(const E12& f) {
  if (!e2_eq(f.a[0], e2_one())) return false;
  for (int k = 1; k < 6; k++)
    if (!e2_is_zero(f.a[k])) return false;
  return true;
}

// One item of pm_accum_decide_host (quad: w, zw, f, e) or of the pair check
// (pair: A, C).  Returns ok; *status the outgoing status word; gt (may be
// null) the 48 words, zero for an item that is not evaluated.
inline uint32_t decide_item(const HostTables& t, const uint64_t* pts, bool quad, uint32_t status_in, uint32_t* status,
                            uint64_t* gt) {
  if (gt) memset(gt, 0, 48 * 8);
  *status = status_in;
  if (status_in) return 0;
  const int np = quad ? 4 : 2;
  G1 p[4];
  for (int i = 0; i < np; i++) {
    p[i] = g1_from_words(pts + 8 * i);
    if (!g1_on_curve(p[i])) *status |= kNotOnCurveBit;
  }
  if (*status) return 0;
  G1 A = p[0], C = p[1];
  if (quad) {
    C = g1_add(g1_add(p[1], p[2]), p[3]);
    if (!C.inf) C.y = e1_neg(C.y);
  }
  const E12 g = run_program(t, A, C);
  if (gt) e12_to_words(g, gt);
  return e12_is_one(g) ? 1u : 0u;
}

}  // namespace pairing
}  // namespace pm

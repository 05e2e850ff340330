// pairing_host.cpp -- stand-alone host program over pairing_host.hpp and
// pairing_plan.hpp (`make -C halo2-aggregation_amd pairing_asan`: g++ with ASan +
// UBSan; tests/test_pairing_native.py).  It checks the host tower, the G2 table
// builder and the decider against values it recomputes naively here:
//   * Fp12 products against a schoolbook product of degree-11 polynomials over
//     Fp modulo w^12 - 18 w^6 + 82 (u = w^6 - 9), no tower at all;
//   * the sparse line product against the dense product;
//   * the coefficient-wise Frobenius against x^p by square and multiply;
//   * every line coefficient against the chord / tangent equations on a G2
//     walk recomputed here, and the point checks on bad points;
//   * the program on a dozen quads built from small discrete logs, accept and
//     reject, special cases of the three-point sum, and bilinearity between two
//     different pm_pairing tables.
// Exit status 0 and "pairing_host: all checks passed", or 1 at the first mismatch.
#include <stdio.h>
#include <stdlib.h>

#include "../../halo2-aggregation_amd/csrc/pairing_host.hpp"

using namespace pm::pairing;
namespace host = pm::host;

static int g_checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    g_checks++;                                                     \
    if (!(c)) {                                                     \
      fprintf(stderr, "pairing_host: FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                      \
    }                                                               \
  } while (0)

// the G2 generator of DESIGN §10g, canonical
static const uint64_t kG2[4][4] = {
    {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},
    {0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},
    {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull},
    {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull}};

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}
static E1 rnd_e1() {
  uint64_t w[4] = {rnd(), rnd(), rnd(), rnd() >> 3};  // < 2^253 < p
  return e1_to_mont(w);
}
static E12 rnd_e12() {
  E12 r;
  for (int k = 0; k < 6; k++) r.a[k] = E2{rnd_e1(), rnd_e1()};
  return r;
}
static bool e12_eq(const E12& a, const E12& b) {
  for (int k = 0; k < 6; k++)
    if (!e2_eq(a.a[k], b.a[k])) return false;
  return true;
}

// ---- naive Fp12: 12 coefficients of Fp[w] / (w^12 - 18 w^6 + 82)
struct Poly {
  E1 c[12];
};
static Poly to_poly(const E12& x) {  // (c0 + c1 u) w^k = (c0 - 9 c1) w^k + c1 w^(k+6)
  Poly p;
  const E1 nine = e1_small(9);
  for (int k = 0; k < 6; k++) {
    p.c[k] = e1_sub(x.a[k].c0, e1_mul(nine, x.a[k].c1));
    p.c[k + 6] = x.a[k].c1;
  }
  return p;
}
static E12 from_poly(const Poly& p) {
  E12 r;
  const E1 nine = e1_small(9);
  for (int k = 0; k < 6; k++) r.a[k] = E2{e1_add(p.c[k], e1_mul(nine, p.c[k + 6])), p.c[k + 6]};
  return r;
}
static Poly poly_mul(const Poly& a, const Poly& b) {
  E1 t[23];
  for (int i = 0; i < 23; i++) t[i] = e1_zero();
  for (int i = 0; i < 12; i++)
    for (int j = 0; j < 12; j++) t[i + j] = e1_add(t[i + j], e1_mul(a.c[i], b.c[j]));
  const E1 c18 = e1_small(18), c82 = e1_small(82);
  for (int i = 22; i >= 12; i--) {  // w^i = 18 w^(i-6) - 82 w^(i-12)
    t[i - 6] = e1_add(t[i - 6], e1_mul(c18, t[i]));
    t[i - 12] = e1_sub(t[i - 12], e1_mul(c82, t[i]));
  }
  Poly r;
  for (int i = 0; i < 12; i++) r.c[i] = t[i];
  return r;
}
static E12 naive_mul(const E12& a, const E12& b) { return from_poly(poly_mul(to_poly(a), to_poly(b))); }

static void test_tower() {
  for (int it = 0; it < 6; it++) {
    const E12 a = rnd_e12(), b = rnd_e12();
    CHECK(e12_eq(e12_mul(a, b), naive_mul(a, b)));
    CHECK(e12_eq(e12_mul(a, a), naive_mul(a, a)));
    // the sparse product against the dense one
    const E1 l0 = rnd_e1();
    const E2 l1{rnd_e1(), rnd_e1()}, l3{rnd_e1(), rnd_e1()};
    E12 line;
    for (int k = 0; k < 6; k++) line.a[k] = e2_zero();
    line.a[0] = E2{l0, e1_zero()};
    line.a[1] = l1;
    line.a[3] = l3;
    CHECK(e12_eq(e12_mul_line(a, l0, l1, l3), naive_mul(a, line)));
  }
  const E12 y = rnd_e12();
  CHECK(e12_eq(e12_mul(y, e12_one()), y) && e12_eq(e12_conj(e12_conj(y)), y));
  // u^2 = -1, xi = 9 + u, inverses
  const E2 u{e1_zero(), e1_one()};
  CHECK(e2_eq(e2_mul(u, u), e2_neg(e2_one())));
  const E2 x{rnd_e1(), rnd_e1()};
  CHECK(e2_eq(e2_mul_xi(x), e2_mul(x, E2{e1_small(9), e1_one()})));
  CHECK(e2_eq(e2_mul(x, e2_inv(x)), e2_one()));
  CHECK(e1_eq(e1_mul(x.c0, e1_inv(x.c0)), e1_one()));
  CHECK(host::is_zero(e1_inv(e1_zero())));
  // a word that is not reduced is taken mod p
  uint64_t pw[4];
  for (int i = 0; i < 4; i++) pw[i] = host::F64<Fq>::mod(i);
  CHECK(host::is_zero(e1_canon(e1_words(pw))));
  const uint64_t ones[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  const E1 c = e1_canon(e1_words(ones));
  CHECK(e1_eq(c, e1_canon(c)));
}

static void test_frobenius() {
  HostTables t;
  host_frob(&t);
  const E12 x = rnd_e12();
  // x^p by square and multiply
  E12 r = e12_one();
  for (int bit = 253; bit >= 0; bit--) {
    r = e12_mul(r, r);
    if ((host::F64<Fq>::mod(bit >> 6) >> (bit & 63)) & 1) r = e12_mul(r, x);
  }
  E12 f1, f2;
  for (int k = 0; k < 6; k++) {
    f1.a[k] = e2_mul(e2_conj(x.a[k]), t.frob[0][k]);
    f2.a[k] = e2_mul(x.a[k], t.frob[1][k]);
  }
  CHECK(e12_eq(f1, r));
  E12 f11;
  for (int k = 0; k < 6; k++) f11.a[k] = e2_mul(e2_conj(f1.a[k]), t.frob[0][k]);
  CHECK(e12_eq(f11, f2));
  // conjugation is the p^6 Frobenius: three times p^2
  E12 f6 = x;
  for (int rep = 0; rep < 3; rep++)
    for (int k = 0; k < 6; k++) f6.a[k] = e2_mul(f6.a[k], t.frob[1][k]);
  CHECK(e12_eq(f6, e12_conj(x)));
}

static G2 generator() {
  return G2{E2{e1_to_mont(kG2[0]), e1_to_mont(kG2[1])}, E2{e1_to_mont(kG2[2]), e1_to_mont(kG2[3])}, false};
}
static G2 g2_mul_small(uint64_t k, const G2& q) {
  G2 acc{e2_zero(), e2_zero(), true}, b = q;
  for (; k; k >>= 1) {
    if (k & 1) acc = g2_add(acc, b);
    b = g2_add(b, b);
  }
  return acc;
}

static void test_tables() {
  const G2 g = generator();
  CHECK(g2_on_curve(g));
  CHECK(g2_order_r(g));
  G2 bad = g;
  bad.y.c0 = e1_add(bad.y.c0, e1_one());
  CHECK(!g2_on_curve(bad));
  uint64_t zero[16] = {0};
  G2 tmp;
  CHECK(!g2_from_words(zero, &tmp));
  uint64_t w[16];
  memcpy(w, g.x.c0.v, 32), memcpy(w + 4, g.x.c1.v, 32), memcpy(w + 8, g.y.c0.v, 32), memcpy(w + 12, g.y.c1.v, 32);
  CHECK(g2_from_words(w, &tmp) && e2_eq(tmp.x, g.x) && e2_eq(tmp.y, g.y));
  w[3] = ~0ull;
  CHECK(!g2_from_words(w, &tmp));

  for (uint64_t tau : {1ull, 12345ull}) {
    const G2 q = g2_mul_small(tau, g);
    std::vector<LineCoef> tab;
    CHECK(g2_line_table(q, &tab));
    CHECK((int)tab.size() == kSteps);
    // the walk recomputed here: T_0 = Q; a doubling step's slope satisfies 2 y lambda = 3 x^2, an
    // addition's lambda (x_O - x_T) = y_O - y_T, and c = lambda x_T - y_T
    const G2 q1 = g2_frobenius(q), q2 = g2_neg(g2_frobenius(q1));
    CHECK(g2_on_curve(q1) && g2_on_curve(q2));
    G2 T = q;
    int s = 0, adds = 0;
    auto check = [&](const G2& other, bool dbl) {
      const LineCoef& lc = tab[(size_t)s];
      CHECK(step_doubles(s) == dbl);
      if (dbl) {
        const E2 xx = e2_mul(T.x, T.x);
        CHECK(e2_eq(e2_mul(e2_add(T.y, T.y), lc.lam), e2_add(e2_add(xx, xx), xx)));
      } else {
        CHECK(e2_eq(e2_mul(lc.lam, e2_sub(other.x, T.x)), e2_sub(other.y, T.y)));
        adds++;
      }
      CHECK(e2_eq(lc.c, e2_sub(e2_mul(lc.lam, T.x), T.y)));
      T = g2_add(T, other);
      s++;
    };
    for (int bit = kLoopBits - 2; bit >= 0; bit--) {
      check(T, true);
      if ((kLoopLow >> bit) & 1) check(q, false);
    }
    check(q1, false);
    check(q2, false);
    CHECK(s == kSteps && adds == kSteps - 64);
    CHECK(g2_add(T, g2_frobenius(g2_frobenius(q1))).inf);  // [6x + 2]Q + pi Q - pi^2 Q + pi^3 Q = O on G2
  }
  // device words: 29-bit limbs of value * 2^261 mod p; 1 -> F29Consts<Bn254Fq>::ONE
  uint32_t l[9];
  e1_to_words29(e1_one(), l);
  const uint32_t one29[9] = {0x157ccc21u, 0x141c2758u, 0x185230d3u, 0x014c0419u, 0x0aa36fb9u,
                             0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
  for (int i = 0; i < 9; i++) CHECK(l[i] == one29[i]);
}

static G1 g1_mul_small(uint64_t k) {
  G1 acc{e1_zero(), e1_zero(), true}, b{e1_small(1), e1_small(2), false};
  for (; k; k >>= 1) {
    if (k & 1) acc = g1_add(acc, b);
    b = g1_add(b, b);
  }
  return acc;
}
static void put(uint64_t* q, const G1& p) {
  memset(q, 0, 64);
  if (p.inf) return;
  memcpy(q, p.x.v, 32);
  memcpy(q + 4, p.y.v, 32);
}

static void test_decider() {
  const uint64_t tau = 12345;
  const G2 g = generator();
  HostTables t, t1;
  host_frob(&t);
  host_frob(&t1);
  CHECK(g2_line_table(g2_mul_small(tau, g), &t.lines[0]) && g2_line_table(g, &t.lines[1]));
  CHECK(g2_line_table(g, &t1.lines[0]) && g2_line_table(g, &t1.lines[1]));
  CHECK(g1_on_curve(g1_mul_small(7)) && g1_mul_small(0).inf);
  CHECK(kProgram.n == kProgOps && count_ops(kOpLine) == 2 * kSteps && count_ops(kOpScaleInv) == 1);

  struct Case {
    uint64_t a, b, c, d;
    uint32_t ok;
  };
  // a tau = b + c + d accepts
  const Case cases[] = {
      {3, 5, 7, 3 * tau - 12, 1},      {3, 5, 7, 3 * tau - 11, 0},   {1, 0, 0, tau, 1},
      {1, 0, 0, tau + 1, 0},           {0, 5, 7, 0, 0},              {0, 0, 0, 0, 1},
      {2, 9, 9, 2 * tau - 18, 1},      {2, 9, 9, 2 * tau - 17, 0},   {4, tau, tau, 2 * tau, 1},
      {4, tau, tau, 2 * tau + 2, 0},   {5, 1, 2, 5 * tau - 3, 1},    {5, 1, 2, 5 * tau - 2, 0},
  };
  int n = 0;
  for (const Case& cs : cases) {
    uint64_t q[32], gt[48];
    put(q, g1_mul_small(cs.a)), put(q + 8, g1_mul_small(cs.b)), put(q + 16, g1_mul_small(cs.c)),
        put(q + 24, g1_mul_small(cs.d));
    uint32_t st = 99;
    const uint32_t ok = decide_item(t, q, true, 0, &st, gt);
    CHECK(ok == cs.ok && st == 0);
    CHECK(decide_item(t, q, true, 0, &st, nullptr) == cs.ok);
    // out_gt is one exactly when the item is accepted
    bool one = memcmp(gt, e1_one().v, 32) == 0;
    for (int i = 4; i < 48; i++) one = one && gt[i] == 0;
    CHECK(one == (cs.ok == 1));
    n++;
  }
  CHECK(n == 12);
  // opposite points: zw = -f leaves e alone
  {
    uint64_t q[32];
    G1 f = g1_mul_small(5);
    put(q, g1_mul_small(2)), put(q + 8, f);
    f.y = e1_neg(f.y);
    put(q + 16, f), put(q + 24, g1_mul_small(2 * tau));
    uint32_t st;
    CHECK(decide_item(t, q, true, 0, &st, nullptr) == 1 && st == 0);
  }
  // bilinearity across two tables: e([a]G, [tau]G2) = e([a tau]G, G2) (C = O in both)
  {
    uint64_t q[32], g0[48], g1[48];
    uint32_t st;
    memset(q, 0, sizeof(q));
    put(q, g1_mul_small(6));
    CHECK(decide_item(t, q, true, 0, &st, g0) == 0);
    put(q, g1_mul_small(6 * tau));
    CHECK(decide_item(t1, q, true, 0, &st, g1) == 0);
    CHECK(memcmp(g0, g1, sizeof(g0)) == 0);
  }
  // off-curve point, incoming status word
  {
    uint64_t q[32], gt[48];
    put(q, g1_mul_small(3)), put(q + 8, g1_mul_small(5)), put(q + 16, g1_mul_small(7)), put(q + 24, g1_mul_small(9));
    q[20] ^= 2;
    uint32_t st;
    CHECK(decide_item(t, q, true, 0, &st, gt) == 0 && st == kNotOnCurveBit);
    for (int i = 0; i < 48; i++) CHECK(gt[i] == 0);
    CHECK(decide_item(t, q, true, 0x11, &st, gt) == 0 && st == 0x11);
    // the pair form: A = [a]G, C = -[a tau]G
    uint64_t pr[16];
    G1 c = g1_mul_small(3 * tau);
    c.y = e1_neg(c.y);
    put(pr, g1_mul_small(3)), put(pr + 8, c);
    CHECK(decide_item(t, pr, false, 0, &st, nullptr) == 1 && st == 0);
  }
}

int main() {
  test_tower();
  test_frobenius();
  test_tables();
  test_decider();
  printf("pairing_host: all checks passed (%d)\n", g_checks);
  return 0;
}

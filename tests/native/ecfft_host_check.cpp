// ecfft_host_check.cpp -- the point transform's host form (ecfft_host.hpp) under
// g++ ASan + UBSan: a stand-alone program, no GPU and no HIP library.
//
// For each curve and log_n = 0 .. 6 it runs, on 1 and on 3 threads:
//   * identity inputs                 -> identities;
//   * all-equal inputs P              -> out[0] = [n]P, every other output the identity;
//   * a single non-identity input     -> at index 0 every output is P; at index 1 out[k] = [omega^k]P;
//   * a forward transform then the inverse (omega^-1, n^-1) returns the input word for word;
//   * an omega of the wrong order is refused and nothing is written.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../halo2-aggregation_amd/csrc/ecfft_host.hpp"

using namespace pm;

static int g_fail = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

template <class Fs>
static host::E<Fs> sc_pow(const host::E<Fs>& b, const uint64_t e[4]) {
  host::E<Fs> r = ecfft::sc_one<Fs>();
  for (int i = 255; i >= 0; i--) {
    r = host::mul<Fs>(r, r);
    if ((e[i / 64] >> (i % 64)) & 1) r = host::mul<Fs>(r, b);
  }
  return r;
}

// a primitive 2^log_n-th root of unity: x^((r - 1) / 2^log_n) for the first x = 2, 3, .. that has the order
template <class Fs>
static host::E<Fs> root_of_unity(uint32_t log_n) {
  uint64_t e[4];
  for (int i = 0; i < 4; i++) e[i] = host::F64<Fs>::mod(i);
  e[0] -= 1;  // r - 1 (r is odd)
  for (uint32_t s = 0; s < log_n; s++) {
    for (int i = 0; i < 4; i++) e[i] = (e[i] >> 1) | (i < 3 ? e[i + 1] << 63 : 0);
  }
  host::E<Fs> x = ecfft::sc_one<Fs>();
  for (;;) {
    x = host::add<Fs>(x, ecfft::sc_one<Fs>());
    const host::E<Fs> w = sc_pow<Fs>(x, e);
    if (ecfft::omega_has_order<Fs>(w.v, log_n)) return w;
  }
}

template <class Fs>
static host::E<Fs> sc_inv(const host::E<Fs>& a) {  // a^(r - 2)
  uint64_t e[4];
  for (int i = 0; i < 4; i++) e[i] = host::F64<Fs>::mod(i);
  e[0] -= 2;
  return sc_pow<Fs>(a, e);
}

template <class Cv>
static std::vector<uint64_t> some_points(size_t n, const uint64_t gen[8]) {
  using F = typename Cv::Base;
  // P_i = [3 i + 2]G by a running sum
  std::vector<uint64_t> out(8 * n);
  const host::Pt<F> g = ecfft::pt_load<F>(gen);
  const host::Pt<F> g3 = host::addp<F>(host::dbl<F>(g), g);
  host::Pt<F> p = host::dbl<F>(g);
  for (size_t i = 0; i < n; i++) {
    ecfft::pt_store<F>(p, &out[8 * i]);
    p = host::addp<F>(p, g3);
  }
  return out;
}

template <class Cv>
static void run_curve(const char* name, uint64_t gx, uint64_t gy_small, bool gx_is_minus_one) {
  using F = typename Cv::Base;
  using Fs = typename Cv::Scalar;
  // the generator in Montgomery form: (1, 2) on BN254, (-1, 2) on Pasta
  uint64_t gen[8];
  {
    host::E<F> one, x, y, zero;
    memcpy(one.v, F::ONE, 32);
    memset(&zero, 0, sizeof(zero));
    x = one;
    for (uint64_t i = 1; i < gx; i++) x = host::add<F>(x, one);
    if (gx_is_minus_one) x = host::sub<F>(zero, x);
    y = one;
    for (uint64_t i = 1; i < gy_small; i++) y = host::add<F>(y, one);
    memcpy(gen, x.v, 32);
    memcpy(gen + 4, y.v, 32);
  }
  for (uint32_t log_n = 0; log_n <= 6; log_n++) {
    const size_t n = (size_t)1 << log_n;
    const host::E<Fs> w = root_of_unity<Fs>(log_n), wi = sc_inv<Fs>(w);
    host::E<Fs> nn = ecfft::sc_one<Fs>();
    for (uint32_t i = 0; i < log_n; i++) nn = host::add<Fs>(nn, nn);
    const host::E<Fs> ninv = sc_inv<Fs>(nn);
    CHECK(ecfft::omega_has_order<Fs>(wi.v, log_n));
    for (int threads : {1, 3}) {
      // identities
      std::vector<uint64_t> z(8 * n, 0);
      CHECK(ecfft::fft_points_host<Cv>(z.data(), log_n, w.v, nullptr, threads));
      for (uint64_t v : z) CHECK(v == 0);
      // all equal
      const std::vector<uint64_t> P = some_points<Cv>(1, gen);
      std::vector<uint64_t> eq(8 * n);
      for (size_t i = 0; i < n; i++) memcpy(&eq[8 * i], P.data(), 64);
      CHECK(ecfft::fft_points_host<Cv>(eq.data(), log_n, w.v, nullptr, threads));
      {
        uint64_t want[8];
        const uint64_t k[4] = {(uint64_t)n, 0, 0, 0};
        ecfft::pt_store<F>(ecfft::pt_mul<F>(ecfft::pt_load<F>(P.data()), k), want);
        CHECK(memcmp(eq.data(), want, 64) == 0);
        for (size_t i = 8; i < 8 * n; i++) CHECK(eq[i] == 0);
      }
      // a single point at index 0, and at index 1
      std::vector<uint64_t> s0(8 * n, 0);
      memcpy(s0.data(), P.data(), 64);
      CHECK(ecfft::fft_points_host<Cv>(s0.data(), log_n, w.v, nullptr, threads));
      for (size_t i = 0; i < n; i++) CHECK(memcmp(&s0[8 * i], P.data(), 64) == 0);
      if (n > 1) {
        std::vector<uint64_t> s1(8 * n, 0);
        memcpy(&s1[8], P.data(), 64);
        CHECK(ecfft::fft_points_host<Cv>(s1.data(), log_n, w.v, nullptr, threads));
        host::E<Fs> wk = ecfft::sc_one<Fs>();
        for (size_t k = 0; k < n; k++) {
          uint64_t want[8];
          ecfft::pt_store<F>(ecfft::pt_mul<F>(ecfft::pt_load<F>(P.data()), ecfft::sc_canon<Fs>(wk).v), want);
          CHECK(memcmp(&s1[8 * k], want, 64) == 0);
          wk = host::mul<Fs>(wk, w);
        }
      }
      // forward, then inverse with n^-1: the input again (one identity among the points)
      std::vector<uint64_t> in = some_points<Cv>(n, gen);
      if (n > 2) memset(&in[8 * 2], 0, 64);
      std::vector<uint64_t> rt = in;
      CHECK(ecfft::fft_points_host<Cv>(rt.data(), log_n, w.v, nullptr, threads));
      if (n > 1) CHECK(rt != in);
      CHECK(ecfft::fft_points_host<Cv>(rt.data(), log_n, wi.v, ninv.v, threads));
      CHECK(rt == in);
      // scale = 0: identities
      std::vector<uint64_t> zs = in;
      const uint64_t zero[4] = {0, 0, 0, 0};
      CHECK(ecfft::fft_points_host<Cv>(zs.data(), log_n, w.v, zero, threads));
      for (uint64_t v : zs) CHECK(v == 0);
      // a root of the wrong order is refused, the points untouched
      std::vector<uint64_t> keep = in;
      const host::E<Fs> bad = log_n == 0 ? root_of_unity<Fs>(1) : host::mul<Fs>(w, w);
      CHECK(!ecfft::fft_points_host<Cv>(keep.data(), log_n, bad.v, nullptr, threads));
      CHECK(keep == in);
    }
  }
  printf("ecfft_host_check: %s done\n", name);
}

int main() {
  run_curve<PallasCurve>("pallas", 1, 2, true);
  run_curve<VestaCurve>("vesta", 1, 2, true);
  run_curve<Bn254Curve>("bn254", 1, 2, false);
  if (g_fail) {
    printf("ecfft_host_check: %d checks FAILED\n", g_fail);
    return 1;
  }
  printf("ecfft_host_check: all checks passed\n");
  return 0;
}

// ecfft_host.hpp -- halo2's best_fft over curve points on the CPU
// (pm_fft_points_host: the parity form of ecfft_kernels.hpp and the CPU
// baseline).  HIP-free; host_ec.hpp's 4 x 64 Montgomery arithmetic.
//
//   out[k] = [scale] sum_j [omega^{jk}] in[j],   0 <= k < n = 2^log_n
//
// in place, natural order in and out.  Points are the boundary's affine form
// (8 x u64, Montgomery R = 2^256, (0,0) the identity); omega and scale are
// Montgomery too.  The loop is best_fft's: a bit reversal, then log_n
// decimation-in-time stages of n/2 butterflies  t = [w] b, b' = a - t,
// a' = a + t,  the points kept XYZZ until one conversion at the end.
#pragma once
#include <stdint.h>
#include <string.h>

#include <thread>
#include <vector>

#include "host_ec.hpp"

namespace pm {
namespace ecfft {

constexpr uint32_t kMaxLog = 26;  // n <= kMaxPoints, the MSM's limit on a base set

template <class Fs>
inline host::E<Fs> sc_load(const uint64_t* w) {
  host::E<Fs> r;
  memcpy(r.v, w, 32);
  return r;
}
template <class Fs>
inline host::E<Fs> sc_one() {  // 1 in Montgomery form
  host::E<Fs> r;
  memcpy(r.v, Fs::ONE, 32);
  return r;
}
// Montgomery -> the integer in [0, r)
template <class Fs>
inline host::E<Fs> sc_canon(const host::E<Fs>& a) {
  host::E<Fs> u;
  u.v[0] = 1, u.v[1] = u.v[2] = u.v[3] = 0;
  return host::mul<Fs>(a, u);
}
template <class Fs>
inline bool sc_eq(const host::E<Fs>& a, const host::E<Fs>& b) {
  return memcmp(a.v, b.v, 32) == 0;
}

// omega has exact order n = 2^log_n: omega^(n/2) = -1, and omega = 1 at n = 1
template <class Fs>
inline bool omega_has_order(const uint64_t omega[4], uint32_t log_n) {
  host::E<Fs> w = sc_load<Fs>(omega);
  bool below = false;  // canonical: below the modulus
  for (int i = 3; i >= 0 && !below; i--) {
    if (w.v[i] > host::F64<Fs>::mod(i)) return false;
    below = w.v[i] < host::F64<Fs>::mod(i);
  }
  if (!below) return false;
  const host::E<Fs> one = sc_one<Fs>();
  if (log_n == 0) return sc_eq<Fs>(w, one);
  for (uint32_t i = 0; i + 1 < log_n; i++) w = host::mul<Fs>(w, w);
  host::E<Fs> zero;
  memset(&zero, 0, sizeof(zero));
  return sc_eq<Fs>(w, host::sub<Fs>(zero, one));
}

template <class F>
inline host::Pt<F> pt_load(const uint64_t* w) {
  host::Pt<F> p;
  memcpy(p.X.v, w, 32);
  memcpy(p.Y.v, w + 4, 32);
  if (host::is_zero(p.X) && host::is_zero(p.Y)) return host::inf<F>();
  memcpy(p.ZZ.v, F::ONE, 32);
  memcpy(p.ZZZ.v, F::ONE, 32);
  return p;
}
template <class F>
inline void pt_store(const host::Pt<F>& p, uint64_t* w) {
  const Aff<F> a = xyzz_to_aff<F>(host::to_dev<F>(p));
  memcpy(w, a.x.l, 32);
  memcpy(w + 4, a.y.l, 32);
}
template <class F>
inline host::Pt<F> pt_neg(const host::Pt<F>& p) {
  host::Pt<F> r = p;
  host::E<F> zero;
  memset(&zero, 0, sizeof(zero));
  r.Y = host::sub<F>(zero, p.Y);
  return r;
}

// [k] p for the integer k (4 x u64): 4-bit windows from the top
template <class F>
inline host::Pt<F> pt_mul(const host::Pt<F>& p, const uint64_t k[4]) {
  if (host::is_zero(p.ZZ) || (k[0] | k[1] | k[2] | k[3]) == 0) return host::inf<F>();
  host::Pt<F> tab[16];
  tab[0] = host::inf<F>();
  tab[1] = p;
  for (int i = 2; i < 16; i++) tab[i] = (i & 1) ? host::addp<F>(tab[i - 1], p) : host::dbl<F>(tab[i / 2]);
  host::Pt<F> acc = host::inf<F>();
  for (int i = 63; i >= 0; i--) {
    for (int d = 0; d < 4; d++) acc = host::dbl<F>(acc);
    const unsigned dg = (unsigned)(k[i / 16] >> (4 * (i % 16))) & 15u;
    if (dg) acc = host::addp<F>(acc, tab[dg]);
  }
  return acc;
}

// job(lo, hi) over [0, count) on up to `threads` threads
template <class Job>
inline void par_for(size_t count, int threads, Job job) {
  size_t nt = threads < 1 ? 1 : (size_t)threads;
  if (nt > count / 8) nt = count / 8;  // not worth a thread below 8 items
  if (nt <= 1) {
    job((size_t)0, count);
    return;
  }
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(job, count * t / nt, count * (t + 1) / nt);
  job((size_t)0, count / nt);
  for (auto& x : th) x.join();
}

// Returns false when omega has not order 2^log_n (nothing is written then).
template <class Cv>
inline bool fft_points_host(uint64_t* points, uint32_t log_n, const uint64_t omega[4], const uint64_t* scale,
                            int threads) {
  using F = typename Cv::Base;
  using Fs = typename Cv::Scalar;
  if (!omega_has_order<Fs>(omega, log_n)) return false;
  const size_t n = (size_t)1 << log_n;
  std::vector<host::Pt<F>> a(n);
  // the bit reversal rides on the load
  for (size_t i = 0; i < n; i++) {
    size_t r = 0;
    for (uint32_t b = 0; b < log_n; b++) r |= ((i >> b) & 1) << (log_n - 1 - b);
    a[r] = pt_load<F>(points + 8 * i);
  }
  // omega^j, j < n/2, as integers
  std::vector<host::E<Fs>> tw(n > 1 ? n / 2 : 1);
  {
    const host::E<Fs> w = sc_load<Fs>(omega);
    host::E<Fs> c = sc_one<Fs>();
    for (size_t j = 0; j < tw.size(); j++) {
      tw[j] = sc_canon<Fs>(c);
      c = host::mul<Fs>(c, w);
    }
  }
  for (uint32_t s = 1; s <= log_n; s++) {
    const size_t m = (size_t)1 << (s - 1);
    par_for(n / 2, threads, [&a, &tw, m, s, log_n](size_t lo, size_t hi) {
      for (size_t g = lo; g < hi; g++) {
        const size_t j = g & (m - 1), ia = ((g >> (s - 1)) << s) + j, ib = ia + m;
        const host::Pt<F> t = j == 0 ? a[ib] : pt_mul<F>(a[ib], tw[j << (log_n - s)].v);
        const host::Pt<F> u = a[ia];
        a[ia] = host::addp<F>(u, t);
        a[ib] = host::addp<F>(u, pt_neg<F>(t));
      }
    });
  }
  host::E<Fs> sc;
  if (scale) sc = sc_canon<Fs>(sc_load<Fs>(scale));
  par_for(n, threads, [&a, &sc, scale, points](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi; i++) pt_store<F>(scale ? pt_mul<F>(a[i], sc.v) : a[i], points + 8 * i);
  });
  return true;
}

}  // namespace ecfft
}  // namespace pm

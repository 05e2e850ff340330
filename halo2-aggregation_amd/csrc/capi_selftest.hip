// capi_selftest.hip -- pm_selftest_field and pm_selftest_host.  The host
// self-test compares the engine's host tail (engine.hpp: MsmTail, tail_run,
// tail_split_bmi2) against itself, so this unit includes the engine header;
// it instantiates no kernel.
#include <cstring>
#include <type_traits>
#include <vector>

#include "capi_internal.hpp"
#include "engine.hpp"
#include "host_ec.hpp"

using namespace pm;

extern "C" {

int pm_selftest_field(pm_ctx* ctx, int curve, uint64_t seed, size_t n, uint64_t* mismatches) {
  if (!ctx || !mismatches) return set_error(PM_ERR_ARG, "null argument");
  if (n > (1u << 24)) return set_error(PM_ERR_ARG, "n too large");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return ops->selftest_field(ctx, seed, (uint32_t)n, mismatches);
}

extern "C++" {
namespace {
template <class P>
uint64_t selftest_host_field(uint64_t seed, size_t n) {
  using namespace pm::host;
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1, bad = 0;
  auto rnd = [&]() {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  auto fe = [&]() {  // uniform-ish below p, plus the edges 0, 1, p - 1
    E<P> e;
    const uint64_t k = rnd() % 16;
    for (int i = 0; i < 4; i++) e.v[i] = k == 0 ? 0 : k == 1 ? (i == 0) : k == 2 ? F64<P>::mod(i) - (i == 0) : rnd();
    if (k > 2) {
      e.v[3] %= F64<P>::mod(3);
    }
    return e;
  };
  for (size_t i = 0; i < n; i++) {
    const E<P> a = fe(), b = fe();
    const E<P> x = mul<P>(a, b), y = mul_adx<P>(a, b);
    bad += memcmp(x.v, y.v, 32) != 0;
  }
  Pt<P> h0{fe(), fe(), fe(), fe()}, h1 = h0, g{fe(), fe(), fe(), fe()};
  for (size_t i = 0; i < 64; i++) {
    h0 = dbl<P, false>(h0);
    h1 = dbl<P, true>(h1);
    if (i & 1) {
      h0 = addp<P, false>(h0, g);
      h1 = addp<P, true>(h1, g);
    }
  }
  bad += memcmp(&h0, &h1, sizeof(h0)) != 0;
  // Jacobian chain (jdbl / jadd, the small-MSM Horner) == the XYZZ chain: the
  // same rational maps, so any (x, y) works; both start from the same point
  // under a random z (Jacobian (X, Y, z), XYZZ (X, Y, z^2, z^3))
  auto both = [&](Pt<P>& x, Jac<P>& j) {
    const E<P> z = fe(), zz = mul<P>(z, z), zzz = mul<P>(zz, z);
    x = Pt<P>{fe(), fe(), zz, zzz};
    j = Jac<P>{x.X, x.Y, z};
  };
  Pt<P> xa, xg;
  Jac<P> ja, jg;
  both(xa, ja);
  both(xg, jg);
  for (size_t i = 0; i < 40; i++) {
    xa = dbl<P, true>(xa);
    ja = jdbl<P, true>(ja);
    if (i % 3 == 0) {
      xa = addp<P, true>(xa, xg);
      ja = jadd<P, false>(ja, jg);
    }
  }
  const Pt<P> jx = jac_to_xyzz<P, true>(ja);  // equal points: X1 ZZ2 == X2 ZZ1, Y1 ZZZ2 == Y2 ZZZ1
  auto same = [&](const Pt<P>& u, const Pt<P>& v) {
    const E<P> l1 = mul<P>(u.X, v.ZZ), r1 = mul<P>(v.X, u.ZZ), l2 = mul<P>(u.Y, v.ZZZ), r2 = mul<P>(v.Y, u.ZZZ);
    return memcmp(&l1, &r1, 32) == 0 && memcmp(&l2, &r2, 32) == 0 && !is_zero(u.ZZ) && !is_zero(v.ZZ);
  };
  bad += !same(xa, jx);
  // the split host tail (sets claimed by pool threads, engine.hpp tail_split)
  // == the single Horner (tail_terms / tail_run) on the variable-base
  // geometry (16 sets of 16 bits), with identity terms among random ones, on
  // pools of 1, 3 and 16 threads
  {
    pm::MsmTail<P> t;
    t.Wr = 16;
    t.NB2 = 13;
    t.NQ = t.NB2 + pm::kTJobs + 1;
    t.base = 16;
    t.extra = 0;
    t.log2L1 = 2;
    t.cmax = 16;
    t.empty = false;
    // terms on the curve (the group law is associative only there, and the
    // two forms add the terms in different orders): multiples of the
    // generator by a random double-and-add walk, each under a random z
    auto e_of = [](const pm::Fe<P>& f) {
      E<P> e;
      for (int k = 0; k < 4; k++) e.v[k] = (uint64_t)f.l[2 * k] | ((uint64_t)f.l[2 * k + 1] << 32);
      return e;
    };
    const pm::Fe<P> one = pm::fe_one<P>();
    const bool pasta = !std::is_same<P, pm::Bn254Fq>::value;  // generators (-1, 2) / (1, 2)
    const Pt<P> G{e_of(pasta ? pm::fe_neg<P>(one) : one), e_of(pm::fe_add<P>(one, one)), e_of(one), e_of(one)};
    std::vector<pm::Xyzz<P>> Q((size_t)t.Wr * t.NQ);
    Pt<P> cur = G;
    for (size_t k = 0; k < Q.size(); k++) {
      cur = (rnd() & 1) ? dbl<P, true>(cur) : addp<P, true>(cur, G);
      const E<P> z = fe(), zz = mul<P>(z, z), zzz = mul<P>(zz, z);
      const Pt<P> x{mul<P>(cur.X, zz), mul<P>(cur.Y, zzz), mul<P>(cur.ZZ, zz), mul<P>(cur.ZZZ, zzz)};
      Q[k] = to_dev<P>(k % 37 == 5 || is_zero(z) ? inf<P>() : x);
    }
    t.hQ = Q.data();
    const Pt<P> want = pm::tail_run<P>(t, pm::tail_terms<P>(t));
    for (int th : {1, 3, 16}) {
      pm::HostPool pool(th);
      bad += !same(pm::tail_split_bmi2<P>(pool, t), want);
    }
  }
  return bad;
}
}  // namespace
}  // extern "C++"

int pm_selftest_host(int curve, uint64_t seed, size_t n, uint64_t* mismatches) {
  if (!mismatches) return set_error(PM_ERR_ARG, "null argument");
  if (n > (1u << 24)) return set_error(PM_ERR_ARG, "n too large");
  if (!pm::host_has_bmi2()) return set_error(PM_ERR_UNSUPPORTED, "CPU without BMI2/ADX");
  switch (curve) {
    case PM_CURVE_PALLAS: *mismatches = selftest_host_field<pm::PallasFp>(seed, n); break;
    case PM_CURVE_VESTA: *mismatches = selftest_host_field<pm::VestaFp>(seed, n); break;
    case PM_CURVE_BN254: *mismatches = selftest_host_field<pm::Bn254Fq>(seed, n); break;
    default: return set_error(PM_ERR_ARG, "unknown curve id");
  }
  return PM_OK;
}

}  // extern "C"

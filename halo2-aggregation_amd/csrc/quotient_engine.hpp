// quotient_engine.hpp -- host driver of the quotient numerator (pm_quotient_*,
// SURVEY §8f-8): the per-call constant table, the launch of k_quot_eval, and
// the program run on the CPU (pm_quotient_eval_host).  Arguments are validated
// by the C-ABI (capi_poly.hip), which also builds the quotient's own columns with
// pm_fft_batch_device / pm_coeff_to_extended_device's driver (domain_engine.hpp).
#pragma once
#include <cstring>
#include <vector>

#include "domain_engine.hpp"
#include "quotient_kernels.hpp"

namespace pm {

static_assert(kDomTabT == kDomTabHead, "pm_quotient_create copies t from behind the table's head");

template <class Fs>
void quot_words(const Fe<Fs>& v, uint64_t* o) {
  for (int i = 0; i < 4; i++) o[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
}
// 2^t in Montgomery form; t may be negative
template <class Fs>
Fe<Fs> quot_pow2(int t) {
  Fe<Fs> r = fe_one<Fs>();
  for (int i = 0; i < (t < 0 ? -t : t); i++) r = fe_dbl<Fs>(r);
  return t < 0 ? fe_inv_bgcd<Fs>(r) : r;
}

// The constant table of one call: entry (source, k) = v 2^(261 + 5 k), v the
// plain value behind the Montgomery word m = v 2^256, so the entry is
// m 2^(5 (k + 1)).  Canonical 4 x u64, read alike by the kernel and the host.
template <class Fs>
void quot_const_words(const QuotPlan& pl, const uint64_t* shape_consts, const uint64_t* delta, const uint64_t* ch,
                      std::vector<uint64_t>* out) {
  const Fe<Fs> beta = fe_from_u64<Fs>(ch + 4), dl = fe_from_u64<Fs>(delta);
  std::vector<Fe<Fs>> bd;  // beta delta^i
  out->assign(pl.consts.size() * 4, 0);
  for (size_t i = 0; i < pl.consts.size(); i++) {
    const QuotConst& c = pl.consts[i];
    Fe<Fs> m;
    switch (c.src) {
      case kQcShape: m = fe_from_u64<Fs>(shape_consts + 4 * c.index); break;
      case kQcTheta: m = fe_from_u64<Fs>(ch); break;
      case kQcBeta: m = beta; break;
      case kQcGamma: m = fe_from_u64<Fs>(ch + 8); break;
      case kQcY: m = fe_from_u64<Fs>(ch + 12); break;
      case kQcBetaDelta:
        while (bd.size() <= c.index) bd.push_back(bd.empty() ? beta : fe_mul<Fs>(bd.back(), dl));
        m = bd[c.index];
        break;
      case kQcOne: m = fe_one<Fs>(); break;
      default: m = fe_zero<Fs>();
    }
    if (c.k != -1) m = fe_mul<Fs>(m, quot_pow2<Fs>(5 * (c.k + 1)));
    if (c.neg) m = fe_neg<Fs>(m);
    quot_words<Fs>(m, out->data() + 4 * i);
  }
}

// What pm_quotient_create needs from the field: omega^-1 and n^-1 of the
// inverse transform, and the words of 1 in the native (2^261) and the columns'
// (2^256) form.  out: 4 scalars.
template <class Cv>
int quotient_seed_impl(const pm_domain* d, uint64_t* out) {
  using Fs = typename Cv::Scalar;
  Fe<Fs> nn = fe_one<Fs>();
  for (uint32_t i = 0; i < d->k; i++) nn = fe_dbl<Fs>(nn);
  quot_words<Fs>(fe_inv_bgcd<Fs>(fe_from_u64<Fs>(d->omega)), out);
  quot_words<Fs>(fe_inv_bgcd<Fs>(nn), out + 4);
  quot_words<Fs>(quot_pow2<Fs>(5), out + 8);
  quot_words<Fs>(fe_one<Fs>(), out + 12);
  return PM_OK;
}

// ptrs: the call's column pointers in pm_quotient_columns order (plan.group_base)
template <class Cv>
int quotient_run_impl(Ctx* ctx, const pm_quotient* q, const void* const* ptrs, const uint64_t* ch, uint32_t flags,
                      void* d_out) {
  using Fs = typename Cv::Scalar;
  const hipStream_t st = ctx->stream;
  const QuotPlan& pl = q->plan;
  const size_t N = (size_t)1 << q->ext_k;
  std::vector<uint64_t> consts;
  quot_const_words<Fs>(pl, q->shape_consts.data(), q->delta, ch, &consts);
  const uint32_t n_user = pl.group_base[kQlOwn], n_ptrs = pl.group_base[kQlKinds];
  std::vector<const void*> host(n_ptrs);
  for (uint32_t i = 0; i < n_user; i++) host[i] = ptrs[i];
  for (uint32_t i = 0; i < kQownCols; i++)  // a gates-only program owns and reads none
    host[n_user + i] = q->d_own.p ? (const char*)q->d_own.p + (size_t)i * N * 32 : nullptr;
  const size_t off_consts = (n_ptrs * sizeof(void*) + 31) / 32 * 32;
  int rc;
  if ((rc = ctx->quot_io.ensure(off_consts + consts.size() * 8))) return rc;
  char* base = (char*)ctx->quot_io.p;
  HIP_TRY(hipMemcpyAsync(base, host.data(), n_ptrs * sizeof(void*), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(base + off_consts, consts.data(), consts.size() * 8, hipMemcpyHostToDevice, st));
  QuotArgs a{};
  a.prog = (const uint32_t*)q->d_prog.p;
  a.leaves = (const uint32_t*)q->d_leaves.p;
  a.ptrs = (const uint32_t* const*)base;
  a.consts = (const uint32_t*)(base + off_consts);
  a.t = (const uint32_t*)q->d_t.p;
  a.out = (uint32_t*)d_out;
  a.nops = (uint32_t)pl.ops.size();
  a.n = (uint32_t)N;
  a.tmask = (1u << (q->ext_k - q->k)) - 1u;
  a.y_const = pl.y_const;
  a.divide = flags & 1u;
  a.accumulate = flags & 2u;
  const unsigned grid = (unsigned)((N + kQuotThreads - 1) / kQuotThreads);
  PM_LAUNCH(ctx, "quot_eval", (k_quot_eval<Fs><<<grid, kQuotThreads, pl.slots * kQuotSlotBytes, st>>>(a)));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

// The compiled program on the CPU at R independent points (host keys: a leaf
// is an evaluation of the proof's scalar array; l_0, l_last and l_last +
// l_blind from the closed form of verifier.rs:553-591).  The arithmetic is
// the kernel's: a product is a b 2^-261, here two Montgomery products.
template <class Cv>
int quotient_eval_host_impl(const pm_proof_shape* s, size_t R, const uint64_t* scalars, const uint64_t* x,
                            const uint64_t* ch, uint64_t* out) {
  using Fs = typename Cv::Scalar;
  using E = host::E<Fs>;
  QuotPlan pl;
  AccLayout L;
  bool unsupported = false;
  const std::string err = quot_compile(s, -1, 0, kQuotCacheSlots, &pl, &L, &unsupported);
  if (!err.empty()) return set_error(unsupported ? PM_ERR_UNSUPPORTED : PM_ERR_ARG, "quotient: " + err);
  auto to_e = [](const Fe<Fs>& v) {
    E r;
    quot_words<Fs>(v, r.v);
    return r;
  };
  auto ld = [](const uint64_t* p) {
    E r;
    std::memcpy(r.v, p, 32);
    return r;
  };
  const E c251 = to_e(quot_pow2<Fs>(-5));  // (a b 2^-256) (2^251) 2^-256 = a b 2^-261
  const E zero = to_e(fe_zero<Fs>());
  auto mulc = [&](const E& a, const E& b) { return host::mul<Fs>(host::mul<Fs>(a, b), c251); };
  const Fe<Fs> one = fe_one<Fs>(), to_native = quot_pow2<Fs>(5);
  const Fe<Fs> omega_inv = fe_inv_bgcd<Fs>(fe_from_u64<Fs>(s->omega));
  Fe<Fs> nn = one;
  for (uint32_t i = 0; i < s->log_n; i++) nn = fe_dbl<Fs>(nn);
  const uint32_t bf = s->blinding_factors;
  std::vector<uint64_t> consts;
  std::vector<E> slot(pl.slots ? pl.slots : 1);
  for (size_t r = 0; r < R; r++) {
    const uint64_t* sc = scalars + r * (size_t)L.nsc * 4;
    quot_const_words<Fs>(pl, s->constants, s->delta, ch + r * 16, &consts);
    E own[kQownCols] = {zero, zero, zero, ld(x + 4 * r)};
    if (pl.need_l) {
      const Fe<Fs> xr = fe_from_u64<Fs>(x + 4 * r);
      Fe<Fs> xn = xr;
      for (uint32_t i = 0; i < s->log_n; i++) xn = fe_sqr<Fs>(xn);
      const Fe<Fs> num = fe_sub<Fs>(xn, one);
      if (fe_is_zero<Fs>(num)) return set_error(PM_ERR_ARG, "quotient: x^n = 1, the Lagrange closed form has a pole");
      Fe<Fs> w = one, sum = fe_zero<Fs>();
      for (uint32_t jj = 0; jj < bf + 2; jj++) {  // l of row -jj: w (x^n - 1) / (n (x - w)), w = omega^-jj
        const Fe<Fs> den = fe_mul<Fs>(fe_sub<Fs>(xr, w), nn);
        const Fe<Fs> l = fe_mul<Fs>(fe_mul<Fs>(fe_mul<Fs>(w, num), fe_inv_bgcd<Fs>(den)), to_native);
        if (jj == 0) own[kQownL0] = to_e(l);
        else sum = fe_add<Fs>(sum, l);
        if (jj == bf + 1) own[kQownLast] = to_e(l);
        w = fe_mul<Fs>(w, omega_inv);
      }
      own[kQownSum] = to_e(sum);
    }
    const E y = ld(consts.data() + 4 * pl.y_const);
    E h = zero;
    for (uint32_t w : pl.ops) {
      const uint32_t op = w & 7u, cb = w & kQConstB, dst = (w >> 4) & 63u, sa = (w >> 10) & 63u, b = w >> 16;
      if (op == kQLoad) {
        const QuotLeaf& lf = pl.leaves[b];
        slot[dst] = lf.kind == kQlOwn ? own[lf.eval] : ld(sc + 4 * (size_t)lf.eval);
        continue;
      }
      if (op == kQConst) {
        slot[dst] = ld(consts.data() + 4 * b);
        continue;
      }
      const E xa = slot[sa];
      if (op == kQFold) {
        h = b ? xa : host::add<Fs>(mulc(h, y), xa);
        continue;
      }
      const E z = op == kQNeg ? zero : cb ? ld(consts.data() + 4 * b) : slot[b & 63u];
      if (op == kQMul) slot[dst] = mulc(xa, z);
      else if (op == kQAdd) slot[dst] = host::add<Fs>(xa, z);
      else if (op == kQSub) slot[dst] = cb ? host::sub<Fs>(z, xa) : host::sub<Fs>(xa, z);
      else slot[dst] = host::sub<Fs>(zero, xa);
    }
    std::memcpy(out + 4 * r, h.v, 32);
  }
  return PM_OK;
}

}  // namespace pm

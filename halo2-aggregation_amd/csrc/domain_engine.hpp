// domain_engine.hpp -- host driver of the extended-domain conversions
// (pm_domain_*, pm_coeff_to_extended*, pm_extended_to_coeff*,
// pm_divide_by_vanishing_device, pm_fft_batch_device).
// Boundary: halo2 EvaluationDomain::{coeff_to_extended, extended_to_coeff,
// divide_by_vanishing_poly} [3P poly/domain.rs], reached from create_proof's
// quotient step.  Arguments are validated by the C-ABI (capi_poly.hip) before
// domain_run_impl runs; domain_tables_impl is the part of that validation
// that needs field arithmetic, and runs on the host alone.
#pragma once
#include <cstring>
#include <vector>

#include "domain_kernels.hpp"
#include "engine.hpp"
#include "ntt_engine.hpp"

namespace pm {

// Columns of one call run in groups whose scratch (N x 32 B per column and
// pass buffer) fits this budget, at least one column per group.
constexpr size_t kDomScratchBytes = size_t(256) << 20;

template <class Fs>
void dom_put(std::vector<uint64_t>* tab, const Fe<Fs>& v, const Fe<Fs>& to261) {
  const Fe<Fs> w = fe_mul<Fs>(v, to261);  // x 2^256 -> x 2^261, canonical
  for (int k = 0; k < 4; k++) tab->push_back((uint64_t)w.l[2 * k] | ((uint64_t)w.l[2 * k + 1] << 32));
}

// Checks omega_e and zeta, fills the domain's roots and the table the
// kernels read (R = 2^261 canonical packed, 4 x u64 per entry):
// [zeta^0..2 | N^-1 zeta^-0..-2 | t_0 .. t_{2^e - 1}].
template <class Cv>
int domain_tables_impl(uint32_t k, uint32_t ext_k, const uint64_t* omega_e, const uint64_t* zeta, pm_domain* d,
                       std::vector<uint64_t>* tab) {
  using Fs = typename Cv::Scalar;
  const uint32_t e = ext_k - k;
  const Fe<Fs> one = fe_one<Fs>(), we = fe_from_u64<Fs>(omega_e), z = fe_from_u64<Fs>(zeta);
  const Fe<Fs> z2 = fe_sqr<Fs>(z);
  if (fe_eq<Fs>(z, one) || !fe_eq<Fs>(fe_mul<Fs>(z2, z), one))
    return set_error(PM_ERR_ARG, "zeta is not a primitive cube root of unity");
  Fe<Fs> h = we;  // omega_e^(N/2), passing omega = omega_e^(2^e) on the way
  Fe<Fs> w = we;
  for (uint32_t i = 0; i + 1 < ext_k; i++) {
    h = fe_sqr<Fs>(h);
    if (i + 1 == e) w = h;
  }
  if (e == ext_k && ext_k) w = fe_sqr<Fs>(h);  // k = 0: omega = omega_e^N = 1
  if (ext_k == 0 ? !fe_eq<Fs>(we, one) : !fe_eq<Fs>(h, fe_neg<Fs>(one)))
    return set_error(PM_ERR_ARG, "extended_omega is not a primitive 2^extended_k-th root of unity");
  const Fe<Fs> we_inv = fe_inv_bgcd<Fs>(we);
  Fe<Fs> nn = one, to261 = one;  // N and 2^5 in Montgomery form
  for (uint32_t i = 0; i < ext_k; i++) nn = fe_dbl<Fs>(nn);
  for (int i = 0; i < 5; i++) to261 = fe_dbl<Fs>(to261);
  const Fe<Fs> n_inv = fe_inv_bgcd<Fs>(nn);
  tab->clear();
  dom_put<Fs>(tab, one, to261);
  dom_put<Fs>(tab, z, to261);
  dom_put<Fs>(tab, z2, to261);
  dom_put<Fs>(tab, n_inv, to261);
  dom_put<Fs>(tab, fe_mul<Fs>(n_inv, z2), to261);  // zeta^-1 = zeta^2
  dom_put<Fs>(tab, fe_mul<Fs>(n_inv, z), to261);   // zeta^-2 = zeta
  // t_i = (zeta^n (omega_e^n)^i - 1)^-1; zeta^(2^k) = zeta for even k, zeta^2 for odd
  Fe<Fs> wn = we;
  for (uint32_t i = 0; i < k; i++) wn = fe_sqr<Fs>(wn);
  Fe<Fs> cur = (k & 1) ? z2 : z;
  for (uint32_t i = 0; i < (1u << e); i++) {
    const Fe<Fs> den = fe_sub<Fs>(cur, one);
    if (fe_is_zero<Fs>(den)) return set_error(PM_ERR_ARG, "the coset meets the domain");  // unreachable: orders 3 and 2^e
    dom_put<Fs>(tab, fe_inv_bgcd<Fs>(den), to261);
    cur = fe_mul<Fs>(cur, wn);
  }
  auto out = [](const Fe<Fs>& v, uint64_t* o) {
    for (int i = 0; i < 4; i++) o[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
  };
  out(w, d->omega);
  out(we, d->omega_e);
  out(we_inv, d->omega_e_inv);
  return PM_OK;
}

constexpr int kDomTabZeta = 0, kDomTabScale = 3, kDomTabT = 6;  // entries of pm_domain::d_tab

template <class Cv>
int domain_run_impl(Ctx* ctx, const DomJob* jp) {
  using Fs = typename Cv::Scalar;
  const DomJob& j = *jp;
  const hipStream_t st = ctx->stream;
  const uint32_t logn = j.logn;
  const size_t N = (size_t)1 << logn, C = j.C;
  const size_t stride = 8 * N;  // words per scratch row
  const uint32_t* dtab = j.dom ? (const uint32_t*)j.dom->d_tab.p : nullptr;
  const uint32_t e = j.dom ? j.dom->ext_k - j.dom->k : 0;
  const int passes = logn <= (uint32_t)kNttOnePassLog ? 1 : ntt_passes(ctx, logn);
  // every buffer is sized before the first launch is queued
  const bool via_scratch = passes >= 2 || j.op == kDomOpToCoeff;
  const size_t G = j.op == kDomOpDivide ? C : std::min(C, std::max<size_t>(1, kDomScratchBytes / (N * 32)));
  int rc;
  if ((rc = ctx->dom_ptrs.ensure(2 * C * sizeof(void*)))) return rc;
  if (j.op != kDomOpDivide && via_scratch && (rc = ctx->ntt_scratch.ensure(G * N * 32))) return rc;
  if (j.op != kDomOpDivide && passes == 3 && (rc = ctx->ntt_scratch2.ensure(G * N * 32))) return rc;
  NttPlan pl{};
  if (j.op != kDomOpDivide && (rc = ntt_plan<Fs>(ctx, j.curve, logn, j.omega, &pl))) return rc;
  std::vector<const void*> host(2 * C);
  for (size_t c = 0; c < C; c++) {
    host[c] = j.d_in ? j.d_in[c] : j.d_out[c];
    host[C + c] = j.d_out[c];
  }
  HIP_TRY(hipMemcpyAsync(ctx->dom_ptrs.p, host.data(), 2 * C * sizeof(void*), hipMemcpyHostToDevice, st));
  uint32_t* const* in_tab = (uint32_t* const*)ctx->dom_ptrs.p;
  uint32_t* const* out_tab = in_tab + C;

  if (j.op == kDomOpDivide) {
    const unsigned bx = (unsigned)std::max<size_t>(1, (N + 4 * kDomDivThreads - 1) / (4 * kDomDivThreads));
    PM_LAUNCH(ctx, "dom_divide", (k_dom_divide<Fs><<<dim3(bx, (unsigned)C), kDomDivThreads, 0, st>>>(
                                     out_tab, (uint32_t)N, dtab + 8 * kDomTabT, (1u << e) - 1u)));
    HIP_TRY(hipStreamSynchronize(st));
    ctx->end_call();
    return PM_OK;
  }

  const int log1 = pl.log1, loga = pl.loga, logb = pl.logb, s2 = pl.s2;
  const unsigned nt = passes == 3 ? kNttThreads3 : kNttThreads2;
  const FeArg sc = j.scale ? fearg_from_u64<Fs>(j.scale) : FeArg{};
  uint32_t* tmp = (uint32_t*)ctx->ntt_scratch.p;
  uint32_t* tmp2 = (uint32_t*)ctx->ntt_scratch2.p;
  // first-pass loader and last-pass epilogue of the operation
  const uint32_t* ld_tab = nullptr;
  uint32_t ld_lim = 0;
  int ld_mode = kDomPlain;
  if (j.op == kDomOpToExt) {
    ld_mode = kDomCoset;
    ld_tab = dtab + 8 * kDomTabZeta;
    ld_lim = 1u << j.dom->k;
  } else if (j.op == kDomOpToCoeff && (j.flags & kDomDivideVanishing)) {
    ld_mode = kDomVanish;
    ld_tab = dtab + 8 * kDomTabT;
    ld_lim = (1u << e) - 1u;
  }
  const bool coset_store = j.op == kDomOpToCoeff;
  const uint32_t* st_tab = coset_store ? dtab + 8 * kDomTabScale : nullptr;
  const uint32_t keep = coset_store ? (uint32_t)j.keep : 0u;
  const uint32_t use_scale = j.scale ? 1u : 0u;

  // pass A over `cols` columns from the caller's buffers
  auto launch_cols = [&](unsigned bx, unsigned cols, size_t lds, uint32_t* const* it, uint32_t* const* ot, uint32_t* ob,
                         int lg1, int logC, uint32_t last) -> int {
    const dim3 grid(bx, cols);
    switch (ld_mode) {
      case kDomCoset:
        PM_LAUNCH(ctx, "dom_cols", (k_dom_cols<Fs, kDomCoset><<<grid, nt, lds, st>>>(
                                       it, nullptr, ot, ob, stride, (int)logn, lg1, logC, pl.twA, pl.twLo, pl.twHi, s2,
                                       last, ld_tab, ld_lim)));
        break;
      case kDomVanish:
        PM_LAUNCH(ctx, "dom_cols", (k_dom_cols<Fs, kDomVanish><<<grid, nt, lds, st>>>(
                                       it, nullptr, ot, ob, stride, (int)logn, lg1, logC, pl.twA, pl.twLo, pl.twHi, s2,
                                       last, ld_tab, ld_lim)));
        break;
      default:
        PM_LAUNCH(ctx, "dom_cols", (k_dom_cols<Fs, kDomPlain><<<grid, nt, lds, st>>>(
                                       it, nullptr, ot, ob, stride, (int)logn, lg1, logC, pl.twA, pl.twLo, pl.twHi, s2,
                                       last, ld_tab, ld_lim)));
    }
    return PM_OK;
  };
  // pass B over `cols` columns into the caller's buffers
  auto launch_rows = [&](unsigned bx, unsigned cols, size_t lds, uint32_t* const* it, uint32_t* ib, uint32_t* const* ot,
                         int lg2, int logR) -> int {
    const dim3 grid(bx, cols);
    if (coset_store)
      PM_LAUNCH(ctx, "dom_rows", (k_dom_rows<Fs, kDomCoset><<<grid, nt, lds, st>>>(
                                     it, ib, ot, nullptr, stride, (int)logn, lg2, logR, pl.twB, sc, 0u, st_tab, keep)));
    else
      PM_LAUNCH(ctx, "dom_rows", (k_dom_rows<Fs, kDomPlain><<<grid, nt, lds, st>>>(
                                     it, ib, ot, nullptr, stride, (int)logn, lg2, logR, pl.twB, sc, use_scale, nullptr,
                                     0u)));
    return PM_OK;
  };

  for (size_t g0 = 0; g0 < C; g0 += G) {
    const unsigned cols = (unsigned)std::min(G, C - g0);
    uint32_t* const* it = in_tab + g0;
    uint32_t* const* ot = out_tab + g0;
    if (passes == 1) {
      // one sub-transform in LDS per column; what follows it (pm_fft's scale,
      // the coset store) rides on a rows pass of one element per row
      const bool tail = coset_store || use_scale;
      const int logR = (int)std::min<uint32_t>(logn, 8);
      if ((rc = launch_cols(1, cols, N * kNttLdsBytes, it, via_scratch ? nullptr : ot, via_scratch ? tmp : nullptr,
                            (int)logn, 0, tail ? 0u : 1u)))
        return rc;
      if (tail && (rc = launch_rows((unsigned)(N >> logR), cols, ((size_t)1 << logR) * kNttLdsBytes,
                                    via_scratch ? nullptr : ot, via_scratch ? tmp : nullptr, ot, 0, logR)))
        return rc;
    } else if (passes == 2) {
      const int logC = std::max(0, std::min(kNttMaxLogC, kNttPlaneLog - log1)),
                logR = std::max(0, std::min(kNttMaxLogC, kNttPlaneLog - logb));
      const size_t ldsA = ((size_t)1 << (log1 + logC)) * kNttLdsBytes, ldsB = ((size_t)1 << (logb + logR)) * kNttLdsBytes;
      if ((rc = launch_cols((unsigned)((size_t)1 << (logb - logC)), cols, ldsA, it, nullptr, tmp, log1, logC, 0u)))
        return rc;
      if ((rc = launch_rows((unsigned)((size_t)1 << (log1 - logR)), cols, ldsB, nullptr, tmp, ot, logb, logR))) return rc;
    } else {
      const int logC = std::max(0, std::min(kNttMaxLogC, kNttPlaneLog - log1)),
                logM = std::max(0, std::min(kNttMaxLogC, kNttPlaneLog - loga)),
                logR = std::max(0, std::min(kNttMaxLogC, kNttPlaneLog - logb));
      const size_t ldsA = ((size_t)1 << (log1 + logC)) * kNttLdsBytes, ldsM = ((size_t)1 << (loga + logM)) * kNttLdsBytes,
                   ldsB = ((size_t)1 << (logb + logR)) * kNttLdsBytes;
      if ((rc = launch_cols((unsigned)(N >> (log1 + logC)), cols, ldsA, it, nullptr, tmp, log1, logC, 0u))) return rc;
      PM_LAUNCH(ctx, "dom_mid", (k_dom_mid<Fs><<<dim3((unsigned)(N >> (loga + logM)), cols), nt, ldsM, st>>>(
                                    tmp, tmp2, stride, (int)logn, log1, loga, logM, pl.twM, pl.twLo, pl.twHi, s2)));
      if ((rc = launch_rows((unsigned)(N >> (logb + logR)), cols, ldsB, nullptr, tmp2, ot, logb, logR))) return rc;
    }
  }
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

}  // namespace pm

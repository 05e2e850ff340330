// gp_engine.hpp -- host driver of the grand products and the batch inversion
// (pm_grand_product_device, pm_batch_invert*).  Boundary: halo2
// plonk/permutation/prover.rs::commit, plonk/lookup/prover.rs::commit_product
// and ff::BatchInvert [3P], reached from create_proof
// (examples/simple-example.rs:663-710).  Arguments are validated by the C-ABI
// (capi_poly.hip) before this runs.
#pragma once
#include <cstring>
#include <vector>

#include "engine.hpp"
#include "gp_kernels.hpp"

namespace pm {

constexpr uint32_t kGpChain = 1u;             // PM_GP_CHAIN

// flags & kGpInvert (runtime.hpp): the batch inversion; d_out holds the n values, every list argument is ignored
template <class Cv>
int grand_product_impl(Ctx* ctx, int curve, const void* const* d_cols, size_t C, size_t n, const pm_gp_factor* num,
                       const uint32_t* num_off, const pm_gp_factor* den, const uint32_t* den_off, size_t S,
                       const uint64_t* omega, const uint64_t* start, size_t active, uint32_t flags, void* d_out,
                       uint64_t* out_last) {
  using Fs = typename Cv::Scalar;
  static_assert(sizeof(pm_gp_factor) == kGpFactorWords * 4, "pm_gp_factor is read as 18 words");
  const hipStream_t st = ctx->stream;
  const bool invert = flags & kGpInvert;
  pm_gp_factor self{};
  const uint32_t one_list[2] = {0, 1};
  if (invert) {
    self.x = 0;
    self.y = kGpNone;
    d_cols = &d_out;
    C = S = 1;
    num = den = &self;
    num_off = den_off = one_list;
    omega = start = nullptr;
    active = n;
  }
  const size_t Fn = num_off[S], Fd = den_off[S], F = Fn + Fd;
  bool any_omega = false;
  for (size_t i = 0; i < Fn; i++) any_omega |= num[i].y == kGpOmega;
  for (size_t i = 0; i < Fd; i++) any_omega |= den[i].y == kGpOmega;
  const uint32_t nblk = (uint32_t)((n + kPolyTile - 1) >> kPolyTileLog);
  const size_t tiles = S * (size_t)nblk;

  // one upload: [omega | start | column pointers | numerator, denominator factors | the two offset lists]
  const size_t off_ptrs = 64, off_fac = off_ptrs + C * sizeof(void*), off_words = off_fac + F * sizeof(pm_gp_factor);
  std::vector<uint8_t> host(off_words + 2 * (S + 1) * 4, 0);
  if (omega) std::memcpy(host.data(), omega, 32);
  if (start) std::memcpy(host.data() + 32, start, 32);
  if (C) std::memcpy(host.data() + off_ptrs, d_cols, C * sizeof(void*));
  if (Fn) std::memcpy(host.data() + off_fac, num, Fn * sizeof(pm_gp_factor));
  if (Fd) std::memcpy(host.data() + off_fac + Fn * sizeof(pm_gp_factor), den, Fd * sizeof(pm_gp_factor));
  std::memcpy(host.data() + off_words, num_off, (S + 1) * 4);
  {
    // the denominators follow the numerators in the one factor table
    uint32_t* d = reinterpret_cast<uint32_t*>(host.data() + off_words) + S + 1;
    for (size_t j = 0; j <= S; j++) d[j] = den_off[j] + (uint32_t)Fn;
  }

  // scratch, in 32-byte entries: lane carries, tile aggregates and carries
  // (pairs), per set [total N, inverse, scale], last, K pairs; then the
  // converted factor table and the first-zero indices
  const size_t e_lane_d = tiles * kPolyThreads, e_agg = 2 * e_lane_d, e_carry = e_agg + 2 * tiles,
               e_setv = e_carry + 2 * tiles, e_last = e_setv + 3 * S, e_kform = e_last + S, e_fac = e_kform + 2 * S;
  const size_t fac_bytes = (F * sizeof(pm_gp_factor) + 31) / 32 * 32;
  int rc;
  if ((rc = ctx->poly_job.ensure(host.size())) || (rc = ctx->gp_tab.ensure(kPolyTabStride * 32)) ||
      (rc = ctx->poly_aux.ensure(e_fac * 32 + fac_bytes + S * 4)) ||
      (rc = ctx->gp_rows.ensure(S * n * 32)))
    return rc;
  HIP_TRY(hipMemcpyAsync(ctx->poly_job.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
  const char* job = (const char*)ctx->poly_job.p;
  uint32_t* aux = (uint32_t*)ctx->poly_aux.p;
  uint32_t* lane_n = aux;
  uint32_t* lane_d = aux + e_lane_d * 8;
  uint32_t* agg = aux + e_agg * 8;
  uint32_t* carry = aux + e_carry * 8;
  uint32_t* setv = aux + e_setv * 8;
  uint32_t* last = aux + e_last * 8;
  uint32_t* kform = aux + e_kform * 8;
  uint32_t* fac = aux + e_fac * 8;
  uint32_t* zidx = fac + fac_bytes / 4;
  uint32_t* tab = (uint32_t*)ctx->gp_tab.p;
  uint32_t* sd = (uint32_t*)ctx->gp_rows.p;
  GpJob jb{};
  jb.cols = (const uint32_t* const*)(job + off_ptrs);
  jb.num = fac;
  jb.den = fac;
  jb.num_off = (const uint32_t*)(job + off_words);
  jb.den_off = jb.num_off + S + 1;
  jb.kform = kform;
  jb.tab = any_omega ? tab : nullptr;
  jb.S = (uint32_t)S;
  jb.nblk = nblk;
  jb.invert = invert ? 1u : 0u;
  jb.n = n;
  jb.prod_rows = invert ? n : active - 1;
  jb.store_rows = active;
  if (any_omega) {
    // omega^(2^k) up to the largest tile offset, (nblk - 1) 2^11; kept across calls (runtime.hpp)
    uint32_t bits = 0;
    for (uint32_t b = nblk; b; b >>= 1) bits++;
    const uint32_t need = (uint32_t)kPolyTileLog + bits, nsq = need < 12u ? 12u : (need > 29u ? 29u : need);
    if (ctx->gp_tab_gen != ctx->gp_tab.gen || ctx->gp_tab_curve != curve || ctx->gp_tab_nsq < nsq ||
        std::memcmp(ctx->gp_tab_omega, omega, 32) != 0) {
      ctx->gp_tab_gen = ~0ull;  // not valid until the launch below is queued
      PM_LAUNCH(ctx, "poly_table", (k_poly_table<Fs><<<1, kPolyThreads, 0, st>>>((const uint32_t*)job, 1u, nsq, tab)));
      ctx->gp_tab_gen = ctx->gp_tab.gen;
      ctx->gp_tab_curve = curve;
      ctx->gp_tab_nsq = nsq;
      std::memcpy(ctx->gp_tab_omega, omega, 32);
    }
  }
  const unsigned prep_threads = (unsigned)(F + 2 * S);  // one per factor, then one per list (>= S: the zidx resets)
  PM_LAUNCH(ctx, "gp_prep", (k_gp_prep<Fs><<<(prep_threads + 255u) / 256u, 256, 0, st>>>(
                                (const uint32_t*)(job + off_fac), fac, (uint32_t)F, jb.num_off, jb.den_off,
                                (uint32_t)S, kform, zidx)));
  const dim3 grid(nblk, (unsigned)S);
  PM_LAUNCH(ctx, "gp_local", (k_gp_local<Fs><<<grid, kPolyThreads, kPolyDivLds, st>>>(jb, (uint32_t*)d_out, sd, lane_n,
                                                                                       lane_d, agg, zidx)));
  PM_LAUNCH(ctx, "gp_carry", (k_gp_carry<Fs><<<(unsigned)S, kPolyThreads, 0, st>>>(jb, agg, carry, setv)));
  PM_LAUNCH(ctx, "gp_chain", (k_gp_chain<Fs><<<1, 64, 0, st>>>(jb, (const uint32_t*)(job + 32), flags & kGpChain,
                                                               zidx, setv, last)));
  PM_LAUNCH(ctx, "gp_sweep", (k_gp_sweep<Fs><<<grid, kPolyThreads, 0, st>>>(jb, (uint32_t*)d_out, sd, lane_n, lane_d,
                                                                            carry, setv, zidx)));
  if (out_last && !invert) HIP_TRY(hipMemcpyAsync(out_last, last, S * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

}  // namespace pm

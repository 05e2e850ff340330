// poly_engine.hpp -- host driver of the polynomial openings (pm_poly_eval*,
// pm_multiopen_witness*).  Boundary: halo2 `eval_polynomial`,
// `kate_division` [3P] and the witness loop of poly/multiopen/gwc/prover.rs
// [3P], reached from create_proof (examples/simple-example.rs:606,702).
// Arguments are validated by the C-ABI (capi_poly.hip) before these run.
#pragma once
#include <cstring>
#include <vector>

#include "engine.hpp"
#include "poly_kernels.hpp"

namespace pm {

// One upload per call: [points, 32 B each | polynomial pointers | u32 words]
struct PolyUpload {
  std::vector<uint8_t> host;
  size_t off_ptrs = 0, off_words = 0;
  PolyUpload(const uint64_t* points, size_t npts, const uint64_t* extra_point, const void* const* d_polys, size_t P,
             size_t nwords) {
    const size_t np = npts + (extra_point ? 1 : 0);
    off_ptrs = np * 32;
    off_words = off_ptrs + P * sizeof(void*);
    host.resize(off_words + nwords * 4);
    if (npts) std::memcpy(host.data(), points, npts * 32);
    if (extra_point) std::memcpy(host.data() + npts * 32, extra_point, 32);
    if (P) std::memcpy(host.data() + off_ptrs, d_polys, P * sizeof(void*));
  }
  uint32_t* words() { return reinterpret_cast<uint32_t*>(host.data() + off_words); }
};

template <class Cv>
int poly_witness_impl(Ctx* ctx, const void* const* d_polys, size_t P, size_t n, const uint32_t* set_offsets,
                      const uint32_t* set_polys, const uint64_t* points, const uint64_t* v, size_t S, void* d_out,
                      uint64_t* out_evals) {
  using Fs = typename Cv::Scalar;
  const hipStream_t st = ctx->stream;
  const size_t M = set_offsets[S];
  const uint32_t nblk = (uint32_t)((n + kPolyTile - 1) >> kPolyTileLog);
  PolyUpload up(points, S, v, d_polys, P, S + 1 + M);
  std::memcpy(up.words(), set_offsets, (S + 1) * 4);
  if (M) std::memcpy(up.words() + S + 1, set_polys, M * 4);
  const size_t tiles = S * (size_t)nblk;
  int rc;
  if ((rc = ctx->poly_job.ensure(up.host.size())) || (rc = ctx->poly_tab.ensure((S + 1) * kPolyTabStride * 32)) ||
      (rc = ctx->poly_aux.ensure((tiles * (kPolyThreads + 2) + S) * 32)))
    return rc;
  HIP_TRY(hipMemcpyAsync(ctx->poly_job.p, up.host.data(), up.host.size(), hipMemcpyHostToDevice, st));
  const char* job = (const char*)ctx->poly_job.p;
  uint32_t* tab = (uint32_t*)ctx->poly_tab.p;
  uint32_t* lane_carry = (uint32_t*)ctx->poly_aux.p;
  uint32_t* agg = lane_carry + tiles * kPolyThreads * 8;
  uint32_t* carry = agg + tiles * 8;
  uint32_t* evals = carry + tiles * 8;
  PolyJob jb{};
  jb.polys = (const uint32_t* const*)(job + up.off_ptrs);
  jb.set_offsets = (const uint32_t*)(job + up.off_words);
  jb.set_polys = jb.set_offsets + S + 1;
  jb.tab = tab;
  jb.S = (uint32_t)S;
  jb.nblk = nblk;
  jb.n = n;
  PM_LAUNCH(ctx, "poly_table",
            (k_poly_table<Fs><<<(unsigned)(S + 1), kPolyThreads, 0, st>>>((const uint32_t*)job, (uint32_t)(S + 1),
                                                                           poly_table_squarings(nblk, kPolyTileLog), tab)));
  const dim3 grid(nblk, (unsigned)S);
  PM_LAUNCH(ctx, "poly_div_local", (k_poly_div_local<Fs><<<grid, kPolyThreads, kPolyDivLds, st>>>(
                                       jb, (uint32_t*)d_out, lane_carry, agg)));
  PM_LAUNCH(ctx, "poly_div_carry", (k_poly_div_carry<Fs><<<(unsigned)S, kPolyThreads, 0, st>>>(jb, agg, carry)));
  PM_LAUNCH(ctx, "poly_div_sweep", (k_poly_div_sweep<Fs><<<grid, kPolyThreads, 0, st>>>(jb, (uint32_t*)d_out,
                                                                                          lane_carry, carry, evals)));
  if (out_evals) HIP_TRY(hipMemcpyAsync(out_evals, evals, S * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

template <class Cv>
int poly_eval_impl(Ctx* ctx, const void* const* d_polys, size_t P, size_t n, const uint32_t* poly_index,
                   const uint64_t* points, size_t E, uint64_t* out_evals) {
  using Fs = typename Cv::Scalar;
  const hipStream_t st = ctx->stream;
  const uint32_t nblk = (uint32_t)((n + kPolyEvalTile - 1) >> kPolyEvalTileLog);
  PolyUpload up(points, E, nullptr, d_polys, P, E);
  std::memcpy(up.words(), poly_index, E * 4);
  int rc;
  if ((rc = ctx->poly_job.ensure(up.host.size())) || (rc = ctx->poly_tab.ensure(E * kPolyTabStride * 32)) ||
      (rc = ctx->poly_aux.ensure((E * (size_t)nblk + E) * 32)))
    return rc;
  HIP_TRY(hipMemcpyAsync(ctx->poly_job.p, up.host.data(), up.host.size(), hipMemcpyHostToDevice, st));
  const char* job = (const char*)ctx->poly_job.p;
  uint32_t* tab = (uint32_t*)ctx->poly_tab.p;
  uint32_t* part = (uint32_t*)ctx->poly_aux.p;
  uint32_t* out = part + E * (size_t)nblk * 8;
  PM_LAUNCH(ctx, "poly_table",
            (k_poly_table<Fs><<<(unsigned)E, kPolyThreads, 0, st>>>((const uint32_t*)job, (uint32_t)E,
                                                                     poly_table_squarings(nblk, kPolyEvalTileLog), tab)));
  PM_LAUNCH(ctx, "poly_eval_part", (k_poly_eval_part<Fs><<<dim3(nblk, (unsigned)E), kPolyThreads, 0, st>>>(
                                       (const uint32_t* const*)(job + up.off_ptrs),
                                       (const uint32_t*)(job + up.off_words), n, tab, part)));
  PM_LAUNCH(ctx, "poly_eval_comb", (k_poly_eval_comb<Fs><<<(unsigned)E, kPolyThreads, 0, st>>>(part, nblk, tab, out)));
  HIP_TRY(hipMemcpyAsync(out_evals, out, E * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

}  // namespace pm

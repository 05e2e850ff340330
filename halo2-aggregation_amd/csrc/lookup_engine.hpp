// lookup_engine.hpp -- host driver of the lookup argument's permuted columns
// (pm_lookup_compress_device, pm_lookup_permute*).  Boundary:
// halo2 plonk/lookup/prover.rs::compress_expressions and
// permute_expression_pair [3P], reached from create_proof between the advice
// commit and commit_product.  Arguments are validated by the C-ABI
// (capi_lookup.hip) before this runs.
#pragma once
#include <cstring>
#include <vector>

#include "engine.hpp"
#include "lookup_kernels.hpp"

namespace pm {

// theta may be null when m == 1 (the kernel does not read it)
template <class Cv>
int lookup_compress_impl(Ctx* ctx, const void* const* d_cols, size_t m, size_t n, const uint64_t* theta, void* d_out) {
  using Fs = typename Cv::Scalar;
  const hipStream_t st = ctx->stream;
  // one upload: [theta | column pointers]
  std::vector<uint8_t> host(32 + m * sizeof(void*), 0);
  if (theta) std::memcpy(host.data(), theta, 32);
  std::memcpy(host.data() + 32, d_cols, m * sizeof(void*));
  int rc;
  if ((rc = ctx->lk_job.ensure(host.size()))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->lk_job.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
  const char* job = (const char*)ctx->lk_job.p;
  const unsigned grid = (unsigned)((n + kPolyThreads - 1) / kPolyThreads);
  PM_LAUNCH(ctx, "lk_compress", (k_lk_compress<Fs><<<grid, kPolyThreads, 0, st>>>(
                                    (const uint32_t* const*)(job + 32), (uint32_t)m, n, (const uint32_t*)job,
                                    (uint32_t*)d_out)));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

// merge passes over the sorted tiles of `usable` keys
inline uint32_t lookup_merge_passes(size_t usable) {
  uint32_t passes = 0;
  for (size_t run = kLkTile; run < usable; run <<= 1) passes++;
  return passes;
}
// one key buffer of a permute call: 2 P columns of `usable` canonical keys
inline size_t lookup_key_bytes(size_t P, size_t usable) { return 2 * P * usable * 32; }

template <class Cv>
int lookup_permute_impl(Ctx* ctx, const void* const* d_a, const void* const* d_s, size_t P, size_t usable,
                        void* const* d_out_a, void* const* d_out_s, uint32_t* out_status) {
  using Fs = typename Cv::Scalar;
  const hipStream_t st = ctx->stream;
  const size_t u = usable;
  const uint32_t tiles = (uint32_t)((u + kLkTile - 1) >> kLkTileLog);
  const uint32_t nblk = (uint32_t)((u + kLkThreads - 1) / kLkThreads);

  // one upload: [input pointers a_0, s_0, ... | output pointers out_a_0, out_s_0, ...]
  std::vector<const void*> host(4 * P);
  for (size_t p = 0; p < P; p++) {
    host[2 * p] = d_a[p];
    host[2 * p + 1] = d_s[p];
    host[2 * P + 2 * p] = d_out_a[p];
    host[2 * P + 2 * p + 1] = d_out_s[p];
  }
  // scratch, sized for the whole call before the first launch is queued (the header states it per
  // pair): the two key buffers; in words the row map, the block counts, the totals and the failing
  // rows; then the leftover flags, a byte per row
  const size_t w_rowof = 0, w_cnt = w_rowof + P * u, w_tot = w_cnt + 2 * P * nblk, w_fail = w_tot + 2 * P,
               w_end = w_fail + P;
  int rc;
  if ((rc = ctx->lk_job.ensure(host.size() * sizeof(void*))) ||
      (rc = ctx->lk_keys.ensure(2 * lookup_key_bytes(P, u))) || (rc = ctx->lk_aux.ensure(w_end * 4 + P * u)))
    return rc;
  HIP_TRY(hipMemcpyAsync(ctx->lk_job.p, host.data(), host.size() * sizeof(void*), hipMemcpyHostToDevice, st));
  uint32_t* aux = (uint32_t*)ctx->lk_aux.p;
  uint32_t* keys[2] = {(uint32_t*)ctx->lk_keys.p, (uint32_t*)((char*)ctx->lk_keys.p + lookup_key_bytes(P, u))};
  LkJob jb{};
  jb.in = (const uint32_t* const*)ctx->lk_job.p;
  jb.out = (uint32_t* const*)ctx->lk_job.p + 2 * P;
  jb.rowof = aux + w_rowof;
  jb.cnt = aux + w_cnt;
  jb.tot = aux + w_tot;
  jb.fail = aux + w_fail;
  jb.left = (uint8_t*)(aux + w_end);
  jb.usable = (uint32_t)u;
  jb.nblk = nblk;

  const dim3 sort_grid(tiles, (unsigned)(2 * P)), pair_grid(nblk, (unsigned)P);
  PM_LAUNCH(ctx, "lk_tile_sort", (k_lk_tile_sort<Fs><<<sort_grid, kLkThreads, kLkLds, st>>>(jb, keys[0])));
  const uint32_t passes = lookup_merge_passes(u);
  for (uint32_t k = 0; k < passes; k++)
    PM_LAUNCH(ctx, "lk_merge", (k_lk_merge<<<sort_grid, kLkThreads, kLkLds, st>>>(keys[k & 1], keys[(k + 1) & 1],
                                                                                   (uint32_t)u, kLkTileLog + k)));
  const uint32_t* sorted = keys[passes & 1];
  PM_LAUNCH(ctx, "lk_flags", (k_lk_flags<<<pair_grid, kLkThreads, 0, st>>>(jb, sorted)));
  PM_LAUNCH(ctx, "lk_carry", (k_lk_carry<<<(unsigned)(2 * P), kScanThreads, 0, st>>>(jb)));
  PM_LAUNCH(ctx, "lk_rows", (k_lk_rows<Fs><<<pair_grid, kLkThreads, 0, st>>>(jb, sorted)));
  PM_LAUNCH(ctx, "lk_scatter", (k_lk_scatter<Fs><<<pair_grid, kLkThreads, 0, st>>>(jb, sorted)));
  std::vector<uint32_t> fail(P);
  HIP_TRY(hipMemcpyAsync(fail.data(), jb.fail, P * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t p = 0; p < P; p++) {
    const bool bad = fail[p] != kLkNoRow;
    out_status[2 * p] = bad ? 1u : 0u;
    out_status[2 * p + 1] = bad ? fail[p] : 0u;
  }
  ctx->end_call();
  return PM_OK;
}

}  // namespace pm

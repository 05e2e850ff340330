// pairing_batch_engine.hpp -- host driver of the batch decider
// (pm_accum_decide_batch*, pm_verify_proofs_batch_device).
// Arguments are validated by the C-ABI (capi_pairing_batch.hip) before this
// runs.  The driver and its kernels are compiled by pairing_batch_bn254.hip
// alone (PM_PAIRING_BATCH_IMPL).
#pragma once
#include "pairing_batch_host.hpp"
#include "pairing_engine.hpp"

namespace pm {
namespace pairing {

// The caller holds ctx->mu and has called begin_call.  d_status_in,
// d_out_item_ok, d_out_status and out_pair may be null.  Synchronises the stream.
int decide_batch_device(Ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads, const void* d_status_in,
                        const uint64_t seed[4], uint32_t flags, uint32_t* out_ok, void* d_out_item_ok,
                        void* d_out_status, uint64_t* out_pair);

}  // namespace pairing
}  // namespace pm

#ifdef PM_PAIRING_BATCH_IMPL
#include <chrono>
#include <cstdlib>

#include "pairing_batch_kernels.hpp"

namespace pm {
namespace pairing {

// the launches between two events when the phase is timed (pm_ctx_kernel_stats)
#define PM_BATCH_LAUNCH(ctx, name, ...)                                                                       \
  do {                                                                                                        \
    hipEvent_t a_ = nullptr, b_ = nullptr;                                                                    \
    const bool tm_ = (ctx)->timed(name);                                                                      \
    if (tm_) {                                                                                                \
      a_ = (ctx)->next_event();                                                                               \
      b_ = (ctx)->next_event();                                                                               \
      (void)hipEventRecord(a_, (ctx)->stream);                                                                \
    }                                                                                                         \
    __VA_ARGS__;                                                                                              \
    hipError_t le_ = hipGetLastError();                                                                       \
    if (le_ != hipSuccess)                                                                                    \
      return pm::set_error(PM_ERR_HIP, std::string("launch ") + (name) + ": " + hipGetErrorString(le_));     \
    if (tm_) {                                                                                                \
      (void)hipEventRecord(b_, (ctx)->stream);                                                                \
      (ctx)->mark((name), a_, b_);                                                                            \
    }                                                                                                         \
  } while (0)

int decide_batch_device(Ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads, const void* d_status_in,
                        const uint64_t seed[4], uint32_t flags, uint32_t* out_ok, void* d_out_item_ok,
                        void* d_out_status, uint64_t* out_pair) {
  const hipStream_t st = ctx->stream;
  int rc;
  // host phases (recorded with the kernels' when timing is on): decide_batch_horner, decide_batch_pairing
  auto phase = [&](const char* name, std::chrono::steady_clock::time_point t0) {
    if (!ctx->timing) return;
    auto& stt = ctx->stats[name];
    stt.first += 1;
    stt.second += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  // items per chunk: kBatchChunk; PM_DECIDE_BATCH_CHUNK (test hook, as PM_NTT_PASSES: 64 .. kBatchChunk)
  // lets tests/test_decide_batch_gpu.py cross the chunk boundary without a batch of 2^16 items
  size_t chunk = kBatchChunk;
  if (const char* e = std::getenv("PM_DECIDE_BATCH_CHUNK")) {
    const long v = std::atol(e);
    if (v >= (long)kBatchQuads && v <= (long)kBatchChunk) chunk = (size_t)v;
  }
  const size_t cap = B < chunk ? B : chunk;  // items of the largest chunk
  const BatchPlan big = batch_plan(cap);
  if ((rc = ctx->pair_io.ensure(batch_bases_bytes(cap) + kBatchSlots * sizeof(uint32_t)))) return rc;
  if ((rc = ctx->small_dig.ensure(batch_digits_bytes(cap)))) return rc;
  if ((rc = ctx->small_tab.ensure(2 * cap * kSmallMults * sizeof(Xyzz<Fq>)))) return rc;
  if ((rc = ctx->small_part.ensure((size_t)kBatchSlots * big.ns * sizeof(Xyzz<Fq>)))) return rc;
  // window sums and the any-status word in mapped host memory: no copy back
  if ((rc = ctx->ensure_pinned(kBatchSlots * sizeof(Xyzz<Fq>) + 64))) return rc;
  uint32_t* bases = (uint32_t*)ctx->pair_io.p;
  uint32_t* tickets = (uint32_t*)((char*)ctx->pair_io.p + batch_bases_bytes(cap));
  int8_t* digits = (int8_t*)ctx->small_dig.p;
  Xyzz<Fq>* tab = (Xyzz<Fq>*)ctx->small_tab.p;
  Xyzz<Fq>* part = (Xyzz<Fq>*)ctx->small_part.p;
  Xyzz<Fq>* hW = (Xyzz<Fq>*)ctx->h_pinned;
  volatile uint32_t* hbad = (volatile uint32_t*)(hW + kBatchSlots);
  Xyzz<Fq>* dW = (Xyzz<Fq>*)ctx->h_pinned_dev;
  uint32_t* dbad = (uint32_t*)(dW + kBatchSlots);
  *hbad = 0;
  BatchSeed sd;
  std::memcpy(sd.w, seed, 32);
  J1 sum[kBatchOutputs] = {j1_inf(), j1_inf()};
  for (size_t i0 = 0; i0 < B; i0 += chunk) {
    const size_t n = B - i0 < chunk ? B - i0 : chunk;
    const BatchPlan bp = batch_plan(n);
    const BatchGeom g{(uint32_t)n, bp.kq, bp.ns};
    SmallGeom tg{};
    tg.n = 2u * (uint32_t)n;
    tg.r261 = 1u;
    const uint32_t nb_tab = (tg.n + kSmallTabPts - 1) / kSmallTabPts;
    const uint32_t* si = d_status_in ? (const uint32_t*)d_status_in + i0 : nullptr;
    uint32_t* so = d_out_status ? (uint32_t*)d_out_status + i0 : nullptr;
    HIP_TRY(hipMemsetAsync(tickets, 0, kBatchSlots * sizeof(uint32_t), st));
    PM_BATCH_LAUNCH(ctx, "decide_batch_prep",
                   (k_batch_prep<<<(unsigned)((n + kPrepBlock - 1) / kPrepBlock), kPrepBlock, 0, st>>>(
                       g.n, (uint64_t)i0, sd, (const uint64_t*)d_quads + i0 * 32, si, bases, digits, so, dbad)));
    // the table's digit blocks are not launched: the digits are k_batch_prep's
    PM_BATCH_LAUNCH(ctx, "decide_batch_sum",
                   (k_small_table<Bn254Curve><<<nb_tab, 256, 0, st>>>(tg, nb_tab, nullptr, bases, tab, nullptr),
                    k_batch_sum<<<dim3(g.ns, kBatchWin, kBatchOutputs), 256, 0, st>>>(g, tab, digits, part, tickets,
                                                                                       dW)));
    HIP_TRY(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    for (int o = 0; o < kBatchOutputs; o++) {
      J1 W[kBatchWin];
      for (int j = 0; j < kBatchWin; j++) std::memcpy(&W[j], &hW[o * kBatchWin + j], sizeof(J1));
      sum[o] = host::jadd<Fq>(sum[o], batch_horner(W));
    }
    phase("decide_batch_horner", t0);
  }
  const bool clean = *hbad == 0;
  const auto t1 = std::chrono::steady_clock::now();
  const G1 L = j1_affine(sum[0]), R = j1_affine(sum[1]);
  if (out_pair) {
    g1_to_words(L, out_pair);
    g1_to_words(R, out_pair + 8);
  }
  *out_ok = batch_decide(pr->host, clean, L, R);
  phase("decide_batch_pairing", t1);
  if ((flags & kDecideLocate) && d_out_item_ok) {
    if (*out_ok) {
      HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d_out_item_ok, 1, B, st));
      HIP_TRY(hipStreamSynchronize(st));
    } else if ((rc = decide_device(ctx, pr, B, d_quads, true, d_status_in, d_out_item_ok, nullptr, nullptr))) {
      return rc;  // the per-proof decider names the culprits
    }
  }
  ctx->end_call();
  return PM_OK;
}

}  // namespace pairing
}  // namespace pm
#endif  // PM_PAIRING_BATCH_IMPL

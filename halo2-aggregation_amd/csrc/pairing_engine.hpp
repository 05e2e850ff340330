// pairing_engine.hpp -- the pm_pairing object and the host driver of the BN254
// pairing decider (pm_pairing_check_device, pm_accum_decide*).
// Arguments are validated by the C-ABI (capi_pairing.hip) before this runs.
// capi_pairing.hip sees the object and the driver's declaration; the driver and
// its kernels are compiled by pairing_bn254.hip alone (PM_PAIRING_IMPL).
#pragma once
#include <vector>

#include "pairing_host.hpp"
#include "runtime.hpp"

// Both G2 arguments of the decider, checked, with their line tables: the host
// copy pm_accum_decide_host runs on, and (with a context) the device words
// [lines | Frobenius constants | program] of pairing_plan.hpp.
struct pm_pairing {
  int device = -1;  // -1: created without a context, host only
  pm::pairing::HostTables host;
  pm::Buf d_tab;
};

namespace pm {
namespace pairing {

// the device words of a pm_pairing (pairing_plan.hpp's layout)
inline std::vector<uint32_t> device_words(const HostTables& t) {
  std::vector<uint32_t> w((size_t)kDeviceWords);
  uint32_t* o = w.data();
  for (int s = 0; s < kSteps; s++)
    for (int pr = 0; pr < 2; pr++) {
      const LineCoef& lc = t.lines[pr][(size_t)s];
      const E1* v[4] = {&lc.lam.c0, &lc.lam.c1, &lc.c.c0, &lc.c.c1};
      for (int i = 0; i < 4; i++, o += 9) e1_to_words29(*v[i], o);
    }
  for (int j = 0; j < 2; j++)
    for (int k = 0; k < 6; k++) {
      e1_to_words29(t.frob[j][k].c0, o);
      e1_to_words29(t.frob[j][k].c1, o + 9);
      o += 18;
    }
  for (int i = 0; i < kProgOps; i++) *o++ = kProgram.w[i];
  return w;
}

// quad: d_in is B x 4 x 8 (w, zw, f, e), else B x 2 x 8 (A, C).  Synchronises the stream.
int decide_device(Ctx* ctx, const pm_pairing* pr, size_t B, const void* d_in, bool quad, const void* d_status_in,
                  void* d_out_ok, void* d_out_status, void* d_out_gt);

}  // namespace pairing
}  // namespace pm

#ifdef PM_PAIRING_IMPL
#include "pairing_kernels.hpp"

namespace pm {
namespace pairing {

#define PM_PAIR_LAUNCH(ctx, name, ...)                                                                        \
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

int decide_device(Ctx* ctx, const pm_pairing* pr, size_t B, const void* d_in, bool quad, const void* d_status_in,
                  void* d_out_ok, void* d_out_status, void* d_out_gt) {
  const hipStream_t st = ctx->stream;
  int rc;
  if ((rc = ctx->pair_io.ensure(pairing_scratch_bytes(B)))) return rc;
  uint32_t* items = (uint32_t*)ctx->pair_io.p;
  const unsigned prep_grid = (unsigned)((B + kPrepBlock - 1) / kPrepBlock);
  if (quad)
    PM_PAIR_LAUNCH(ctx, "pairing_prep",
                   (k_pairing_prep<true><<<prep_grid, kPrepBlock, 0, st>>>((uint32_t)B, (const uint64_t*)d_in,
                                                                           (const uint32_t*)d_status_in, items,
                                                                           (uint32_t*)d_out_status)));
  else
    PM_PAIR_LAUNCH(ctx, "pairing_prep",
                   (k_pairing_prep<false><<<prep_grid, kPrepBlock, 0, st>>>((uint32_t)B, (const uint64_t*)d_in,
                                                                            (const uint32_t*)d_status_in, items,
                                                                            (uint32_t*)d_out_status)));
  PM_PAIR_LAUNCH(ctx, "pairing_run",
                 (k_pairing_run<<<pairing_blocks(B), kPairBlock, 0, st>>>((uint32_t)B, (const uint32_t*)pr->d_tab.p, items,
                                                                          (uint32_t*)d_out_ok, (uint64_t*)d_out_gt)));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

}  // namespace pairing
}  // namespace pm
#endif  // PM_PAIRING_IMPL

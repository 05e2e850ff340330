// capi_internal.hpp -- what the units of the extern "C" boundary share
// (capi_ctx / capi_msm / capi_dropin / capi_poly / capi_lookup / capi_proofs /
// capi_selftest .hip).  Host only: no kernel header is included here.
#pragma once
#include <cstring>
#include <memory>
#include <mutex>
#include <string>

#include "runtime.hpp"

// Resident SRS bases: stored in the pipeline's R = 2^261 canonical form
// (converted once at upload), so pm_msm_resident* skips the per-call
// conversion.  From 2^18 points on the upload also keeps rows [2^{256 j / r}] P,
// j < r, with r = resident_rows(n) (8 rows up to 2^20 points, 4 up to 2^22,
// 2 above): a full-length resident MSM then runs as an r-row table MSM
// (pm_fixed_bases_create_rows), whose bucket reduction and host Horner are r
// times shorter (4 rows at 2^20: 1.61 -> 1.40 ms, profiles/r02/rows/).  Row 0
// is the bases themselves, so windows with an offset still run the plain
// pipeline on it.
struct pm_bases {
  int curve;
  int device;
  size_t n;
  // row 0 (64 B per point), not owning: the row table's memory when there is
  // one, else `own`
  const void* d;
  pm::Buf own;
  std::unique_ptr<pm_fixed_bases> table;  // rows > 1, or null
  // multiples table of pm_msm_resident_many* (msm_many.hpp), built on demand
  mutable pm::ManyTable many;
  mutable std::mutex many_mu;
};

namespace pm {

extern thread_local std::string g_last_error;

inline const CurveOps* curve_ops(int curve) {
  switch (curve) {
    case PM_CURVE_PALLAS: return &kPallasOps;
    case PM_CURVE_VESTA: return &kVestaOps;
    case PM_CURVE_BN254: return &kBn254Ops;
    default: return nullptr;
  }
}
// curve_ops with the entries' error for an unknown id set (the caller returns PM_ERR_ARG)
inline const CurveOps* checked_ops(int curve) {
  const CurveOps* ops = curve_ops(curve);
  if (!ops) set_error(PM_ERR_ARG, "unknown curve id");
  return ops;
}

// the empty sum: the point at infinity in the ABI's affine form
inline int zero_point(uint64_t out[8]) {
  std::memset(out, 0, 64);
  return PM_OK;
}

// the small-MSM path (msm_small.hpp) takes n <= small_max under the automatic
// window (an explicit pm_ctx_set_window selects the sorting pipeline)
inline bool use_small(const Ctx* ctx, size_t n) { return n <= ctx->small_max && ctx->window_c == 0; }

// pre29: d_b holds resident bases already in the R = 2^261 form (pm_bases);
// h_s != nullptr: the scalars are still on the host (d_s is their buffer)
inline int dispatch_msm_device(Ctx* ctx, int curve, const void* d_s, const void* d_b, size_t n, uint32_t flags,
                               uint64_t out[8], bool pre29 = false, const void* h_s = nullptr) {
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  flags &= ~kBasesR261;  // internal bit: never taken from the caller
  return ops->msm(ctx, d_s, d_b, n, flags | (pre29 ? kBasesR261 : 0u), out, h_s);
}

constexpr size_t kResidentRowsMinN = size_t(1) << 18;
inline int resident_rows(size_t n) {
  if (n < kResidentRowsMinN) return 1;
  // round 3, after the sort changes (profiles/r03/rows_ab/, same box, 3
  // interleaved runs): 8 rows (two bucket sets) win up to 2^20 (2^20
  // 1.193-1.221 vs 1.224-1.273 ms; 2^19 0.738 vs 0.759), 4 rows at 2^21
  // (2.33-2.35 vs 2.35-2.39) and 2^22 (4.73-4.75 vs 2 rows 4.80-4.98);
  // larger sets keep 2 rows (unmeasured: the table grows past 1 GiB)
  if (n <= (size_t(1) << 20)) return 8;
  return n <= (size_t(1) << 22) ? 4 : 2;
}
// a resident MSM takes the row-table path when it starts at the first base
// and covers at least half of the table (rows past n are zero digits)
inline bool resident_use_table(const pm_bases* b, size_t offset, size_t n) {
  return b->table && offset == 0 && n >= kResidentRowsMinN && 2 * n >= b->table->npad;
}

// capi_ctx.hip: the default context of a device (lazily created, process lifetime)
int default_ctx(int device, Ctx** out);
// capi_msm.hip; the caller holds ctx->mu.  bases_upload_locked after
// begin_call (the drop-in cache admits a set with it); msm_resident_locked
// with validated arguments (pm_multiopen_open_device commits its quotient rows
// under one lock)
int bases_upload_locked(pm_ctx* ctx, int curve, const void* bases, bool host, size_t n, pm_bases** out);
int msm_resident_locked(pm_ctx* ctx, const pm_bases* b, size_t offset, const void* scalars, bool host, size_t n,
                        uint32_t flags, uint64_t out[8]);
// capi_dropin.hip: every resident set of the drop-in cache (~pm_ctx)
void dropin_release_all(pm_ctx* ctx);

}  // namespace pm

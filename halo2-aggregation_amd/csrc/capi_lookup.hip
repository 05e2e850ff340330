// capi_lookup.hip -- lookup entries of the C-ABI: the theta-compression and
// the permuted columns A', S' (SURVEY §8f-9).
#include <algorithm>
#include <functional>
#include <vector>

#include "capi_internal.hpp"

using namespace pm;

namespace {
// Everything here runs before the device is touched.  The context is looked at
// last: the argument checks need none, and tests/test_lookup_capi.py reaches
// every one of them with a null context on a machine without a device.
int compress_check(pm_ctx* ctx, int curve, const void* const* d_cols, size_t m, size_t n, const uint64_t* theta,
                   const void* d_out, const CurveOps** ops) {
  if (!d_cols || !d_out) return set_error(PM_ERR_ARG, "null argument");
  if (!(*ops = curve_ops(curve))) return set_error(PM_ERR_ARG, "unknown curve id");
  if (n == 0) return set_error(PM_ERR_ARG, "empty columns");
  if (m == 0) return set_error(PM_ERR_ARG, "no column");
  if (m > 1 && !theta) return set_error(PM_ERR_ARG, "null argument (theta with more than one column)");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "columns longer than 2^28");
  if (m > pm::kLkMaxCols) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 columns in one call");
  for (size_t k = 0; k < m; k++)
    if (!d_cols[k]) return set_error(PM_ERR_ARG, "null column pointer");
  if (!ctx) return set_error(PM_ERR_ARG, "null argument (context)");
  return PM_OK;
}

int rows_check(size_t n, size_t usable) {
  if (n == 0) return set_error(PM_ERR_ARG, "empty columns");
  if (usable == 0 || usable > n) return set_error(PM_ERR_ARG, "usable out of range (1 <= usable <= n)");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "columns longer than 2^28");
  return PM_OK;
}

// A pointer may occur as several inputs.  An output may share its pointer with
// the same-role input of its own pair and with nothing else of the call.
struct PtrUse {
  const void* ptr;
  uint32_t pair;
  uint8_t role;  // 0 A, 1 S
  bool out;
  bool operator<(const PtrUse& o) const { return std::less<const void*>()(ptr, o.ptr); }
};
int alias_check(std::vector<PtrUse>& uses) {
  std::sort(uses.begin(), uses.end());
  for (size_t i = 0; i < uses.size();) {
    size_t j = i, outs = 0;
    for (; j < uses.size() && uses[j].ptr == uses[i].ptr; j++) outs += uses[j].out;
    if (outs) {
      const PtrUse &x = uses[i], &y = uses[i + 1 < j ? i + 1 : i];
      const bool own_input = j - i == 2 && outs == 1 && x.pair == y.pair && x.role == y.role;
      if (j - i > 1 && !own_input)
        return set_error(PM_ERR_ARG, "an output column aliases a column other than its own input");
    }
    i = j;
  }
  return PM_OK;
}

int permute_check(pm_ctx* ctx, int curve, const void* const* d_a, const void* const* d_s, size_t P, size_t n,
                  size_t usable, void* const* d_out_a, void* const* d_out_s, const uint32_t* out_status,
                  const CurveOps** ops) {
  if (!d_a || !d_s || !d_out_a || !d_out_s || !out_status) return set_error(PM_ERR_ARG, "null argument");
  if (!(*ops = curve_ops(curve))) return set_error(PM_ERR_ARG, "unknown curve id");
  if (P == 0) return set_error(PM_ERR_ARG, "no pair");
  int rc = rows_check(n, usable);
  if (rc) return rc;
  if (P > pm::kLkMaxPairs) return set_error(PM_ERR_UNSUPPORTED, "more than 32767 pairs in one call");
  std::vector<PtrUse> uses;
  uses.reserve(4 * P);
  for (size_t p = 0; p < P; p++) {
    if (!d_a[p] || !d_s[p] || !d_out_a[p] || !d_out_s[p]) return set_error(PM_ERR_ARG, "null column pointer");
    uses.push_back({d_a[p], (uint32_t)p, 0, false});
    uses.push_back({d_s[p], (uint32_t)p, 1, false});
    uses.push_back({d_out_a[p], (uint32_t)p, 0, true});
    uses.push_back({d_out_s[p], (uint32_t)p, 1, true});
  }
  if ((rc = alias_check(uses))) return rc;
  if (!ctx) return set_error(PM_ERR_ARG, "null argument (context)");
  return PM_OK;
}
}  // namespace

extern "C" {

int pm_lookup_compress_device(pm_ctx* ctx, int curve, const void* const* d_cols, size_t m, size_t n,
                              const uint64_t theta[4], void* d_out) {
  const CurveOps* ops = nullptr;
  int rc = compress_check(ctx, curve, d_cols, m, n, theta, d_out, &ops);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return ops->lookup_compress(ctx, d_cols, m, n, theta, d_out);
}

int pm_lookup_permute_device(pm_ctx* ctx, int curve, const void* const* d_a, const void* const* d_s, size_t P, size_t n,
                             size_t usable, void* const* d_out_a, void* const* d_out_s, uint32_t* out_status) {
  const CurveOps* ops = nullptr;
  int rc = permute_check(ctx, curve, d_a, d_s, P, n, usable, d_out_a, d_out_s, out_status, &ops);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return ops->lookup_permute(ctx, d_a, d_s, P, usable, d_out_a, d_out_s, out_status);
}

int pm_lookup_permute(pm_ctx* ctx, int curve, const uint64_t* a, const uint64_t* s, size_t n, size_t usable,
                      uint64_t* out_a, uint64_t* out_s, uint32_t out_status[2]) {
  if (!a || !s || !out_a || !out_s || !out_status) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  int rc = rows_check(n, usable);
  if (rc) return rc;
  std::vector<PtrUse> uses = {{a, 0, 0, false}, {s, 0, 1, false}, {out_a, 0, 0, true}, {out_s, 0, 1, true}};
  if ((rc = alias_check(uses))) return rc;
  if (!ctx) return set_error(PM_ERR_ARG, "null argument (context)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  // the usable rows of both columns side by side in the staging buffer, permuted in place
  const size_t bytes = usable * 32;
  if ((rc = ctx->in_scalars.ensure(2 * bytes))) return rc;
  char* d = (char*)ctx->in_scalars.p;
  HIP_TRY(hipMemcpyAsync(d, a, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(d + bytes, s, bytes, hipMemcpyHostToDevice, ctx->stream));
  void* pa = d;
  void* ps = d + bytes;
  if ((rc = ops->lookup_permute(ctx, &pa, &ps, 1, usable, &pa, &ps, out_status))) return rc;
  HIP_TRY(hipMemcpyAsync(out_a, pa, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(out_s, ps, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

}  // extern "C"

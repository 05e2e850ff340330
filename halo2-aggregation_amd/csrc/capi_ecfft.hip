// capi_ecfft.hip -- best_fft over curve points at the C-ABI: pm_fft_points*
// (DESIGN §10i).  The arguments are checked before the context is looked at.
#include "capi_internal.hpp"

using namespace pm;

namespace {
int fft_points_check(int curve, const void* points, uint32_t log_n, const uint64_t* omega, const CurveOps** ops) {
  if (!points || !omega) return set_error(PM_ERR_ARG, "null argument");
  if (!(*ops = checked_ops(curve))) return PM_ERR_ARG;
  if (log_n > kEcfftMaxLog) return set_error(PM_ERR_UNSUPPORTED, "point transform longer than 2^26");
  if (!(*ops)->fft_points_omega_ok(omega, log_n))
    return set_error(PM_ERR_ARG, "omega is not a primitive 2^log_n-th root of unity");
  return PM_OK;
}

int fft_points(pm_ctx* ctx, int curve, void* points, bool host, uint32_t log_n, const uint64_t* omega,
               const uint64_t* scale) {
  const CurveOps* ops = nullptr;
  int rc = fft_points_check(curve, points, log_n, omega, &ops);
  if (rc) return rc;
  if (!ctx) return set_error(PM_ERR_ARG, "null context");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  if (!host) return ops->fft_points(ctx, curve, points, log_n, omega, scale);
  const size_t bytes = ((size_t)1 << log_n) * 64;
  if ((rc = ctx->in_bases.ensure(bytes))) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->in_bases.p, points, bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ops->fft_points(ctx, curve, ctx->in_bases.p, log_n, omega, scale))) return rc;
  HIP_TRY(hipMemcpyAsync(points, ctx->in_bases.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}
}  // namespace

extern "C" {

int pm_fft_points_device(pm_ctx* ctx, int curve, void* d_points, uint32_t log_n, const uint64_t omega[4],
                         const uint64_t* scale) {
  return fft_points(ctx, curve, d_points, false, log_n, omega, scale);
}

int pm_fft_points(pm_ctx* ctx, int curve, uint64_t* points, uint32_t log_n, const uint64_t omega[4],
                  const uint64_t* scale) {
  return fft_points(ctx, curve, points, true, log_n, omega, scale);
}

int pm_fft_points_host(int curve, uint64_t* points, uint32_t log_n, const uint64_t omega[4], const uint64_t* scale,
                       int threads) {
  const CurveOps* ops = nullptr;
  const int rc = fft_points_check(curve, points, log_n, omega, &ops);
  if (rc) return rc;
  return ops->fft_points_host(points, log_n, omega, scale, threads);
}

}  // extern "C"

// ecfft_engine.hpp -- host driver of best_fft over curve points
// (pm_fft_points*).  Boundary: halo2 `best_fft(a: &mut [G], omega,
// log_n)` with G the curve, as ParamsKZG::setup runs it to turn the monomial
// SRS g into g_lagrange (omega^-1, then every point times n^-1).
#pragma once
#include <cstring>

#include "ecfft_kernels.hpp"
#include "engine.hpp"
#include "ntt_engine.hpp"

namespace pm {

// the code table of (curve, log_n, omega), cached like the NTT's twiddles
inline int ecfft_twiddles_lookup(Ctx* ctx, int curve, uint32_t logn, const uint64_t omega[4], size_t bytes,
                                 NttTwiddles** out, bool* fresh) {
  for (auto& e : ctx->ecfft_tw) {
    if (e.curve == curve && e.logn == logn && std::memcmp(e.omega, omega, 32) == 0) {
      e.stamp = ++ctx->ecfft_clock;
      *out = &e;
      *fresh = false;
      return PM_OK;
    }
  }
  NttTwiddles* slot = nullptr;
  if (ctx->ecfft_tw.size() < kEcfftTwiddleSlots) {
    ctx->ecfft_tw.emplace_back();
    slot = &ctx->ecfft_tw.back();
  } else {
    slot = &ctx->ecfft_tw[0];
    for (auto& e : ctx->ecfft_tw)
      if (e.stamp < slot->stamp) slot = &e;
  }
  slot->curve = -1;  // not valid until the caller's fill is queued
  int rc = slot->buf.ensure(bytes);
  if (rc) return rc;
  slot->curve = curve;
  slot->logn = logn;
  std::memcpy(slot->omega, omega, 32);
  slot->stamp = ++ctx->ecfft_clock;
  *out = slot;
  *fresh = true;
  return PM_OK;
}

// d_points: n = 2^logn affine points (64 B each), transformed in place.  The
// caller has checked logn and omega's order (capi_ecfft.hip).
template <class Cv>
int ecfft_device_impl(Ctx* ctx, int curve, void* d_points, uint32_t logn, const uint64_t omega[4],
                      const uint64_t* scale) {
  using Fs = typename Cv::Scalar;
  if (logn > kEcfftMaxLog) return set_error(PM_ERR_UNSUPPORTED, "point transform longer than 2^26");
  const hipStream_t st = ctx->stream;
  const uint32_t n = 1u << logn, half = n >> 1;
  uint32_t* pts = (uint32_t*)d_points;
  if (logn >= 1) {
    PM_LAUNCH(ctx, "ecfft_bitrev", (k_ecfft_bitrev<Cv><<<(n + 255) / 256, 256, 0, st>>>((uint4*)d_points, logn)));
    PM_LAUNCH(ctx, "ecfft_first", (k_ecfft_first<Cv><<<(half + 255) / 256, 256, 0, st>>>(pts, half)));
  }
  if (logn >= 2) {
    NttTwiddles* twe = nullptr;
    bool fresh = false;
    int rc = ecfft_twiddles_lookup(ctx, curve, logn, omega, (size_t)half * kEcfftTwWords * 4, &twe, &fresh);
    if (rc) return rc;
    uint4* tw = (uint4*)twe->buf.p;
    if (fresh)
      PM_LAUNCH(ctx, "ecfft_twiddles",
                (k_ecfft_twiddles<Cv><<<(half + 255) / 256, 256, 0, st>>>(fearg_from_u64<Fs>(omega), half, tw)));
    for (uint32_t s = 2; s <= logn; s++)
      PM_LAUNCH(ctx, "ecfft_stage", (k_ecfft_stage<Cv><<<(half + 255) / 256, 256, 0, st>>>(pts, tw, logn, s)));
  }
  if (scale) {
    const Fe<Fs> k = fe_from_mont<Fs>(fe_from_u64<Fs>(scale));
    FeArg ka;
    for (int i = 0; i < 8; i++) ka.l[i] = k.l[i];
    PM_LAUNCH(ctx, "ecfft_scale", (k_ecfft_scale<Cv><<<(n + 255) / 256, 256, 0, st>>>(pts, n, ka)));
  }
  HIP_TRY(hipStreamSynchronize(st));
  ctx->end_call();
  return PM_OK;
}

}  // namespace pm

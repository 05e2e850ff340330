// capi_pairing_batch.hip -- batch decider entries of the C-ABI: pm_accum_decide_batch*,
// pm_verify_proofs_batch_device.
#include <cstring>
#include <random>

#include "capi_internal.hpp"
#include "pairing_batch_engine.hpp"

using namespace pm;
using namespace pm::pairing;

namespace {
// Everything here runs before the device is touched, the context last:
// tests/test_decide_batch_capi.py reaches every argument error with a null context.
int batch_check_host(const pm_pairing* pr, size_t B, const void* quads, uint32_t flags, const void* out_ok) {
  if (!pr || !quads || !out_ok) return set_error(PM_ERR_ARG, "null argument");
  if (B > kPairMaxB) return set_error(PM_ERR_UNSUPPORTED, "more than 2^24 items in one call");
  if (flags & ~kDecideLocate) return set_error(PM_ERR_ARG, "unknown flag bit");
  return PM_OK;
}
int batch_check_ctx(pm_ctx* ctx, const pm_pairing* pr) {
  if (!ctx) return set_error(PM_ERR_ARG, "null argument (context)");
  if (pr->device < 0) return set_error(PM_ERR_ARG, "the pm_pairing was created without a context (host only)");
  if (pr->device != ctx->device) return set_error(PM_ERR_ARG, "the pm_pairing belongs to another device");
  return PM_OK;
}
int batch_check(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* quads, uint32_t flags, const void* out_ok) {
  const int rc = batch_check_host(pr, B, quads, flags, out_ok);
  return rc ? rc : batch_check_ctx(ctx, pr);
}

// the seed of a call: the caller's, or 32 bytes from the OS (the source of the
// drop-in cache key, dropin_digest.hpp); out_seed receives it
int batch_seed(const uint8_t* seed, uint64_t w[4], uint8_t* out_seed) {
  if (seed) {
    std::memcpy(w, seed, 32);
  } else {
    try {  // std::random_device may throw when no entropy source is available
      std::random_device rd;  // getrandom / /dev/urandom
      for (int i = 0; i < 4; i++) w[i] = ((uint64_t)rd() << 32) ^ (uint64_t)rd();
    } catch (const std::exception& e) {
      return set_error(PM_ERR_HIP, std::string("batch decider seed: no entropy source: ") + e.what());
    }
  }
  if (out_seed) std::memcpy(out_seed, w, 32);
  return PM_OK;
}

// the empty batch: accepted, both sums the identity
int batch_empty(const uint8_t* seed, uint32_t* out_ok, uint64_t* out_pair, uint8_t* out_seed) {
  uint64_t w[4];
  int rc = batch_seed(seed, w, out_seed);
  if (rc) return rc;
  if (out_ok) *out_ok = 1u;
  if (out_pair) std::memset(out_pair, 0, 128);
  return PM_OK;
}
}  // namespace

extern "C" {

int pm_accum_decide_batch_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads,
                                 const void* d_status_in, const uint8_t* seed, uint32_t flags, uint32_t* out_ok,
                                 void* d_out_item_ok, void* d_out_status, uint64_t* out_pair, uint8_t* out_seed) {
  if (B == 0) return batch_empty(seed, out_ok, out_pair, out_seed);
  int rc = batch_check(ctx, pr, B, d_quads, flags, out_ok);
  if (rc) return rc;
  uint64_t sw[4];
  if ((rc = batch_seed(seed, sw, out_seed))) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return decide_batch_device(ctx, pr, B, d_quads, d_status_in, sw, flags, out_ok, d_out_item_ok, d_out_status,
                             out_pair);
}

int pm_accum_decide_batch(pm_ctx* ctx, const pm_pairing* pr, size_t B, const uint64_t* quads,
                          const uint32_t* status_in, const uint8_t* seed, uint32_t flags, uint32_t* out_ok,
                          uint32_t* out_item_ok, uint32_t* out_status, uint64_t* out_pair, uint8_t* out_seed) {
  if (B == 0) return batch_empty(seed, out_ok, out_pair, out_seed);
  int rc = batch_check(ctx, pr, B, quads, flags, out_ok);
  if (rc) return rc;
  uint64_t sw[4];
  if ((rc = batch_seed(seed, sw, out_seed))) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  // staged in one buffer: [quads | status in | item ok | status out]
  const bool locate = (flags & kDecideLocate) && out_item_ok;
  const size_t bq = B * 256, bw = B * 4;
  if ((rc = ctx->in_bases.ensure(bq + 3 * bw))) return rc;
  char* d = (char*)ctx->in_bases.p;
  char *d_si = d + bq, *d_io = d_si + bw, *d_so = d_io + bw;
  HIP_TRY(hipMemcpyAsync(d, quads, bq, hipMemcpyHostToDevice, ctx->stream));
  if (status_in) HIP_TRY(hipMemcpyAsync(d_si, status_in, bw, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = decide_batch_device(ctx, pr, B, d, status_in ? d_si : nullptr, sw, flags, out_ok,
                                locate ? d_io : nullptr, out_status ? d_so : nullptr, out_pair)))
    return rc;
  if (locate) HIP_TRY(hipMemcpyAsync(out_item_ok, d_io, bw, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) HIP_TRY(hipMemcpyAsync(out_status, d_so, bw, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

int pm_accum_decide_batch_host(const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                               const uint8_t* seed, uint32_t flags, uint32_t* out_ok, uint32_t* out_item_ok,
                               uint32_t* out_status, uint64_t* out_pair, uint8_t* out_seed) {
  if (B == 0) return batch_empty(seed, out_ok, out_pair, out_seed);
  int rc = batch_check_host(pr, B, quads, flags, out_ok);
  if (rc) return rc;
  uint64_t sw[4];
  if ((rc = batch_seed(seed, sw, out_seed))) return rc;
  J1 Lj, Rj;
  const bool clean = batch_fold(B, quads, status_in, sw, out_status, &Lj, &Rj);
  const G1 L = j1_affine(Lj), R = j1_affine(Rj);
  if (out_pair) {
    g1_to_words(L, out_pair);
    g1_to_words(R, out_pair + 8);
  }
  *out_ok = batch_decide(pr->host, clean, L, R);
  if ((flags & kDecideLocate) && out_item_ok) {
    if (*out_ok) {
      for (size_t i = 0; i < B; i++) out_item_ok[i] = 1u;
    } else if ((rc = pm_accum_decide_host(pr, B, quads, status_in, out_item_ok, nullptr, nullptr))) {
      return rc;
    }
  }
  return PM_OK;
}

int pm_verify_proofs_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                  const uint64_t vk_repr[4], const void* d_proofs, size_t stride,
                                  const void* d_instance_points, void* d_challenges, void* d_out_quads,
                                  void* d_out_h_eval, void* d_out_status, const pm_pairing* pr, const uint8_t* seed,
                                  uint32_t flags, uint32_t* out_ok, void* d_out_item_ok, uint64_t* out_pair,
                                  uint8_t* out_seed) {
  if (curve != PM_CURVE_BN254) return set_error(PM_ERR_ARG, "the batch decider is BN254 only");
  if (B == 0) return batch_empty(seed, out_ok, out_pair, out_seed);
  int rc = batch_check_host(pr, B, d_out_quads, flags, out_ok);
  if (rc) return rc;
  if (!d_out_status) return set_error(PM_ERR_ARG, "null argument (d_out_status carries the status to the decider)");
  if ((rc = batch_check_ctx(ctx, pr))) return rc;
  // the accumulator from the proof bytes; quads and status stay where they lie
  if ((rc = pm_accum_batch_proofs_device(ctx, curve, shape, B, vk_repr, d_proofs, stride, d_instance_points,
                                         d_challenges, d_out_quads, d_out_h_eval, d_out_status)))
    return rc;
  return pm_accum_decide_batch_device(ctx, pr, B, d_out_quads, d_out_status, seed, flags, out_ok, d_out_item_ok,
                                      d_out_status, out_pair, out_seed);
}

}  // extern "C"

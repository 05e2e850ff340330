// capi_proofs.hip -- proof entries of the C-ABI: shape layout, multiopen
// accumulator, Blake2b transcript replay, proof bytes, and the batch sharded
// over several contexts.
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "accum_plan.hpp"
#include "blake2b.hpp"
#include "capi_internal.hpp"

using namespace pm;

namespace {
// Staging layout of the host-buffer entries in one context buffer:
// [proofs | instance points |] points | scalars | challenges | quads | h_eval | status
// (the first two only on the proof-byte path: psize bytes per proof, ni instance points).
struct Staging {
  size_t bpf, bin, bp, bs, bc, bo, bh, bst;           // bytes of each part
  char *dpf, *din, *dp, *ds, *dc, *dq, *dh, *dst;  // set by place()
  Staging(size_t B, uint32_t npts, uint32_t nsc, size_t psize = 0, size_t ni = 0)
      : bpf((B * psize + 255) & ~size_t(255)), bin((B * ni * 64 + 255) & ~size_t(255)), bp(B * npts * 64),
        bs(B * nsc * 32), bc(B * 7 * 32), bo(B * 4 * 64), bh(B * 32), bst(B * 4) {}
  int place(Buf& buf) {
    if (const int rc = buf.ensure(bpf + bin + bp + bs + bc + bo + bh + bst)) return rc;
    dpf = (char*)buf.p, din = dpf + bpf, dp = din + bin, ds = dp + bp;
    dc = ds + bs, dq = dc + bc, dh = dq + bo, dst = dh + bh;
    return PM_OK;
  }
};
}  // namespace

extern "C" {

// ------------------------------------------------- multiopen accumulator
int pm_shape_layout(const pm_proof_shape* shape, uint32_t* points_per_proof, uint32_t* scalars_per_proof,
                    uint32_t* num_sets) {
  std::vector<AccQuery> q;
  AccLayout L;
  const std::string err = acc_validate(shape, q, L, nullptr);
  if (!err.empty()) return set_error(PM_ERR_ARG, "accum shape: " + err);
  if (points_per_proof) *points_per_proof = L.npts;
  if (scalars_per_proof) *scalars_per_proof = L.nsc;
  if (num_sets) *num_sets = L.nsets;
  return PM_OK;
}

int pm_accum_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const void* d_points,
                          const void* d_scalars, const void* d_challenges, void* d_out_quads, void* d_out_h_eval,
                          void* d_out_status) {
  if (!ctx || !shape || (B && (!d_points || !d_scalars || !d_challenges || !d_out_quads)))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return ops->accum(ctx, shape, B, d_points, d_scalars, const_cast<void*>(d_challenges), d_out_quads, d_out_h_eval, nullptr,
                    d_out_status);
}

int pm_accum_batch(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t* points,
                   const uint64_t* scalars, const uint64_t* challenges, uint64_t* out_quads, uint64_t* out_h_eval,
                   uint32_t* out_status) {
  if (!ctx || !shape || (B && (!points || !scalars || !challenges || !out_quads)))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (B == 0) return PM_OK;
  if ((rc = ctx->begin_call())) return rc;
  Staging g(B, npts, nsc);
  if ((rc = g.place(ctx->acc_io))) return rc;
  HIP_TRY(hipMemcpyAsync(g.dp, points, g.bp, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.ds, scalars, g.bs, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.dc, challenges, g.bc, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ops->accum(ctx, shape, B, g.dp, g.ds, g.dc, g.dq, g.dh, nullptr, out_status ? g.dst : nullptr))) return rc;
  HIP_TRY(hipMemcpyAsync(out_quads, g.dq, g.bo, hipMemcpyDeviceToHost, ctx->stream));
  if (out_h_eval) HIP_TRY(hipMemcpyAsync(out_h_eval, g.dh, g.bh, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) HIP_TRY(hipMemcpyAsync(out_status, g.dst, g.bst, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

// ------------------------------------------------- Blake2b transcript replay
int pm_vk_transcript_repr(int curve, const uint8_t* pinned, size_t len, uint64_t out[4]) {
  if (!out || (len && !pinned)) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  Blake2bHost hs(kVerifyKeyPersonal);
  uint8_t le[8];
  for (int i = 0; i < 8; i++) le[i] = (uint8_t)((uint64_t)len >> (8 * i));
  hs.update(le, 8);
  hs.update(pinned, len);
  uint8_t d[64];
  hs.finalize(d);
  return ops->vk_repr(d, out);
}

int pm_transcript_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                               const uint64_t vk_repr[4], const void* d_points, const void* d_scalars,
                               void* d_out_challenges, void* d_out_status) {
  if (!ctx || !shape || !vk_repr || (B && (!d_points || !d_scalars || !d_out_challenges)))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if ((rc = ops->transcript(ctx, shape, B, vk_repr, d_points, d_scalars, d_out_challenges, d_out_status))) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->end_call();
  return PM_OK;
}

int pm_accum_batch_transcript_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                     const uint64_t vk_repr[4], const void* d_points, const void* d_scalars,
                                     void* d_challenges, void* d_out_quads, void* d_out_h_eval,
                                     void* d_out_status) {
  if (!ctx || !shape || !vk_repr || (B && (!d_points || !d_scalars || !d_challenges || !d_out_quads)))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return ops->accum(ctx, shape, B, d_points, d_scalars, d_challenges, d_out_quads, d_out_h_eval, vk_repr, d_out_status);
}

// Host-buffer variants: the Staging layout in acc_io.
static int transcript_host(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4],
                           const uint64_t* points, const uint64_t* scalars, uint64_t* out_challenges,
                           uint64_t* out_quads, uint64_t* out_h_eval, uint32_t* out_status, bool accum) {
  if (!ctx || !shape || !vk_repr || (B && (!points || !scalars || (accum ? !out_quads : !out_challenges))))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (B == 0) return PM_OK;
  if (B > (1u << 20)) return set_error(PM_ERR_UNSUPPORTED, "transcript batch larger than 2^20 proofs");
  if ((rc = ctx->begin_call())) return rc;
  Staging g(B, npts, nsc);
  if ((rc = g.place(ctx->acc_io))) return rc;
  HIP_TRY(hipMemcpyAsync(g.dp, points, g.bp, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(g.ds, scalars, g.bs, hipMemcpyHostToDevice, ctx->stream));
  if (accum) {
    if ((rc = ops->accum(ctx, shape, B, g.dp, g.ds, g.dc, g.dq, g.dh, vk_repr, g.dst))) return rc;
  } else if ((rc = ops->transcript(ctx, shape, B, vk_repr, g.dp, g.ds, g.dc, g.dst))) {
    return rc;
  }
  if (out_challenges) HIP_TRY(hipMemcpyAsync(out_challenges, g.dc, g.bc, hipMemcpyDeviceToHost, ctx->stream));
  if (accum) HIP_TRY(hipMemcpyAsync(out_quads, g.dq, g.bo, hipMemcpyDeviceToHost, ctx->stream));
  if (accum && out_h_eval) HIP_TRY(hipMemcpyAsync(out_h_eval, g.dh, g.bh, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) HIP_TRY(hipMemcpyAsync(out_status, g.dst, g.bst, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (!accum) ctx->end_call();
  return PM_OK;
}

int pm_transcript_batch(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4],
                        const uint64_t* points, const uint64_t* scalars, uint64_t* out_challenges,
                        uint32_t* out_status) {
  return transcript_host(ctx, curve, shape, B, vk_repr, points, scalars, out_challenges, nullptr, nullptr,
                         out_status, false);
}

int pm_accum_batch_transcript(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                              const uint64_t vk_repr[4], const uint64_t* points, const uint64_t* scalars,
                              uint64_t* out_challenges, uint64_t* out_quads, uint64_t* out_h_eval,
                              uint32_t* out_status) {
  return transcript_host(ctx, curve, shape, B, vk_repr, points, scalars, out_challenges, out_quads, out_h_eval,
                         out_status, true);
}

// ------------------------------------------------- proof bytes (read_point / read_scalar)
int pm_proof_size(const pm_proof_shape* shape, size_t* bytes) {
  if (!shape || !bytes) return set_error(PM_ERR_ARG, "null argument");
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  *bytes = 32ull * (npts - shape->num_instance_columns + nsc);
  return PM_OK;
}

int pm_decode_proofs_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const void* d_proofs,
                            size_t stride, const void* d_instance_points, void* d_out_points, void* d_out_scalars,
                            void* d_out_status) {
  if (!ctx || !shape || (B && (!d_proofs || !d_out_points || !d_out_scalars || !d_out_status)) ||
      (B && shape->num_instance_columns && !d_instance_points))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return ops->proofs(ctx, shape, B, d_proofs, stride, d_instance_points, d_out_points, d_out_scalars, d_out_status,
                     nullptr, nullptr, nullptr, nullptr);
}

int pm_accum_batch_proofs_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                 const uint64_t vk_repr[4], const void* d_proofs, size_t stride,
                                 const void* d_instance_points, void* d_challenges, void* d_out_quads,
                                 void* d_out_h_eval, void* d_out_status) {
  if (!ctx || !shape || !vk_repr || (B && (!d_proofs || !d_challenges || !d_out_quads)) ||
      (B && shape->num_instance_columns && !d_instance_points))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (B == 0) return PM_OK;
  if ((rc = ctx->begin_call())) return rc;
  // decoded points / scalars (and the status words when the caller passes none) in context scratch
  const size_t bp = B * npts * 64, bs = B * nsc * 32, bst = B * 4;
  if ((rc = ctx->pf_io.ensure(bp + bs + bst))) return rc;
  char* dp = (char*)ctx->pf_io.p;
  return ops->proofs(ctx, shape, B, d_proofs, stride, d_instance_points, dp, dp + bp,
                     d_out_status ? d_out_status : dp + bp + bs, vk_repr, d_challenges, d_out_quads, d_out_h_eval);
}

// Host-buffer variants: the Staging layout (with the proofs and instance points, decoded into its points / scalars) in pf_io.
static int proofs_host(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t* vk_repr,
                       const uint8_t* proofs, size_t stride, const uint64_t* inst, uint64_t* out_points,
                       uint64_t* out_scalars, uint64_t* out_challenges, uint64_t* out_quads, uint64_t* out_h_eval,
                       uint32_t* out_status) {
  const bool accum = vk_repr != nullptr;
  if (!ctx || !shape || (B && !proofs) || (B && shape->num_instance_columns && !inst) ||
      (B && (accum ? !out_quads : (!out_points || !out_scalars))))
    return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  size_t psize = 0;
  if ((rc = pm_proof_size(shape, &psize))) return rc;
  if (stride < psize) return set_error(PM_ERR_ARG, "proof stride below the proof size");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (B == 0) return PM_OK;
  if (B > (1u << 20)) return set_error(PM_ERR_UNSUPPORTED, "proof batch larger than 2^20 proofs");
  if ((rc = ctx->begin_call())) return rc;
  const size_t ni = shape->num_instance_columns;
  Staging g(B, npts, nsc, psize, ni);
  if ((rc = g.place(ctx->pf_io))) return rc;
  // the proofs packed densely (stride = psize) for the device
  if (stride == psize) {
    HIP_TRY(hipMemcpyAsync(g.dpf, proofs, B * psize, hipMemcpyHostToDevice, ctx->stream));
  } else {
    HIP_TRY(hipMemcpy2DAsync(g.dpf, psize, proofs, stride, psize, B, hipMemcpyHostToDevice, ctx->stream));
  }
  if (ni) HIP_TRY(hipMemcpyAsync(g.din, inst, B * ni * 64, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = ops->proofs(ctx, shape, B, g.dpf, psize, g.din, g.dp, g.ds, g.dst, vk_repr, g.dc, g.dq, g.dh))) return rc;
  if (out_points) HIP_TRY(hipMemcpyAsync(out_points, g.dp, g.bp, hipMemcpyDeviceToHost, ctx->stream));
  if (out_scalars) HIP_TRY(hipMemcpyAsync(out_scalars, g.ds, g.bs, hipMemcpyDeviceToHost, ctx->stream));
  if (accum && out_challenges) HIP_TRY(hipMemcpyAsync(out_challenges, g.dc, g.bc, hipMemcpyDeviceToHost, ctx->stream));
  if (accum) HIP_TRY(hipMemcpyAsync(out_quads, g.dq, g.bo, hipMemcpyDeviceToHost, ctx->stream));
  if (accum && out_h_eval) HIP_TRY(hipMemcpyAsync(out_h_eval, g.dh, g.bh, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) HIP_TRY(hipMemcpyAsync(out_status, g.dst, g.bst, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

int pm_decode_proofs(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint8_t* proofs,
                     size_t stride, const uint64_t* instance_points, uint64_t* out_points, uint64_t* out_scalars,
                     uint32_t* out_status) {
  return proofs_host(ctx, curve, shape, B, nullptr, proofs, stride, instance_points, out_points, out_scalars, nullptr,
                     nullptr, nullptr, out_status);
}

int pm_accum_batch_proofs(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4],
                          const uint8_t* proofs, size_t stride, const uint64_t* instance_points,
                          uint64_t* out_challenges, uint64_t* out_quads, uint64_t* out_h_eval, uint32_t* out_status) {
  if (!vk_repr) return set_error(PM_ERR_ARG, "null argument");
  return proofs_host(ctx, curve, shape, B, vk_repr, proofs, stride, instance_points, nullptr, nullptr,
                     out_challenges, out_quads, out_h_eval, out_status);
}

// Proof batch sharded over several contexts (devices) in one process: proofs
// are independent, so context k takes the contiguous range
// [k*per, (k+1)*per) and runs the single-context host entry on it in its own
// thread; the outputs land in place.  challenges == NULL replays the
// transcript (vk_repr required), else vk_repr is ignored.
int pm_accum_batch_multi(pm_ctx* const* ctxs, int nctx, int curve, const pm_proof_shape* shape, size_t B,
                         const uint64_t* points, const uint64_t* scalars, const uint64_t* challenges,
                         const uint64_t vk_repr[4], uint64_t* out_challenges, uint64_t* out_quads,
                         uint64_t* out_h_eval, uint32_t* out_status) {
  if (!ctxs || nctx < 1 || !shape || (B && (!points || !scalars || !out_quads)) || (!challenges && !vk_repr))
    return set_error(PM_ERR_ARG, "null argument");
  for (int k = 0; k < nctx; k++)
    if (!ctxs[k]) return set_error(PM_ERR_ARG, "null context");
  if (!checked_ops(curve)) return PM_ERR_ARG;
  uint32_t npts = 0, nsc = 0, ns = 0;
  int rc = pm_shape_layout(shape, &npts, &nsc, &ns);
  if (rc) return rc;
  if (B == 0) return PM_OK;
  const size_t per = (B + nctx - 1) / nctx;
  std::vector<int> rcs(nctx, PM_OK);
  std::vector<std::string> errs(nctx);
  std::vector<std::thread> th;
  for (int k = 0; k < nctx; k++) {
    const size_t lo = std::min(B, per * k), cnt = std::min(B, lo + per) - lo;
    if (cnt == 0) continue;
    th.emplace_back([&, k, lo, cnt] {
      const uint64_t* p = points + lo * npts * 8;
      const uint64_t* sc = scalars + lo * nsc * 4;
      uint64_t* q = out_quads + lo * 32;
      uint64_t* h = out_h_eval ? out_h_eval + lo * 4 : nullptr;
      uint32_t* st = out_status ? out_status + lo : nullptr;
      int r;
      if (challenges)
        r = pm_accum_batch(ctxs[k], curve, shape, cnt, p, sc, challenges + lo * 28, q, h, st);
      else
        r = pm_accum_batch_transcript(ctxs[k], curve, shape, cnt, vk_repr, p, sc,
                                      out_challenges ? out_challenges + lo * 28 : nullptr, q, h, st);
      rcs[k] = r;
      if (r) errs[k] = pm::g_last_error;
    });
  }
  for (auto& t : th) t.join();
  for (int k = 0; k < nctx; k++)
    if (rcs[k]) return set_error(rcs[k], "context " + std::to_string(k) + ": " + errs[k]);
  if (challenges && out_challenges) std::memcpy(out_challenges, challenges, B * 7 * 32);
  return PM_OK;
}


}  // extern "C"

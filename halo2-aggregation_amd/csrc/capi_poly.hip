// capi_poly.hip -- polynomial entries of the C-ABI: NTT, openings, grand
// products and the batch inversion, extended-domain conversions, quotient
// numerator.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "accum_plan.hpp"
#include "capi_internal.hpp"

using namespace pm;

namespace {
// The host-array wrappers, with ctx->mu held after begin_call: the first
// in_bytes of in_scalars (grown to cap bytes) are the caller's array, run(d)
// works on that buffer, and out_bytes come back from `from` (null: the same
// buffer) before the stream is synchronised; out_bytes == 0: neither.
template <class Run>
int staged_call(pm_ctx* ctx, const void* in, size_t in_bytes, size_t cap, Run run, void* out, size_t out_bytes,
                const void* from = nullptr) {
  int rc = ctx->in_scalars.ensure(cap);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ctx->in_scalars.p, in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = run(ctx->in_scalars.p)) || !out_bytes) return rc;
  HIP_TRY(hipMemcpyAsync(out, from ? from : ctx->in_scalars.p, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}
}  // namespace

extern "C" {

// ------------------------------------------------- NTT (§8f-4)
static int fft(pm_ctx* ctx, int curve, void* data, bool host, uint32_t log_n, const uint64_t omega[4],
               const uint64_t* scale) {
  if (!ctx || !data || !omega) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (log_n > pm::kNttMaxLog) return set_error(PM_ERR_UNSUPPORTED, "NTT longer than 2^28");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  auto run = [&](void* d) { return ops->ntt(ctx, curve, d, log_n, omega, scale); };
  const size_t bytes = ((size_t)1 << log_n) * 32;
  return host ? staged_call(ctx, data, bytes, bytes, run, data, bytes) : run(data);
}

int pm_fft_device(pm_ctx* ctx, int curve, void* d_data, uint32_t log_n, const uint64_t omega[4],
                  const uint64_t* scale) {
  return fft(ctx, curve, d_data, false, log_n, omega, scale);
}

int pm_fft(pm_ctx* ctx, int curve, uint64_t* data, uint32_t log_n, const uint64_t omega[4], const uint64_t* scale) {
  return fft(ctx, curve, data, true, log_n, omega, scale);
}

// ------------------------------------------------- polynomial openings (§8f-5)
// As everywhere in this file, an error after begin_call() returns at once (a
// failed ensure / HIP call, or an MSM failing between the witness and the
// commits of pm_multiopen_open_device): the context's per-call state is reset
// by the next begin_call(), and the outputs of the failed call are unspecified.
namespace {
// shared checks of the evaluation / witness entries; everything here runs before the device is touched
int poly_check_common(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n, const CurveOps** ops) {
  if (!ctx || !d_polys) return set_error(PM_ERR_ARG, "null argument");
  if (!(*ops = curve_ops(curve))) return set_error(PM_ERR_ARG, "unknown curve id");
  if (n == 0) return set_error(PM_ERR_ARG, "empty polynomial");
  for (size_t i = 0; i < P; i++)
    if (!d_polys[i]) return set_error(PM_ERR_ARG, "null polynomial pointer");
  return PM_OK;
}

int witness_check(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n, const uint32_t* set_offsets,
                  const uint32_t* set_polys, const uint64_t* points, const uint64_t* v, size_t S, size_t max_n,
                  const CurveOps** ops) {
  int rc = poly_check_common(ctx, curve, d_polys, P, n, ops);
  if (rc) return rc;
  if (S == 0) return PM_OK;
  if (!set_offsets || !set_polys || !points || !v) return set_error(PM_ERR_ARG, "null argument");
  if (set_offsets[0] != 0) return set_error(PM_ERR_ARG, "set_offsets[0] must be 0");
  for (size_t j = 0; j < S; j++) {
    if (set_offsets[j + 1] <= set_offsets[j]) return set_error(PM_ERR_ARG, "a rotation set has no polynomial");
    for (uint32_t i = set_offsets[j]; i < set_offsets[j + 1]; i++)
      if (set_polys[i] >= P) return set_error(PM_ERR_ARG, "polynomial index out of range");
  }
  if (n > max_n)
    return set_error(PM_ERR_UNSUPPORTED, max_n == pm::kMaxPoints ? "opening longer than 2^26 (the MSM's limit)"
                                                                   : "polynomial longer than 2^28");
  if (S > pm::kPolyMaxGridY) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 rotation sets in one call");
  return PM_OK;
}
}  // namespace

int pm_poly_eval_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                        const uint32_t* poly_index, const uint64_t* points, size_t E, uint64_t* out_evals) {
  const CurveOps* ops = nullptr;
  int rc = poly_check_common(ctx, curve, d_polys, P, n, &ops);
  if (rc) return rc;
  if (E == 0) return PM_OK;
  if (!poly_index || !points || !out_evals) return set_error(PM_ERR_ARG, "null argument");
  for (size_t e = 0; e < E; e++)
    if (poly_index[e] >= P) return set_error(PM_ERR_ARG, "polynomial index out of range");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "polynomial longer than 2^28");
  if (E > pm::kPolyMaxGridY) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 evaluations in one call");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return ops->poly_eval(ctx, d_polys, P, n, poly_index, points, E, out_evals);
}

int pm_multiopen_witness_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                                const uint32_t* set_offsets, const uint32_t* set_polys, const uint64_t* points,
                                const uint64_t v[4], size_t S, void* d_out_quotients, uint64_t* out_evals) {
  const CurveOps* ops = nullptr;
  int rc = witness_check(ctx, curve, d_polys, P, n, set_offsets, set_polys, points, v, S, pm::kPolyMaxN, &ops);
  if (rc) return rc;
  if (S == 0) return PM_OK;
  if (!d_out_quotients) return set_error(PM_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return ops->poly_witness(ctx, d_polys, P, n, set_offsets, set_polys, points, v, S, d_out_quotients, out_evals);
}

int pm_multiopen_open_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                             const uint32_t* set_offsets, const uint32_t* set_polys, const uint64_t* points,
                             const uint64_t v[4], size_t S, const pm_bases* srs, uint64_t* out_w,
                             uint64_t* out_evals) {
  const CurveOps* ops = nullptr;
  int rc = witness_check(ctx, curve, d_polys, P, n, set_offsets, set_polys, points, v, S, pm::kMaxPoints, &ops);
  if (rc) return rc;
  if (!srs) return set_error(PM_ERR_ARG, "null argument");
  if (S == 0) return PM_OK;
  if (!out_w) return set_error(PM_ERR_ARG, "null argument");
  if (srs->curve != curve) return set_error(PM_ERR_ARG, "the SRS belongs to another curve");
  if (srs->device != ctx->device) return set_error(PM_ERR_ARG, "bases live on another device");
  if (n > srs->n) return set_error(PM_ERR_ARG, "the SRS is shorter than the polynomials");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  if ((rc = ctx->poly_q.ensure(S * n * 32))) return rc;
  if ((rc = ops->poly_witness(ctx, d_polys, P, n, set_offsets, set_polys, points, v, S, ctx->poly_q.p, out_evals)))
    return rc;
  for (size_t j = 0; j < S; j++)
    if ((rc = msm_resident_locked(ctx, srs, 0, (const char*)ctx->poly_q.p + j * n * 32, false, n, 0, out_w + 8 * j)))
      return rc;
  return PM_OK;
}

int pm_eval_polynomial(pm_ctx* ctx, int curve, const uint64_t* coeffs, size_t n, const uint64_t point[4],
                       uint64_t out[4]) {
  if (!ctx || !coeffs || !point || !out) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (n == 0) return set_error(PM_ERR_ARG, "empty polynomial");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "polynomial longer than 2^28");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  auto run = [&](const void* poly) {  // writes `out` itself
    const uint32_t index = 0;
    return ops->poly_eval(ctx, &poly, 1, n, &index, point, 1, out);
  };
  return staged_call(ctx, coeffs, n * 32, n * 32, run, nullptr, 0);
}

int pm_kate_division(pm_ctx* ctx, int curve, const uint64_t* coeffs, size_t n, const uint64_t z[4], uint64_t* out_q) {
  if (!ctx || !coeffs || !z || (n > 1 && !out_q)) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (n == 0) return set_error(PM_ERR_ARG, "empty polynomial");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "polynomial longer than 2^28");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if ((rc = ctx->poly_q.ensure(n * 32))) return rc;
  auto run = [&](const void* poly) {
    const uint32_t offsets[2] = {0, 1}, index = 0;
    // one set of one polynomial: v does not enter (any value serves)
    return ops->poly_witness(ctx, &poly, 1, n, offsets, &index, z, z, 1, ctx->poly_q.p, nullptr);
  };
  return staged_call(ctx, coeffs, n * 32, n * 32, run, out_q, (n - 1) * 32, ctx->poly_q.p);
}

// ------------------------------------------------- grand products (§8f-6)
namespace {
// everything here runs before the device is touched
int gp_check(pm_ctx* ctx, int curve, const void* const* d_cols, size_t C, size_t n, const pm_gp_factor* num,
             const uint32_t* num_offsets, const pm_gp_factor* den, const uint32_t* den_offsets, size_t S,
             const uint64_t* omega, const uint64_t* start, size_t active, uint32_t flags, const void* d_out_z,
             const CurveOps** ops) {
  if (!ctx || !num_offsets || !den_offsets || !start || !d_out_z || (C && !d_cols))
    return set_error(PM_ERR_ARG, "null argument");
  if (!(*ops = curve_ops(curve))) return set_error(PM_ERR_ARG, "unknown curve id");
  if (n == 0) return set_error(PM_ERR_ARG, "empty columns");
  if (active == 0 || active > n) return set_error(PM_ERR_ARG, "active out of range (1 <= active <= n)");
  if (S == 0) return set_error(PM_ERR_ARG, "no set");
  if (flags & ~(uint32_t)PM_GP_CHAIN) return set_error(PM_ERR_ARG, "unknown flag bits");
  for (size_t i = 0; i < C; i++)
    if (!d_cols[i]) return set_error(PM_ERR_ARG, "null column pointer");
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "columns longer than 2^28");
  if (S > pm::kPolyMaxGridY) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 sets in one call");
  const pm_gp_factor* lists[2] = {num, den};
  const uint32_t* offs[2] = {num_offsets, den_offsets};
  for (int l = 0; l < 2; l++) {
    if (offs[l][0] != 0) return set_error(PM_ERR_ARG, "offsets[0] must be 0");
    for (size_t j = 0; j < S; j++) {
      if (offs[l][j + 1] < offs[l][j]) return set_error(PM_ERR_ARG, "offsets must not decrease");
      if (offs[l][j + 1] - offs[l][j] > PM_GP_MAX_FACTORS)
        return set_error(PM_ERR_ARG, "more than PM_GP_MAX_FACTORS factors in a list");
    }
    if (offs[l][S] && !lists[l]) return set_error(PM_ERR_ARG, "null argument");
    for (uint32_t i = 0; i < offs[l][S]; i++) {
      const pm_gp_factor& f = lists[l][i];
      if (f.x != PM_GP_NONE && f.x >= C) return set_error(PM_ERR_ARG, "column index out of range");
      if (f.y == PM_GP_OMEGA) {
        if (!omega) return set_error(PM_ERR_ARG, "a factor names PM_GP_OMEGA and omega is null");
      } else if (f.y != PM_GP_NONE && f.y >= C) {
        return set_error(PM_ERR_ARG, "column index out of range");
      }
    }
  }
  return PM_OK;
}
}  // namespace

int pm_grand_product_device(pm_ctx* ctx, int curve, const void* const* d_cols, size_t C, size_t n,
                            const pm_gp_factor* num, const uint32_t* num_offsets, const pm_gp_factor* den,
                            const uint32_t* den_offsets, size_t S, const uint64_t omega[4], const uint64_t start[4],
                            size_t active, uint32_t flags, void* d_out_z, uint64_t* out_last) {
  const CurveOps* ops = nullptr;
  int rc = gp_check(ctx, curve, d_cols, C, n, num, num_offsets, den, den_offsets, S, omega, start, active, flags,
                    d_out_z, &ops);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return ops->grand_product(ctx, curve, d_cols, C, n, num, num_offsets, den, den_offsets, S, omega, start, active, flags,
                            d_out_z, out_last);
}

static int batch_invert(pm_ctx* ctx, int curve, void* data, bool host, size_t n) {
  if (!ctx || (n && !data)) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (n == 0) return PM_OK;
  if (n > pm::kPolyMaxN) return set_error(PM_ERR_UNSUPPORTED, "more than 2^28 values");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  auto run = [&](void* d) {
    return ops->grand_product(ctx, curve, nullptr, 0, n, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, n,
                              pm::kGpInvert, d, nullptr);
  };
  return host ? staged_call(ctx, data, n * 32, n * 32, run, data, n * 32) : run(data);
}

int pm_batch_invert_device(pm_ctx* ctx, int curve, void* d_data, size_t n) {
  return batch_invert(ctx, curve, d_data, false, n);
}

int pm_batch_invert(pm_ctx* ctx, int curve, uint64_t* data, size_t n) { return batch_invert(ctx, curve, data, true, n); }

// ------------------------------------------------- extended-domain conversions (§8f-7)
int pm_domain_create(pm_ctx* ctx, int curve, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                     const uint64_t zeta[4], pm_domain** out) {
  if (!ctx || !extended_omega || !zeta || !out) return set_error(PM_ERR_ARG, "null argument");
  *out = nullptr;
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (extended_k < k) return set_error(PM_ERR_ARG, "extended_k below k");
  if (extended_k > pm::kNttMaxLog) return set_error(PM_ERR_UNSUPPORTED, "extended domain longer than 2^28");
  if (extended_k - k > pm::kDomMaxE) return set_error(PM_ERR_UNSUPPORTED, "extended_k - k above 8");
  std::unique_ptr<pm_domain> d(new pm_domain{curve, ctx->device, k, extended_k, {}, {}, {}});
  std::vector<uint64_t> tab;
  int rc = ops->domain_tables(k, extended_k, extended_omega, zeta, d.get(), &tab);  // host only
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  if ((rc = d->d_tab.ensure(tab.size() * 8))) return rc;
  if (hipMemcpy(d->d_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return set_error(PM_ERR_HIP, "upload of the domain tables failed");
  *out = d.release();
  return PM_OK;
}

int pm_domain_info(const pm_domain* d, uint32_t* k, uint32_t* extended_k, uint64_t omega[4], uint32_t* t_len) {
  if (!d) return set_error(PM_ERR_ARG, "null argument");
  if (k) *k = d->k;
  if (extended_k) *extended_k = d->ext_k;
  if (omega) std::memcpy(omega, d->omega, 32);
  if (t_len) *t_len = 1u << (d->ext_k - d->k);
  return PM_OK;
}

int pm_domain_release(pm_domain* d) {
  if (!d) return PM_OK;
  (void)hipSetDevice(d->device);
  delete d;
  return PM_OK;
}

namespace {
// shared checks of the column entries; everything here runs before the device is touched
int domain_check(pm_ctx* ctx, const pm_domain* d, const void* const* d_in, bool has_in, void* const* d_out, size_t C) {
  if (!ctx || !d || (C && (!d_out || (has_in && !d_in)))) return set_error(PM_ERR_ARG, "null argument");
  if (d->device != ctx->device) return set_error(PM_ERR_ARG, "the domain lives on another device");
  for (size_t c = 0; c < C; c++)
    if (!d_out[c] || (has_in && !d_in[c])) return set_error(PM_ERR_ARG, "null column pointer");
  if (C > pm::kPolyMaxGridY) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 columns in one call");
  return PM_OK;
}

// with the context's mutex held
int domain_run_locked(pm_ctx* ctx, const pm_domain* d, int op, const void* const* d_in, void* const* d_out, size_t C,
                      size_t keep, uint32_t flags) {
  int rc = ctx->begin_call();
  if (rc) return rc;
  pm::DomJob job{};
  job.op = op;
  job.curve = d->curve;
  job.logn = d->ext_k;
  job.omega = op == pm::kDomOpToCoeff ? d->omega_e_inv : d->omega_e;
  job.dom = d;
  job.d_in = d_in;
  job.d_out = d_out;
  job.C = C;
  job.keep = keep;
  job.flags = flags;
  return curve_ops(d->curve)->domain_run(ctx, &job);
}

int ext_to_coeff_check(const pm_domain* d, size_t keep, uint32_t flags) {
  if (keep == 0 || keep > ((size_t)1 << d->ext_k)) return set_error(PM_ERR_ARG, "keep out of range (1 <= keep <= N)");
  if (flags & ~(uint32_t)PM_EXT_DIVIDE_VANISHING) return set_error(PM_ERR_ARG, "unknown flag bits");
  return PM_OK;
}
}  // namespace

int pm_coeff_to_extended_device(pm_ctx* ctx, const pm_domain* d, const void* const* d_in, void* const* d_out,
                                size_t C) {
  int rc = domain_check(ctx, d, d_in, true, d_out, C);
  if (rc || C == 0) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return domain_run_locked(ctx, d, pm::kDomOpToExt, d_in, d_out, C, 0, 0);
}

int pm_extended_to_coeff_device(pm_ctx* ctx, const pm_domain* d, const void* const* d_in, void* const* d_out, size_t C,
                                size_t keep, uint32_t flags) {
  int rc = domain_check(ctx, d, d_in, true, d_out, C);
  if (rc || (rc = ext_to_coeff_check(d, keep, flags)) || C == 0) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return domain_run_locked(ctx, d, pm::kDomOpToCoeff, d_in, d_out, C, keep, flags);
}

int pm_divide_by_vanishing_device(pm_ctx* ctx, const pm_domain* d, void* const* d_data, size_t C) {
  int rc = domain_check(ctx, d, nullptr, false, d_data, C);
  if (rc || C == 0) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return domain_run_locked(ctx, d, pm::kDomOpDivide, nullptr, d_data, C, 0, 0);
}

int pm_fft_batch_device(pm_ctx* ctx, int curve, void* const* d_data, size_t C, uint32_t log_n, const uint64_t omega[4],
                        const uint64_t* scale) {
  if (!ctx || !omega || (C && !d_data)) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  for (size_t c = 0; c < C; c++)
    if (!d_data[c]) return set_error(PM_ERR_ARG, "null column pointer");
  if (log_n > pm::kNttMaxLog) return set_error(PM_ERR_UNSUPPORTED, "NTT longer than 2^28");
  if (C > pm::kPolyMaxGridY) return set_error(PM_ERR_UNSUPPORTED, "more than 65535 columns in one call");
  if (C == 0) return PM_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  pm::DomJob job{};
  job.op = pm::kDomOpFft;
  job.curve = curve;
  job.logn = log_n;
  job.omega = omega;
  job.scale = scale;
  job.d_out = d_data;
  job.C = C;
  return ops->domain_run(ctx, &job);
}

int pm_coeff_to_extended(pm_ctx* ctx, const pm_domain* d, const uint64_t* coeffs, uint64_t* out) {
  if (!ctx || !d || !coeffs || !out) return set_error(PM_ERR_ARG, "null argument");
  if (d->device != ctx->device) return set_error(PM_ERR_ARG, "the domain lives on another device");
  const size_t n = (size_t)1 << d->k, N = (size_t)1 << d->ext_k;
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  auto run = [&](void* buf) {
    const void* in = buf;  // the input is the prefix of its own output buffer
    return domain_run_locked(ctx, d, pm::kDomOpToExt, &in, &buf, 1, 0, 0);
  };
  return staged_call(ctx, coeffs, n * 32, N * 32, run, out, N * 32);
}

int pm_extended_to_coeff(pm_ctx* ctx, const pm_domain* d, const uint64_t* evals, size_t keep, uint32_t flags,
                         uint64_t* out) {
  if (!ctx || !d || !evals || !out) return set_error(PM_ERR_ARG, "null argument");
  if (d->device != ctx->device) return set_error(PM_ERR_ARG, "the domain lives on another device");
  int rc = ext_to_coeff_check(d, keep, flags);
  if (rc) return rc;
  const size_t N = (size_t)1 << d->ext_k;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  auto run = [&](void* buf) {
    const void* in = buf;
    return domain_run_locked(ctx, d, pm::kDomOpToCoeff, &in, &buf, 1, keep, flags);
  };
  return staged_call(ctx, evals, N * 32, N * 32, run, out, keep * 32);
}

// ------------------------------------------------- quotient numerator (§8f-8)
int pm_quotient_release(pm_quotient* q) {
  if (!q) return PM_OK;
  (void)hipSetDevice(q->device);
  delete q;
  return PM_OK;
}

namespace {
// test hook (as PM_NTT_PASSES): the slot bound under which repeated leaves stay resident, 0 = every use loads
uint32_t quot_cache_slots() {
  const char* e = std::getenv("PM_QUOT_CACHE_SLOTS");
  if (!e || !*e) return pm::kQuotCacheSlots;
  return (uint32_t)std::min<long>(std::max<long>(std::atol(e), 0), pm::kQuotMaxSlots);
}

// the quotient's buffers: program, leaf table, t, and its own columns (with the context's mutex held)
int quotient_build_locked(pm_ctx* ctx, const pm_domain* d, const pm_proof_shape* shape, pm_quotient* q) {
  const CurveOps* ops = curve_ops(d->curve);
  const pm::QuotPlan& pl = q->plan;
  const uint32_t e = d->ext_k - d->k, bf = shape->blinding_factors;
  const size_t n = (size_t)1 << d->k, N = (size_t)1 << d->ext_k, tl = (size_t)1 << e;
  const hipStream_t st = ctx->stream;
  int rc = ctx->begin_call();
  if (rc) return rc;
  std::vector<uint32_t> leaves(2 * pl.leaves.size() + 2, 0);
  for (size_t i = 0; i < pl.leaves.size(); i++) {
    leaves[2 * i] = pl.group_base[pl.leaves[i].kind] + pl.leaves[i].index;
    leaves[2 * i + 1] = (uint32_t)(((int64_t)pl.leaves[i].rot * ((int64_t)1 << e)) & (int64_t)(N - 1));
  }
  const size_t ncols = pl.need_x ? pm::kQownCols : pl.need_l ? pm::kQownX : 0;
  if ((rc = q->d_prog.ensure(pl.ops.size() * 4)) || (rc = q->d_leaves.ensure(leaves.size() * 4)) ||
      (rc = q->d_t.ensure(tl * 32)) || (rc = q->d_own.ensure(ncols * N * 32)))
    return rc;
  q->device_bytes = pl.ops.size() * 4 + leaves.size() * 4 + tl * 32 + ncols * N * 32;
  HIP_TRY(hipMemcpyAsync(q->d_prog.p, pl.ops.data(), pl.ops.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(q->d_leaves.p, leaves.data(), leaves.size() * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(q->d_t.p, (const char*)d->d_tab.p + (size_t)pm::kDomTabHead * 32, tl * 32, hipMemcpyDeviceToDevice,
                         st));
  if (!ncols) {
    HIP_TRY(hipStreamSynchronize(st));
    return PM_OK;
  }
  // unit vectors of the Lagrange basis, in the native form (x 2^261, so the columns need no
  // repair in a product): row 0; row n - bf - 1; rows n - bf - 1 .. n - 1; and X as a polynomial
  uint64_t seed[16];
  if ((rc = ops->quotient_seed(d, seed))) return rc;
  char* own = (char*)q->d_own.p;
  std::vector<uint64_t> ones(4 * ((size_t)bf + 1));
  for (size_t i = 0; i < ones.size(); i++) ones[i] = seed[8 + (i & 3)];
  for (size_t c = 0; c < ncols; c++) HIP_TRY(hipMemsetAsync(own + c * N * 32, 0, n * 32, st));
  HIP_TRY(hipMemcpyAsync(own + pm::kQownL0 * N * 32, ones.data(), 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(own + pm::kQownLast * N * 32 + (n - bf - 1) * 32, ones.data(), 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(own + pm::kQownSum * N * 32 + (n - bf - 1) * 32, ones.data(), ones.size() * 8,
                         hipMemcpyHostToDevice, st));
  if (pl.need_x) HIP_TRY(hipMemcpyAsync(own + pm::kQownX * N * 32 + 32, seed + 12, 32, hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  void* ptrs[pm::kQownCols];
  for (size_t c = 0; c < pm::kQownCols; c++) ptrs[c] = own + c * N * 32;
  pm::DomJob job{};  // Lagrange -> coefficients: pm_fft_batch_device with omega^-1 and n^-1
  job.op = pm::kDomOpFft;
  job.curve = d->curve;
  job.logn = d->k;
  job.omega = seed;
  job.scale = seed + 4;
  job.d_out = ptrs;
  job.C = pm::kQownX;
  if ((rc = ops->domain_run(ctx, &job))) return rc;
  return domain_run_locked(ctx, d, pm::kDomOpToExt, ptrs, ptrs, ncols, 0, 0);
}
}  // namespace

int pm_quotient_create(pm_ctx* ctx, const pm_domain* d, const pm_proof_shape* shape, pm_quotient** out) {
  if (!ctx || !d || !shape || !out) return set_error(PM_ERR_ARG, "null argument");
  *out = nullptr;
  if (d->device != ctx->device) return set_error(PM_ERR_ARG, "the domain lives on another device");
  if (shape->log_n != d->k) return set_error(PM_ERR_ARG, "shape.log_n differs from the domain's k");
  if (std::memcmp(shape->omega, d->omega, 32)) return set_error(PM_ERR_ARG, "shape.omega differs from the domain's omega");
  if (d->ext_k > pm::kQuotMaxLogN) return set_error(PM_ERR_UNSUPPORTED, "extended domain longer than 2^28");
  std::unique_ptr<pm_quotient> q(new pm_quotient{});
  AccLayout L;
  bool unsupported = false;
  const std::string err =
      pm::quot_compile(shape, (int)(d->ext_k - d->k), d->ext_k, quot_cache_slots(), &q->plan, &L, &unsupported);
  if (!err.empty()) return set_error(unsupported ? PM_ERR_UNSUPPORTED : PM_ERR_ARG, "quotient: " + err);
  if (((uint64_t)1 << d->k) < (uint64_t)shape->blinding_factors + 2)
    return set_error(PM_ERR_ARG, "quotient: fewer rows than blinding_factors + 2");
  q->curve = d->curve;
  q->device = ctx->device;
  q->k = d->k;
  q->ext_k = d->ext_k;
  if (shape->n_constants) q->shape_consts.assign(shape->constants, shape->constants + 4 * (size_t)shape->n_constants);
  std::memcpy(q->delta, shape->delta, 32);
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (const int rc = quotient_build_locked(ctx, d, shape, q.get())) return rc;  // q frees what it built, on ctx->device
  *out = q.release();
  return PM_OK;
}

int pm_quotient_info(const pm_quotient* q, uint32_t* n_expressions, uint32_t* products_per_row, uint32_t* loads_per_row,
                     uint32_t* slots, size_t* device_bytes) {
  if (!q) return set_error(PM_ERR_ARG, "null argument");
  if (n_expressions) *n_expressions = q->plan.n_expr;
  if (products_per_row) *products_per_row = q->plan.products;
  if (loads_per_row) *loads_per_row = q->plan.loads;
  if (slots) *slots = q->plan.slots;
  if (device_bytes) *device_bytes = q->device_bytes;
  return PM_OK;
}

int pm_quotient_device(pm_ctx* ctx, const pm_quotient* q, const pm_quotient_columns* cols, const uint64_t challenges[16],
                       uint32_t flags, void* d_out) {
  if (!ctx || !q || !cols || !challenges || !d_out) return set_error(PM_ERR_ARG, "null argument");
  if (q->device != ctx->device) return set_error(PM_ERR_ARG, "the quotient lives on another device");
  if (flags & ~(uint32_t)(PM_QUOT_DIVIDE_VANISHING | PM_QUOT_ACCUMULATE)) return set_error(PM_ERR_ARG, "unknown flag bits");
  const void* const* groups[pm::kQlOwn] = {cols->advice, cols->fixed,    cols->instance, cols->sigma,
                                           cols->perm_z, cols->lookup_a, cols->lookup_s, cols->lookup_z};
  const uint32_t* base = q->plan.group_base;
  std::vector<const void*> ptrs(base[pm::kQlOwn] + 1);
  for (uint32_t g = 0; g < pm::kQlOwn; g++) {
    const uint32_t cnt = base[g + 1] - base[g];
    if (cnt && !groups[g]) return set_error(PM_ERR_ARG, "null column array");
    for (uint32_t i = 0; i < cnt; i++) {
      if (!groups[g][i]) return set_error(PM_ERR_ARG, "null column pointer");
      ptrs[base[g] + i] = groups[g][i];
    }
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  const int rc = ctx->begin_call();
  if (rc) return rc;
  return curve_ops(q->curve)->quotient_run(ctx, q, ptrs.data(), challenges, flags, d_out);
}

int pm_quotient_eval_host(int curve, const pm_proof_shape* shape, size_t R, const uint64_t* scalars, const uint64_t* x,
                          const uint64_t* challenges, uint64_t* out) {
  if (!shape || (R && (!scalars || !x || !challenges || !out))) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  return ops->quotient_eval_host(shape, R, scalars, x, challenges, out);
}


}  // extern "C"

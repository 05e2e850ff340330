// capi_msm.hip -- MSM entries of the C-ABI: device / multi-device MSM,
// resident bases and their row tables, many short MSMs, fixed-base tables,
// point sums and the synthetic inputs.  (pm_msm / pm_msm_ctx: capi_dropin.hip.)
#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.hpp"

using namespace pm;

// the caller holds ctx->mu and has run begin_call
int pm::bases_upload_locked(pm_ctx* ctx, int curve, const void* bases, bool host, size_t n, pm_bases** out) {
  const CurveOps* ops = curve_ops(curve);
  int rc;
  std::unique_ptr<pm_bases> b(new pm_bases{curve, ctx->device, n, nullptr});
  const void* src = bases;
  if (host && n) {
    if ((rc = ctx->in_bases.ensure(n * 64)) || (rc = ctx->upload_h2d(ctx->in_bases.p, bases, n * 64, ctx->stream)))
      return rc;
    src = ctx->in_bases.p;
  }
  const int rows = resident_rows(n);
  if (rows > 1) {
    b->table.reset(new pm_fixed_bases{curve, ctx->device, 16, 0, rows, n, 0});
    if ((rc = ops->fixed_table(ctx, src, b->table.get()))) return rc;
    b->d = b->table->d.p;
  } else {
    if ((rc = b->own.ensure(std::max<size_t>(64, n * 64))) || (rc = ops->bases_to29(ctx, src, n, b->own.p))) return rc;
    b->d = b->own.p;
  }
  *out = b.release();
  return PM_OK;
}

// arguments validated, ctx->mu held (pm_multiopen_open_device commits its quotient rows under one lock)
int pm::msm_resident_locked(pm_ctx* ctx, const pm_bases* b, size_t offset, const void* scalars, bool host, size_t n,
                            uint32_t flags, uint64_t out[8]) {
  if (n == 0) return zero_point(out);
  int rc = ctx->begin_call();
  if (rc) return rc;
  const void* d_s = scalars;
  if (host) {  // copied by msm_device_impl (in two parts with a row table)
    if ((rc = ctx->in_scalars.ensure(n * 32))) return rc;
    d_s = ctx->in_scalars.p;
  }
  if (use_small(ctx, n))  // row 0 of a row table is the bases themselves
    return curve_ops(b->curve)->msm_small(ctx, scalars, host, (const char*)b->d + offset * 64, false, true, n,
                                          flags & ~kBasesR261, out);
  const void* h_s = host ? scalars : nullptr;
  if (resident_use_table(b, offset, n))
    return curve_ops(b->curve)->msm_fixed(ctx, b->table.get(), d_s, n, flags & ~kBasesR261, out, h_s);
  return dispatch_msm_device(ctx, b->curve, d_s, (const char*)b->d + offset * 64, n, flags, out, true, h_s);
}

extern "C" {

int pm_msm_device(pm_ctx* ctx, int curve, const void* d_scalars, const void* d_bases, size_t n, uint32_t flags,
                  uint64_t out[8]) {
  if (!ctx || !out || (n && (!d_scalars || !d_bases))) return set_error(PM_ERR_ARG, "null argument");
  if (!checked_ops(curve)) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return zero_point(out);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if (use_small(ctx, n)) return curve_ops(curve)->msm_small(ctx, d_scalars, false, d_bases, false, false, n, flags, out);
  return dispatch_msm_device(ctx, curve, d_scalars, d_bases, n, flags, out);
}

int pm_msm_multi(int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags, int ngpu,
                 uint64_t out[8]) {
  if (!out || (n && (!scalars || !bases))) return set_error(PM_ERR_ARG, "null argument");
  if (!checked_ops(curve)) return PM_ERR_ARG;
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return set_error(PM_ERR_NODEV, "no HIP device");
  if (ngpu <= 0 || ngpu > cnt) return set_error(PM_ERR_NODEV, "ngpu out of range");
  std::vector<uint64_t> parts((size_t)ngpu * 8, 0);
  std::vector<int> rcs(ngpu, PM_OK);
  std::vector<std::string> errs(ngpu);
  std::vector<std::thread> th;
  const size_t per = (n + ngpu - 1) / ngpu;
  for (int g = 0; g < ngpu; g++) {
    th.emplace_back([&, g]() {
      const size_t lo = std::min(n, per * g), hi = std::min(n, per * (g + 1));
      Ctx* ctx = nullptr;
      int rc = default_ctx(g, &ctx);
      if (!rc) rc = pm_msm_ctx(ctx, curve, scalars + 4 * lo, bases + 8 * lo, hi - lo, flags, &parts[8 * g]);
      rcs[g] = rc;
      if (rc) errs[g] = pm::g_last_error;
    });
  }
  for (auto& t : th) t.join();
  for (int g = 0; g < ngpu; g++)
    if (rcs[g]) return set_error(rcs[g], "device " + std::to_string(g) + ": " + errs[g]);
  return pm_points_sum(curve, parts.data(), (size_t)ngpu, out);
}

static int bases_upload(pm_ctx* ctx, int curve, const void* bases, bool host, size_t n, pm_bases** out) {
  if (!ctx || !out || (n && !bases)) return set_error(PM_ERR_ARG, "null argument");
  *out = nullptr;
  if (!checked_ops(curve)) return PM_ERR_ARG;
  if (n > kMaxPoints) return set_error(PM_ERR_UNSUPPORTED, "more than 2^26 resident bases");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return bases_upload_locked(ctx, curve, bases, host, n, out);
}

int pm_bases_upload(pm_ctx* ctx, int curve, const uint64_t* bases, size_t n, pm_bases** out) {
  return bases_upload(ctx, curve, bases, true, n, out);
}

int pm_bases_upload_device(pm_ctx* ctx, int curve, const void* d_bases, size_t n, pm_bases** out) {
  return bases_upload(ctx, curve, d_bases, false, n, out);
}

int pm_bases_info(const pm_bases* b, size_t* n, int* rows, size_t* device_bytes) {
  if (!b) return set_error(PM_ERR_ARG, "null argument");
  if (n) *n = b->n;
  if (rows) *rows = b->table ? b->table->rows : 1;
  if (device_bytes)
    *device_bytes = b->table ? (size_t)b->table->rows * b->table->npad * 64 : std::max<size_t>(64, b->n * 64);
  return PM_OK;
}

int pm_bases_release(pm_bases* b) {
  if (!b) return PM_OK;
  (void)hipSetDevice(b->device);
  delete b;
  return PM_OK;
}

static int msm_resident(pm_ctx* ctx, const pm_bases* b, size_t offset, const void* scalars, bool host, size_t n,
                        uint32_t flags, uint64_t out[8]) {
  if (!ctx || !b || !out || (n && !scalars)) return set_error(PM_ERR_ARG, "null argument");
  if (b->device != ctx->device) return set_error(PM_ERR_ARG, "bases live on another device");
  if (offset > b->n || n > b->n - offset) return set_error(PM_ERR_ARG, "window exceeds resident bases");
  std::lock_guard<std::mutex> lk(ctx->mu);
  return msm_resident_locked(ctx, b, offset, scalars, host, n, flags, out);
}

// ------------------------------------- many short MSMs (pm_msm_resident_many)
namespace {
// the multiples table covers the first n bases (grown to a power of two,
// at least 64, at most the set); the caller holds ctx->mu and b->many_mu
int many_ensure(pm_ctx* ctx, const pm_bases* b, size_t need) {
  if (b->many.d.p && b->many.n >= need) return PM_OK;
  size_t n = 64;
  while (n < need) n <<= 1;
  n = std::max(need, std::min({n, b->n, pm::kManyTabCap / pm::many_bytes_per_base(4)}));
  return curve_ops(b->curve)->many_table(ctx, b->d, n, &b->many);
}
}  // namespace

static int msm_many(pm_ctx* ctx, const pm_bases* b, size_t B, const size_t* n, const size_t* offsets,
                    const void* scalars, bool host, uint32_t flags, uint64_t* out) {
  if (!ctx || !b || (B && (!n || !out))) return set_error(PM_ERR_ARG, "null argument");
  if (b->device != ctx->device) return set_error(PM_ERR_ARG, "bases live on another device");
  if (B > (size_t(1) << 20)) return set_error(PM_ERR_UNSUPPORTED, "more than 2^20 MSMs in one call");
  size_t need = 0, total = 0;
  for (size_t i = 0; i < B; i++) {
    const size_t o = offsets ? offsets[i] : 0;
    if (o > b->n || n[i] > b->n - o) return set_error(PM_ERR_ARG, "an MSM window exceeds the resident bases");
    if (n[i]) need = std::max(need, o + n[i]);
    total += n[i];
  }
  if (total && !scalars) return set_error(PM_ERR_ARG, "null scalars");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if (need * pm::many_bytes_per_base(4) > pm::kManyTabCap) {
    // a prefix too long for a table: one resident MSM per entry (same results)
    size_t s0 = 0;
    for (size_t i = 0; i < B; i++) {
      const void* si = (const char*)scalars + s0 * 32;
      const size_t o = offsets ? offsets[i] : 0;
      if (n[i] == 0) std::memset(out + 8 * i, 0, 64);
      else if (use_small(ctx, n[i]))
        rc = curve_ops(b->curve)->msm_small(ctx, si, host, (const char*)b->d + o * 64, false, true, n[i],
                                            flags & ~kBasesR261, out + 8 * i);
      else {
        const void* d_s = si;
        if (host) {
          if ((rc = ctx->in_scalars.ensure(n[i] * 32))) return rc;
          d_s = ctx->in_scalars.p;
        }
        rc = dispatch_msm_device(ctx, b->curve, d_s, (const char*)b->d + o * 64, n[i], flags, out + 8 * i, true,
                                 host ? si : nullptr);
      }
      if (rc) return rc;
      if ((rc = ctx->begin_call())) return rc;
      s0 += n[i];
    }
    return PM_OK;
  }
  std::lock_guard<std::mutex> lt(b->many_mu);
  if (need && (rc = many_ensure(ctx, b, need))) return rc;
  return curve_ops(b->curve)->msm_many(ctx, &b->many, B, n, offsets, scalars, host, flags, out);
}

int pm_msm_resident_many(pm_ctx* ctx, const pm_bases* bases, size_t B, const size_t* n, const size_t* offsets,
                         const uint64_t* scalars, uint32_t flags, uint64_t* out) {
  return msm_many(ctx, bases, B, n, offsets, scalars, true, flags, out);
}

int pm_msm_resident_many_device(pm_ctx* ctx, const pm_bases* bases, size_t B, const size_t* n, const size_t* offsets,
                                const void* d_scalars, uint32_t flags, uint64_t* out) {
  return msm_many(ctx, bases, B, n, offsets, d_scalars, false, flags, out);
}

int pm_bases_many_prepare(pm_ctx* ctx, const pm_bases* bases, size_t max_n) {
  if (!ctx || !bases) return set_error(PM_ERR_ARG, "null argument");
  if (bases->device != ctx->device) return set_error(PM_ERR_ARG, "bases live on another device");
  if (max_n > bases->n) return set_error(PM_ERR_ARG, "prefix exceeds the resident bases");
  if (max_n * pm::many_bytes_per_base(4) > pm::kManyTabCap)
    return set_error(PM_ERR_UNSUPPORTED, "prefix too long for a multiples table");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  std::lock_guard<std::mutex> lt(bases->many_mu);
  return max_n ? many_ensure(ctx, bases, max_n) : PM_OK;
}

int pm_bases_many_info(const pm_bases* bases, size_t* n, int* window, size_t* device_bytes) {
  if (!bases) return set_error(PM_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lt(bases->many_mu);
  if (n) *n = bases->many.d.p ? bases->many.n : 0;
  if (window) *window = bases->many.d.p ? (int)bases->many.c : 0;
  if (device_bytes) *device_bytes = bases->many.d.p ? bases->many.n * pm::many_bytes_per_base(bases->many.c) : 0;
  return PM_OK;
}

int pm_msm_resident(pm_ctx* ctx, const pm_bases* b, size_t offset, const uint64_t* scalars, size_t n,
                    uint32_t flags, uint64_t out[8]) {
  return msm_resident(ctx, b, offset, scalars, true, n, flags, out);
}

int pm_msm_resident_device(pm_ctx* ctx, const pm_bases* b, size_t offset, const void* d_scalars, size_t n,
                           uint32_t flags, uint64_t out[8]) {
  return msm_resident(ctx, b, offset, d_scalars, false, n, flags, out);
}

int pm_msm_resident_batch(pm_ctx* ctx, const pm_bases* b, size_t offset, const uint64_t* const* scalars, size_t k,
                          size_t n, uint32_t flags, uint64_t* out) {
  if (!ctx || !b || (k && (!scalars || !out))) return set_error(PM_ERR_ARG, "null argument");
  for (size_t j = 0; j < k && n; j++)
    if (!scalars[j]) return set_error(PM_ERR_ARG, "null scalar array");
  if (b->device != ctx->device) return set_error(PM_ERR_ARG, "bases live on another device");
  if (offset > b->n || n > b->n - offset) return set_error(PM_ERR_ARG, "window exceeds resident bases");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  return curve_ops(b->curve)->msm_resident_batch(ctx, (const char*)b->d + offset * 64,
                                                 resident_use_table(b, offset, n) ? b->table.get() : nullptr, scalars, k,
                                                 n, flags & ~kBasesR261, out);
}

// ------------------------------------------------- fixed-base MSM (§8f-3)
static int fixed_create(pm_ctx* ctx, int curve, const void* bases, bool host, size_t n, int c, int rows,
                        pm_fixed_bases** out) {
  if (!ctx || !out || (n && !bases)) return set_error(PM_ERR_ARG, "null argument");
  *out = nullptr;
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (n == 0) return set_error(PM_ERR_ARG, "empty base set");
  if (n > kMaxPoints) return set_error(PM_ERR_UNSUPPORTED, "more than 2^26 fixed bases");
  if (c == 0) c = n > (size_t(1) << 21) ? kAutoFixedCLarge : kAutoFixedC;
  if (c < kMinC || c > kFixedMaxC) return set_error(PM_ERR_ARG, "fixed-base window out of range");
  std::lock_guard<std::mutex> lk(ctx->mu);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if (rows < 0) return set_error(PM_ERR_ARG, "negative table rows");
  std::unique_ptr<pm_fixed_bases> ft(new pm_fixed_bases{curve, ctx->device, c, 0, rows, n, 0});
  const void* d = bases;
  if (host) {
    if ((rc = ctx->in_bases.ensure(n * 64))) return rc;
    if ((rc = ctx->upload_h2d(ctx->in_bases.p, bases, n * 64, ctx->stream))) return rc;
    d = ctx->in_bases.p;
  }
  if ((rc = ops->fixed_table(ctx, d, ft.get()))) return rc;
  *out = ft.release();
  return PM_OK;
}

int pm_fixed_bases_create(pm_ctx* ctx, int curve, const uint64_t* bases, size_t n, int c, pm_fixed_bases** out) {
  return fixed_create(ctx, curve, bases, true, n, c, 0, out);
}

int pm_fixed_bases_create_device(pm_ctx* ctx, int curve, const void* d_bases, size_t n, int c,
                                 pm_fixed_bases** out) {
  return fixed_create(ctx, curve, d_bases, false, n, c, 0, out);
}

int pm_fixed_bases_create_rows(pm_ctx* ctx, int curve, const void* bases, int bases_on_device, size_t n, int c,
                               int rows, pm_fixed_bases** out) {
  return fixed_create(ctx, curve, bases, bases_on_device == 0, n, c, rows, out);
}

int pm_fixed_bases_info(const pm_fixed_bases* fb, size_t* n, int* c, int* windows, size_t* table_bytes) {
  if (!fb) return set_error(PM_ERR_ARG, "null argument");
  if (n) *n = fb->n;
  if (c) *c = fb->c;
  if (windows) *windows = fb->W;
  if (table_bytes) *table_bytes = (size_t)fb->rows * fb->npad * 64;
  return PM_OK;
}

int pm_fixed_bases_release(pm_fixed_bases* fb) {
  if (!fb) return PM_OK;
  (void)hipSetDevice(fb->device);
  delete fb;
  return PM_OK;
}

// host: the scalars are in host memory (copied by the MSM itself into in_scalars)
static int msm_fixed(pm_ctx* ctx, const pm_fixed_bases* fb, const void* scalars, bool host, size_t n, uint32_t flags,
                     uint64_t out[8]) {
  if (!ctx || !fb || !out || (n && !scalars)) return set_error(PM_ERR_ARG, "null argument");
  if (fb->device != ctx->device) return set_error(PM_ERR_ARG, "fixed bases live on another device");
  if (n > fb->n) return set_error(PM_ERR_ARG, "more scalars than fixed bases");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return zero_point(out);
  int rc = ctx->begin_call();
  if (rc) return rc;
  if (host && (rc = ctx->in_scalars.ensure(n * 32))) return rc;
  return curve_ops(fb->curve)->msm_fixed(ctx, fb, host ? ctx->in_scalars.p : scalars, n, flags & ~kBasesR261, out,
                                         host ? scalars : nullptr);
}

int pm_msm_fixed_device(pm_ctx* ctx, const pm_fixed_bases* fb, const void* d_scalars, size_t n, uint32_t flags,
                        uint64_t out[8]) {
  return msm_fixed(ctx, fb, d_scalars, false, n, flags, out);
}

int pm_msm_fixed(pm_ctx* ctx, const pm_fixed_bases* fb, const uint64_t* scalars, size_t n, uint32_t flags,
                 uint64_t out[8]) {
  return msm_fixed(ctx, fb, scalars, true, n, flags, out);
}

int pm_point_add(int curve, const uint64_t a[8], const uint64_t b[8], uint64_t out[8]) {
  if (!a || !b || !out) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  return ops->point_add(a, b, out);
}

int pm_points_sum(int curve, const uint64_t* points, size_t n, uint64_t out[8]) {
  if (!out || (n && !points)) return set_error(PM_ERR_ARG, "null argument");
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  if (n == 0) return zero_point(out);
  return ops->points_sum(points, n, out);
}

static int synth(pm_ctx* ctx, int curve, uint64_t seed, uint64_t i0, size_t n, bool bases, uint32_t mont, void* d_out) {
  if (!ctx || (n && !d_out)) return set_error(PM_ERR_ARG, "null argument");
  if (n > 0xffffffffull) return set_error(PM_ERR_ARG, "n too large");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (n == 0) return PM_OK;
  int rc = ctx->begin_call();
  if (rc) return rc;
  const CurveOps* ops = checked_ops(curve);
  if (!ops) return PM_ERR_ARG;
  return bases ? ops->synth_bases(ctx, seed, i0, (uint32_t)n, d_out)
               : ops->synth_scalars(ctx, seed, i0, (uint32_t)n, mont, d_out);
}

int pm_synth_scalars(pm_ctx* ctx, int curve, uint64_t seed, uint64_t i0, size_t n, uint32_t flags, void* d_out) {
  return synth(ctx, curve, seed, i0, n, false, (flags & PM_SCALARS_CANONICAL) ? 0u : 1u, d_out);
}

int pm_synth_bases(pm_ctx* ctx, int curve, uint64_t seed, uint64_t i0, size_t n, void* d_out) {
  return synth(ctx, curve, seed, i0, n, true, 0, d_out);
}

}  // extern "C"

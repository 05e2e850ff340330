// capi_dropin.hip -- pm_msm / pm_msm_ctx and the drop-in base cache behind them.
#include <algorithm>
#include <chrono>
#include <vector>

#include "blake2b.hpp"
#include "capi_internal.hpp"

using namespace pm;

// ------------------------------------------------ drop-in base cache (pm_msm)
// halo2 calls best_multiexp with the same SRS bases over and over
// (commit_lagrange over params.g_lagrange, the commits inside create_proof:
// examples/simple-example.rs:606,638-640,702).  pm_msm / pm_msm_ctx keep base
// sets of >= kDropinMinN points resident, keyed by (curve, n, a keyed 254-bit
// digest of the base bytes: dropin_digest.hpp, secret key per context), so a
// repeated set skips its 64 B/point upload and runs as a resident (row-table)
// MSM.  The digest is computed on the host pool while the scalars cross
// PCIe; any change of the bytes (same pointer or not) changes the key.
//  * admission on the second sighting: the first call with a set runs the
//    plain pipeline on uploaded bases (no row-table build for one-shot sets)
//    and only remembers the digest;
//  * memory: least recently used sets are evicted BEFORE a new one is built,
//    against kDropinEntries and min(kDropinBytes, free device memory /
//    kDropinFreeDiv); if the build still fails, every set is released and the
//    build retried once, and if that fails the call runs the plain pipeline.
namespace {
constexpr size_t kDigestChunk = size_t(1) << 15;  // points per chunk (2 MiB)

// device bytes of a resident set of n points (bases_upload_locked's layout)
size_t dropin_bytes(size_t n) {
  const int rows = resident_rows(n);
  if (rows <= 1) return std::max<size_t>(64, n * 64);
  return (size_t)rows * std::max<size_t>(kSortB, (n + kSortB - 1) / kSortB * kSortB) * 64;  // fixed_table's npad
}

bool same_key(const pm::DropinEntry& e, int curve, size_t n, const uint64_t d[4]) {
  return e.curve == curve && e.n == n && std::memcmp(e.d, d, sizeof(e.d)) == 0;
}
}  // namespace

void pm::dropin_release_all(pm_ctx* ctx) {
  for (auto& e : ctx->dropin) pm_bases_release(e.b);
  ctx->dropin.clear();
  for (auto& e : ctx->dropin_small) pm_bases_release(e.b);
  ctx->dropin_small.clear();
}

static size_t dropin_small_total(const pm_ctx* ctx) {
  size_t s = 0;
  for (auto& e : ctx->dropin_small) s += e.bytes;
  return s;
}

// every byte the drop-in cache holds: the large sets and the small sets' tables
static size_t dropin_total(const pm_ctx* ctx) {
  size_t s = dropin_small_total(ctx);
  for (auto& e : ctx->dropin) s += e.bytes;
  return s;
}

static void dropin_evict_lru(pm_ctx* ctx) {
  auto lru = std::min_element(ctx->dropin.begin(), ctx->dropin.end(),
                              [](const pm::DropinEntry& x, const pm::DropinEntry& y) { return x.last_use < y.last_use; });
  pm_bases_release(lru->b);
  ctx->dropin.erase(lru);
}

// make room for `bytes` more: LRU eviction against the entry count and the
// memory budget (the fixed cap and a fraction of what the device has free)
static void dropin_make_room(pm_ctx* ctx, size_t bytes) {
  size_t free_b = 0, total_b = 0;
  const bool have_info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
  for (;;) {
    if (ctx->dropin.empty()) return;
    const size_t held = dropin_total(ctx);
    size_t budget = kDropinBytes;
    if (have_info) budget = std::min(budget, (free_b + held) / kDropinFreeDiv);
    if ((int)ctx->dropin.size() < kDropinEntries && held + bytes <= budget) return;
    const size_t before = ctx->dropin.size();
    dropin_evict_lru(ctx);
    if (have_info) free_b += held - dropin_total(ctx);
    if (ctx->dropin.size() == before) return;
  }
}

// Small sets (the small-MSM path's sizes): a repeated set -- halo2's
// commit_lagrange of a few public inputs against the first bases of
// g_lagrange, examples/simple-example.rs:632-641 -- is kept resident with a
// multiples table after its second sighting and then runs as ONE short MSM of
// pm_msm_resident_many (no doublings, no host Horner); first sightings and
// sets that do not fit run the small-MSM path on the host inputs.  The keyed
// digest of a small set is cheap (at most 1 MiB of bases).
// up to pm::kDropinSmallMaxN = 64 points (measured,
// profiles/r05/small_n_cache.json: a kept set against the small-MSM path 38 vs
// 66 us at n = 1, 63 vs 73 at 32, 82 vs 93 at 512 -- the last not worth its
// 256 MiB table, ADVICE r5 -- 107 vs 106 at 1024, 174 vs 139 at 4096)
static int dropin_small_msm(Ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* bases, size_t n,
                            uint32_t flags, uint64_t out[8]) {
  const CurveOps* ops = curve_ops(curve);
  auto small = [&]() { return ops->msm_small(ctx, scalars, true, bases, true, false, n, flags, out); };
  const size_t tbytes = n * pm::many_bytes_per_base(pm::many_pick_c(n));
  if (n > pm::kDropinSmallMaxN || tbytes > pm::kDropinSmallBytes / 2) return small();
  pm::u128 part[2];
  pm::digest_chunk(ctx->dropin_key, bases, 8 * n, part);
  uint64_t d[4];
  pm::digest_combine(ctx->dropin_key, part, 1, d);
  pm_bases* b = nullptr;
  for (auto& e : ctx->dropin_small)
    if (same_key(e, curve, n, d)) {
      e.last_use = ++ctx->dropin_clock;
      b = e.b;
      break;
    }
  if (!b) {
    auto seen = std::find_if(ctx->dropin_small_seen.begin(), ctx->dropin_small_seen.end(),
                             [&](const pm::DropinEntry& e) { return same_key(e, curve, n, d); });
    if (seen == ctx->dropin_small_seen.end()) {  // first sighting
      if ((int)ctx->dropin_small_seen.size() >= kDropinSeen) ctx->dropin_small_seen.erase(ctx->dropin_small_seen.begin());
      ctx->dropin_small_seen.push_back(pm::DropinEntry{curve, n, {d[0], d[1], d[2], d[3]}, nullptr, 0, ++ctx->dropin_clock});
      return small();
    }
    ctx->dropin_small_seen.erase(seen);
    // LRU room against the entry count, the small sets' byte cap and the
    // drop-in cache's whole budget (large sets included: min(kDropinBytes,
    // free device memory / kDropinFreeDiv)); a set that still does not fit
    // is not admitted
    const size_t need = tbytes + 64 * n;
    size_t free_b = 0, total_b = 0;
    const bool have_info = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
    for (;;) {
      const size_t held = dropin_total(ctx), held_small = dropin_small_total(ctx);
      size_t budget = kDropinBytes;
      if (have_info) budget = std::min(budget, (free_b + held) / kDropinFreeDiv);
      if ((int)ctx->dropin_small.size() < kDropinSmallEntries && held_small + need <= pm::kDropinSmallBytes &&
          held + need <= budget)
        break;
      // the large sets alone leave no room: keep the small sets, do not admit
      if (ctx->dropin_small.empty() || held - held_small + need > budget) return small();
      auto lru = std::min_element(ctx->dropin_small.begin(), ctx->dropin_small.end(),
                                  [](const pm::DropinEntry& x, const pm::DropinEntry& y) { return x.last_use < y.last_use; });
      if (have_info) free_b += lru->bytes;
      pm_bases_release(lru->b);
      ctx->dropin_small.erase(lru);
    }
    int rc = bases_upload_locked(ctx, curve, bases, true, n, &b);
    if (!rc) {
      std::lock_guard<std::mutex> lt(b->many_mu);
      rc = ops->many_table(ctx, b->d, n, &b->many);
    }
    if (rc) {  // not admitted (e.g. out of memory): the small path still computes it
      if (b) pm_bases_release(b);
      pm::g_last_error.clear();
      if ((rc = ctx->begin_call())) return rc;
      return small();
    }
    ctx->dropin_small_admits++;
    ctx->dropin_small.push_back(pm::DropinEntry{curve, n, {d[0], d[1], d[2], d[3]}, b, tbytes + 64 * n,
                                                ++ctx->dropin_clock});
    if (int r = ctx->begin_call()) return r;
  } else {
    ctx->dropin_small_hits++;
  }
  std::lock_guard<std::mutex> lt(b->many_mu);
  return ops->msm_many(ctx, &b->many, 1, &n, nullptr, scalars, true, flags, out);
}

static int dropin_msm(Ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags,
                      uint64_t out[8]) {
  if (n == 0) return zero_point(out);
  int rc;
  if ((rc = ctx->begin_call())) return rc;
  if (use_small(ctx, n)) return dropin_small_msm(ctx, curve, scalars, bases, n, flags, out);
  if ((rc = ctx->in_scalars.ensure(n * 32))) return rc;
  auto plain = [&]() -> int {  // both inputs uploaded, plain pipeline
    int r;
    if ((r = ctx->in_bases.ensure(n * 64))) return r;
    if ((r = ctx->upload_h2d(ctx->in_bases.p, bases, n * 64, ctx->stream))) return r;
    return dispatch_msm_device(ctx, curve, ctx->in_scalars.p, ctx->in_bases.p, n, flags, out);
  };
  if (n < kDropinMinN || n > kMaxPoints) {  // small MSMs bypass the cache
    if ((rc = ctx->upload_h2d(ctx->in_scalars.p, scalars, n * 32, ctx->stream))) return rc;
    return plain();
  }
  // keyed digest of the bases on the pool's workers while this thread copies the scalars
  const size_t nch = (n + kDigestChunk - 1) / kDigestChunk;
  std::vector<pm::u128> part(2 * nch);
  pm::HostPool& pool = ctx->host_pool();
  const int nw = std::max(1, pool.size() - 1);
  const pm::DigestKey& key = ctx->dropin_key;
  auto job = [&](int t, int) {
    for (size_t k = (size_t)(t - 1); k < nch; k += (size_t)nw) {
      const size_t p0 = k * kDigestChunk, p1 = std::min(n, p0 + kDigestChunk);
      pm::digest_chunk(key, bases + 8 * p0, 8 * (p1 - p0), &part[2 * k]);
    }
  };
  // a cheap keyed hash of the first and last 8 points names the resident set
  // this call most likely hits; its MSM starts right behind the scalar copy,
  // while the pool still hashes every byte, and its result is returned only
  // if the full digest then names the same set (else it is drained and the
  // call goes on as a miss)
  uint64_t quick;
  {
    const size_t k = std::min<size_t>(n, 8);
    pm::u128 a[2], z[2];
    pm::digest_chunk(key, bases, 8 * k, a);
    pm::digest_chunk(key, bases + 8 * (n - k), 8 * k, z);
    quick = (uint64_t)a[0] ^ ((uint64_t)(z[1] >> 64) * 0x9E3779B97F4A7C15ull) ^ (uint64_t)n;
  }
  const pm_bases* spec = nullptr;
  uint64_t spec_use = 0;
  for (auto& e : ctx->dropin)
    if (e.curve == curve && e.n == n && e.quick == quick && e.last_use >= spec_use) {
      spec = e.b;
      spec_use = e.last_use;
    }
  const bool threaded = pool.size() > 1;
  const auto t0 = std::chrono::steady_clock::now();
  if (threaded) pool.start(pool.size(), job);
  // with a predicted set the MSM copies the scalars itself (a row table's
  // MSM in two parts, the first part's sort and accumulation beside the
  // second part's copy: engine.hpp); else one copy here
  alignas(16) unsigned char tail[pm::kTailBytes];
  int spec_rc = -1, copy_rc = 0;
  if (spec)
    spec_rc = curve_ops(curve)->msm_start(ctx, resident_use_table(spec, 0, n) ? spec->table.get() : nullptr, spec->d,
                                          ctx->in_scalars.p, n, flags, tail, scalars);
  else
    copy_rc = ctx->upload_h2d(ctx->in_scalars.p, scalars, n * 32, ctx->stream);
  const auto t1 = std::chrono::steady_clock::now();
  if (threaded) pool.wait();
  else job(1, 1);
  if (copy_rc) return copy_rc;
  if (spec && spec_rc) return spec_rc;
  uint64_t d[4];
  pm::digest_combine(key, part.data(), nch, d);
  if (ctx->timing) {  // host-side phases of the drop-in call (bench.py dropin_pm_msm)
    const auto t2 = std::chrono::steady_clock::now();
    auto add = [&](const char* k, double ms) {
      auto& e = ctx->stats[k];
      e.first += 1;
      e.second += ms;
    };
    add("dropin_copy_call", std::chrono::duration<double, std::milli>(t1 - t0).count());
    add("dropin_digest", std::chrono::duration<double, std::milli>(t2 - t0).count());
  }
  pm_bases* b = nullptr;
  for (auto& e : ctx->dropin)
    if (same_key(e, curve, n, d)) {
      e.last_use = ++ctx->dropin_clock;
      e.quick = quick;
      b = e.b;
      ctx->dropin_hits++;
      break;
    }
  if (spec) {
    if (b == spec) {
      ctx->dropin_spec_hits++;
      return curve_ops(curve)->msm_finish(ctx, tail, out);
    }
    uint64_t junk[8];  // another set: drain the speculative MSM
    if ((rc = curve_ops(curve)->msm_finish(ctx, tail, junk))) return rc;
    ctx->dropin_spec_misses++;
    if ((rc = ctx->begin_call())) return rc;
  }
  if (!b) {
    ctx->dropin_misses++;
    auto seen = std::find_if(ctx->dropin_seen.begin(), ctx->dropin_seen.end(),
                             [&](const pm::DropinEntry& e) { return same_key(e, curve, n, d); });
    if (seen == ctx->dropin_seen.end()) {  // first sighting: remember it, plain pipeline
      if ((int)ctx->dropin_seen.size() >= kDropinSeen) ctx->dropin_seen.erase(ctx->dropin_seen.begin());
      pm::DropinEntry e{curve, n, {d[0], d[1], d[2], d[3]}, nullptr, 0, ++ctx->dropin_clock};
      ctx->dropin_seen.push_back(e);
      return plain();
    }
    ctx->dropin_seen.erase(seen);
    dropin_make_room(ctx, dropin_bytes(n));
    rc = bases_upload_locked(ctx, curve, bases, true, n, &b);
    if (rc && !ctx->dropin.empty()) {  // out of device memory: release every set and retry once
      dropin_release_all(ctx);
      ctx->dropin_oom_flushes++;
      rc = bases_upload_locked(ctx, curve, bases, true, n, &b);
    }
    if (rc) {  // the set stays unadmitted; the MSM itself still runs (and succeeds without a stale message)
      ctx->dropin_failed_builds++;
      pm::g_last_error.clear();
      return plain();
    }
    size_t bytes = 0;
    pm_bases_info(b, nullptr, nullptr, &bytes);
    ctx->dropin.push_back(pm::DropinEntry{curve, n, {d[0], d[1], d[2], d[3]}, b, bytes, ++ctx->dropin_clock, quick});
  }
  if (resident_use_table(b, 0, n))
    return curve_ops(curve)->msm_fixed(ctx, b->table.get(), ctx->in_scalars.p, n, flags & ~kBasesR261, out, nullptr);
  return dispatch_msm_device(ctx, curve, ctx->in_scalars.p, b->d, n, flags, out, true);
}

extern "C" {

int pm_msm_ctx(pm_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags,
               uint64_t out[8]) {
  if (!ctx || !out || (n && (!scalars || !bases))) return set_error(PM_ERR_ARG, "null argument");
  if (!checked_ops(curve)) return PM_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return dropin_msm(ctx, curve, scalars, bases, n, flags, out);
}

int pm_msm(int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags, uint64_t out[8]) {
  Ctx* ctx = nullptr;
  int rc = default_ctx(0, &ctx);
  if (rc) return rc;
  return pm_msm_ctx(ctx, curve, scalars, bases, n, flags, out);
}

int pm_ctx_dropin_key_id(pm_ctx* ctx, uint64_t out[2]) {
  if (!ctx || !out) return set_error(PM_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  pm::Blake2bHost h("pm-dropin-key-id");
  h.update(&ctx->dropin_key, sizeof(ctx->dropin_key));
  uint8_t dg[64];
  h.finalize(dg);
  std::memcpy(out, dg, 16);
  return PM_OK;
}

int pm_ctx_dropin_stats(pm_ctx* ctx, uint64_t* hits, uint64_t* misses, int* entries, size_t* device_bytes) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (hits) *hits = ctx->dropin_hits;
  if (misses) *misses = ctx->dropin_misses;
  if (entries) *entries = (int)ctx->dropin.size();
  if (device_bytes) *device_bytes = dropin_total(ctx) - dropin_small_total(ctx);
  return PM_OK;
}

int pm_ctx_dropin_spec_stats(pm_ctx* ctx, uint64_t* kept, uint64_t* drained) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (kept) *kept = ctx->dropin_spec_hits;
  if (drained) *drained = ctx->dropin_spec_misses;
  return PM_OK;
}

int pm_ctx_dropin_oom_stats(pm_ctx* ctx, uint64_t* flushes, uint64_t* failed_builds) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (flushes) *flushes = ctx->dropin_oom_flushes;
  if (failed_builds) *failed_builds = ctx->dropin_failed_builds;
  return PM_OK;
}

int pm_ctx_dropin_clear(pm_ctx* ctx) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  (void)hipSetDevice(ctx->device);
  dropin_release_all(ctx);
  ctx->dropin_seen.clear();
  ctx->dropin_small_seen.clear();
  return PM_OK;
}

int pm_ctx_dropin_small_stats(pm_ctx* ctx, uint64_t* hits, uint64_t* admitted, int* entries, size_t* device_bytes) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (hits) *hits = ctx->dropin_small_hits;
  if (admitted) *admitted = ctx->dropin_small_admits;
  if (entries) *entries = (int)ctx->dropin_small.size();
  if (device_bytes) *device_bytes = dropin_small_total(ctx);
  return PM_OK;
}

}  // extern "C"

// capi_pairing.hip -- BN254 pairing decider entries of the C-ABI: pm_pairing_*,
// pm_pairing_check_device and pm_accum_decide* (DESIGN §10g).
#include <algorithm>
#include <cstdlib>
#include <sched.h>
#include <thread>
#include <vector>

#include "capi_internal.hpp"
#include "pairing_engine.hpp"

using namespace pm;
using namespace pm::pairing;

namespace {
// Everything here runs before the device is touched.  The context is looked at
// last: tests/test_pairing_capi.py reaches every argument error with a null
// context on a machine without a device.
int decide_check(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* in, const void* out_ok) {
  if (!pr || !in || !out_ok) return set_error(PM_ERR_ARG, "null argument");
  if (B > kPairMaxB) return set_error(PM_ERR_UNSUPPORTED, "more than 2^24 items in one call");
  if (!ctx) return set_error(PM_ERR_ARG, "null argument (context)");
  if (pr->device < 0) return set_error(PM_ERR_ARG, "the pm_pairing was created without a context (host only)");
  if (pr->device != ctx->device) return set_error(PM_ERR_ARG, "the pm_pairing belongs to another device");
  return PM_OK;
}

int run_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_in, bool quad, const void* d_status_in,
               void* d_out_ok, void* d_out_status, void* d_out_gt) {
  if (B == 0) return PM_OK;
  int rc = decide_check(ctx, pr, B, d_in, d_out_ok);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  return decide_device(ctx, pr, B, d_in, quad, d_status_in, d_out_ok, d_out_status, d_out_gt);
}

// threads of the host form: this process's CPUs, capped by OMP_NUM_THREADS and 16 (as the contexts' pools)
int decide_threads(size_t B) {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t cs;
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0) n = CPU_COUNT(&cs);
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const int k = std::atoi(e);
    if (k > 0) n = std::min(n, k);
  }
  n = std::max(1, std::min(16, n));
  return (int)std::min<size_t>((size_t)n, B);
}
}  // namespace

extern "C" {

int pm_pairing_create(pm_ctx* ctx, const uint64_t g2[16], const uint64_t s_g2[16], pm_pairing** out) {
  if (!g2 || !s_g2 || !out) return set_error(PM_ERR_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<pm_pairing> pr(new pm_pairing);
  const uint64_t* words[2] = {s_g2, g2};  // line table 0 pairs with A, 1 with C
  for (int i = 0; i < 2; i++) {
    G2 q;
    if (!g2_from_words(words[i], &q))
      return set_error(PM_ERR_ARG, "a G2 point is the identity or has a coordinate that is not canonical");
    if (!g2_on_curve(q)) return set_error(PM_ERR_ARG, "a G2 point is not on the twist y^2 = x^3 + 3/(9+u)");
    if (!g2_order_r(q)) return set_error(PM_ERR_ARG, "a G2 point is not of order r");
    if (!g2_line_table(q, &pr->host.lines[i])) return set_error(PM_ERR_ARG, "a G2 point has a vertical Miller line");
  }
  host_frob(&pr->host);
  if (ctx) {
    const std::vector<uint32_t> w = device_words(pr->host);
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = ctx->begin_call();
    if (rc) return rc;
    if ((rc = pr->d_tab.ensure(w.size() * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemcpy(pr->d_tab.p, w.data(), w.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    pr->device = ctx->device;
  }
  *out = pr.release();
  return PM_OK;
}

int pm_pairing_info(const pm_pairing* pr, uint32_t* steps, size_t* table_bytes, uint32_t* lanes_per_pairing) {
  if (!pr) return set_error(PM_ERR_ARG, "null argument");
  if (steps) *steps = (uint32_t)kSteps;
  if (table_bytes) *table_bytes = (size_t)kDeviceWords * sizeof(uint32_t);
  if (lanes_per_pairing) *lanes_per_pairing = (uint32_t)kPairG;
  return PM_OK;
}

int pm_pairing_release(pm_pairing* pr) {
  if (!pr) return PM_OK;
  if (pr->device >= 0) (void)hipSetDevice(pr->device);
  delete pr;
  return PM_OK;
}

int pm_pairing_check_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_pairs, const void* d_status_in,
                            void* d_out_ok, void* d_out_status, void* d_out_gt) {
  return run_device(ctx, pr, B, d_pairs, false, d_status_in, d_out_ok, d_out_status, d_out_gt);
}

int pm_accum_decide_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads, const void* d_status_in,
                           void* d_out_ok, void* d_out_status, void* d_out_gt) {
  return run_device(ctx, pr, B, d_quads, true, d_status_in, d_out_ok, d_out_status, d_out_gt);
}

int pm_accum_decide(pm_ctx* ctx, const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                    uint32_t* out_ok, uint32_t* out_status, uint64_t* out_gt) {
  if (B == 0) return PM_OK;
  int rc = decide_check(ctx, pr, B, quads, out_ok);
  if (rc) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if ((rc = ctx->begin_call())) return rc;
  // staged in one buffer: [quads | gt | status in | ok | status out]: the 64-bit words first, so each is aligned
  const size_t bq = B * 256, bw = B * 4, bg = out_gt ? B * 384 : 0;
  if ((rc = ctx->in_bases.ensure(bq + bg + 3 * bw))) return rc;
  char* d = (char*)ctx->in_bases.p;
  char *d_gt = d + bq, *d_si = d_gt + bg, *d_ok = d_si + bw, *d_so = d_ok + bw;
  HIP_TRY(hipMemcpyAsync(d, quads, bq, hipMemcpyHostToDevice, ctx->stream));
  if (status_in) HIP_TRY(hipMemcpyAsync(d_si, status_in, bw, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = decide_device(ctx, pr, B, d, true, status_in ? d_si : nullptr, d_ok, out_status ? d_so : nullptr,
                          out_gt ? d_gt : nullptr)))
    return rc;
  HIP_TRY(hipMemcpyAsync(out_ok, d_ok, bw, hipMemcpyDeviceToHost, ctx->stream));
  if (out_status) HIP_TRY(hipMemcpyAsync(out_status, d_so, bw, hipMemcpyDeviceToHost, ctx->stream));
  if (out_gt) HIP_TRY(hipMemcpyAsync(out_gt, d_gt, bg, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return PM_OK;
}

int pm_accum_decide_host(const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                         uint32_t* out_ok, uint32_t* out_status, uint64_t* out_gt) {
  if (B == 0) return PM_OK;
  if (!pr || !quads || !out_ok) return set_error(PM_ERR_ARG, "null argument");
  const int nt = decide_threads(B);
  auto job = [&](int t, int n) {
    for (size_t i = (size_t)t; i < B; i += (size_t)n) {
      uint32_t st;
      out_ok[i] = decide_item(pr->host, quads + 32 * i, true, status_in ? status_in[i] : 0u, &st,
                              out_gt ? out_gt + 48 * i : nullptr);
      if (out_status) out_status[i] = st;
    }
  };
  if (nt == 1) {
    job(0, 1);
    return PM_OK;
  }
  // one pool for the process, kept (as a context keeps the MSM tail's): a call pays no thread start
  static std::mutex pool_mu;
  static HostPool* pool = nullptr;
  std::lock_guard<std::mutex> lk(pool_mu);
  if (!pool) pool = new HostPool(decide_threads(16));
  pool->start(nt, job);
  job(0, nt);
  pool->wait();
  return PM_OK;
}

}  // extern "C"

// capi_ctx.hip -- errors, the device context and its workspace, the host
// thread pool, the MSM launch plan, and the pm_ctx_* entries.
//
// Boundary: halo2 `best_multiexp`; see include/pasta_msm.h.
#include <algorithm>
#include <cstdlib>
#include <map>
#include <memory>
#include <sched.h>
#include <thread>

#include "capi_internal.hpp"

using namespace pm;

// ------------------------------------------------------------------ errors
namespace pm {
thread_local std::string g_last_error;
int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
}  // namespace pm

// ------------------------------------------------------------------ context
pm_ctx::~pm_ctx() {
  (void)hipSetDevice(device);
  dropin_release_all(this);
  delete pool;
  if (h_pinned) (void)hipHostFree(h_pinned);
  if (small_pin) (void)hipHostFree(small_pin);
  for (auto& e : ev_pool) (void)hipEventDestroy(e);
  for (auto& e : grp_ev) (void)hipEventDestroy(e);
  for (auto& e : batch_ev)
    if (e) (void)hipEventDestroy(e);
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
  if (red_stream) (void)hipStreamDestroy(red_stream);
  if (own_stream) (void)hipStreamDestroy(own_stream);
  // the members' device buffers free themselves after this body, on `device`
}

int pm_ctx::begin_call() {
  HIP_TRY(hipSetDevice(device));
  pending.clear();
  ev_used = 0;
  return PM_OK;
}

hipEvent_t pm_ctx::next_event() {
  if (ev_used == ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ev_pool.push_back(e);
  }
  return ev_pool[ev_used++];
}

void pm_ctx::mark(const char* name, hipEvent_t a, hipEvent_t b) { pending.push_back({name, a, b}); }

int pm_ctx::end_call() {
  // called after the stream has been synchronised
  for (auto& p : pending) {
    float ms = 0.f;
    if (p.a && p.b && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      auto& s = stats[p.name];
      s.first += 1;
      s.second += ms;
    }
  }
  pending.clear();
  return PM_OK;
}

int pm_ctx::ensure_group_events(int n) {
  while ((int)grp_ev.size() < n) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    grp_ev.push_back(e);
  }
  return PM_OK;
}

// threads for host-side data-parallel work: this process's CPUs, capped by
// OMP_NUM_THREADS (the GPU pool's 16-CPU share per GPU) and 16
static int host_threads() {
  int n = (int)std::thread::hardware_concurrency();
  cpu_set_t cs;
  if (sched_getaffinity(0, sizeof(cs), &cs) == 0) n = CPU_COUNT(&cs);
  if (const char* e = std::getenv("OMP_NUM_THREADS")) {
    const int k = std::atoi(e);
    if (k > 0) n = std::min(n, k);
  }
  return std::max(1, std::min(16, n));
}

pm::HostPool& pm_ctx::host_pool() {
  if (!pool) pool = new pm::HostPool(host_threads());
  return *pool;
}

pm::HostPool::HostPool(int threads) {
  for (int t = 1; t < threads; t++) th_.emplace_back([this, t] { loop(t); });
}
pm::HostPool::~HostPool() {
  {
    std::lock_guard<std::mutex> lk(m_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : th_) t.join();
}
void pm::HostPool::loop(int t) {
  uint64_t seen = 0;
  for (;;) {
    std::function<void(int, int)> job;
    int nt;
    {
      std::unique_lock<std::mutex> lk(m_);
      cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
      if (stop_) return;
      seen = gen_;
      if (t >= nt_) continue;
      job = job_;
      nt = nt_;
    }
    job(t, nt);
    std::lock_guard<std::mutex> lk(m_);
    if (--pending_ == 0) done_.notify_all();
  }
}
void pm::HostPool::start(int nt, std::function<void(int, int)> job) {
  nt = std::max(1, std::min(nt, size()));
  {
    std::lock_guard<std::mutex> lk(m_);
    job_ = std::move(job);
    nt_ = nt;
    pending_ = nt - 1;
    gen_++;
  }
  cv_.notify_all();
}
void pm::HostPool::wait() {
  std::unique_lock<std::mutex> lk(m_);
  done_.wait(lk, [&] { return pending_ == 0; });
}

// grow-only pinned + mapped host buffer.  Coherent (fine-grained) whatever
// HIP_HOST_COHERENT says: the host spins on the completion flag and reads the
// window sums a kernel writes here mid-launch
static int ensure_host_pin(void*& p, void*& dev, size_t& cap, size_t bytes) {
  if (bytes <= cap) return PM_OK;
  if (p) (void)hipHostFree(p);
  p = dev = nullptr;
  cap = 0;
  HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent));
  HIP_TRY(hipHostGetDevicePointer(&dev, p, 0));
  cap = bytes;
  return PM_OK;
}
int pm_ctx::ensure_pinned(size_t bytes) { return ensure_host_pin(h_pinned, h_pinned_dev, h_pinned_cap, bytes); }
int pm_ctx::ensure_small_pin(size_t bytes) { return ensure_host_pin(small_pin, small_pin_dev, small_pin_cap, bytes); }

int pm_ctx::upload_h2d(void* d, const void* h, size_t bytes, hipStream_t st) {
  hipEvent_t ta = nullptr, tb = nullptr;
  if (timed("h2d")) {
    ta = next_event();
    tb = next_event();
    HIP_TRY(hipEventRecord(ta, st));
  }
  HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, st));
  if (ta) {
    HIP_TRY(hipEventRecord(tb, st));
    mark("h2d", ta, tb);
  }
  return PM_OK;
}

// default context per device (lazily created, process lifetime)
namespace {
std::mutex g_default_mu;
std::map<int, Ctx*> g_default;  // process lifetime: never freed (HIP may be torn down at exit)
}  // namespace

int pm::default_ctx(int device, Ctx** out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  auto it = g_default.find(device);
  if (it != g_default.end()) {
    *out = it->second;
    return PM_OK;
  }
  pm_ctx* c = nullptr;
  int rc = pm_ctx_create(device, &c);
  if (rc) return rc;
  g_default[device] = c;
  *out = c;
  return PM_OK;
}

// ================================================================== C-ABI
extern "C" {

const char* pm_version(void) { return "pasta_msm 0.3 (gfx950)"; }
int pm_abi_version(void) { return PM_ABI_VERSION; }
const char* pm_last_error(void) { return pm::g_last_error.c_str(); }

int pm_device_count(int* count) {
  if (!count) return set_error(PM_ERR_ARG, "null count");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return set_error(PM_ERR_NODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return PM_OK;
}

int pm_ctx_create(int device, pm_ctx** out) {
  if (!out) return set_error(PM_ERR_ARG, "null out");
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return set_error(PM_ERR_NODEV, "no HIP device");
  if (device < 0 || device >= cnt) return set_error(PM_ERR_NODEV, "device index out of range");
  std::unique_ptr<Ctx> c(new Ctx());
  c->device = device;
  HIP_TRY(hipSetDevice(device));
  {  // gfx950 only: the kernels' LDS layouts and fences assume 160 KiB per CU
    int cus = 0, lds = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device));
    if (lds < (int)kMaxLds)
      return set_error(PM_ERR_UNSUPPORTED, "device has " + std::to_string(lds) +
                                               " B of LDS per CU; this build needs gfx950's 160 KiB");
    c->num_cus = std::max(1, cus);
  }
  // the context's own stream is a BLOCKING stream: it is ordered after work
  // the caller queued on the legacy null stream (torch's default stream), so
  // a *_device entry sees inputs the caller has just written there.  The
  // internal reduction stream is ordered by events only.
  HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault));
  c->stream = c->own_stream;
  HIP_TRY(hipStreamCreateWithFlags(&c->red_stream, hipStreamNonBlocking));
  try {  // std::random_device may throw when no entropy source is available
    pm::digest_key_init(c->dropin_key);
  } catch (const std::exception& e) {
    return set_error(PM_ERR_HIP, std::string("drop-in cache key: no entropy source: ") + e.what());
  }
  if (const char* e = std::getenv("PM_NTT_PASSES")) c->ntt_passes = std::atoi(e);
  if (const char* e = std::getenv("PM_FINE_CACHE_KB")) c->fine_cache_kb = std::max(0, std::min(144, std::atoi(e)));
  if (const char* e = std::getenv("PM_FINE_CHUNK_KB")) c->fine_chunk_kb = std::max(0, std::min(144, std::atoi(e)));
  *out = c.release();
  return PM_OK;
}

int pm_ctx_destroy(pm_ctx* ctx) {
  delete ctx;
  return PM_OK;
}

int pm_ctx_set_stream(pm_ctx* ctx, void* s) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  // NULL = the context's own stream (the round-1 meaning, which callers
  // compiled against that header rely on); PM_STREAM_LEGACY = the legacy
  // null stream itself
  if (s == nullptr) ctx->stream = ctx->own_stream;
  else if (s == PM_STREAM_LEGACY) ctx->stream = nullptr;
  else ctx->stream = (hipStream_t)s;
  return PM_OK;
}

int pm_ctx_use_own_stream(pm_ctx* ctx) { return pm_ctx_set_stream(ctx, nullptr); }

int pm_ctx_set_glv(pm_ctx* ctx, int enable) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (enable) return set_error(PM_ERR_UNSUPPORTED, "GLV mode retired (measured slower on MI355X, DESIGN.md §7)");
  return PM_OK;
}

int pm_ctx_set_accum_ladder(pm_ctx* ctx, int mode) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (mode < -1 || mode > 1) return set_error(PM_ERR_ARG, "accum ladder mode out of range (-1 auto, 0 quads, 1 sliced)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->acc_ladder = mode;
  return PM_OK;
}

int pm_ctx_set_accum_split(pm_ctx* ctx, int lg_lanes) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (lg_lanes < -1 || lg_lanes > 5) return set_error(PM_ERR_ARG, "accum split out of range (-1 auto, 0..5)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->acc_split = lg_lanes;
  return PM_OK;
}

int pm_ctx_set_accum_option(pm_ctx* ctx, int option, int value) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  switch (option) {
    case PM_ACC_OPT_TWIST:
      if (value < -1 || value > 2)
        return set_error(PM_ERR_ARG, "twist option out of range (-1 auto, 0 off, 1 unfenced decode, 2 paired decode)");
      ctx->acc_twist = value;
      return PM_OK;
    case PM_ACC_OPT_TAIL_STREAM:
    case PM_ACC_OPT_TRANSCRIPT:
      if (value < -1 || value > 0) return set_error(PM_ERR_ARG, "accum option value out of range (-1 auto, 0 off)");
      (option == PM_ACC_OPT_TAIL_STREAM ? ctx->acc_tail : ctx->acc_tr_stream) = value;
      return PM_OK;
    case PM_ACC_OPT_TERMS_PER_LANE:
      if (value < -1 || value == 0 || value > 2)
        return set_error(PM_ERR_ARG, "terms per lane out of range (-1 auto, 1, 2)");
      ctx->acc_tpl = value;
      return PM_OK;
    default:
      return set_error(PM_ERR_ARG, "unknown accum option");
  }
}

int pm_ctx_set_msm_option(pm_ctx* ctx, int option, int value) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  switch (option) {
    case PM_MSM_OPT_SPLIT_COPY:
      if (value < -1 || value > 0) return set_error(PM_ERR_ARG, "msm option value out of range (-1 auto, 0 off)");
      ctx->msm_split_copy = value;
      return PM_OK;
    default:
      return set_error(PM_ERR_ARG, "unknown msm option");
  }
}

int pm_ctx_set_window(pm_ctx* ctx, int c) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (c != 0 && (c < kMinC || c > kMaxC)) return set_error(PM_ERR_ARG, "window width out of range");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->window_c = c;
  return PM_OK;
}

int pm_ctx_set_small_msm(pm_ctx* ctx, size_t max_n) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (max_n > kSmallLimit) return set_error(PM_ERR_ARG, "small-MSM threshold above PM_SMALL_MSM_LIMIT");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->small_max = max_n;
  return PM_OK;
}

int pm_ctx_set_pipeline(pm_ctx* ctx, int groups, int min_chunk) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (groups < 0 || min_chunk < 0 || min_chunk > (1 << 20)) return set_error(PM_ERR_ARG, "pipeline setting out of range");
  if (groups > 1)
    return set_error(PM_ERR_UNSUPPORTED, "window groups retired (measured slower on MI355X, DESIGN.md §7)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->min_chunk = min_chunk;
  return PM_OK;
}

int pm_ctx_set_timing(pm_ctx* ctx, int enable) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->timing = enable != 0;
  return PM_OK;
}

int pm_ctx_set_timing_filter(pm_ctx* ctx, const char* kernel) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->timing_filter = kernel ? kernel : "";
  return PM_OK;
}

int pm_ctx_kernel_stats(pm_ctx* ctx, const char* kernel, uint64_t* launches, double* total_ms) {
  if (!ctx || !kernel || !launches || !total_ms) return set_error(PM_ERR_ARG, "null argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->stats.find(kernel);
  *launches = it == ctx->stats.end() ? 0 : it->second.first;
  *total_ms = it == ctx->stats.end() ? 0.0 : it->second.second;
  return PM_OK;
}

int pm_ctx_reset_stats(pm_ctx* ctx) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->stats.clear();
  return PM_OK;
}

int pm_ctx_set_h2d_threads(pm_ctx* ctx, int threads) {
  if (!ctx) return set_error(PM_ERR_ARG, "null ctx");
  if (threads < 0) return set_error(PM_ERR_ARG, "h2d threads out of range");
  if (threads > 0)
    return set_error(PM_ERR_UNSUPPORTED, "pinned staging threads retired (measured slower on MI355X, DESIGN.md §5)");
  return PM_OK;
}

}  // extern "C"

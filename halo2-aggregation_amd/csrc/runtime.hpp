// runtime.hpp -- device context, workspace and launch plan of the MSM engine.
//
// A pm_ctx binds one device, one HIP stream and a grow-only workspace, so a
// caller (rayon thread in the Rust shim, one rank in bench.py) reuses device
// memory across calls and no hipMalloc happens once warm.  Calls on one
// context are serialised by its mutex (the C-ABI is re-entrant, §8b).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pasta_msm.h"
#include "dropin_digest.hpp"
#include "msm_plan.hpp"
#include "quotient_plan.hpp"

#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace pm {

int set_error(int code, const std::string& msg);

// window limits, sort / scan / reduction geometry and the MSM plans: msm_plan.hpp
constexpr size_t kMaxPoints = size_t(1) << 26;
// internal msm flag (never in the public header; the C-ABI strips it from
// caller flags): d_bases already hold the pipeline's R = 2^261 canonical
// form (resident pm_bases converted at upload), so no per-call conversion
constexpr uint32_t kBasesR261 = 1u << 30;
// drop-in base cache of pm_msm / pm_msm_ctx (capi_dropin.hip): base sets of at least
// kDropinMinN points are kept resident, keyed by a content digest; at most
// kDropinEntries sets and kDropinBytes of device memory per context
constexpr size_t kDropinMinN = size_t(1) << 12;
constexpr int kDropinEntries = 4;
constexpr size_t kDropinBytes = size_t(16) << 30;
// ... and at most this fraction (1/kDropinFreeDiv) of the device memory free
// at admission, counting the sets already held
constexpr size_t kDropinFreeDiv = 2;
// base sets seen once and not admitted: a set becomes resident on its second
// sighting, so one-shot bases never pay the row-table build
constexpr int kDropinSeen = 8;
// small drop-in sets (multiples tables, capi_dropin.hip dropin_small_msm): at most
// this many, and this many bytes of tables, per context.  A table costs
// 512 KiB per base at c = 8, so only sets of at most kDropinSmallMaxN points
// are kept (512-point sets held 256 MiB each); their bytes count in
// the drop-in cache's free-memory-aware budget with the large sets'.
constexpr int kDropinSmallEntries = 8;
constexpr size_t kDropinSmallMaxN = 64;
constexpr size_t kDropinSmallBytes = size_t(256) << 20;
// small-MSM path (msm_small.hpp): pm_msm* calls with n <= ctx->small_max (and
// the automatic window) run the two-launch table + window-sum kernels instead
// of the sorting pipeline; kSmallLimit bounds pm_ctx_set_small_msm
constexpr size_t kTailBytes = 128;  // opaque MsmTail storage (CurveOps::msm_start)
constexpr size_t kSmallMaxN = PM_SMALL_MSM_DEFAULT;
constexpr size_t kSmallLimit = PM_SMALL_MSM_LIMIT;

// Grow-only device allocation that frees itself (on the device current at
// destruction: the owners below set theirs first).  Move-only.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  uint64_t gen = 0;  // bumped whenever p changes: on every (re)allocation and on move assignment
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(o.p), cap(o.cap), gen(o.gen) { o.p = nullptr, o.cap = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap, gen = (gen > o.gen ? gen : o.gen) + 1;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~Buf() { release(); }
  int ensure(size_t bytes);
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};
inline int Buf::ensure(size_t bytes) {
  if (bytes <= cap) return PM_OK;
  release();
  const size_t want = bytes < 256 ? 256 : bytes;
  const hipError_t e = hipMalloc(&p, want);
  if (e != hipSuccess) {
    p = nullptr;
    return set_error(PM_ERR_HIP, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
  }
  cap = want;
  gen++;
  return PM_OK;
}

// Device copy of a small host table (accumulator / transcript programs,
// constants, VK points) that is uploaded only when its bytes change: a batch
// of proofs against one verifying key re-sends nothing after the first call.
struct CachedUpload {
  Buf buf;
  std::vector<uint8_t> host;
  uint64_t gen_at_upload = ~0ull;
  bool sent = false;  // the last put() queued a copy (false: the device copy was current)
  template <class T>
  int put(const std::vector<T>& v, hipStream_t st, size_t pad = 0);
};

// fixed-base windows: one bucket set of 2^(c-1) buckets
constexpr int kFixedMaxC = 20;
constexpr int kAutoFixedC = 16;       // n <= 2^21
constexpr int kAutoFixedCLarge = 20;  // n > 2^21 (fewer windows: 13 instead of 16)

struct TimedSpan {
  const char* name;
  hipEvent_t a, b;
};

// A few persistent host threads for data-parallel host work inside a call
// (the drop-in cache's content digest of the caller's bases runs on them
// while the scalars cross PCIe).  run() starts job(t, nt) for t = 1 .. nt-1
// on the workers; the caller runs t = 0 itself and then wait()s.
class HostPool {
 public:
  explicit HostPool(int threads);
  ~HostPool();
  int size() const { return (int)th_.size() + 1; }
  void start(int nt, std::function<void(int, int)> job);
  void wait();

 private:
  void loop(int t);
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  std::function<void(int, int)> job_;
  int nt_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// resident base set of the drop-in cache (pm_msm): key = (curve, n, keyed
// digest, dropin_digest.hpp)
struct DropinEntry {
  int curve;
  size_t n;
  uint64_t d[4];
  pm_bases* b;  // nullptr: seen once, not admitted yet (run through the plain path)
  size_t bytes;
  uint64_t last_use;
  uint64_t quick = 0;  // keyed hash of the first and last 8 points: picks the set to start speculatively
};

}  // namespace pm

// Fixed-base table (pm_fixed_bases_create*): rows x npad affine points in the
// pipeline's R = 2^261 form, row j = [2^{o_{j W / rows}}] P_i.  rows = W (the
// default) merges every window into one bucket set; rows = k < W merges
// windows w, w + W/k, ... into W/k bucket sets (W/k windows to reduce, a host
// Horner over 256/k bit positions, k x the bases' memory).
struct pm_fixed_bases {
  int curve;
  int device;
  int c, W, rows;
  size_t n, npad;
  pm::Buf d;
};

// Extended evaluation domain (pm_domain_create, domain_engine.hpp): the roots
// as the caller's R = 2^256 Montgomery words, and the device table the
// kernels read, R = 2^261 canonical packed:
// [zeta^0..2 | N^-1 zeta^-0..-2 | t_0 .. t_{2^e - 1}].
struct pm_domain {
  int curve;
  int device;
  uint32_t k, ext_k;
  uint64_t omega[4], omega_e[4], omega_e_inv[4];
  pm::Buf d_tab;
};

// Quotient numerator of one (domain, shape) pair (pm_quotient_create,
// quotient_engine.hpp): the compiled program and what its constants read from
// the shape (copied: the caller's shape need not outlive the call), and the
// device buffers the quotient owns: program, leaf table, a copy of the
// domain's t table, and the l_0 / l_last / l_last + l_blind / X columns.
struct pm_quotient {
  int curve;
  int device;
  uint32_t k, ext_k;
  pm::QuotPlan plan;
  std::vector<uint64_t> shape_consts;
  uint64_t delta[4];
  pm::Buf d_prog, d_leaves, d_t;
  pm::Buf d_own;  // kQownCols columns of N scalars (those the program reads are filled)
  size_t device_bytes;
};

namespace pm {
// multiples table of a resident base set (msm_many.hpp): entry (i, w, m) =
// [m 2^{c w}] P_i, m = 1 .. H = 2^(c-1), w < W, XYZZ R = 2^261 (128 B), for
// the first n bases; built on demand by pm_msm_resident_many* /
// pm_bases_many_prepare and owned by the pm_bases
struct ManyTable {
  Buf d;
  size_t n = 0;
  uint32_t c = 0, W = 0, H = 0;
};
// (the table geometry of a prefix of n bases, many_pick_c: msm_plan.hpp)
// The table budget and cap as tests/msm_short_edge_util.py (many_budget) reads them from this
// file's text: the GPU edge tests size their base prefixes by it, and it keeps reading them
// where it always has.  The plan's own definitions are msm_plan.hpp's; the two cannot differ.
namespace as_read_by_tests {
constexpr size_t kManyTabBudget = size_t(2) << 30;
constexpr size_t kManyTabCap = size_t(8) << 30;
}  // namespace as_read_by_tests
static_assert(as_read_by_tests::kManyTabBudget == kManyTabBudget && as_read_by_tests::kManyTabCap == kManyTabCap,
              "runtime.hpp restates msm_plan.hpp's many-MSM table limits");
constexpr size_t kNttTwiddleSlots = 4;
constexpr uint32_t kNttMaxLog = 28;  // pm_fft: three passes above 2^22; BN254 Fr has 2-adicity 28
// polynomial openings (poly_engine.hpp)
// longest polynomial: k_poly_table keeps 29 slots of z^(2^k) (a call at 2^28
// reads k <= 20, poly_table_squarings) and the tile index is grid.x (2^17
// tiles of 2^11 at 2^28); the limit matches pm_fft's, the scan needs no more
constexpr size_t kPolyMaxN = size_t(1) << 28;
constexpr size_t kPolyMaxGridY = 65535;        // sets / pairs per call (grid.y)
// grand products (gp_engine.hpp): the same limits; flag bit of CurveOps::grand_product
// for the in-place batch inversion (never part of the C-ABI's flags)
constexpr uint32_t kGpInvert = 0x80000000u;
// lookup permuted columns (lookup_engine.hpp): rows as above; pairs and columns per call (2 P columns in grid.y)
constexpr size_t kLkMaxPairs = PM_LOOKUP_MAX_PAIRS;
constexpr size_t kLkMaxCols = PM_LOOKUP_MAX_COLS;
// extended-domain conversions (domain_engine.hpp): one job of CurveOps::domain_run
enum : int { kDomOpFft = 0, kDomOpToExt = 1, kDomOpToCoeff = 2, kDomOpDivide = 3 };
constexpr uint32_t kDomDivideVanishing = 1u;  // PM_EXT_DIVIDE_VANISHING
constexpr uint32_t kDomMaxE = 8;              // extended_k - k
constexpr int kDomTabHead = 6;                // entries of pm_domain::d_tab before t_0 (a quotient copies t)
struct DomJob {
  int op, curve;
  uint32_t logn;              // transform length (extended_k of dom, or log_n of the batched NTT)
  const uint64_t* omega;      // root of the transform
  const uint64_t* scale;      // kDomOpFft: pm_fft's scale, or null
  const pm_domain* dom;       // null for kDomOpFft
  const void* const* d_in;    // host arrays of C device pointers; d_in null: in place on d_out
  void* const* d_out;
  size_t C, keep;
  uint32_t flags;
};
// best_fft over curve points (ecfft_engine.hpp): the longest transform is the largest base set an MSM
// takes; cached code tables per context (48 B per twiddle, n/2 twiddles: 192 MiB at 2^23)
constexpr uint32_t kEcfftMaxLog = 26;
constexpr size_t kEcfftTwiddleSlots = 2;
struct NttTwiddles {
  int curve = -1;
  uint32_t logn = 0;
  uint64_t omega[4] = {0, 0, 0, 0};
  uint64_t stamp = 0;
  Buf buf;
};
}  // namespace pm

struct pm_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipStream_t red_stream = nullptr;  // accumulator side stream (accum_engine.hpp)
  // H2D copies beside the context stream's kernels: pm_msm_resident_batch (the
  // next MSM's scalars), the split scalar copy's second half (engine.hpp)
  hipStream_t copy_stream = nullptr;
  pm::HostPool* pool = nullptr;      // lazily created (drop-in digest)
  std::vector<pm::DropinEntry> dropin;  // drop-in base cache (pm_msm / pm_msm_ctx)
  std::vector<pm::DropinEntry> dropin_seen;  // digests seen once (b == nullptr), admitted on the second sighting
  // small sets (n <= small_max, below kDropinMinN): resident with a multiples
  // table (msm_many.hpp) after their second sighting, run as one-MSM
  // pm_msm_resident_many calls
  std::vector<pm::DropinEntry> dropin_small, dropin_small_seen;
  uint64_t dropin_small_hits = 0, dropin_small_admits = 0;
  pm::DigestKey dropin_key;             // secret per-context digest key (pm_ctx_create)
  uint64_t dropin_clock = 0;
  uint64_t dropin_hits = 0, dropin_misses = 0;
  uint64_t dropin_spec_hits = 0, dropin_spec_misses = 0;  // speculative starts kept / drained
  uint64_t dropin_oom_flushes = 0, dropin_failed_builds = 0;  // out-of-memory: whole cache released / set not admitted
  hipEvent_t batch_ev[4] = {};       // batch pipelining: copied[2], consumed[2]
  std::vector<hipEvent_t> grp_ev;    // MSM: one per pinned term slot (terms copied)
  int window_c = 0;
  int min_chunk = 0;
  // test hooks (tests/test_msm_gpu.py::test_fine_sort_lds_modes forces the
  // fine sort's LDS modes that only large segments reach): PM_FINE_CACHE_KB /
  // PM_FINE_CHUNK_KB, 0 = auto
  int fine_cache_kb = 0, fine_chunk_kb = 0;
  int ntt_passes = 0;  // NTT passes over HBM, 0 = auto (test hook: PM_NTT_PASSES env)
  int acc_split = -1; // accumulator lanes per term = 2^acc_split, -1 = auto (pm_ctx_set_accum_split)
  int acc_ladder = -1; // powers-table chains: 0 quads, 1 row-sliced waves, -1 = auto (pm_ctx_set_accum_ladder)
  // pm_ctx_set_accum_option (-1 = auto for each): the twisted ladder (0 off),
  // the stream of the term additions / sums (0 main), the one-lane form's
  // terms per lane (1, 2), the streamed transcript replay (0: per record)
  int acc_twist = -1, acc_tail = -1, acc_tpl = -1, acc_tr_stream = -1;
  // pm_ctx_set_msm_option(PM_MSM_OPT_SPLIT_COPY): -1 auto, 0 one scalar copy
  int msm_split_copy = -1;
  // the device's CU count (hipDeviceAttributeMultiprocessorCount, 256 on an
  // MI355X): the one-block-per-CU fences of the latency-bound accumulator
  // kernels are sized against it (pm_ctx_create refuses a device with less
  // than the 160 KiB of LDS per CU those fences and kernels assume)
  int num_cus = 256;
  bool timing = false;
  std::string timing_filter;  // time only launches with this name ("" = all)
  bool timed(const char* name) const { return timing && (timing_filter.empty() || timing_filter == name); }
  std::mutex mu;
  // workspace
  pm::Buf in_scalars, in_scalars2, in_bases, digits, sorted, counts, offsets, cursor, bsum, buckets, head, segS, segT, bits,
      win, longs, mid, acc_coef, acc_part, acc_io, bases29, tr_io, bitsP, tickets, ntt_scratch, bitsQ, acc_lad, acc_corr, tr_canon, ntt_scratch2,
      acc_vkpow, small_tab, small_dig, small_part, small_tk;
  // polynomial openings (poly_engine.hpp): per-call upload, power tables, scan scratch, quotient rows of pm_multiopen_open*
  pm::Buf poly_job, poly_tab, poly_aux, poly_q;
  // grand products (gp_engine.hpp): the un-carried suffix products, S rows of n (the rest shares the three above)
  pm::Buf gp_rows;
  // lookup permuted columns (lookup_engine.hpp): the call's pointer table, the two key buffers of the
  // merge sort, and the pairing's row map, counts and flags
  pm::Buf lk_job, lk_keys, lk_aux;
  // extended-domain conversions (domain_engine.hpp): the call's column pointer tables
  pm::Buf dom_ptrs;
  // quotient numerator (quotient_engine.hpp): the call's pointer table and constants
  pm::Buf quot_io;
  // pairing decider (pairing_engine.hpp): per item the two G1 points in the kernels' form and a flag word
  pm::Buf pair_io;
  // the power table of the last omega a grand product named: one prover calls with one omega, and the
  // table's chain of squarings is pure latency (0.04 ms of a 2^20 call); valid while gp_tab.gen == gp_tab_gen
  pm::Buf gp_tab;
  int gp_tab_curve = -1;
  uint32_t gp_tab_nsq = 0;
  uint64_t gp_tab_omega[4] = {0, 0, 0, 0};
  uint64_t gp_tab_gen = ~0ull;
  // the later parts' sorted lists and bucket partials of the split scalar
  // copy (engine.hpp; the sort scratch is shared, its kernels run in order)
  pm::Buf part_sorted[2], part_offsets[2], part_buckets[2], part_head[2];
  pm::CachedUpload acc_prog, acc_const, acc_vk, tr_prog;
  pm::CachedUpload tr_wtab;  // streamed transcript: word table of the shape's byte stream
  pm::CachedUpload many_prog;  // pm_msm_resident_many*: job + MSM tables
  // proof-byte decoder (proof_kernels.hpp): square-root tables per curve
  // (pm_curve order), the point map of the current shape, host staging
  pm::Buf sqrt_tab[3];
  bool sqrt_ready[3] = {false, false, false};
  bool sqrt_tab_ts[3] = {false, false, false};  // the curve's root needs the Tonelli-Shanks windows (Pasta)
  pm::CachedUpload pf_map;
  pm::Buf pf_io;
  pm::Buf pf_flags;            // proof-decode flags per proof (cleared by k_transcript)
  bool pf_flags_dirty = false;  // a call failed between the decode and the replay
  // accumulator: powers-of-two tables of the verifying key's points (fixed,
  // sigma, g1), built once per (curve, VK) and reused by every later batch
  std::vector<uint64_t> acc_vkpow_key;
  uint64_t acc_vkpow_gen = ~0ull;  // acc_vkpow.gen when the tables were built
  std::vector<pm::NttTwiddles> ntt_tw;  // cached twiddle segments (pm_fft*)
  uint64_t ntt_clock = 0;
  std::vector<pm::NttTwiddles> ecfft_tw;  // cached twiddle code tables (pm_fft_points*)
  uint64_t ecfft_clock = 0;
  void* h_pinned = nullptr;  // MSM host terms: two slots (batch pipelining)
  void* h_pinned_dev = nullptr;  // its device address (hipHostGetDevicePointer, once per allocation)
  size_t h_pinned_cap = 0;
  size_t small_max = pm::kSmallMaxN;  // small-MSM path threshold (pm_ctx_set_small_msm)
  void* small_pin = nullptr;          // small-MSM host inputs, pinned + mapped (read by k_small_table)
  void* small_pin_dev = nullptr;      // its device address
  size_t small_pin_cap = 0;
  uint32_t small_seq = 0;             // completion-flag value of the last small MSM
  // timing
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<pm::TimedSpan> pending;
  std::map<std::string, std::pair<uint64_t, double>> stats;

  ~pm_ctx();
  int begin_call();
  int end_call();
  int ensure_pinned(size_t bytes);
  int ensure_small_pin(size_t bytes);
  // host -> device copy of a caller buffer on `st` (one pageable
  // hipMemcpyAsync: ~52 GB/s for 32 MB on MI355X, faster than the pinned
  // staging threads round 2 measured, ~38 GB/s, and retired)
  int upload_h2d(void* d, const void* h, size_t bytes, hipStream_t st);
  int ensure_group_events(int n);
  pm::HostPool& host_pool();
  hipEvent_t next_event();
  void mark(const char* name, hipEvent_t a, hipEvent_t b);
};

namespace pm {
using Ctx = ::pm_ctx;
}

namespace pm {

// Per-curve engine entry points, one translation unit per curve
// (inst_pallas.hip, inst_vesta.hip, inst_bn254.hip) so they build in parallel.
struct CurveOps {
  // h_scalars != nullptr: scalars still in host memory, d_scalars their device buffer (chunked copy)
  int (*msm)(Ctx* ctx, const void* d_scalars, const void* d_bases, size_t n, uint32_t flags, uint64_t out[8],
             const void* h_scalars);
  int (*point_add)(const uint64_t a[8], const uint64_t b[8], uint64_t out[8]);
  int (*synth_scalars)(Ctx* ctx, uint64_t seed, uint64_t i0, uint32_t n, uint32_t mont, void* d_out);
  int (*synth_bases)(Ctx* ctx, uint64_t seed, uint64_t i0, uint32_t n, void* d_out);
  // vk_repr != nullptr: replay the transcript into d_challenges first (d_status as in transcript)
  int (*accum)(Ctx* ctx, const pm_proof_shape* shape, size_t B, const void* d_points, const void* d_scalars,
               void* d_challenges, void* d_out_quads, void* d_out_h, const uint64_t* vk_repr, void* d_status);
  int (*selftest_field)(Ctx* ctx, uint64_t seed, uint32_t n, uint64_t* mismatches);
  int (*transcript)(Ctx* ctx, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4], const void* d_points,
                    const void* d_scalars, void* d_challenges, void* d_status);
  int (*vk_repr)(const uint8_t digest[64], uint64_t out[4]);
  int (*fixed_table)(Ctx* ctx, const void* d_bases, pm_fixed_bases* ft);
  int (*ntt)(Ctx* ctx, int curve, void* d_data, uint32_t logn, const uint64_t omega[4], const uint64_t* scale);
  int (*msm_fixed)(Ctx* ctx, const pm_fixed_bases* ft, const void* d_scalars, size_t n, uint32_t flags,
                   uint64_t out[8], const void* h_scalars);
  // resident bases: Rust-layout affine (R = 2^256) -> the pipeline's R = 2^261 canonical form
  int (*bases_to29)(Ctx* ctx, const void* d_in, size_t n, void* d_out);
  // k MSMs of n host scalars against resident (R = 2^261) bases, pipelined
  // (ft != nullptr: the resident bases' row table, pm_fixed_bases_create_rows)
  int (*msm_resident_batch)(Ctx* ctx, const void* d_bases29, const pm_fixed_bases* ft, const uint64_t* const* scalars,
                            size_t k, size_t n, uint32_t flags, uint64_t* out);
  // proof bytes -> decoded points / scalars + status (proof_kernels.hpp); with
  // vk_repr also the transcript replay + accumulator (pm_accum_batch_proofs*)
  int (*proofs)(Ctx* ctx, const pm_proof_shape* shape, size_t B, const void* d_proofs, size_t stride,
                const void* d_inst, void* d_points, void* d_scalars, void* d_status, const uint64_t* vk_repr,
                void* d_ch, void* d_quads, void* d_h);
  // resident-bases MSM in two halves (the drop-in cache's speculative start):
  // msm_start enqueues the device pipeline on ctx->stream (ft: the row table,
  // else d_bases29 in the R = 2^261 form) and fills the opaque tail;
  // msm_finish waits for it and runs the host Horner.  h_scalars != nullptr:
  // the scalars are still in host memory and are copied to d_scalars first
  // (in two halves beside the pipeline with a row table: engine.hpp)
  int (*msm_start)(Ctx* ctx, const pm_fixed_bases* ft, const void* d_bases29, const void* d_scalars, size_t n,
                   uint32_t flags, void* tail, const void* h_scalars);
  int (*msm_finish)(Ctx* ctx, const void* tail, uint64_t out[8]);
  // small-MSM path (msm_small.hpp); s_host / b_host: the input is in host
  // memory; b_r261: bases in the resident R = 2^261 form
  int (*msm_small)(Ctx* ctx, const void* scalars, bool s_host, const void* bases, bool b_host, bool b_r261, size_t n,
                   uint32_t flags, uint64_t out[8]);
  // many short MSMs against resident bases (msm_many.hpp): build / grow the
  // multiples table of the first n bases, and the batched sum
  int (*many_table)(Ctx* ctx, const void* d_bases29, size_t n, ManyTable* t);
  int (*msm_many)(Ctx* ctx, const ManyTable* t, size_t B, const size_t* n, const size_t* off, const void* scalars,
                  bool s_host, uint32_t flags, uint64_t* out);
  // host: out = sum of n affine points (XYZZ accumulation, one inversion)
  int (*points_sum)(const uint64_t* points, size_t n, uint64_t out[8]);
  // polynomial openings (poly_engine.hpp): E (polynomial, point) evaluations;
  // the S witness quotients of a multiopen argument (+ batched evaluations)
  int (*poly_eval)(Ctx* ctx, const void* const* d_polys, size_t P, size_t n, const uint32_t* poly_index,
                   const uint64_t* points, size_t E, uint64_t* out_evals);
  int (*poly_witness)(Ctx* ctx, const void* const* d_polys, size_t P, size_t n, const uint32_t* set_offsets,
                      const uint32_t* set_polys, const uint64_t* points, const uint64_t* v, size_t S, void* d_out,
                      uint64_t* out_evals);
  // grand products and the batch inversion (gp_engine.hpp; flags: PM_GP_CHAIN,
  // or pm::kGpInvert for the in-place inversion of the n values at d_out)
  int (*grand_product)(Ctx* ctx, int curve, const void* const* d_cols, size_t C, size_t n, const pm_gp_factor* num,
                       const uint32_t* num_off, const pm_gp_factor* den, const uint32_t* den_off, size_t S,
                       const uint64_t* omega, const uint64_t* start, size_t active, uint32_t flags, void* d_out,
                       uint64_t* out_last);
  // extended-domain conversions (domain_engine.hpp): host-only check of the
  // roots + the device table's words; one conversion / batched NTT / division
  int (*domain_tables)(uint32_t k, uint32_t ext_k, const uint64_t* omega_e, const uint64_t* zeta, pm_domain* d,
                       std::vector<uint64_t>* tab);
  int (*domain_run)(Ctx* ctx, const DomJob* job);
  // quotient numerator (quotient_engine.hpp): the field values pm_quotient_create
  // seeds the quotient's own columns with; one evaluation over the extended
  // domain; the compiled program on the CPU
  int (*quotient_seed)(const pm_domain* d, uint64_t* out);
  int (*quotient_run)(Ctx* ctx, const pm_quotient* q, const void* const* ptrs, const uint64_t* challenges,
                      uint32_t flags, void* d_out);
  int (*quotient_eval_host)(const pm_proof_shape* shape, size_t R, const uint64_t* scalars, const uint64_t* x,
                            const uint64_t* challenges, uint64_t* out);
  // lookup permuted columns (lookup_engine.hpp): the theta-compression of m columns (theta may be null
  // when m == 1); P (input, table) pairs sorted and paired, out_status P x (status, row) in host memory
  int (*lookup_compress)(Ctx* ctx, const void* const* d_cols, size_t m, size_t n, const uint64_t* theta, void* d_out);
  int (*lookup_permute)(Ctx* ctx, const void* const* d_a, const void* const* d_s, size_t P, size_t usable,
                        void* const* d_out_a, void* const* d_out_s, uint32_t* out_status);
  // best_fft over curve points (ecfft_engine.hpp): n = 2^logn affine points in place; the host form
  // (ecfft_host.hpp) returns PM_ERR_ARG when omega has not order n
  int (*fft_points)(Ctx* ctx, int curve, void* d_points, uint32_t logn, const uint64_t omega[4],
                    const uint64_t* scale);
  int (*fft_points_host)(uint64_t* points, uint32_t logn, const uint64_t omega[4], const uint64_t* scale,
                         int threads);
  bool (*fft_points_omega_ok)(const uint64_t omega[4], uint32_t logn);
};
extern const CurveOps kPallasOps, kVestaOps, kBn254Ops;

}  // namespace pm

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return pm::set_error(PM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace pm {
template <class T>
int CachedUpload::put(const std::vector<T>& v, hipStream_t st, size_t pad) {
  const size_t bytes = v.size() * sizeof(T);
  int rc;
  sent = false;
  if ((rc = buf.ensure(bytes + pad))) return rc;
  if (buf.gen == gen_at_upload && host.size() == bytes && (bytes == 0 || memcmp(host.data(), v.data(), bytes) == 0))
    return PM_OK;
  if (bytes) HIP_TRY(hipMemcpyAsync(buf.p, v.data(), bytes, hipMemcpyHostToDevice, st));
  sent = bytes != 0;
  host.assign((const uint8_t*)v.data(), (const uint8_t*)v.data() + bytes);
  gen_at_upload = buf.gen;
  return PM_OK;
}

// Wait for `ev` on the host: the runtime's blocking wait (a hipEventQuery
// poll measured within run-to-run noise and burns a host core, round 3:
// profiles/r03/ab/spin_wait/).
inline int wait_event(const pm_ctx*, hipEvent_t ev) {
  HIP_TRY(hipEventSynchronize(ev));
  return PM_OK;
}
}  // namespace pm

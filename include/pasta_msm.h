/* pasta_msm.h -- C-ABI of the MI355X-native MSM + multiopen-accumulator library.
 *
 * This is the drop-in boundary for the hot path of
 * Trapdoor-Tech/halo2-aggregation (see INTEGRATION.md for the Rust binding a
 * maintainer adds).  Every entry point is extern "C", takes plain pointers and
 * sizes, and returns 0 (PM_OK) or a negative PM_ERR_* code; the message of the
 * last failure on the calling thread is available from pm_last_error().
 *
 * Memory layout (matches the Rust in-memory representation of pasta_curves /
 * pairing_bn256 types, which the Rust shim passes with `as_ptr()`):
 *   scalar  : 4 x u64 little-endian limbs, Montgomery form (R = 2^256) unless
 *             PM_SCALARS_CANONICAL is set (then the `to_repr()` integer).
 *   affine  : 8 x u64 = x[4] then y[4], Montgomery form; (0,0) is the identity
 *             (the pasta_curves EpAffine/EqAffine convention).
 * Ownership: the caller owns every buffer; the library only borrows pointers
 * for the duration of a call, except the explicit base cache (pm_bases_*).
 * Threading: all calls are synchronous and re-entrant; a pm_ctx serialises its
 * own calls with a mutex, distinct contexts run concurrently.
 */
#ifndef PASTA_MSM_H
#define PASTA_MSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum pm_curve { PM_CURVE_PALLAS = 0, PM_CURVE_VESTA = 1, PM_CURVE_BN254 = 2 };

enum pm_flags {
  PM_SCALARS_CANONICAL = 1u /* scalars are canonical integers (to_repr), not Montgomery */
};

enum pm_status {
  PM_OK = 0,
  PM_ERR_ARG = -1,         /* bad argument (null pointer, unknown curve, size) */
  PM_ERR_HIP = -2,         /* HIP runtime error (message in pm_last_error) */
  PM_ERR_NODEV = -3,       /* no HIP device / device index out of range */
  PM_ERR_UNSUPPORTED = -4  /* shape or option not supported by this build */
};

/* ABI version: bumped on every change of a signature or of an argument's
 * meaning.  3 = round 3 (pm_ctx_set_stream(ctx, NULL) selects the context's
 * own stream again; the accumulator entries take the trailing out_status
 * argument); 4 = round 4 (proof-byte entries pm_*_proofs*, the drop-in cache
 * admits a base set on its second sighting under a keyed digest).  A binding
 * asserts pm_abi_version() == PM_ABI_VERSION at load. */
#define PM_ABI_VERSION 4

typedef struct pm_ctx pm_ctx;     /* one device + one HIP stream + workspace */
typedef struct pm_bases pm_bases; /* device-resident base points (SRS cache) */

/* ---------------------------------------------------------------- misc */
const char* pm_version(void);
int pm_abi_version(void);
const char* pm_last_error(void);
int pm_device_count(int* count);

/* ------------------------------------------------------------- context */
int pm_ctx_create(int device, pm_ctx** out);
int pm_ctx_destroy(pm_ctx* ctx);
/* Stream ordering contract.  Every entry point is synchronous: it returns
 * after its own work has finished.  Its device work is queued on the
 * context's current stream, so inputs the caller wrote on the device must be
 * ordered before it:
 *   - by default the context runs on its own BLOCKING stream, which is
 *     ordered after everything queued on the legacy null stream (torch's
 *     default stream, the hipMemcpy / hipMemset default);
 *   - pm_ctx_set_stream(ctx, s) runs on the caller's stream s instead
 *     (e.g. torch.cuda.current_stream().cuda_stream); s == NULL goes back to
 *     the context's own stream, s == PM_STREAM_LEGACY selects the legacy
 *     null stream itself;
 *   - pm_ctx_use_own_stream(ctx) also goes back to the context's own stream.
 * Work the caller queues on any other non-blocking stream must be
 * synchronised by the caller before the call. */
#define PM_STREAM_LEGACY ((void*)1) /* the HIP legacy null stream (hipStreamLegacy) */
int pm_ctx_set_stream(pm_ctx* ctx, void* hip_stream);
int pm_ctx_use_own_stream(pm_ctx* ctx);
/* Force the window width c (0 = automatic). */
int pm_ctx_set_window(pm_ctx* ctx, int c);
/* Pipeline tuning: the minimum accumulate slice per lane (0 = automatic).
 * `groups` must be 0 or 1: pipelined window groups measured slower on MI355X
 * and were retired (PM_ERR_UNSUPPORTED for groups > 1). */
int pm_ctx_set_pipeline(pm_ctx* ctx, int groups, int min_chunk);
/* Small-MSM path: MSM calls (pm_msm*, pm_msm_device, pm_msm_resident*) of at
 * most max_n terms under the automatic window run two launches -- a table of
 * [1..8] P_i with the GLV-split 4-bit digits, then per-window sums -- and a
 * 33-window host Horner instead of the sorting pipeline.  Default
 * PM_SMALL_MSM_DEFAULT, 0 disables it, at most PM_SMALL_MSM_LIMIT.  Results do
 * not depend on it. */
#define PM_SMALL_MSM_DEFAULT 16384
#define PM_SMALL_MSM_LIMIT 65536
int pm_ctx_set_small_msm(pm_ctx* ctx, size_t max_n);
/* Retired: the GLV-mode variable-base MSM measured slower on MI355X
 * (DESIGN.md §7).  enable == 0 succeeds, anything else returns
 * PM_ERR_UNSUPPORTED.  Kept so older bindings still link. */
int pm_ctx_set_glv(pm_ctx* ctx, int enable);
/* Batch accumulator: each MSM term's scalar is split into 2^lg_lanes bit
 * segments, one lane each (0..5; 0 = one lane per term; -1 = automatic: more
 * lanes per term while the batch leaves SIMDs idle).  Results do not depend
 * on it. */
int pm_ctx_set_accum_split(pm_ctx* ctx, int lg_lanes);
/* Batch accumulator: how the powers-of-two table chains run (mode 0: a quad
 * of lanes per chain; 1: one wave per chain with row-sliced field elements,
 * shorter steps while the chains fit one wave per SIMD; -1 = automatic: 1 for
 * up to 800 chains, and the proof decoder's square roots row-sliced for up
 * to 4096 points on BN254).  Results do not depend on it. */
int pm_ctx_set_accum_ladder(pm_ctx* ctx, int mode);
/* Batch accumulator schedule options (round 6; they replace the PM_ACC_*
 * environment switches of round 5, so a test can flip them per context).
 * value -1 = automatic (the default) for every option.  Results never depend
 * on them.
 *   PM_ACC_OPT_TWIST           0: no twisted ladder (the powers-table ladder
 *                                 waits for the decoded points); 1 / 2: the
 *                                 twisted ladder whenever the powers tables
 *                                 are built, the decode unfenced beside it
 *                                 (1) or two decode blocks per CU (2)
 *   PM_ACC_OPT_TAIL_STREAM     0: term additions and sums on the main stream
 *   PM_ACC_OPT_TERMS_PER_LANE  1 or 2: the one-lane GLV form's terms per lane
 *   PM_ACC_OPT_TRANSCRIPT      0: per-record transcript replay (no streamed
 *                                 byte layout)
 * PM_ERR_ARG for an unknown option or a value out of range. */
enum {
  PM_ACC_OPT_TWIST = 1,
  PM_ACC_OPT_TAIL_STREAM = 2,
  PM_ACC_OPT_TERMS_PER_LANE = 3,
  PM_ACC_OPT_TRANSCRIPT = 4
};
int pm_ctx_set_accum_option(pm_ctx* ctx, int option, int value);
/* MSM schedule options (round 6); value -1 = automatic (the default).
 * Results never depend on them.
 *   PM_MSM_OPT_SPLIT_COPY   0: one scalar copy.  Automatic: an MSM over a
 *                           resident row table with scalars in host memory
 *                           (pm_msm_resident, the drop-in pm_msm's warm
 *                           calls) of at least PM_SPLIT_COPY_MIN_N points
 *                           copies the scalars in two parts (3/8, 5/8;
 *                           three from 2^21 points) and sorts and
 *                           accumulates each part while the next crosses
 *                           PCIe.
 * PM_ERR_ARG for an unknown option or a value out of range. */
#define PM_SPLIT_COPY_MIN_N 262144
enum { PM_MSM_OPT_SPLIT_COPY = 1 };
int pm_ctx_set_msm_option(pm_ctx* ctx, int option, int value);
/* Per-kernel HIP-event timing on the context stream (for bench/profiling).
 * Every event pair costs ~10 us of stream time on MI355X, so a timed region
 * should restrict events to the kernel it measures:
 * pm_ctx_set_timing_filter(ctx, "accumulate") (NULL or "" = every kernel). */
int pm_ctx_set_timing(pm_ctx* ctx, int enable);
int pm_ctx_set_timing_filter(pm_ctx* ctx, const char* kernel);
int pm_ctx_kernel_stats(pm_ctx* ctx, const char* kernel, uint64_t* launches, double* total_ms);
int pm_ctx_reset_stats(pm_ctx* ctx);

/* ------------------------------------------------------------------ MSM
 * Replaces halo2 `arithmetic::best_multiexp<C>(coeffs: &[C::Scalar],
 * bases: &[C]) -> C::Curve` ([3P] halo2 fork kzg-agg2, /root/reference/
 * Cargo.toml:12), called from Params::commit / commit_lagrange
 * (/root/reference/examples/simple-example.rs:638-640) and inside
 * create_proof / verify_proof (:606,620,702,722).  Result: sum_i s_i * P_i as
 * an affine point (8 limbs, Montgomery, (0,0) = identity); the Rust shim turns
 * it into C::Curve with `to_curve()`.  n == 0 yields the identity. */
int pm_msm(int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags,
           uint64_t out[8]);
/* Below this many terms the Rust shim would keep halo2's CPU multiexp.  Since
 * the small-MSM path (round 4: ~67 us at one term, ~81 us at 32, ~140 us at
 * 4096) every n >= 1 is faster on the GPU than halo2's multiexp on 16 host
 * threads (~150 us at one term, ~700 us at 32: bench.py small_n, DESIGN.md
 * §12), so the threshold is 1.  pm_msm itself computes any n. */
#define PM_MSM_GPU_MIN_N 1
/* Same, on an explicit context (host pointers).
 * Drop-in base cache: from 4096 points on (and above the small-MSM threshold,
 * PM_SMALL_MSM_DEFAULT by default), pm_msm / pm_msm_ctx keep the base
 * sets they see repeatedly resident on the device (converted, with the row
 * table from 2^18 points, like pm_bases_upload), keyed by (curve, n, a keyed
 * 254-bit digest of the base bytes computed on host threads while the
 * scalars are copied).  A set is admitted on its SECOND sighting (the first
 * call runs the plain pipeline on uploaded bases), so one-shot bases never
 * pay the resident build; a repeated set -- halo2's commits against params.g
 * / params.g_lagrange -- then costs only its scalars' transfer.  Changed
 * bytes (at the same address or not) miss.  The digest is a universal hash
 * (NH + two polynomial layers over GF(2^127 - 1)) under a secret key drawn
 * per context from the OS RNG and never returned: a caller cannot construct
 * two base sets that collide except with probability ~2^-128.  At most 4 sets,
 * min(16 GiB, half the free device memory) per context, least recently used
 * evicted before a new set is built; if the build still runs out of memory
 * every set is released and, failing that, the call runs the plain pipeline.
 * A warm call starts the MSM of the set a cheap keyed hash of its first and
 * last 8 points predicts right behind the scalar copy, while the full digest
 * is still being computed; the result is returned only if the digest then
 * names that same set (else the speculative MSM is drained and the call
 * proceeds as a miss).  n <= the small-MSM threshold bypasses the cache. */
int pm_msm_ctx(pm_ctx* ctx, int curve, const uint64_t* scalars, const uint64_t* bases, size_t n,
               uint32_t flags, uint64_t out[8]);
/* Drop-in cache counters of ctx (any pointer may be NULL), and a way to
 * release its sets early. */
int pm_ctx_dropin_stats(pm_ctx* ctx, uint64_t* hits, uint64_t* misses, int* entries, size_t* device_bytes);
int pm_ctx_dropin_clear(pm_ctx* ctx);
/* Speculative starts of pm_msm_ctx: kept (the digest confirmed the predicted
 * set) and drained (it named another set or none). */
int pm_ctx_dropin_spec_stats(pm_ctx* ctx, uint64_t* kept, uint64_t* drained);
/* Out-of-memory events of the drop-in cache: *flushes = builds that failed
 * and released every cached set before their one retry, *failed_builds =
 * sets left unadmitted (that call ran the plain pipeline and succeeded). */
int pm_ctx_dropin_oom_stats(pm_ctx* ctx, uint64_t* flushes, uint64_t* failed_builds);
/* The drop-in cache's small sets (1 <= n <= 512, where the many-MSM path
 * beats the small-MSM path): a set seen twice is kept resident with a multiples table
 * (pm_msm_resident_many's) and later calls with it run as one short MSM of
 * that path; at most 8 sets and 4 GiB per context, LRU; pm_ctx_dropin_clear
 * releases them too.  *hits = calls served from a kept set, *admitted = sets
 * admitted so far, *entries / *device_bytes = what is held now. */
int pm_ctx_dropin_small_stats(pm_ctx* ctx, uint64_t* hits, uint64_t* admitted, int* entries, size_t* device_bytes);
/* A fingerprint of ctx's secret digest key (16 bytes of BLAKE2b of the key,
 * personal "pm-dropin-key-id"): distinct contexts hold distinct keys.  It
 * reveals nothing about the key itself. */
int pm_ctx_dropin_key_id(pm_ctx* ctx, uint64_t out[2]);
/* Same, with scalars and bases already in device memory of ctx's device. */
int pm_msm_device(pm_ctx* ctx, int curve, const void* d_scalars, const void* d_bases, size_t n,
                  uint32_t flags, uint64_t out[8]);
/* Split the points into `ngpu` contiguous slices, one device each (devices
 * 0..ngpu-1), and sum the per-device partial points (the multi-GPU analogue
 * of best_multiexp's per-thread chunks). */
int pm_msm_multi(int curve, const uint64_t* scalars, const uint64_t* bases, size_t n, uint32_t flags,
                 int ngpu, uint64_t out[8]);

/* Device-resident base cache: the SRS bases of halo2 Params (`params.g`,
 * `params.g_lagrange`, replacing the `bases` argument of best_multiexp at
 * examples/simple-example.rs:638-640) are fixed, so a caller uploads them once
 * and runs many MSMs against a window [offset, offset + n) of them.  The
 * library converts them once, at upload, to the pipeline's internal form
 * (64 B per point on the device, no per-call conversion).  From 2^18 points
 * on it also keeps [2^{256 j / rows}] P (rows = 8 up to 2^20 points, 4 up to 2^22, else 2;
 * rows x 64 B per point): an MSM over (at least half of) the set from
 * offset 0 then runs as a row-table MSM (pm_fixed_bases_create_rows) with a
 * rows-times shorter bucket reduction and host tail; other windows run the
 * plain pipeline.  pm_bases_info reports n, the rows and the device bytes.
 * _upload takes host bases (Rust layout, as pm_msm), _upload_device bases
 * already in device memory of ctx's device (copied; the caller keeps its
 * buffer).  pm_msm_resident takes host scalars (one pageable copy),
 * pm_msm_resident_device device scalars. */
int pm_bases_upload(pm_ctx* ctx, int curve, const uint64_t* bases, size_t n, pm_bases** out);
int pm_bases_upload_device(pm_ctx* ctx, int curve, const void* d_bases, size_t n, pm_bases** out);
int pm_bases_info(const pm_bases* b, size_t* n, int* rows, size_t* device_bytes);
int pm_bases_release(pm_bases* b);
int pm_msm_resident(pm_ctx* ctx, const pm_bases* b, size_t offset, const uint64_t* scalars,
                    size_t n, uint32_t flags, uint64_t out[8]);
int pm_msm_resident_device(pm_ctx* ctx, const pm_bases* b, size_t offset, const void* d_scalars,
                           size_t n, uint32_t flags, uint64_t out[8]);
/* k MSMs over the same window of resident bases, one per host scalar array
 * (scalars[j]: n x 4 u64), out: k x 8 u64 -- the prover's commit of many
 * polynomials against params.g / g_lagrange (create_proof,
 * examples/simple-example.rs:606,702).  Pipelined: the H2D copy of MSM j+1's
 * scalars overlaps MSM j's kernels on a second stream, and MSM j-1's host
 * tail overlaps them too.  Same results as k pm_msm_resident calls. */
int pm_msm_resident_batch(pm_ctx* ctx, const pm_bases* b, size_t offset, const uint64_t* const* scalars,
                          size_t k, size_t n, uint32_t flags, uint64_t* out);
/* B independent short MSMs against one resident base set in one launch --
 * the aggregator's per-proof instance commitments
 * params_verifier.commit_lagrange(public_inputs)
 * (examples/simple-example.rs:632-641; verifier.rs:200-225, 312-316 take them
 * as the instance column's commitment), i.e. B calls of
 * best_multiexp(public_inputs_i, g_lagrange[0..n_i]):
 *   out[i] = sum_{t < n[i]} s_i[t] P[offsets[i] + t]   (8 u64 affine each)
 * with s_i the next n[i] scalars of `scalars` (concatenated, n x 4 u64 in
 * the pm_msm scalar form and flags).  offsets == NULL: every MSM starts at
 * base 0 (commit_lagrange).  n[i] == 0 gives the identity (0, 0).
 * The first call that reaches a base beyond the set's multiples table builds
 * it (entry (i, w, m) = [m 2^{c w}] P_i: 2^(c-1) x W(c) x 128 B per base, c = 8
 * for up to 4096 bases, narrower windows for longer prefixes, at most 8 GiB);
 * prefixes beyond that cap run one resident MSM per entry (same results).
 * pm_bases_many_prepare builds the table for [0, max_n) ahead of time;
 * pm_bases_many_info reports its prefix, window and bytes (0 when none).
 * Same results as B pm_msm_resident calls. */
int pm_msm_resident_many(pm_ctx* ctx, const pm_bases* b, size_t B, const size_t* n, const size_t* offsets,
                         const uint64_t* scalars, uint32_t flags, uint64_t* out);
int pm_msm_resident_many_device(pm_ctx* ctx, const pm_bases* b, size_t B, const size_t* n, const size_t* offsets,
                                const void* d_scalars, uint32_t flags, uint64_t* out);
int pm_bases_many_prepare(pm_ctx* ctx, const pm_bases* b, size_t max_n);
int pm_bases_many_info(const pm_bases* b, size_t* n, int* window, size_t* device_bytes);
/* Retired: host inputs are copied with one pageable hipMemcpyAsync, which
 * measured faster on MI355X than pinned staging threads (~52 vs ~38 GB/s for
 * 32 MB).  threads == 0 succeeds, threads > 0 returns PM_ERR_UNSUPPORTED. */
int pm_ctx_set_h2d_threads(pm_ctx* ctx, int threads);

/* Device self-test of the MSM pipeline's radix-2^29 lazy field arithmetic
 * against the 32-bit Montgomery arithmetic (n random + edge operand pairs of
 * the curve's base field); *mismatches = number of failed checks. */
int pm_selftest_field(pm_ctx* ctx, int curve, uint64_t seed, size_t n, uint64_t* mismatches);

/* Host self-test of the MSM's host tail arithmetic (no GPU): n random
 * products and a random Horner chain of doublings / additions of the curve's
 * base field through the BMI2/ADX Montgomery product against the portable
 * one; *mismatches = failed checks.  PM_ERR_UNSUPPORTED when the CPU lacks
 * BMI2/ADX (the tail then runs the portable code). */
int pm_selftest_host(int curve, uint64_t seed, size_t n, uint64_t* mismatches);

/* Affine helpers (host) for combining partial results: out = a + b. */
int pm_point_add(int curve, const uint64_t a[8], const uint64_t b[8], uint64_t out[8]);
/* out = points[0] + ... + points[n-1] (n affine points, 8 limbs each, (0,0) =
 * identity; n == 0 yields the identity): the fold of a sharded MSM's per-rank
 * partials in one call (round 6; one inversion instead of one per addition). */
int pm_points_sum(int curve, const uint64_t* points, size_t n, uint64_t out[8]);

/* Synthetic inputs generated on the device: scalar i is
 * uniform in [0, r) from a SplitMix64 stream keyed by (seed, i0 + i);
 * base i is [a_i]G with a_i drawn the same way.  d_out: n*4 (scalars) or n*8
 * (bases) u64 in device memory.  Scalars are Montgomery unless
 * PM_SCALARS_CANONICAL is set. */
int pm_synth_scalars(pm_ctx* ctx, int curve, uint64_t seed, uint64_t i0, size_t n, uint32_t flags,
                     void* d_out);
int pm_synth_bases(pm_ctx* ctx, int curve, uint64_t seed, uint64_t i0, size_t n, void* d_out);

/* ------------------------------------------------- multiopen accumulator
 * Boundary 2: the native meaning of the reference's in-circuit
 * verifier for a batch of B inner proofs that share one verifying key.
 * Per proof it evaluates the scalar block of VerifierChip::_verify_proof
 * (/root/reference/src/verifier.rs:512-652: x^n, l_0 / l_last / l_blind,
 * gate, permutation (src/permutation.rs:190-324) and lookup
 * (src/lookup.rs:173-311) expressions, vanishing h_eval
 * (src/vanishing.rs:136-201)), assembles the queries in the reference order
 * (verifier.rs:654-715), groups them by rotation (src/multiopen.rs:19-45) and
 * produces MultiopenChip::calc_witness's accumulator (src/multiopen.rs:271-509)
 *     w  = sum_j u^{S-1-j} W_j          zw = sum_j u^{S-1-j} z_j W_j
 *     f  = sum_j u^{S-1-j} sum_i v^{m_j-1-i} C_{j,i}   (H = sum_i x^{n i} h_i)
 *     e  = [-sum_j u^{S-1-j} sum_i v^{m_j-1-i} e_{j,i}] g1
 * as exact affine points, plus h_eval.  The Rust side replays the transcript
 * and passes the challenges in; the EccChip / Transcript / VerifyingKey
 * surfaces stay unchanged.
 *
 * Expression code (halo2 plonk::Expression, compute_expr verifier.rs:58-151)
 * is postfix, one u32 word per node: op | arg << 8.  Each expression ends with
 * PM_EXPR_END.  Leaves index the query evals (advice/fixed/instance query
 * index) or the shape's constant table (CONST, SCALED). */
enum pm_expr_op {
  PM_EXPR_END = 0,
  PM_EXPR_CONST = 1,    /* push constants[arg] */
  PM_EXPR_FIXED = 2,    /* push fixed_evals[arg] */
  PM_EXPR_ADVICE = 3,   /* push advice_evals[arg] */
  PM_EXPR_INSTANCE = 4, /* push instance_evals[arg] */
  PM_EXPR_NEG = 5,
  PM_EXPR_SUM = 6,
  PM_EXPR_PROD = 7,
  PM_EXPR_SCALED = 8    /* top *= constants[arg] */
};
enum pm_column_kind { PM_COL_ADVICE = 0, PM_COL_FIXED = 1, PM_COL_INSTANCE = 2 };

typedef struct pm_query {
  uint32_t column;
  int32_t rotation;
} pm_query;

typedef struct pm_perm_column {
  uint32_t kind;        /* pm_column_kind */
  uint32_t query_index; /* index into that kind's query evals */
} pm_perm_column;

/* What the accumulator reads from VerifyingKey / ConstraintSystem
 * (verifier.rs:227-285).  Scalars are 4 x u64 Montgomery, points 8 x u64
 * affine Montgomery, (0,0) = identity. */
typedef struct pm_proof_shape {
  uint32_t log_n;
  uint32_t blinding_factors;     /* cs.blinding_factors() */
  uint32_t num_instance_columns;
  uint32_t num_advice_columns;
  uint32_t num_fixed_columns;
  uint32_t num_lookups;
  uint32_t perm_chunk_len;       /* cs.degree() - 2 */
  uint32_t quotient_degree;      /* number of h pieces */
  uint32_t n_instance_queries, n_advice_queries, n_fixed_queries, n_perm_columns;
  const pm_query* instance_queries;
  const pm_query* advice_queries;
  const pm_query* fixed_queries;
  const pm_perm_column* perm_columns;
  const uint32_t* gate_code;         /* all gate polynomials, in gate order */
  uint32_t gate_code_len;
  const uint32_t* lookup_input_code; /* flattened over lookups (verifier.rs:244-251) */
  uint32_t lookup_input_code_len;
  const uint32_t* lookup_table_code;
  uint32_t lookup_table_code_len;
  const uint64_t* constants;         /* n_constants x 4 */
  uint32_t n_constants;
  uint64_t omega[4];                 /* vk.get_domain().get_omega() */
  uint64_t delta[4];                 /* C::ScalarExt::DELTA */
  uint64_t g1[8];                    /* C::generator() */
  const uint64_t* fixed_commitments; /* num_fixed_columns x 8 */
  const uint64_t* sigma_commitments; /* n_perm_columns x 8 */
} pm_proof_shape;

/* Per-proof layout implied by a shape (transcript read order, see
 * oracle/accum.py): points, scalars, and rotation sets S (= number of W_j). */
int pm_shape_layout(const pm_proof_shape* shape, uint32_t* points_per_proof, uint32_t* scalars_per_proof,
                    uint32_t* num_sets);

/* Batch accumulator, host buffers.  points: B x points_per_proof x 8;
 * scalars: B x scalars_per_proof x 4; challenges: B x 7 x 4 (theta, beta,
 * gamma, y, x, v, u); out_quads: B x 4 x 8 (w, zw, f, e); out_h_eval: B x 4
 * (may be NULL).  curve selects the group (PM_CURVE_*); its scalar field is
 * the field of every scalar above. */
int pm_accum_batch(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t* points,
                   const uint64_t* scalars, const uint64_t* challenges, uint64_t* out_quads, uint64_t* out_h_eval,
                   uint32_t* out_status);
/* Same with every buffer in device memory of ctx's device. */
int pm_accum_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const void* d_points,
                          const void* d_scalars, const void* d_challenges, void* d_out_quads, void* d_out_h_eval,
                          void* d_out_status);
/* Per-proof status words (out_status: B x uint32, may be NULL) of every
 * accumulator entry point.  A nonzero word means the reference verifier
 * would not have produced an accumulator for that proof; its quad and h_eval
 * are then unspecified and the caller must reject the proof:
 *   PM_TRANSCRIPT_IDENTITY_SKIPPED (1)  an identity commitment was skipped by
 *       the transcript (transcript.rs:101-110), transcript entries only;
 *   PM_TRANSCRIPT_LOOKUP_Z_IDENTITY (2) that commitment was a lookup product
 *       Z, where the reference propagates the error and aborts (lookup.rs:100);
 *   PM_ACCUM_DENOM_ZERO (4)  x^n = 1 or x = omega^-i for a Lagrange basis
 *       point: the reference's main_gate.div fails (vanishing.rs:175,
 *       verifier.rs:580). */
#define PM_ACCUM_DENOM_ZERO 4u
/* A batch sharded over nctx contexts (one per device) in one process: proofs
 * are independent, context k takes the contiguous range [k*ceil(B/nctx), ...)
 * in its own host thread (the multi-GPU form of VerifierChip::verify_proof
 * over many proofs, src/verifier.rs:227-285).  challenges == NULL replays
 * the Blake2b transcript from vk_repr (as pm_accum_batch_transcript);
 * otherwise the given challenges are used and vk_repr may be NULL.
 * out_challenges, out_h_eval and out_status may be NULL. */
int pm_accum_batch_multi(pm_ctx* const* ctxs, int nctx, int curve, const pm_proof_shape* shape, size_t B,
                         const uint64_t* points, const uint64_t* scalars, const uint64_t* challenges,
                         const uint64_t vk_repr[4], uint64_t* out_challenges, uint64_t* out_quads,
                         uint64_t* out_h_eval, uint32_t* out_status);

/* ---- Fixed-base MSM ----------------------------------------
 * The prover's commitments (Params::commit / commit_lagrange,
 * examples/simple-example.rs:638-640,702) are MSMs against the static SRS
 * bases.  pm_fixed_bases_create precomputes, once per SRS, the table
 * [2^{o_w}] P_i for every window offset o_w (W = ceil(256 / c) windows, c = 0
 * picks the default); every later MSM then sorts all W digits of every scalar
 * into ONE set of 2^(c-1) buckets and skips the per-window bucket reduction
 * and the cross-window doublings.  Table size: W x n x 64 bytes of device
 * memory (2^20 bases, c = 16: 1 GiB).  pm_msm_fixed* use the first n bases
 * (n <= the table's n); results are bit-identical to pm_msm. */
typedef struct pm_fixed_bases pm_fixed_bases;
int pm_fixed_bases_create(pm_ctx* ctx, int curve, const uint64_t* bases, size_t n, int c, pm_fixed_bases** out);
int pm_fixed_bases_create_device(pm_ctx* ctx, int curve, const void* d_bases, size_t n, int c,
                                 pm_fixed_bases** out);
/* A table of `rows` rows (rows divides W, and rows < W needs equal window
 * widths, 256 % W == 0, e.g. c = 16; 0 = W): row j = [2^{o_{jW/rows}}] P_i,
 * so windows w, w + W/rows, ... share one of W/rows bucket sets.  rows = W is
 * the table above; rows = 2 at c = 16 keeps P and [2^128] P (2 x the bases'
 * memory), halves the bucket reduction and the host Horner (128 instead of
 * 256 doublings) of a plain MSM.  bases_on_device: bases is a device pointer. */
int pm_fixed_bases_create_rows(pm_ctx* ctx, int curve, const void* bases, int bases_on_device, size_t n, int c,
                               int rows, pm_fixed_bases** out);
int pm_fixed_bases_info(const pm_fixed_bases* fb, size_t* n, int* c, int* windows, size_t* table_bytes);
int pm_fixed_bases_release(pm_fixed_bases* fb);
int pm_msm_fixed(pm_ctx* ctx, const pm_fixed_bases* fb, const uint64_t* scalars, size_t n, uint32_t flags,
                 uint64_t out[8]);
int pm_msm_fixed_device(pm_ctx* ctx, const pm_fixed_bases* fb, const void* d_scalars, size_t n, uint32_t flags,
                        uint64_t out[8]);

/* ---- NTT over the scalar field -------------------------------
 * halo2 `best_fft(a, omega, log_n)` [3P] (EvaluationDomain::fft / ifft /
 * coset conversions inside create_proof): in place, natural order in and out,
 * a_k <- sum_j a_j omega^{jk} over the scalar field of `curve` (Montgomery
 * 4 x u64 per element, like pm_msm's scalars).  Elements, omega and scale are
 * canonical (< the modulus), as every value of the Rust field types is; the
 * outputs are canonical.  omega must be a primitive
 * 2^log_n-th root of unity.  scale (may be NULL) multiplies every output:
 * EvaluationDomain::ifft is pm_fft(omega_inv, scale = 1/n).  log_n <= 28
 * (create_proof at k = 23 transforms the extended domain, 2^25); above 2^22
 * the transform takes three passes and 2 n x 32 B of context scratch.  The
 * twiddle tables (each sub-transform's root powers and a two-level table of
 * the inter-pass twiddles, ~0.4 MB at 2^25) are cached in the context (4 most
 * recent (curve, log_n, omega)). */
int pm_fft(pm_ctx* ctx, int curve, uint64_t* data, uint32_t log_n, const uint64_t omega[4], const uint64_t* scale);
int pm_fft_device(pm_ctx* ctx, int curve, void* d_data, uint32_t log_n, const uint64_t omega[4],
                  const uint64_t* scale);

/* ---- Polynomial openings -------------------------------------
 * The prover's half of the GWC multiopen argument, between the coefficients
 * pm_fft_device leaves on the device and the commits of pm_msm_resident*:
 * halo2 `eval_polynomial(a, x)` = sum_t a_t x^t, `kate_division(a, z)` (the
 * n - 1 quotient coefficients of a(X) / (X - z): q_{n-2} = a_{n-1},
 * q_{t-1} = a_t + z q_t; a_0 only enters the remainder a_0 + z q_0 = a(z))
 * [3P arithmetic.rs], and the witness polynomials of
 * poly/multiopen/gwc/prover.rs [3P]: for rotation set j with queries
 * i = 0 .. m_j - 1 at the point z_j,
 *   batch_j = sum_i v^{m_j-1-i} p_{j,i}    (the order of `f` above)
 *   q_j     = kate_division(batch_j, z_j)
 *   W_j     = commit(q_j)
 * (subtracting the batched evaluation first, as halo2 does, only changes a_0
 * and so not q_j).  Exact field arithmetic over the scalar field of `curve`;
 * every scalar is 4 x u64 Montgomery and canonical, like pm_fft's elements,
 * in and out.
 *
 * d_polys is a HOST array of P DEVICE pointers, each to n coefficients.
 * Index, offset and point arrays, v and the evaluations are host memory.
 *
 * pm_poly_eval_device: out_evals[e] = p_{poly_index[e]}(points[e]) for E
 *   (polynomial, point) pairs in one call; a polynomial may appear under
 *   several points (its rotations).
 * pm_multiopen_witness_device: set j uses the polynomials
 *   set_polys[set_offsets[j] .. set_offsets[j+1]) in query order
 *   (set_offsets[0] = 0), at points[j].  d_out_quotients is S x n scalars on
 *   the device: row j holds q_j in elements [0, n-1) and an explicit zero in
 *   element n-1, so a row is a valid n-term MSM or NTT input.  out_evals
 *   (S scalars, may be NULL) receives batch_j(z_j) = a_0 + z_j q_0, the batched
 *   evaluation the verifier's `e` is built from.  An output row must not
 *   alias an input polynomial.
 * pm_multiopen_open_device: the same witness into context scratch
 *   (S x n x 32 B), then S commits over srs[0, n) by the resident MSM path;
 *   out_w is S affine points, (0,0) for the identity.  Same results as the
 *   witness call followed by S pm_msm_resident_device calls.
 * pm_eval_polynomial / pm_kate_division: host-pointer forms in the shape of
 *   the halo2 functions (copy in, one set of one polynomial, copy out;
 *   out_q is n - 1 scalars and may be NULL for n == 1).  They pay two PCIe
 *   crossings: parity, not speed.
 *
 * PM_ERR_ARG: a null pointer, an unknown curve, n == 0, a set with no
 * polynomial, a polynomial index >= P, an SRS shorter than n (checked before
 * the device is touched).  PM_ERR_UNSUPPORTED: n > 2^28, n > 2^26 for the
 * open entry (the MSM's limit), more than 65535 sets or pairs in one call.
 * n == 1 is legal (the quotient row is the single zero, W_j the identity,
 * out_evals the batched constant).  S == 0 and E == 0 succeed and write
 * nothing.  Context scratch: 4 n bytes per set (witness), n / 128 bytes per
 * pair (evaluation). */
int pm_poly_eval_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                        const uint32_t* poly_index, const uint64_t* points, size_t E, uint64_t* out_evals);
int pm_multiopen_witness_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                                const uint32_t* set_offsets, const uint32_t* set_polys, const uint64_t* points,
                                const uint64_t v[4], size_t S, void* d_out_quotients, uint64_t* out_evals);
int pm_multiopen_open_device(pm_ctx* ctx, int curve, const void* const* d_polys, size_t P, size_t n,
                             const uint32_t* set_offsets, const uint32_t* set_polys, const uint64_t* points,
                             const uint64_t v[4], size_t S, const pm_bases* srs, uint64_t* out_w,
                             uint64_t* out_evals);
int pm_eval_polynomial(pm_ctx* ctx, int curve, const uint64_t* coeffs, size_t n, const uint64_t point[4],
                       uint64_t out[4]);
int pm_kate_division(pm_ctx* ctx, int curve, const uint64_t* coeffs, size_t n, const uint64_t z[4],
                     uint64_t* out_q);

/* ---- Grand products ------------------------------------------
 * The running-product polynomials Z of the permutation argument
 * (plonk/permutation/prover.rs::commit [3P]) and of every lookup
 * (plonk/lookup/prover.rs::commit_product [3P]), and ff::BatchInvert [3P]:
 * the step of create_proof between "columns on the device" and the commit to
 * Z in Lagrange form (pm_msm_fixed_device).  Exact arithmetic over the scalar
 * field of `curve`; every scalar is 4 x u64 Montgomery and canonical, in and
 * out, like pm_fft_device's elements.
 *
 * pm_batch_invert_device: a[i] <- a[i]^-1 for the n values at d_data, in
 *   place; a zero stays zero (BatchInvert's behaviour).
 * pm_batch_invert: the host-pointer form (copy in, invert, copy out): parity,
 *   not speed.
 * pm_grand_product_device: S sets over the same n rows.  A factor is one
 *   linear term per row,
 *       f[i] = x[i] + b * y[i] + g
 *   x: a column index < C, or PM_GP_NONE (contributes 0); y: a column index,
 *   PM_GP_OMEGA (the implicit column omega^i), or PM_GP_NONE (b is ignored);
 *   b, g: scalars.  Set j has the numerator factors
 *   num[num_offsets[j] .. num_offsets[j+1]) and the denominator factors
 *   den[den_offsets[j] .. den_offsets[j+1]) (offsets[0] = 0; a list may be
 *   empty, its product is 1; at most PM_GP_MAX_FACTORS per list).  With
 *   N[i] / D[i] the products of the two lists at row i and inv0(0) = 0:
 *       z[0]   = start_j
 *       z[i+1] = z[i] * N[i] * inv0(D[i])        0 <= i < active - 1
 *       last_j = z[active - 1]
 *   Rows [0, active) of row j of d_out_z (S rows of n scalars) are written;
 *   rows [active, n) are left exactly as the caller had them (halo2 fills them
 *   with blinding values).  Rows i >= active - 1 of the columns enter no
 *   output.  start_j = start, or with PM_GP_CHAIN in flags start_0 = start and
 *   start_j = last_{j-1} (the permutation argument's last_z across column
 *   chunks).  out_last (S scalars, may be NULL) receives last_j.
 *   d_cols is a HOST array of C DEVICE pointers, each to n scalars; factors,
 *   offsets, omega, start and out_last are host memory.  omega may be NULL
 *   when no factor names PM_GP_OMEGA.  n need not be a power of two.  The
 *   output rows must not alias an input column, nor each other.
 *
 *   A permutation chunk over the columns c_1..c_m of a chunk starting at
 *   column chunk_start: denominators {x = c_k, y = sigma_k, b = beta,
 *   g = gamma}, numerators {x = c_k, y = PM_GP_OMEGA,
 *   b = beta * delta^(chunk_start + k), g = gamma}, start = 1,
 *   active = n - blinding_factors, chunks chained.  A lookup: denominators
 *   {x = A', g = beta}, {x = S', g = gamma}, numerators {x = A, g = beta},
 *   {x = S, g = gamma} (y = PM_GP_NONE), not chained.
 *
 * PM_ERR_ARG: a null context or pointer (d_cols may be NULL when C == 0), an
 * unknown curve, n == 0, active == 0 or active > n, S == 0, offsets that do
 * not start at 0 or decrease, a list longer than PM_GP_MAX_FACTORS, a column
 * index >= C, PM_GP_OMEGA without omega, unknown flag bits (all checked before
 * the device is touched).  PM_ERR_UNSUPPORTED: n > 2^28, more than 65535 sets
 * in one call.  Context scratch: 40 n bytes per set.  One field inversion per
 * set, none per row. */
#define PM_GP_NONE  0xFFFFFFFFu
#define PM_GP_OMEGA 0xFFFFFFFEu
#define PM_GP_CHAIN 1u
#define PM_GP_MAX_FACTORS 16           /* per list per set */

typedef struct pm_gp_factor {
  uint32_t x;        /* column index < C, or PM_GP_NONE */
  uint32_t y;        /* column index < C, PM_GP_OMEGA, or PM_GP_NONE (b ignored) */
  uint64_t b[4];     /* Montgomery, like every scalar of this ABI */
  uint64_t g[4];
} pm_gp_factor;

int pm_batch_invert_device(pm_ctx* ctx, int curve, void* d_data, size_t n);
int pm_batch_invert(pm_ctx* ctx, int curve, uint64_t* data, size_t n);   /* host pointers: parity form */

int pm_grand_product_device(pm_ctx* ctx, int curve, const void* const* d_cols, size_t C, size_t n,
                            const pm_gp_factor* num, const uint32_t* num_offsets,   /* S + 1 entries */
                            const pm_gp_factor* den, const uint32_t* den_offsets,   /* S + 1 entries */
                            size_t S, const uint64_t omega[4], const uint64_t start[4], size_t active,
                            uint32_t flags, void* d_out_z /* S rows of n */, uint64_t* out_last /* S x 4, may be null */);

/* ---- Lookup permuted columns ---------------------------------
 * halo2 plonk/lookup/prover.rs::compress_expressions and
 * permute_expression_pair [3P]: the step of create_proof between the advice
 * commit and the lookup grand product, whose denominators read A' and S'
 * (above).  Every scalar is 4 x u64 Montgomery and canonical, in and out.  The
 * order is halo2's Ord on field elements: the numeric order of the canonical
 * value, not the order of the Montgomery words.
 *
 * pm_lookup_compress_device: out[i] = sum_k theta^(m-1-k) col_k[i] (Horner
 *   from zero: acc = acc * theta + col_k) over m >= 1 columns of n rows.
 *   d_cols is a HOST array of m DEVICE pointers; theta is host memory.  With
 *   m == 1 the output is the column and theta is not read (it may be NULL).
 *   d_out may be one of the columns.
 * pm_lookup_permute_device: P pairs (A, S) of compressed columns of n rows.
 *   With usable <= n (halo2: n - (blinding_factors + 1)), per pair:
 *     A'[0, usable) = A[0, usable) sorted ascending; T = the multiset
 *     S[0, usable).  Row i is "first" when i == 0 or A'[i] != A'[i-1].  At a
 *     first row S'[i] = A'[i], which uses up one instance of that value in T.
 *     With L = T minus one instance per distinct value of A', ascending, and
 *     r_0 < ... < r_{R-1} the rows that are not first, S'[r_{R-1-k}] = L[k].
 *   Rows [usable, n) of both outputs are left exactly as the caller had them
 *   (halo2 fills them with blinding values).  d_a, d_s, d_out_a, d_out_s are
 *   HOST arrays of P DEVICE pointers.  d_out_a[p] may alias d_a[p] and
 *   d_out_s[p] may alias d_s[p]; several pairs may read the same input column;
 *   an output must not alias anything else of the call (another output, the
 *   other input of its pair, any column of another pair).  n need not be a
 *   power of two; usable may be anything in 1 .. n.
 *   out_status (host memory, P x 2 words: status, row).  status 0: ok (row 0).
 *   status 1: an input value is absent from the table (halo2:
 *   Error::ConstraintSystemFailure); row is the smallest first row of A' whose
 *   value T lacks, A' is still the sorted column and S' is unspecified.  The
 *   call returns PM_OK either way: the status carries the circuit's failure,
 *   and the other pairs of the call are unaffected.
 *   All P pairs run in the same launches.  Any key distribution costs the
 *   same: tiles of PM_LOOKUP_TILE keys are sorted in LDS and merged in
 *   ceil(log2(usable / PM_LOOKUP_TILE)) passes, each merge block producing
 *   PM_LOOKUP_MERGE keys.
 * pm_lookup_permute: the host-pointer form of one pair (copy in, permute, copy
 *   out): parity, not speed.  out_a may be a and out_s may be s; rows >= usable
 *   of out_a / out_s are untouched.
 *
 * PM_ERR_ARG, all checked before the device is touched (the arguments before
 * the context, so a binding can test them without a device): a null pointer
 * (theta only when m > 1) or context, an unknown curve, n == 0, usable == 0 or
 * usable > n, P == 0, m == 0, an output pointer equal to a pointer it may not
 * alias.  PM_ERR_UNSUPPORTED: n > 2^28, P > PM_LOOKUP_MAX_PAIRS,
 * m > PM_LOOKUP_MAX_COLS.  Context scratch (grow-only, sized for the whole call
 * before the first launch is queued): 133 bytes per usable row per pair (two
 * key buffers of 2 x 32, a row map and a flag), plus 8 bytes per 1024 rows. */
#define PM_LOOKUP_MAX_PAIRS 32767      /* two columns per pair in one grid dimension */
#define PM_LOOKUP_MAX_COLS  65535
#define PM_LOOKUP_TILE  2048           /* keys sorted per block */
#define PM_LOOKUP_MERGE 2048           /* keys produced per merge block */

int pm_lookup_compress_device(pm_ctx* ctx, int curve, const void* const* d_cols /* host array of m device pointers */,
                              size_t m, size_t n, const uint64_t theta[4], void* d_out);
int pm_lookup_permute_device(pm_ctx* ctx, int curve, const void* const* d_a, const void* const* d_s, /* P pointers each */
                             size_t P, size_t n, size_t usable,
                             void* const* d_out_a, void* const* d_out_s, uint32_t* out_status /* P x 2: status,row */);
int pm_lookup_permute(pm_ctx* ctx, int curve, const uint64_t* a, const uint64_t* s, size_t n, size_t usable,
                      uint64_t* out_a, uint64_t* out_s, uint32_t out_status[2]);   /* host pointers: parity form */

/* ---- Extended-domain conversions -----------------------------
 * halo2 `EvaluationDomain::{coeff_to_extended, extended_to_coeff,
 * divide_by_vanishing_poly}` [3P poly/domain.rs]: the transforms around the
 * quotient polynomial h(X) in create_proof, batched over columns and fused
 * into the NTT passes of pm_fft_device (no pass over memory of their own).
 * With r the scalar field of `curve`, n = 2^k, N = 2^extended_k,
 * e = extended_k - k, omega_e = extended_omega a primitive N-th root of unity
 * and zeta a primitive cube root of unity (halo2's g_coset = ZETA,
 * g_coset_inv = zeta^2):
 *   coeff_to_extended(a), |a| = n:  out[j] = a(zeta omega_e^j), 0 <= j < N
 *     (a[i] zeta^(i mod 3), zero-extended to N, best_fft with omega_e);
 *   divide_by_vanishing_poly(h), |h| = N:  h[j] <- h[j] t[j mod 2^e],
 *     t[i] = (zeta^n (omega_e^n)^i - 1)^-1, the inverse of X^n - 1 on the coset;
 *   extended_to_coeff(h), |h| = N:  best_fft with omega_e^-1, times N^-1,
 *     times zeta^-(i mod 3), truncated to `keep` coefficients (halo2:
 *     keep = n * quotient_poly_degree, extended_k the smallest with N >= keep).
 * Exact field arithmetic; every scalar is 4 x u64 Montgomery and canonical,
 * in and out, like pm_fft's elements.
 *
 * pm_domain_create computes on the host, and checks before the device is
 *   touched: omega = omega_e^(2^e), omega_e^-1, the three output scales
 *   N^-1 zeta^-j and the 2^e entries of t; then uploads the tables the kernels
 *   read ((6 + 2^e) x 32 B).  A domain belongs to the context's device and
 *   may be used by any context of that device; release it with
 *   pm_domain_release.  pm_domain_info returns k, extended_k, omega and 2^e
 *   (any output pointer may be NULL).
 *
 * d_in / d_out / d_data are HOST arrays of C DEVICE pointers, one per column.
 * C == 0 succeeds and writes nothing.
 * pm_coeff_to_extended_device: column c reads n scalars at d_in[c] and
 *   writes N at d_out[c].  d_out[c] may equal d_in[c] (the input is the
 *   prefix of its own output buffer); otherwise it must not overlap d_in[c].
 *   No column's buffer may overlap another column's.
 * pm_extended_to_coeff_device: column c reads N scalars at d_in[c] and writes
 *   `keep` at d_out[c], 1 <= keep <= N; nothing beyond d_out[c][keep) is
 *   written.  d_out[c] may equal d_in[c], and elements [keep, N) of the
 *   buffer are then unspecified; otherwise d_out[c] must not overlap d_in[c]
 *   and the input is left unchanged.  With PM_EXT_DIVIDE_VANISHING in flags
 *   the input is divided by the vanishing polynomial on the way in: the same
 *   result as pm_divide_by_vanishing_device followed by the plain call.  No
 *   column's buffer may overlap another column's.
 * pm_divide_by_vanishing_device: N scalars per column, in place.
 * pm_fft_batch_device: pm_fft_device on each of the C columns at d_data, in
 *   place, with one synchronisation: the same results as C calls.
 * pm_coeff_to_extended / pm_extended_to_coeff: host-pointer forms of one
 *   column (copy in, convert, copy out; out holds N resp. keep scalars).
 *   Two PCIe crossings: parity, not speed.
 *
 * PM_ERR_ARG: a null context, domain or pointer (a column array may be NULL
 * when C == 0), an unknown curve, extended_k < k, zeta = 1 or zeta^3 != 1,
 * omega_e not of exact order N (omega_e^(N/2) != -1; omega_e != 1 when
 * N = 1), a domain of another device, keep == 0 or keep > N, unknown flag
 * bits.  PM_ERR_UNSUPPORTED: extended_k > 28, e > 8, more than 65535 columns
 * in one call.  k == 0 and e == 0 are legal.
 * Context scratch: the transforms above 2^7 take N x 32 B per column in
 * flight (twice that above 2^22, the three-pass form), shared with pm_fft's;
 * the columns of a call run in groups whose scratch fits 256 MiB per pass
 * buffer, at least one column at a time. */
typedef struct pm_domain pm_domain;
int pm_domain_create(pm_ctx* ctx, int curve, uint32_t k, uint32_t extended_k, const uint64_t extended_omega[4],
                     const uint64_t zeta[4], pm_domain** out);
int pm_domain_info(const pm_domain* d, uint32_t* k, uint32_t* extended_k, uint64_t omega[4], uint32_t* t_len);
int pm_domain_release(pm_domain* d);

#define PM_EXT_DIVIDE_VANISHING 1u
int pm_coeff_to_extended_device(pm_ctx* ctx, const pm_domain* d, const void* const* d_in /* C x n */,
                                void* const* d_out /* C x N */, size_t C);
int pm_extended_to_coeff_device(pm_ctx* ctx, const pm_domain* d, const void* const* d_in /* C x N */,
                                void* const* d_out /* C x keep */, size_t C, size_t keep, uint32_t flags);
int pm_divide_by_vanishing_device(pm_ctx* ctx, const pm_domain* d, void* const* d_data /* C x N, in place */,
                                  size_t C);
int pm_fft_batch_device(pm_ctx* ctx, int curve, void* const* d_data, size_t C, uint32_t log_n,
                        const uint64_t omega[4], const uint64_t* scale);
/* host pointers, one column: parity forms */
int pm_coeff_to_extended(pm_ctx* ctx, const pm_domain* d, const uint64_t* coeffs, uint64_t* out);
int pm_extended_to_coeff(pm_ctx* ctx, const pm_domain* d, const uint64_t* evals, size_t keep, uint32_t flags,
                         uint64_t* out);

/* ---- Quotient numerator on the extended domain ---------------
 * halo2 `evaluate_h`, the input of `vanishing::Argument::construct` [3P
 * plonk/prover.rs]: the step of create_proof between
 * pm_coeff_to_extended_device (every column on the coset) and
 * pm_extended_to_coeff_device (h back to coefficients).  With n = 2^k,
 * N = 2^extended_k, e = extended_k - k and X_j = zeta omega_e^j of the domain,
 * for every 0 <= j < N
 *     out[j] = fold(exprs_j),   h = exprs[0]; for each later expression: h = h y + expr
 * where exprs_j is the list of the verifier's identities (verifier.rs:593-643:
 * the gates, permutation.rs:190-324, lookup.rs:173-311, in that order; the
 * list oracle/accum.py::scalar_block builds) at x = X_j with every evaluation
 * replaced by a read of the column's extended form col[j] = p(X_j):
 *   rotation rule: a query (column, rot) at row j reads
 *     col[(j + rot 2^e) mod N], which is p(omega^rot X_j); rot may be negative.
 *   The permutation product Z of set i is read at rot 0, 1 and
 *     -(blinding_factors + 1); a lookup's Z at rot 0 and 1, its permuted input
 *     A' at rot 0 and -1, its permuted table S' at rot 0; a sigma column at
 *     rot 0; a permutation column through its query index, whatever that
 *     query's rotation.  l_0, l_last and l_blind are the Lagrange polynomials
 *     of rows 0, n - blinding_factors - 1 and the rows after it, at X_j.
 *   The lookup compress runs over the flattened expression lists, and an empty
 *     permutation argument contributes no identity, as in the accumulator.
 * There is no division by X^n - 1 unless PM_QUOT_DIVIDE_VANISHING asks for it.
 *
 * pm_quotient_create compiles the shape into one linear program for the
 *   domain (checked on the host before the device is touched), and builds
 *   l_0, l_last, l_last + l_blind and X_j on the coset (pm_fft_batch_device
 *   with omega^-1, pm_coeff_to_extended_device).  The quotient owns these
 *   buffers (pm_quotient_info: device_bytes) and copies what it needs of the
 *   shape and the domain, so neither has to outlive the call.  It belongs to
 *   the context's device and may be used by any context of that device.
 * pm_quotient_info: the number of folded expressions, field products and
 *   column loads per extended row, value slots of the program and device
 *   bytes owned (any output pointer may be NULL).
 * pm_quotient_device: one launch, one canonical store per row.  The column
 *   arrays are HOST arrays of DEVICE pointers to N scalars each; an array may
 *   be NULL when its count is 0.  challenges: theta, beta, gamma, y.
 *   no-overlap rule: d_out must not overlap any input column (a row reads
 *   other rows of its inputs); no input is written.
 *   PM_QUOT_DIVIDE_VANISHING: out[j] *= t[j mod 2^e] after the fold, the same
 *     result as the plain call followed by pm_divide_by_vanishing_device.
 *   PM_QUOT_ACCUMULATE: the fold starts from d_out[j] instead of 0, so the
 *     expressions of several circuits fold into one h.
 * pm_quotient_eval_host: the compiled program on the CPU at R independent
 *   points.  scalars: R x scalars_per_proof x 4 in pm_shape_layout's per-proof
 *   scalar order (the "rand" evaluation is ignored), x: R x 4, challenges:
 *   R x 16, out: R x 4; l_0, l_last, l_blind from the closed form at x
 *   (x^n = 1 is PM_ERR_ARG).  It needs no device.
 * Every scalar is 4 x u64 Montgomery and canonical, in and out.
 *
 * PM_ERR_ARG, before the device is touched: a null context, domain, shape,
 * quotient, columns or pointer; a null column pointer; shape.log_n != k;
 * shape.omega != the domain's omega; a shape pm_shape_layout rejects; a shape
 * with no expression at all; 2^k < blinding_factors + 2; unknown flag bits; a
 * domain or quotient of another device.  PM_ERR_UNSUPPORTED: N > 2^28; a
 * program longer than 65536 ops, leaves or constants; a program that needs
 * more than 28 value slots (a gate of stack depth 16 needs 16, a lookup
 * expression of that depth 19: every shape pm_shape_layout accepts fits). */
typedef struct pm_quotient pm_quotient;
typedef struct pm_quotient_columns {      /* HOST arrays of DEVICE pointers, N scalars each */
  const void* const* advice;    /* shape.num_advice_columns   */
  const void* const* fixed;     /* shape.num_fixed_columns    */
  const void* const* instance;  /* shape.num_instance_columns */
  const void* const* sigma;     /* shape.n_perm_columns       */
  const void* const* perm_z;    /* permutation sets (ceil(n_perm_columns / perm_chunk_len)) */
  const void* const* lookup_a;  /* permuted input A', shape.num_lookups */
  const void* const* lookup_s;  /* permuted table S' */
  const void* const* lookup_z;
} pm_quotient_columns;
#define PM_QUOT_DIVIDE_VANISHING 1u  /* out[j] *= t[j mod 2^e] after the fold */
#define PM_QUOT_ACCUMULATE       2u  /* the fold starts from d_out[j] instead of 0 (several circuits into one h) */

int pm_quotient_create(pm_ctx* ctx, const pm_domain* d, const pm_proof_shape* shape, pm_quotient** out);
int pm_quotient_info(const pm_quotient* q, uint32_t* n_expressions, uint32_t* products_per_row,
                     uint32_t* loads_per_row, uint32_t* slots, size_t* device_bytes);
int pm_quotient_release(pm_quotient* q);   /* NULL is fine, as pm_domain_release */
int pm_quotient_device(pm_ctx* ctx, const pm_quotient* q, const pm_quotient_columns* cols,
                       const uint64_t challenges[16] /* theta, beta, gamma, y */, uint32_t flags, void* d_out /* N */);
int pm_quotient_eval_host(int curve, const pm_proof_shape* shape, size_t R, const uint64_t* scalars,
                          const uint64_t* x, const uint64_t* challenges, uint64_t* out);

/* ---- Blake2b transcript replay ------------------------------
 * The verifier squeezes theta, beta, gamma, y, x, v, u from a halo2
 * Blake2bWrite/Challenge255 transcript (TranscriptChip,
 * /root/reference/src/transcript.rs:57-145) fed in the verifier's read order
 * (src/verifier.rs:341-719).  These entry points replay it for B proofs at
 * once, one GPU lane per proof, from the same points / scalars buffers
 * pm_accum_batch reads (the W_j are not absorbed).
 *
 * vk_repr: the scalar the verifier absorbs first, Montgomery form; it is
 *   pm_vk_transcript_repr() of the pinned-VK debug string (verifier.rs:341-358).
 * out_status (may be NULL): B x uint32; bit 0 = an identity point was
 *   skipped (TranscriptChip::common_point rejects the identity before hashing,
 *   transcript.rs:101-110).  Such a proof's challenges differ from an honest
 *   prover's; the caller should reject it.  Bit 1 = that point was a lookup
 *   product commitment Z (the reference aborts there, lookup.rs:100).  The
 *   fused accumulator entries add PM_ACCUM_DENOM_ZERO (see pm_accum_batch). */
#define PM_TRANSCRIPT_IDENTITY_SKIPPED 1u
#define PM_TRANSCRIPT_LOOKUP_Z_IDENTITY 2u

/* vk_repr = from_bytes_wide(Blake2b-512(personal "Halo2-Verify-Key",
 *   le_u64(len) || pinned[0..len))) in Montgomery form (verifier.rs:341-358).
 *   Host only; needs no device. */
int pm_vk_transcript_repr(int curve, const uint8_t* pinned, size_t len, uint64_t out[4]);
/* out_challenges: B x 7 x 4 (theta, beta, gamma, y, x, v, u), Montgomery. */
int pm_transcript_batch(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4],
                        const uint64_t* points, const uint64_t* scalars, uint64_t* out_challenges,
                        uint32_t* out_status);
int pm_transcript_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                               const uint64_t vk_repr[4], const void* d_points, const void* d_scalars,
                               void* d_out_challenges, void* d_out_status);
/* Transcript replay + accumulator in one call (challenges stay on the
 * device).  out_challenges, out_h_eval and out_status may be NULL. */
int pm_accum_batch_transcript(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                              const uint64_t vk_repr[4], const uint64_t* points, const uint64_t* scalars,
                              uint64_t* out_challenges, uint64_t* out_quads, uint64_t* out_h_eval,
                              uint32_t* out_status);
/* Device-buffer variant; d_challenges is caller-provided B x 7 x 4 scratch
 * (it receives the replayed challenges). */
int pm_accum_batch_transcript_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                     const uint64_t vk_repr[4], const void* d_points, const void* d_scalars,
                                     void* d_challenges, void* d_out_quads, void* d_out_h_eval,
                                     void* d_out_status);

/* ---- Proof bytes (SURVEY §8b boundary 2, from the serialized proofs) --------
 * The reference verifier reads each inner proof from halo2's byte transcript
 * (Blake2bRead): t.read_point() (src/verifier.rs:370, src/lookup.rs:64-65,96,
 * src/permutation.rs:67, src/vanishing.rs:67,94, src/multiopen.rs:210) and
 * t.read_scalar() (src/verifier.rs:443,456,469, src/vanishing.rs:122,
 * src/permutation.rs:100-107,163, src/lookup.rs:124-128).  These entries take
 * the proofs as those bytes and do the reads on the device, B proofs at once:
 *   point  = 32 bytes: canonical little-endian x, bit 255 = parity of the
 *            canonical y (GroupEncoding::to_bytes of pasta_curves /
 *            pairing_bn256 [3P]); decompressed with a square root;
 *   scalar = 32 bytes: canonical little-endian (PrimeField::to_repr).
 * Byte layout of one proof, pm_proof_size() bytes: the proof points of the
 * accumulator layout after the instance commitments (advice, per lookup A'
 * and S', permutation Z_p, per lookup Z, vanishing r, h_0..h_{d-1}), then every
 * scalar in the accumulator layout, then the multiopen witnesses W_0..W_{S-1}
 * -- the verifier's read order.  Instance commitments do not travel in the
 * proof (verifier.rs:312-316 takes them from the instance column); the caller
 * passes them as affine Montgomery points, B x num_instance_columns x 8 u64.
 * proofs: B proofs, proof i at byte i * stride (stride >= pm_proof_size; the
 * device variants need stride % 4 == 0).
 * Status bits (out_status), where the reference's read fails and it aborts:
 *   PM_PROOF_BAD_POINT (8)   a point encoding is invalid: x not canonical,
 *       x^3 + b a non-residue, or the identity (Blake2bRead's common_point
 *       rejects it);
 *   PM_PROOF_BAD_SCALAR (16) a scalar encoding is >= r.
 * Such a proof's decoded slot holds the identity / zero and its quad is
 * unspecified; the rest of the batch is unaffected. */
#define PM_PROOF_BAD_POINT 8u
#define PM_PROOF_BAD_SCALAR 16u
int pm_proof_size(const pm_proof_shape* shape, size_t* bytes);
/* Decode only: out_points B x points_per_proof x 8 (instance commitments
 * copied in), out_scalars B x scalars_per_proof x 4, out_status B (required):
 * the inputs of pm_accum_batch*. */
int pm_decode_proofs(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint8_t* proofs,
                     size_t stride, const uint64_t* instance_points, uint64_t* out_points, uint64_t* out_scalars,
                     uint32_t* out_status);
int pm_decode_proofs_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const void* d_proofs,
                            size_t stride, const void* d_instance_points, void* d_out_points, void* d_out_scalars,
                            void* d_out_status);
/* Decode + transcript replay + accumulator in one call (pm_accum_batch_transcript
 * on the decoded proofs; the decoded points and scalars stay on the device).
 * out_challenges, out_h_eval and out_status may be NULL; the status words
 * carry the decoder's bits as well as the replay's and PM_ACCUM_DENOM_ZERO. */
int pm_accum_batch_proofs(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B, const uint64_t vk_repr[4],
                          const uint8_t* proofs, size_t stride, const uint64_t* instance_points,
                          uint64_t* out_challenges, uint64_t* out_quads, uint64_t* out_h_eval, uint32_t* out_status);
/* Device-buffer variant; d_challenges: B x 7 x 4 caller scratch (receives the
 * challenges); d_out_h_eval and d_out_status may be NULL. */
int pm_accum_batch_proofs_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                 const uint64_t vk_repr[4], const void* d_proofs, size_t stride,
                                 const void* d_instance_points, void* d_challenges, void* d_out_quads,
                                 void* d_out_h_eval, void* d_out_status);

/* ---- BN254 pairing decider -----------------------------
 * The fork's verify_proof returns (Choice, efw); the accumulator entries above
 * deliver efw.  These entries deliver the Choice: for an accumulator quad
 * (w, zw, f, e), where e is already negated (multiopen.rs:490-492),
 *     ok = [ e(w, s_g2) e(-(zw + f + e), g2) == 1 ]
 * per item, with ParamsVerifier's s_g2 = [tau]G2 and g2.  BN254 only: the
 * entries take no curve argument.
 *
 * Pairing: optimal ate, loop scalar 6x + 2 (x = 4965661367192848881) from the
 * top bit down, over Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3 - (9+u)),
 * Fp12 = Fp6[w]/(w^2 - v), the D-type twist y^2 = x^3 + 3/(9+u); the exponent
 * of the final exponentiation is exactly (p^12 - 1)/r (no cofactor).
 *
 * G2 point (assumed layout, the in-memory pairing_bn256 G2Affine): 16 x u64 =
 *   x.c0[4], x.c1[4], y.c0[4], y.c1[4], each Montgomery with R = 2^256 and
 *   canonical.
 * pm_pairing_create checks on the host, once, that both points are on the
 *   twist and of order r (an off-curve, wrong-order, non-canonical or identity
 *   point is PM_ERR_ARG), and computes every line coefficient of both Miller
 *   loops (inversions included): the device never touches G2 arithmetic.  With
 *   a context the tables are uploaded to its device and the object may be used
 *   by any context of that device; ctx may be NULL for a host-only object
 *   (pm_accum_decide_host).  pm_pairing_info: line evaluations per pairing,
 *   bytes of the device table, lanes per pairing product (any output pointer
 *   may be NULL).  pm_pairing_release: NULL is fine.
 * pm_pairing_check_device: d_pairs B x 2 x 8 u64, affine G1 points (A, C) as
 *   everywhere in this header ((0,0) = identity);
 *   ok = [e(A, s_g2) e(C, g2) == 1].  An identity point contributes 1 (not an
 *   error).  A point that is neither (0,0) nor on y^2 = x^3 + 3 gives ok = 0
 *   and status bit PM_DECIDE_NOT_ON_CURVE.
 * pm_accum_decide_device: d_quads B x 4 x 8 u64 as the accumulator entries
 *   write them; A = w, C = -(zw + f + e), the sum by the complete group law on
 *   the device.  The accumulator's d_out_status can be passed as d_status_in.
 * d_status_in (may be NULL): B x u32; a non-zero word gives ok = 0 without
 *   evaluation and is passed through to d_out_status.
 * d_out_ok: B x u32, 1 = accepted, 0 = rejected.  d_out_status (may be NULL):
 *   B x u32.  d_out_gt (may be NULL): B x 48 u64, the final-exponentiated
 *   product as 12 Fp values of 4 x u64, canonical, Montgomery with R = 2^256,
 *   in the tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1; all zero for
 *   an item that was not evaluated (status != 0).
 * pm_accum_decide: the host-pointer form (staged through the context).
 * pm_accum_decide_host: the same check on the CPU, on the process's threads
 *   (at most 16; one pool kept for the process, so concurrent calls take
 *   turns); it needs no device and no context, and gives the same words as the
 *   device forms.
 * B == 0 succeeds and writes nothing.  PM_ERR_ARG, checked before the context
 *   is looked at: a null pm_pairing, input or out_ok; then a null context, a
 *   pm_pairing created without a context or for another device.
 *   PM_ERR_UNSUPPORTED: B > 2^24. */
#define PM_DECIDE_NOT_ON_CURVE 8u
typedef struct pm_pairing pm_pairing;
int pm_pairing_create(pm_ctx* ctx, const uint64_t g2[16], const uint64_t s_g2[16], pm_pairing** out);
int pm_pairing_info(const pm_pairing* pr, uint32_t* steps, size_t* table_bytes, uint32_t* lanes_per_pairing);
int pm_pairing_release(pm_pairing* pr);
int pm_pairing_check_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_pairs /* B x 2 x 8 */,
                            const void* d_status_in, void* d_out_ok, void* d_out_status, void* d_out_gt);
int pm_accum_decide_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads /* B x 4 x 8 */,
                           const void* d_status_in, void* d_out_ok, void* d_out_status, void* d_out_gt);
int pm_accum_decide(pm_ctx* ctx, const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                    uint32_t* out_ok, uint32_t* out_status, uint64_t* out_gt);
int pm_accum_decide_host(const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                         uint32_t* out_ok, uint32_t* out_status, uint64_t* out_gt);

/* ---- Batch decider --------------------------------------
 * "Are all B proofs valid?" with ONE pairing product instead of B: with 128-bit
 * coefficients r_i,
 *     L = sum r_i w_i,   R = sum r_i C_i,   C_i = -(zw_i + f_i + e_i),
 *     ok = [ e(L, s_g2) e(R, g2) == 1 ].
 * Every accepted batch of the per-proof decider is accepted.  A batch with a
 * proof the per-proof decider rejects is rejected except with probability
 * about 2^-127 over the seed.  SOUNDNESS CONDITION: the seed must be fixed after
 * the proofs are fixed and must be unknown to whoever made them (with a known
 * seed two invalid proofs can be made to cancel).  BN254 only.
 *
 * r_i = the first 16 bytes, little-endian, of BLAKE2b-512 with the
 *   personalisation "pm-batch-decide" (zero-padded to 16 bytes) over
 *   seed[32] || le64(i); used as it comes (a zero is not special-cased).
 * Item status: a non-zero d_status_in word is passed through; a point that is
 *   neither (0,0) nor on the curve gives PM_DECIDE_NOT_ON_CURVE.  An item with a
 *   non-zero status makes ok = 0 and contributes nothing to L and R.  An
 *   identity w_i or C_i contributes nothing and is not an error.  ok = 1 iff
 *   every status is 0 and the product is 1; L = R = identity gives 1.
 * seed: 32 bytes, or NULL: the library draws them from the OS (the source of
 *   the drop-in cache key; its failure is PM_ERR_HIP).  out_seed (32 bytes,
 *   may be NULL) receives the seed that was used, so a result can be reproduced.
 * out_ok: one u32 in host memory.  out_pair (may be NULL): 2 x 8 u64 in host
 *   memory, L then R, affine as everywhere in this header.
 * d_out_status (may be NULL): B x u32, may be d_status_in itself.
 * flags: PM_DECIDE_LOCATE with d_out_item_ok (B x u32) non-NULL: an accepted
 *   batch writes all ones; a rejected batch runs pm_accum_decide_device on the
 *   same quads and d_out_item_ok receives its words.  Without the flag
 *   d_out_item_ok is not touched.  Any other flag bit is PM_ERR_ARG.
 * pm_accum_decide_batch: the host-pointer form (staged through the context).
 * pm_accum_decide_batch_host: the same definition on the CPU (one thread), no
 *   context: the parity form and the CPU baseline; the same words as the device
 *   forms.
 * pm_verify_proofs_batch_device: pm_accum_batch_proofs_device (same arguments,
 *   curve must be PM_CURVE_BN254) and then the batch decider on d_out_quads and
 *   d_out_status where they lie on the device: the fork's
 *   verify_proof(...) -> (Choice, efw) for a batch, in one call.  d_out_status
 *   is required here: it carries the decoder's and the replay's status words to
 *   the decider and receives the decider's.
 * B == 0 succeeds and writes ok = 1 (and zero out_pair).  PM_ERR_ARG, checked
 *   before the context is looked at: a null pm_pairing, input or out_ok, an
 *   unknown flag bit; then a null context, a pm_pairing created without a
 *   context or for another device.  PM_ERR_UNSUPPORTED: B > 2^24. */
#define PM_DECIDE_LOCATE 1u
int pm_accum_decide_batch_device(pm_ctx* ctx, const pm_pairing* pr, size_t B, const void* d_quads /* B x 4 x 8 */,
                                 const void* d_status_in, const uint8_t* seed /* 32 bytes or NULL */, uint32_t flags,
                                 uint32_t* out_ok, void* d_out_item_ok, void* d_out_status,
                                 uint64_t* out_pair /* 2 x 8 */, uint8_t* out_seed /* 32 bytes */);
int pm_accum_decide_batch(pm_ctx* ctx, const pm_pairing* pr, size_t B, const uint64_t* quads,
                          const uint32_t* status_in, const uint8_t* seed, uint32_t flags, uint32_t* out_ok,
                          uint32_t* out_item_ok, uint32_t* out_status, uint64_t* out_pair, uint8_t* out_seed);
int pm_accum_decide_batch_host(const pm_pairing* pr, size_t B, const uint64_t* quads, const uint32_t* status_in,
                               const uint8_t* seed, uint32_t flags, uint32_t* out_ok, uint32_t* out_item_ok,
                               uint32_t* out_status, uint64_t* out_pair, uint8_t* out_seed);
int pm_verify_proofs_batch_device(pm_ctx* ctx, int curve, const pm_proof_shape* shape, size_t B,
                                  const uint64_t vk_repr[4], const void* d_proofs, size_t stride,
                                  const void* d_instance_points, void* d_challenges, void* d_out_quads,
                                  void* d_out_h_eval, void* d_out_status, const pm_pairing* pr, const uint8_t* seed,
                                  uint32_t flags, uint32_t* out_ok, void* d_out_item_ok, uint64_t* out_pair,
                                  uint8_t* out_seed);

/* ---- NTT over the group: the SRS's Lagrange basis -------
 * halo2's best_fft is generic over Group; pm_fft* is its scalar half, this is
 * the half over curve points:
 *
 *     out[k] = [scale] sum_j [omega^{jk}] in[j],    0 <= k < n = 2^log_n
 *
 * in place, natural order in and out.  Points are the boundary's affine form
 * (8 x u64, Montgomery R = 2^256, (0,0) the identity); the results are affine
 * and canonical, an identity result is (0,0), so they are unique: the three
 * entries agree limb for limb.  Inputs are assumed to be on the curve, as for
 * pm_msm; they are not checked.  omega (4 x u64 Montgomery, canonical) must be a
 * primitive 2^log_n-th root of unity in the curve's scalar field; scale
 * (likewise, or NULL: no scaling pass) may be any scalar, scale = 0 gives n
 * identities.  log_n = 0 is legal: out[0] = [scale] in[0].
 *   g_lagrange = pm_fft_points(g, omega^-1, scale = n^-1)
 * as ParamsKZG::setup computes it from the monomial basis g.
 *
 * pm_fft_points_device: n points in device memory, on the context's stream.
 * pm_fft_points: the host-pointer form, staged through the context.
 * pm_fft_points_host: the same definition on the CPU, no context: the parity
 *   form and the CPU baseline, on `threads` host threads (0 or 1: the caller's).
 * PM_ERR_ARG, checked before the context is looked at: a null pointer or omega,
 *   an unknown curve, omega not of exact order n (omega^(n/2) != -1; at n = 1,
 *   omega != 1); then a null context.  PM_ERR_UNSUPPORTED: log_n > 26.
 * Context scratch is grow-only: 48 B per twiddle, n/2 twiddles, cached per
 *   (curve, log_n, omega) in two slots; the host-pointer form stages 64 n B. */
int pm_fft_points_device(pm_ctx* ctx, int curve, void* d_points, uint32_t log_n, const uint64_t omega[4],
                         const uint64_t* scale /* may be NULL */);
int pm_fft_points(pm_ctx* ctx, int curve, uint64_t* points, uint32_t log_n, const uint64_t omega[4],
                  const uint64_t* scale);
int pm_fft_points_host(int curve, uint64_t* points, uint32_t log_n, const uint64_t omega[4], const uint64_t* scale,
                       int threads);

#ifdef __cplusplus
}
#endif
#endif /* PASTA_MSM_H */

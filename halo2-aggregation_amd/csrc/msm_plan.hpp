// msm_plan.hpp -- host-side geometry of the MSM drivers, free of HIP.
//
// Everything engine.hpp and msm_many.hpp decide from n, the batch and the
// context options before they launch: the window plan, the split scalar
// copy's parts, each part's sort geometry and LDS requests, the reduction's
// grids, and the small / many paths' slices.  The drivers only follow these
// structs; tests/native/plan_dump.cpp and host_asan.cpp call the same
// functions under g++.  Constants the kernels share (block sizes, tile
// layouts) are defined here once and the kernel headers include this file.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/pasta_msm.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define PM_PLAN_HD __host__ __device__ inline
#else
#define PM_PLAN_HD inline
#endif

namespace pm {

constexpr int kMinC = 4;
constexpr int kMaxC = 20;
// Widest automatic window.  Measured on MI355X (profiles/r01_s2/diag22): once
// the bucket array (W * 2^(c-1) * 128 B) outgrows the caches, the scattered
// 128-B bucket stores of k_accumulate dominate: at 2^22, c = 18 took 11.7 ms
// in accumulate vs 6.1 ms at c = 16; at 2^20, c = 20 took 23.8 ms vs 1.4 ms.
constexpr int kAutoMaxC = 16;
constexpr int kL1 = 4;  // bucket-segment length of k_bucket_seg_q (one quad per segment)
// k_bucket_bits blocks per job = kBitsSplitK / (bucket sets): the bit sums of
// few sets (row tables, the fixed-base MSM) are split over more blocks; every
// extra lane also adds one tree addition (round 3 sweep of 4..64 / Wr at
// 2^19-2^22, profiles/r03/ab/bits_split_sweep.jsonl: 16 best)
constexpr int kBitsSplitK = 16;
// the split scalar copy of row-table MSMs with host scalars (engine.hpp)
constexpr size_t kSplitCopyMinN = PM_SPLIT_COPY_MIN_N;
constexpr size_t kSplitCopy3MinN = size_t(1) << 21;  // three parts from here (measured at 2^20 and 2^22)

// ----------------------------------------------------------------- scan
constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 16;
constexpr int kScanChunk = kScanThreads * kScanPerThread;

// The block histograms are stored in tiles (k_sort_hist): rows of `nblk`
// block counters, R = kScanChunk / nblk rows per tile, and inside a tile
// block-major (counter (row, blk) at blk * Rt + row % R, Rt = the tile's
// rows), so each histogram block writes runs of Rt counters instead of one
// 4-B store per row (2^20: 8 us, 2^22: 24 us of strided stores before).  A
// scan block covers one tile (chunk = R nblk) and reads it in logical
// (row, blk) order; R = 1 (nblk > kScanChunk / 2) is the plain row-major
// layout with chunk = kScanChunk.
struct ScanTiles {
  uint32_t chunk;  // counters per scan block (one tile)
  uint32_t R;      // rows per tile (1: row-major)
  uint32_t nblk;   // counters per row
  uint32_t rows;   // histogram rows (the sentinel follows them)
};
PM_PLAN_HD ScanTiles scan_tiles(uint32_t rows, uint32_t nblk) {
  const uint32_t R = nblk <= (uint32_t)kScanChunk / 2 ? (uint32_t)kScanChunk / nblk : 1u;
  return ScanTiles{R > 1 ? R * nblk : (uint32_t)kScanChunk, R, nblk, rows};
}

// ----------------------------------------------------------------- sort
constexpr int kSortThreads = 1024;
constexpr int kSortPerThread = 8;                      // max points per thread (SortGeom::ppt)
constexpr int kSortB = kSortThreads * kSortPerThread;  // max points per block (fixed-base padding)
constexpr uint32_t kFineChunkBytes = 32768;            // auto: chunk buffer of segments larger than one chunk
constexpr size_t kMaxLds = 160 * 1024;                 // LDS per CU (one workgroup may take all of it)
#ifndef PM_FINE_THREADS  // A/B builds only: 256 / 1024 measured slower (profiles/r03/sort_fine/fine_threads.jsonl)
#define PM_FINE_THREADS 512
#endif
constexpr int kFineThreads = PM_FINE_THREADS;

struct SortGeom {
  int FB;    // fine bits
  int NCB;   // coarse bins per window
  int nblk;  // point blocks of ppt * kSortThreads points
  int blk0;  // k_sort_hist: first block of this launch (chunked launches behind a chunked scalar copy)
  int ppt;   // points per thread, <= kSortPerThread
  int hsub;  // coarse geometry: histogram blocks per coarse block (bofs rows hold nblk histogram blocks)
  // words the histogram kernel zeroes for later stages (instead of two
  // hipMemsetAsync fills per call): the scan sentinel, and the chain-list
  // counters (4 words) of each window group
  uint32_t* clr_bh;
  uint32_t* clr_longs;
  uint32_t clr_stride;  // words between group headers
  int clr_groups;
  // entry index remap of k_sort_coarse (a part of a row table's points, the
  // split scalar copy): sort-row entry e = j rstride + i -> table index
  // e + j rdelta + roff (= j npad + c0 + i); rdelta = roff = 0: e itself
  uint32_t rstride, rdelta, roff;
};

// ------------------------------------------------------------ reduction
constexpr int kMaxParts = 3;
constexpr int kRedThreads = 512;
constexpr int kTJobs = 2;
constexpr int kMaxSplit = 64;

// ---------------------------------------------------------- window plan
struct MsmPlan {
  int c;          // target window width (bits)
  int W;          // windows = ceil(256 / c); widths base or base+1 (WinGeom)
  int base, extra;
  int cmax;       // widest window
  int K;          // max |digit| = 2^(cmax-1)
  int L1;         // bucket-segment length of k_bucket_seg_q
  int log2L1;
  int NB;         // bucket slots per window (K+1 rounded up to L1)
  int M1;         // segments per window: K / L1 (slots [0, K); bucket K apart)
  int NB2;        // bits of the segment index
  uint32_t n;
  uint32_t chunk;     // sorted entries per accumulate lane
  uint32_t nthreads;  // accumulate lanes
  int width(int w) const { return base + (w < extra ? 1 : 0); }
};

inline int plan_bit_length(uint32_t v) {
  int b = 0;
  while (v) {
    b++;
    v >>= 1;
  }
  return b;
}

inline MsmPlan make_plan(size_t n, int c_override, int min_chunk = 0) {
  MsmPlan pl;
  int lg = plan_bit_length((uint32_t)std::max<size_t>(n, 1)) - 1;
  // auto window: lg - 2 from 2^14 up (capped at 16), lg - 4 below; swept on
  // MI355X (profiles/r01_s3/c_sweep_*.jsonl): 2^16 c = 14, 2^18 c = 16 (was
  // lg - 4 everywhere: 2^18 0.85 -> 0.77 ms, 2^16 0.68 -> 0.61 ms)
  int c = c_override > 0 ? c_override : std::max(4, std::min(kAutoMaxC, lg >= 14 ? lg - 2 : lg - 4));
  c = std::max(kMinC, std::min(kMaxC, c));
  pl.c = c;
  pl.W = (256 + c - 1) / c;
  pl.base = 256 / pl.W;
  pl.extra = 256 % pl.W;
  pl.cmax = pl.base + (pl.extra ? 1 : 0);
  pl.K = 1 << (pl.cmax - 1);
  pl.L1 = std::min(kL1, pl.K);
  pl.log2L1 = plan_bit_length((uint32_t)pl.L1) - 1;
  pl.NB = ((pl.K + 1 + pl.L1 - 1) / pl.L1) * pl.L1;
  // segments cover slots [0, K); the top bucket K (the only one past them)
  // is folded by segment 0's unused slot-0 lane and reaches the host Horner
  // on its own (weight K): K / L1 is a power of two, so the segment grids
  // fill whole block rounds (2^20: 2048 blocks of k_bucket_seg_q, not 2049)
  pl.M1 = pl.K / pl.L1;
  pl.NB2 = plan_bit_length((uint32_t)(pl.M1 - 1));
  pl.n = (uint32_t)n;
  // one window group: round 1 measured pipelined window groups (reduction of
  // group g beside the accumulation of g-1) slower at every size -- the
  // reduction kernels compete for the same VALU slots and each smaller
  // accumulate launch loses occupancy (2^20: G=1 2.29 ms, G=2 2.43, G=4 2.95;
  // profiles/r01_s2/pipe2) -- and round 3 retired them
  const size_t work = (size_t)n * pl.W;
  const size_t target = 256 * 1024;  // lanes in flight: 256 CUs x 16 waves x 64
  const size_t mc = min_chunk > 0 ? (size_t)min_chunk : 16;
  pl.chunk = (uint32_t)std::max<size_t>(mc, (work + target - 1) / target);
  pl.nthreads = (uint32_t)((work + pl.chunk - 1) / pl.chunk);
  return pl;
}

// fixed-base MSM over a table of npad rows per window (accumulate work =
// W * npad entries)
// the accumulate work of a table is every window's entries, npad * W: make_plan's over npad points
inline MsmPlan make_plan_fixed(size_t npad, int c, int min_chunk = 0) { return make_plan(npad, c, min_chunk); }

// ------------------------------------------------- split scalar copy parts
// Split scalar copy (round 6): a row-table MSM with scalars in host memory
// sorts and accumulates a first part of its points while the rest of the
// scalars cross PCIe.  A pageable hipMemcpyAsync blocks the calling thread
// for the whole copy but overlaps kernels on other streams
// (tools/h2d_overlap.hip: 32 MB in 0.60 ms, 2 x 16 MB 0.62, a 0.45 ms kernel
// meanwhile hidden), so: copy part 0 on the context stream (blocks), queue
// its sort and accumulation there, copy part 1 on the copy stream (blocks
// while part 0 runs), then queue part 1's sort and accumulation on the
// context stream behind an event of that copy, and one bucket reduction
// over both sorted lists (k_bucket_seg_q<F, 2>).  Part 1's kernels stay on
// the context stream: beside part 0's accumulation on a queue of their own
// they only slowed it (sort 0.10 -> 0.27 ms, accumulation 0.49 -> 0.52,
// same end; rocprofv3 trace, round 6).  Each part is sorted as a table of
// its own points (digit rows of its padded length) and k_sort_coarse
// writes the full table's indices.
struct MsmParts {
  int nch;
  size_t pstart[kMaxParts + 1];
};
inline size_t sort_round(size_t v) { return (v + kSortB - 1) / kSortB * kSortB; }
// split_copy_option: the context's PM_MSM_OPT_SPLIT_COPY (-1 auto, 0 one scalar copy)
inline MsmParts msm_parts(size_t n, bool fixed, bool host_scalars, int split_copy_option) {
  MsmParts p{1, {0, n, n, n}};
  p.nch = fixed && host_scalars && split_copy_option != 0 && n >= kSplitCopyMinN
              ? (n >= kSplitCopy3MinN ? 3 : 2) : 1;
  // Two parts: the first is 3/8 of the points -- its copy is the exposed one,
  // and the second part's copy (5/8) still ends before the first part's sort
  // and accumulation do (2^20 with host scalars: 1/2 1.61 ms, 5/16
  // 1.57-1.58, 3/8 1.57, 7/16 1.64; 2^22: 3/8 5.68 ms, 1/2 6.00 ms, one copy
  // 7.3-7.4).  Three parts (1/4, 3/8, 3/8) from kSplitCopy3MinN points: the
  // exposed copy shrinks with n while each extra part costs a fixed sort
  // (~0.04 ms) and chain fold (2^20: 1.64-1.68 ms against 1.59-1.62 with two;
  // 2^22: 5.25-5.32 against 5.63-5.66; profiles/r06/split_copy_ab.jsonl)
  // part starts (multiples of kSortB): two parts 3/8 + 5/8, three 1/4 + 3/8 + 3/8
  if (p.nch == 2) p.pstart[1] = sort_round(n * 3 / 8);
  if (p.nch == 3) {
    p.pstart[1] = sort_round(n / 4);
    p.pstart[2] = sort_round(n * 5 / 8);
  }
  p.pstart[p.nch] = n;
  return p;
}
// digit row length: n, the table's padded rows, or a part's own padded length
inline size_t part_stride(const MsmParts& p, int ch, size_t n, bool fixed, size_t npad) {
  return !fixed ? n
         : p.nch > 1 ? std::max<size_t>(kSortB, sort_round(p.pstart[ch + 1] - p.pstart[ch]))
                     : npad;
}

// ------------------------------------------------------ per-part sort plan
// what one MSM call fixes for every part (msm_schedule fills it)
struct MsmShape {
  size_t n;
  bool fixed;          // a fixed-base / row table (npad, fixed_c, rows)
  size_t npad;
  int fixed_c, rows;
  bool host_scalars;
  int window_c, min_chunk, split_copy;  // context options
  int fine_cache_kb, fine_chunk_kb;     // PM_FINE_CACHE_KB / PM_FINE_CHUNK_KB (0 = auto)
};
enum : int { kPlanOk = 0, kPlanFineTooWide = 1 };  // "sort: fine bits too wide"
// sort geometry of a digit row length (the whole MSM's, or a part's)
struct SortPlan {
  size_t c0, nc;  // the part's points [c0, c0 + nc)
  size_t stride;  // digit row length
  size_t E, nW, TOTB;
  SortGeom g, gm;  // histogram / coarse + fine geometry (gm carries rstride, rdelta, roff)
  ScanTiles tiles;
  uint32_t nb;
  bool wide;
  size_t lds_coarse;                // k_sort_coarse
  size_t cache_n, chn, lds_fine;    // k_sort_fine
  uint32_t chunk, nthreads;         // k_accumulate
  int err;
};

inline SortPlan sort_plan(const MsmPlan& pl, const MsmShape& sh, int kmerge, int nch, size_t c0, size_t nc,
                          size_t stride) {
  const bool fixed = sh.fixed;
  SortPlan r{};
  r.c0 = c0;
  r.nc = nc;
  r.stride = stride;
  r.E = (size_t)kmerge * stride;  // entries of one sort row
  r.nW = (size_t)stride * pl.W;
  SortGeom& g = r.g;  // histogram geometry (blocks of scalars)
  g.FB = std::max(0, pl.cmax - 1 - 8);
  // the fixed-base MSM's merged sort rows are W x longer: 4x more coarse bins
  // once they exceed 2^24 entries (2^23, c = 20: FB 11 -> 9, sort 3.4 -> 2.3 ms)
  if (fixed && r.E > (size_t(1) << 24)) g.FB = std::max(0, pl.cmax - 1 - 10);
  g.NCB = (pl.K >> g.FB) + 1;
  // points per thread: blocks of 1024 threads x ppt points, ppt the largest
  // power of two <= 8 that still gives >= 128 blocks (2^20: 8192 points per
  // block; larger blocks give longer contiguous runs per coarse bin in
  // k_sort_coarse and a 4x smaller block histogram to scan: sort 0.19 ->
  // 0.16 ms at 2^20; small n keeps enough blocks)
  g.ppt = 1;
  while (g.ppt < kSortPerThread && stride >= (size_t)256 * g.ppt * kSortThreads) g.ppt *= 2;
  g.nblk = (int)((stride + (size_t)g.ppt * kSortThreads - 1) / ((size_t)g.ppt * kSortThreads));
  // The histogram pass is compute-bound per block (Montgomery -> canonical,
  // W signed digits and LDS atomics per scalar); with 8192-point blocks 2^20
  // gives 128 blocks for 256 CUs.  Split each coarse block's points over 2
  // histogram blocks when the grid is short of the CUs: the coarse pass keeps
  // its long runs and reads its start offsets at every hsub-th histogram
  // block.  The scan doubles with it, so one split only (same box, 2^20:
  // histogram 0.049-0.050 -> 0.035-0.041 ms, scan 0.014 -> 0.019 ms; below
  // 128 blocks the scan's growth cancels the gain: 2^19 +-0, 2^18 +3-5 us,
  // profiles/r02/hs/ab.txt and profiles/r02/p/ab.txt).
  int hsub = 1;
  if (g.ppt >= 2 && g.nblk >= 128 && g.nblk < 256) hsub = 2;
  g.hsub = 1;
  r.gm = g;         // coarse / fine geometry (blocks of sort-row entries)
  g.ppt /= hsub;    // histogram geometry
  g.nblk *= hsub;
  r.gm.nblk = g.nblk * kmerge;
  r.gm.hsub = hsub;
  r.TOTB = (size_t)pl.W * g.NCB * g.nblk + 1;
  r.tiles = scan_tiles((uint32_t)(pl.W * g.NCB), (uint32_t)g.nblk);  // k_sort_hist's layout
  r.nb = (uint32_t)((r.TOTB + r.tiles.chunk - 1) / r.tiles.chunk);
  // 4-B coarse entries when the entry index fits beside the fine bits and
  // the sign (a part's entries carry the full table's indices)
  const size_t imax = nch > 1 ? (size_t)kmerge * sh.npad : r.E;
  r.wide = imax > (size_t(1) << (31 - g.FB));
  // a part's entries carry table indices j npad + c0 + i (k_sort_coarse)
  r.gm.rstride = (uint32_t)stride;
  r.gm.rdelta = nch > 1 ? (uint32_t)(sh.npad - stride) : 0u;
  r.gm.roff = nch > 1 ? (uint32_t)c0 : 0u;
  // accumulation lanes: each part's own plan (~4 waves per SIMD; a part's
  // buckets reach as many slices as a full sort's).  The whole MSM's slice
  // length instead (fewer lanes, shorter chains) measured the same with
  // equal halves and 0.17 ms slower with a 3/8 first part (1.5 waves per
  // SIMD in its accumulation)
  r.chunk = nch > 1 ? make_plan_fixed(stride, sh.fixed_c, sh.min_chunk).chunk : pl.chunk;
  r.nthreads = nch > 1 ? (uint32_t)((r.nW + r.chunk - 1) / r.chunk) : pl.nthreads;
  const bool wide = r.wide;
  r.lds_coarse = (size_t)r.gm.ppt * kSortThreads * ((wide ? 8 : 4) + 2) + (size_t)(2 * g.NCB + 1) * 4 + (kSortThreads / 64 + 1) * 4;
  // fine sort LDS: segment cache + chunk buffer (k_sort_fine).  A mean
  // segment that fits 24 KiB is cached whole with room for 1.5x its size and
  // sorted as one chunk; larger ones are re-read from mid in 32 KiB chunks
  // (2 blocks per CU).  Sweep with 16-B loads (profiles/r03/sort_fine/): 16
  // KiB chunks 2^20 0.065 / 2^22 0.233 ms, 24-32 KiB 0.056 / 0.210, 40-64 KiB
  // (one block per CU) 0.064-0.074 / 0.256-0.288; the whole segment cached in
  // LDS (64-136 KiB) 0.069-0.107 / 0.34-0.44.  PM_FINE_CACHE_KB /
  // PM_FINE_CHUNK_KB override both (A/B).
  const size_t esz = wide ? 8 : 4;
  const size_t mean_seg = r.E / std::max(1, g.NCB - 1) + 1;
  const size_t fine_fixed = ((size_t)3 * (1 << g.FB) + kFineThreads / 64 + 1) * 4;  // hist, lcur, lst, scan
  size_t cache_n = (mean_seg * 3 / 2 + 63) & ~size_t(63), chn;
  if (cache_n * esz > 24576) cache_n = kFineChunkBytes / esz;
  chn = cache_n;
  if (sh.fine_cache_kb > 0) cache_n = ((size_t)sh.fine_cache_kb * 1024 / esz) & ~size_t(63);
  if (sh.fine_chunk_kb > 0) chn = ((size_t)sh.fine_chunk_kb * 1024 / esz) & ~size_t(63);
  chn = std::max<size_t>(64, std::min(chn, cache_n));
  cache_n = std::max(cache_n, chn);
  if (fine_fixed + 128 * esz > kMaxLds) {
    r.err = kPlanFineTooWide;
    return r;
  }
  while (cache_n > 64 && (cache_n + chn) * esz + fine_fixed > kMaxLds) {
    cache_n /= 2;
    chn = std::min(chn, cache_n);
  }
  r.cache_n = cache_n;
  r.chn = chn;
  r.lds_fine = (cache_n + chn) * esz + fine_fixed;
  return r;
}

// ------------------------------------------------------------- reduction
// Host terms per bucket set (NQ = NB2 + kTJobs + 1): the bit sums G_b at
// o + b + log2 L1, the kTJobs partial sums of T at o, the top bucket K at
// o + cmax - 1.
struct ReducePlan {
  int Wr;       // bucket sets (reduced windows)
  size_t TOT;   // bucket offsets of a sorted list: Wr * NB + 1
  int NJ;       // bit-sum jobs per set
  int NQ;       // host terms per set
  unsigned seg_blocks;  // k_bucket_seg_q
  int nsplit;           // k_bucket_bits blocks per job
};
inline ReducePlan reduce_plan(const MsmPlan& pl, int kmerge) {
  ReducePlan r;
  r.Wr = pl.W / kmerge;
  r.TOT = (size_t)r.Wr * pl.NB + 1;
  r.NJ = pl.NB2 + kTJobs;
  r.NQ = r.NJ + 1;
  // chains (long ones wave-cooperatively) + segment sums + the top bucket
  r.seg_blocks = (unsigned)((4ull * r.Wr * pl.M1 + 255) / 256);
  // bit sums of few sets (the row tables, the fixed-base MSM's one set) are
  // split over more blocks.  Every extra lane also adds one tree addition, so
  // the split stops at ~16 blocks per job (c = 20, 2^19 buckets: 16 -> 0.33
  // ms, 64 -> 0.47 ms; round 3, 16 / Wr against 4, 8, 32, 64 / Wr at 2^19 -
  // 2^22, resident and raw: profiles/r03/ab/bits_split_sweep.jsonl).
  r.nsplit = std::max(1, std::min(kMaxSplit, kBitsSplitK / r.Wr));
  return r;
}

// ------------------------------------------------------- one call's schedule
// The whole plan of one msm_device_impl call: a part's plan is computed once,
// into an array of kMaxParts on the caller's stack.
struct MsmSchedule {
  MsmPlan pl;
  int kmerge;  // windows merged into one bucket set (a table's rows), else 1
  bool d16;    // 2-B digit codes
  ReducePlan red;
  MsmParts parts;
  SortPlan part[kMaxParts];
  int err;     // the first part's refusal, kPlanOk otherwise
};
inline MsmSchedule msm_schedule(const MsmShape& sh) {
  MsmSchedule s{};
  s.pl = sh.fixed ? make_plan_fixed(sh.npad, sh.fixed_c, sh.min_chunk) : make_plan(sh.n, sh.window_c, sh.min_chunk);
  s.kmerge = sh.fixed ? sh.rows : 1;
  s.d16 = s.pl.cmax <= 16;
  s.red = reduce_plan(s.pl, s.kmerge);
  s.parts = msm_parts(sh.n, sh.fixed, sh.host_scalars, sh.split_copy);
  for (int ch = 0; ch < s.parts.nch; ch++) {
    const size_t c0 = s.parts.pstart[ch];
    s.part[ch] = sort_plan(s.pl, sh, s.kmerge, s.parts.nch, c0, s.parts.pstart[ch + 1] - c0,
                           part_stride(s.parts, ch, sh.n, sh.fixed, sh.npad));
    if (s.part[ch].err && !s.err) s.err = s.part[ch].err;
  }
  return s;
}

// ---------------------------------------------------------- small-MSM path
constexpr int kSmallWin = 33;          // 4-bit windows of a 128-bit GLV half (+ the carry window)
constexpr int kSmallQuads = 64;        // k_small_sum: quads per block
// k_small_fused up to here (one slice per window).  Several slices per window
// (one term per quad, the last block folding) measured slower than table + sum
// from 64 points on (64 / 128 / 256: 86.6-87.1 / 92.3-93.1 / 95.1-100.8 us
// against 83.4 / 89.0 / 95.1; profiles/r04/small/fused_ab.jsonl)
constexpr uint32_t kSmallFusedN = 32;
// slices per window: up to kSmallSlices blocks of 64 quads (or, from 4096
// terms, 256 lanes with one-lane additions), each adding kq terms serially.
// Measured (profiles/r04/small/ab.jsonl, n = 256 .. 8192, quads / lanes x
// 4 .. 32 slices): 8 slices best at every size, lanes ahead from n = 2048
// (121 vs 132 us; 4096: 138 vs 167 us), even at 1024.
constexpr uint32_t kSmallSlices = 8;
constexpr uint32_t kSmallLanesT = 4096;  // terms (2 n) from which k_small_sum_lanes runs
struct SmallPlan {
  bool fused;   // k_small_fused: one launch, one term per quad
  bool lanes;   // k_small_sum_lanes (else k_small_sum); read only when !fused
  uint32_t kq;  // terms per quad and slice
  uint32_t ns;  // slices per window
};
inline SmallPlan small_plan(size_t n) {
  const uint32_t un = (uint32_t)n, T = 2u * un;
  SmallPlan p;
  p.fused = un <= kSmallFusedN;
  p.lanes = T >= kSmallLanesT;
  const uint32_t per = p.lanes ? 256u : (uint32_t)kSmallQuads;  // terms per block and round
  p.kq = std::max<uint32_t>(1u, (T + per * kSmallSlices - 1) / (per * kSmallSlices));
  p.ns = (T + per * p.kq - 1) / (per * p.kq);
  if (p.fused) {  // one term per quad: 64 per slice
    p.kq = 1;
    p.ns = (T + kSmallQuads - 1) / kSmallQuads;
  }
  return p;
}

// ----------------------------------------------------------- many-MSM path
constexpr uint32_t kManyQuads = 64;          // quads per block (256 threads)
constexpr uint32_t kManyQuadBudget = 32768;  // quads in flight: ~2 waves per SIMD of the 1024
// geometry for a prefix of n bases: the widest window (fewest additions per
// scalar, W(c) of them) whose table fits kManyTabBudget; c = 4 up to the hard
// cap, beyond it pm_msm_resident_many falls back to one resident MSM each.
// W(c): signed digits in [-(2^(c-1) - 1), 2^(c-1)] of a scalar < 2^255 need a
// carry window only when c divides 255.
constexpr size_t kManyTabBudget = size_t(2) << 30;
constexpr size_t kManyTabCap = size_t(8) << 30;
inline uint32_t many_windows(uint32_t c) { return 255u % c == 0 ? 255u / c + 1u : (255u + c - 1u) / c; }
inline size_t many_bytes_per_base(uint32_t c) { return (size_t)many_windows(c) << (c - 1) << 7; }
inline uint32_t many_pick_c(size_t n) {
  for (uint32_t c = 8; c > 4; c--)
    if (n * many_bytes_per_base(c) <= kManyTabBudget) return c;
  return 4;
}
// terms per quad and slice of a call of total_entries = sum n_i W terms
inline uint32_t many_kq(size_t total_entries) {
  return (uint32_t)std::max<size_t>(1, (total_entries + kManyQuadBudget - 1) / kManyQuadBudget);
}

}  // namespace pm

// gp_kernels.hpp -- grand products over a scalar field: the
// running products Z of halo2's permutation argument
// (plonk/permutation/prover.rs::commit [3P]) and of every lookup
// (plonk/lookup/prover.rs::commit_product [3P]), and ff::BatchInvert, the step
// of create_proof (examples/simple-example.rs:663-710) between "columns on the
// device" and the commit to Z (pm_msm_fixed_device).
//
// Per set, with N[i] / D[i] the products of the numerator / denominator
// factors f[i] = x[i] + b y[i] + g of row i (rows i >= active - 1 count as 1):
//   z[i] = start * PN[i] * SD[i] * SD[0]^-1,
//   PN[i] = prod_{j < i} N[j]                 (exclusive prefix product),
//   SD[i] = prod_{i <= j < active-1} D'[j]    (inclusive suffix product),
// D' = D with zeros replaced by 1, and z[i] = 0 for every i past the first zero
// denominator (one atomicMin per set): one inversion per set, none per row or
// lane.  Batch inversion is the same machinery with N = D = a', the suffix
// exclusive: a[i]^-1 = P_excl[i] * S_excl[i] * total^-1, zeros staying zero.
//
// Launches, each on the context stream (no block ever waits on another):
//   k_gp_prep   per factor: b into the form its product needs; per list the
//     form constant K; the first-zero index of every set reset.
//   k_gp_local  grid (tiles, S), tiles of 2^11 rows.  N and D are formed row by
//     row from coalesced column loads (element k 256 + tid), omega^i from the
//     power table of omega (k_poly_table) with one product per row; each is
//     transposed through LDS so a lane owns a run of 8 consecutive rows, runs
//     its in-run prefix / suffix product, and goes back through LDS for a
//     coalesced store of the un-carried values (PN into the output row, SD
//     into scratch).  The 256 run aggregates are combined by a product scan in
//     LDS.  Out: per lane the exclusive prefix (N) / suffix (D) over the lanes
//     of the tile, per tile one (N, D) aggregate pair.
//   k_gp_carry  one block per set: exclusive prefix of the tile N aggregates,
//     exclusive suffix of the tile D aggregates, the set's total N and the
//     single inverse of its total D (f29_inv_q).
//   k_gp_chain  one lane: start or the previous set's last folded into each
//     set's scale, in set order; writes every `last`.
//   k_gp_sweep  per row: PN x SD x (lane carries x tile carries x scale),
//     canonical; zero past the first zero denominator; rows < active only.
//
// Arithmetic.  f29_mul_c(a, b) = a b 2^-261.  Columns, g and the output keep
// the caller's R = 2^256 Montgomery meaning ("data" form, x 2^256, unpacked
// into 29-bit limbs); every product of stored values lives in the pipeline's
// native R = 2^261 form (x 2^261), which is closed under f29_mul_c:
//   * a factor is x + y b + g in the data form: y (data) by b converted to the
//     native form, or omega^i (native, from the table) by b as given (data);
//   * a list of p factors is multiplied as (((f_1 K) f_2) ...) f_p with
//     K = 2^(5 p) in the native form (TO261 to the p-th), so the list's
//     product lands in the native form with p products and no conversion of
//     its own (data x data would be x 2^251);
//   * the set's scale carries TO256 = 2^-5, so PN x SD x scale is the data
//     form again.
// Bounds: an unpacked input is Norm, < 2^256 (< 5.4p); a product is Norm,
// < 2p; a factor's lazy sum (input + product + input) is < 12.8p with limbs
// < 3 2^29 and is normalised and reduced (f29_nr: < 16p -> Norm, < 3p) before
// it enters a product.  Every f29_mul_c here therefore takes two Norm operands
// below 6p (one of the shapes tests/test_fp29_asm.py pins); no new lazy
// operand shape arises.  Everything stored is Norm, < 2p (< 2^256, packable);
// the output and `last` are canonical.
#pragma once
#include "poly_kernels.hpp"

namespace pm {

constexpr uint32_t kGpNone = 0xFFFFFFFFu, kGpOmega = 0xFFFFFFFEu;  // PM_GP_NONE / PM_GP_OMEGA
constexpr uint32_t kGpNoZero = 0xFFFFFFFFu;                        // no zero denominator in the set
constexpr uint32_t kGpFactorWords = 18;                            // pm_gp_factor: x, y, b[8], g[8]

struct GpJob {
  const uint32_t* const* cols;  // device array of C column pointers
  const uint32_t* num;          // device factor table (b converted by k_gp_prep)
  const uint32_t* den;
  const uint32_t* num_off;      // S + 1
  const uint32_t* den_off;      // S + 1
  const uint32_t* kform;        // per set: K of the numerator list, K of the denominator list
  const uint32_t* tab;          // power table of omega (nullptr: no factor names it)
  uint32_t S;
  uint32_t nblk;                // tiles per set
  uint32_t invert;              // batch inversion: N = D, exclusive suffix, zeros stay zero
  size_t n;
  size_t prod_rows;             // rows entering the products: active - 1 (inversion: n)
  size_t store_rows;            // rows written: active (inversion: n)
};

template <class Fs>
__device__ __forceinline__ F29<Fs> gp_one() {
  return f29_const<Fs>(F29Consts<Fs>::ONE);
}
// 8 words at any 4-byte alignment (the factor table)
template <class Fs>
__device__ __forceinline__ F29<Fs> gp_ldw(const uint32_t* __restrict__ p) {
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = p[k];
  return f29_unpack<Fs>(w);
}
template <class Fs>
__device__ __forceinline__ void gp_stw(uint32_t* p, const F29<Fs>& v) {  // v Norm, < 2^256
  uint32_t w[8];
  f29_pack<Fs>(v, w);
#pragma unroll
  for (int k = 0; k < 8; k++) p[k] = w[k];
}

// threads [0, F): factor t of the uploaded lists (numerators first), b -> the
// native form when y is a column; threads [F, F + 2 S): K of list t - F
// (numerator lists, then denominator lists); threads < S reset zidx.
template <class Fs>
__global__ void __launch_bounds__(256) k_gp_prep(const uint32_t* __restrict__ fac_in, uint32_t* __restrict__ fac_out,
                                                 uint32_t F, const uint32_t* __restrict__ num_off,
                                                 const uint32_t* __restrict__ den_off, uint32_t S,
                                                 uint32_t* __restrict__ kform, uint32_t* __restrict__ zidx) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < S) zidx[t] = kGpNoZero;
  if (t < F) {
    const uint32_t* in = fac_in + (size_t)t * kGpFactorWords;
    uint32_t* out = fac_out + (size_t)t * kGpFactorWords;
    const uint32_t y = in[1];
    out[0] = in[0];
    out[1] = y;
    uint32_t b[8];
#pragma unroll
    for (int k = 0; k < 8; k++) b[k] = in[2 + k];
    if (y != kGpNone && y != kGpOmega) {
      gp_stw<Fs>(out + 2, f29_from_r256<Fs>(b));
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) out[2 + k] = b[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) out[10 + k] = in[10 + k];
  } else if (t < F + 2 * S) {
    const uint32_t l = t - F, j = l < S ? l : l - S;
    const uint32_t* off = l < S ? num_off : den_off;
    const uint32_t p = off[j + 1] - off[j];
    const F29<Fs> c = f29_const<Fs>(F29Consts<Fs>::TO261);
    F29<Fs> k = c;
    for (uint32_t i = 1; i < p; i++) k = f29_mul_c<Fs>(k, c);
    gp_stw<Fs>(kform + ((size_t)2 * j + (l < S ? 0 : 1)) * 8, k);
  }
}

// product of the factors [lo, hi) at row i, native form (Norm, < 2p); w = omega^i
template <class Fs>
__device__ __forceinline__ F29<Fs> gp_row_product(const GpJob& jb, const uint32_t* __restrict__ fac, uint32_t lo,
                                                  uint32_t hi, const F29<Fs>& K, size_t i, const F29<Fs>& w) {
  F29<Fs> acc = gp_one<Fs>();
  for (uint32_t f = lo; f < hi; f++) {
    const uint32_t* fp = fac + (size_t)f * kGpFactorWords;
    const uint32_t x = fp[0], y = fp[1];
    F29<Fs> t = gp_ldw<Fs>(fp + 10);
    if (x != kGpNone) t = f29_add<Fs>(t, g_ld29<Fs>(jb.cols[x], i));
    if (y == kGpOmega)
      t = f29_add<Fs>(t, f29_mul_c<Fs>(w, gp_ldw<Fs>(fp + 2)));
    else if (y != kGpNone)
      t = f29_add<Fs>(t, f29_mul_c<Fs>(g_ld29<Fs>(jb.cols[y], i), gp_ldw<Fs>(fp + 2)));
    t = f29_nr<Fs>(t);
    acc = f == lo ? f29_mul_c<Fs>(t, K) : f29_mul_c<Fs>(acc, t);
  }
  return acc;
}

// Product scan over the block's 256 lanes (x Norm, < 2p): prefix, x becomes
// prod_{l' <= l} x_l'; suffix, prod_{l' >= l}.  *excl receives the neighbour's
// value (1 at the open end), *total the product of all lanes.  All lanes of
// the block call it; sm (kPolyScanLds) is free on entry and on return.
template <class Fs, bool kSuffix>
__device__ __forceinline__ void gp_lane_scan(uint32_t* sm, F29<Fs> x, F29<Fs>* excl, F29<Fs>* total) {
  const uint32_t l = threadIdx.x;
  for (int s = 0; s < 8; s++) {
    const uint32_t d = 1u << s;
    scan_st<Fs>(sm, l, x);
    __syncthreads();
    if (kSuffix ? l + d < (uint32_t)kPolyThreads : l >= d)
      x = f29_mul_c<Fs>(x, scan_ld<Fs>(sm, kSuffix ? l + d : l - d));
    __syncthreads();
  }
  scan_st<Fs>(sm, l, x);
  __syncthreads();
  if (kSuffix)
    *excl = l + 1 < (uint32_t)kPolyThreads ? scan_ld<Fs>(sm, l + 1) : gp_one<Fs>();
  else
    *excl = l ? scan_ld<Fs>(sm, l - 1) : gp_one<Fs>();
  *total = scan_ld<Fs>(sm, kSuffix ? 0u : (uint32_t)kPolyThreads - 1u);
  __syncthreads();
}

// coalesced store of the tile in LDS: rows [base, base + 2^11) below `rows`
__device__ __forceinline__ void gp_tile_out(const uint32_t* sm, uint32_t* row, size_t base, size_t rows) {
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kPolyRun; k++) {
    const uint32_t idx = k * kPolyThreads + tid;
    const size_t i = base + idx;
    if (i < rows) {
      const uint32_t p = tile_pos(idx);
      uint4 a, c;
      a.x = sm[0 * kPolyTilePlane + p], a.y = sm[1 * kPolyTilePlane + p];
      a.z = sm[2 * kPolyTilePlane + p], a.w = sm[3 * kPolyTilePlane + p];
      c.x = sm[4 * kPolyTilePlane + p], c.y = sm[5 * kPolyTilePlane + p];
      c.z = sm[6 * kPolyTilePlane + p], c.w = sm[7 * kPolyTilePlane + p];
      uint4* o = reinterpret_cast<uint4*>(row + 8ull * i);
      o[0] = a;
      o[1] = c;
    }
  }
}

// omega^(tile base + tid); row k 256 + tid takes one more product by omega^(256 k)
template <class Fs>
__device__ __forceinline__ F29<Fs> gp_omega_lane(const GpJob& jb, uint32_t blk) {
  const uint32_t tid = threadIdx.x;
  if (!jb.tab) return gp_one<Fs>();
  return f29_mul_c<Fs>(f29_mul_c<Fs>(poly_tab_pow<Fs>(jb.tab, blk, kPolyTileLog), g_ld29<Fs>(jb.tab, kPolyTabZ8 + (tid >> 3))),
                       g_ld29<Fs>(jb.tab, kPolyTabZj + (tid & 7u)));
}

// The denominators' pass of tile blk of set j: D row by row (coalesced),
// through LDS to the runs, the suffix product within each run (zeros count as
// 1), and back into LDS: on return (after its last barrier) sm holds the
// tile's un-carried SD.  Returns the run's aggregate.  The set's first zero
// denominator is recorded in zidx (not for the inversion, whose zeros stay
// zero: their rows get 0 instead of the running product).
template <class Fs>
__device__ __forceinline__ F29<Fs> gp_den_pass(const GpJob& jb, uint32_t* sm, uint32_t blk, uint32_t j,
                                               const F29<Fs>& w0, uint32_t* zidx) {
  const uint32_t tid = threadIdx.x;
  const size_t base = (size_t)blk << kPolyTileLog;
  F29<Fs> a[kPolyRun];
  {
    const uint32_t lo = jb.den_off[j], hi = jb.den_off[j + 1];
    const F29<Fs> K = gp_ldw<Fs>(jb.kform + ((size_t)2 * j + 1) * 8);
    uint32_t zmin = kGpNoZero;
#pragma unroll
    for (int k = 0; k < kPolyRun; k++) {
      const uint32_t idx = k * kPolyThreads + tid;
      const size_t i = base + idx;
      F29<Fs> v = gp_one<Fs>();
      if (i < jb.prod_rows) {
        const F29<Fs> w = jb.tab && k ? f29_mul_c<Fs>(w0, g_ld29<Fs>(jb.tab, kPolyTabZ8 + 32u * k)) : w0;
        v = gp_row_product<Fs>(jb, jb.den, lo, hi, K, i, w);
        if (f29_is_zero_mod<Fs>(v)) {
          if (jb.invert) {
            v = f29_zero<Fs>();  // flag for the run's owner: counts as 1, stays 0
          } else {
            zmin = min(zmin, (uint32_t)i);
            v = gp_one<Fs>();
          }
        }
      }
      tile_st<Fs>(sm, idx, v);
    }
    if (zmin != kGpNoZero) atomicMin(zidx + j, zmin);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kPolyRun; r++) a[r] = tile_ld<Fs>(sm, tid * kPolyRun + r);
  F29<Fs> sdl = gp_one<Fs>();
  if (jb.invert) {
#pragma unroll
    for (int r = kPolyRun - 1; r >= 0; r--) {
      const F29<Fs> t = a[r];
      const bool z = f29_is_zero_exact<Fs>(t);
      a[r] = z ? t : sdl;
      if (!z) sdl = f29_mul_c<Fs>(sdl, t);
    }
  } else {
    sdl = a[kPolyRun - 1];
#pragma unroll
    for (int r = kPolyRun - 2; r >= 0; r--) {
      sdl = f29_mul_c<Fs>(sdl, a[r]);
      a[r] = sdl;
    }
  }
#pragma unroll
  for (int r = 0; r < kPolyRun; r++) tile_st<Fs>(sm, tid * kPolyRun + r, a[r]);
  __syncthreads();
  return sdl;
}

// grid (nblk, S), kPolyDivLds bytes of LDS.  out: S rows of n (un-carried PN,
// rows < store_rows); sd: S rows of n (un-carried SD); lane_n / lane_d:
// S nblk 256 lane carries; agg: S nblk (N, D) pairs.  With jb.invert the one
// column is `out` itself: a block reads its tile before it writes it.
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_gp_local(GpJob jb, uint32_t* out, uint32_t* __restrict__ sd,
                                                           uint32_t* __restrict__ lane_n,
                                                           uint32_t* __restrict__ lane_d, uint32_t* __restrict__ agg,
                                                           uint32_t* __restrict__ zidx) {
  extern __shared__ uint32_t sm[];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, j = blockIdx.y;
  const size_t n = jb.n, base = (size_t)blk << kPolyTileLog;
  uint32_t* row = out + (size_t)j * n * 8;
  const F29<Fs> w0 = gp_omega_lane<Fs>(jb, blk);
  F29<Fs> a[kPolyRun];

  // ---- denominators.  First, so that the inversion, whose column is the
  // output row, has read its tile for both passes before the numerators' pass
  // overwrites it (the second read below comes before this block's first
  // store to `out`)
  const F29<Fs> sdl = gp_den_pass<Fs>(jb, sm, blk, j, w0, zidx);
  gp_tile_out(sm, sd + (size_t)j * n * 8, base, jb.store_rows);
  __syncthreads();

  // ---- numerators: exclusive prefix product within the run
  {
    const uint32_t lo = jb.num_off[j], hi = jb.num_off[j + 1];
    const F29<Fs> K = gp_ldw<Fs>(jb.kform + (size_t)2 * j * 8);
#pragma unroll
    for (int k = 0; k < kPolyRun; k++) {
      const uint32_t idx = k * kPolyThreads + tid;
      const size_t i = base + idx;
      F29<Fs> v = gp_one<Fs>();
      if (i < jb.prod_rows) {
        const F29<Fs> w = jb.tab && k ? f29_mul_c<Fs>(w0, g_ld29<Fs>(jb.tab, kPolyTabZ8 + 32u * k)) : w0;
        v = gp_row_product<Fs>(jb, jb.num, lo, hi, K, i, w);
        if (jb.invert && f29_is_zero_mod<Fs>(v)) v = gp_one<Fs>();
      }
      tile_st<Fs>(sm, idx, v);
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kPolyRun; r++) a[r] = tile_ld<Fs>(sm, tid * kPolyRun + r);
  F29<Fs> pn = a[0];
  a[0] = gp_one<Fs>();
#pragma unroll
  for (int r = 1; r < kPolyRun; r++) {
    const F29<Fs> t = a[r];
    a[r] = pn;
    pn = f29_mul_c<Fs>(pn, t);
  }
#pragma unroll
  for (int r = 0; r < kPolyRun; r++) tile_st<Fs>(sm, tid * kPolyRun + r, a[r]);
  __syncthreads();
  gp_tile_out(sm, row, base, jb.store_rows);
  __syncthreads();

  // ---- run aggregates -> carries into each run from the other lanes of the tile
  const size_t tile = (size_t)j * jb.nblk + blk;
  F29<Fs> excl, total;
  gp_lane_scan<Fs, false>(sm, pn, &excl, &total);
  g_st29<Fs>(lane_n, tile * kPolyThreads + tid, excl);
  if (tid == 0) g_st29<Fs>(agg, 2 * tile, total);
  gp_lane_scan<Fs, true>(sm, sdl, &excl, &total);
  g_st29<Fs>(lane_d, tile * kPolyThreads + tid, excl);
  if (tid == 0) g_st29<Fs>(agg, 2 * tile + 1, total);
}

// grid S.  carry: S nblk (N, D) pairs; setv: per set [total N, 1 / total D, scale]
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_gp_carry(GpJob jb, const uint32_t* __restrict__ agg,
                                                           uint32_t* __restrict__ carry,
                                                           uint32_t* __restrict__ setv) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t tid = threadIdx.x, j = blockIdx.x, count = jb.nblk;
  const uint32_t* vals = agg + (size_t)j * count * 16;
  uint32_t* cj = carry + (size_t)j * count * 16;
  const uint32_t chunk = (count + kPolyThreads - 1) / kPolyThreads;
  const uint32_t lo = min(count, tid * chunk), hi = min(count, lo + chunk);
  F29<Fs> excl, total_n, total_d;
  {
    F29<Fs> g = gp_one<Fs>();
    for (uint32_t b = lo; b < hi; b++) g = f29_mul_c<Fs>(g, g_ld29<Fs>(vals, 2ull * b));
    gp_lane_scan<Fs, false>(sm, g, &excl, &total_n);
    F29<Fs> c = excl;
    for (uint32_t b = lo; b < hi; b++) {
      g_st29<Fs>(cj, 2ull * b, c);
      c = f29_mul_c<Fs>(c, g_ld29<Fs>(vals, 2ull * b));
    }
  }
  {
    F29<Fs> g = gp_one<Fs>();
    for (uint32_t b = hi; b > lo; b--) g = f29_mul_c<Fs>(g, g_ld29<Fs>(vals, 2ull * (b - 1) + 1));
    gp_lane_scan<Fs, true>(sm, g, &excl, &total_d);
    F29<Fs> c = excl;
    for (uint32_t b = hi; b > lo; b--) {
      g_st29<Fs>(cj, 2ull * (b - 1) + 1, c);
      c = f29_mul_c<Fs>(c, g_ld29<Fs>(vals, 2ull * (b - 1) + 1));
    }
  }
  const F29<Fs> inv = f29_inv_q<Fs>(total_d);  // every quad of the block, the same input
  if (tid == 0) {
    g_st29<Fs>(setv, 3ull * j, total_n);
    g_st29<Fs>(setv, 3ull * j + 1, inv);
  }
}

// one lane: the chain over the sets.  start_w: `start` as given (R = 2^256,
// packed; unused by the inversion, which starts from 1); last_out: S x 8 words
template <class Fs>
__global__ void k_gp_chain(GpJob jb, const uint32_t* __restrict__ start_w, uint32_t chain,
                           const uint32_t* __restrict__ zidx, uint32_t* __restrict__ setv,
                           uint32_t* __restrict__ last_out) {
  if (blockIdx.x || threadIdx.x) return;
  const F29<Fs> to256 = f29_const<Fs>(F29Consts<Fs>::TO256);
  F29<Fs> first = gp_one<Fs>();
  if (!jb.invert) {
    uint32_t w[8];
#pragma unroll
    for (int k = 0; k < 8; k++) w[k] = start_w[k];
    first = f29_from_r256<Fs>(w);
  }
  F29<Fs> cur = first;
  for (uint32_t j = 0; j < jb.S; j++) {
    if (!chain) cur = first;
    const F29<Fs> inv = g_ld29<Fs>(setv, 3ull * j + 1);
    const F29<Fs> s = f29_mul_c<Fs>(cur, inv);
    g_st29<Fs>(setv, 3ull * j + 2, f29_mul_c<Fs>(s, to256));
    F29<Fs> last = f29_zero<Fs>();
    if (zidx[j] == kGpNoZero) last = f29_mul_c<Fs>(s, g_ld29<Fs>(setv, 3ull * j));
    g_st29<Fs>(last_out, j, f29_canon<Fs>(f29_mul_c<Fs>(last, to256)));
    cur = last;
  }
}

// grid (nblk, S)
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_gp_sweep(GpJob jb, uint32_t* out, const uint32_t* __restrict__ sd,
                                                           const uint32_t* __restrict__ lane_n,
                                                           const uint32_t* __restrict__ lane_d,
                                                           const uint32_t* __restrict__ carry,
                                                           const uint32_t* __restrict__ setv,
                                                           const uint32_t* __restrict__ zidx) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, j = blockIdx.y;
  const size_t n = jb.n, base = (size_t)blk << kPolyTileLog;
  if (base >= jb.store_rows) return;
  uint32_t* row = out + (size_t)j * n * 8;
  const uint32_t* sdrow = sd + (size_t)j * n * 8;
  const size_t tile = (size_t)j * jb.nblk + blk;
  {
    // what every row of this lane's run is multiplied by
    const F29<Fs> ln = f29_mul_c<Fs>(g_ld29<Fs>(lane_n, tile * kPolyThreads + tid), g_ld29<Fs>(carry, 2 * tile));
    const F29<Fs> ld = f29_mul_c<Fs>(g_ld29<Fs>(lane_d, tile * kPolyThreads + tid), g_ld29<Fs>(carry, 2 * tile + 1));
    scan_st<Fs>(sm, tid, f29_mul_c<Fs>(f29_mul_c<Fs>(ln, ld), g_ld29<Fs>(setv, 3ull * j + 2)));
  }
  __syncthreads();
  const uint32_t zi = zidx[j];
#pragma unroll
  for (int k = 0; k < kPolyRun; k++) {
    const uint32_t idx = k * kPolyThreads + tid;
    const size_t i = base + idx;
    if (i >= jb.store_rows) continue;
    F29<Fs> val = f29_zero<Fs>();
    if (i <= (size_t)zi)
      val = f29_canon<Fs>(f29_mul_c<Fs>(f29_mul_c<Fs>(g_ld29<Fs>(row, i), g_ld29<Fs>(sdrow, i)),
                                         scan_ld<Fs>(sm, idx / kPolyRun)));
    g_st29<Fs>(row, i, val);
  }
}

}  // namespace pm

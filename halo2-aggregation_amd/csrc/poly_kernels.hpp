// poly_kernels.hpp -- polynomial openings over a scalar field:
// halo2's `eval_polynomial(a, x)` and `kate_division(a, z)` (arithmetic.rs
// [3P]) and the GWC prover's witness polynomials
//   q_j = kate_division(sum_i v^{m_j-1-i} p_{j,i}, z_j)
// (poly/multiopen/gwc/prover.rs [3P]), the step of create_proof
// (examples/simple-example.rs:606,702) between "coefficients on the device"
// (pm_fft_device) and the commits (pm_msm_resident_device).
//
// Division is a suffix scan.  With c_t = sum_{s >= t} a_s z^{s-t} the quotient
// is q_{t-1} = c_t (t = 1 .. n-1) and c_0 = a(z) is the remainder, and
// c_t = a_t + z c_{t+1} composes as affine maps c -> H + z^L c.  Three phases,
// each its own launch on the context stream (no block ever waits on another):
//   k_poly_div_local  one block per tile of 2^11 coefficients: forms the batch
//     polynomial of the tile in registers (Horner in v over the set's
//     polynomials, coalesced loads; it is never written to HBM), transposes it
//     through LDS so every lane owns a run of 8 consecutive coefficients, runs
//     the z recurrence over the run, stores the un-carried values (coalesced,
//     through LDS again), and combines the 256 run aggregates with powers of
//     z^8 (a suffix scan in LDS).  Out: per lane the carry into its run from
//     the lanes above it in the tile, per tile one aggregate.
//   k_poly_div_carry  one block per set: suffix scan of the tile aggregates
//     with z^2048 (a run of tiles per lane, the same LDS scan across lanes).
//   k_poly_div_sweep  per tile: carry of a lane = its in-tile carry + z^(8 x
//     lanes above) x the tile's carry; every element adds carry x z^distance
//     and is canonicalised.
// Products per coefficient: m - 1 (v) + 1 (z) + 1 (LDS scan, 8 steps per run
// of 8) + 1 (sweep) + 1/8.
//
// Evaluation: lane l of a tile of 2^12 coefficients takes t = l mod 256
// (coalesced), Horner in z^256 over its 16 coefficients, times z^l, summed
// over the block in LDS; a second launch combines the tile values with powers
// of z^4096.  One product per coefficient.
//
// Arithmetic as in the NTT (ntt_kernels.hpp): data keeps the caller's
// R = 2^256 Montgomery meaning unpacked into 29-bit limbs, multipliers (powers
// of z, v) are canonical in the R = 2^261 form, so data x multiplier x 2^-261
// stays in the data's form.  Bounds: an unpacked input is Norm, < 2^256
// (< 5.4p); a product is Norm, < 2p; `input + product` has limbs < 2^30 and
// is < 8p, a legal lazy first operand of f29_mul_c (< 9p, limbs < 2^30, by a
// Norm multiplier < 2p: tests/test_fp29_asm.py::test_ntt_operand_bounds), so
// the Horner recurrences carry no normalisation; everything stored is
// normalised and reduced to < 3p (< 2^256, packable), final values canonical.
#pragma once
#include "ntt_kernels.hpp"

namespace pm {

constexpr int kPolyThreads = 256;
constexpr int kPolyRun = 8;                              // coefficients per lane (division)
constexpr uint32_t kPolyTile = kPolyThreads * kPolyRun;  // 2^11
constexpr int kPolyTileLog = 11;
constexpr int kPolyEvalRun = 16;                         // coefficients per lane (evaluation)
constexpr uint32_t kPolyEvalTile = kPolyThreads * kPolyEvalRun;  // 2^12
constexpr int kPolyEvalTileLog = 12;
// Power table of one point (R = 2^261, canonical, packed), kPolyTabStride
// entries: [k] = z^(2^k), k <= 28; [kPolyTabZ8 + l] = z^(8 l), l <= 256;
// [kPolyTabZj + j] = z^j, j <= 8.
constexpr uint32_t kPolyTabZ8 = 32, kPolyTabZj = 292, kPolyTabStride = 304;
// packed tile in LDS: 8 word planes, position idx at idx + idx / 8 (a lane's
// run of 8 then starts 9 words after its neighbour's: no bank conflicts)
constexpr uint32_t kPolyTilePlane = kPolyTile + kPolyTile / 8;
constexpr size_t kPolyDivLds = (size_t)kPolyTilePlane * 8 * 4;
constexpr size_t kPolyScanLds = (size_t)kPolyThreads * 9 * 4;

// k_poly_table: one block per point (R = 2^256 Montgomery, packed).  Only
// z^(2^k) for k < nsq is built (12 <= nsq <= 29: the chain of squarings is the
// kernel's whole latency, and a call reads no further than poly_table_squarings).
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_table(const uint32_t* __restrict__ pts, uint32_t npts,
                                                             uint32_t nsq, uint32_t* __restrict__ tab) {
  __shared__ uint32_t p2[29 * 8];
  const uint32_t pt = blockIdx.x, tid = threadIdx.x;
  if (pt >= npts) return;
  uint32_t* out = tab + (size_t)pt * kPolyTabStride * 8;
  auto put = [&](uint32_t slot, const Fe<Fs>& r) {
    Fe<Fs> o;
    f29_pack<Fs>(f29_canon<Fs>(f29_from_r256<Fs>(r.l)), o.l);
    store_fe4<Fs>(reinterpret_cast<uint4*>(out + 8ull * slot), o);
  };
  if (tid < nsq) {
    Fe<Fs> b = load_fe4<Fs>(reinterpret_cast<const uint4*>(pts + 8ull * pt));
    for (uint32_t i = 0; i < tid; i++) b = fe_sqr<Fs>(b);
#pragma unroll
    for (int k = 0; k < 8; k++) p2[tid * 8 + k] = b.l[k];
    put(tid, b);
  }
  __syncthreads();
  auto power = [&](uint32_t e, int k0) {  // z^(e 2^k0), e < 2^9
    Fe<Fs> r = fe_one<Fs>();
    for (int bit = 0; bit < 9; bit++) {
      if (!((e >> bit) & 1u)) continue;
      Fe<Fs> b;
#pragma unroll
      for (int k = 0; k < 8; k++) b.l[k] = p2[(k0 + bit) * 8 + k];
      r = fe_mul<Fs>(r, b);
    }
    return r;
  };
  for (uint32_t l = tid; l <= 256; l += kPolyThreads) put(kPolyTabZ8 + l, power(l, 3));
  if (tid <= 8) put(kPolyTabZj + tid, power(tid, 0));
}

// entries [0, nsq) a call over `count` tiles of 2^k0 coefficients reads: the
// z^8 .. z^2048 of the in-tile scan and the z^(8 l) table (k <= 11), and
// poly_block_scan's z^(2^k0 x chunk) (poly_tab_pow: one entry per bit of chunk)
inline uint32_t poly_table_squarings(uint32_t count, int k0) {
  uint32_t chunk = (count + kPolyThreads - 1) / kPolyThreads, bits = 0;
  for (; chunk; chunk >>= 1) bits++;
  const uint32_t need = (uint32_t)k0 + bits;
  return need < 12u ? 12u : (need > 29u ? 29u : need);
}

// scan area: 9 limb planes of 256 words
template <class Fs>
__device__ __forceinline__ F29<Fs> scan_ld(const uint32_t* sm, uint32_t l) {
  F29<Fs> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.l[k] = sm[k * kPolyThreads + l];
  return r;
}
template <class Fs>
__device__ __forceinline__ void scan_st(uint32_t* sm, uint32_t l, const F29<Fs>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) sm[k * kPolyThreads + l] = v.l[k];
}

// Suffix scan over the block's 256 lanes: x (Norm, < 3p) becomes
// sum_{l' >= l} x_{l'} W^(l' - l); *excl receives the value of lane l + 1
// (zero for the last lane).  Step s multiplies by W^(2^s): read from the
// point's table at [k0 + s] when tab != nullptr (W = z^(2^k0)), else squared
// from w.  All lanes of the block call it; sm (kPolyScanLds) is free on entry.
template <class Fs>
__device__ __forceinline__ F29<Fs> poly_suffix_scan(uint32_t* sm, F29<Fs> x, F29<Fs> w,
                                                    const uint32_t* __restrict__ tab, int k0, F29<Fs>* excl) {
  const uint32_t l = threadIdx.x;
  for (int s = 0; s < 8; s++) {
    const uint32_t d = 1u << s;
    scan_st<Fs>(sm, l, x);
    __syncthreads();
    if (tab) w = g_ld29<Fs>(tab, (size_t)(k0 + s));
    if (l + d < (uint32_t)kPolyThreads) x = f29_nr<Fs>(f29_add<Fs>(x, f29_mul_c<Fs>(scan_ld<Fs>(sm, l + d), w)));
    __syncthreads();
    if (!tab) w = f29_sqr_c<Fs>(w);
  }
  scan_st<Fs>(sm, l, x);
  __syncthreads();
  *excl = l + 1 < (uint32_t)kPolyThreads ? scan_ld<Fs>(sm, l + 1) : f29_zero<Fs>();
  __syncthreads();
  return x;
}

__device__ __forceinline__ uint32_t tile_pos(uint32_t idx) { return idx + (idx >> 3); }
template <class Fs>
__device__ __forceinline__ void tile_st(uint32_t* sm, uint32_t idx, const F29<Fs>& v) {  // v Norm, < 2^256
  uint32_t w[8];
  f29_pack<Fs>(v, w);
  const uint32_t p = tile_pos(idx);
#pragma unroll
  for (int k = 0; k < 8; k++) sm[k * kPolyTilePlane + p] = w[k];
}
template <class Fs>
__device__ __forceinline__ F29<Fs> tile_ld(const uint32_t* sm, uint32_t idx) {
  uint32_t w[8];
  const uint32_t p = tile_pos(idx);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = sm[k * kPolyTilePlane + p];
  return f29_unpack<Fs>(w);
}

// where c_t lives in the output row: q_{t-1}; c_0 is parked in the row's last
// element until the sweep moves it to the evaluations and writes the zero
__device__ __forceinline__ size_t poly_slot(size_t t, size_t n) { return t ? t - 1 : n - 1; }

struct PolyJob {
  const uint32_t* const* polys;  // device array of P pointers
  const uint32_t* set_offsets;   // S + 1
  const uint32_t* set_polys;
  const uint32_t* tab;           // S point tables, then v's
  uint32_t S;
  uint32_t nblk;                 // tiles per polynomial
  size_t n;
};

// grid (nblk, S), kPolyDivLds bytes of LDS
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_div_local(PolyJob jb, uint32_t* __restrict__ out,
                                                                 uint32_t* __restrict__ lane_carry,
                                                                 uint32_t* __restrict__ agg) {
  extern __shared__ uint32_t sm[];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, j = blockIdx.y;
  const size_t n = jb.n, base = (size_t)blk << kPolyTileLog;
  const uint32_t lo = jb.set_offsets[j], m = jb.set_offsets[j + 1] - lo;
  const uint32_t* tabj = jb.tab + (size_t)j * kPolyTabStride * 8;
  uint32_t* row = out + (size_t)j * n * 8;
  {
    // batch polynomial of the tile: b = p_0, then b = b v + p_i
    const F29<Fs> v = g_ld29<Fs>(jb.tab + (size_t)jb.S * kPolyTabStride * 8, 0);
    F29<Fs> b[kPolyRun];
    const uint32_t* p = jb.polys[jb.set_polys[lo]];
#pragma unroll
    for (int k = 0; k < kPolyRun; k++) {
      const size_t t = base + (size_t)k * kPolyThreads + tid;
      b[k] = t < n ? g_ld29<Fs>(p, t) : f29_zero<Fs>();
    }
    for (uint32_t i = 1; i < m; i++) {
      p = jb.polys[jb.set_polys[lo + i]];
#pragma unroll
      for (int k = 0; k < kPolyRun; k++) {
        const size_t t = base + (size_t)k * kPolyThreads + tid;
        if (t < n) b[k] = f29_add<Fs>(g_ld29<Fs>(p, t), f29_mul_c<Fs>(b[k], v));
      }
    }
#pragma unroll
    for (int k = 0; k < kPolyRun; k++) tile_st<Fs>(sm, k * kPolyThreads + tid, m > 1 ? f29_nr<Fs>(b[k]) : b[k]);
  }
  __syncthreads();
  // the z recurrence over this lane's run, top down; un-carried values in place
  const F29<Fs> z = g_ld29<Fs>(tabj, 0);
  F29<Fs> h = f29_zero<Fs>();
#pragma unroll
  for (int r = kPolyRun - 1; r >= 0; r--) {
    h = f29_add<Fs>(tile_ld<Fs>(sm, tid * kPolyRun + r), f29_mul_c<Fs>(h, z));
    tile_st<Fs>(sm, tid * kPolyRun + r, f29_nr<Fs>(h));
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPolyRun; k++) {
    const uint32_t idx = k * kPolyThreads + tid;
    const size_t t = base + idx;
    if (t < n) {
      const uint32_t p = tile_pos(idx);
      uint4 a, c;
      a.x = sm[0 * kPolyTilePlane + p], a.y = sm[1 * kPolyTilePlane + p];
      a.z = sm[2 * kPolyTilePlane + p], a.w = sm[3 * kPolyTilePlane + p];
      c.x = sm[4 * kPolyTilePlane + p], c.y = sm[5 * kPolyTilePlane + p];
      c.z = sm[6 * kPolyTilePlane + p], c.w = sm[7 * kPolyTilePlane + p];
      uint4* o = reinterpret_cast<uint4*>(row + 8ull * poly_slot(t, n));
      o[0] = a;
      o[1] = c;
    }
  }
  __syncthreads();
  // run aggregates -> carry into each run from the lanes above (W = z^8)
  F29<Fs> excl;
  const F29<Fs> incl = poly_suffix_scan<Fs>(sm, f29_nr<Fs>(h), z, tabj, 3, &excl);
  const size_t tile = (size_t)j * jb.nblk + blk;
  g_st29<Fs>(lane_carry, tile * kPolyThreads + tid, excl);
  if (tid == 0) g_st29<Fs>(agg, tile, incl);
}

// z^(e 2^k0) from the point's table (R261, Norm, < 2p); e 2^k0 < 2^29
template <class Fs>
__device__ __forceinline__ F29<Fs> poly_tab_pow(const uint32_t* __restrict__ tab, uint32_t e, int k0) {
  F29<Fs> r = f29_const<Fs>(F29Consts<Fs>::ONE);
  for (int bit = 0; e; bit++, e >>= 1)
    if (e & 1u) r = f29_mul_c<Fs>(r, g_ld29<Fs>(tab, (size_t)(k0 + bit)));
  return r;
}

// Suffix scan of `count` values with multiplier z^(2^k0), one block: vals[b]
// (Norm, < 3p, packed) for b < count.  Lane l takes the run [l chunk,
// (l + 1) chunk).  carry != nullptr: carry[b] = sum_{b' > b} vals[b']
// W^(b' - b - 1).  Returns (lane 0) the inclusive total sum_b vals[b] W^b.
template <class Fs>
__device__ __forceinline__ F29<Fs> poly_block_scan(uint32_t* sm, const uint32_t* __restrict__ vals, uint32_t count,
                                                   const uint32_t* __restrict__ tab, int k0,
                                                   uint32_t* __restrict__ carry) {
  const uint32_t tid = threadIdx.x;
  const uint32_t chunk = (count + kPolyThreads - 1) / kPolyThreads;
  const uint32_t lo = min(count, tid * chunk), hi = min(count, lo + chunk);
  const F29<Fs> w = g_ld29<Fs>(tab, (size_t)k0);
  F29<Fs> g = f29_zero<Fs>();
  for (uint32_t b = hi; b > lo; b--) g = f29_add<Fs>(g_ld29<Fs>(vals, b - 1), f29_mul_c<Fs>(g, w));
  F29<Fs> excl;
  const F29<Fs> incl =
      poly_suffix_scan<Fs>(sm, f29_nr<Fs>(g), poly_tab_pow<Fs>(tab, chunk, k0), nullptr, 0, &excl);
  if (carry) {
    F29<Fs> c = excl;  // Norm, < 3p
    for (uint32_t b = hi; b > lo; b--) {
      g_st29<Fs>(carry, b - 1, c);
      c = f29_nr<Fs>(f29_add<Fs>(g_ld29<Fs>(vals, b - 1), f29_mul_c<Fs>(c, w)));
    }
  }
  return incl;
}

// grid S: carries of the tiles of set j
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_div_carry(PolyJob jb, const uint32_t* __restrict__ agg,
                                                                 uint32_t* __restrict__ carry) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t j = blockIdx.x;
  poly_block_scan<Fs>(sm, agg + (size_t)j * jb.nblk * 8, jb.nblk, jb.tab + (size_t)j * kPolyTabStride * 8,
                      kPolyTileLog, carry + (size_t)j * jb.nblk * 8);
}

// grid (nblk, S)
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_div_sweep(PolyJob jb, uint32_t* __restrict__ out,
                                                                 const uint32_t* __restrict__ lane_carry,
                                                                 const uint32_t* __restrict__ carry,
                                                                 uint32_t* __restrict__ evals) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, j = blockIdx.y;
  const size_t n = jb.n, base = (size_t)blk << kPolyTileLog;
  const uint32_t* tabj = jb.tab + (size_t)j * kPolyTabStride * 8;
  uint32_t* row = out + (size_t)j * n * 8;
  const size_t tile = (size_t)j * jb.nblk + blk;
  {
    // carry into this lane's run: in-tile part + z^(8 x lanes above) x the tile's
    const F29<Fs> kb = g_ld29<Fs>(carry, tile);
    const F29<Fs> zl = g_ld29<Fs>(tabj, kPolyTabZ8 + (kPolyThreads - 1 - tid));
    scan_st<Fs>(sm, tid,
                f29_nr<Fs>(f29_add<Fs>(g_ld29<Fs>(lane_carry, tile * kPolyThreads + tid), f29_mul_c<Fs>(kb, zl))));
  }
  __syncthreads();
  // element idx = k 256 + tid belongs to lane idx / 8 at run position tid % 8
  const F29<Fs> zd = g_ld29<Fs>(tabj, kPolyTabZj + (kPolyRun - (tid & (kPolyRun - 1))));
#pragma unroll
  for (int k = 0; k < kPolyRun; k++) {
    const uint32_t idx = k * kPolyThreads + tid;
    const size_t t = base + idx;
    if (t >= n) continue;
    const size_t slot = poly_slot(t, n);
    const F29<Fs> c = scan_ld<Fs>(sm, idx / kPolyRun);
    const F29<Fs> val = f29_canon<Fs>(f29_nr<Fs>(f29_add<Fs>(g_ld29<Fs>(row, slot), f29_mul_c<Fs>(c, zd))));
    if (t == 0) {
      g_st29<Fs>(evals, j, val);
      g_st29<Fs>(row, slot, f29_zero<Fs>());
    } else {
      g_st29<Fs>(row, slot, val);
    }
  }
}

// grid (nblk, E): part[e nblk + blk] = sum over the tile of a_t z^(t - base)
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_eval_part(const uint32_t* const* __restrict__ polys,
                                                                 const uint32_t* __restrict__ poly_index, size_t n,
                                                                 const uint32_t* __restrict__ tab,
                                                                 uint32_t* __restrict__ part) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t tid = threadIdx.x, blk = blockIdx.x, e = blockIdx.y;
  const size_t base = (size_t)blk << kPolyEvalTileLog;
  const uint32_t* p = polys[poly_index[e]];
  const uint32_t* tabe = tab + (size_t)e * kPolyTabStride * 8;
  const F29<Fs> zt = g_ld29<Fs>(tabe, 8);  // z^256
  F29<Fs> acc = f29_zero<Fs>();
#pragma unroll
  for (int k = kPolyEvalRun - 1; k >= 0; k--) {
    const size_t t = base + (size_t)k * kPolyThreads + tid;
    const F29<Fs> a = t < n ? g_ld29<Fs>(p, t) : f29_zero<Fs>();
    acc = f29_add<Fs>(a, f29_mul_c<Fs>(acc, zt));
  }
  // times z^tid = z^(8 (tid / 8)) z^(tid % 8)
  acc = f29_mul_c<Fs>(f29_mul_c<Fs>(acc, g_ld29<Fs>(tabe, kPolyTabZ8 + (tid >> 3))),
                      g_ld29<Fs>(tabe, kPolyTabZj + (tid & 7)));
  for (uint32_t s = kPolyThreads / 2; s; s >>= 1) {
    scan_st<Fs>(sm, tid, acc);
    __syncthreads();
    if (tid < s) acc = f29_nr<Fs>(f29_add<Fs>(acc, scan_ld<Fs>(sm, tid + s)));
    __syncthreads();
  }
  if (tid == 0) g_st29<Fs>(part, (size_t)e * gridDim.x + blk, f29_nr<Fs>(acc));
}

// grid E: out[e] = sum_b part[e nblk + b] z^(4096 b), canonical
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_poly_eval_comb(const uint32_t* __restrict__ part, uint32_t nblk,
                                                                 const uint32_t* __restrict__ tab,
                                                                 uint32_t* __restrict__ out) {
  __shared__ uint32_t sm[kPolyThreads * 9];
  const uint32_t e = blockIdx.x;
  const F29<Fs> r = poly_block_scan<Fs>(sm, part + (size_t)e * nblk * 8, nblk,
                                        tab + (size_t)e * kPolyTabStride * 8, kPolyEvalTileLog, nullptr);
  if (threadIdx.x == 0) g_st29<Fs>(out, e, f29_canon<Fs>(r));
}

}  // namespace pm

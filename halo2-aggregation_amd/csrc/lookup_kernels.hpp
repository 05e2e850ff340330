// lookup_kernels.hpp -- the lookup argument's permuted columns:
// halo2 plonk/lookup/prover.rs::compress_expressions and
// permute_expression_pair [3P], the step of create_proof between the advice
// commit and the lookup grand product (pm_grand_product_device reads A' and S').
//
// Unlike every other kernel of the library this is no field arithmetic: a
// comparison sort of 256-bit keys, a merge-join and a scatter.  The order is
// halo2's Ord on field elements, the numeric order of the canonical value, so a
// key is the canonical integer (8 words, little endian), made from the caller's
// Montgomery words with one product on load (x 2^256 times 2^5, times 2^-261)
// and turned back with one product on store (x times 2^517, times 2^-261).
// Keys carry no payload and equal keys are indistinguishable: stability does
// not matter, and S'[i] = A'[i] is bit-identical because both stores start from
// the same key.
//
// Launches, each on the context stream (no block ever waits on another), with
// the pair / column in grid.y:
//   k_lk_tile_sort  grid (tiles, 2 P): 2^11 keys per block, converted on load,
//     padded with the all-ones key (above every canonical value), bitonic
//     network in LDS (8 word planes, one compare-exchange per lane and step),
//     canonical keys to the scratch column.
//   k_lk_merge      grid (tiles, 2 P), once per doubling of the run length:
//     a block owns 2^11 consecutive outputs of one pair of runs, finds its two
//     merge-path split points by binary search in global memory, loads the two
//     input pieces (2^11 keys together) into LDS, ranks every key in the other
//     piece by binary search in LDS (ties: the first run first), permutes in
//     LDS and stores coalesced.  Cost is independent of the key distribution.
//   k_lk_flags      grid (blocks of 1024 rows, P), on sorted A' and sorted T:
//     "not first" flags of A'; every first row searches T (a miss is the
//     circuit's failure: atomicMin of the row); every first occurrence of T
//     searches A' (a hit uses that instance up), every other row of T is a
//     leftover.  Per block the two counts.
//   k_lk_carry      one block per count row: exclusive prefix over the blocks
//     and the total.
//   k_lk_rows       A'[i] and, at first rows, S'[i] stored (Montgomery); the
//     repeated row of rank q recorded.
//   k_lk_scatter    leftover of rank k stored to the repeated row of rank
//     R - 1 - k (halo2 pops the repeated rows from the back).
//   k_lk_compress   one lane per row: Horner over the m columns.
//
// Arithmetic of the compression: columns and the accumulator keep the caller's
// R = 2^256 meaning ("data" form, unpacked); theta is converted to the native
// R = 2^261 form once per lane, so f29_mul_c(acc, theta) is the data form
// again.  An input is Norm, < 2^256 (< 5.4p); the lazy sum input + product is
// < 7.4p and is normalised and reduced (f29_nr: < 16p -> Norm, < 3p) before it
// enters the next product: the operand shapes of gp_kernels.hpp.
#pragma once
#include "msm_kernels.hpp"
#include "poly_kernels.hpp"

namespace pm {

constexpr int kLkTileLog = 11;
constexpr uint32_t kLkTile = 1u << kLkTileLog;  // keys per sorted tile = outputs per merge block
constexpr int kLkThreads = 1024;
constexpr size_t kLkLds = (size_t)kLkTile * 32;  // 64 KiB: two blocks per CU
constexpr uint32_t kLkNoRow = 0xFFFFFFFFu;       // no failing row
static_assert(kLkTile == PM_LOOKUP_TILE && kLkTile == PM_LOOKUP_MERGE, "the header states the kernels' geometry");
static_assert(kLkTile == 2 * kLkThreads, "one compare-exchange per lane and step; two keys per lane elsewhere");

// 2^517 mod r: canonical integer -> R = 2^256 Montgomery in one f29_mul_c
template <class P>
struct LkConsts;
template <>
struct LkConsts<VestaFp> {
  static constexpr uint32_t R517[9] = {0x000001dcu, 0x0d9b9ae0u, 0x1c0e4258u, 0x1c0781f9u, 0x0b20c6e4u,
                                       0x11004ccfu, 0x14bfd711u, 0x1df33f6au, 0x002da835u};
};
template <>
struct LkConsts<PallasFp> {
  static constexpr uint32_t R517[9] = {0x000001dcu, 0x13469560u, 0x020e20cau, 0x0ea78279u, 0x1a31a714u,
                                       0x19bc3c95u, 0x0a3bcbd4u, 0x1dee72dcu, 0x002da835u};
};
template <>
struct LkConsts<Bn254Fr> {
  static constexpr uint32_t R517[9] = {0x142db4dfu, 0x19d6990eu, 0x1472f48cu, 0x06dbe7e3u, 0x0b84d579u,
                                       0x10f9faf7u, 0x121f4380u, 0x17a112deu, 0x001275c7u};
};

struct LkJob {
  const uint32_t* const* in;  // device array of 2 P pointers: a_0, s_0, a_1, s_1, ...
  uint32_t* const* out;       // likewise: out_a_0, out_s_0, ...
  uint32_t* rowof;            // P x usable: the repeated row of rank q
  uint8_t* left;              // P x usable: leftover flags of sorted T
  uint32_t* cnt;              // 2 P rows of nblk: per-block counts (not first | leftover), then their prefixes
  uint32_t* tot;              // 2 P: the totals
  uint32_t* fail;             // P: the smallest first row of A' whose value T lacks
  uint32_t usable;
  uint32_t nblk;              // pairing blocks per pair: ceil(usable / 1024)
};

// ------------------------------------------------------------------ keys
__device__ __forceinline__ void lk_ld(const uint32_t* __restrict__ g, size_t i, uint32_t k[8]) {
  const uint4* q = reinterpret_cast<const uint4*>(g + 8ull * i);
  const uint4 a = q[0], b = q[1];
  k[0] = a.x, k[1] = a.y, k[2] = a.z, k[3] = a.w;
  k[4] = b.x, k[5] = b.y, k[6] = b.z, k[7] = b.w;
}
__device__ __forceinline__ void lk_st(uint32_t* g, size_t i, const uint32_t k[8]) {
  uint4* q = reinterpret_cast<uint4*>(g + 8ull * i);
  q[0] = make_uint4(k[0], k[1], k[2], k[3]);
  q[1] = make_uint4(k[4], k[5], k[6], k[7]);
}
// LDS image: 8 word planes of kLkTile words (a wave reads consecutive words of one plane)
__device__ __forceinline__ void lk_sld(const uint32_t* sm, uint32_t i, uint32_t k[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) k[w] = sm[w * kLkTile + i];
}
__device__ __forceinline__ void lk_sst(uint32_t* sm, uint32_t i, const uint32_t k[8]) {
#pragma unroll
  for (int w = 0; w < 8; w++) sm[w * kLkTile + i] = k[w];
}
// a < b as 256-bit integers (the top word decides last)
__device__ __forceinline__ bool lk_lt(const uint32_t a[8], const uint32_t b[8]) {
  bool lt = false;
#pragma unroll
  for (int w = 0; w < 8; w++) lt = a[w] < b[w] || (a[w] == b[w] && lt);
  return lt;
}
__device__ __forceinline__ bool lk_eq(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d |= a[w] ^ b[w];
  return d == 0;
}
// Montgomery words of the caller's column -> canonical key
template <class Fs>
__device__ __forceinline__ void lk_key_from_col(const uint32_t* __restrict__ col, size_t i, uint32_t k[8]) {
  F29<Fs> c = f29_zero<Fs>();
  c.l[0] = 32u;  // (x 2^256) 2^5 2^-261 = x
  f29_pack<Fs>(f29_canon<Fs>(f29_mul_c<Fs>(g_ld29<Fs>(col, i), c)), k);
}
// canonical key -> Montgomery, canonical (Norm, < p)
template <class Fs>
__device__ __forceinline__ F29<Fs> lk_key_mont(const uint32_t k[8]) {
  return f29_canon<Fs>(f29_mul_c<Fs>(f29_unpack<Fs>(k), f29_const<Fs>(LkConsts<Fs>::R517)));
}
// the first index in [0, cnt) of the sorted global column whose key is not below `key`
__device__ __forceinline__ uint32_t lk_lower_bound(const uint32_t* __restrict__ col, uint32_t cnt,
                                                   const uint32_t key[8]) {
  uint32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    uint32_t v[8];
    lk_ld(col, mid, v);
    if (lk_lt(v, key))
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------ sort
// grid (ceil(usable / 2^11), 2 P), kLkLds bytes of LDS.  keys: 2 P columns of
// `usable` canonical keys; tile t of column c holds its keys sorted.
template <class Fs>
__global__ void __launch_bounds__(kLkThreads) k_lk_tile_sort(LkJob jb, uint32_t* __restrict__ keys) {
  extern __shared__ uint32_t sm[];
  const uint32_t tid = threadIdx.x, c = blockIdx.y, u = jb.usable;
  const size_t base = (size_t)blockIdx.x << kLkTileLog;
  if (blockIdx.x == 0 && tid == 0 && !(c & 1u)) jb.fail[c >> 1] = kLkNoRow;
  const uint32_t* col = jb.in[c];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t e = tid + h * kLkThreads;
    uint32_t k[8];
#pragma unroll
    for (int w = 0; w < 8; w++) k[w] = 0xFFFFFFFFu;
    if (base + e < u) lk_key_from_col<Fs>(col, base + e, k);
    lk_sst(sm, e, k);
  }
  __syncthreads();
  for (uint32_t k = 2; k <= kLkTile; k <<= 1) {
    for (uint32_t j = k >> 1; j; j >>= 1) {
      const uint32_t i = ((tid & ~(j - 1u)) << 1) | (tid & (j - 1u)), l = i | j;
      uint32_t a[8], b[8];
      lk_sld(sm, i, a);
      lk_sld(sm, l, b);
      const bool up = !(i & k);  // k == kLkTile: every pair ascending
      if (up ? lk_lt(b, a) : lk_lt(a, b)) {
        lk_sst(sm, i, b);
        lk_sst(sm, l, a);
      }
      __syncthreads();
    }
  }
  uint32_t* dst = keys + (size_t)c * u * 8;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t e = tid + h * kLkThreads;
    if (base + e < u) {  // the padding sorted behind the tile's keys
      uint32_t k[8];
      lk_sld(sm, e, k);
      lk_st(dst, base + e, k);
    }
  }
}

// grid (ceil(usable / 2^11), 2 P), kLkLds bytes of LDS.  src holds sorted runs
// of 2^runlog keys (the last one shorter); dst receives runs of twice that.
static __global__ void __launch_bounds__(kLkThreads) k_lk_merge(const uint32_t* __restrict__ src,
                                                               uint32_t* __restrict__ dst, uint32_t u,
                                                               uint32_t runlog) {
  extern __shared__ uint32_t sm[];
  __shared__ uint32_t split[2];
  const uint32_t tid = threadIdx.x;
  const uint32_t* s = src + (size_t)blockIdx.y * u * 8;
  uint32_t* d = dst + (size_t)blockIdx.y * u * 8;
  const uint32_t run = 1u << runlog;
  const uint32_t o0 = blockIdx.x << kLkTileLog;        // this block's first output
  const uint32_t a0 = o0 & ~(2u * run - 1u);           // the pair of runs it lies in
  const uint32_t len_a = min(run, u - a0), b0 = a0 + len_a, len_b = min(run, u - b0);
  const uint32_t d0 = o0 - a0, d1 = min(d0 + kLkTile, len_a + len_b);
  if (tid < 2) {
    // merge path: how many of the first dg outputs come from run A (ties: A first)
    const uint32_t dg = tid ? d1 : d0;
    uint32_t lo = dg > len_b ? dg - len_b : 0u, hi = min(dg, len_a);
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      uint32_t ka[8], kb[8];
      lk_ld(s, (size_t)a0 + mid, ka);
      lk_ld(s, (size_t)b0 + (dg - mid - 1u), kb);
      if (!lk_lt(kb, ka))  // A[mid] <= B[dg - mid - 1]: A[mid] is among the first dg
        lo = mid + 1;
      else
        hi = mid;
    }
    split[tid] = lo;
  }
  __syncthreads();
  const uint32_t i0 = split[0], j0 = d0 - i0, na = split[1] - i0, nb = (d1 - d0) - na;
  uint32_t key[2][8], pos[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t e = tid + h * kLkThreads;
    if (e < na + nb) {
      lk_ld(s, e < na ? (size_t)a0 + i0 + e : (size_t)b0 + j0 + (e - na), key[h]);
      lk_sst(sm, e, key[h]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t e = tid + h * kLkThreads;
    pos[h] = 0;
    if (e < na) {  // keys of B's piece below this one
      uint32_t lo = 0, hi = nb;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t v[8];
        lk_sld(sm, na + mid, v);
        if (lk_lt(v, key[h]))
          lo = mid + 1;
        else
          hi = mid;
      }
      pos[h] = e + lo;
    } else if (e < na + nb) {  // keys of A's piece not above this one
      uint32_t lo = 0, hi = na;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t v[8];
        lk_sld(sm, mid, v);
        if (!lk_lt(key[h], v))
          lo = mid + 1;
        else
          hi = mid;
      }
      pos[h] = (e - na) + lo;
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; h++)
    if (tid + h * kLkThreads < na + nb) lk_sst(sm, pos[h], key[h]);
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t e = tid + h * kLkThreads;
    if (e < na + nb) {
      uint32_t k[8];
      lk_sld(sm, e, k);
      lk_st(d, (size_t)o0 + e, k);
    }
  }
}

// ------------------------------------------------------------------ pairing
// block sum of a 0 / 1 flag into *slot (LDS, zeroed before)
__device__ __forceinline__ void lk_count(uint32_t* slot, bool flag) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63u) == 0 && m) atomicAdd(slot, (uint32_t)__popcll(m));
}

// grid (nblk, P).  keys: the sorted columns (A' of pair p at column 2 p, T at 2 p + 1)
static __global__ void __launch_bounds__(kLkThreads) k_lk_flags(LkJob jb, const uint32_t* __restrict__ keys) {
  __shared__ uint32_t cnts[2];
  const uint32_t tid = threadIdx.x, p = blockIdx.y, u = jb.usable;
  const uint32_t i = blockIdx.x * kLkThreads + tid;
  const uint32_t* a = keys + (size_t)(2 * p) * u * 8;
  const uint32_t* t = a + (size_t)u * 8;
  if (tid < 2) cnts[tid] = 0;
  __syncthreads();
  bool nf = false, lf = false;
  if (i < u) {
    uint32_t ka[8], kt[8], v[8];
    lk_ld(a, i, ka);
    lk_ld(t, i, kt);
    if (i) {
      lk_ld(a, i - 1, v);
      nf = lk_eq(v, ka);
    }
    if (!nf) {
      const uint32_t pos = lk_lower_bound(t, u, ka);
      bool hit = false;
      if (pos < u) {
        lk_ld(t, pos, v);
        hit = lk_eq(v, ka);
      }
      if (!hit) atomicMin(jb.fail + p, i);
    }
    bool ft = true;
    if (i) {
      lk_ld(t, i - 1, v);
      ft = !lk_eq(v, kt);
    }
    lf = true;
    if (ft) {
      const uint32_t pos = lk_lower_bound(a, u, kt);
      if (pos < u) {
        lk_ld(a, pos, v);
        lf = !lk_eq(v, kt);
      }
    }
    jb.left[(size_t)p * u + i] = lf ? 1 : 0;
  }
  lk_count(cnts, nf);
  lk_count(cnts + 1, lf);
  __syncthreads();
  if (tid < 2) jb.cnt[(size_t)(2 * p + tid) * jb.nblk + blockIdx.x] = cnts[tid];
}

// grid 2 P: row r of cnt -> exclusive prefixes in place, tot[r] the sum
static __global__ void __launch_bounds__(kScanThreads) k_lk_carry(LkJob jb) {
  __shared__ uint32_t lds[kScanThreads / 64 + 1];
  const uint32_t tid = threadIdx.x, count = jb.nblk;
  uint32_t* v = jb.cnt + (size_t)blockIdx.x * count;
  const uint32_t chunk = (count + kScanThreads - 1) / kScanThreads;
  const uint32_t lo = min(count, tid * chunk), hi = min(count, lo + chunk);
  uint32_t s = 0, total;
  for (uint32_t b = lo; b < hi; b++) s += v[b];
  uint32_t ex = block_excl_scan(s, lds, total);
  for (uint32_t b = lo; b < hi; b++) {
    const uint32_t x = v[b];
    v[b] = ex;
    ex += x;
  }
  if (tid == 0) jb.tot[blockIdx.x] = total;
}

// grid (nblk, P)
template <class Fs>
__global__ void __launch_bounds__(kLkThreads) k_lk_rows(LkJob jb, const uint32_t* __restrict__ keys) {
  __shared__ uint32_t lds[kLkThreads / 64 + 1];
  const uint32_t p = blockIdx.y, u = jb.usable;
  const uint32_t i = blockIdx.x * kLkThreads + threadIdx.x;
  const uint32_t* a = keys + (size_t)(2 * p) * u * 8;
  uint32_t ka[8];
  bool nf = false;
  if (i < u) {
    lk_ld(a, i, ka);
    if (i) {
      uint32_t v[8];
      lk_ld(a, i - 1, v);
      nf = lk_eq(v, ka);
    }
  }
  uint32_t total;
  const uint32_t q = jb.cnt[(size_t)(2 * p) * jb.nblk + blockIdx.x] + block_excl_scan(nf ? 1u : 0u, lds, total);
  if (i < u) {
    const F29<Fs> m = lk_key_mont<Fs>(ka);
    g_st29<Fs>(jb.out[2 * p], i, m);
    if (nf)
      jb.rowof[(size_t)p * u + q] = i;
    else
      g_st29<Fs>(jb.out[2 * p + 1], i, m);
  }
}

// grid (nblk, P)
template <class Fs>
__global__ void __launch_bounds__(kLkThreads) k_lk_scatter(LkJob jb, const uint32_t* __restrict__ keys) {
  __shared__ uint32_t lds[kLkThreads / 64 + 1];
  const uint32_t p = blockIdx.y, u = jb.usable;
  const uint32_t i = blockIdx.x * kLkThreads + threadIdx.x;
  const uint32_t* t = keys + (size_t)(2 * p + 1) * u * 8;
  const bool lf = i < u && jb.left[(size_t)p * u + i];
  uint32_t total;
  const uint32_t e = jb.cnt[(size_t)(2 * p + 1) * jb.nblk + blockIdx.x] + block_excl_scan(lf ? 1u : 0u, lds, total);
  const uint32_t R = jb.tot[2 * p];  // repeated rows; a failed pair has more leftovers than that
  if (lf && e < R) {
    uint32_t kt[8];
    lk_ld(t, i, kt);
    g_st29<Fs>(jb.out[2 * p + 1], jb.rowof[(size_t)p * u + (R - 1u - e)], lk_key_mont<Fs>(kt));
  }
}

// ------------------------------------------------------------------ compress
// cols: device array of m pointers; theta: 8 words (R = 2^256), read when m > 1
template <class Fs>
__global__ void __launch_bounds__(kPolyThreads) k_lk_compress(const uint32_t* const* __restrict__ cols, uint32_t m,
                                                              size_t n, const uint32_t* __restrict__ theta,
                                                              uint32_t* out) {
  const size_t i = (size_t)blockIdx.x * kPolyThreads + threadIdx.x;
  if (i >= n) return;
  if (m == 1) {
    uint32_t k[8];
    lk_ld(cols[0], i, k);
    lk_st(out, i, k);
    return;
  }
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = theta[k];
  const F29<Fs> th = f29_from_r256<Fs>(w);
  F29<Fs> acc = g_ld29<Fs>(cols[0], i);
  for (uint32_t k = 1; k < m; k++) acc = f29_nr<Fs>(f29_add<Fs>(g_ld29<Fs>(cols[k], i), f29_mul_c<Fs>(acc, th)));
  g_st29<Fs>(out, i, f29_canon<Fs>(acc));
}

}  // namespace pm

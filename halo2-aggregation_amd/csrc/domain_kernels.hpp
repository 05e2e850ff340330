// domain_kernels.hpp -- the extended-domain conversions of halo2's
// EvaluationDomain [3P domain.rs]: coeff_to_extended, extended_to_coeff,
// divide_by_vanishing_poly, and the NTT over a batch of columns
// (pm_domain_*, pm_fft_batch_device).
//
// The transforms are the passes of ntt_kernels.hpp (ntt_load_first, lds_ntt4,
// ntt_rounds_store) with a column dimension (blockIdx.y over a device table of
// column pointers, the twiddle segments shared) and the conversions' extra
// factors folded into the first pass's loader and the last pass's epilogue,
// so none of them costs a pass over HBM:
//   * coset load (coeff_to_extended): input idx >= n is a zero that is never
//     read; idx < n is a[idx] zeta^(idx mod 3), no product for idx mod 3 = 0;
//   * vanishing load (extended_to_coeff with PM_EXT_DIVIDE_VANISHING): the
//     input times t[idx mod 2^e];
//   * coset store (extended_to_coeff): output j times N^-1 zeta^-(j mod 3),
//     one of three precomputed scales fetched at the store (not kept live
//     across the rounds: the trap recorded at ntt_rounds_store), and no store
//     for j >= keep.
// The tables (pm_domain, domain_engine.hpp) are R = 2^261 canonical packed,
// like the twiddles: a product with one keeps the data's R = 2^256 meaning.
// Bounds: a loader's product is Norm, < 2p, inside the < 3p that
// ntt_load_first takes; the coset store multiplies a Norm < 3p round output
// like k_ntt_rows' scale does.
#pragma once
#include "ntt_kernels.hpp"

namespace pm {

enum : int { kDomPlain = 0, kDomCoset = 1, kDomVanish = 2 };

// column blockIdx.y of a launch: its entry of a device pointer table, or
// (tab == nullptr) row blockIdx.y of a scratch buffer of `stride` words per row
__device__ __forceinline__ uint32_t* dom_col(uint32_t* const* tab, uint32_t* base, size_t stride) {
  return tab ? tab[blockIdx.y] : base + (size_t)blockIdx.y * stride;
}

// ntt_load_first (c fastest) for a sub-transform whose inputs i >= nz are
// zeros (the zero padding of coeff_to_extended).  When every partner of the
// first unit is such a zero (nz <= L/2 for the radix-2 stage 0, nz <= L/4 for
// the radix-4 unit) all its outputs equal its first input x0: u + 0, u - 0,
// and y2 = y3 = z3 = 0.  x0 is Norm, < 2p (canonical, or a product), inside
// the < 3p the stored outputs keep.  Otherwise the general loader runs.
template <class Fs, class Src>
__device__ __forceinline__ int dom_load_first_padded(uint32_t* sm, int logL, int logC, const uint32_t* __restrict__ tw,
                                                     uint32_t nz, Src src) {
  const int f = (logL & 1) ? 1 : 2;  // stages of the first unit
  if (logL == 0 || nz > (1u << (logL - f))) return ntt_load_first<Fs>(sm, logL, logC, 1, tw, false, src);
  const uint32_t plane = 1u << (logL + logC), C = 1u << logC;
  for (uint32_t b = threadIdx.x; b < (plane >> f); b += blockDim.x) {
    const uint32_t i = b >> logC, c = b & (C - 1);
    const uint32_t pos = ntt_brev(i, logL);  // i < L / 2^f: the unit's first position
    const F29<Fs> x0 = src(i, c);
    for (uint32_t q = 0; q < (1u << f); q++) lds_st<Fs>(sm, plane, ((pos + q) << logC) | c, x0);
  }
  return f;
}

// pass A of k_ntt_cols per column.  Mode kDomCoset: dtab = zeta^0..2, lim = n
// (inputs at idx >= lim are zeros); kDomVanish: dtab = t, lim = 2^e - 1.
template <class Fs, int Mode>
__global__ void __launch_bounds__(kNttMaxThreads) k_dom_cols(uint32_t* const* in_tab, uint32_t* in_base,  // may alias out
                                                          uint32_t* const* out_tab, uint32_t* out_base, size_t stride,
                                                          int logn, int log1, int logC,
                                                          const uint32_t* __restrict__ tw,
                                                          const uint32_t* __restrict__ lo,
                                                          const uint32_t* __restrict__ hi, int s, uint32_t last,
                                                          const uint32_t* __restrict__ dtab, uint32_t lim) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  const uint32_t* in = dom_col(in_tab, in_base, stride);
  uint32_t* out = dom_col(out_tab, out_base, stride);
  const int log2 = logn - log1;
  const uint32_t n2 = 1u << log2;
  const uint32_t col0 = ntt_block(n2 >> logC) << logC;
  const auto src = [&](uint32_t i1, uint32_t c) {
    const uint32_t idx = i1 * n2 + col0 + c;  // < 2^logn <= 2^28
    if constexpr (Mode == kDomCoset) {
      if (idx >= lim) return f29_zero<Fs>();
      F29<Fs> v = g_ld29<Fs>(in, idx);
      const uint32_t m = idx % 3u;
      if (m) v = f29_mul_c<Fs>(v, g_ld29<Fs>(dtab, m));
      return v;
    } else if constexpr (Mode == kDomVanish) {
      return f29_mul_c<Fs>(g_ld29<Fs>(in, idx), g_ld29<Fs>(dtab, idx & lim));
    } else {
      return g_ld29<Fs>(in, idx);
    }
  };
  int t0;
  if constexpr (Mode == kDomCoset) {
    // whole rows of the n1 x n2 matrix are padding when n2 divides n: inputs i1 >= n / n2
    t0 = dom_load_first_padded<Fs>(sm, log1, logC, tw, (lim & (n2 - 1)) ? (1u << log1) : lim >> log2, src);
  } else {
    t0 = ntt_load_first<Fs>(sm, log1, logC, 1, tw, false, src);
  }
  __syncthreads();
  ntt_rounds_store<Fs>(sm, log1, logC, 1, tw, t0, [&] {
    return [&](uint32_t k1, uint32_t c, F29<Fs> v) {
      const uint32_t i2 = col0 + c;
      if (log2 > 0 && i2 && k1) v = f29_mul_c<Fs>(v, tw_two<Fs>(lo, hi, i2 * k1, s));  // i2 k1 < n
      if (last) v = f29_canon<Fs>(v);
      g_st29<Fs>(out, (size_t)k1 * n2 + i2, v);
    };
  });
}

// the middle pass of k_ntt_mid per column (scratch to scratch)
template <class Fs>
__global__ void __launch_bounds__(kNttMaxThreads) k_dom_mid(const uint32_t* __restrict__ in_base,
                                                         uint32_t* __restrict__ out_base, size_t stride, int logn,
                                                         int log1, int loga, int logC,
                                                         const uint32_t* __restrict__ tw,
                                                         const uint32_t* __restrict__ lo,
                                                         const uint32_t* __restrict__ hi, int s) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  const uint32_t* in = in_base + (size_t)blockIdx.y * stride;
  uint32_t* out = out_base + (size_t)blockIdx.y * stride;
  const int logb = logn - log1 - loga;
  const uint32_t n1 = 1u << log1, nb = 1u << logb;
  const uint32_t groups = nb >> logC;
  const uint32_t blk = ntt_block(n1 * groups);
  const uint32_t k1 = blk / groups, col0 = (blk - k1 * groups) << logC;
  const uint32_t* row = in + 8ull * ((size_t)k1 << (loga + logb));
  const int t0 = ntt_load_first<Fs>(sm, loga, logC, 1, tw, false, [&](uint32_t ia, uint32_t c) {
    return g_ld29<Fs>(row, (size_t)ia * nb + col0 + c);
  });
  __syncthreads();
  ntt_rounds_store<Fs>(sm, loga, logC, 1, tw, t0, [&] {
    return [&](uint32_t ka, uint32_t c, F29<Fs> v) {
      const uint32_t ib = col0 + c;
      if (ib && ka) v = f29_mul_c<Fs>(v, tw_two<Fs>(lo, hi, n1 * ib * ka, s));  // n1 ib ka < n
      g_st29<Fs>(out, ((size_t)ka * n1 + k1) * nb + ib, v);
    };
  });
}

// pass B of k_ntt_rows per column.  Mode kDomPlain: the optional scale of
// pm_fft; kDomCoset: dtab = the three scales N^-1 zeta^-j, outputs j < keep only.
template <class Fs, int Mode>
__global__ void __launch_bounds__(kNttMaxThreads) k_dom_rows(uint32_t* const* in_tab, uint32_t* in_base,  // may alias out (log2 = 0)
                                                          uint32_t* const* out_tab, uint32_t* out_base, size_t stride,
                                                          int logn, int log2, int logR,
                                                          const uint32_t* __restrict__ tw, FeArg scale,
                                                          uint32_t use_scale, const uint32_t* __restrict__ dtab,
                                                          uint32_t keep) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sm[];
  const uint32_t* in = dom_col(in_tab, in_base, stride);
  uint32_t* out = dom_col(out_tab, out_base, stride);
  const int log1 = logn - log2;
  const uint32_t n1 = 1u << log1, L = 1u << log2;
  const uint32_t row0 = ntt_block(n1 >> logR) << logR;
  const int t0 = ntt_load_first<Fs>(sm, log2, logR, 1, tw, true, [&](uint32_t i2, uint32_t r) {
    return g_ld29<Fs>(in, (size_t)(row0 + r) * L + i2);
  });
  __syncthreads();
  if constexpr (Mode == kDomCoset) {
    ntt_rounds_store<Fs>(sm, log2, logR, 1, tw, t0, [&] {
      return [&](uint32_t k2, uint32_t r, F29<Fs> v) {
        const uint32_t j = row0 + r + n1 * k2;  // < 2^logn
        if (j >= keep) return;
        v = f29_mul_c<Fs>(v, g_ld29<Fs>(dtab, j % 3u));
        g_st29<Fs>(out, j, f29_canon<Fs>(v));
      };
    });
  } else {
    ntt_rounds_store<Fs>(sm, log2, logR, 1, tw, t0, [&] {
      const F29<Fs> sc = use_scale ? f29_from_r256<Fs>(scale.l) : f29_zero<Fs>();  // Norm, < 2p
      return [&, sc](uint32_t k2, uint32_t r, F29<Fs> v) {
        if (use_scale) v = f29_mul_c<Fs>(v, sc);
        g_st29<Fs>(out, (size_t)(row0 + r) + (size_t)n1 * k2, f29_canon<Fs>(v));
      };
    });
  }
}

// divide_by_vanishing_poly: h[j] <- h[j] t[j mod 2^e], canonical in and out.
// A thread's elements are gridDim.x * blockDim.x apart, a multiple of 256 >=
// 2^e, so it holds its one table entry in registers.
constexpr unsigned kDomDivThreads = 256;
template <class Fs>
__global__ void __launch_bounds__(kDomDivThreads) k_dom_divide(uint32_t* const* tab, uint32_t n,
                                                               const uint32_t* __restrict__ t, uint32_t mask) {
  uint32_t* h = tab[blockIdx.y];
  const uint32_t i0 = blockIdx.x * kDomDivThreads + threadIdx.x, step = gridDim.x * kDomDivThreads;
  if (i0 >= n) return;
  const F29<Fs> ti = g_ld29<Fs>(t, i0 & mask);
  for (uint32_t i = i0; i < n; i += step) g_st29<Fs>(h, i, f29_canon<Fs>(f29_mul_c<Fs>(g_ld29<Fs>(h, i), ti)));
}

}  // namespace pm

// ecfft_kernels.hpp -- best_fft over curve points (pm_fft_points*).
//
//   out[k] = [scale] sum_j [omega^{jk}] in[j],   n = 2^log_n points, in place
//
// Decimation in time after a bit reversal, as halo2's best_fft: stage s
// (1 .. log_n) runs n/2 butterflies  t = [w] b, a' = a + t, b' = a - t  over
// pairs 2^(s-1) apart, w = omega^(j n / 2^s).  The group is exact, so the
// order of the operations is free; the result is the same affine point.
//
//   k_ecfft_twiddles  omega^j, j < n/2, stored as the multiplication consumes
//                     it: the signed 3-bit codes of the rounded GLV halves
//                     (w3_codes, accum_kernels.hpp), 48 B per twiddle, the
//                     halves' signs in bit 31 of each half's last word.  No
//                     stage splits a scalar again.
//   k_ecfft_bitrev    the reversal: lane i swaps slots i and rev(i), i < rev(i)
//   k_ecfft_first     stage 1 (w = 1): a + b, a - b, no multiplication
//   k_ecfft_stage     stages 2 .. log_n: a lane per butterfly, in place on its
//                     own two slots (no block waits on another); the one-term
//                     windowed GLV multiplication of k_acc_termmul (129
//                     doublings, 86 mixed additions, the [1..4]P table in LDS)
//                     with the codes read instead of derived
//   k_ecfft_scale     [scale] P per point (glv_mul_w3 itself)
//
// Between stages the points stay in the caller's form, affine R = 2^256 at
// 64 B each: the next stage's table takes an affine point (mixed additions),
// a + t and a - t are mixed additions onto t, and the two outputs share one
// inversion (Montgomery's trick), about 1 % of the lane's multiplication.
// So every stage starts and ends on valid boundary data, and a transform of
// one point or two needs no conversion pass at all.
#pragma once
#include "accum_kernels.hpp"

namespace pm {

constexpr uint32_t kEcfftTwWords = 12;  // per twiddle: c1[6] | c2[6]

// [k]P from k's codes (w3_codes<Cv, false>; s1, s2: 8 when the half is
// negated): glv_mul_w3's loop.
template <class Cv>
__device__ __forceinline__ Xyzz29<typename Cv::Base> ecfft_mul_codes(const uint32_t c1[6], const uint32_t c2[6],
                                                                    uint32_t s1, uint32_t s2,
                                                                    const Aff<typename Cv::Base>& P,
                                                                    uint32_t (*tab)[256]) {
  using F = typename Cv::Base;
  constexpr int kWin = 43;
  w3_table<Cv>(P, tab, 0);
  const uint32_t ln = threadIdx.x;
  const F29<F> beta = f29_const<F>(Glv<Cv>::BETA29);
  Xyzz29<F> acc = xyzz29_inf<F>();
  bool acc_inf = true;
  for (int i = kWin - 1; i >= 0; i--) {
    acc = xyzz29_dbl<F>(xyzz29_dbl<F>(xyzz29_dbl<F>(acc)));
    uint32_t w1 = 0, w2 = 0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      w1 = j == (i >> 3) ? c1[j] : w1;
      w2 = j == (i >> 3) ? c2[j] : w2;
    }
    const uint32_t sh = 4u * (uint32_t)(i & 7);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const uint32_t e = ((half ? w2 : w1) >> sh) & 15u, m = e & 7u;
      if (m == 0) continue;
      F29<F> qx, qy;
      const uint32_t r0 = 18u * (m - 1u);
#pragma unroll
      for (int t = 0; t < 9; t++) {
        qx.l[t] = tab[r0 + t][ln];
        qy.l[t] = tab[r0 + 9 + t][ln];
      }
      if (half) qx = f29_canon<F>(f29_mul_c<F>(beta, qx));
      if (((e ^ (half ? s2 : s1)) & 8u) != 0u) qy = f29_canon<F>(f29_neg_canon<F>(qy));
      acc = xyzz29_madd<F>(acc, qx, qy, acc_inf);
    }
  }
  return acc;
}

template <class Cv>
__global__ void __launch_bounds__(256) k_ecfft_twiddles(FeArg omega, uint32_t half_n, uint4* __restrict__ tw) {
  using Fs = typename Cv::Scalar;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= half_n) return;
  Fe<Fs> r = fe_one<Fs>(), b = fe_of<Fs>(omega);
  for (uint32_t e = j; e; e >>= 1) {
    if (e & 1) r = fe_mul<Fs>(r, b);
    b = fe_sqr<Fs>(b);
  }
  uint32_t c1[6] = {0, 0, 0, 0, 0, 0}, c2[6] = {0, 0, 0, 0, 0, 0}, s1, s2;
  w3_codes<Cv, false>(fe_from_mont<Fs>(r), c1, c2, s1, s2);
  c1[5] |= s1 << 28;  // 43 codes fill bits 0..11 of word 5
  c2[5] |= s2 << 28;
  uint4* o = tw + 3ull * j;
  o[0] = make_uint4(c1[0], c1[1], c1[2], c1[3]);
  o[1] = make_uint4(c1[4], c1[5], c2[0], c2[1]);
  o[2] = make_uint4(c2[2], c2[3], c2[4], c2[5]);
}

template <class Cv>  // (a template for its linkage only: one copy per curve unit)
__global__ void __launch_bounds__(256) k_ecfft_bitrev(uint4* __restrict__ pts, uint32_t logn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << logn)) return;
  const uint32_t r = __brev(i) >> (32 - logn);  // logn >= 1
  if (i >= r) return;
  uint4* a = pts + 4ull * i;
  uint4* b = pts + 4ull * r;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint4 u = a[k], v = b[k];
    a[k] = v;
    b[k] = u;
  }
}

template <class F>
__device__ __forceinline__ void ecfft_store_aff(uint32_t* dst, const F29<F>& x, const F29<F>& y) {
  Fe<F> wx, wy;
  f29_to_r256<F>(x, wx.l);
  f29_to_r256<F>(y, wy.l);
  uint4* q = reinterpret_cast<uint4*>(dst);
  store_fe4<F>(q, wx);
  store_fe4<F>(q + 2, wy);
}
template <class F>
__device__ __forceinline__ void ecfft_store_inf(uint32_t* dst) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  const uint4 z = make_uint4(0, 0, 0, 0);
  q[0] = z, q[1] = z, q[2] = z, q[3] = z;
}

// The butterfly's two outputs from t: A = a + t at pa, and -(t - a) = a - t at
// pb, as canonical affine points with one shared inversion.  a: the affine
// input (R = 2^261 canonical), a_inf / t_inf: a / t is the identity.  Complete:
// a = t doubles, a = -t gives the identity (xyzz29_madd's branches).
template <class F>
__device__ __forceinline__ void ecfft_butterfly_out(uint32_t* pa, uint32_t* pb, const Xyzz29<F>& t, bool t_inf,
                                                    const F29<F>& ax, const F29<F>& ay, bool a_inf) {
  const F29<F> one = f29_const<F>(F29Consts<F>::ONE);
  Xyzz29<F> A = t, D = t;
  bool A_inf = t_inf, D_inf = t_inf;
  if (!a_inf) {
    A = xyzz29_madd<F>(t, ax, ay, A_inf);
    D = xyzz29_madd<F>(t, ax, f29_canon<F>(f29_neg_canon<F>(ay)), D_inf);
  }
  const F29<F> dA = A_inf ? one : f29_mul_c<F>(A.ZZ, A.ZZZ), dD = D_inf ? one : f29_mul_c<F>(D.ZZ, D.ZZZ);
  const F29<F> inv = f29_inv<F>(f29_mul_c<F>(dA, dD));
  const F29<F> iA = f29_mul_c<F>(inv, dD), iD = f29_mul_c<F>(inv, dA);  // 1 / (ZZ ZZZ)
  if (A_inf) {
    ecfft_store_inf<F>(pa);
  } else {
    ecfft_store_aff<F>(pa, f29_mul_c<F>(A.X, f29_mul_c<F>(iA, A.ZZZ)), f29_mul_c<F>(A.Y, f29_mul_c<F>(iA, A.ZZ)));
  }
  if (D_inf) {
    ecfft_store_inf<F>(pb);
  } else {
    const F29<F> y = f29_canon<F>(f29_mul_c<F>(D.Y, f29_mul_c<F>(iD, D.ZZ)));
    ecfft_store_aff<F>(pb, f29_mul_c<F>(D.X, f29_mul_c<F>(iD, D.ZZZ)), f29_neg_canon<F>(y));
  }
}

// affine boundary point -> R = 2^261 canonical
template <class F>
__device__ __forceinline__ void ecfft_aff29(const Aff<F>& P, F29<F>& x, F29<F>& y) {
  x = f29_canon<F>(f29_from_r256<F>(P.x.l));
  y = f29_canon<F>(f29_from_r256<F>(P.y.l));
}

// stage 1: pairs (2g, 2g + 1), w = 1
template <class Cv>
__global__ void __launch_bounds__(256) k_ecfft_first(uint32_t* pts, uint32_t half_n) {
  using F = typename Cv::Base;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= half_n) return;
  uint32_t* pa = pts + 32ull * g;
  uint32_t* pb = pa + 16;
  const Aff<F> a = load_aff<F>(pa), b = load_aff<F>(pb);
  const bool a_inf = aff_is_inf<F>(a), b_inf = aff_is_inf<F>(b);
  F29<F> ax, ay, bx, by;
  ecfft_aff29<F>(a, ax, ay);
  ecfft_aff29<F>(b, bx, by);
  const F29<F> one = f29_const<F>(F29Consts<F>::ONE);
  const Xyzz29<F> t = b_inf ? xyzz29_inf<F>() : Xyzz29<F>{bx, by, one, one};
  ecfft_butterfly_out<F>(pa, pb, t, b_inf, ax, ay, a_inf);
}

// stage s >= 2: butterfly g on slots ia = (g >> (s-1)) 2^s + j and ia + 2^(s-1),
// j = g mod 2^(s-1), twiddle omega^(j 2^(logn - s))
template <class Cv>
__global__ void __launch_bounds__(256) k_ecfft_stage(uint32_t* pts, const uint4* __restrict__ tw, uint32_t logn,
                                                     uint32_t s) {
  using F = typename Cv::Base;
  __shared__ uint32_t w3tab[kW3Words][256];
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (1u << (logn - 1))) return;
  const uint32_t m = 1u << (s - 1), j = g & (m - 1);
  const size_t ia = ((size_t)(g >> (s - 1)) << s) + j;
  uint32_t* pa = pts + 16 * ia;
  uint32_t* pb = pa + 16ull * m;
  const Aff<F> b = load_aff<F>(pb);
  const bool b_inf = aff_is_inf<F>(b);
  Xyzz29<F> t = xyzz29_inf<F>();
  if (!b_inf && j == 0) {
    const F29<F> one = f29_const<F>(F29Consts<F>::ONE);
    F29<F> bx, by;
    ecfft_aff29<F>(b, bx, by);
    t = Xyzz29<F>{bx, by, one, one};
  } else if (!b_inf) {
    const uint4* q = tw + 3ull * ((size_t)j << (logn - s));
    const uint4 u0 = q[0], u1 = q[1], u2 = q[2];
    const uint32_t c1[6] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y & 0x0FFFFFFFu};
    const uint32_t c2[6] = {u1.z, u1.w, u2.x, u2.y, u2.z, u2.w & 0x0FFFFFFFu};
    t = ecfft_mul_codes<Cv>(c1, c2, u1.y >> 28, u2.w >> 28, b, w3tab);
  }
  const Aff<F> a = load_aff<F>(pa);
  F29<F> ax, ay;
  ecfft_aff29<F>(a, ax, ay);
  ecfft_butterfly_out<F>(pa, pb, t, xyzz29_is_inf<F>(t), ax, ay, aff_is_inf<F>(a));
}

// [scale] P per point; scale: the integer, not Montgomery
template <class Cv>
__global__ void __launch_bounds__(256) k_ecfft_scale(uint32_t* pts, uint32_t n, FeArg scale) {
  using F = typename Cv::Base;
  using Fs = typename Cv::Scalar;
  __shared__ uint32_t w3tab[kW3Words][256];
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t* p = pts + 16ull * i;
  const Aff<F> P = load_aff<F>(p);
  if (aff_is_inf<F>(P)) return;
  const Xyzz29<F> r = glv_mul_w3<Cv>(fe_of<Fs>(scale), P, w3tab);
  if (xyzz29_is_inf<F>(r)) {
    ecfft_store_inf<F>(p);
    return;
  }
  F29<F> x, y;
  xyzz29_to_aff<F>(r, x, y);
  ecfft_store_aff<F>(p, x, y);
}

}  // namespace pm

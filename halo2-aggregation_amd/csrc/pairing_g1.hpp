// pairing_g1.hpp -- BN254 G1 in affine form on the device, shared by the pairing
// decider's prep kernel (pairing_kernels.hpp) and the batch
// decider's (pairing_batch_kernels.hpp, §10h): the conversion from the ABI's
// R = 2^256 words, the curve check and the complete affine group law.
// Coordinates are canonical, so equality is limb equality.
#pragma once
#include "pairing_fq.hpp"

namespace pm {
namespace pairing {

struct G1a {
  F x, y;
  bool inf;
};
__device__ __forceinline__ bool fq_eq(const F& a, const F& b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) o |= a.l[i] ^ b.l[i];
  return o == 0;
}
// a + 6p - b for canonical b, then reduced: canonical
__device__ __forceinline__ F fq_subc(const F& a, const F& b) {
  return f29_canon<Fq>(f29_reduce3<Fq>(f29_norm<Fq>(f29_sub<Fq>(a, b, KQ::K6))));  // a < 4p: < 10p
}
__device__ __forceinline__ F fq_mulc(const F& a, const F& b) { return f29_canon<Fq>(f29_mul_c<Fq>(a, b)); }
// 8 x u64 affine R = 2^256 (all words zero: the identity; other words are taken mod p)
__device__ __forceinline__ G1a g1_load(const uint64_t* p) {
  uint32_t wx[8], wy[8], any = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint64_t a = p[i], b = p[4 + i];
    wx[2 * i] = (uint32_t)a, wx[2 * i + 1] = (uint32_t)(a >> 32);
    wy[2 * i] = (uint32_t)b, wy[2 * i + 1] = (uint32_t)(b >> 32);
    any |= wx[2 * i] | wx[2 * i + 1] | wy[2 * i] | wy[2 * i + 1];
  }
  G1a r;
  r.x = f29_canon<Fq>(f29_from_r256<Fq>(wx));  // 2^256 2^266 / 2^261 < R p: Norm, < 2p
  r.y = f29_canon<Fq>(f29_from_r256<Fq>(wy));
  r.inf = any == 0;
  return r;
}
__device__ __forceinline__ bool g1_on_curve(const G1a& p) {
  if (p.inf) return true;
  const F one = fq_one();
  const F three = f29_canon<Fq>(f29_norm<Fq>(f29_add<Fq>(f29_add<Fq>(one, one), one)));  // ONE < p: < 3p
  const F rhs = f29_canon<Fq>(f29_norm<Fq>(f29_add<Fq>(fq_mulc(fq_mulc(p.x, p.x), p.x), three)));  // < 2p
  return fq_eq(fq_mulc(p.y, p.y), rhs);
}
// complete: either operand the identity, equal, opposite; one inversion
__device__ G1a g1_add(const G1a& p, const G1a& q) {
  if (p.inf) return q;
  if (q.inf) return p;
  F num, den;
  if (fq_eq(p.x, q.x)) {
    // on the curve equal x leaves y2 = y1 or y2 = -y1 (y = 0 is its own opposite)
    if (!fq_eq(p.y, q.y) || f29_is_zero_exact<Fq>(p.y)) {
      G1a o;
      o.x = f29_zero<Fq>();
      o.y = f29_zero<Fq>();
      o.inf = true;
      return o;
    }
    const F xx = fq_mulc(p.x, p.x);
    num = f29_canon<Fq>(f29_norm<Fq>(f29_add<Fq>(f29_add<Fq>(xx, xx), xx)));  // < 3p
    den = f29_canon<Fq>(f29_norm<Fq>(f29_add<Fq>(p.y, p.y)));
  } else {
    num = fq_subc(q.y, p.y);
    den = fq_subc(q.x, p.x);
  }
  const F lam = fq_mulc(num, f29_inv<Fq>(den));  // inverse < 2p
  G1a r;
  r.x = fq_subc(fq_subc(fq_mulc(lam, lam), p.x), q.x);
  r.y = fq_subc(fq_mulc(lam, fq_subc(p.x, r.x)), p.y);
  r.inf = false;
  return r;
}

}  // namespace pairing
}  // namespace pm

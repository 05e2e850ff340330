// pairing_plan.hpp -- host plan of the BN254 pairing decider: the
// Miller loop's schedule, the Frobenius constants, the layout of the line table,
// the program both the device kernel and the host form interpret, and the launch
// geometry.  HIP-free: plain C++, read by pairing_host.hpp, the kernels and
// tests/native/pairing_host.cpp alike.
//
// Representation.  An Fp12 value is held as six Fp2 coefficients of
//   Fp12 = Fp2[w] / (w^6 - xi),   xi = 9 + u,   Fp2 = Fp[u] / (u^2 + 1),
// which is the tower Fp6 = Fp2[v]/(v^3 - xi), Fp12 = Fp6[w]/(w^2 - v) with
// v = w^2 written out: tower coefficient c_i.c_j is the coefficient of
// w^(2 j + i).  In this form
//   * a product is   c_k = sum_{i+j=k} a_i b_j + xi sum_{i+j=k+6} a_i b_j,
//     six Fp2 products per coefficient, all independent: one dependency level;
//   * a line  l0 + l1 w + l3 w^3  (l0 in Fp) multiplies in two Fp2 products and
//     one scaling per coefficient;
//   * the p^j Frobenius is  a_k -> conj^j(a_k) gamma_{j,k},
//     gamma_{j,k} = xi^(k (p^j - 1) / 6), and conjugation over Fp6 (the p^6
//     Frobenius) negates the odd coefficients: both touch one coefficient alone.
// So coefficient k of every value lives in lane k of a group of kPairG = 6 lanes
// (pairing_kernels.hpp), and the host form loops over k.
#pragma once
#include <stdint.h>

namespace pm {
namespace pairing {

// ---- curve parameter and loop scalar
constexpr uint64_t kX = 0x44e992b44a6909f1ull;       // 4965661367192848881
constexpr uint64_t kLoopLow = 0x9d797039be763ba8ull;  // 6x + 2 = 2^64 + kLoopLow (65 bits, top bit implied)
constexpr int kLoopBits = 65;

constexpr int popcount64(uint64_t v) {
  int n = 0;
  for (; v; v &= v - 1) n++;
  return n;
}
// line evaluations of one pairing: a doubling per bit below the top one, an
// addition per set bit among them, and the two Frobenius additions
constexpr int kSteps = (kLoopBits - 1) + popcount64(kLoopLow) + 2;
static_assert(kSteps == 102, "6x + 2 has 37 set bits");
// step i doubles (f is squared before its lines are multiplied in)?
constexpr bool step_doubles(int step) {
  int s = 0;
  for (int bit = kLoopBits - 2; bit >= 0; bit--) {
    if (s == step) return true;
    s++;
    if ((kLoopLow >> bit) & 1) {
      if (s == step) return false;
      s++;
    }
  }
  return false;  // pi Q and -pi^2 Q
}

// ---- line table.  Both G2 arguments are fixed per pm_pairing, so every slope
// is known on the host.  Step i holds, for the pair (A, s_g2) and then for
// (C, g2), lambda and c = lambda x_T - y_T (Fp2 each): the line at P is
//   y_P - (lambda x_P) w + c w^3.
// Host copy: canonical Montgomery R = 2^256, 4 x u64 per Fp.  Device copy: the
// same values in the kernels' R = 2^261 form, canonical, 9 limbs of 29 bits.
constexpr int kLineFp = 4;                       // lambda.c0, lambda.c1, c.c0, c.c1
constexpr int kStepFp = 2 * kLineFp;             // (A, s_g2) then (C, g2)
constexpr int kStepWords29 = kStepFp * 9;        // u32 per step on the device
constexpr int kTableWords29 = kSteps * kStepWords29;
// the device table goes on with the Frobenius constants, [j - 1][k][c0, c1], 9 limbs each,
// and ends with the program's words (kDeviceWords below)
constexpr int kFrobWords29 = 2 * 6 * 2 * 9;

// gamma_{j,k} = xi^(k (p^j - 1) / 6), j = 1, 2, canonical (not Montgomery), c0 then c1
constexpr uint64_t kFrob[2][6][2][4] = {
  {  // p^1
    {{0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0xd60b35dadcc9e470ull, 0x5c521e08292f2176ull, 0xe8b99fdd76e68b60ull, 0x1284b71c2865a7dfull},
     {0xca5cf05f80f362acull, 0x747992778eeec7e5ull, 0xa6327cfe12150b8eull, 0x246996f3b4fae7e6ull}},
    {{0x99e39557176f553dull, 0xb78cc310c2c3330cull, 0x4c0bec3cf559b143ull, 0x2fb347984f7911f7ull},
     {0x1665d51c640fcba2ull, 0x32ae2a1d0b7c9dceull, 0x4ba4cc8bd75a0794ull, 0x16c9e55061ebae20ull}},
    {{0xdc54014671a0135aull, 0xdbaae0eda9c95998ull, 0xdc5ec698b6e2f9b9ull, 0x063cf305489af5dcull},
     {0x82d37f632623b0e3ull, 0x21807dc98fa25bd2ull, 0x0704b5a7ec796f2bull, 0x07c03cbcac41049aull}},
    {{0x848a1f55921ea762ull, 0xd33365f7be94ec72ull, 0x80f3c0b75a181e84ull, 0x05b54f5e64eea801ull},
     {0xc13b4711cd2b8126ull, 0x3685d2ea1bdec763ull, 0x9f3a80b03b0b1c92ull, 0x2c145edbe7fd8aeeull}},
    {{0x2ea2c810eab7692full, 0x425c459b55aa1bd3ull, 0xe93a3661a4353ff4ull, 0x0183c1e74f798649ull},
     {0x24c6b8ee6e0c2c4bull, 0xb080cb99678e2ac0ull, 0xa27fb246c7729f7dull, 0x12acf2ca76fd0675ull}},
  },
  {  // p^2
    {{0x0000000000000001ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0xe4bd44e5607cfd49ull, 0xc28f069fbb966e3dull, 0x5e6dd9e7e0acccb0ull, 0x30644e72e131a029ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0xe4bd44e5607cfd48ull, 0xc28f069fbb966e3dull, 0x5e6dd9e7e0acccb0ull, 0x30644e72e131a029ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x3c208c16d87cfd46ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x5763473177fffffeull, 0xd4f263f1acdb5c4full, 0x59e26bcea0d48bacull, 0x0000000000000000ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
    {{0x5763473177ffffffull, 0xd4f263f1acdb5c4full, 0x59e26bcea0d48bacull, 0x0000000000000000ull},
     {0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull}},
  },
};
// the twist's Frobenius pi(x', y') = (conj(x') gamma_{1,2}, conj(y') gamma_{1,3})
// uses xi^((p-1)/3) = gamma_{1,2} and xi^((p-1)/2) = gamma_{1,3}

// ---- the program.  One pairing product e(A, s_g2) e(C, g2) and its final
// exponentiation as a straight line of operations on kSlots Fp12 registers;
// the kernel keeps the registers in LDS and the host form in an array, and
// both run this list.  Every operation is uniform over the batch.
enum Op : uint32_t {
  kOpMul = 0,       // d = a * b                     (a == b: a square)
  kOpLine = 1,      // s0 = s0 * line(step a, pair b)
  kOpFrob = 2,      // d = a^(p^b), b = 1, 2
  kOpConj = 3,      // d = a^(p^6)
  kOpScaleInv = 4,  // d = a / n, n the coefficient 0 (in Fp2) of b
};
constexpr int kSlots = 8;
constexpr uint32_t op_word(uint32_t op, uint32_t d, uint32_t a, uint32_t b) { return op | (d << 8) | (a << 16) | (b << 24); }
constexpr uint32_t op_code(uint32_t w) { return w & 255u; }
constexpr uint32_t op_d(uint32_t w) { return (w >> 8) & 255u; }
constexpr uint32_t op_a(uint32_t w) { return (w >> 16) & 255u; }
constexpr uint32_t op_b(uint32_t w) { return w >> 24; }

constexpr int kPowXOps = 62 + popcount64(kX) - 1;  // x has 63 bits
constexpr int kMillerOps = (kLoopBits - 1) + 2 * kSteps;
constexpr int kFinalOps = 12 + 3 * kPowXOps + 29;
constexpr int kProgOps = kMillerOps + kFinalOps;
constexpr int kDeviceWords = kTableWords29 + kFrobWords29 + kProgOps;

struct Program {
  uint32_t w[kProgOps];
  int n;
};
struct ProgBuilder {
  Program p{};
  constexpr void emit(uint32_t op, uint32_t d, uint32_t a, uint32_t b) { p.w[p.n++] = op_word(op, d, a, b); }
  constexpr void mul(uint32_t d, uint32_t a, uint32_t b) { emit(kOpMul, d, a, b); }
  constexpr void frob(uint32_t d, uint32_t a, uint32_t j) { emit(kOpFrob, d, a, j); }
  constexpr void conj(uint32_t d, uint32_t a) { emit(kOpConj, d, a, 0); }
  // d = a^x, left to right from the bit below the top one (d != a)
  constexpr void powx(uint32_t d, uint32_t a) {
    for (int bit = 61; bit >= 0; bit--) {
      if (bit == 61) mul(d, a, a);
      else mul(d, d, d);
      if ((kX >> bit) & 1) mul(d, d, a);
    }
  }
};
// Slot 0 starts as 1 and ends as the result.  The exponent is exactly
// (p^12 - 1) / r = (p^6 - 1)(p^2 + 1) (p^4 - p^2 + 1) / r: the easy part with one
// inversion, the hard part by the Devegili / Scott / Dahab addition chain (three
// exponentiations by x; no cofactor).
constexpr Program build_program() {
  ProgBuilder b;
  // Miller loop: f = f^2 then the two lines of each step
  for (int s = 0; s < kSteps; s++) {
    if (step_doubles(s)) b.mul(0, 0, 0);
    b.emit(kOpLine, 0, (uint32_t)s, 0);
    b.emit(kOpLine, 0, (uint32_t)s, 1);
  }
  // f^-1 = h / n:  A = f^(p^2 + p^4), B = f A = f^(1 + p^2 + p^4),
  // h = A conj(B) = f^(p^2 + p^4 + p^6 + p^8 + p^10), n = B conj(B) = f h, the
  // norm of f down to Fp2: the one inversion is of an Fp2 value
  b.frob(1, 0, 2);
  b.frob(2, 1, 2);
  b.mul(1, 1, 2);   // A
  b.mul(2, 0, 1);   // B
  b.conj(3, 2);
  b.mul(1, 1, 3);   // h
  b.mul(3, 2, 3);   // n
  b.emit(kOpScaleInv, 1, 1, 3);  // f^-1
  b.conj(2, 0);
  b.mul(0, 2, 1);   // f^(p^6 - 1)
  b.frob(1, 0, 2);
  b.mul(0, 1, 0);   // t = f^((p^6 - 1)(p^2 + 1))
  // hard part
  b.powx(1, 0);     // fu
  b.powx(2, 1);     // fu2
  b.powx(3, 2);     // fu3
  b.frob(4, 0, 1);
  b.frob(5, 0, 2);
  b.frob(6, 5, 1);
  b.mul(4, 4, 5);
  b.mul(4, 4, 6);   // y0 = t^p t^(p^2) t^(p^3)
  b.frob(5, 1, 1);
  b.conj(5, 5);     // y3 = conj(fu^p)
  b.frob(6, 2, 1);
  b.mul(6, 1, 6);
  b.conj(6, 6);     // y4 = conj(fu fu2^p)
  b.frob(7, 3, 1);
  b.mul(7, 3, 7);
  b.conj(7, 7);     // y6 = conj(fu3 fu3^p)
  b.frob(1, 2, 2);  // y2 = fu2^(p^2)
  b.conj(2, 2);     // y5 = conj(fu2)
  b.conj(0, 0);     // y1 = conj(t)
  b.mul(3, 7, 7);
  b.mul(3, 3, 6);
  b.mul(3, 3, 2);   // t0 = y6^2 y4 y5
  b.mul(5, 5, 2);
  b.mul(5, 5, 3);   // t1 = y3 y5 t0
  b.mul(3, 3, 1);   // t0 = t0 y2
  b.mul(5, 5, 5);
  b.mul(5, 5, 3);
  b.mul(5, 5, 5);   // t1 = (t1^2 t0)^2
  b.mul(3, 5, 0);   // t0 = t1 y1
  b.mul(5, 5, 4);   // t1 = t1 y0
  b.mul(3, 3, 3);
  b.mul(0, 3, 5);   // t0^2 t1
  return b.p;
}
constexpr Program kProgram = build_program();
static_assert(kProgram.n == kProgOps, "the program's length is part of the plan");

// products of the program by kind (pm_pairing_info, DESIGN §10g's level model)
constexpr int count_ops(uint32_t op) {
  int n = 0;
  for (int i = 0; i < kProgram.n; i++) n += op_code(kProgram.w[i]) == op;
  return n;
}

// ---- launch geometry.  A group of kPairG lanes per pairing product, one
// coefficient per lane; a wave holds kPairPerWave groups (lanes 60..63 repeat
// the last group's first lanes and store nothing to global memory), a block is one wave: at the
// batch sizes of a verifier (10^2 .. 10^4 items) the grid has fewer waves than
// the device has SIMDs, so blocks of one wave spread it over the most CUs.
constexpr int kPairG = 6;
constexpr int kPairWave = 64;
constexpr int kPairPerWave = kPairWave / kPairG;  // 10
constexpr int kPairBlock = kPairWave;
constexpr int kPairPerBlock = kPairPerWave * (kPairBlock / kPairWave);
constexpr int kPrepBlock = 64;  // k_pairing_prep: one lane per item
// LDS of k_pairing_run: kSlots registers and the item's two points, limb-major
// ([value][limb][lane]) so a lane's own access is conflict-free and a group's
// read of one coefficient is a broadcast
constexpr int kSlotWords = 18 * kPairWave;
constexpr int kPointWords = 4 * 9 * kPairWave;
constexpr int kLdsWords = kSlots * kSlotWords + kPointWords + kPairWave;
static_assert(kLdsWords * 4 <= 65536, "static LDS of one block");
// scratch per item between the two kernels: x_A, y_A, x_C, y_C (9 limbs each) and a flag word
constexpr int kItemWords = 4 * 9 + 1;
constexpr uint32_t kFlagAInf = 1u, kFlagCInf = 2u, kFlagSkip = 4u;
constexpr uint32_t kNotOnCurveBit = 8u;  // PM_DECIDE_NOT_ON_CURVE
inline uint32_t pairing_blocks(size_t B) { return (uint32_t)((B + kPairPerBlock - 1) / kPairPerBlock); }
inline size_t pairing_scratch_bytes(size_t B) { return B * kItemWords * sizeof(uint32_t); }
constexpr size_t kPairMaxB = size_t(1) << 24;

}  // namespace pairing
}  // namespace pm

"""Limb-level CPU model of k_pairing_run (csrc/pairing_kernels.hpp).

The model follows the kernel statement for statement, for the six lanes of one
group (lane k holds coefficient k of Fp2[w] / (w^6 - xi)):
  * Montgomery products (f29_mul_c, f29_mul2_c) at the value level, exactly:
    (a b + u v + M p) / 2^261 with M = -(a b + u v) / p mod 2^261, split back
    into nine 29-bit limbs (the generated asm itself is tests/test_fp29_asm.py's);
  * every linear step at the limb level, Python integers standing in for the
    u32 / i64 values: acc_masked, f29_add, fq_negn's K6[i] - a.l[i], the << 2
    and the 2u * q + h + (K6 - h) lines of fq2_fold_xi, f29_norm, f29_reduce3
    with its magic multiply, f29_canon and f29_to_r256.
Its data is the code's: the limb constants are read from fp29.hpp's
F29Consts<Bn254Fq>, the program, step_doubles and kFrob are asked of the compiled
pairing_plan.hpp (tests/native/plan_dump.cpp, query "pairing"), and the line
coefficients are pairing_ref's G2 walk, canonical, in the R = 2^261 form.

Every step asserts the kernel's stated invariant and raises BoundError (with a
kind) when one is broken:
  limb            a u32 expression outside [0, 2^32 - 8) before a f29_norm
  dominance       K[i] < a.l[i] in fq_negn (or in fold_xi's K6 - h1)
  operand_norm    an operand of a product with a limb >= 2^29
  product_bound   a b + u v >= 2^261 p / 1.7 (f29_mul2_c), a b >= 2^261 p (f29_mul_c)
  reduce3_input   f29_reduce3's input not Norm or >= 16p
  reduce3_output  its result negative, not Norm or >= 3p
  lds             a value stored to LDS not Norm or >= 3p
  inv_input       f29_inv's input not Norm or >= 4p
  to_r256_input   f29_to_r256's input not Norm or >= 4p
Two switches break the arithmetic on purpose (the sensitivity tests):
neg_const="K2" negates with 2p instead of 6p, and fold_reduce_shift=False drops
the reduction after fq2_fold_xi's << 2.
"""
import os
import re

import numpy as np
import pairing_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = PR.P
R = 1 << 261
M29 = (1 << 29) - 1
U32_LIMIT = (1 << 32) - 8
PINV = pow(P, -1, R)
RINV = pow(R, -1, P)
MUL2_BOUND = R * P * 10 // 17   # f29_mul2_c: a b + u v < 2^261 p / 1.7
MUL_BOUND = R * P               # f29_mul: a b < R p


class BoundError(AssertionError):
    def __init__(self, kind, msg=""):
        super().__init__("%s: %s" % (kind, msg))
        self.kind = kind


def consts():
    """F29Consts<Bn254Fq> as fp29.hpp states it"""
    txt = open(os.path.join(ROOT, "halo2-aggregation_amd", "csrc", "fp29.hpp")).read()
    blk = txt[txt.index("struct F29Consts<Bn254Fq>"):]
    blk = blk[:blk.index("\n};")]

    def arr(name):
        m = re.search(r"\b%s\[9\] = \{([^}]*)\}" % name, blk)
        return [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]

    def word(name):
        return int(re.search(r"\b%s = (0x[0-9a-f]+)u;" % name, blk).group(1), 16)

    k = {n: arr(n) for n in ("P", "ONE", "TO256", "K2", "K6", "R783")}
    k["INV"], k["QMAGIC"] = word("INV"), word("QMAGIC")
    return k


def val(a):
    return sum(x << (29 * i) for i, x in enumerate(a))


def limbs(v):
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def to_mont(x):
    """canonical x -> canonical x 2^261 mod p, 9 limbs: the device table's form (pairing_plan.hpp)"""
    return limbs(x * R % P)


def from_mont(a):
    return val(a) * RINV % P


def is_norm(a):
    return all(0 <= x <= M29 for x in a)


ZERO = [0] * 9


class Plan:
    """what plan_dump.cpp's "pairing" query answers"""

    def __init__(self, d):
        self.steps, self.ops, self.slots = d["kSteps"], d["kProgOps"], d["kSlots"]
        assert d["n"] == self.ops == len(d["prog"]) and len(d["doubles"]) == self.steps
        self.prog = d["prog"]
        self.doubles = d["doubles"]
        self.op = {n: d[n] for n in ("kOpMul", "kOpLine", "kOpFrob", "kOpConj", "kOpScaleInv")}
        f = d["frob"]
        assert len(f) == 2 * 6 * 2 * 4
        v = [sum(f[4 * i + t] << (64 * t) for t in range(4)) for i in range(24)]
        # [j - 1][k] = (c0, c1), canonical
        self.frob = [[(v[(j * 6 + k) * 2], v[(j * 6 + k) * 2 + 1]) for k in range(6)] for j in range(2)]


def line_coefs(plan, Q):
    """(lambda, lambda x_T - y_T) of every step for the fixed G2 point Q, by pairing_ref's affine
    walk in the order step_doubles gives: a tangent where the step doubles, a chord to Q where it
    does not, then the chords to pi Q and -pi^2 Q."""
    out, T = [], Q
    q1 = PR.g2_frobenius(Q)
    q2 = PR.g2_neg(PR.g2_frobenius(q1))
    for s in range(plan.steps):
        other = q1 if s == plan.steps - 2 else q2 if s == plan.steps - 1 else T if plan.doubles[s] else Q
        lam = PR.g2_slope(T, other)
        out.append((lam, PR.f2_sub(PR.f2_mul(lam, T[0]), T[1])))
        T = PR.g2_add(T, other)
    return out


def device_lines(plan, s_g2, g2):
    """[step][pair] = [lambda.c0, lambda.c1, c.c0, c.c1] in limbs: pair 0 is (A, s_g2), pair 1 (C, g2)"""
    la, lc = line_coefs(plan, s_g2), line_coefs(plan, g2)
    return [[[to_mont(x) for f2 in la[s] for x in f2], [to_mont(x) for f2 in lc[s] for x in f2]]
            for s in range(plan.steps)]


class Model:
    def __init__(self, plan, neg_const="K6", fold_reduce_shift=True):
        self.plan = plan
        self.K = consts()
        self.PL = self.K["P"]
        self.neg = self.K[neg_const]
        self.K6 = self.K["K6"]
        self.fold_reduce_shift = fold_reduce_shift
        self.frob = [[(to_mont(c0), to_mont(c1)) for c0, c1 in row] for row in plan.frob]
        # the largest values seen, as integers: LDS value, reduce3 input and output, a b + u v
        self.mx = {"lds": 0, "reduce3_in": 0, "reduce3_out": 0, "prod": 0}

    def maxima(self):
        """in units of p (prod: of p^2)"""
        return {k: (v / P / P if k == "prod" else v / P) for k, v in self.mx.items()}

    # ---- fp29.hpp
    def u32(self, a, what):
        for x in a:
            if not 0 <= x < U32_LIMIT:
                raise BoundError("limb", "%s: %#x" % (what, x))
        return a

    def norm(self, a):
        self.u32(a, "f29_norm input")
        r, c = [0] * 9, 0
        for i in range(8):
            v = a[i] + c
            if v >= 1 << 32:
                raise BoundError("limb", "f29_norm carry")
            r[i], c = v & M29, v >> 29
        r[8] = a[8] + c
        if r[8] >= 1 << 32:
            raise BoundError("limb", "f29_norm top")
        return r

    def reduce3(self, a):
        if not (is_norm(a[:8]) and 0 <= a[8] < 1 << 32) or val(a) >= 16 * P:
            raise BoundError("reduce3_input", "%.4f p" % (val(a) / P))
        self.mx["reduce3_in"] = max(self.mx["reduce3_in"], val(a))
        q = (a[8] * self.K["QMAGIC"]) >> 40
        r, c = [0] * 9, 0
        for i in range(9):
            v = a[i] - q * self.PL[i] + c
            r[i] = v & M29 if i < 8 else v
            c = v >> 29
        if r[8] < 0 or not is_norm(r) or val(r) >= 3 * P:
            raise BoundError("reduce3_output", "%.6f p" % (val(r) / P))
        self.mx["reduce3_out"] = max(self.mx["reduce3_out"], val(r))
        return r

    def red(self, a):
        return self.reduce3(self.norm(a))

    def add(self, a, b):
        return self.u32([x + y for x, y in zip(a, b)], "f29_add")

    def canon(self, a):
        assert is_norm(a) and val(a) < 4 * P
        v = list(a)
        for _ in range(3):
            d, c = [0] * 9, 0
            for i in range(9):
                x = v[i] - self.PL[i] + c
                d[i], c = x & M29, x >> 29
            if c >= 0:
                v = d
        assert val(v) == val(a) % P
        return v

    def _mont(self, t):
        m = (-t * PINV) % R
        r = limbs((t + m * P) >> 261)
        assert is_norm(r) and val(r) < 2 * P
        return r

    def _operands(self, *ops):
        for a in ops:
            if not is_norm(a):
                raise BoundError("operand_norm", str([hex(x) for x in a]))

    def mul(self, a, b):
        """f29_mul_c"""
        self._operands(a, b)
        t = val(a) * val(b)
        if t >= MUL_BOUND:
            raise BoundError("product_bound", "a b = %.2f p^2" % (t / P / P))
        self.mx["prod"] = max(self.mx["prod"], t)
        return self._mont(t)

    def mul2(self, a, b, u, v):
        """f29_mul2_c"""
        self._operands(a, b, u, v)
        t = val(a) * val(b) + val(u) * val(v)
        if t >= MUL2_BOUND:
            raise BoundError("product_bound", "a b + u v = %.2f p^2" % (t / P / P))
        self.mx["prod"] = max(self.mx["prod"], t)
        return self._mont(t)

    def inv(self, a):
        """f29_inv: canonical, safegcd inverse (0 -> 0), times 2^783 / 2^261"""
        if not is_norm(a) or val(a) >= 4 * P:
            raise BoundError("inv_input", "%.4f p" % (val(a) / P))
        c = val(self.canon(a))
        v = pow(c, -1, P) if c else 0
        return self.mul(limbs(v), self.K["R783"])

    def to_r256(self, a):
        """f29_to_r256 -> the canonical R = 2^256 value's four u64 words"""
        if not is_norm(a) or val(a) >= 4 * P:
            raise BoundError("to_r256_input", "%.4f p" % (val(a) / P))
        v = val(self.canon(self.mul(a, self.K["TO256"])))
        assert v < 1 << 256
        return [(v >> (64 * i)) & (2**64 - 1) for i in range(4)]

    # ---- pairing_kernels.hpp
    def negn(self, a):
        """fq_negn"""
        for k, x in zip(self.neg, a):
            if k < x:
                raise BoundError("dominance", "K %#x < limb %#x" % (k, x))
        return self.norm([k - x for k, x in zip(self.neg, a)])

    def f2mul(self, a, b):
        """fq2_mul"""
        nb1 = self.negn(b[1])
        return (self.mul2(a[0], b[0], a[1], nb1), self.mul2(a[0], b[1], a[1], b[0]))

    def acc(self, r, t):
        """acc_masked with the mask all ones (with the mask zero it adds nothing)"""
        return (self.u32([x + y for x, y in zip(r[0], t[0])], "acc_masked"),
                self.u32([x + y for x, y in zip(r[1], t[1])], "acc_masked"))

    def fold_xi(self, lo, hi):
        """fq2_fold_xi"""
        h0, h1 = self.red(hi[0]), self.red(hi[1])
        t0 = self.u32([x << 2 for x in h0], "h0 << 2")
        t1 = self.u32([x << 2 for x in h1], "h1 << 2")
        q0, q1 = (self.red(t0), self.red(t1)) if self.fold_reduce_shift else (t0, t1)
        for k, x in zip(self.K6, h1):
            if k < x:
                raise BoundError("dominance", "fold_xi K6 %#x < limb %#x" % (k, x))
        n0 = self.u32([2 * q0[i] + h0[i] + (self.K6[i] - h1[i]) for i in range(9)], "fold_xi n0")
        n1 = self.u32([2 * q1[i] + h1[i] + h0[i] for i in range(9)], "fold_xi n1")
        x0, x1 = self.red(n0), self.red(n1)
        return (self.red(self.add(lo[0], x0)), self.red(self.add(lo[1], x1)))

    def store(self, a, what="slot"):
        """a value on its way to LDS"""
        if not is_norm(a) or val(a) >= 3 * P:
            raise BoundError("lds", "%s: %.4f p" % (what, val(a) / P))
        self.mx["lds"] = max(self.mx["lds"], val(a))
        return a

    def put(self, r6):
        return [(self.store(c0), self.store(c1)) for c0, c1 in r6]

    def op_mul(self, a6, b6):
        out = []
        for k in range(6):
            lo, hi = (ZERO, ZERO), (ZERO, ZERO)
            for i in range(6):
                wrap = i > k
                j = k - i + (6 if wrap else 0)
                t = self.f2mul(a6[i], b6[j])
                if wrap:
                    hi = self.acc(hi, t)
                else:
                    lo = self.acc(lo, t)
            out.append(self.fold_xi(lo, hi))
        return out

    def op_line(self, f6, lc, xp, yp, inf):
        """lc = [lambda.c0, lambda.c1, c.c0, c.c1]; the flag masks the w^3 term"""
        out = []
        for k in range(6):
            nx = self.negn(xp)
            l1 = (self.mul(lc[0], nx), self.mul(lc[1], nx))
            l3 = (ZERO, ZERO) if inf else (lc[2], lc[3])
            ak = f6[k]
            t1 = self.f2mul(f6[(k + 5) % 6], l1)
            t3 = self.f2mul(f6[(k + 3) % 6], l3)
            lo, hi = (self.mul(ak[0], yp), self.mul(ak[1], yp)), (ZERO, ZERO)
            if k < 1:
                hi = self.acc(hi, t1)
            else:
                lo = self.acc(lo, t1)
            if k < 3:
                hi = self.acc(hi, t3)
            else:
                lo = self.acc(lo, t3)
            out.append(self.fold_xi(lo, hi))
        return out

    def op_frob(self, a6, j):
        out = []
        for k in range(6):
            x = a6[k]
            if j & 1:
                x = (x[0], self.negn(x[1]))
            out.append(self.f2mul(x, self.frob[j - 1][k]))
        return out

    def op_conj(self, a6):
        return [(self.reduce3(self.negn(c0)), self.reduce3(self.negn(c1))) if k & 1 else (c0, c1)
                for k, (c0, c1) in enumerate(a6)]

    def op_scale_inv(self, a6, n):
        out = []
        for k in range(6):
            di = self.inv(self.mul2(n[0], n[0], n[1], n[1]))
            ni = (self.mul(n[0], di), self.mul(self.negn(n[1]), di))
            out.append(self.f2mul(a6[k], ni))
        return out

    def run(self, lines, A, C):
        """k_pairing_run for one item as k_pairing_prep hands it over: A, C affine points of
        pairing_ref (None: the identity).  -> (ok, out_gt words (12, 4) u64)"""
        one = to_mont(1)
        assert one == self.K["ONE"]
        pts, flags = [], 0
        for b, pt in enumerate((A, C)):
            if pt is None:
                flags |= 1 << b
                pts += [list(ZERO), list(one)]
            else:
                pts += [to_mont(pt[0]), to_mont(pt[1])]
        for v in pts:
            self.store(v, "point")
        s = [None] * self.plan.slots
        s[0] = self.put([(list(one) if k == 0 else list(ZERO), list(ZERO)) for k in range(6)])
        op = self.plan.op
        for w in self.plan.prog:
            code, d, a, b = w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24
            if code == op["kOpMul"]:
                r = self.op_mul(s[a], s[b])
            elif code == op["kOpLine"]:
                d = 0
                r = self.op_line(s[0], lines[a][b], pts[2 * b], pts[2 * b + 1], (flags >> b) & 1)
            elif code == op["kOpFrob"]:
                r = self.op_frob(s[a], b)
            elif code == op["kOpConj"]:
                r = self.op_conj(s[a])
            else:
                assert code == op["kOpScaleInv"]
                r = self.op_scale_inv(s[a], s[b][0])
            s[d] = self.put(r)
        out = np.zeros((12, 4), dtype=np.uint64)
        any_diff = 0
        one256 = PR.fp_words(1)
        for k in range(6):
            w0, w1 = self.to_r256(s[0][k][0]), self.to_r256(s[0][k][1])
            for i in range(4):
                any_diff |= (w0[i] ^ (one256[i] if k == 0 else 0)) | w1[i]
            row = ((k & 1) * 3 + (k >> 1)) * 2   # the ABI's order: tower c_i.c_j is w^(2 j + i)
            out[row], out[row + 1] = w0, w1
        return (1 if any_diff == 0 else 0), out


# ---- Fp12 values of pairing_ref <-> six coefficients
def to_f12(c6):
    """six Fp2 coefficients (canonical pairs) of w^k -> pairing_ref's tower value"""
    return ((c6[0], c6[2], c6[4]), (c6[1], c6[3], c6[5]))


def from_f12(f):
    return [f[k & 1][k >> 1] for k in range(6)]


def decode(r6):
    """limbs in Montgomery form -> canonical pairs"""
    return [(from_mont(c0), from_mont(c1)) for c0, c1 in r6]

"""Adversarial inputs for the SHORT MSM paths (tests only, host only): the
small-MSM kernels (msm_small.hpp: k_small_fused, k_small_table + k_small_sum /
k_small_sum_lanes) and the many-MSM path (msm_many.hpp).  Builds on
msm_edge_util (synth, the base transforms, expected_by_dlog, to_limbs /
to_ints); same conventions: S Montgomery (n, 4), B affine Montgomery (n, 8),
D the discrete logs in Montgomery form, so that sum s_i B_i = [sum s_i d_i] G.

GLV model (the small path).  Glv<Curve> is parsed from csrc/glv.hpp.
glv_model(curve, k) restates glv_split<Cv, true>: c_i = (k G_i + 2^383) >> 384,
k1 = k - c1 a1 - c2 a2, k2 = -c1 b1 - c2 b2, signed.  small_digits(h) restates
small_recode: 33 digits of |h| with nibble + carry >= 8 -> minus 16 and a
carry, every digit negated for h < 0: magnitudes 0 .. 8, digit -8 (+8 for a
negative half) from a raw value of exactly 8.

GLV special scalars: k = (+-p1 + lambda (+-p2)) mod r for every pair of the
31-nibble half patterns

    0, 1              a half that is zero / the smallest one
    0x77...78         raw digits 8, 7 + 1, 7 + 1, ...: EVERY digit is -8 and the
                      carry ripples to the top only because of the lowest nibble
    0x88...8          -8 first, then 8 + 1 - 16 = -7 in every window, carry to the top
    0xFF...F          -1, then 15 + 1 - 16 = 0 everywhere with the carry chain
    0x77...7          +7 in every window, the largest digit that does not carry
    8 << 120          a single -8 in window 30 and its carry in window 31

and both signs of each half; every one is checked against glv_model before it
is used (k really splits into the planted halves).  With them go the constants
of msm_edge_util.CONSTANTS, lambda, lambda +- 1, r - lambda, and the scalars on
both sides of the first rounding boundaries of c1 and c2,
((2 t + 1) 2^383 // G_i) + {0, 1}.

The 33rd window.  |k_i| <= (|a1| + |a2|) / 2 + 1 resp. (|b1| + |b2|) / 2 + 1, so
the top nibble (bits 124 .. 127) of a half is at most TOP_NIBBLE_MAX = 6 on
Pallas and Vesta and 3 on BN254: with a carry it stays below 8 and window 32
(the carry window) is zero for EVERY input.  test_msm_short_edges_oracle.py
asserts this on the model; nobody needs to hunt for an input that reaches it.

Many-MSM geometry: many_geom(c) = (many_windows(c), 2^(c-1)); many_digits(s, c)
are the digits of k_many_sum: uniform width c at offset w c (bits past 255
read as zero), u > H -> u - 2 H and a carry.  (Not WinGeom, which spreads 256
bits evenly: it differs for c = 7, 6, 5.)  many_pattern_scalar has the kinds
of msm_edge_util plus "straddle:<kind>": the digit value only in the windows
whose bits cross a 32-bit word boundary (the hi-word branch of many_bits), over
a random fill.

Base gadgets beyond dup / neg / identity: phi_base (row i = phi(row src) =
(beta x, y), dlog lambda d), its negation, phi^2 and pow_base (row i =
[2^k] row src).

Collisions these kernels can meet and no large-n path can:
  * small_tree pairs quad v with v + m: in the fused kernel bases i and
    i + dist, dist = pow2(2 n) / 4, meet as raw affine points at the first
    level (equal: the doubling branch with ZZ = 1; opposite: cancellation);
    i, i + dist / 2, i + dist, i + 3 dist / 2 equal meet as equal two-term sums
    at the second.
  * k_small_sum's quad v adds terms t0 + 64 r + v, a lane of k_small_sum_lanes
    t0 + 256 r + l: bases 32 resp. 128 rows apart meet inside one serial
    accumulation when one slice holds both; every second round of gadgets
    sits at half that distance (the first tree level; the lanes' 256 -> 128
    fold), and so do all of them when kq = 1 (n = 33: no serial part).  Two
    runs of equal rows one slice apart give equal multi-term sums.
  * GLV collision: with Q = phi(P) in its own row, the term (P, second half,
    digit d) and the term (Q, first half, digit d) are the same point.  Terms
    of the first half sit on even quads / lanes and those of the second on odd
    ones, and every tree pairs equal parities until its last level, so the two
    meet only there, as whole sums: glv_collision_case makes the two sums of
    every slice equal (rows P_j with lambda b, phi(P_j) with b: first halves
    0 / b, second halves b / 0), the last addition of every tree is then
    [d] Q + [d] phi(P), the P == Q branch with ZZ != 1; with -phi(P_j) it is
    the cancellation branch and the MSM is the identity.
  * many path: entries (t, w) and (t', w) of equal (scalar, base) rows are
    equal points; k_many_sum's quads hold kq consecutive terms e = t W + w.
    At c = 8 (W = 32, kq = 1) neighbouring rows are 32 quads apart: the first
    tree level.  At c = 4 (W = 64) a slice is one row: rows 64 apart meet in
    the slice fold's serial part and rows 32 apart at its first tree level
    (the far rows 8, 40, 72, 104 / 9, 41, 73, 105).  Where W is no power of
    two (c = 7, 6, 5) the pow gadget (row n - 1 = [2^(c (W - 32))] row n - 2,
    both with every digit equal) puts equal points 32 terms apart.
small_events / many_events restate the kernels' order of additions on discrete
logs and count the additions with equal and with opposite operands per stage;
test_msm_short_edges_oracle.py asserts with them that the planted collisions
arrive where this list says.
short_mixed_case() plants all of it and returns the list of what it planted.
"""
from __future__ import annotations

import os
import re

import numpy as np

import msm_edge_util as E
import msm_ref
import pasta as P
from msm_edge_util import expected_by_dlog, synth, to_ints, to_limbs  # noqa: F401  (re-exported)

GLV_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halo2-aggregation_amd", "csrc",
                       "glv.hpp")
RUNTIME_HDR = os.path.join(os.path.dirname(GLV_HDR), "runtime.hpp")
GLV_CURVES = {"PallasCurve": P.PALLAS, "VestaCurve": P.VESTA, "Bn254Curve": P.BN254}
_GLV_NAME = {0: "PallasCurve", 1: "VestaCurve", 2: "Bn254Curve"}

SMALL_WIN = 33        # msm_plan.hpp kSmallWin
SMALL_FUSED_N = 32    # kSmallFusedN
SMALL_QUADS = 64      # kSmallQuads
SMALL_SLICES = 8      # kSmallSlices
SMALL_LANES_T = 4096  # kSmallLanesT: 2 n from which k_small_sum_lanes runs
MANY_QUADS = 64       # kManyQuads
MANY_QUAD_BUDGET = 32768   # kManyQuadBudget
# many-MSM base prefix -> window width of the GPU tests
MANY_PREFIX = ((4096, 8), (6000, 7), (8192, 6), (16384, 5), (32768, 4))
TOP_NIBBLE_MAX = {0: 6, 1: 6, 2: 3}


# ------------------------------------------------------------------ GLV model
def parse_glv(path=GLV_HDR):
    """{curve struct name: {constant name: int}} of every Glv<Curve> in glv.hpp
    (uint32_t limb arrays, little endian)."""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"template <> struct Glv<(\w+)> \{(.*?)\n\};", txt, re.S):
        d = {}
        for a in re.finditer(r"static constexpr uint32_t (\w+)\[\d+\] = \{([^}]*)\}", m.group(2)):
            limbs = [int(x.strip().rstrip("u"), 16) for x in a.group(2).split(",")]
            d[a.group(1)] = sum(v << (32 * i) for i, v in enumerate(limbs))
        out[m.group(1)] = d
    return out


_GLV = {}


def glv(curve):
    """dict(a1, b1, a2, b2, g1, g2, beta (canonical), lam) of curve 0 / 1 / 2;
    lam from a1 + b1 lam = 0 mod r, checked: [lam] G = (beta Gx, Gy)."""
    if curve not in _GLV:
        C = P.CURVES[curve]
        g = parse_glv()[_GLV_NAME[curve]]
        a1, b1, a2, b2 = g["A1"], -g["NB1"], g["A2"], g["B2"]
        beta = g["BETA"] * pow(P.R_MONT, -1, C.p) % C.p
        lam = -a1 * pow(b1, -1, C.r) % C.r
        assert pow(beta, 3, C.p) == 1 and beta != 1 and pow(lam, 3, C.r) == 1 and lam != 1
        assert (a1 + b1 * lam) % C.r == 0 and (a2 + b2 * lam) % C.r == 0
        assert C.mul(lam, C.gen) == (beta * C.gen[0] % C.p, C.gen[1])
        _GLV[curve] = dict(a1=a1, b1=b1, a2=a2, b2=b2, g1=g["G1"], g2=g["G2"], beta=beta, lam=lam)
    return _GLV[curve]


def glv_model(curve, k):
    """glv_split<Cv, true> of canonical k < r -> signed (k1, k2), k = k1 + lam k2 mod r."""
    g = glv(curve)
    c1 = (k * g["g1"] + (1 << 383)) >> 384
    c2 = (k * g["g2"] + (1 << 383)) >> 384
    return k - c1 * g["a1"] - c2 * g["a2"], -c1 * g["b1"] - c2 * g["b2"]


def small_digits(h, drop_carry_at=None):
    """small_recode of the signed half h (|h| < 2^128) -> 33 signed digits,
    sum_w d_w 16^w = h.  drop_carry_at = w forgets the carry out of window w
    (a deliberately wrong recoding, for the sensitivity tests)."""
    mag, out, carry = abs(h), [], 0
    assert mag < 1 << 128
    for w in range(SMALL_WIN):
        v = ((mag >> (4 * w)) & 15 if w < 32 else 0) + carry
        carry = 1 if v >= 8 else 0
        d = v - 16 * carry
        out.append(-d if h < 0 else d)
        if w == drop_carry_at:
            carry = 0
    return out


def small_from_digits(d):
    return sum(x << (4 * w) for w, x in enumerate(d))


HALF_PATTERNS = (("0", 0), ("1", 1), ("7..78", int("7" * 30 + "8", 16)), ("8..8", int("8" * 31, 16)),
                 ("F..F", int("F" * 31, 16)), ("7..7", int("7" * 31, 16)), ("8<<120", 8 << 120))
ROUND_T = range(4)
_SPECIALS = {}


def glv_special_scalars(curve):
    """[(name, canonical k, (k1, k2))]: every pair of half patterns with every
    sign pair (name "glv:<+-p1>,<+-p2>", the planted halves asserted on the
    model), then the constants, lambda's neighbours and the rounding
    boundaries of c1 / c2 (halves from the model)."""
    if curve in _SPECIALS:
        return _SPECIALS[curve]
    C = P.CURVES[curve]
    g = glv(curve)
    lam, r = g["lam"], C.r
    out, seen = [], set()

    def add(name, k, halves=None):
        k %= r
        m = glv_model(curve, k)
        assert halves is None or m == halves, (curve, name, m, halves)
        assert (m[0] + lam * m[1] - k) % r == 0
        if (name[:4], k) not in seen:   # a zero half has one sign
            seen.add((name[:4], k))
            out.append((name, k, m))

    for n1, p1 in HALF_PATTERNS:
        for n2, p2 in HALF_PATTERNS:
            for s1 in (1, -1):
                for s2 in (1, -1):
                    add(f"glv:{'+-'[s1 < 0]}{n1},{'+-'[s2 < 0]}{n2}", s1 * p1 + lam * s2 * p2, (s1 * p1, s2 * p2))
    for nm in E.CONSTANTS:
        add("const:" + nm, E.constant_scalar(curve, nm))
    for nm, k in (("lam", lam), ("lam+1", lam + 1), ("lam-1", lam - 1), ("r-lam", r - lam)):
        add("lam:" + nm, k)
    for i in (1, 2):
        for t in ROUND_T:
            for e in (0, 1):
                add(f"round:c{i},t{t},+{e}", ((2 * t + 1) << 383) // g[f"g{i}"] + e)
    _SPECIALS[curve] = out
    return out


def sym_special_scalars(curve):
    """The GLV specials with k1 == k2 != 0: on the rows P, phi(P) every digit
    of (P, second half) equals the digit of (phi(P), first half)."""
    return [(nm, k, m) for nm, k, m in glv_special_scalars(curve) if m[0] == m[1] != 0]


# --------------------------------------------------------- many-MSM geometry
def many_windows(c):
    return 255 // c + 1 if 255 % c == 0 else (255 + c - 1) // c


def many_geom(c):
    """(W, H) of msm_plan.hpp many_windows(c) and the largest digit 2^(c-1)."""
    return many_windows(c), 1 << (c - 1)


def many_bytes_per_base(c):
    return (many_windows(c) << (c - 1)) << 7


def many_budget(path=RUNTIME_HDR):
    """(kManyTabBudget, kManyTabCap) read from runtime.hpp (held equal to msm_plan.hpp's there)."""
    txt = open(path).read()
    v = {}
    for nm in ("kManyTabBudget", "kManyTabCap"):
        m = re.search(r"constexpr size_t %s = size_t\((\d+)\) << (\d+);" % nm, txt)
        v[nm] = int(m.group(1)) << int(m.group(2))
    return v["kManyTabBudget"], v["kManyTabCap"]


def many_pick_c(n, budget=None):
    budget = many_budget()[0] if budget is None else budget
    for c in range(8, 4, -1):
        if n * many_bytes_per_base(c) <= budget:
            return c
    return 4


def many_digits(s, c, drop_carry_at=None):
    """k_many_sum's digits of canonical s < r -> (digits, carries), digits[w] in
    [-(H - 1), H]; the top window never carries for s < 2^255."""
    W, H = many_geom(c)
    digits, carries, carry = [], [], 0
    for w in range(W):
        u = ((s >> (w * c)) & ((1 << c) - 1)) + carry
        carry = 1 if u > H else 0
        digits.append(u - 2 * H * carry)
        carries.append(carry)
        if w == drop_carry_at:
            carry = 0
    return digits, carries


def many_from_digits(d, c):
    return sum(x << (w * c) for w, x in enumerate(d))


def straddle_windows(c):
    """Windows of width c whose bits cross a 32-bit word boundary (inside bits 0 .. 255)."""
    return [w for w in range(many_windows(c)) if (w * c) // 32 != (w * c + c - 1) // 32 and w * c + c <= 256]


MANY_KINDS = ("half", "half+1", "half-1", "ones", "alt")


def many_pattern_scalar(curve, c, kind, seed=0x5A17):
    """Canonical scalar whose raw c-bit digit is the `kind` value (msm_edge_util:
    half, half+1, half-1, ones, alt) in every whole window below bit 256, or,
    kind "straddle:<kind>" ("straddle" = "straddle:half+1"), only in the
    windows that cross a 32-bit word boundary, over a random fill.  Top bits
    are cleared until the value is < r (clear_top)."""
    C = P.CURVES[curve]
    W = many_windows(c)
    if kind == "straddle":
        kind = "straddle:half+1"
    if kind.startswith("straddle:"):
        kind = kind[len("straddle:"):]
        wins = straddle_windows(c)
        s = P.synth_scalar(seed + 977 * c + MANY_KINDS.index(kind), c, C.r, C.scalar_bits)
    else:
        wins, s = [w for w in range(W) if w * c + c <= 256], 0
    for w in wins:
        k = kind if kind != "alt" else ("half", "half+1")[w & 1]
        s &= ~(((1 << c) - 1) << (w * c))
        s |= E._digit_value(k, c) << (w * c)
    s, _ = E.clear_top(s & ((1 << 256) - 1), C.r)
    return s


def many_special_scalars(curve, c):
    """[(name, canonical int)]: constants, whole-scalar patterns of width c and
    (c = 7, 6, 5) the straddle patterns."""
    out = [("const:" + k, E.constant_scalar(curve, k)) for k in E.CONSTANTS]
    out += [("pattern:" + k, many_pattern_scalar(curve, c, k)) for k in MANY_KINDS]
    if straddle_windows(c):
        out += [("straddle:" + k, many_pattern_scalar(curve, c, "straddle:" + k)) for k in MANY_KINDS]
    return out


def many_kq(ns, c):
    """kq of msm_many_impl (msm_plan.hpp many_kq) for a call of MSM lengths ns."""
    return max(1, -(-sum(ns) * many_windows(c) // MANY_QUAD_BUDGET))


def many_quad_starts(ns, c):
    """Every quad's first term (MSM index, scalar row t, window w) with w != 0:
    the quads that start mid-scalar and recompute the carry from window 0."""
    W, kq = many_windows(c), many_kq(ns, c)
    out = []
    for i, n in enumerate(ns):
        for e in range(0, n * W, kq):
            if e % W:
                out.append((i, e // W, e % W))
    return out


# ----------------------------------------------------------- small-MSM geometry
def small_geom(n):
    """(path, kq, ns) of msm_small_impl (msm_plan.hpp small_plan): "fused" (n <= 32: one term per quad),
    "quads" or "lanes" (2 n >= 4096)."""
    T = 2 * n
    if n <= SMALL_FUSED_N:
        return "fused", 1, -(-T // SMALL_QUADS)
    per = 256 if T >= SMALL_LANES_T else SMALL_QUADS
    kq = max(1, -(-T // (per * SMALL_SLICES)))
    return ("lanes" if T >= SMALL_LANES_T else "quads"), kq, -(-T // (per * kq))


def pow2(x):
    c = 1
    while c < x:
        c <<= 1
    return c


# --------------------------------------------------------------- base gadgets
def _set_base(curve, B, D, i, pt, dlog_mont):
    B[i] = np.array(P.point_to_limbs(P.CURVES[curve], pt), dtype=np.uint64)
    D[i] = np.array(P.to_limbs(dlog_mont), dtype=np.uint64)


def phi_base(curve, B, D, i, src, power=1, negate=False):
    """Row i becomes phi^power(row src) = (beta^power x, y) with dlog
    lam^power d (negate: (beta^power x, -y), dlog -lam^power d)."""
    C, g = P.CURVES[curve], glv(curve)
    x, y = P.from_limbs(B[src, :4]), P.from_limbs(B[src, 4:])
    d = P.from_limbs(D[src])
    assert (x or y) and d
    x = x * pow(g["beta"], power, C.p) % C.p          # Montgomery form is linear
    d = d * pow(g["lam"], power, C.r) % C.r
    if negate:
        y, d = C.p - y, C.r - d
    B[i, :4] = np.array(P.to_limbs(x), dtype=np.uint64)
    B[i, 4:] = np.array(P.to_limbs(y), dtype=np.uint64)
    D[i] = np.array(P.to_limbs(d), dtype=np.uint64)


def phi_neg_base(curve, B, D, i, src):
    phi_base(curve, B, D, i, src, 1, True)


def phi2_base(curve, B, D, i, src):
    phi_base(curve, B, D, i, src, 2)


def pow_base(curve, B, D, i, src, k):
    """Row i becomes [2^k] row src (one host scalar multiplication)."""
    C = P.CURVES[curve]
    d = P.from_limbs(D[src]) * pow(2, k, C.r) % C.r
    _set_base(curve, B, D, i, C.mul(d * pow(P.R_MONT, -1, C.r) % C.r, C.gen), d)


def _mont(curve, k):
    C = P.CURVES[curve]
    return np.array(P.to_limbs(k * P.R_MONT % C.r), dtype=np.uint64)


# ------------------------------------------------------------------ the cases
SMALL_GADGETS = ("dup", "neg", "identity", "phi", "phi-neg", "phi2", "quad", "special")
MANY_GADGETS = ("special", "dup", "neg", "identity", "phi", "run")


def gadget_distance(n, path):
    """Rows between the two bases of a gadget: the first tree level of the
    fused kernel (pow2(2 n) / 4); 64 terms for the quads and 256 for the lanes,
    the stride of one quad's / lane's serial accumulation (every second round
    of gadgets sits at half of it: the first tree level, resp. the lanes' 256 ->
    128 fold).  With one term per quad (kq = 1) there is no serial
    accumulation and 64 terms apart is another slice: half of it there too."""
    if path == "fused":
        return max(1, pow2(2 * n) // 4)
    return {"quads": 32, "lanes": 128}[path] // (1 if small_geom(n)[1] > 1 else 2)


def _plant_pair(curve, kind, S, B, D, a, b, sm):
    """Gadget `kind` on rows a < b: the base of row b derived from row a's,
    both scalars sm (identity: row a the identity with sm, row b scalar 0)."""
    if kind == "dup":
        E.dup_base(B, D, a, b)
    elif kind == "neg":
        E.neg_base(curve, B, D, b, a)
    elif kind == "phi":
        phi_base(curve, B, D, b, a)
    elif kind == "phi-neg":
        phi_neg_base(curve, B, D, b, a)
    elif kind == "phi2":
        phi2_base(curve, B, D, b, a)
    if kind == "identity":
        E.identity_base(B, D, a)
        S[a] = sm
        S[b] = 0
    else:
        S[a] = S[b] = sm


def _inputs(curve, n, seed, bases, dlogs):
    """E.synth, or (dlogs given: a window of a base set that does not start at
    base 0) synthetic scalars beside copies of the given bases and dlogs."""
    if dlogs is None:
        return E.synth(curve, n, seed, bases)
    S = msm_ref.synth_scalars(curve, P.SEED_SCALARS ^ seed, 0, n)
    return S, np.array(bases, dtype=np.uint64).reshape(n, 8), np.array(dlogs, dtype=np.uint64).reshape(n, 4)


def _small_mixed(curve, n, path, rot, seed, bases, dlogs=None):
    geom = small_geom(n)
    assert geom[0] == path, (n, geom, path)
    S, B, D = _inputs(curve, n, seed, bases, dlogs)
    sp = glv_special_scalars(curve)
    sym = sym_special_scalars(curve)
    used = np.zeros(n, dtype=bool)
    planted = []
    dist = gadget_distance(n, path)
    state = {"sp": rot, "sym": rot}

    def nxt(kind):
        which, lst = ("sym", sym) if kind in ("phi", "phi-neg") else ("sp", sp)   # phi pairs: equal halves, the GLV collision
        nm, k, _ = lst[state[which] % len(lst)]
        state[which] += 1
        return nm, _mont(curve, k)

    def free(rows):
        return all(0 <= r < n and not used[r] for r in rows)

    def take(kind, rows, nm):
        used[list(rows)] = True
        planted.append((kind, [int(r) for r in rows], nm))

    # anchors: row 0, the last pair, and evenly spread; at each the next gadget in turn
    if path == "fused" or n < 128:
        anchors = list(range(n))
    else:
        # both sides of every slice cut (the pair then meets in the slice fold
        # only) and evenly in between (inside one serial accumulation)
        rows_per_slice = geom[1] * (128 if path == "lanes" else 32)
        anchors = [0] + [s * rows_per_slice - 1 for s in range(1, geom[2])]
        anchors += list(range(3, n, max(7, n // 400 * 2 + 1)))
    def rows_of(kind, a):
        if kind == "special":
            return [a]
        if kind == "quad":   # four equal rows half a distance apart: equal two-term sums one tree level up
            h = max(1, dist // 2)
            rows = [a, a + h, a + 2 * h, a + 3 * h]
            if len(set(rows)) == 4 and free(rows):
                return rows
        d = dist // 2 if path != "fused" and (gi - gi0) // len(SMALL_GADGETS) & 1 else dist
        return [a, a + d]

    gi = gi0 = rot + rot // len(sp)   # rot + len(sp): the same scalars, the gadgets one further
    for a in anchors:
        for tr in range(len(SMALL_GADGETS)):   # the gadget whose turn it is, else the next one that fits here
            kind = SMALL_GADGETS[(gi + tr) % len(SMALL_GADGETS)]
            rows = rows_of(kind, a)
            if len(set(rows)) == len(rows) and free(rows):
                break
        else:
            continue
        gi += tr == 0
        nm, sm = nxt(kind)
        if kind == "special":
            S[a] = sm
        elif kind == "quad":
            for r in rows[1:]:
                E.dup_base(B, D, rows[0], r)
            S[rows] = sm
        else:
            _plant_pair(curve, kind, S, B, D, rows[0], rows[1], sm)
        take(kind, rows, nm)
    # every row still free: a special scalar on its ordinary base
    for a in np.flatnonzero(~used):
        nm, sm = nxt("special")
        S[a] = sm
        take("special", [int(a)], nm)
    # two runs of g consecutive equal (scalar, base) rows one slice apart: equal
    # multi-term sums in two quads / lanes and in two slices (overwrites
    # earlier gadgets' rows; the list keeps only gadgets left intact)
    if path != "fused":
        rows_per_slice = geom[1] * (128 if path == "lanes" else 32)
        g = min(rows_per_slice, n // 8)
        a0 = (n // 3) // rows_per_slice * rows_per_slice
        if geom[2] > 2 and a0 + rows_per_slice + g <= n and g >= 2:
            runs = [list(range(a0, a0 + g)), list(range(a0 + rows_per_slice, a0 + rows_per_slice + g))]
            hit = set(runs[0]) | set(runs[1])
            # (the rows a broken gadget leaves outside the runs stay valid rows)
            planted = [p for p in planted if not hit & set(p[1])]
            nm, sm = nxt("special")
            src = runs[0][0]
            if not D[src].any():   # not a run of identities
                E.dup_base(B, D, next(r for r in range(n) if D[r].any()), src)
            for r in runs[0] + runs[1]:
                if r != src:
                    E.dup_base(B, D, src, r)
                S[r] = sm
            S[src] = sm
            planted.append(("run", runs[0] + runs[1], nm))
    return S, B, D, planted


def _many_mixed(curve, n, c, rot, seed, bases, dlogs=None):
    """One MSM of the many path (n rows of its base window)."""
    W, H = many_geom(c)
    S, B, D = _inputs(curve, n, seed, bases, dlogs)
    sp = many_special_scalars(curve, c)
    sym = sym_special_scalars(curve)
    planted = []
    k = rot
    a = 0
    gi = rot
    use_pow = bool(W & (W - 1)) and n >= 8
    end = n - 2 if use_pow else n
    # every row belongs to a gadget, so gadget rows lie on both sides of every
    # quad boundary e0 + v kq whatever the call's kq is
    while a < end:
        kind = MANY_GADGETS[gi % len(MANY_GADGETS)]
        gi += 1
        nm, sv = sp[k % len(sp)]
        k += 1
        if kind == "special" or a + 1 >= end:
            S[a] = _mont(curve, sv)
            planted.append(("special", [a], nm))
            a += 1
            continue
        if kind == "run":   # 4 equal rows (c = 8: two whole 64-term slices; c = 4: four)
            rows = list(range(a, min(end, a + 4)))
            for r in rows[1:]:
                E.dup_base(B, D, a, r)
            S[rows] = _mont(curve, sv)
            planted.append(("run", rows, nm))
            a += len(rows)
            continue
        if kind == "phi":
            nm, sv, _ = sym[k % len(sym)]
        _plant_pair(curve, kind, S, B, D, a, a + 1, _mont(curve, sv))
        planted.append((kind, [a, a + 1], nm))
        a += 2
    # pow gadget where W is no power of two: row n - 1 = [2^(c (W - 32))] row
    # n - 2, every digit of both scalars equal (half-1: no carries): the entries
    # (n - 2, w) and (n - 1, w - (W - 32)) are one point, 32 terms apart
    # far rows: where a slice is a whole number of rows (c = 4: one row, so
    # neighbours never meet) the slice fold adds rows 64 apart serially and
    # pairs rows 32 apart at its first tree level: P P P P on rows 8, 40, 72,
    # 104 and P -P P -P on rows 9, 41, 73, 105
    if n >= 112:
        src = next(r for r in range(n) if D[r].any())
        for kind, rows in (("far-dup", [8, 40, 72, 104]), ("far-neg", [9, 41, 73, 105])):
            hit = [p for p in planted if set(rows) & set(p[1])]
            planted = [p for p in planted if p not in hit]
            nm, sv = sp[(k + rows[0]) % len(sp)]
            if not D[rows[0]].any():
                E.dup_base(B, D, src, rows[0])
            for i, r in enumerate(rows[1:], 1):
                if kind == "far-neg" and i & 1:
                    E.neg_base(curve, B, D, r, rows[0])
                else:
                    E.dup_base(B, D, rows[0], r)
            S[rows] = _mont(curve, sv)
            planted.append((kind, rows, nm))
            # the rows a broken gadget leaves behind keep their scalars on valid bases
            planted += [("special", [r], p[2]) for p in hit for r in p[1] if r not in rows]
    if use_pow:
        pow_base(curve, B, D, n - 1, n - 2, c * (W - 32))
        S[n - 2] = S[n - 1] = _mont(curve, many_pattern_scalar(curve, c, "half-1"))
        planted.append(("pow", [n - 2, n - 1], "pattern:half-1"))
    return S, B, D, planted


def short_mixed_case(curve, n, path, c=None, rot=0, seed=0, bases=None, dlogs=None):
    """Random scalars and bases of n rows with the special scalars and base
    gadgets of `path` ("fused", "quads", "lanes": the small-MSM kernel that n
    selects; "many": one MSM of the many path at window width c) planted ->
    (S, B, D, planted), planted a list of (gadget, rows, scalar name).  The
    special scalars are taken in turn starting at number `rot`, so cases that
    are too short to hold all of them cover them between them.  bases: the
    synthetic bases (seed SEED_BASES ^ seed) when the caller has them; with
    dlogs as well, any bases and their discrete logs (Montgomery)."""
    if path == "many":
        return _many_mixed(curve, n, c, rot, seed, bases, dlogs)
    return _small_mixed(curve, n, path, rot, seed, bases, dlogs)


_ROTS = {}


def covering_rots(curve, n, path):
    """Values of `rot` whose small-path cases of n rows hold every GLV special
    scalar between them (each case starts at the first one not yet planted),
    and every gadget that fits into n rows."""
    if (curve, n, path) not in _ROTS:
        names = [nm for nm, _, _ in glv_special_scalars(curve)]
        dummy = np.ones((n, 8), np.uint64)
        seen, rots = set(), []

        def case(rot):
            pl = _small_mixed(curve, n, path, rot, 0, dummy)[3]
            return {nm for _, _, nm in pl}, None

        while len(seen) < len(names):
            first = next(i for i, nm in enumerate(names) if nm not in seen)
            for j in range(len(SMALL_GADGETS)):   # a phi pair takes its scalar from the equal-halves list: next gadget
                rot = first + j * len(names)
                got, kd = case(rot)
                if names[first] in got:
                    break
            assert names[first] in got
            seen |= got
            rots.append(rot)
        # short cases hold one gadget each: a round of all of them, from the
        # first scalar with 0x77...78 in a half on (a non-zero digit in every window)
        rich = names.index("glv:+7..78,+7..78") // len(SMALL_GADGETS) * len(SMALL_GADGETS)
        if n > 1 and len([p for p in _small_mixed(curve, n, path, rich, 0, dummy)[3] if len(p[1]) > 1]) <= 2:
            rots += list(range(rich, rich + len(SMALL_GADGETS)))
        _ROTS[(curve, n, path)] = rots
    return _ROTS[(curve, n, path)]


def whole_array_case(curve, n, name):
    """Every scalar equal to the GLV special `name` -> Montgomery (n, 4)."""
    k = {nm: v for nm, v, _ in glv_special_scalars(curve)}[name]
    return np.repeat(_mont(curve, k)[None, :], n, axis=0)


def glv_collision_case(curve, n, pattern="7..78", negate=False, seed=0, bases=None):
    """Rows 2 j = P_j with scalar lam b, rows 2 j + 1 = phi(P_j) (negate:
    -phi(P_j)) with scalar b, b the half pattern: halves (0, b) and (b, 0), so
    in every window the first-half terms and the second-half terms of a slice
    have the same sum (negate: opposite sums) -> (S, B, D).  An odd last row
    gets a zero scalar."""
    C, g = P.CURVES[curve], glv(curve)
    b = dict(HALF_PATTERNS)[pattern]
    assert glv_model(curve, g["lam"] * b % C.r) == (0, b) and glv_model(curve, b) == (b, 0)
    S, B, D = E.synth(curve, n, seed, bases)
    for j in range(0, n - 1, 2):
        phi_base(curve, B, D, j + 1, j, 1, negate)
    S[0::2] = _mont(curve, g["lam"] * b % C.r)
    S[1::2] = _mont(curve, b)
    if n & 1:
        S[n - 1] = 0
    return S, B, D


MANY_FRONT = 1024   # many_batch: the kq = 1 call's leading windows lie below this base, the other call's from it on


def many_batch(nb, c, big):
    """(ns, offsets) of one many-MSM call on a prefix of nb bases: n_i from 1
    to about 600 in disjoint windows, the last one the last base of the prefix.
    big = False: sum n_i W <= 32768 (kq = 1), windows [0, MANY_FRONT) and the
    end of the prefix; big = True: kq > 1 and kq does not divide W, windows from
    MANY_FRONT on and just before the other call's last windows.  The two
    calls share only the one-row window at the last base."""
    W = many_windows(c)
    if big:
        ns = [1, 2, 3, 17, 64, 65, 130, 257, 600, 331, 600, 509, 1]
        while W % many_kq(ns, c) == 0:
            ns.insert(0, 487)
    else:
        ns = [1, 2, 3, 5, 33, 64, 97, 130, 200, 1]
        while sum(ns) * W > MANY_QUAD_BUDGET:
            ns[ns.index(max(ns))] //= 2
    offs, o = [], MANY_FRONT if big else 0
    for n in ns[:-2]:
        offs.append(o)
        o += n
    assert big or o <= MANY_FRONT
    tail = nb - 1 - (256 if big else 0)          # 256 >= the kq = 1 call's window before the last base
    offs += [tail - ns[-2], nb - 1]
    assert offs[-2] >= o and (not big or many_batch(nb, c, False)[0][-2] <= 256)
    return ns, offs


def many_batch_case(curve, c, ns, offs, B, D, seed=0):
    """Every MSM of the call a mixed case of its own over its window of the
    base set: B (nb, 8) and D (nb, 4) are changed in place inside the windows
    (one-row windows keep their base) -> (S, planted): the concatenated
    Montgomery scalars and [(MSM index, gadget, rows, scalar name)]."""
    Ss, planted = [], []
    for i, (n, o) in enumerate(zip(ns, offs)):
        S, b, d, pl = _many_mixed(curve, n, c, i, seed + i, B[o:o + n], D[o:o + n])
        B[o:o + n], D[o:o + n] = b, d
        Ss.append(S)
        planted += [(i, k, rws, nm) for k, rws, nm in pl]
    return np.concatenate(Ss), planted


# ------------------------------------------------- which additions collide
# The kernels' order of additions restated on discrete logs: a point [a] G is
# the integer a mod r, so P == Q is a == b and P == -Q is a + b == 0.  Counts,
# per stage, the additions that meet equal operands ("double": the P == Q
# branch of xyzz29_add_q / xyzz29_add) and opposite ones ("cancel"); a
# "+multi" count is the same with an operand that is already a sum of several
# terms (ZZ != 1 whatever the table holds).  Tests only: it shows that the
# planted collisions reach those branches, and its total must restate the MSM.
class Events(dict):
    def add(self, a, b, stage):
        """a, b = (dlog, terms) or None (the identity passes through)."""
        if a is None or b is None:
            return b if a is None else a
        if a[0] == b[0]:
            kind = "double"
        elif (a[0] + b[0]) % self.r == 0:
            kind = "cancel"
        else:
            kind = None
        if kind:
            self[(stage, kind)] = self.get((stage, kind), 0) + 1
            if a[1] > 1 or b[1] > 1:
                self[(stage, kind + "+multi")] = self.get((stage, kind + "+multi"), 0) + 1
        v = (a[0] + b[0]) % self.r
        return (v, a[1] + b[1]) if v else None

    def tree(self, slots, stage):
        """small_tree over slots (a power of two of them, None = identity)."""
        m = len(slots) >> 1
        while m:
            for v in range(m):
                slots[v] = self.add(slots[v], slots[v + m], f"{stage}{m}")
            m >>= 1
        return slots[0]

    def fold(self, parts):
        """small_fold / k_many_sum's last block over the slices' partial sums."""
        if len(parts) == 1:
            return parts[0]
        q = pow2(min(len(parts), 64))
        slots = [None] * q
        for v in range(min(q, len(parts))):
            for u in range(v, len(parts), 64):
                slots[v] = self.add(slots[v], parts[u], "fold-serial")
        return self.tree(slots, "fold")

    def count(self, kind, stage=""):
        return sum(n for (st, k), n in self.items() if k == kind and st.startswith(stage))


def _canon(curve, A):
    C = P.CURVES[curve]
    rinv = pow(P.R_MONT, -1, C.r)
    return [int(a) * rinv % C.r for a in E.to_ints(A)]


def small_events(curve, S, D):
    """The small-MSM path of the case (S, D Montgomery; a zero dlog is an
    identity base) -> (Events, total): stages "serial" (one quad's or lane's
    accumulation), "lanes128" / "lanes64" (the lanes kernel's two one-to-one
    folds), "tree<m>" (small_tree level m), "fold-serial" / "fold<m>"; total =
    sum_j 16^j (window sum j) mod r, which must be sum s_i d_i."""
    C, g = P.CURVES[curve], glv(curve)
    ev = Events()
    ev.r = C.r
    sc, dl = _canon(curve, S), _canon(curve, D)
    n = len(sc)
    path, kq, ns = small_geom(n)
    T = 2 * n
    dig = []   # per term: 33 digits and the term's dlog
    for s, d in zip(sc, dl):
        k1, k2 = glv_model(curve, s) if d else (0, 0)
        dig.append((small_digits(k1), d))
        dig.append((small_digits(k2), d * g["lam"] % C.r))
    per = 256 if path == "lanes" else SMALL_QUADS
    total = 0
    for j in range(SMALL_WIN):
        term = lambda t: ((dig[t][0][j] * dig[t][1]) % C.r, 1) if dig[t][0][j] and dig[t][1] else None  # noqa: E731
        parts = []
        for s in range(ns):
            t0 = s * kq * per
            acc = [None] * per
            for v in range(per):
                for r in range(kq):
                    t = t0 + r * per + v
                    if t >= T:
                        break
                    acc[v] = ev.add(acc[v], term(t), "serial")
            if path == "lanes":
                acc = [ev.add(acc[v], acc[v + 128], "lanes128") for v in range(128)]
                acc = [ev.add(acc[v], acc[v + 64], "lanes64") for v in range(64)]
                parts.append(ev.tree(acc, "tree"))
            else:
                parts.append(ev.tree(acc[:pow2(min(SMALL_QUADS, T - t0))], "tree"))
        w = ev.fold(parts)
        total = (total + (w[0] if w else 0) * pow(16, j, C.r)) % C.r
    return ev, total


def many_events(curve, c, ns, S, Ds, kq=None):
    """k_many_sum on the call (ns, concatenated S, Ds = the dlog window of each
    MSM) -> (Events, [total of each MSM]); stages as in small_events."""
    C = P.CURVES[curve]
    W, H = many_geom(c)
    kq = many_kq(ns, c) if kq is None else kq
    ev = Events()
    ev.r = C.r
    sc = _canon(curve, S)
    totals, s0 = [], 0
    for n, D in zip(ns, Ds):
        dl = _canon(curve, D)
        dig = [many_digits(s, c)[0] for s in sc[s0:s0 + n]]
        s0 += n
        te, per = n * W, MANY_QUADS * kq
        parts = []
        for e0 in range(0, te, per):
            e1 = min(te, e0 + per)
            slots = [None] * pow2(min(-(-(e1 - e0) // kq), MANY_QUADS))
            for v in range(len(slots)):
                for e in range(e0 + v * kq, min(e0 + (v + 1) * kq, e1)):
                    t, w = divmod(e, W)
                    x = dig[t][w] * pow(2, c * w, C.r) * dl[t] % C.r
                    slots[v] = ev.add(slots[v], (x, 1) if x else None, "serial")
            parts.append(ev.tree(slots, "tree"))
        w = ev.fold(parts)
        totals.append(w[0] if w else 0)
    return ev, totals

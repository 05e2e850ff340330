"""Adversarial proofs for the batched multiopen accumulator (tests only, host
only): a model of which additions the device performs for a given proof, and
gadgets that plant scalars and relations between points so that the special
branches of the group law are reached.

Why the accumulator can be driven exactly.  With caller challenges every
coefficient is a known function of (x, v, u) (oracle/accum.py accumulate_msm):
W_j carries u^(S-1-j) in w and u^(S-1-j) omega^rot_j x in zw, a commitment of f
the sum over its queries of u^(S-1-j) v^(m_j-1-i), h_i that of H times xn^i,
and g1 carries -eval_multi in e.  Every synthetic point is [a]G with a known
a, so each output is [sum c_t a_t]G: a third check beside the Python oracle and
the C port.  pm_accum_batch_proofs from bytes is OUT OF SCOPE for the planted
relations: its challenges are hashed from the points, so no coefficient can be
chosen (its points still reach the same kernels).

term_plan restates acc_terms and its pairing loop (accum_plan.hpp): the f
slots (one per distinct commitment in first-use order over the rotation sets
in ascending order), the h_i, W_0..W_{S-1} for w and again for zw, g1; with
each term's output, source and integer coefficient, and the (t, t + 1) pairs
of the two-term lanes.

Digit models.  glv_model (msm_short_edge_util) is glv_split<Cv, true>.
w3_digits restates w3_codes: 43 base-8 digits in [-4, 4] of |half|, u = v +
carry, u > 4 -> u - 8 and a carry (u = 8: digit 0, carry 1), all negated for a
negative half.  naf_digits restates naf128: digit i = bit i+1 of 3 k minus bit
i+1 of k, 128 positions.  deal() is k_acc_termadd's round-robin: the nonzero
digits of k1 in ascending position, then k2's, rank n to lane n mod S.

acc_path restates the thresholds of accum_plan.hpp acc_path from kAccLaneBudget and
kAccSumLanes as parsed from the header, so a test can assert the path it means
to hit and fails when a threshold moves.

Addition-order models work on discrete logs (a point [a]G is a mod r; phi(P)
has dlog lambda a, so "a + b lambda" is just an integer mod r and P == Q is
equality): AccEvents extends msm_short_edge_util.Events with the events
  dbl, cancel           xyzz29_add / xyzz29_add_q with equal / opposite operands
  inf+Q, inf+inf        an identity operand passing through
  madd_dbl, madd_cancel xyzz29_madd's two branches
  restart_after_cancel  xyzz29_madd's acc_inf arm taken after a cancellation
sum_events is k_acc_sum (lane and quad form), termmul_events the window loops
of glv_mul_w3 / glv_mul_w3n, termadd_events k_acc_termadd's lane sums and
butterfly.

No collision between partial sums of k_acc_termadd is planted, and none is
claimed.  Every partial sum there (a lane's running sum, a butterfly operand)
is (a + lambda b) d with a, b sums of digits d_i 2^i of k1 resp. k2 over a set
of table positions, and two operands that meet always have DISJOINT position
sets.  X == +-Y for d of prime order means (a_X -+ a_Y) + lambda (b_X -+ b_Y) =
0 mod r: both coordinates are signed-digit strings supported inside the NAFs
of k1 and k2, so non-adjacent, and by the uniqueness of the NAF they are the
NAFs of a lattice vector (a', b') of {a + lambda b = 0}.  It is not (0, 0)
unless both operands are the identity (disjoint supports), so its NAFs, with
the signs of one operand flipped, would have to be contained in the NAFs of
the halves: |k1|, |k2| would be at least sum |d_i| 2^i over the NAF of a
vector no shorter than the shortest one (about 2^126 .. 2^127), which is the
size of the halves' own bound, and the deal would have to put exactly those
digits on the two operands.  No scalar of the families does (asserted on the
model in test_accum_edges_oracle.py); termadd is covered by scalars, identity
operands (inf + inf, inf + Q) and table position 127 only.

Case holds a batch under construction: per proof the dlog of every point, the
scalars and the challenges; the VK dlogs; gadgets edit dlogs and challenges and
Case.expected() returns the dlog of every output.  A gadget never drops a case
silently: a failed draw (zero coefficient, a root of unity for x) is redrawn
from the proof's seeded stream at most 8 times, then raises.
"""
from __future__ import annotations

import os
import re

import numpy as np

import accum as A
import accum_util as U
import pasta as P
from msm_short_edge_util import Events, glv, glv_model, glv_special_scalars

ENGINE_HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halo2-aggregation_amd", "csrc",
                          "accum_engine.hpp")
OUTPUTS = ("w", "zw", "f", "e")   # MultiopenVar order (the quad's rows)
W3_WIN = 43
MAX_REDRAW = 8


# ------------------------------------------------------------------ term plan
class Plan:
    """terms: [dict(out, src, coef, queries)] in device order; ranges: {out:
    (lo, hi)}; pairs: [(t0, t1 or None)] per output range f, w, zw, e."""


def _queries(sh):
    npts, nsc = sh.points_per_proof(), sh.scalars_per_proof()
    d = A._split(sh, A.Proof(points=[None] * npts, scalars=[0] * nsc, challenges=[0] * 7))
    return A.construct_intermediate_sets(A.build_queries(sh, d, 0))


def term_plan(C, sh, challenges, scalars=None):
    """The per-proof term list in device order.  scalars (the proof's
    evaluations) are needed only for e's coefficient -eval_multi (None without)."""
    r = C.r
    x, v, u = challenges[4] % r, challenges[5] % r, challenges[6] % r
    xn = pow(x, 1 << sh.log_n, r)
    sets = _queries(sh)
    S = len(sets)
    slot_of, terms, hq = {}, [], []
    for j, (rot, qs) in enumerate(sets):
        m = len(qs)
        for i, (ref, _, _) in enumerate(qs):
            c = pow(u, S - 1 - j, r) * pow(v, m - 1 - i, r) % r
            if ref == A.H_POINT:
                hq.append((j, i, m, c))
                continue
            if ref not in slot_of:
                slot_of[ref] = len(terms)
                terms.append(dict(out="f", src=ref, coef=0, queries=[]))
            t = terms[slot_of[ref]]
            t["coef"] = (t["coef"] + c) % r
            t["queries"].append((j, i, m))
    cH = sum(c for _, _, _, c in hq) % r
    po = sh.point_offsets()
    for i in range(sh.quotient_degree):
        terms.append(dict(out="f", src=("proof", po["h"][0] + i), coef=cH * pow(xn, i, r) % r, queries=[]))
    pl = Plan()
    pl.nslots = len(terms)
    winv = pow(sh.omega, -1, r)
    for out in ("w", "zw"):
        for j, (rot, _) in enumerate(sets):
            c = pow(u, S - 1 - j, r)
            if out == "zw":
                c = c * (pow(sh.omega, rot, r) if rot >= 0 else pow(winv, -rot, r)) % r * x % r
            terms.append(dict(out=out, src=("proof", po["W"][0] + j), coef=c, queries=[]))
    ce = None
    if scalars is not None:
        pf = A.Proof(points=[None] * sh.points_per_proof(), scalars=list(scalars), challenges=list(challenges))
        d = A._split(sh, pf)
        _, _, h_eval = A.scalar_block(C, sh, d, pf.challenges)
        ev = 0
        for j, (rot, qs) in enumerate(A.construct_intermediate_sets(A.build_queries(sh, d, h_eval))):
            for i, (_, _, e_) in enumerate(qs):
                ev = (ev + pow(u, S - 1 - j, r) * pow(v, len(qs) - 1 - i, r) * e_) % r
        ce = (-ev) % r
    terms.append(dict(out="e", src=("g1", 0), coef=ce, queries=[]))
    pl.terms, pl.S, pl.T = terms, S, len(terms)
    pl.Tp = sum(1 for t in terms if t["src"][0] == "proof")
    ns = pl.nslots
    pl.ranges = {"f": (0, ns), "w": (ns, ns + S), "zw": (ns + S, ns + 2 * S), "e": (pl.T - 1, pl.T)}
    pl.pairs = []
    for out in ("f", "w", "zw", "e"):
        lo, hi = pl.ranges[out]
        pl.pairs += [(t, t + 1 if t + 1 < hi else None) for t in range(lo, hi, 2)]
    pl.npair = len(pl.pairs)
    pl.rots = [rot for rot, _ in sets]
    return pl


# --------------------------------------------------------------- digit models
def w3_digits(half, drop_carry_at=None):
    """w3_codes on the signed half (|half| < 2^127) -> 43 digits in [-4, 4],
    sum d_i 8^i = half.  drop_carry_at = i forgets the carry out of window i (a
    deliberately wrong recoding, for the sensitivity tests)."""
    mag, out, cy = abs(half), [], 0
    assert mag < 1 << 129
    for i in range(W3_WIN):
        u = ((mag >> (3 * i)) & 7) + cy
        cy = 1 if u > 4 else 0
        d = u - 8 * cy          # u = 8: digit 0, carry 1
        out.append(-d if half < 0 else d)
        if i == drop_carry_at:
            cy = 0
    return out


def naf_digits(half):
    """naf128 on the signed half (|half| < 2^128 / 3 * ... any 128-bit value
    whose NAF fits positions 0..127) -> 128 digits in {-1, 0, 1}."""
    k = abs(half)
    h = 3 * k
    d = [((h >> (i + 1)) & 1) - ((k >> (i + 1)) & 1) for i in range(128)]
    return [-x for x in d] if half < 0 else d


def deal(k1, k2, S):
    """k_acc_termadd's deal -> per lane a list of (half, position, digit)."""
    ranked = [(0, i, d) for i, d in enumerate(naf_digits(k1)) if d] + \
             [(1, i, d) for i, d in enumerate(naf_digits(k2)) if d]
    return [ranked[j::S] for j in range(S)]


# ------------------------------------------------------------- path constants
def engine_constants(path=ENGINE_HDR):
    txt = open(path).read()
    out = {}
    for nm in ("kAccLaneBudget", "kAccSumLanes"):
        m = re.search(r"constexpr size_t %s = ([0-9 *]+);" % nm, txt)
        v = 1
        for f in m.group(1).split("*"):
            v *= int(f)
        out[nm] = v
    return out


def acc_path(B, T, Tp, npair, split=-1, tpl=-1):
    """accum_plan.hpp acc_path's choices -> dict(lgS, quad_terms, tpl (0 in the split
    form), pstep, lgL)."""
    k = engine_constants()
    budget, sumlanes = k["kAccLaneBudget"], k["kAccSumLanes"]
    nterm, nprf = B * T, B * Tp
    if split >= 0:
        lgS = split
    elif 4 * (nprf << 2) > 3 * budget:
        lgS = 0
    else:
        lgS = 0
        while lgS < 3 and (nterm << (lgS + 1)) <= budget:
            lgS += 1
    if split < 0 and lgS == 3:
        while lgS < 5 and (nterm << (lgS + 1)) <= budget // 2:
            lgS += 1
    quad = split < 0 and lgS == 5 and nterm * 64 <= budget // 2
    t = 0
    if lgS == 0:
        t = tpl if tpl > 0 else (2 if nterm > budget // 2 and B * npair <= budget // 2 else 1)
    lgL = 0
    while lgL < 5 and ((B * 4) << (lgL + 1)) <= sumlanes:
        lgL += 1
    while lgL < 3 and ((B * 4) << (lgL + 1)) <= budget // 2:
        lgL += 1
    return dict(lgS=lgS, quad_terms=quad, tpl=t, pstep=2 if t == 2 else 1, lgL=lgL)


def batch_for_lgL(lgL, T, Tp, npair):
    """The smallest B at which k_acc_sum runs with 2^lgL lanes per output."""
    B = 1
    while acc_path(B, T, Tp, npair)["lgL"] > lgL:
        B *= 2
    lo = B // 2
    while lo + 1 < B:                      # first B with lgL' <= lgL
        mid = (lo + B) // 2
        if acc_path(mid, T, Tp, npair)["lgL"] > lgL:
            lo = mid
        else:
            B = mid
    assert acc_path(B, T, Tp, npair)["lgL"] == lgL, (lgL, B)
    return B


# -------------------------------------------------------- addition-order models
class AccEvents(Events):
    """Events on discrete logs; wrong_dbl / wrong_cancel model a deliberately
    broken group law (doubling returns the identity / cancellation falls
    through to the general formula, which yields a point that is NOT the
    identity: modelled as the dlog 1)."""

    def __init__(self, r, wrong_dbl=False, wrong_cancel=False):
        super().__init__()
        self.r, self.wrong_dbl, self.wrong_cancel = r, wrong_dbl, wrong_cancel
        self.cancelled = False

    def note(self, stage, kind):
        self[(stage, kind)] = self.get((stage, kind), 0) + 1

    def kinds(self, stage=""):
        return {k for (st, k) in self if st.startswith(stage)}

    def _sum(self, a, b, stage, pre):
        if a[0] == b[0]:
            self.note(stage, pre + "dbl")
            if self.wrong_dbl:
                return None
        elif (a[0] + b[0]) % self.r == 0:
            self.note(stage, pre + "cancel")
            if self.wrong_cancel:
                return (1, a[1] + b[1])
        v = (a[0] + b[0]) % self.r
        return (v, a[1] + b[1]) if v else None

    def add(self, a, b, stage):
        if a is None and b is None:
            self.note(stage, "inf+inf")
            return None
        if a is None or b is None:
            self.note(stage, "inf+Q")
            return b if a is None else a
        return self._sum(a, b, stage, "")

    def madd(self, acc, q, stage):
        """xyzz29_madd: acc None = acc_inf; q a table point's dlog (never 0)."""
        if acc is None:
            self.note(stage, "inf+Q")
            if self.cancelled:
                self.note(stage, "restart_after_cancel")
                self.cancelled = False
            return (q, 1)
        out = self._sum(acc, (q, 1), stage, "madd_")
        if out is None:
            self.cancelled = True
        return out


def _val(x):
    return x[0] if x else 0


def termmul_events(cid, terms, ev, drop_carry_at=None):
    """glv_mul_w3 (one term) / glv_mul_w3n<.., 2> (two) on terms = [(k, dlog)]
    (dlog 0: an identity point, not live) -> the lane's sum as a dlog."""
    C, lam = P.CURVES[cid], glv(cid)["lam"]
    digs = []
    for k, d in terms:
        h1, h2 = glv_model(cid, k % C.r)
        digs.append((w3_digits(h1, drop_carry_at), w3_digits(h2, drop_carry_at)))
    acc, ev.cancelled = None, False
    for i in range(W3_WIN - 1, -1, -1):
        if acc:
            acc = (acc[0] * 8 % C.r, acc[1])
        for j, (k, d) in enumerate(terms):
            if d % C.r == 0:
                continue
            for half in (0, 1):
                dg = digs[j][half][i]
                if dg:
                    acc = ev.madd(acc, dg * d * (lam if half else 1) % C.r, "termmul")
    return _val(acc)


def termadd_events(cid, k, d, lgS, ev):
    """k_acc_termadd on one term (k, dlog != 0) with 2^lgS lanes (or quads)."""
    C, lam = P.CURVES[cid], glv(cid)["lam"]
    h1, h2 = glv_model(cid, k % C.r)
    S = 1 << lgS
    acc = []
    for lane in deal(h1, h2, S):
        a = None
        for half, pos, dg in lane:
            a = ev.add(a, (dg * (1 << pos) * d * (lam if half else 1) % C.r, 1), "termadd-lane")
        acc.append(a)
    m = 1
    while m < S:
        acc = [ev.add(acc[l], acc[l ^ m], f"termadd-bfly{m}") for l in range(S)]
        m <<= 1
    return _val(acc[0])


def sum_events(vals, lgL, pstep, ev):
    """k_acc_sum on one output range: vals = the dlog of every row of the
    range (0 = identity) as the term kernel left them."""
    NL = 1 << lgL
    NV = NL >> 2 if NL >= 4 else NL
    acc = []
    for v in range(NV):
        a = None
        for t in range(v * pstep, len(vals), NV * pstep):
            a = ev.add(a, (vals[t], 1) if vals[t] else None, "sum-loop")
        acc.append(a)
    m = 1
    while m < NV:
        acc = [ev.add(acc[l], acc[l ^ m], f"sum-bfly{m}") for l in range(NV)]
        m <<= 1
    return _val(acc[0])


def rows_after_termmul(cid, plan, coefs, dlogs, tpl, ev, drop_carry_at=None):
    """The T rows of one proof as k_acc_termmul<Cv, tpl> stores them (dlogs)."""
    C = P.CURVES[cid]
    rows = [0] * plan.T
    if tpl == 1:
        for t in range(plan.T):
            rows[t] = termmul_events(cid, [(coefs[t], dlogs[t])], ev, drop_carry_at) if dlogs[t] % C.r else 0
    else:
        for t0, t1 in plan.pairs:
            tt = [(coefs[t0], dlogs[t0])] + ([(coefs[t1], dlogs[t1])] if t1 is not None else [])
            rows[t0] = termmul_events(cid, tt, ev, drop_carry_at)
    return rows


# ------------------------------------------------------------ scalar families
def _from_halves(cid, h1, h2):
    C = P.CURVES[cid]
    return (h1 + glv(cid)["lam"] * h2) % C.r


OCT_PATTERNS = (("4..4", int("4" * 41, 8)), ("5..5", int("5" * 41, 8)), ("3..34", int("3" * 40 + "4", 8)),
                ("7..7", int("7" * 41, 8)), ("4<<123", 4 << 123))
NAF_PATTERNS = (("0x5..5", int("5" * 31, 16)), ("0xA..A", int("A" * 31, 16) >> 1 << 1), ("0xF..F", int("F" * 31, 16)),
                ("0x7..7", int("7" * 31, 16)), ("2^126+2^125", (1 << 126) + (1 << 125)))


def corner_scalars(cid):
    """[(name, k)]: the lattice-cell corners (+-v1 +- v2) / 2 and their
    neighbours +-2 in each coordinate, as x + lambda y mod r."""
    g = glv(cid)
    out = []
    for s1 in (1, -1):
        for s2 in (1, -1):
            cx, cy = (s1 * g["a1"] + s2 * g["a2"]) // 2, (s1 * g["b1"] + s2 * g["b2"]) // 2
            for dx in range(-2, 3):
                for dy in range(-2, 3):
                    out.append((f"corner:{'+-'[s1 < 0]}{'+-'[s2 < 0]},{dx},{dy}", _from_halves(cid, cx + dx, cy + dy)))
    return out


_FAM = {}


def w3_pattern_scalars(cid):
    """The base-8 half patterns in the first half, in the second, and in
    both, with every sign pair; the planted halves are asserted on the model."""
    out = []
    for nm, p in OCT_PATTERNS:
        for s1, s2 in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            for h1, h2, tag in ((s1 * p, 0, "a"), (0, s2 * p, "b"), (s1 * p, s2 * p, "ab")):
                if (tag == "a" and s2 < 0) or (tag == "b" and s1 < 0):
                    continue
                k = _from_halves(cid, h1, h2)
                assert glv_model(cid, k) == (h1, h2), (cid, nm, tag, s1, s2)
                out.append((f"w3:{tag}:{'+-'[s1 < 0]}{'+-'[s2 < 0]}{nm}", k))
    return out


def scalar_family(cid):
    """[(name, canonical k)] of section 2 of the issue for curve cid."""
    if cid in _FAM:
        return _FAM[cid]
    C, lam = P.CURVES[cid], glv(cid)["lam"]
    out = [(nm, k) for nm, k, _ in glv_special_scalars(cid)]
    out.append(("two", 2))
    for i in (1, 63, 64, 126):
        out += [(f"2^{i}", 1 << i), (f"lam*2^{i}", lam * (1 << i) % C.r), (f"-2^{i}", C.r - (1 << i))]
    out += w3_pattern_scalars(cid)
    for nm, p in NAF_PATTERNS:
        out += [("naf:a:" + nm, p % C.r), ("naf:b:" + nm, lam * p % C.r), ("naf:ab:-" + nm, (lam * p - p) % C.r)]
    out += corner_scalars(cid)
    _FAM[cid] = out
    return out


# ---------------------------------------------------------------------- cases
class Case:
    """A batch under construction on curve cid and shape `shape` ("simple" /
    "rich"): per proof dict(name, dl: the dlog of every point (0 = identity),
    scalars, challenges); vkdl: {("fixed", i) / ("sigma", k): dlog}."""

    def __init__(self, cid, shape, log_n, seed):
        self.cid, self.C, self.seed, self.shape_name = cid, P.CURVES[cid], seed, shape
        C = self.C
        self.sh = U.SHAPES[shape](C, log_n)
        vs = seed ^ 0x7EC
        self.vkdl = {("fixed", i): P.synth_base_dlog(C, vs, i) for i in range(self.sh.num_fixed_columns)}
        self.vkdl.update({("sigma", k): P.synth_base_dlog(C, vs, 1000 + k) for k in range(len(self.sh.perm_columns))})
        self.proofs = []
        self._pt = {0: None}
        self._draws = {}
        self.shared = None
        self.enumerated = 0       # cases a gadget was asked for (the tests compare it with len(proofs))

    # -- construction
    def point(self, d):
        d %= self.C.r
        if d not in self._pt:
            self._pt[d] = self.C.mul(d, self.C.gen)
        return self._pt[d]

    def draw(self, b):
        """The next scalar of proof b's seeded stream (redraws)."""
        n = self._draws.get(b, 0)
        self._draws[b] = n + 1
        return P.synth_scalar(self.seed ^ 0xD4A3, b * 4096 + 100 + n, self.C.r)

    def add_proof(self, name, like=None):
        """A random shape-conformant proof (oracle synth_proof's streams);
        like = b: the points and evaluations of proof b (shared packing)."""
        C, sh = self.C, self.sh
        b = len(self.proofs)
        self.enumerated += 1
        if like is not None:
            src = self.proofs[like]
            pf = dict(name=name, dl=list(src["dl"]), scalars=list(src["scalars"]), challenges=list(src["challenges"]))
        else:
            base = b * 4096
            pf = dict(name=name, dl=[P.synth_base_dlog(C, self.seed, base + i) for i in range(sh.points_per_proof())],
                      scalars=[P.synth_scalar(self.seed ^ 0x5CA1A, base + i, C.r) for i in range(sh.scalars_per_proof())],
                      challenges=[P.synth_scalar(self.seed ^ 0xC4A1, base + i, C.r) for i in range(7)])
        self.proofs.append(pf)
        return b

    def plan(self, b, with_e=False):
        pf = self.proofs[b]
        return term_plan(self.C, self.sh, pf["challenges"], pf["scalars"] if with_e else None)

    def status(self, b):
        return A.proof_status(self.C, self.sh, self.proofs[b]["challenges"])

    def set_challenges(self, b, **kw):
        idx = dict(theta=0, beta=1, gamma=2, y=3, x=4, v=5, u=6)
        for k, val in kw.items():
            self.proofs[b]["challenges"][idx[k]] = val % self.C.r

    def src_dlog(self, b, src):
        if src[0] == "proof":
            return self.proofs[b]["dl"][src[1]]
        return 1 if src[0] == "g1" else self.vkdl[src]

    def term_dlogs(self, b, plan):
        return [self.src_dlog(b, t["src"]) for t in plan.terms]

    def expected(self, b):
        """{output: dlog} of proof b."""
        pl = self.plan(b, with_e=True)
        out = dict.fromkeys(OUTPUTS, 0)
        for t in pl.terms:
            out[t["out"]] = (out[t["out"]] + t["coef"] * self.src_dlog(b, t["src"])) % self.C.r
        return out

    def expected_quad(self, b):
        e = self.expected(b)
        return np.array([P.point_to_limbs(self.C, self.point(e[o])) for o in OUTPUTS], dtype=np.uint64)

    # -- materialisation
    def shape(self):
        self.sh.fixed_commitments = [self.point(self.vkdl[("fixed", i)]) for i in range(self.sh.num_fixed_columns)]
        self.sh.sigma_commitments = [self.point(self.vkdl[("sigma", k)]) for k in range(len(self.sh.perm_columns))]
        return self.sh

    def oracle_proof(self, b):
        pf = self.proofs[b]
        return A.Proof(points=[self.point(d) for d in pf["dl"]], scalars=list(pf["scalars"]),
                       challenges=list(pf["challenges"]))

    def pack(self):
        """-> (points (B, npts, 8), scalars (B, nsc, 4), challenges (B, 7, 4)) u64 Montgomery."""
        C, r = self.C, self.C.r
        lim = {}

        def pl(d):
            if d not in lim:
                lim[d] = P.point_to_limbs(C, self.point(d))
            return lim[d]

        pts = np.array([[pl(d % r) for d in pf["dl"]] for pf in self.proofs], dtype=np.uint64)
        scs = np.array([[P.to_limbs(s * P.R_MONT % r) for s in pf["scalars"]] for pf in self.proofs], dtype=np.uint64)
        chs = np.array([[P.to_limbs(s * P.R_MONT % r) for s in pf["challenges"]] for pf in self.proofs], dtype=np.uint64)
        return pts, scs, chs

    # -- gadgets
    def _retry(self, b, fn):
        """fn() -> True when the planting succeeded; else redraw (x, v, u) of
        proof b from its stream, at most MAX_REDRAW times."""
        for _ in range(MAX_REDRAW + 1):
            if fn() and self.status(b) == 0:
                return
            self.set_challenges(b, x=self.draw(b), v=self.draw(b), u=self.draw(b))
        raise RuntimeError(f"planting failed after {MAX_REDRAW} redraws: {self.proofs[b]['name']}")

    def plant_products(self, b, out, mults, q=None, vk=False):
        """Term t of output `out` becomes the point [mults[t - lo] q]G (0: the
        identity; None: left alone), by setting its source's dlog to
        mults q / c_t.  Only proof-point terms, unless vk: then the VK terms of f
        are planted too (mult 1), once per Case: every later vk planting
        reuses the first one's (x, v, u, q).  -> q."""
        C, r = self.C, self.C.r
        if vk and self.shared:
            x, v, u, q = self.shared
            self.set_challenges(b, x=x, v=v, u=u)
        q = q if q is not None else self.draw(b) or 1

        def go():
            pl = self.plan(b)
            lo, hi = pl.ranges[out]
            todo = []
            for t in range(lo, hi):
                m, term = mults[t - lo], pl.terms[t]
                if term["src"][0] != "proof" and not (vk and not self.shared):
                    continue
                if m is None:
                    continue
                if term["coef"] == 0:
                    return False
                todo.append((term["src"], (1 if term["src"][0] != "proof" else m) * q * pow(term["coef"], -1, r) % r))
            for src, d in todo:
                if src[0] == "proof":
                    self.proofs[b]["dl"][src[1]] = d
                else:
                    self.vkdl[src] = d
            return True

        self._retry(b, go)
        if vk and not self.shared:
            c = self.proofs[b]["challenges"]
            self.shared = (c[4], c[5], c[6], q)
        return q

    def equal_products(self, b, out, vk=False):
        lo, hi = self.plan(b).ranges[out]
        return self.plant_products(b, out, [1] * (hi - lo), vk=vk)

    def cancelling_products(self, b, out, pattern):
        """pattern "adjacent": + - + - ...; "halves": the first half +, the
        second -; "all-but-one": as adjacent with the last term 2 Q (n odd) or
        the last two + + (n even), so the sum is not the identity."""
        lo, hi = self.plan(b).ranges[out]
        n = hi - lo
        if pattern == "adjacent":
            m = [1 if i % 2 == 0 else -1 for i in range(n)]
        elif pattern == "halves":
            m = [1 if i < n // 2 else -1 for i in range(n)]
            if n & 1:
                m[-1] = 0
        else:
            m = [1 if i % 2 == 0 else -1 for i in range(n)]
            m[-1] = 2 if n & 1 else 1
        return self.plant_products(b, out, m), m

    def scalar_on_W(self, b, k):
        """u = k: W_{S-2} carries exactly k in w, beside W_{S-1} with 1."""
        self.set_challenges(b, u=k)
        pl = self.plan(b)
        lo, hi = pl.ranges["w"]
        assert pl.terms[hi - 2]["coef"] == k % self.C.r and pl.terms[hi - 1]["coef"] == 1
        if self.status(b):
            raise RuntimeError("scalar_on_W: x is a root of unity")
        return hi - 2

    def last_pair(self, b, out):
        pl = self.plan(b)
        lo, hi = pl.ranges[out]
        return [p for p in pl.pairs if lo <= p[0] < hi and p[1] is not None][-1]

    def pair_on_zw(self, b, k0, k1):
        """Solve x and u so that the last zw pair carries (k0, k1), both nonzero
        and k1 != +-1 (x would be an n-th root of unity).  -> the pair (t0, t1)."""
        C, r, sh = self.C, self.C.r, self.sh
        k0, k1 = k0 % r, k1 % r
        if k0 == 0 or k1 in (0, 1, r - 1):
            raise ValueError("pair_on_zw: not available for these scalars")
        pl = self.plan(b)
        t0, t1 = self.last_pair(b, "zw")
        lo = pl.ranges["zw"][0]
        j = t0 - lo
        e = pl.S - 2 - j                     # W_{j+1} carries u^e z_{j+1}
        wi = pow(sh.omega, -1, r)
        om = lambda rot: pow(sh.omega, rot, r) if rot >= 0 else pow(wi, -rot, r)  # noqa: E731
        u = k0 * pow(k1, -1, r) % r * om(pl.rots[j + 1]) % r * pow(om(pl.rots[j]), -1, r) % r
        x = k1 * pow(pow(u, e, r) * om(pl.rots[j + 1]) % r, -1, r) % r
        self.set_challenges(b, u=u, x=x)
        pl = self.plan(b)
        assert (pl.terms[t0]["coef"], pl.terms[t1]["coef"]) == (k0, k1)
        if self.status(b):
            raise RuntimeError("pair_on_zw: x is a root of unity")
        return t0, t1

    def zero_coefficient(self, b):
        """Choose u so that the coefficient of a commitment queried in two
        adjacent rotation sets is 0 mod r (its point stays live) -> term index."""
        r = self.C.r
        pl = self.plan(b)
        for t, term in enumerate(pl.terms):
            q = term["queries"]
            if len(q) == 2 and q[1][0] == q[0][0] + 1 and term["src"][0] == "proof":
                break
        else:
            raise RuntimeError("no commitment queried in two adjacent sets")
        (j0, i0, m0), (j1, i1, m1) = q

        def go():
            v = self.proofs[b]["challenges"][5]
            if v == 0:
                return False
            # u^(S-1-j0) v^(m0-1-i0) + u^(S-2-j0) v^(m1-1-i1) = 0
            self.set_challenges(b, u=-pow(v, m1 - 1 - i1, r) * pow(pow(v, m0 - 1 - i0, r), -1, r))
            return self.plan(b).terms[t]["coef"] == 0 and self.proofs[b]["dl"][term["src"][1]] != 0

        self._retry(b, go)
        return t

    def relate(self, b, t1, t0, rel):
        """The point of term t1 becomes rel(point of term t0): "+", "-", "2",
        "3", "4" (multiples), "phi", "-phi"."""
        pl = self.plan(b)
        lam = glv(self.cid)["lam"]
        f = {"+": 1, "-": -1, "2": 2, "3": 3, "4": 4, "phi": lam, "-phi": -lam}[rel]
        d0 = self.src_dlog(b, pl.terms[t0]["src"])
        assert pl.terms[t1]["src"][0] == "proof" and d0
        self.proofs[b]["dl"][pl.terms[t1]["src"][1]] = f * d0 % self.C.r

    def zero_e(self, b):
        """Set r(x)'s evaluation so that eval_multi = 0: e is the identity."""
        r, sh = self.C.r, self.sh
        so = sh.scalar_offsets()["rand"][0]
        pf = self.proofs[b]
        pl = self.plan(b)
        ridx = sh.point_offsets()["rand"][0]
        c = next(t["coef"] for t in pl.terms if t["src"] == ("proof", ridx))
        # rand's only query is (rotation 0, last of its set): coefficient of its evaluation = its point's
        pf["scalars"][so] = 0
        ev0 = (-self.plan(b, with_e=True).terms[-1]["coef"]) % r
        if c == 0:
            raise RuntimeError("zero_e: zero coefficient")
        pf["scalars"][so] = (-ev0) * pow(c, -1, r) % r
        assert self.plan(b, with_e=True).terms[-1]["coef"] == 0


def tile(arrs, B):
    """Repeat the distinct proofs' packed arrays up to B rows."""
    n = arrs[0].shape[0]
    reps = -(-B // n)
    return [np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:B] for a in arrs]


# ------------------------------------------------------------ the device model
def model_outputs(case, b, path, ev, drop_carry_at=None):
    """The four outputs of proof b as the device computes them on `path`
    (acc_path's dict), over discrete logs, recording every special addition in
    ev -> {output: dlog}.  With the right models this equals case.expected(b)."""
    pl = case.plan(b, with_e=True)
    r = case.C.r
    coefs = [t["coef"] for t in pl.terms]
    dl = [d % r for d in case.term_dlogs(b, pl)]
    if path["lgS"] == 0:
        rows = rows_after_termmul(case.cid, pl, coefs, dl, path["tpl"], ev, drop_carry_at)
    else:
        lg = 4 if path["quad_terms"] else path["lgS"]
        rows = [termadd_events(case.cid, coefs[t], dl[t], lg, ev) if dl[t] else 0 for t in range(pl.T)]
    return {o: sum_events(rows[pl.ranges[o][0]:pl.ranges[o][1]], path["lgL"], path["pstep"], ev) for o in OUTPUTS}


# ------------------------------------------------------------------ the cases
# Each builder returns a Case whose proofs carry "claims": the events the model
# must show for the proof on the path the builder is meant for (the CPU file
# asserts them, the GPU file runs the same cases on the device).
TERMADD_NAMES = ("const:", "lam:", "two", "2^", "lam*2^", "-2^", "naf:", "corner:")


def family_case(cid, shape, log_n, seed, names=None):
    """One proof per scalar of scalar_family (names: only those whose name
    starts with one of the prefixes), all on the points and evaluations of
    proof 0, with u = the scalar (scalar_on_W)."""
    c = Case(cid, shape, log_n, seed)
    c.add_proof("random")
    c.proofs[0]["claims"] = set()
    for nm, k in scalar_family(cid):
        if names and not nm.startswith(tuple(names)):
            continue
        b = c.add_proof(nm, like=0)
        c.scalar_on_W(b, k)
        c.proofs[b]["claims"] = set()
        c.proofs[b]["k"] = k
    # a VK term and a proof term holding the same point (the per-VK table and
    # the proof's own ladder chain must agree on it)
    b = c.add_proof("vk twin", like=0)
    c.proofs[b]["claims"] = set()
    c.proofs[b]["dl"][c.sh.point_offsets()["adv"][0]] = c.vkdl[("fixed", 0)]
    return c


def pattern_pairs_case(cid, shape, log_n, seed):
    """pair_on_zw over consecutive base-8 pattern scalars: both rows of the
    last zw pair carry a pattern (one- and two-term lanes)."""
    c = Case(cid, shape, log_n, seed)
    c.add_proof("random")
    c.proofs[0]["claims"] = set()
    pats = w3_pattern_scalars(cid)
    for (n0, k0), (n1, k1) in zip(pats, pats[1:] + pats[:1]):
        b = c.add_proof(f"zw:{n0}|{n1}", like=0)
        c.pair_on_zw(b, k0, k1)
        c.proofs[b]["claims"] = set()
    return c


MID_CHAIN = [(i, m) for i in (1, 20, 42) for m in (1, 2, 3, 4)]


def two_term_case(cid, shape, log_n, seed):
    """The collisions of the two-term lanes (k_acc_termmul<Cv, 2>), through
    the last w pair (u = 1) and the last zw pair (pair_on_zw)."""
    c = Case(cid, shape, log_n, seed)
    C, lam = c.C, glv(cid)["lam"]

    def new(name, claims):
        b = c.add_proof(name)
        c.proofs[b]["claims"] = set(claims)
        return b

    for rel, claim in (("+", "madd_dbl"), ("-", "madd_cancel")):
        b = new(f"w:(1,1),P1={rel}P0", [claim])
        c.set_challenges(b, u=1)
        t0, t1 = c.last_pair(b, "w")
        c.relate(b, t1, t0, rel)
    for i, m in MID_CHAIN:
        b = new(f"zw:mid-chain,i={i},m={m}", ["madd_cancel", "restart_after_cancel"])
        t0, t1 = c.pair_on_zw(b, (8 ** i) * m + 3, -(8 ** i) * m + 2)
        c.relate(b, t1, t0, "+")
    for m in (2, 3, 4):
        for i in (1, 7):
            for sgn, claim in ((1, "madd_dbl"), (-1, "madd_cancel")):
                b = new(f"zw:[{m}]P0,i={i},{'+-'[sgn < 0]}", [claim])
                t0, t1 = c.pair_on_zw(b, (8 ** i) * m + 3, sgn * (8 ** i) + 2)
                c.relate(b, t1, t0, str(m))
    for rel, claim in (("phi", "madd_dbl"), ("-phi", "madd_cancel")):
        for i in (1, 7):
            b = new(f"zw:{rel}(P0),i={i}", [claim])
            t0, t1 = c.pair_on_zw(b, lam * (8 ** i) + 3, (8 ** i) + 2)
            c.relate(b, t1, t0, rel)
    for which in (0, 1):
        b = new(f"zw:identity P{which}", ["inf+Q"])
        pl = c.plan(b)
        t = c.last_pair(b, "zw")[which]
        c.proofs[b]["dl"][pl.terms[t]["src"][1]] = 0
    b = new("zero coefficient on a live point", [])
    c.zero_coefficient(b)
    b = new("random", [])
    return c


def sum_case(cid, shape, log_n, seed):
    """The collisions of k_acc_sum: equal and cancelling products on every
    output, an identity output, e with eval_multi = 0."""
    c = Case(cid, shape, log_n, seed)

    def new(name, claims):
        b = c.add_proof(name)
        c.proofs[b]["claims"] = set(claims)
        return b

    for vk in (True, False):   # the VK planting first: it fixes the shared (x, v, u)
        # (proof terms only: the random VK terms in between keep some lane
        # layouts free of collisions, so that proof claims nothing)
        b = new(f"equal:f{',vk' if vk else ''}", ["dbl"] if vk else [])
        c.equal_products(b, "f", vk=vk)
    for out in ("w", "zw"):
        b = new(f"equal:{out}", ["dbl"])
        c.equal_products(b, out)
    for i in (1, 64):
        b = new(f"w:W_last=[2^{i}]W_prev", ["dbl"])
        c.set_challenges(b, u=1 << i)
        pl = c.plan(b)
        lo, hi = pl.ranges["w"]
        for t in range(lo, hi - 2):
            c.proofs[b]["dl"][pl.terms[t]["src"][1]] = 0
        d = c.src_dlog(b, pl.terms[hi - 2]["src"])
        c.proofs[b]["dl"][pl.terms[hi - 1]["src"][1]] = d * (1 << i) % c.C.r
    for out in ("w", "zw", "f"):
        for pat in ("adjacent", "halves", "all-but-one"):
            # (f: proof terms only, so as for equal:f nothing is claimed)
            b = new(f"cancel:{out},{pat}", ["cancel"] if out != "f" else [])
            c.cancelling_products(b, out, pat)
    b = new("e:ev=0", [])
    c.zero_e(b)
    b = new("random", [])
    return c

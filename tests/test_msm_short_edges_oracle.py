"""CPU tests that pin the short-path edge-input generator
(tests/msm_short_edge_util.py) and the MSM references to each other before the
GPU sees these inputs:

* the C port of best_multiexp == expected_by_dlog == the Python restatement on
  the mixed case of every path (n = 32 fused, 300 quads, 2048 lanes, one
  many-MSM batch per window width 8 .. 4), on the GLV collision cases and on
  the whole-array cases, all three curves;
* the GLV model reproduces k = k1 + lambda k2 mod r and the planted halves; the
  recoded digits contain what the pattern names claim; the 33rd window of the
  small path and the 52nd of the many path at c = 5 are zero for every input;
* the many-MSM digit patterns contain what they claim, and for c = 7, 6, 5 every
  straddle scalar has planted windows that really cross a 32-bit word boundary;
* sensitivity: with one planted row's contribution changed, or one carry
  dropped in small_digits / many_digits, each comparison fails;
* the geometry the GPU tests rely on (kernel thresholds, slices, kq, the
  many_pick_c thresholds recomputed from many_bytes_per_base) restates the
  sources.
"""
import math
import random

import numpy as np
import pytest

import msm_edge_util as E
import msm_ref
import msm_short_edge_util as U
import pasta as P
import plan_native as N

SMALL_N = (("fused", 32), ("quads", 300), ("lanes", 2048))
MANY_PREFIX = U.MANY_PREFIX
_CACHE = {}


def _mixed(curve, n, path, c=None, rot=0):
    key = (curve, n, path, c, rot)
    if key not in _CACHE:
        S, B, D, planted = U.short_mixed_case(curve, n, path, c, rot=rot)
        for a in (S, B, D):
            a.setflags(write=False)
        _CACHE[key] = (S, B, D, planted)
    return _CACHE[key]


def _c_point(curve, S, B, **kw):
    return P.limbs_to_point(P.CURVES[curve], [int(x) for x in msm_ref.best_multiexp(curve, S, B, **kw)])


def _py_inputs(curve, S, B):
    C = P.CURVES[curve]
    rinv = pow(P.R_MONT, -1, C.r)
    return [int(s) * rinv % C.r for s in E.to_ints(S)], [P.limbs_to_point(C, [int(x) for x in row]) for row in B]


def _total(curve, S, D):
    """sum s_i d_i mod r (Montgomery factors left in): expected_by_dlog is
    [this / R^2] G and G has order r, so two inputs give the same point exactly
    when their totals agree."""
    return int(np.dot(E.to_ints(S), E.to_ints(D))) % P.CURVES[curve].r


def _perturbed_total(curve, S, D, row):
    """_total with row `row`'s contribution changed: its term removed, or (a
    zero scalar / identity base) made non-zero."""
    s, d = int(E.to_ints(S[row:row + 1])[0]), int(E.to_ints(D[row:row + 1])[0])
    t = _total(curve, S, D)
    r = P.CURVES[curve].r
    if s and d:
        return (t - s * d) % r
    return (t + (s or 1) * (d or 1)) % r


def _check_planted(curve, S, B, D, planted):
    """The planted rows are what they claim, and each one's contribution is
    visible in the answer."""
    C, g = P.CURVES[curve], U.glv(curve)
    sc, pts = _py_inputs(curve, S, B)
    assert all(C.on_curve(p) for p in pts)
    phi = lambda p, k=1: (pow(g["beta"], k, C.p) * p[0] % C.p, p[1])  # noqa: E731
    tot = _total(curve, S, D)
    for kind, rws, name in planted:
        a = rws[0]
        if kind in ("dup", "quad", "run"):
            assert all(np.array_equal(S[r], S[a]) and np.array_equal(B[r], B[a]) for r in rws), kind
        elif kind == "neg":
            assert pts[rws[1]] == C.neg(pts[a]) and sc[rws[1]] == sc[a]
        elif kind == "identity":
            assert pts[a] is None and sc[a] != 0 or name == "const:zero"
            assert sc[rws[1]] == 0
        elif kind in ("phi", "phi-neg", "phi2"):
            want = phi(pts[a], 2 if kind == "phi2" else 1)
            assert pts[rws[1]] == (C.neg(want) if kind == "phi-neg" else want) and sc[rws[1]] == sc[a]
            if kind != "phi2":   # the GLV collision: (P, second half) and (phi(P), first half) have equal digits
                k1, k2 = U.glv_model(curve, sc[a])
                assert k1 == k2 != 0 and U.small_digits(k1) == U.small_digits(k2)
        elif kind == "pow":
            assert sc[rws[1]] == sc[a]
        # the dlog column follows the base
        for r in rws:
            d = int(E.to_ints(D[r:r + 1])[0]) * pow(P.R_MONT, -1, C.r) % C.r
            if kind in ("phi", "phi-neg", "phi2", "pow", "neg") and r != a:
                assert C.mul(d, C.gen) == pts[r], (kind, r)
        # sensitivity (P, -P cancel: removing ONE of them must show)
        rows_to_try = rws[:1] if kind in ("neg", "run", "quad") else rws
        for r in rows_to_try:
            assert _perturbed_total(curve, S, D, r) != tot, (kind, r, name)
    return sc, pts


# ------------------------------------------------------------- references agree
@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("path,n", SMALL_N)
def test_references_agree_small_paths(curve, path, n):
    C = P.CURVES[curve]
    names = {nm for nm, _, _ in U.glv_special_scalars(curve)}
    seen = set()
    for rot in U.covering_rots(curve, n, path):
        S, B, D, planted = _mixed(curve, n, path, rot=rot)
        assert U.small_geom(n)[0] == path
        assert {k for k, _, _ in planted} >= set(U.SMALL_GADGETS)
        assert path == "fused" or "run" in {k for k, _, _ in planted}
        seen |= {nm for _, _, nm in planted}
        want = E.expected_by_dlog(curve, S, D)
        assert _c_point(curve, S, B) == want
        Sc = E.canonical(curve, S)
        assert _c_point(curve, Sc, B, canonical=True) == want
        if rot == 0:
            sc, pts = _check_planted(curve, S, B, D, planted)
            assert C.best_multiexp(sc, pts) == want
            if n <= 300:
                assert C.msm_naive(sc, pts) == want
    assert seen == names   # between them the cases hold every special scalar


def test_gadget_distances():
    """Where the pairs sit: the fused kernel's first tree level, one quad's or
    lane's stride; pairs inside one slice and pairs across a slice cut."""
    assert [U.gadget_distance(n, "fused") for n in (1, 2, 16, 17, 32)] == [1, 1, 8, 16, 16]
    for path, n in SMALL_N[1:]:
        _, kq, ns = U.small_geom(n)
        per = kq * (128 if path == "lanes" else 32)      # rows per slice
        dist = U.gadget_distance(n, path)
        pairs = [rws for k, rws, _ in _mixed(0, n, path)[3] if k in ("dup", "neg", "phi", "phi-neg")]
        same = [p for p in pairs if p[0] // per == p[1] // per]
        assert all(p[1] - p[0] in (dist, dist // 2) for p in pairs)   # every second round at half the distance
        assert kq > 1 and same and len(same) < len(pairs), (path, len(same), len(pairs))
    for n in (2, 16, 17, 32):   # some gadget sits at the first tree level in every fused size
        d = U.gadget_distance(n, "fused")
        kinds = set()
        for rot in range(8):
            kinds |= {k for k, rws, _ in U.short_mixed_case(0, n, "fused", rot=rot)[3] if len(rws) > 1 and rws[1] - rws[0] in (d, d // 2)}
        assert kinds >= {"dup", "neg", "identity", "phi", "phi-neg", "phi2"}, (n, kinds)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_references_agree_collision_and_whole_array(curve):
    C = P.CURVES[curve]
    for n in (2, 33, 300):
        for pat in ("7..78", "7..7", "8..8"):
            S, B, D = U.glv_collision_case(curve, n, pat)
            want = E.expected_by_dlog(curve, S, D)
            assert want is not None and _c_point(curve, S, B) == want
            sc, pts = _py_inputs(curve, S, B)
            if n <= 33:
                assert C.msm_naive(sc, pts) == want
            # the two halves' sums agree window by window: rows (P, lam b), (phi(P), b)
            h0, h1 = U.glv_model(curve, sc[0]), U.glv_model(curve, sc[1])
            assert h0[0] == 0 and h1[1] == 0 and h0[1] == h1[0] and U.small_digits(h0[1]) == U.small_digits(h1[0])
            assert _perturbed_total(curve, S, D, 0) != _total(curve, S, D)
            S, B, D = U.glv_collision_case(curve, n, pat, negate=True)
            assert E.expected_by_dlog(curve, S, D) is None and not msm_ref.best_multiexp(curve, S, B).any()
            assert _perturbed_total(curve, S, D, 1) != 0 == _total(curve, S, D)
    _, B, D, _ = _mixed(curve, 300, "quads")
    for name in ("const:r-1", "glv:+8..8,+8..8", "glv:-7..78,+7..78"):
        S = U.whole_array_case(curve, 300, name)
        assert _c_point(curve, S, B) == E.expected_by_dlog(curve, S, D), name
        assert _perturbed_total(curve, S, D, 150) != _total(curve, S, D)
    one = np.repeat(B[:1], 300, axis=0), np.repeat(D[:1], 300, axis=0)    # every base equal
    S = _mixed(curve, 300, "quads")[0]
    assert _c_point(curve, S, one[0]) == E.expected_by_dlog(curve, S, one[1])


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("nb,c", MANY_PREFIX)
def test_references_agree_many_batch(curve, nb, c):
    """One batch per window width: every MSM of it is a mixed case of its own
    (disjoint base windows)."""
    C = P.CURVES[curve]
    ns, offs = U.many_batch(nb, c, False)
    names = {nm for nm, _ in U.many_special_scalars(curve, c)}
    seen, kinds = set(), set()
    for i, n in enumerate(ns):
        S, B, D, planted = _mixed(curve, n, "many", c, rot=i)
        seen |= {nm for _, _, nm in planted}
        kinds |= {k for k, _, _ in planted}
        # every row is a gadget's: gadget rows on both sides of every quad boundary
        assert sorted(r for _, rws, _ in planted for r in rws) == list(range(n))
        want = E.expected_by_dlog(curve, S, D)
        assert _c_point(curve, S, B) == want
        assert _c_point(curve, E.canonical(curve, S), B, canonical=True) == want
        if n <= 100:
            sc, pts = _check_planted(curve, S, B, D, planted)
            assert C.best_multiexp(sc, pts) == want and C.msm_naive(sc, pts) == want
    assert seen >= names
    W = U.many_geom(c)[0]
    assert kinds >= set(U.MANY_GADGETS) | ({"pow"} if W & (W - 1) else set())


# ----------------------------------------------------------------- GLV model
@pytest.mark.parametrize("curve", [0, 1, 2])
def test_glv_model_and_small_digits(curve):
    C, g = P.CURVES[curve], U.glv(curve)
    sp = U.glv_special_scalars(curve)
    pat = dict(U.HALF_PATTERNS)
    names = [nm for nm, _, _ in sp]
    # every pair of patterns and signs is there (a zero half has one sign)
    assert len([nm for nm in names if nm.startswith("glv:")]) == 13 * 13
    for fam in ("const:", "lam:", "round:"):
        assert any(nm.startswith(fam) for nm in names)
    top = 0
    for name, k, (k1, k2) in sp:
        assert 0 <= k < C.r and (k1 + g["lam"] * k2 - k) % C.r == 0 and U.glv_model(curve, k) == (k1, k2)
        if name.startswith("glv:"):   # the halves are the planted ones
            a, b = name[4:].split(",")
            assert k1 == (-1 if a[0] == "-" else 1) * pat[a[1:]] and k2 == (-1 if b[0] == "-" else 1) * pat[b[1:]]
        for h in (k1, k2):
            d = U.small_digits(h)
            assert U.small_from_digits(d) == h and len(d) == U.SMALL_WIN and all(-8 <= x <= 8 for x in d)
            assert d[32] == 0
            top = max(top, abs(h) >> 124)
            # sensitivity: a carry dropped in the recoding no longer restates the half
            m = abs(h)
            for w in range(32):
                carried = sum(x << (4 * i) for i, x in enumerate(U.small_digits(m)[:w + 1])) != m & ((1 << (4 * w + 4)) - 1)
                if carried:
                    assert U.small_from_digits(U.small_digits(h, drop_carry_at=w)) != h, (name, w)
    assert top <= U.TOP_NIBBLE_MAX[curve]
    # the patterns hold what they claim (a negative half flips every digit)
    for sgn in (1, -1):
        assert U.small_digits(sgn * pat["7..78"]) == [-8 * sgn] * 31 + [sgn, 0]        # every digit -8, carry to the top
        assert U.small_digits(sgn * pat["8..8"]) == [-8 * sgn] + [-7 * sgn] * 30 + [sgn, 0]
        assert U.small_digits(sgn * pat["F..F"]) == [-sgn] + [0] * 30 + [sgn, 0]        # digits 0 with a carry chain
        assert U.small_digits(sgn * pat["7..7"]) == [7 * sgn] * 31 + [0, 0]             # largest carry-free digit
        assert U.small_digits(sgn * pat["8<<120"]) == [0] * 30 + [-8 * sgn, sgn, 0]
    assert U.small_digits(0) == [0] * 33 and U.small_digits(-1) == [-1] + [0] * 32
    # without the lowest nibble's 8 nothing ripples
    assert U.small_digits(pat["7..78"] - 1) == [7] * 31 + [0, 0]
    # every digit magnitude 0 .. 8 occurs, 8 with both signs
    ds = {x for _, _, m in sp for h in m for x in U.small_digits(h)}
    assert ds >= set(range(-8, 9))
    # the rounding boundaries: c_i steps between the two neighbours
    for i in (1, 2):
        for t in U.ROUND_T:
            k0 = ((2 * t + 1) << 383) // g[f"g{i}"]
            q = [(k * g[f"g{i}"] + (1 << 383)) >> 384 for k in (k0, k0 + 1)]
            assert q == [t, t + 1], (i, t, q)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_carry_windows_are_never_reached(curve):
    """The 33rd window of small_recode is zero for every scalar: the halves are
    bounded by half the basis sum (+ rounding), so their top nibble is at most
    6 (Pallas, Vesta) / 3 (BN254) and with a carry stays below 8.  Likewise
    window 51 of the many path at c = 5 (many_windows(5) = 52 because 5 divides
    255): window 50 holds bits 250 .. 254, at most 16 = H for a scalar < r, and
    exactly 16 only when bits 125 .. 249 are zero and no carry arrives."""
    C, g = P.CURVES[curve], U.glv(curve)
    bound = max(abs(g["a1"]) + abs(g["a2"]), abs(g["b1"]) + abs(g["b2"])) // 2 + 2
    assert bound >> 124 <= U.TOP_NIBBLE_MAX[curve] < 7
    rng = random.Random(0x33 + curve)
    ks = [k for _, k, _ in U.glv_special_scalars(curve)] + [rng.randrange(C.r) for _ in range(4000)]
    ks += [s for c in (8, 7, 6, 5, 4) for _, s in U.many_special_scalars(curve, c)]
    ks += [C.r - 1 - rng.randrange(1 << 120) for _ in range(200)] + [(1 << 254) - 1 - rng.randrange(1 << 20) for _ in range(50)
                                                                      if (1 << 254) < C.r]
    for k in ks:
        for h in U.glv_model(curve, k):
            assert abs(h) <= bound and U.small_digits(h)[32] == 0
        d, cy = U.many_digits(k, 5)
        assert d[51] == 0 and cy[50] == 0, hex(k)
    assert C.r >> 250 <= 16


# ------------------------------------------------------------ many-MSM digits
@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("c", [8, 7, 6, 5, 4])
def test_many_digit_patterns_hold_what_they_claim(curve, c):
    C = P.CURVES[curve]
    W, H = U.many_geom(c)
    assert (W, H) == {8: (32, 128), 7: (37, 64), 6: (43, 32), 5: (52, 16), 4: (64, 8)}[c]
    assert W * c >= 255 + (255 % c == 0)
    sp = dict(U.many_special_scalars(curve, c))
    for name, s in sp.items():
        d, cy = U.many_digits(s, c)
        assert 0 <= s < C.r and U.many_from_digits(d, c) == s, name
        assert cy[-1] == 0 and d[-1] >= 0 and all(-H < x <= H for x in d), name
        for w in range(W):   # sensitivity: a dropped carry no longer restates the scalar
            if cy[w]:
                assert U.many_from_digits(U.many_digits(s, c, drop_carry_at=w)[0], c) != s, (name, w)
    raw = lambda s, w: (s >> (w * c)) & ((1 << c) - 1)  # noqa: E731
    # windows the < r reduction left alone
    full = [w for w in range(W) if w * c + c <= C.scalar_bits - 2]
    assert len(full) >= W - 2
    d, cy = U.many_digits(sp["pattern:half"], c)
    assert all(d[w] == H and cy[w] == 0 for w in full)            # the largest digit, no carry
    d, cy = U.many_digits(sp["pattern:half-1"], c)
    assert all(d[w] == H - 1 and cy[w] == 0 for w in full)
    d, cy = U.many_digits(sp["pattern:half+1"], c)
    assert d[0] == -(H - 1) and all(d[w] == -(H - 2) and cy[w] == 1 for w in full[1:])
    d, cy = U.many_digits(sp["pattern:ones"], c)
    assert d[0] == -1 and all(d[w] == 0 and cy[w] == 1 for w in full[1:])   # the carry ripples through every window
    assert max(d[full[-1] + 1:]) > 0                                        # and lands near the top
    d, cy = U.many_digits(sp["pattern:alt"], c)
    assert d[0] == H and cy[0] == 0 and all(d[w] < 0 and cy[w] == 1 for w in full[1:])
    # differs from WinGeom exactly where the issue says
    assert (E.win_geom(c)[0] == W and set(E.win_geom(c)[1]) == {c}) == (c in (8, 4))
    st = U.straddle_windows(c)
    assert bool(st) == (c in (7, 6, 5))
    for w in st:
        assert (w * c) // 32 + 1 == (w * c + c - 1) // 32      # lo word and the next one
    # every word cut that is no window cut has its window
    assert st == [b // c for b in range(32, 256, 32) if b % c and b // c * c + c <= 256]
    for k in U.MANY_KINDS if st else ():
        s = sp["straddle:" + k]
        kept = [w for w in st if w in full]
        assert len(kept) >= len(st) - 1 and kept
        for w in kept:
            want = E._digit_value(k if k != "alt" else ("half", "half+1")[w & 1], c)
            assert raw(s, w) == want, (k, w)
        # the fill is random elsewhere: not the whole-scalar pattern
        assert s != sp["pattern:" + k]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return N.build(tmp_path_factory)


def test_many_batches_and_thresholds(plan_exe):
    """The geometry the GPU tests rely on, asked of the product's plan code
    (tests/native/plan_dump.cpp over csrc/msm_plan.hpp)."""
    budget, cap = U.many_budget()
    assert (budget, cap) == (2 << 30, 8 << 30)
    k = N.ask1(plan_exe, "consts")
    assert (k["kManyTabBudget"], k["kManyTabCap"]) == (budget, cap)
    for c, g in zip(range(1, 21), N.ask(plan_exe, ("manyc %d" % c for c in range(1, 21)))):
        # a carry window only when c divides 255; 128-B entries, 2^(c-1) per window
        assert g["W"] == (255 // c + 1 if 255 % c == 0 else (255 + c - 1) // c) == U.many_windows(c)
        assert g["bytes_per_base"] == g["W"] << (c - 1) << 7 == U.many_bytes_per_base(c)
    # many_pick_c: the widest window whose table fits the budget
    for c in (8, 7, 6, 5):
        top = budget // U.many_bytes_per_base(c)
        assert U.many_pick_c(top) == c and U.many_pick_c(top + 1) == c - 1
    assert [budget // U.many_bytes_per_base(c) for c in (8, 7, 6, 5)] == [4096, 7084, 12192, 20164]
    assert [U.many_pick_c(n) for n, _ in MANY_PREFIX] == [c for _, c in MANY_PREFIX]
    assert [U.many_pick_c(n) for n in (6000, 8192, 16384, 32768)] == [7, 6, 5, 4]
    tops = [t + d for t in (4096, 7084, 12192, 20164) for d in (0, 1)]
    assert [g["c"] for g in N.ask(plan_exe, ("many %d" % n for n in tops))] == [8, 7, 7, 6, 6, 5, 5, 4]
    assert [g["c"] for g in N.ask(plan_exe, ("many %d" % n for n, _ in MANY_PREFIX))] == [c for _, c in MANY_PREFIX]
    assert cap // U.many_bytes_per_base(4) == 131072      # one base more: no table, the fallback
    assert (k["kManyQuads"], k["kManyQuadBudget"]) == (U.MANY_QUADS, U.MANY_QUAD_BUDGET)
    for nb, c in MANY_PREFIX:
        W = U.many_geom(c)[0]
        for big in (False, True):
            ns, offs = U.many_batch(nb, c, big)
            kq = U.many_kq(ns, c)
            assert N.ask1(plan_exe, "manykq %d" % (sum(ns) * W))["kq"] == kq
            assert min(ns) == 1 and 500 <= max(ns) <= 600 or not big
            assert offs[-1] + ns[-1] == nb                       # the last base of the prefix
            iv = sorted(zip(offs, ns))
            assert all(a + n <= b for (a, n), (b, _) in zip(iv[:-1], iv[1:]))   # disjoint windows
            if big:   # quads start mid-scalar and recompute the carry from window 0
                assert kq > 1 and W % kq != 0 and kq < W
                st = U.many_quad_starts(ns, c)
                g = math.gcd(kq, W)   # the starts drift through the scalar from row to row
                assert g < kq and {w for _, _, w in st} == set(range(g, W, g))
            else:
                assert kq == 1 and sum(ns) * W <= U.MANY_QUAD_BUDGET


def test_small_path_geometry(plan_exe):
    k = N.ask1(plan_exe, "consts")
    assert k["kSmallWin"] == U.SMALL_WIN
    assert k["kSmallFusedN"] == U.SMALL_FUSED_N
    assert k["kSmallQuads"] == U.SMALL_QUADS
    assert k["kSmallSlices"] == U.SMALL_SLICES
    assert k["kSmallLanesT"] == U.SMALL_LANES_T   # lanes = T >= 4096
    lanes_from = U.SMALL_LANES_T // 2            # the first n whose 2 n terms run k_small_sum_lanes
    assert [g["path"] for g in N.ask(plan_exe, ("small %d" % n for n in (lanes_from - 1, lanes_from)))] == \
        ["quads", "lanes"]
    want = {1: ("fused", 1, 1), 2: ("fused", 1, 1), 16: ("fused", 1, 1), 17: ("fused", 1, 1), 32: ("fused", 1, 1),
            33: ("quads", 1, 2), 300: ("quads", 2, 5), 2047: ("quads", 8, 8), 2048: ("lanes", 2, 8),
            4097: ("lanes", 5, 7)}
    for (n, g), d in zip(want.items(), N.ask(plan_exe, ("small %d" % n for n in want))):
        assert U.small_geom(n) == g, n
        assert (d["path"], d["kq"], d["ns"]) == g, n


# ---------------------------------------- the planted collisions are reached
def _canon_total(curve, S, D):
    r = P.CURVES[curve].r
    return _total(curve, S, D) * pow(P.R_MONT, -2, r) % r


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_small_path_collisions_reach_the_branches(curve):
    """The kernels' order of additions restated on discrete logs (small_events):
    its total restates the MSM (so the GLV split, the recoding and the term /
    slice / tree indexing of the model are the kernels'), and the planted pairs
    meet as equal operands (the P == Q branch of the addition) and as opposite
    ones (cancellation) where the generator says: as raw terms at the fused
    kernel's first tree level and as equal two-term sums one level up; inside
    one quad's or lane's serial accumulation, at the lanes' 256 -> 128 fold and
    in the tree on the table paths; the GLV collision at the last tree level of
    every window and slice, as whole sums."""
    for n in (2, 16, 17, 32):
        first = "tree%d" % (U.pow2(2 * n) // 2)
        ev = U.Events()
        for rot in U.covering_rots(curve, n, "fused"):
            S, _, D, _ = U.short_mixed_case(curve, n, "fused", rot=rot)
            e, total = U.small_events(curve, S, D)
            assert total == _canon_total(curve, S, D)
            for k, v in e.items():
                ev[k] = ev.get(k, 0) + v
        assert ev.get((first, "double"), 0) >= 31 and ev.get((first, "cancel"), 0) >= 31, (n, dict(ev))
        if n in (16, 32):   # the four equal rows: equal two-term sums at the second level
            assert ev.get(("tree%d" % (U.pow2(2 * n) // 4), "double+multi"), 0) >= 1
        assert ev.count("double", "serial") == 0     # one term per quad
    want = {33: ["tree32"], 300: ["serial", "tree32"], 2047: ["serial"], 2048: ["serial", "lanes128"]}
    for path, n in (("quads", 33), ("quads", 300), ("quads", 2047), ("lanes", 2048)):
        ev = U.Events()
        for rot in U.covering_rots(curve, n, path):
            S, _, D, _ = _mixed(curve, n, path, rot=rot) if rot == 0 else U.short_mixed_case(curve, n, path, rot=rot)
            e, total = U.small_events(curve, S, D)
            assert total == _canon_total(curve, S, D)
            for k, v in e.items():
                ev[k] = ev.get(k, 0) + v
        for stage in want[n]:
            assert ev.get((stage, "double"), 0) >= 1 and ev.get((stage, "cancel"), 0) >= 1, (n, stage, dict(ev))
        # equal multi-term sums (the runs, the four equal rows): ZZ != 1 whatever the table holds
        assert ev.count("double+multi", "tree") >= 1 or n == 33, (n, dict(ev))
    for n in (2, 32, 300, 2048 if curve == 0 else 33):
        for pat in ("7..78", "8..8"):
            nz = sum(1 for d in U.small_digits(dict(U.HALF_PATTERNS)[pat]) if d)
            path, kq, _ = U.small_geom(n)
            # slices that hold a pair (an odd last row has a zero scalar)
            slices = -(-(n // 2 * 2) // (kq * (128 if path == "lanes" else 32)))
            for negate, kind in ((False, "double"), (True, "cancel")):
                S, _, D = U.glv_collision_case(curve, n, pat, negate)
                e, total = U.small_events(curve, S, D)
                assert total == _canon_total(curve, S, D)
                # nothing else collides, and the last addition of every slice's tree does, in every non-zero window
                assert set(e) <= {("tree1", kind), ("tree1", kind + "+multi"), ("fold1", kind), ("fold1", kind + "+multi")}, dict(e)
                assert e[("tree1", kind)] == nz * slices, (n, pat, dict(e))
                assert n == 2 or e[("tree1", kind + "+multi")] == nz * slices


@pytest.mark.parametrize("curve", [0, 2])
@pytest.mark.parametrize("nb,c", MANY_PREFIX)
def test_many_path_collisions_reach_the_branches(curve, nb, c):
    """many_events restates k_many_sum's additions: its totals are the MSMs
    (digits, quad starts and slices as in the kernel, for kq = 1 and for a kq
    that does not divide W), and the call with kq = 1 meets equal operands: 32
    terms apart in the tree (neighbouring equal rows at c = 8, the pow gadget
    at c = 7, 6, 5), in the slice fold at c = 4 (one row per slice)."""
    for big in (False, True):
        ns, _ = U.many_batch(nb, c, big)
        cases = [_mixed(curve, n, "many", c, rot=i) if not big else U.short_mixed_case(curve, n, "many", c, rot=i, seed=17 + i)
                 for i, n in enumerate(ns)]
        ev, totals = U.many_events(curve, c, ns, np.concatenate([x[0] for x in cases]), [x[2] for x in cases])
        assert totals == [_canon_total(curve, x[0], x[2]) for x in cases]
        if not big:
            if c == 4:
                for st in ("fold-serial", "fold32"):
                    assert ev.get((st, "double+multi"), 0) >= 1, dict(ev)
                assert ev.get(("fold32", "cancel+multi"), 0) >= 1
            else:
                assert ev.get(("tree32", "double"), 0) >= 30, dict(ev)
                assert c != 8 or ev.get(("tree32", "cancel"), 0) >= 30
        else:
            assert ev.count("double") >= 1
    # the model is sensitive: one carry dropped in one scalar's digits changes that MSM's total
    S = cases[-2][0]
    s = U._canon(curve, S)[0]
    cy = U.many_digits(s, c)[1]
    if any(cy):
        assert U.many_from_digits(U.many_digits(s, c, drop_carry_at=cy.index(1))[0], c) != s

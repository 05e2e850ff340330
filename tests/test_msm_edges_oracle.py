"""CPU tests that pin the edge-input generator (tests/msm_edge_util.py) and the
two MSM references to each other before the GPU sees these inputs:

* n = 257 and 4096, all three curves: the C port of best_multiexp ==
  expected_by_dlog == the Python restatement (== msm_naive at 257) on the mixed
  input (every special scalar, base transform and collision group planted) and
  on every whole-array family;
* n = 2^18 + 11 (Pallas, BN254): the C port == expected_by_dlog on the mixed
  and the all-ones input;
* the digit patterns contain what they claim (signed digits recomputed with the
  WinGeom formulas), for every width the GPU paths use;
* sensitivity: with one planted row's contribution changed, or one carry
  dropped in the digit recomputation, each comparison fails -- no family is
  vacuous.
"""
import numpy as np
import pytest

import msm_edge_util as E
import msm_ref
import pasta as P
import plan_native as N

# (c, rows) of the GPU paths; a fixed table keeps one row per window
WIDTHS = ((16, 8), (16, 4), (16, 2), (16, 16), (20, 13), (16, 1), (20, 1), (13, 1), (12, 1))
_CACHE = {}


def _mixed(curve, n, c=16, rows=8, table=True):
    key = (curve, n, c, rows, table)
    if key not in _CACHE:
        S, B, D, planted = E.mixed_case(curve, n, c, rows, table)
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


def _perturbed(curve, S, D, row):
    """Inputs of expected_by_dlog with row `row`'s contribution changed: its
    term removed, or (a term that is zero: a zero scalar or an identity base)
    made non-zero."""
    S2, D2 = S.copy(), D.copy()
    if S2[row].any() and D2[row].any():
        S2[row] = 0
    else:
        if not S2[row].any():
            S2[row, 0] = 1
        if not D2[row].any():
            D2[row, 0] = 1
    return S2, D2


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("n", [257, 4096])
def test_references_agree_mixed(curve, n):
    C = P.CURVES[curve]
    S, B, D, planted = _mixed(curve, n)
    kinds = {k for k, _, _ in planted}
    assert set(E.GADGETS) <= kinds and {"group2", "group3", "group64"} <= kinds
    names = [nm for nm, _ in E.special_scalars(curve, 16, 8)]
    # 4096 rows hold every special scalar in every gadget; 257 rows the first 32 of the 43 scalars
    assert {nm for _, _, nm in planted} >= set(names if n == 4096 else names[:32])
    if n == 4096:
        assert len({(k, nm) for k, _, nm in planted if k in E.GADGETS}) >= len(E.GADGETS) * len(names) - 2
    want = E.expected_by_dlog(curve, S, D)
    assert _c_point(curve, S, B) == want
    Sc = E.canonical(curve, S)
    assert np.array_equal(E.montgomery(curve, Sc), S)
    assert _c_point(curve, Sc, B, canonical=True) == want
    assert E.expected_by_dlog(curve, Sc, D, canonical=True) == want
    sc, pts = _py_inputs(curve, S, B)
    assert all(C.on_curve(p) for p in pts)
    assert C.best_multiexp(sc, pts) == want
    if n == 257:
        assert C.msm_naive(sc, pts) == want
    # the planted rows are what they claim
    for kind, rws, _ in planted:
        if kind == "dup" or kind.startswith("group"):   # one bucket in every window
            assert all(np.array_equal(S[r], S[rws[0]]) and np.array_equal(B[r], B[rws[0]]) for r in rws), kind
        elif kind in ("neg", "ppn"):
            assert pts[rws[-1]] == C.neg(pts[rws[0]]) and sc[rws[-1]] == sc[rws[0]]
            assert kind == "neg" or (pts[rws[1]] == pts[rws[0]] and sc[rws[1]] == sc[rws[0]])
        elif kind == "identity":
            assert pts[rws[0]] is None and sc[rws[1]] == 0
    # sensitivity: each planted gadget's contribution is visible in the answer
    for kind, rws, name in planted:
        if kind == "neg":   # P, -P cancel: removing ONE of them must show
            rows_to_try = rws[:1]
        else:
            rows_to_try = rws[:1] if kind.startswith("group") else rws
        for r in rows_to_try:
            S2, D2 = _perturbed(curve, S, D, r)
            assert E.expected_by_dlog(curve, S2, D2) != want, (kind, r, name)


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("n", [257, 4096])
def test_references_agree_whole_array(curve, n):
    """Every constant and every digit pattern as the scalar of every point
    (over the mixed input's bases: duplicates, negated pairs, identities)."""
    C = P.CURVES[curve]
    _, B, D, _ = _mixed(curve, n)
    pts = None
    for c in (16, 20, 13):
        for name in E.WHOLE_ARRAY:
            if c != 16 and name.startswith("const:"):
                continue
            S = E.whole_array_case(curve, n, name, c)
            want = E.expected_by_dlog(curve, S, D)
            assert _c_point(curve, S, B) == want, (name, c)
            if n == 257 and c == 16:
                if pts is None:
                    pts = _py_inputs(curve, S, B)[1]
                sc = [dict(E.special_scalars(curve, c))[name]] * n
                assert C.best_multiexp(sc, pts) == want, name
            # sensitivity: one point's term changed
            S2, D2 = _perturbed(curve, S, D, n // 2)
            assert E.expected_by_dlog(curve, S2, D2) != want, (name, c)


@pytest.mark.parametrize("curve", [0, 2])
def test_c_port_large(curve):
    """2^18 + 11 (the 8-row table's geometry: two sort blocks per thread, the
    split copy's parts): the C port == the known-dlog point."""
    n = (1 << 18) + 11
    S, B, D, planted = E.mixed_case(curve, n, 16, 8, True)
    assert {k for k, _, _ in planted} >= set(E.GADGETS) | {f"group{g}" for g in E.GROUPS}
    # every boundary of the pipeline carries a gadget
    at = {r for _, rws, _ in planted for r in rws}
    for b in E.boundaries(n, True) + [1, n - 1]:
        assert b - 1 in at and b in at, b
    want = E.expected_by_dlog(curve, S, D)
    assert _c_point(curve, S, B) == want
    S2, D2 = _perturbed(curve, S, D, n - 1)
    assert E.expected_by_dlog(curve, S2, D2) != want
    S = E.whole_array_case(curve, n, "pattern:ones", 16)
    assert _c_point(curve, S, B) == E.expected_by_dlog(curve, S, D)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return N.build(tmp_path_factory)


def test_boundaries_follow_engine(plan_exe):
    """part_starts / sort_block restate csrc/msm_plan.hpp (msm_parts, sort_plan),
    asked through tests/native/plan_dump.cpp."""
    def parts(n, split):   # a row table, host scalars (the split copy) or device scalars
        return N.ask1(plan_exe, "parts %d 1 %d -1" % (n, 1 if split else 0))["pstart"]

    def block(stride):     # (points per coarse thread, points per histogram block) of a raw row
        g = N.ask1(plan_exe, "sort %d 0 0 0 1 0 -1 0 0" % stride)
        return g["p0_gm_ppt"], g["p0_g_ppt"] * k["kSortThreads"]

    k = N.ask1(plan_exe, "consts")
    assert (k["kSortThreads"], k["kSortPerThread"], k["kSortB"]) == (E.SORT_THREADS, E.SORT_PER_THREAD, E.SORT_B)
    assert (k["kSplitCopyMinN"], k["kSplitCopy3MinN"]) == (E.SPLIT_COPY_MIN_N, E.SPLIT_COPY3_MIN_N)
    n = (1 << 18) + 11
    assert E.part_starts(n, True) == [0, 106496, n] and E.part_starts(n, False) == [0, n]
    assert parts(n, True) == [0, 106496, n] and parts(n, False) == [0, n]
    assert E.part_starts((1 << 18) - 1, True) == [0, (1 << 18) - 1] == parts((1 << 18) - 1, True)
    m = (1 << 22) + 3
    assert E.part_starts(m, True) == [0, 1048576, 2621440 + 8192, m] == parts(m, True)
    for s in ((1 << 14) + 5, (1 << 18) - 1, (1 << 18) + 5, 1 << 19, 1 << 20, 1 << 22, (1 << 22) + 3):
        assert block(s) == (E.sort_ppt(s), E.sort_block(s)), s
    assert E.sort_ppt((1 << 14) + 5) == 1 and E.sort_ppt((1 << 18) - 1) == 1 and E.sort_ppt((1 << 18) + 5) == 2
    assert E.sort_ppt(1 << 19) == 4 and E.sort_ppt(1 << 20) == 8 and E.sort_ppt(1 << 22) == 8
    assert E.sort_block(1 << 20) == 4096      # 128 blocks of 8192 points: histogram blocks split in two
    assert E.sort_block((1 << 22) + 3) == 8192
    b = E.boundaries(n, True)
    assert 106496 in b and all(x % 1024 == 0 for x in b) and len(b) == n // 1024


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("c,rows", WIDTHS)
def test_digit_patterns_hold_what_they_claim(curve, c, rows):
    C = P.CURVES[curve]
    W, widths, offsets = E.win_geom(c)
    assert W == (256 + c - 1) // c and sum(widths) == 256 and offsets[-1] + widths[-1] == 256
    assert max(widths) == c
    sp = dict(E.special_scalars(curve, c, rows))
    half = [1 << (cw - 1) for cw in widths]

    def intact(s_kept_bits):
        """windows below the top one whose bits the < r reduction left alone"""
        return [w for w in range(W - 1) if offsets[w] + widths[w] <= s_kept_bits]

    for name, s in sp.items():
        d, cy = E.signed_digits(s, c)
        assert E.from_digits(d, c) == s, name                  # the digits restate the scalar
        assert cy[-1] == 0 and 0 <= d[-1] <= half[-1], name    # the top window never carries
        assert all(-half[w] < d[w] <= half[w] for w in range(W)), name
        # sensitivity: a carry dropped in the recomputation no longer restates the scalar
        for w in range(W):
            if cy[w]:
                assert E.from_digits(E.signed_digits(s, c, drop_carry_at=w)[0], c) != s, (name, w)
    kept = {k: E.clear_top(sum(E._digit_value(k, cw) << o for cw, o in zip(widths, offsets)), C.r)[1]
            for k in E.PATTERN_KINDS}
    d, cy = E.signed_digits(sp["pattern:half"], c)
    ws = intact(kept["half"])
    assert len(ws) >= W - 2 and all(d[w] == half[w] and cy[w] == 0 for w in ws)   # largest digit, no carry
    d, cy = E.signed_digits(sp["pattern:half-1"], c)
    assert all(d[w] == half[w] - 1 and cy[w] == 0 for w in intact(kept["half-1"]))
    d, cy = E.signed_digits(sp["pattern:half+1"], c)
    ws = intact(kept["half+1"])
    assert len(ws) >= W - 2 and d[0] == -(half[0] - 1)
    assert all(d[w] < 0 and cy[w] == 1 for w in ws)          # every window below the top negative with carry
    d, cy = E.signed_digits(sp["pattern:ones"], c)
    ws = intact(kept["ones"])
    assert len(ws) >= W - 2 and d[0] == -1 and cy[0] == 1
    assert all(d[w] == 0 and cy[w] == 1 for w in ws[1:])     # code 0 in every later window, the carry goes on
    assert d[-1] > 0                                           # and lands in the top window
    d, cy = E.signed_digits(sp["pattern:alt"], c)
    assert d[0] == half[0] and cy[0] == 0 and all(d[w] < 0 and cy[w] == 1 for w in intact(kept["half"])[1:])
    # constants: r - 1 and r - 2 differ in window 0 only; (r +- 1) / 2 are neighbours
    assert E.signed_digits(0, c) == ([0] * W, [0] * W)
    assert E.signed_digits(1, c)[0] == [1] + [0] * (W - 1)
    assert sp["const:(r-1)/2"] + sp["const:(r+1)/2"] == C.r and sp["const:r-1"] == C.r - 1
    for j in range(rows if rows > 1 else 0):
        wins = E.row_windows(c, rows, j)
        top_row = j == rows - 1
        body = [w for w in wins if w < W - 1 and offsets[w] + widths[w] <= C.scalar_bits - 1]
        assert top_row or body == wins
        d, cy = E.signed_digits(sp[f"row{j}:half"], c)
        assert all(d[w] == half[w] and cy[w] == 0 for w in body)          # digit == 2^(c-1) in every window of row j
        d, cy = E.signed_digits(sp[f"row{j}:half-1"], c)
        assert all(d[w] == half[w] - 1 and cy[w] == 0 for w in body)
        for kind in ("half+1", "ones"):
            d, cy = E.signed_digits(sp[f"row{j}:{kind}"], c)
            assert j == 0 or cy[wins[0] - 1] == 1                          # the carry enters the row
            assert all(cy[w] == 1 and d[w] <= 0 for w in body)             # goes through it
            assert top_row or cy[wins[-1]] == 1                            # and leaves into row j + 1
            if kind == "ones" and j > 0:
                assert all(d[w] == 0 for w in body)                        # every window of the row is code 0


def test_digit_recomputation_matches_pipeline_model():
    """signed_digits agrees with the pipeline model's k_digits restatement."""
    import pipeline_model as PM

    for c, rows in WIDTHS:
        W = E.win_geom(c)[0]
        for _, s in E.special_scalars(0, c, rows):
            d, _ = E.signed_digits(s, c)
            for x, (mag, neg) in zip(d, PM.digits(s, W)):
                assert abs(x) == mag and (x == 0 or (x < 0) == bool(neg))


def test_plan_widths():
    """The widths the GPU module takes for each path are the plan's."""
    import pipeline_model as PM

    assert PM.make_plan((1 << 14) + 5)["c"] == 12 and PM.make_plan((1 << 18) + 5)["c"] == 16
    assert PM.make_plan((1 << 18) + 5, 13)["W"] == 20 and PM.make_plan((1 << 18) + 5, 20)["W"] == 13

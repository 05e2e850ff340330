"""CPU checks of tests/accum_edge_util.py: the term plan and the digit models
are pinned to the references, every planted proof has accumulate ==
accumulate_msm == the C port == [dlog]G, the event model reaches the branches
each planted case claims on each device path, and a deliberately wrong group
law or recoding gives a different result for every case that claims one."""
import math

import numpy as np
import pytest

import accum as A
import accum_edge_util as X
import accum_ref as R
import accum_util as U
import pasta as P
import plan_native as N
from msm_short_edge_util import glv_model

CURVES = (0, 1, 2)
SHAPE_OF = {0: "simple", 1: "rich", 2: "simple"}   # two-term / sum cases: both shapes between the curves


def _path(lgS=0, tpl=1, lgL=5, quad=False):
    return dict(lgS=lgS, quad_terms=quad, tpl=tpl if lgS == 0 else 0, pstep=2 if lgS == 0 and tpl == 2 else 1, lgL=lgL)


def _check_all_references(case, sample=None):
    """C port == [dlog]G bit for bit for every proof, status 0; both Python
    restatements for the proofs in `sample` (all when None)."""
    sh = case.shape()
    ps = U.to_product_shape(case.cid, sh)
    pts, scs, chs = case.pack()
    _, q, h, st = R.accum_batch(case.cid, ps.c, pts, scs, chs, threads=4)
    assert not st.any()
    n = 0
    for b, pf in enumerate(case.proofs):
        assert case.status(b) == 0, pf["name"]
        want = case.expected_quad(b)
        assert np.array_equal(q[b], want), pf["name"]
        if sample is None or b in sample:
            op = case.oracle_proof(b)
            q1, h1 = A.pack_result(case.C, A.accumulate(case.C, sh, op))
            q2, h2 = A.pack_result(case.C, A.accumulate_msm(case.C, sh, op))
            assert np.array_equal(q1, want) and np.array_equal(q2, want), pf["name"]
            assert np.array_equal(h1, h[b]) and np.array_equal(h2, h[b]), pf["name"]
        n += 1
    assert n == case.enumerated == len(case.proofs)
    return q


# ----------------------------------------------------------------- the models
@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("shape", ["simple", "rich"])
def test_term_plan_matches_accumulate_msm(cid, shape):
    """term_plan's coefficients (e's included) on the known dlogs give the
    points of accumulate_msm on random proofs; the layout matches the
    product's (T terms, pairs inside each output range)."""
    case = X.Case(cid, shape, 11, 0x7E57 + cid)
    for i in range(2):
        case.add_proof(f"random{i}")
    sh = case.shape()
    for b in range(2):
        q, _ = A.pack_result(case.C, A.accumulate_msm(case.C, sh, case.oracle_proof(b)))
        assert np.array_equal(q, case.expected_quad(b))
    pl = case.plan(0)
    npts, _, nsets = U.to_product_shape(cid, sh).layout()
    assert pl.S == nsets and len(case.proofs[0]["dl"]) == npts
    assert pl.T == pl.nslots + 2 * pl.S + 1
    for t0, t1 in pl.pairs:
        assert t1 is None or (t1 == t0 + 1 and pl.terms[t0]["out"] == pl.terms[t1]["out"])
    assert sorted(t for p in pl.pairs for t in p if t is not None) == list(range(pl.T))
    # f slots: first use over the ascending rotation sets, then the h_i
    firsts = []
    for _, qs in X._queries(sh):
        for ref, _, _ in qs:
            if ref != A.H_POINT and ref not in firsts:
                firsts.append(ref)
    assert [t["src"] for t in pl.terms[:len(firsts)]] == firsts
    assert pl.nslots == len(firsts) + sh.quotient_degree


@pytest.mark.parametrize("cid", CURVES)
def test_digit_models_restate_the_halves(cid):
    """sum d_i 8^i == half and sum d_i 2^i == half for both halves of every
    family scalar; the digits stay in range; the deal covers every digit once."""
    fam = X.scalar_family(cid)
    assert len({k for _, k in fam}) > 250
    u8 = 0
    for nm, k in fam:
        for h in glv_model(cid, k):
            assert abs(h) < 1 << 127, nm
            d = X.w3_digits(h)
            assert len(d) == 43 and all(-4 <= x <= 4 for x in d) and sum(x * 8 ** i for i, x in enumerate(d)) == h, nm
            n = X.naf_digits(h)
            assert len(n) == 128 and all(-1 <= x <= 1 for x in n) and sum(x << i for i, x in enumerate(n)) == h, nm
            assert all(not (n[i] and n[i + 1]) for i in range(127)), nm
            # the u = 8 arm: a raw 7 with a carry in
            cy = 0
            for i in range(43):
                u = ((abs(h) >> (3 * i)) & 7) + cy
                cy = u > 4
                u8 += u == 8
        h1, h2 = glv_model(cid, k)
        for S in (1, 2, 8, 32):
            lanes = X.deal(h1, h2, S)
            got = sorted(x for lane in lanes for x in lane)
            want = sorted([(0, i, d) for i, d in enumerate(X.naf_digits(h1)) if d] +
                          [(1, i, d) for i, d in enumerate(X.naf_digits(h2)) if d])
            assert got == want and max(len(x) for x in lanes) - min(len(x) for x in lanes) <= 1
    assert u8 > 100   # "digit 0, carry 1" is exercised
    # a dropped carry changes the value (the sensitivity tests rely on it)
    p = dict(X.OCT_PATTERNS)["5..5"]
    assert sum(x * 8 ** i for i, x in enumerate(X.w3_digits(p, drop_carry_at=3))) != p


@pytest.mark.parametrize("cid", CURVES)
def test_corner_halves_stay_below_2_127(cid):
    """The rounded GLV halves at the lattice-cell corners stay below 2^127 (what
    naf128 and the 43 windows assume); on Pallas and Vesta at least one puts a
    NAF digit at table position 127."""
    top, mx = 0, 0
    for nm, k in X.corner_scalars(cid):
        for h in glv_model(cid, k):
            assert abs(h) < 1 << 127, (nm, math.log2(abs(h)))
            mx = max(mx, abs(h))
            top += X.naf_digits(h)[127] != 0
    assert mx > 1 << 125
    if cid in (0, 1):
        assert top > 0 and 3 * mx > 1 << 128
    else:
        assert top == 0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return N.build(tmp_path_factory)


def test_path_constants(plan_exe):
    """acc_path on the header's constants: the batch sizes of every lgL, the
    quad form of the term additions and the automatic two-term lanes; the
    constants and the same paths asked of the product's acc_path
    (tests/native/plan_dump.cpp over csrc/accum_plan.hpp)."""
    k = X.engine_constants()
    assert k == {"kAccLaneBudget": 1024 * 2 * 64, "kAccSumLanes": 16384}
    kc = N.ask1(plan_exe, "consts")
    assert {nm: kc[nm] for nm in k} == k
    T, Tp, npair = 30, 21, 16

    def native(B, split=-1, tpl=-1):
        g = N.ask1(plan_exe, "acc %d %d %d %d %d %d -1" % (B, T, Tp, npair, split, tpl))
        return dict(lgS=g["lgS"], quad_terms=bool(g["quad_terms"]), tpl=g["tpl"], pstep=g["pstep"], lgL=g["lgL"])

    for B in (8193, 4097, 2049, 257, 129, 1, 34, 35, 3000):
        assert native(B) == X.acc_path(B, T, Tp, npair), B
    assert native(8, split=0, tpl=2) == X.acc_path(8, T, Tp, npair, split=0, tpl=2)
    assert [X.batch_for_lgL(lg, T, Tp, npair) for lg in range(6)] == [8193, 4097, 2049, 257, 129, 1]
    assert X.acc_path(34, T, Tp, npair)["quad_terms"] and not X.acc_path(35, T, Tp, npair)["quad_terms"]
    assert X.acc_path(3000, T, Tp, npair) == dict(lgS=0, quad_terms=False, tpl=2, pstep=2, lgL=2)
    assert X.acc_path(8, T, Tp, npair, split=0, tpl=2)["pstep"] == 2
    for lg in range(1, 6):
        assert X.acc_path(8, T, Tp, npair, split=lg)["lgS"] == lg


# ------------------------------------------------------------ planted proofs
@pytest.fixture(scope="module")
def two_term_cases():
    return {cid: X.two_term_case(cid, SHAPE_OF[cid], 10, 0x2731 + cid) for cid in CURVES}


@pytest.fixture(scope="module")
def sum_cases():
    return {cid: X.sum_case(cid, SHAPE_OF[(cid + 1) % 3], 10, 0x5C3 + cid) for cid in CURVES}


@pytest.mark.parametrize("cid", CURVES)
def test_two_term_cases_references_and_events(cid, two_term_cases):
    """Every planted two-term proof: all references agree with [dlog]G; on the
    k_acc_termmul<2> path the model reproduces the expected dlogs and shows
    the claimed branch of xyzz29_madd; a group law whose doubling returns the
    identity, or whose cancellation falls through, gives a different result."""
    case = two_term_cases[cid]
    _check_all_references(case)
    ran = 0
    for b, pf in enumerate(case.proofs):
        want = case.expected(b)
        for tpl in (2, 1):
            ev = X.AccEvents(case.C.r)
            assert X.model_outputs(case, b, _path(tpl=tpl), ev) == want, (pf["name"], tpl)
            if tpl == 2:
                assert pf["claims"] <= ev.kinds("termmul"), (pf["name"], ev)
        if "madd_dbl" in pf["claims"]:
            assert X.model_outputs(case, b, _path(tpl=2), X.AccEvents(case.C.r, wrong_dbl=True)) != want, pf["name"]
        if "madd_cancel" in pf["claims"]:
            assert X.model_outputs(case, b, _path(tpl=2), X.AccEvents(case.C.r, wrong_cancel=True)) != want, pf["name"]
        ran += 1
    assert ran == case.enumerated
    # the odd range's unpaired last term exists on this shape
    assert any(t1 is None and case.plan(0).terms[t0]["out"] in ("f", "w") for t0, t1 in case.plan(0).pairs) or \
        case.shape_name == "rich"


@pytest.mark.parametrize("cid", CURVES)
def test_sum_cases_references_and_events(cid, sum_cases):
    """Every planted k_acc_sum proof at every lgL and both row steps: the
    model reproduces the expected dlogs, shows the claimed doubling /
    cancellation in the loop or the butterfly, and the wrong group laws give a
    different result.  lgL <= 1 is xyzz29_add, above it xyzz29_add_q."""
    case = sum_cases[cid]
    q = _check_all_references(case)
    for b, pf in enumerate(case.proofs):
        if pf["name"].endswith("adjacent") and "zw" not in pf["name"] and ":f" not in pf["name"]:
            assert not q[b][0].any()      # w = identity: all zero words
        if pf["name"] == "e:ev=0":
            assert not q[b][3].any()
    ran = 0
    seen = {}
    for b, pf in enumerate(case.proofs):
        want = case.expected(b)
        for lgL in range(6):
            for tpl in (1, 2):
                p = _path(tpl=tpl, lgL=lgL)
                ev = X.AccEvents(case.C.r)
                assert X.model_outputs(case, b, p, ev) == want, (pf["name"], p)
                # which of the two a +- pattern meets depends on the lanes (with
                # two-term lanes a pair meets inside its lane, in xyzz29_madd):
                # every planted proof collides on every path, and each path
                # sees both branches between the proofs (below)
                kinds = ev.kinds("sum") if tpl == 1 else {k.replace("madd_", "") for k in ev.kinds()}
                if pf["claims"]:
                    assert kinds & {"dbl", "cancel"}, (pf["name"], p, ev)
                seen.setdefault((lgL, tpl), set()).update(kinds)
                if tpl == 1 and lgL in (1, 3, 4, 5):   # more than one lane / quad: a butterfly
                    seen.setdefault((lgL, "bfly"), set()).update(ev.kinds("sum-bfly"))
                for claim, wrong in (("dbl", dict(wrong_dbl=True)), ("cancel", dict(wrong_cancel=True))):
                    # (the branch the proof was planted for; a +- pattern whose lanes
                    # also double can hide a wrong doubling behind its zero sum)
                    if claim in kinds and claim in pf["claims"]:
                        assert X.model_outputs(case, b, p, X.AccEvents(case.C.r, **wrong)) != want, (pf["name"], p)
        ran += 1
    assert ran == case.enumerated
    for key, kinds in seen.items():
        assert {"dbl", "cancel", "inf+Q"} <= kinds, (key, kinds)


@pytest.mark.parametrize("cid", CURVES)
def test_scalar_family_events_and_dropped_carry(cid):
    """The scalar family through scalar_on_W: references agree (C port for all,
    Python for a sample); on the one-lane path a dropped carry changes the
    result of every scalar that has a carry, and the others have none; on the
    term-addition path 0, +-1, 2^i and lambda 2^i give inf + inf and inf + Q in
    the butterfly and a sum of one table point."""
    case = X.family_case(cid, "simple", 10, 0xFA3 + cid)
    _check_all_references(case, sample=(0, 1, 2, len(case.proofs) // 2, len(case.proofs) - 1))
    with_carry = 0
    for b, pf in enumerate(case.proofs):
        want = case.expected(b)
        pl = case.plan(b)
        ev = X.AccEvents(case.C.r)
        assert X.model_outputs(case, b, _path(), ev) == want, pf["name"]
        # the first window of any term's halves that carries
        drop = None
        for t in pl.terms[:-1]:
            for h in glv_model(cid, t["coef"]):
                cy = 0
                for i in range(42):
                    cy = ((abs(h) >> (3 * i)) & 7) + cy > 4
                    if cy:
                        drop = i if drop is None else min(drop, i)
                        break
        if drop is None:
            continue
        with_carry += 1
        assert X.model_outputs(case, b, _path(), X.AccEvents(case.C.r), drop_carry_at=drop) != want, pf["name"]
    assert with_carry >= len(case.proofs) - 8
    by = {pf["name"]: b for b, pf in enumerate(case.proofs)}
    # no scalar of the term-addition family makes two partial sums collide
    top = 0
    for b, pf in enumerate(case.proofs):
        if pf["name"].startswith(X.TERMADD_NAMES):
            ev = X.AccEvents(case.C.r)
            assert X.model_outputs(case, b, _path(lgS=3), ev) == case.expected(b), pf["name"]
            assert not ev.kinds("termadd") & {"dbl", "cancel"}, (pf["name"], ev)
            top += any(X.naf_digits(h)[127] for t in case.plan(b).terms[:-1] for h in glv_model(cid, t["coef"]))
    assert top > 0 if cid in (0, 1) else top == 0      # table position 127 is read on Pallas and Vesta
    for lgS, quad in ((1, False), (3, False), (5, False), (5, True)):
        for nm in ("const:zero", "const:one", "const:r-1", "2^64", "lam*2^126", "corner:++,0,0"):
            ev = X.AccEvents(case.C.r)
            assert X.model_outputs(case, by[nm], _path(lgS=lgS, quad=quad), ev) == case.expected(by[nm]), (nm, lgS)
            # W_{S-1} always carries 1: one table point on lane 0, nothing on the others
            assert "inf+Q" in ev.kinds("termadd-bfly"), (nm, lgS, ev)
            if lgS >= 2 or nm == "const:zero":
                assert "inf+inf" in ev.kinds("termadd-bfly"), (nm, lgS, ev)
            assert not ev.kinds("termadd") & {"dbl", "cancel"}


@pytest.mark.parametrize("cid", CURVES)
def test_pattern_pairs_references(cid):
    """pair_on_zw puts two base-8 patterns on the last zw pair: references
    agree and the model reproduces them on both one-lane forms."""
    case = X.pattern_pairs_case(cid, SHAPE_OF[cid], 10, 0x9A7 + cid)
    _check_all_references(case, sample=(0, 1, len(case.proofs) - 1))
    for b in range(len(case.proofs)):
        for tpl in (1, 2):
            assert X.model_outputs(case, b, _path(tpl=tpl), X.AccEvents(case.C.r)) == case.expected(b)


def test_gadgets_refuse_instead_of_dropping():
    """pair_on_zw refuses k1 = +-1 (x would be an n-th root of unity) and zero
    scalars; a planting that cannot succeed raises after the redraws."""
    case = X.Case(0, "simple", 10, 1)
    b = case.add_proof("p")
    for k0, k1 in ((5, 1), (5, -1), (0, 7), (5, 0)):
        with pytest.raises(ValueError):
            case.pair_on_zw(b, k0, k1)
    case.set_challenges(b, x=1)
    with pytest.raises(RuntimeError):
        case.scalar_on_W(b, 5)
    calls = []
    with pytest.raises(RuntimeError):
        case._retry(b, lambda: calls.append(1) and False)
    assert len(calls) == X.MAX_REDRAW + 1


# --------------------------------------------------------------- shape limits
def _limit_shape(cid, **kw):
    C = P.CURVES[cid]
    sh = A.synth_vk_points(C, A.simple_example_shape(C, 10), seed=0x11)
    for k, v in kw.items():
        setattr(sh, k, v)
    return sh


def nested_sum(n):
    """A right-nested Sum of n leaves: the postfix stack grows to n."""
    e = A.Advice(n % 3)
    for i in range(n - 1):
        e = A.Sum(A.Advice(i % 3), e)
    return e


def many_rotations_shape(cid, nrot):
    """nrot distinct rotations in all (the shape's own -6, -1, 0, 1 included)."""
    sh = _limit_shape(cid)
    have = set(sh.rotations())
    extra = [r for r in range(2, 200) if r not in have][:nrot - len(have)]
    sh.advice_queries = list(sh.advice_queries) + [(1, r) for r in extra]
    assert len(sh.rotations()) == nrot
    return A.synth_vk_points(P.CURVES[cid], sh, seed=0x11)


def big_set_shape(cid, nq):
    """nq queries in rotation set 0 (advice column 1 queried again and again)."""
    sh = _limit_shape(cid)
    n0 = sum(1 for _, qs in X._queries(sh) for q in qs if q[1] == 0)
    sh.advice_queries = list(sh.advice_queries) + [(1, 0)] * (nq - n0)
    assert max(len(qs) for _, qs in X._queries(sh)) == nq
    return sh


def test_shape_limits_refused():
    """ProofShape.layout() refuses a 17-deep expression stack, 65 rotation
    sets and 62 blinding factors and accepts 16 / 64 / 61.  kAccMaxPerSet (256
    queries in one set) is NOT enforced by the layout call: only
    pm_accum_batch* checks it, when the sets are grouped (covered on the device
    in test_accum_edges_gpu.py)."""
    import halo2_amd as H

    ok = _limit_shape(2, gates=[nested_sum(16)])
    U.to_product_shape(2, ok).layout()
    with pytest.raises(H.PmError, match="deeper than 16"):
        U.to_product_shape(2, _limit_shape(2, gates=[nested_sum(17)])).layout()
    U.to_product_shape(2, many_rotations_shape(2, 64)).layout()
    with pytest.raises(H.PmError, match="too many rotation sets"):
        U.to_product_shape(2, many_rotations_shape(2, 65)).layout()
    U.to_product_shape(2, _limit_shape(2, blinding_factors=61)).layout()
    with pytest.raises(H.PmError, match="blinding_factors too large"):
        U.to_product_shape(2, _limit_shape(2, blinding_factors=62)).layout()
    assert U.to_product_shape(2, big_set_shape(2, 257)).layout()[2] == 4

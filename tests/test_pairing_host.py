"""CPU: pm_accum_decide_host, the host form of the BN254 pairing decider (the
parity form of the kernels and the CPU baseline), against tests/pairing_ref.py,
and pairing_plan.hpp's constants against pow-derived values."""
import json
import os
import re

import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = os.path.join(ROOT, "halo2-aggregation_amd", "csrc", "pairing_plan.hpp")
RAND_TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % PR.R


@pytest.fixture(scope="module")
def pairing():
    return H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


def test_info(pairing):
    info = pairing.info()
    assert info["steps"] == 64 + bin(PR.LOOP)[3:].count("1") + 2 == 102
    assert info["lanes_per_pairing"] == 6 and info["table_bytes"] > 102 * 8 * 36


def test_gt_matches_reference_bit_for_bit(pairing):
    """at most 8 items: the golden pairings as quads (w = [a]G against s_g2 = [b]G2 is e(G1,G2)^(ab) when
    the other three are the identity), the constructed accept / reject, and one random tau"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_bn254.json")))
    n = 0
    for c in g["cases"]:
        a, b = int(c["a"], 16), int(c["b"], 16)
        pr = H.Pairing(None, U.g2_words(PR.G2), U.g2_words(PR.g2_mul(b, PR.G2)))
        q = U.quad_words(U.pt(a), None, None, None)[None]
        ok, st, gt = H.accum_decide_host(pr, q, want_gt=True)
        want = np.array([PR.fp_words(int(x, 16)) for x in c["gt"]], dtype=np.uint64)
        assert np.array_equal(gt[0], want), (c["a"], c["b"])
        assert ok[0] == 0 and st[0] == 0
        n += 1
    fam = {f[0]: f for f in U.family()}
    for name in ("accept", "reject_d_plus_1", "zw_eq_f_reject"):
        q = fam[name][1][None]
        ok, st, gt = H.accum_decide_host(pairing, q, want_gt=True)
        assert np.array_equal(gt[0], U.ref_gt_words(q[0])), name
        n += 1
    pr = H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2(RAND_TAU)))
    q = U.family(RAND_TAU, 3)[1][1][None]
    ok, st, gt = H.accum_decide_host(pr, q, want_gt=True)
    assert np.array_equal(gt[0], U.ref_gt_words(q[0], RAND_TAU)) and ok[0] == 0
    assert n + 1 == 8


@pytest.mark.parametrize("B", [1, 33])
def test_decisions_on_constructed_families(pairing, B):
    q, si, ok, st = U.batch(B)
    h_ok, h_st = H.accum_decide_host(pairing, q, si)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)


def test_every_family(pairing):
    fam = U.family()
    q = np.stack([f[1] for f in fam])
    si = np.array([f[2] for f in fam], dtype=np.uint32)
    ok, st, gt = H.accum_decide_host(pairing, q, si, want_gt=True)
    for f, o, s in zip(fam, ok, st):
        assert (int(o), int(s)) == (f[3], f[4]), f[0]
    names = [f[0] for f in fam]
    assert not gt[names.index("status_in")].any() and not gt[names.index("off_curve")].any()
    one = np.array(PR.gt_words(PR.F12_ONE), dtype=np.uint64).reshape(12, 4)
    assert np.array_equal(gt[names.index("accept")], one) and np.array_equal(gt[names.index("all_inf")], one)
    # without out_gt and without status_in the decisions are the same
    keep = [i for i, f in enumerate(fam) if f[2] == 0]
    ok2, st2 = H.accum_decide_host(pairing, q[keep])
    assert np.array_equal(ok2, ok[keep]) and np.array_equal(st2, st[keep])


def test_plan_constants_match_pow():
    src = open(PLAN).read()
    assert int(re.search(r"constexpr uint64_t kX = (0x[0-9a-f]+)ull;", src).group(1), 16) == PR.X
    low = int(re.search(r"constexpr uint64_t kLoopLow = (0x[0-9a-f]+)ull;", src).group(1), 16)
    assert (1 << 64) + low == PR.LOOP and "constexpr int kLoopBits = 65;" in src
    body = src[src.index("constexpr uint64_t kFrob[2][6][2][4]"):src.index("// the twist's Frobenius")]
    words = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", body)]
    assert len(words) == 2 * 6 * 2 * 4
    it = iter(words)
    for j in (1, 2):
        for k in range(6):
            want = PR.f2_pow(PR.XI, k * (PR.P**j - 1) // 6)
            got = tuple(sum(next(it) << (64 * i) for i in range(4)) for _ in range(2))
            assert got == want, (j, k)
    assert PR.f2_pow(PR.XI, 2 * (PR.P - 1) // 6) == PR.FROB_X and PR.f2_pow(PR.XI, 3 * (PR.P - 1) // 6) == PR.FROB_Y


def test_walk_items_decide_as_constructed(pairing):
    """pairing_util.walk: distinct items, and the host form decides them as the construction states"""
    q, si, ok, st = U.walk(200)
    assert len({q[i].tobytes() for i in range(200)}) == 200
    assert list(np.flatnonzero(si)) == [96, 193] and list(np.flatnonzero(st)) == [U.WALK_OFF_CURVE, 96, 193]
    assert st[U.WALK_OFF_CURVE] == H.DECIDE_NOT_ON_CURVE
    assert [int(v) for v in ok[:9]] == [1, 1, 0, 1, 0, 0, 1, 1, 0] and ok[96] == 0 and ok.sum() == 131
    h_ok, h_st, h_gt = H.accum_decide_host(pairing, q, si, want_gt=True)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)
    for i in (0, 2, 199):
        assert np.array_equal(h_gt[i], U.ref_gt_words(q[i])), i

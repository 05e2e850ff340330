"""CPU: tests/pairing_ref.py, the big-integer restatement of the BN254 optimal ate
pairing that the decider's tests compare against, pinned by the properties a
pairing has (there is no published vector for this exact tower and line form),
and tests/golden/pairing_bn254.json, which tools/make_pairing_golden.py wrote
from it."""
import json
import os

import pairing_ref as PR
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def e11():
    return PR.pairing(PR.G1, PR.G2)


def test_parameters():
    assert PR.P == 36 * PR.X**4 + 36 * PR.X**3 + 24 * PR.X**2 + 6 * PR.X + 1
    assert PR.R == 36 * PR.X**4 + 36 * PR.X**3 + 18 * PR.X**2 + 6 * PR.X + 1
    assert PR.LOOP == 6 * PR.X + 2 == 29793968203157093288
    assert (PR.P**12 - 1) % PR.R == 0
    assert PR.f2_mul(PR.B2, PR.XI) == (3, 0)


def test_g2_generator_on_twist_and_of_order_r():
    assert PR.g2_on_curve(PR.G2)
    assert PR.g2_mul(PR.R, PR.G2, reduce=False) is None
    assert PR.g2_mul(PR.R - 1, PR.G2) == PR.g2_neg(PR.G2)


def test_frobenius_images_lie_on_the_twist():
    q1 = PR.g2_frobenius(PR.G2)
    q2 = PR.g2_neg(PR.g2_frobenius(q1))
    assert PR.g2_on_curve(q1) and PR.g2_on_curve(q2)
    # pi acts on G2 as multiplication by p
    assert q1 == PR.g2_mul(PR.P % PR.R, PR.G2)


def test_nondegenerate_and_of_order_r(e11):
    assert e11 != PR.F12_ONE
    assert PR.f12_pow(e11, PR.R) == PR.F12_ONE


@pytest.mark.parametrize("a", [0x9E3779B97F4A7C15, 0x5EED5EED5EED5EED5EED5EED5EED5EED5EED])
def test_bilinear_in_both_arguments(e11, a):
    want = PR.f12_pow(e11, a)
    assert PR.pairing(PR.g1_mul(a, PR.G1), PR.G2) == want
    assert PR.pairing(PR.G1, PR.g2_mul(a, PR.G2)) == want


def test_identity_pairs_to_one():
    assert PR.pairing(None, PR.G2) == PR.F12_ONE


def test_product_of_miller_values_then_one_exponentiation(e11):
    a, b = 777, 999
    Pa, Qb = PR.g1_mul(a, PR.G1), PR.g2_mul(b, PR.G2)
    both = PR.final_exp(PR.f12_mul(PR.miller(Pa, PR.G2), PR.miller(PR.G1, Qb)))
    assert both == PR.f12_mul(PR.pairing(Pa, PR.G2), PR.pairing(PR.G1, Qb)) == PR.f12_pow(e11, a + b)


def test_decider_identity_on_known_discrete_logs():
    tau, a, b, c = 0x1234567890ABCDEF1234567890ABCDEF, 55555, 777, 999
    d = (a * tau - b - c) % PR.R
    s = PR.g2_mul(tau, PR.G2)
    g = [PR.g1_mul(k, PR.G1) for k in (a, b, c, d)]
    assert PR.accum_gt(*g, s) == PR.F12_ONE
    g[3] = PR.g1_mul(d + 1, PR.G1)
    assert PR.accum_gt(*g, s) != PR.F12_ONE


def test_words_round_trip():
    assert PR.words_fp(PR.fp_words(12345)) == 12345
    assert PR.gt_words(PR.F12_ONE)[:4] == PR.fp_words(1) and not any(PR.gt_words(PR.F12_ONE)[4:])
    assert PR.honest_W(10, 4, 2, 5) * (5 - 2) % PR.R == 6


def test_golden_file_matches(e11):
    import importlib.util

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "pairing_bn254.json")))
    spec = importlib.util.spec_from_file_location("make_pairing_golden", os.path.join(ROOT, "tools", "make_pairing_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert [(int(c["a"], 16), int(c["b"], 16)) for c in g["cases"]] == tool.CASES and len(tool.CASES) == 4
    assert [int(x, 16) for x in g["cases"][0]["gt"]] == PR.f12_flat(e11)
    for c in g["cases"][1:]:
        a, b = int(c["a"], 16), int(c["b"], 16)
        assert [int(x, 16) for x in c["gt"]] == PR.f12_flat(PR.f12_pow(e11, a * b % PR.R))

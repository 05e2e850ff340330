"""CPU tests of the extended-domain reference (tests/domain_ref.py): the
restated conversions against their defining properties on the three scalar
fields, k <= 6 and extended_k - k <= 3."""
import random

import pytest

import domain_ref as D
import pasta as P
import poly_ref as R

SHAPES = [(k, e) for k in range(0, 7) for e in range(0, 4)]


def _rand(rng, r, m):
    return [rng.randrange(r) for _ in range(m)]


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_coeff_to_extended_is_evaluation_on_the_coset(cid):
    r = P.CURVES[cid].r
    for k, e in SHAPES:
        for zeta in D.cube_roots(r):
            d = D.Domain(r, k, k + e, zeta=zeta)
            a = _rand(random.Random(100 * k + e), r, d.n)
            got = d.coeff_to_extended(a)
            assert len(got) == d.N
            for j in range(d.N):
                x = zeta * pow(d.extended_omega, j, r) % r
                assert got[j] == R.eval_polynomial(a, x, r), (k, e, j)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_round_trip_and_truncation(cid):
    r = P.CURVES[cid].r
    for k, e in SHAPES:
        d = D.Domain(r, k, k + e)
        a = _rand(random.Random(7 * k + e), r, d.n)
        ext = d.coeff_to_extended(a)
        assert d.extended_to_coeff(ext) == a + [0] * (d.N - d.n)
        assert d.extended_to_coeff(ext, keep=d.n) == a
        assert d.extended_to_coeff(ext, keep=1) == a[:1]


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_vanishing_division_recovers_the_quotient(cid):
    """h = q (X^n - 1) with deg q < n (d - 1), d = 2^e: dividing h's coset
    evaluations by the vanishing polynomial gives q's, and extended_to_coeff
    returns q."""
    r = P.CURVES[cid].r
    for k, e in SHAPES:
        if e == 0:
            continue  # d = 1: no room for a quotient
        for zeta in D.cube_roots(r):
            d = D.Domain(r, k, k + e, zeta=zeta)
            m = d.n * ((1 << e) - 1)
            q = _rand(random.Random(31 * k + e), r, m)
            h = [0] * (m + d.n)  # q X^n - q
            for i, c in enumerate(q):
                h[i + d.n] = (h[i + d.n] + c) % r
                h[i] = (h[i] - c) % r
            divided = d.divide_by_vanishing_poly(d.coeff_to_extended(h))
            assert divided == d.coeff_to_extended(q), (k, e)
            assert d.extended_to_coeff(divided, keep=m) == q, (k, e)
            assert d.extended_to_coeff(divided) == q + [0] * d.n


def test_t_evaluations_and_roots():
    for cid in (0, 1, 2):
        r = P.CURVES[cid].r
        for k, e in SHAPES:
            d = D.Domain(r, k, k + e)
            assert len(d.t_evaluations) == 1 << e
            assert pow(d.omega, d.n, r) == 1 and (d.n == 1 or pow(d.omega, d.n // 2, r) == r - 1)
            for i, t in enumerate(d.t_evaluations):
                x = d.zeta * pow(d.extended_omega, i, r) % r
                assert t * (pow(x, d.n, r) - 1) % r == 1


def test_extended_k_for():
    assert D.extended_k_for(5, 1) == 5
    assert D.extended_k_for(5, 2) == 6
    assert D.extended_k_for(5, 3) == 7
    assert D.extended_k_for(5, 4) == 7
    assert D.extended_k_for(5, 5) == 8

"""CPU checks of the restated opening arithmetic (tests/poly_ref.py): the
division identity a(X) == q(X)(X - z) + a(z) coefficient by coefficient, and
the linearity the device kernels rely on (the witness of a set is the
v-weighted sum of the members' quotients)."""
import random

import pytest

import pasta as P
import poly_ref as R


def _mul_linear(q, z, r):
    """q(X) (X - z) as a coefficient list of len(q) + 1"""
    out = [0] * (len(q) + 1)
    for t, c in enumerate(q):
        out[t + 1] = (out[t + 1] + c) % r
        out[t] = (out[t] - z * c) % r
    return out


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_division_identity(cid):
    r = P.CURVES[cid].r
    rng = random.Random(31 + cid)
    cases = []
    for n in (1, 2, 3, 8, 9, 64, 257):
        cases.append(([rng.randrange(r) for _ in range(n)], rng.randrange(r)))
    for z in (0, 1, r - 1):
        cases.append(([rng.randrange(r) for _ in range(33)], z))
    cases.append(([r - 1] * 40, r - 1))
    cases.append(([0] * 17, rng.randrange(r)))
    for a, z in cases:
        q = R.kate_division(a, z, r)
        assert len(q) == len(a) - 1
        rem = R.eval_polynomial(a, z, r)
        assert rem == sum(c * pow(z, t, r) for t, c in enumerate(a)) % r
        back = _mul_linear(q, z, r) if q else [0]
        back[0] = (back[0] + rem) % r
        assert back == a
        if q:  # the recurrence as include/pasta_msm.h states it: q_{n-2} = a_{n-1}, q_{t-1} = a_t + z q_t
            assert q[-1] == a[-1]
            assert all(q[t - 1] == (a[t] + z * q[t]) % r for t in range(1, len(q)))
            assert (a[0] + z * q[0]) % r == rem


@pytest.mark.parametrize("cid", [0, 2])
def test_witness_is_linear_in_the_members(cid):
    r = P.CURVES[cid].r
    rng = random.Random(77 + cid)
    for n, m in ((1, 3), (2, 2), (37, 1), (37, 5), (64, 24)):
        polys = [[rng.randrange(r) for _ in range(n)] for _ in range(m)]
        polys.append(polys[0])  # a polynomial listed twice
        for v in (rng.randrange(r), 0, 1, r - 1):
            z = rng.randrange(r)
            wit, ev = R.gwc_witness(polys, z, v, r)
            mm = len(polys)
            want = [0] * (n - 1)
            for i, p in enumerate(polys):
                w = pow(v, mm - 1 - i, r)
                want = [(x + w * y) % r for x, y in zip(want, R.kate_division(p, z, r))]
            assert wit == want
            batch = R.batch_poly(polys, v, r)
            # subtracting the batched evaluation changes a_0 only: same quotient
            assert wit == R.kate_division(batch, z, r)
            assert ev == R.eval_polynomial(batch, z, r)


def test_montgomery_inputs_commute_with_division():
    r = P.CURVES[2].r
    rng = random.Random(5)
    a = [rng.randrange(r) for _ in range(50)]
    z = rng.randrange(r)
    am = R.raw_ints(R.to_array(r, a))
    assert R.from_array(r, R.to_array(r, a)) == a
    assert [x * P.R_MONT % r for x in R.kate_division(a, z, r)] == R.kate_division(am, z, r)

"""CPU tests of tests/gp_ref.py, the restatement the grand-product GPU tests
compare against: the one-inverse form equals the literal loop (zeros at every
position that matters, every `active`, all three moduli), the recurrence
identity, and the permutation argument's end-to-end property."""
import random

import pytest

import gp_ref as G
import pasta as P

MODULI = [P.CURVES[c].r for c in (0, 1, 2)]


def _cols(rng, r, n, count):
    return [[rng.randrange(r) for _ in range(n)] for _ in range(count)]


def _lookup(rng, r):
    return G.lookup_set(0, 1, 2, 3, rng.randrange(r), rng.randrange(r))


def test_batch_invert():
    for r in MODULI:
        vals = [0, 1, r - 1, 2, 0, 12345]
        got = G.batch_invert(vals, r)
        assert [g * v % r for g, v in zip(got, vals)] == [0, 1, 1, 1, 0, 1]


@pytest.mark.parametrize("r", MODULI)
@pytest.mark.parametrize("n", [1, 2, 17, 300])
def test_fast_equals_literal(r, n):
    rng = random.Random(n)
    omega = rng.randrange(r)
    for active in sorted({1, max(1, n - 5), n}):
        base = _cols(rng, r, n, 4)
        num, den = _lookup(rng, r)
        beta, gamma = den[0][3], den[1][3]
        zero_rows = [None, 0, active // 2, active - 2, active - 1, n - 1]
        for zr in zero_rows:
            cols = [list(c) for c in base]
            if zr is not None:
                if not 0 <= zr < n:
                    continue
                cols[2][zr] = -beta % r  # A'[zr] + beta == 0
            for nu, de in ((num, den), ([(0, G.OMEGA, 5, gamma)], den), ([], den), (num, [])):
                want = G.grand_product_literal(cols, nu, de, n, active, 7, omega, r)
                assert G.grand_product_fast(cols, nu, de, n, active, 7, omega, r) == want, (n, active, zr)
                assert len(want[0]) == active and want[1] == want[0][-1]
            if zr is not None and zr >= active - 1:  # such a zero has no effect
                assert G.grand_product_literal(cols, num, den, n, active, 7, omega, r) == \
                    G.grand_product_literal(base, num, den, n, active, 7, omega, r)
        # two zeros: everything past the first is zero
        if active >= 6:
            cols = [list(c) for c in base]
            cols[2][1] = cols[2][3] = -beta % r
            z, last = G.grand_product_fast(cols, num, den, n, active, 7, omega, r)
            assert (z, last) == G.grand_product_literal(cols, num, den, n, active, 7, omega, r)
            assert z[1] != 0 and not any(z[2:]) and last == 0


@pytest.mark.parametrize("r", MODULI)
def test_recurrence_identity(r):
    rng = random.Random(3)
    n, active = 300, 295
    cols = _cols(rng, r, n, 4)
    num, den = _lookup(rng, r)
    cols[2][40] = -den[0][3] % r
    z, _ = G.grand_product_fast(cols, num, den, n, active, 1, None, r)
    for i in range(active - 1):
        N = G.factor_row(cols, num[0], i, None, r) * G.factor_row(cols, num[1], i, None, r) % r
        D = G.factor_row(cols, den[0], i, None, r) * G.factor_row(cols, den[1], i, None, r) % r
        if D:
            assert z[i + 1] * D % r == z[i] * N % r, i
        else:
            assert i == 40 and z[i + 1] == 0


@pytest.mark.parametrize("r", MODULI)
def test_permutation_ends_at_one(r):
    rng = random.Random(11)
    n = 64
    cols, vals, sigmas, omega, delta = G.permutation_instance(r, 4, n, 5)
    cols = [c + [rng.randrange(r)] for c in cols]  # one more row: active - 1 == n covers every cell
    beta, gamma = rng.randrange(r), rng.randrange(r)
    for chunk in (1, 2, 3, 4):
        sets = G.permutation_sets(vals, sigmas, chunk, beta, gamma, delta, r)
        for fn in (G.grand_product_literal, G.grand_product_fast):
            zs, lasts = G.grand_products(cols, sets, n + 1, n + 1, 1, omega, r, chain=True, fn=fn)
            assert lasts[-1] == 1, chunk
            assert all(z[0] == l for z, l in zip(zs[1:], lasts))
        if len(sets) > 1:
            assert lasts[0] != 1

"""CPU tests that pin tests/lookup_ref.py independently of the device code:
the worked example of the header's definition, and on seeded random cases the
properties the lookup argument needs of (A', S') plus a brute-force search for
the failing row."""
import random

import lookup_ref as L
import pasta as P


def test_worked_example():
    a, s = [3, 1, 3, 2, 1, 3], [1, 2, 3, 5, 5, 7]
    assert L.permute_pair(a, s, 6) == ([1, 1, 2, 3, 3, 3], [1, 7, 2, 3, 5, 5])


def test_usable_prefix_only():
    # rows behind `usable` enter neither column
    a, s = [2, 1, 2, 9], [1, 2, 4, 0]
    assert L.permute_pair(a, s, 3) == ([1, 2, 2], [1, 2, 4])
    assert L.permute_pair(a, s, 4) == 3  # 9 is not in the table


def _brute_force_failing_row(a, s, usable):
    sa, table = sorted(a[:usable]), set(s[:usable])
    for row, v in enumerate(sa):
        if (row == 0 or v != sa[row - 1]) and v not in table:
            return row
    return None


def test_random_cases_properties():
    rng = random.Random(0x10C)
    ok = bad = 0
    for case in range(200):
        r = P.CURVES[case % 3].r
        usable = rng.randrange(1, 40)
        n = usable + rng.randrange(0, 3)
        pool = [rng.randrange(r) for _ in range(rng.randrange(1, 12))] + [0, r - 1]
        s = [rng.choice(pool) for _ in range(n)]
        if case % 4 == 0:  # inputs drawn from the whole pool: a value may be absent from the table
            a = [rng.choice(pool) for _ in range(n)]
        else:
            a = [rng.choice(s[:usable]) for _ in range(n)]
        got = L.permute_pair(a, s, usable)
        want_row = _brute_force_failing_row(a, s, usable)
        if want_row is not None:
            assert got == want_row
            bad += 1
            continue
        ok += 1
        ap, sp = got
        assert len(ap) == len(sp) == usable
        assert ap == sorted(a[:usable])           # a sorted permutation of A
        assert sorted(sp) == sorted(s[:usable])   # a permutation of S
        for i in range(usable):
            assert ap[i] == sp[i] or (i > 0 and ap[i] == ap[i - 1])
    assert ok >= 100 and bad >= 10


def test_compress_is_horner():
    r = P.CURVES[2].r
    rng = random.Random(7)
    cols = [[rng.randrange(r) for _ in range(5)] for _ in range(4)]
    theta = rng.randrange(r)
    want = [sum(pow(theta, 3 - k, r) * cols[k][i] for k in range(4)) % r for i in range(5)]
    assert L.compress(cols, theta, r) == want
    assert L.compress(cols[:1], theta, r) == cols[0]

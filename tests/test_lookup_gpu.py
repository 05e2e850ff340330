"""GPU tests of the lookup argument's permuted columns
(pm_lookup_compress_device, pm_lookup_permute*) against tests/lookup_ref.py:
bit-identical A' and S' on the three scalar fields at every size where the sort
or the pairing changes path (T = one sorted tile, M = one merge block's output,
both taken from the wrapper module), key shapes that break a wrong comparator,
the pairing's corner cases, the failure status, batching, the host form, the
compression, and, independent of the restatement, the lookup grand product
closing to 1.

Values are plain integers mod r; the order under test is the order of those
integers, not of the stored Montgomery words, so every random column already
distinguishes the two."""
import functools
import random

import numpy as np
import pytest

import halo2_amd as H
import lookup_ref as L
import pasta as P
import poly_ref as R

pytestmark = pytest.mark.gpu

T, M = H.LOOKUP_TILE, H.LOOKUP_MERGE
SENT = 2**64 - 1
POOL_N = 1 << 14


def _dev(gpu_ctx, arr):
    import torch

    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(torch.device("cuda", gpu_ctx.device))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _arr(r, vals):
    """plain integers -> (n, 4) u64 Montgomery, canonical"""
    return R.from_raw([v * P.R_MONT % r for v in vals])


@functools.lru_cache(maxsize=None)
def _pool(cid):
    """POOL_N distinct random values per field, drawn once"""
    r = P.CURVES[cid].r
    rng = random.Random(0x100C + cid)
    vals = set()
    while len(vals) < POOL_N:
        vals.add(rng.randrange(r))
    vals = list(vals)
    rng.shuffle(vals)
    return vals


def _permute(gpu_ctx, cid, pairs, usable, extra=0, in_place=False):
    """Runs the P pairs (a, s) of integer lists in one call over n = usable +
    extra rows.  Checks what no case may break (rows behind `usable`, and in
    the disjoint form the inputs, are unchanged) and returns per pair
    (A' (usable, 4), S' (usable, 4), status, row)."""
    import torch

    r = P.CURVES[cid].r
    n = usable + extra
    ins = []
    for a, s in pairs:
        # rows behind `usable` hold values that would change the result if they entered it
        ins.append((_arr(r, list(a[:usable]) + [(7 * i + 1) % r for i in range(extra)]),
                    _arr(r, list(s[:usable]) + [(11 * i + 3) % r for i in range(extra)])))
    d_in = [(_dev(gpu_ctx, x), _dev(gpu_ctx, y)) for x, y in ins]
    if in_place:
        d_out = d_in
    else:
        full = np.full((n, 4), SENT, dtype=np.uint64)
        d_out = [(_dev(gpu_ctx, full), _dev(gpu_ctx, full)) for _ in pairs]
    torch.cuda.synchronize()
    st = gpu_ctx.lookup_permute_device(cid, [t[0].data_ptr() for t in d_in], [t[1].data_ptr() for t in d_in], n, usable,
                                       [t[0].data_ptr() for t in d_out], [t[1].data_ptr() for t in d_out])
    assert st.shape == (len(pairs), 2)
    out = []
    for p in range(len(pairs)):
        oa, os_ = _host(d_out[p][0]), _host(d_out[p][1])
        if in_place:
            assert np.array_equal(oa[usable:], ins[p][0][usable:]) and np.array_equal(os_[usable:], ins[p][1][usable:])
        else:
            assert (oa[usable:] == SENT).all() and (os_[usable:] == SENT).all()
            assert np.array_equal(_host(d_in[p][0]), ins[p][0]) and np.array_equal(_host(d_in[p][1]), ins[p][1])
        out.append((oa[:usable], os_[:usable], int(st[p, 0]), int(st[p, 1])))
    return out


def _expect(r, got, a, s, usable, tag=None):
    """one pair's result against the restatement"""
    oa, os_, status, row = got
    want = L.permute_pair(a, s, usable)
    if isinstance(want, int):
        assert (status, row) == (1, want), tag
        assert np.array_equal(oa, _arr(r, sorted(a[:usable]))), tag  # A' is still the sorted column
        return
    assert (status, row) == (0, 0), tag
    assert np.array_equal(oa, _arr(r, want[0])), tag
    assert np.array_equal(os_, _arr(r, want[1])), tag


def _check(gpu_ctx, cid, a, s, usable, extra=0, in_place=False, tag=None):
    got = _permute(gpu_ctx, cid, [(a, s)], usable, extra, in_place)[0]
    _expect(P.CURVES[cid].r, got, a, s, usable, tag)
    return got


def _drawn(cid, usable, seed):
    """a table with a few duplicates and inputs drawn from it with repeats"""
    rng = random.Random(seed)
    pool = _pool(cid)
    distinct = max(1, (3 * usable) // 4)
    s = [pool[i % distinct] for i in range(usable)]
    rng.shuffle(s)
    a = [s[rng.randrange(max(1, usable // 2))] for _ in range(usable)]
    return a, s


# ... and around half a tile, the rows of one block of the pairing kernels
SIZES = [1, 2, 3, 5, 31, 32, 33, 34, T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, T + 1, 2 * T + 1, 5 * T + 7, 3 * M + 1]


# ---------------------------------------------------------------- sizes and forms
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_every_size_disjoint(gpu_ctx, cid):
    for usable in SIZES:
        a, s = _drawn(cid, usable, 0xA0 + usable)
        for extra in (0, 6):
            _check(gpu_ctx, cid, a, s, usable, extra, tag=(usable, extra))


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_in_place(gpu_ctx, cid):
    for usable in (1, 5, 33, T, T + 1, 2 * T + 1):
        a, s = _drawn(cid, usable, 0xB0 + usable)
        for extra in (0, 6):
            _check(gpu_ctx, cid, a, s, usable, extra, in_place=True, tag=(usable, extra))


# ---------------------------------------------------------------- comparator
def _self_table(gpu_ctx, cid, keys, seed, tag):
    """the table is the input in another order: the pairing succeeds whatever the keys"""
    rng = random.Random(seed)
    s = list(keys)
    rng.shuffle(s)
    _check(gpu_ctx, cid, list(keys), s, len(keys), tag=tag)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_key_shapes(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(0xC0 + cid)
    low = rng.getrandbits(224)
    top_only = [low + (k << 224) for k in range(0x30)]            # differ in the top word alone
    high = (rng.getrandbits(221) << 32) % r
    bottom_only = [high + k for k in rng.sample(range(1 << 32), 40)]  # differ in the bottom word alone
    crossed = []                                                  # adjacent words in opposite order
    for j in range(7):
        crossed += [(5 << (32 * j)) + (1 << (32 * (j + 1))), (1 << (32 * j)) + (5 << (32 * (j + 1)))]
    assert all(k < r for k in top_only + bottom_only + crossed)
    for name, keys in (("top", top_only), ("bottom", bottom_only), ("crossed", crossed),
                       ("mixed", top_only + bottom_only + crossed + [0, r - 1, 1, r - 2])):
        keys = list(keys)
        rng.shuffle(keys)
        _self_table(gpu_ctx, cid, keys, 1, name)
    pool = _pool(cid)
    n = T + 5
    ordered = sorted(pool[:n])
    _self_table(gpu_ctx, cid, ordered, 2, "sorted")
    _self_table(gpu_ctx, cid, ordered[::-1], 3, "reversed")
    _self_table(gpu_ctx, cid, [pool[0]] * n, 4, "all equal")
    _self_table(gpu_ctx, cid, [0] * 7 + [r - 1] * 9, 5, "0 and r - 1")


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_long_runs_and_tile_boundaries(gpu_ctx, cid):
    rng = random.Random(0xD0 + cid)
    ordered = sorted(_pool(cid)[:4 * T])
    # a run of T + 300 equal keys that starts at sorted row 1000, mid-tile
    n = 3 * T + 11
    keys = ordered[:1000] + [ordered[1000]] * (T + 300) + ordered[1001:1001 + n - 1000 - (T + 300)]
    assert len(keys) == n and keys == sorted(keys)
    rng.shuffle(keys)
    _self_table(gpu_ctx, cid, keys, 6, "long run")
    # the same keys on both sides of every tile boundary of the sorted column
    keys = list(ordered)
    for b in range(T, 4 * T, T):
        keys[b] = keys[b - 1]
    rng.shuffle(keys)
    _self_table(gpu_ctx, cid, keys, 7, "straddling")
    # ... and runs of three around the boundaries, with a table holding each value once more than needed
    keys = list(ordered[:2 * T + 2])
    for b in (T, 2 * T):
        keys[b + 1] = keys[b] = keys[b - 1]
    a = list(keys)
    rng.shuffle(a)
    _check(gpu_ctx, cid, a, sorted(set(keys)) + ordered[3 * T:3 * T + 4], 2 * T + 2, tag="runs of three")


# ---------------------------------------------------------------- pairing
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_pairing_cases(gpu_ctx, cid):
    r = P.CURVES[cid].r
    pool = _pool(cid)
    rng = random.Random(0xE0 + cid)
    # the table is the input as a multiset, all distinct: no repeated row
    u = T + 37
    s = pool[:u]
    a = list(s)
    rng.shuffle(a)
    got = _check(gpu_ctx, cid, a, s, u, tag="R = 0")
    assert np.array_equal(got[0], got[1])
    # one input value repeated `usable` times: every other table value is scattered, from the back
    for u in (5, T + 1, 2 * T + 3):
        s = pool[:u]
        got = _check(gpu_ctx, cid, [s[u // 2]] * u, s, u, extra=6, tag=("R = usable - 1", u))
        rest = sorted(v for v in s if v != s[u // 2])
        assert np.array_equal(got[1][1:], _arr(r, rest[::-1]))
    # table values absent from the input
    u = T + 37
    s = pool[:u]
    a = [s[rng.randrange(u // 2)] for _ in range(u)]
    _check(gpu_ctx, cid, a, s, u, tag="absent table values")
    # table duplicates where the input has the value once
    s = [pool[0]] * 3 + [pool[1]] * 2 + pool[2:u - 3]
    a = [pool[0], pool[1]] + [pool[2 + rng.randrange(8)] for _ in range(u - 2)]
    rng.shuffle(s)
    rng.shuffle(a)
    assert len(s) == len(a) == u
    _check(gpu_ctx, cid, a, s, u, tag="table duplicates")


def test_range_table_uniform_inputs(gpu_ctx):
    u = (1 << 16) + 1
    rng = random.Random(0xF0)
    s = [i & 0xFFFF for i in range(u)]
    a = [rng.randrange(1 << 16) for _ in range(u)]
    _check(gpu_ctx, 2, a, s, u, extra=6, tag="range table")


# ---------------------------------------------------------------- failure status
@pytest.mark.parametrize("cid", [0, 1, 2])
@pytest.mark.parametrize("usable", [6, T + 9])
def test_missing_values_are_a_status(gpu_ctx, cid, usable):
    r = P.CURVES[cid].r
    rng = random.Random(0x1F0 + cid)
    u = usable
    s = [2 * (i + 1) for i in range(u)]  # even values: every odd one is absent
    base = [s[rng.randrange(u)] for _ in range(u)]
    good = _drawn(cid, u, 0x2F0)
    mid = sorted(base)[u // 2]
    cases = {
        "first row": (base[:-1] + [1], 0),
        "last row": (base[:-1] + [r - 1], u - 1),
        "mid column": (base[:-1] + [mid + 1], None),
        "one above": (base[:-1] + [s[3] + 1], None),
        "one below": (base[:-1] + [s[3] - 1], None),
        "two missing": (base[:-2] + [mid + 1, 1], 0),
        "two missing, neither at row 0": (base[:-2] + [mid + 1, mid - 1], None),
    }
    for tag, (a, want_row) in cases.items():
        want = L.permute_pair(a, s, u)
        assert isinstance(want, int) and (want_row is None or want == want_row), tag
        # the failing pair between two good ones
        got = _permute(gpu_ctx, cid, [good, (a, s), good], u, extra=6)
        _expect(r, got[1], a, s, u, tag)
        assert got[1][2:] == (1, want), tag
        for g in (got[0], got[2]):
            _expect(r, g, good[0], good[1], u, tag)


# ---------------------------------------------------------------- batching and the host form
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_three_pairs_in_one_call(gpu_ctx, cid):
    u = 2 * T + 1
    pairs = [_drawn(cid, u, 0x300), _drawn(cid, u, 0x301), _drawn(cid, u, 0x302)]
    pairs[1] = (pairs[1][0][:-1] + [P.CURVES[cid].r - 1], pairs[1][1])  # fails at the last row
    together = _permute(gpu_ctx, cid, pairs, u, extra=6)
    for p, pair in enumerate(pairs):
        alone = _permute(gpu_ctx, cid, [pair], u, extra=6)[0]
        assert together[p][2:] == alone[2:] == ((1, u - 1) if p == 1 else (0, 0))
        assert np.array_equal(together[p][0], alone[0])
        if p != 1:
            assert np.array_equal(together[p][1], alone[1])
        _expect(P.CURVES[cid].r, together[p], pair[0], pair[1], u, p)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_host_form_matches_device_form(gpu_ctx, cid):
    r = P.CURVES[cid].r
    for usable in (1, 5, T + 1):
        a, s = _drawn(cid, usable, 0x400 + usable)
        n = usable + 2
        ia, is_ = _arr(r, a + [3, 4]), _arr(r, s + [5, 6])
        oa, os_, st = gpu_ctx.lookup_permute(cid, ia, is_, usable)
        dev = _permute(gpu_ctx, cid, [(a, s)], usable, extra=2)[0]
        assert oa.shape == os_.shape == (n, 4) and tuple(st) == (0, 0)
        assert np.array_equal(oa[:usable], dev[0]) and np.array_equal(os_[:usable], dev[1])
        assert np.array_equal(oa[usable:], ia[usable:]) and np.array_equal(os_[usable:], is_[usable:])
    a, s = [5, 3, 5], [3, 4, 6]
    oa, _, st = gpu_ctx.lookup_permute(cid, _arr(r, a), _arr(r, s), 3)
    assert tuple(st) == (1, 1) and np.array_equal(oa, _arr(r, [3, 5, 5]))


# ---------------------------------------------------------------- compression
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_compress(gpu_ctx, cid):
    r = P.CURVES[cid].r
    pool = _pool(cid)
    rng = random.Random(0x500 + cid)
    nmax = (1 << 11) + 1
    cols = [pool[k * nmax:(k + 1) * nmax] for k in range(4)] + [[r - 1] * nmax]
    dcols = [_dev(gpu_ctx, _arr(r, c)) for c in cols]
    thetas = [0, 1, r - 1, rng.randrange(r)]
    for n in (1, 255, 256, 257, nmax):
        for m in (1, 2, 5):
            for theta in thetas if n in (257, nmax) else thetas[-1:]:
                out = _dev(gpu_ctx, np.full((n + 1, 4), SENT, dtype=np.uint64))
                gpu_ctx.lookup_compress_device(cid, [t.data_ptr() for t in dcols[:m]], n, _arr(r, [theta])[0],
                                               out.data_ptr())
                got = _host(out)
                assert np.array_equal(got[:n], _arr(r, L.compress([c[:n] for c in cols[:m]], theta, r))), (n, m, theta)
                assert (got[n] == SENT).all()
        # one column: the column itself, and theta is not read
        out = _dev(gpu_ctx, np.zeros((n, 4), dtype=np.uint64))
        gpu_ctx.lookup_compress_device(cid, [dcols[0].data_ptr()], n, None, out.data_ptr())
        assert np.array_equal(_host(out), _arr(r, cols[0][:n]))
    # all r - 1 columns, and the output on one of the columns
    top = [_dev(gpu_ctx, _arr(r, [r - 1] * 300)) for _ in range(3)]
    want = _arr(r, L.compress([[r - 1] * 300] * 3, r - 1, r))
    gpu_ctx.lookup_compress_device(cid, [t.data_ptr() for t in top], 300, _arr(r, [r - 1])[0], top[1].data_ptr())
    assert np.array_equal(_host(top[1]), want)
    assert np.array_equal(_host(top[0]), _arr(r, [r - 1] * 300))


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("cid", [0, 1, 2])
@pytest.mark.parametrize("usable", [T + 1, (1 << 12) - 5])
def test_lookup_grand_product_closes(gpu_ctx, cid, usable):
    """Independent of the restatement: two-column inputs drawn from a
    two-column table, compressed with a random theta, permuted, and the lookup
    grand product (A + beta)(S + gamma) / ((A' + beta)(S' + gamma)) over the
    usable rows must end at 1."""
    import torch

    r = P.CURVES[cid].r
    pool = _pool(cid)
    rng = random.Random(0x600 + cid + usable)
    n = usable + 6
    t0, t1 = pool[:n], pool[n:2 * n]
    # input rows are table rows 1 .. usable / 3 (with repeats); table row 0 is unique in the table
    # and is taken by the repeated input rows 0 and 1 alone
    pick = [0, 0] + [1 + rng.randrange(usable // 3) for _ in range(n - 2)]
    i0, i1 = [t0[j] for j in pick], [t1[j] for j in pick]
    one = _arr(r, [1])[0]
    theta, beta, gamma = (_arr(r, [rng.randrange(r)])[0] for _ in range(3))

    def run(table0):
        d = [_dev(gpu_ctx, _arr(r, c)) for c in (i0, i1, table0, t1)]
        A, S, Ap, Sp, Z = (torch.zeros((n, 4), dtype=torch.int64, device=d[0].device) for _ in range(5))
        gpu_ctx.lookup_compress_device(cid, [d[0].data_ptr(), d[1].data_ptr()], n, theta, A.data_ptr())
        gpu_ctx.lookup_compress_device(cid, [d[2].data_ptr(), d[3].data_ptr()], n, theta, S.data_ptr())
        st = gpu_ctx.lookup_permute_device(cid, [A.data_ptr()], [S.data_ptr()], n, usable, [Ap.data_ptr()],
                                           [Sp.data_ptr()])
        if st[0, 0]:
            return st, None
        sets = [([(0, None, None, beta), (1, None, None, gamma)], [(2, None, None, beta), (3, None, None, gamma)])]
        last = gpu_ctx.grand_product_device(cid, [t.data_ptr() for t in (A, S, Ap, Sp)], n, sets, None, one,
                                            usable + 1, Z.data_ptr())
        return st, last

    st, last = run(t0)
    assert tuple(st[0]) == (0, 0)
    assert np.array_equal(last[0], one)
    # table row 0 replaced: the repeated input rows 0 and 1 lose their only match
    st, _ = run([pool[2 * n]] + t0[1:])
    assert st[0, 0] == 1


def test_two_to_18_plus_7(gpu_ctx):
    u = (1 << 18) + 7
    r = P.CURVES[2].r
    rng = random.Random(0x700)
    distinct = [rng.randrange(r) for _ in range(u // 2)]
    s = [distinct[i % len(distinct)] for i in range(u)]
    a = [distinct[rng.randrange(len(distinct) // 2)] for _ in range(u)]
    _check(gpu_ctx, 2, a, s, u, extra=6, tag="2^18 + 7")

"""GPU tests of the grand products (pm_grand_product_device) and the batch
inversion (pm_batch_invert*) against tests/gp_ref.py: bit-identical rows and
`last` at every run and tile boundary (runs of 8 rows, tiles of 2^11), zeros at
every position that matters, chaining, and the permutation argument's
end-to-end property.

Products are not linear in the stored words, so values are plain integers mod r
converted with poly_ref.mont / to_array.  A canonical output is unique, so
where a test multiplies back (got * a == 1, got < r) instead of comparing
against gp_ref.batch_invert it checks the same bits without r-sized pows."""
import functools
import random

import numpy as np
import pytest

import gp_ref as G
import halo2_amd as H
import pasta as P
import poly_ref as R

pytestmark = pytest.mark.gpu

TILE = 1 << 11
POOL_N = (1 << 13) + 1


def _dev(gpu_ctx, arr):
    import torch

    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(torch.device("cuda", gpu_ctx.device))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _scalar(r, v):
    return np.array(R.mont(r, v), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _pool(cid):
    """seven random columns of POOL_N rows, drawn once per field: (integers,
    Montgomery arrays); the length sweeps take prefixes"""
    r = P.CURVES[cid].r
    rng = random.Random(0x6B0 + cid)
    cols = [[rng.randrange(r) for _ in range(POOL_N)] for _ in range(7)]
    return cols, [R.to_array(r, c) for c in cols]


@functools.lru_cache(maxsize=None)
def _inverses(cid):
    """gp_ref.batch_invert of the pool's first column with zeros, 1 and r - 1
    planted at the run and tile edges (computed once; prefixes are shared)"""
    r = P.CURVES[cid].r
    vals = list(_pool(cid)[0][0])
    for i in (0, 7, 8, 129, 2047, 2048):
        vals[i] = 0
    vals[1], vals[2] = 1, r - 1
    return vals, G.batch_invert(vals, r)


# ---------------------------------------------------------------- batch inversion
@pytest.mark.parametrize("cid", [0, 1, 2])
def test_batch_invert_host_every_length(gpu_ctx, cid):
    r = P.CURVES[cid].r
    vals, inv = _inverses(cid)
    arr, want = R.to_array(r, vals[:130]), R.to_array(r, inv[:130])
    for n in range(1, 131):
        got = gpu_ctx.batch_invert(cid, arr[:n])
        assert got.shape == (n, 4)
        assert np.array_equal(got, want[:n]), n


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_batch_invert_device_boundaries(gpu_ctx, cid):
    import torch

    r = P.CURVES[cid].r
    vals, inv = _inverses(cid)
    arr, want = R.to_array(r, vals), R.to_array(r, inv)
    for n in [(1 << k) + d for k in range(8, 14) for d in (-1, 0, 1)]:
        # n values and a sentinel row behind them
        t = _dev(gpu_ctx, np.concatenate([arr[:n], np.full((1, 4), 2**64 - 1, dtype=np.uint64)]))
        # a zero in the last row too
        t[n - 1] = 0
        torch.cuda.synchronize()
        gpu_ctx.batch_invert_device(cid, t.data_ptr(), n)
        got = _host(t)
        assert np.array_equal(got[:n - 1], want[:n - 1]), n
        assert not got[n - 1].any(), n
        assert (got[n] == 2**64 - 1).all(), n
    # all zero, and all r - 1 (its own inverse)
    z = _dev(gpu_ctx, np.zeros((300, 4), dtype=np.uint64))
    gpu_ctx.batch_invert_device(cid, z.data_ptr(), 300)
    assert not _host(z).any()
    top = R.to_array(r, [r - 1] * 300)
    t = _dev(gpu_ctx, top)
    gpu_ctx.batch_invert_device(cid, t.data_ptr(), 300)
    assert np.array_equal(_host(t), top)


def _check_inverse_by_product(r, before, after):
    a, b = R.raw_ints(before), R.raw_ints(after)
    rr = P.R_MONT * P.R_MONT % r  # (a R)(b R) == R^2  <=>  a b == 1
    for x, y in zip(a, b):
        assert y < r
        assert (x * y - rr) % r == 0 if x else y == 0


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_batch_invert_device_two_to_16_plus_1(gpu_ctx, cid):
    import torch

    n = (1 << 16) + 1
    t = torch.empty((n, 4), dtype=torch.int64, device=torch.device("cuda", gpu_ctx.device))
    gpu_ctx.synth_scalars(cid, 0x1D, 0, n, t.data_ptr())
    t[5] = 0
    t[n - 1] = 0
    torch.cuda.synchronize()
    before = _host(t).copy()
    gpu_ctx.batch_invert_device(cid, t.data_ptr(), n)
    _check_inverse_by_product(P.CURVES[cid].r, before, _host(t))


# ---------------------------------------------------------------- grand products
def _factor_args(r, factors):
    out = []
    for x, y, b, g in factors:
        out.append((x, H.GP_OMEGA if y == G.OMEGA else y, _scalar(r, b), _scalar(r, g)))
    return out


def _run(gpu_ctx, cid, d_cols, n, sets, omega, start, active, chain=False, want_last=True):
    """Runs the device entry over the integer factor lists of gp_ref and
    returns (rows (S, n, 4) with the sentinel behind `active`, last)."""
    import torch

    r = P.CURVES[cid].r
    out = torch.full((len(sets) * n, 4), -1, dtype=torch.int64, device=torch.device("cuda", gpu_ctx.device))
    torch.cuda.synchronize()
    last = gpu_ctx.grand_product_device(cid, [t.data_ptr() for t in d_cols], n,
                                        [(_factor_args(r, nu), _factor_args(r, de)) for nu, de in sets],
                                        None if omega is None else _scalar(r, omega), _scalar(r, start), active,
                                        out.data_ptr(), chain=chain, want_last=want_last)
    return _host(out).reshape(len(sets), n, 4), last


def _check(gpu_ctx, cid, cols, d_cols, n, sets, omega, start, active, chain=False, fn=G.grand_product_fast):
    r = P.CURVES[cid].r
    rows, last = _run(gpu_ctx, cid, d_cols, n, sets, omega, start, active, chain)
    zs, lasts = G.grand_products(cols, sets, n, active, start, omega, r, chain=chain, fn=fn)
    for j, z in enumerate(zs):
        assert np.array_equal(rows[j, :active], R.to_array(r, z)), (cid, n, active, j)
        assert (rows[j, active:] == 2**64 - 1).all(), (cid, n, active, j)  # the caller's rows
    assert np.array_equal(last, R.to_array(r, lasts)), (cid, n, active)
    return zs, lasts


def _two_shapes(rng, r):
    """a lookup-shaped set over columns 0..3 and a permutation chunk over the
    value columns 0..2 with the sigma columns 4..6"""
    beta, gamma, delta = rng.randrange(r), rng.randrange(r), 7
    return [G.lookup_set(0, 1, 2, 3, beta, gamma),
            G.permutation_sets([0, 1, 2], [4, 5, 6], 3, beta, gamma, delta, r)[0]]


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_every_boundary(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(700 + cid)
    cols, arrs = _pool(cid)
    d_full = [_dev(gpu_ctx, a) for a in arrs]
    sets, omega = _two_shapes(rng, r), rng.randrange(r)
    lengths = list(range(1, 41)) + [TILE + d for d in (-1, 0, 1)] + [2 * TILE + d for d in (-1, 0, 1)]
    for n in lengths:
        d_cols = [t[:n] for t in d_full]  # prefixes: the same device memory
        for active in sorted({a for a in (1, 2, n - 5, n) if 1 <= a <= n}):
            _check(gpu_ctx, cid, cols, d_cols, n, sets, omega, rng.randrange(r), active,
                   fn=G.grand_product_literal if n <= 40 else G.grand_product_fast)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_zero_denominators_and_odd_lists(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(800 + cid)
    n, active = 2 * TILE + 104, 2 * TILE + 94
    base = [c[:n] for c in _pool(cid)[0][:4]]
    num, den = G.lookup_set(0, 1, 2, 3, rng.randrange(r), rng.randrange(r))
    beta = den[0][3]

    def case(zero_rows, sets, num_zero=None, start=None):
        cols = [list(c) for c in base]
        for i in zero_rows:
            cols[2][i] = -beta % r  # A'[i] + beta == 0
        if num_zero is not None:
            cols[0][num_zero] = -num[0][3] % r
        d_cols = [_dev(gpu_ctx, R.to_array(r, c)) for c in cols]
        return _check(gpu_ctx, cid, cols, d_cols, n, sets, rng.randrange(r), start or rng.randrange(1, r), active)

    both = [(num, den)]
    _, clean = case([], both)
    assert clean[0] != 0
    for rows in ([0], [TILE - 1], [TILE], [active - 2], [5, TILE - 1, active - 2]):
        zs, lasts = case(rows, both)
        assert lasts == [0] and zs[0][rows[0]] != 0 and not any(zs[0][rows[0] + 1:])
    # a zero denominator in a row that enters no output has no effect
    for rows in ([active - 1], [n - 1], [active - 1, active, n - 1]):
        zs, lasts = case(rows, both, start=3)
        assert lasts[0] != 0
    assert case([active - 1], both, start=3) == case([], both, start=3)
    # a zero numerator: zero from the next row on, without any special case
    zs, lasts = case([], both, num_zero=TILE + 3)
    assert lasts == [0] and zs[0][TILE + 3] != 0 and not any(zs[0][TILE + 4:])
    # empty lists, x absent (y b + g), both absent (the constant g), one column
    # in both roles, all in one call of independent sets
    odd = [([], den), (num, []), ([], []),
           ([(None, 1, rng.randrange(r), rng.randrange(r))], [(None, None, 0, rng.randrange(1, r))]),
           ([(2, 2, rng.randrange(r), 0)], [(None, G.OMEGA, rng.randrange(r), rng.randrange(r))])]
    case([], odd)
    case([9], odd)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_out_last_may_be_null(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(850 + cid)
    n = 300
    cols = [c[:n] for c in _pool(cid)[0]]
    d_cols = [_dev(gpu_ctx, a[:n]) for a in _pool(cid)[1]]
    sets, omega = _two_shapes(rng, r), rng.randrange(r)
    rows, last = _run(gpu_ctx, cid, d_cols, n, sets, omega, 5, n - 5, want_last=False)
    assert last is None
    zs, _ = G.grand_products(cols, sets, n, n - 5, 5, omega, r)
    for j, z in enumerate(zs):
        assert np.array_equal(rows[j, :n - 5], R.to_array(r, z))


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_chained_against_unchained(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(900 + cid)
    n, active = 300, 295
    cols = [c[:n] for c in _pool(cid)[0]]
    d_cols = [_dev(gpu_ctx, a[:n]) for a in _pool(cid)[1]]
    sets = _two_shapes(rng, r) + [G.lookup_set(3, 4, 5, 6, rng.randrange(r), rng.randrange(r))]
    omega, start = rng.randrange(r), rng.randrange(1, r)
    free_z, free_last = _check(gpu_ctx, cid, cols, d_cols, n, sets, omega, start, active, chain=False)
    zs, lasts = _check(gpu_ctx, cid, cols, d_cols, n, sets, omega, start, active, chain=True)
    assert zs[0] == free_z[0] and zs[1] != free_z[1]
    inv_start = pow(start, r - 2, r)
    for j in (1, 2):  # chained = unchained scaled by the previous last / start
        assert zs[j] == [v * lasts[j - 1] % r * inv_start % r for v in free_z[j]]
    # a zero denominator in the middle set zeroes everything chained behind it
    cols2 = [list(c) for c in cols]
    cols2[4][17] = (-sets[1][1][0][3] - cols2[0][17]) * pow(sets[1][1][0][2], r - 2, r) % r
    d2 = [_dev(gpu_ctx, R.to_array(r, c)) for c in cols2]
    zs, lasts = _check(gpu_ctx, cid, cols2, d2, n, sets, omega, start, active, chain=True)
    assert lasts[0] != 0 and lasts[1:] == [0, 0] and not any(zs[2])


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_permutation_end_to_end(gpu_ctx, cid):
    """4 columns in 2 chained chunks over a genuine permutation of the cells
    of rows [0, n - 1): every row equals the reference and the last chunk
    ends at 1."""
    r = P.CURVES[cid].r
    n = 1 << 12
    cols, vals, sigmas, omega, delta = G.permutation_instance(r, 4, n, 77 + cid, fixed_rows=(n - 1,))
    assert pow(omega, n, r) == 1 and pow(omega, n // 2, r) != 1
    rng = random.Random(950 + cid)
    beta, gamma = rng.randrange(r), rng.randrange(r)
    sets = G.permutation_sets(vals, sigmas, 2, beta, gamma, delta, r)
    assert len(sets) == 2
    d_cols = [_dev(gpu_ctx, R.to_array(r, c)) for c in cols]
    _, lasts = _check(gpu_ctx, cid, cols, d_cols, n, sets, omega, 1, n, chain=True)
    assert lasts[0] not in (0, 1) and lasts[1] == 1


def test_long_case(gpu_ctx):
    import torch

    cid, n = H.BN254, (1 << 18) + 7
    r = P.CURVES[cid].r
    rng = random.Random(18)
    d = [torch.empty((n, 4), dtype=torch.int64, device=torch.device("cuda", gpu_ctx.device)) for _ in range(2)]
    for i, t in enumerate(d):
        gpu_ctx.synth_scalars(cid, 0x60 + i, 0, n, t.data_ptr())
    torch.cuda.synchronize()
    cols = [R.from_array(r, _host(t)) for t in d]
    sets = [([(0, G.OMEGA, rng.randrange(r), rng.randrange(r))], [(0, 1, rng.randrange(r), rng.randrange(r))])]
    omega, start, active = rng.randrange(r), rng.randrange(1, r), n - 6
    rows, last = _run(gpu_ctx, cid, d, n, sets, omega, start, active)
    z, want_last = G.grand_product_fast(cols, sets[0][0], sets[0][1], n, active, start, omega, r)
    assert want_last != 0
    assert R.from_array(r, rows[0, :active]) == z
    assert max(R.raw_ints(rows[0, :active])) < r  # canonical
    assert (rows[0, active:] == 2**64 - 1).all()
    assert R.from_array(r, last) == [want_last]
    before = _host(d[0]).copy()
    gpu_ctx.batch_invert_device(cid, d[0].data_ptr(), n)
    _check_inverse_by_product(r, before, _host(d[0]))


def test_argument_errors_on_a_live_context(gpu_ctx):
    """what the wrappers cannot see: the library's own checks"""
    L = H.lib()
    cid = H.BN254
    d = _dev(gpu_ctx, np.zeros((8, 4), dtype=np.uint64))
    out = _dev(gpu_ctx, np.zeros((8, 4), dtype=np.uint64))
    ptrs = (H._vp * 1)(d.data_ptr())
    fac = (H.PmGpFactor * 2)()
    fac[0].x, fac[0].y = 0, H.GP_NONE
    fac[1].x, fac[1].y = 0, H.GP_NONE
    one = np.zeros(4, dtype=np.uint64)
    p32 = lambda a: a.ctypes.data_as(H._u32p)  # noqa: E731

    def call(offs_n, offs_d, active=8, flags=0, omega=None, C=1, S=1):
        a, b = np.array(offs_n, np.uint32), np.array(offs_d, np.uint32)
        return L.pm_grand_product_device(gpu_ctx.h, cid, ptrs, C, 8, fac, p32(a), fac, p32(b), S, omega, H._p(one),
                                         active, flags, H._vp(out.data_ptr()), None)

    assert call([0, 1], [0, 1]) == 0
    assert call([1, 1], [0, 1]) == -1 and b"offsets" in L.pm_last_error()
    assert call([0, 2, 1], [0, 1, 1], S=2) == -1 and b"decrease" in L.pm_last_error()
    assert call([0, 1], [0, 1], S=0) == -1
    assert call([0, 1], [0, 17]) == -1 and b"PM_GP_MAX_FACTORS" in L.pm_last_error()
    assert call([0, 1], [0, 1], active=0) == -1 and b"active" in L.pm_last_error()
    assert call([0, 1], [0, 1], active=9) == -1
    assert call([0, 1], [0, 1], flags=2) == -1
    assert call([0, 1], [0, 1], C=0) == -1 and b"index" in L.pm_last_error()
    fac[1].y = H.GP_OMEGA
    assert call([0, 1], [0, 2]) == -1 and b"omega" in L.pm_last_error()
    fac[1].y = H.GP_NONE
    assert call([0, 2], [0, 2]) == 0  # the context still computes

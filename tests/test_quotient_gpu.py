"""GPU tests of the quotient numerator (pm_quotient_create / pm_quotient_device,
k_quot_eval), bit for bit against tests/quotient_ref.py on every extended row
unless a test says otherwise.  The kernel is not linear in its data, so the
device columns hold true Montgomery words."""
import ctypes
import functools
import random

import numpy as np
import pytest

import accum as A
import halo2_amd as H
import pasta as P
import poly_ref as R
import quotient_ref as Q
import shape_util as S

pytestmark = pytest.mark.gpu
PM_ERR_ARG = -1
SENTINEL = 0x5A5A5A5A5A5A5A5A
PAD = 4  # sentinel rows behind the output
RANDOM_SEED = 0x0E5  # the seed of tests/test_quotient_host.py: the same 40 shapes per field
CURVES = [0, 1, 2]


def gpu_domain(ctx, cid, d):
    return ctx.domain(cid, d.k, d.extended_k, np.array(R.mont(d.r, d.extended_omega), np.uint64),
                      np.array(R.mont(d.r, d.zeta), np.uint64))


def to_dev(ctx, arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(torch.device("cuda", ctx.device))


def dev_columns(ctx, r, cols):
    """integer columns -> ({group: [tensor]}, {group: [pointer]})"""
    t = {g: [to_dev(ctx, a) for a in arrs] for g, arrs in Q.mont_columns(r, cols).items()}
    return t, {g: [x.data_ptr() for x in ts] for g, ts in t.items()}


def out_buffer(ctx, N, start=None):
    arr = np.full((N + PAD, 4), SENTINEL, dtype=np.uint64)
    if start is not None:
        arr[:N] = start
    return to_dev(ctx, arr)


def words(t, N):
    """the N output rows as stored; the sentinel rows behind them must be intact"""
    import torch

    torch.cuda.synchronize()
    arr = t.cpu().numpy().view(np.uint64)
    assert (arr[N:] == np.uint64(SENTINEL)).all(), "rows behind the output were written"
    return arr[:N]


def run(ctx, q, ptrs, r, ch4, N, **kw):
    out = out_buffer(ctx, N)
    ctx.quotient_device(q, ptrs, Q.challenges_array(r, ch4), out.data_ptr(), **kw)
    return words(out, N)


def challenges(rng, r):
    return [rng.randrange(r) for _ in range(4)]


def assert_rows(got, r, want, rows=None):
    rows = range(len(want)) if rows is None else rows
    w = R.to_array(r, want)
    bad = [j for i, j in enumerate(rows) if not np.array_equal(got[j], w[i])]
    assert not bad, bad[:8]


class Case:
    """one (curve, shape, k, e) on the device with random columns and its reference"""

    def __init__(self, ctx, cid, sh, k, e, seed, cols=None, rows=None):
        self.C = P.CURVES[cid]
        self.r = self.C.r
        self.dom = Q.domain_for(cid, k, e)
        self.sh = Q.on_domain(sh, self.dom)
        self.N = self.dom.N
        self.cols = Q.random_columns(self.sh, self.N, self.r, seed) if cols is None else cols
        self.ch = challenges(random.Random(seed ^ 0xC4A), self.r)
        self.gdom = gpu_domain(ctx, cid, self.dom)
        self.q = ctx.quotient(self.gdom, Q.product_shape(cid, self.sh))
        self.t, self.ptrs = dev_columns(ctx, self.r, self.cols)
        self.rows = rows

    def want(self, ch=None, start=None):
        return Q.numerator(self.C, self.sh, self.dom, self.cols, ch or self.ch, self.rows, start)

    def release(self):
        self.q.release()
        self.gdom.release()


@functools.lru_cache(maxsize=None)
def oracle_shape(cid, name, k):
    C = P.CURVES[cid]
    return A.synth_vk_points(C, (A.simple_example_shape if name == "simple" else A.rich_shape)(C, k))


@pytest.mark.parametrize("cid", CURVES)
def test_random_shapes(gpu_ctx, cid):
    """40 seeded shapes per field, k = 2 .. 8 with e cycling 0 .. 3: N below a
    wave (N = 4 at k = 2, e = 0) up to 32 blocks, rotations -3 .. 3 and the
    `last` rotation -(bf + 1), so every row wraps somewhere."""
    shapes, _ = S.random_shapes(cid, 40, RANDOM_SEED + cid)
    seen = set()
    for i, sh in enumerate(shapes):
        c = Case(gpu_ctx, cid, sh, sh.log_n, i % 4, 3000 + 50 * cid + i)
        info = c.q.info()
        assert info["n_expressions"] == len(sh.gates) + (2 * sh.n_perm_sets + 1 if sh.n_perm_sets else 0) + \
            5 * sh.num_lookups
        assert 1 <= info["slots"] <= 28 and info["loads_per_row"] >= 1
        assert_rows(run(gpu_ctx, c.q, c.ptrs, c.r, c.ch, c.N), c.r, c.want())
        seen.add(c.N)
        c.release()
    assert min(seen) <= 16 and max(seen) >= 512


@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("name", ["simple", "rich"])
def test_oracle_shapes(gpu_ctx, cid, name):
    c = Case(gpu_ctx, cid, oracle_shape(cid, name, 10), 10, 2, 77 + cid)
    got = run(gpu_ctx, c.q, c.ptrs, c.r, c.ch, c.N)
    assert_rows(got, c.r, c.want())
    info = c.q.info()
    assert info["device_bytes"] >= 4 * c.N * 32  # l_0, l_last, l_last + l_blind and X on the coset
    c.release()


def test_many_blocks(gpu_ctx):
    """BN254 simple shape at k = 13, e = 2 (512 blocks): the first and last 64
    rows and 256 seeded rows."""
    cid, k, e = 2, 13, 2
    N = 1 << (k + e)
    rng = random.Random(0xB10C)
    rows = sorted(set(list(range(64)) + list(range(N - 64, N)) + [rng.randrange(N) for _ in range(256)]))
    c = Case(gpu_ctx, cid, oracle_shape(cid, "simple", k), k, e, 1313, rows=rows)
    got = run(gpu_ctx, c.q, c.ptrs, c.r, c.ch, c.N)
    assert_rows(got, c.r, c.want(), rows)
    c.release()


@pytest.mark.parametrize("cid", CURVES)
def test_flags(gpu_ctx, cid):
    """DIVIDE_VANISHING equals the plain call followed by
    pm_divide_by_vanishing_device; ACCUMULATE over two calls (two shapes, one
    y) equals the reference folded across both expression lists; both flags
    together.  Every input column is unchanged after the calls."""
    k, e = 5, 2
    a = Case(gpu_ctx, cid, oracle_shape(cid, "simple", k), k, e, 500 + cid)
    b = Case(gpu_ctx, cid, oracle_shape(cid, "rich", k), k, e, 600 + cid)
    N, r = a.N, a.r
    chb = b.ch[:3] + [a.ch[3]]
    before = {g: [x.clone() for x in ts] for g, ts in b.t.items()}
    plain = run(gpu_ctx, a.q, a.ptrs, r, a.ch, N)
    wa = a.want()
    assert_rows(plain, r, wa)
    # divide: against the two-call form on the device, and against the reference
    fused = run(gpu_ctx, a.q, a.ptrs, r, a.ch, N, divide_vanishing=True)
    two = out_buffer(gpu_ctx, N, plain)
    gpu_ctx.divide_by_vanishing_device(a.gdom, [two.data_ptr()])
    assert np.array_equal(fused, words(two, N))
    t = a.dom.t_evaluations
    assert_rows(fused, r, [v * t[j % len(t)] % r for j, v in enumerate(wa)])
    # accumulate: b's expressions folded onto a's result
    wab = b.want(chb, start=wa)
    acc = out_buffer(gpu_ctx, N, plain)
    gpu_ctx.quotient_device(b.q, b.ptrs, Q.challenges_array(r, chb), acc.data_ptr(), accumulate=True)
    assert_rows(words(acc, N), r, wab)
    both = out_buffer(gpu_ctx, N, plain)
    gpu_ctx.quotient_device(b.q, b.ptrs, Q.challenges_array(r, chb), both.data_ptr(), accumulate=True,
                            divide_vanishing=True)
    assert_rows(words(both, N), r, [v * t[j % len(t)] % r for j, v in enumerate(wab)])
    import torch

    for g, ts in b.t.items():
        for x, y in zip(ts, before[g]):
            assert torch.equal(x, y), g
    a.release()
    b.release()


@pytest.mark.parametrize("cid", CURVES)
def test_adversarial_data(gpu_ctx, cid):
    """All-zero columns; all r - 1; Z = 1 with A' = S' (the lookup identities
    vanish row by row); beta = gamma = 0; theta = y = 0 and r - 1."""
    k, e = 4, 2
    sh = oracle_shape(cid, "rich", k)
    r = P.CURVES[cid].r
    N = 1 << (k + e)
    rng = random.Random(0xAD + cid)
    datasets = {"zero": Q.constant_columns(sh, N, 0), "r-1": Q.constant_columns(sh, N, r - 1)}
    z1 = Q.random_columns(sh, N, r, 0xAD5 + cid)
    z1["lookup_z"] = [[1] * N for _ in z1["lookup_z"]]
    z1["lookup_s"] = [list(a) for a in z1["lookup_a"]]
    datasets["z=1,a=s"] = z1
    for name, cols in datasets.items():
        c = Case(gpu_ctx, cid, sh, k, e, 900 + cid, cols=cols)
        for ch in (c.ch, [c.ch[0], 0, 0, c.ch[3]], [0, c.ch[1], c.ch[2], 0], [r - 1] * 4, [1, 1, 1, 1],
                   [rng.randrange(r), r - 1, 0, 1]):
            assert_rows(run(gpu_ctx, c.q, c.ptrs, c.r, ch, N), r, c.want(ch))
        c.release()


def test_lookup_identities_vanish_with_z_one_and_equal_permuted_columns(gpu_ctx):
    """lookups only: with Z = 1 and A' = S', e1, e2, e4 and e5 are zero on every
    row and e3 is (A' + beta)(S' + gamma) - (compressed input + beta)(compressed
    table + gamma); with the table equal to the input too the row is zero."""
    cid, k, e = 2, 4, 1
    sh = S.build(cid, log_n=k, na=1, nl=1, gates=[], lk_in=[A.Advice(0)], lk_tab=[A.Advice(0)])
    r = P.CURVES[cid].r
    N = 1 << (k + e)
    cols = Q.random_columns(sh, N, r, 0x2E0)
    cols["lookup_z"] = [[1] * N]
    cols["lookup_a"] = [list(cols["advice"][0])]
    cols["lookup_s"] = [list(cols["advice"][0])]
    c = Case(gpu_ctx, cid, sh, k, e, 0x2E1, cols=cols)
    got = run(gpu_ctx, c.q, c.ptrs, c.r, c.ch, N)
    assert not got.any()
    assert c.want() == [0] * N
    c.release()


def horner(coeffs, x, r):
    return R.eval_polynomial(coeffs, x, r)


@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("name", ["simple", "rich"])
def test_polynomial_meaning(gpu_ctx, cid, name):
    """Independent of the pointwise restatement: columns are random coefficient
    vectors of length n pushed through pm_coeff_to_extended_device, the kernel's
    output goes through pm_extended_to_coeff_device (keep = N), and Horner at a
    random x must equal the scalar_block fold at x with evaluations from Horner
    of the same vectors at omega^rot x.  k = 6, e = 3: every identity has degree
    at most 5 (n - 1) < N.  Pins X_j, the rotation direction and the l_i
    columns to the polynomial meaning."""
    k, e = 6, 3
    C = P.CURVES[cid]
    r = C.r
    dom = Q.domain_for(cid, k, e)
    sh = Q.on_domain(oracle_shape(cid, name, k), dom)
    n, N = dom.n, dom.N
    rng = random.Random(0x901 + cid)
    coeffs = {g: [[rng.randrange(r) for _ in range(n)] for _ in range(cnt)] for g, cnt in Q.counts(sh).items()}
    gdom = gpu_domain(gpu_ctx, cid, dom)
    q = gpu_ctx.quotient(gdom, Q.product_shape(cid, sh))
    bufs = {g: [to_dev(gpu_ctx, np.concatenate([R.to_array(r, c), np.zeros((N - n, 4), dtype=np.uint64)]))
                for c in cs] for g, cs in coeffs.items()}
    flat = [t.data_ptr() for ts in bufs.values() for t in ts]
    gpu_ctx.coeff_to_extended_device(gdom, flat, flat)
    ch = challenges(rng, r)
    out = out_buffer(gpu_ctx, N)
    gpu_ctx.quotient_device(q, {g: [t.data_ptr() for t in ts] for g, ts in bufs.items()}, Q.challenges_array(r, ch),
                            out.data_ptr())
    gpu_ctx.extended_to_coeff_device(gdom, [out.data_ptr()], [out.data_ptr()], N)
    h = R.from_array(r, words(out, N))
    assert any(h[n:])  # a product of columns: the coefficients past n are in use
    for _ in range(2):
        x = rng.randrange(r)
        d = Q.evals_from(sh, lambda g, c, rot: horner(coeffs[g][c], pow(dom.omega, rot, r) * x % r, r))
        want = Q.fold(Q.expressions(C, sh, d, ch, x), ch[3], r)
        assert horner(h, x, r) == want
    q.release()
    gdom.release()


def test_two_shapes_alternate_on_one_context(gpu_ctx):
    """No stale program, pointer table or constants: two quotients of
    different shapes and domains take turns, each with new challenges."""
    cid = 2
    a = Case(gpu_ctx, cid, oracle_shape(cid, "simple", 4), 4, 2, 41)
    b = Case(gpu_ctx, cid, S.shape(cid, "mixed"), 5, 1, 42)
    rng = random.Random(43)
    for _ in range(2):
        for c in (a, b):
            ch = challenges(rng, c.r)
            assert_rows(run(gpu_ctx, c.q, c.ptrs, c.r, ch, c.N), c.r, c.want(ch))
    a.release()
    b.release()


@pytest.mark.parametrize("cid", CURVES)
def test_leaf_residency_variants(gpu_ctx, cid, monkeypatch):
    """The two forms of the compiled program (PM_QUOT_CACHE_SLOTS, read when a
    quotient is created): every use of a leaf loads it, or a repeated leaf keeps
    its slot until its last use.  Fewer loads, more slots, the same rows."""
    k, e = 5, 3
    infos = {}
    for slots in ("0", "28"):
        monkeypatch.setenv("PM_QUOT_CACHE_SLOTS", slots)
        c = Case(gpu_ctx, cid, oracle_shape(cid, "rich", k), k, e, 700 + cid)
        monkeypatch.delenv("PM_QUOT_CACHE_SLOTS")
        infos[slots] = c.q.info()
        assert_rows(run(gpu_ctx, c.q, c.ptrs, c.r, c.ch, c.N), c.r, c.want())
        c.release()
    assert infos["28"]["loads_per_row"] < infos["0"]["loads_per_row"]
    assert infos["0"]["slots"] < infos["28"]["slots"] <= 28
    assert infos["0"]["products_per_row"] == infos["28"]["products_per_row"]


def test_mismatched_domain_is_an_argument_error(gpu_ctx):
    cid, k = 2, 4
    r = P.CURVES[cid].r
    dom = Q.domain_for(cid, k, 2)
    gdom = gpu_domain(gpu_ctx, cid, dom)
    sh = oracle_shape(cid, "simple", k)
    other = A.domain_omega(r, k)
    other = other if other != dom.omega else pow(other, 3, r)
    bad = Q.product_shape(cid, Q.on_domain(sh, dom))
    bad.c.omega[:] = H._mont_limbs(other, r)
    with pytest.raises(H.PmError, match="pm error -1.*omega"):
        gpu_ctx.quotient(gdom, bad)
    h = H._vp()
    short = Q.product_shape(cid, oracle_shape(cid, "simple", k + 1))
    assert H.lib().pm_quotient_create(gpu_ctx.h, gdom.h, short.c, ctypes.byref(h)) == PM_ERR_ARG  # shape.log_n != k
    assert b"log_n" in H.lib().pm_last_error()
    q = gpu_ctx.quotient(gdom, Q.product_shape(cid, Q.on_domain(sh, dom)))
    cols = H.PmQuotientColumns()
    ch = np.zeros(16, dtype=np.uint64)
    assert H.lib().pm_quotient_device(gpu_ctx.h, q.h, cols, H._p(ch), 4, H._vp(0x1000)) == PM_ERR_ARG  # flag bits
    assert b"flag" in H.lib().pm_last_error()
    assert H.lib().pm_quotient_device(gpu_ctx.h, q.h, cols, H._p(ch), 0, H._vp(0x1000)) == PM_ERR_ARG
    assert b"null column" in H.lib().pm_last_error()
    if H.device_count() > 1:  # a quotient of another device
        ctx1 = H.Context(1)
        d = {g: [0x1000] * n for g, n in q.counts.items()}
        with pytest.raises(H.PmError, match="pm error -1.*another device"):
            ctx1.quotient_device(q, d, ch, 0x2000)
        with pytest.raises(H.PmError, match="pm error -1.*another device"):
            ctx1.quotient(gdom, Q.product_shape(cid, Q.on_domain(sh, dom)))
        ctx1.close()
    q.release()
    gdom.release()

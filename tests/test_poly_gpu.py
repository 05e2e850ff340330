"""GPU tests of the polynomial openings (pm_poly_eval*, pm_multiopen_*,
pm_eval_polynomial, pm_kate_division) against tests/poly_ref.py: bit-identical
quotients and evaluations at every tile boundary, adversarial values, the
division identity at 2^20 / 2^22, and the opening relation the verifier's
(w, zw, f, e) encode, checked with an SRS of known discrete log.

Division and the batch are linear in the coefficients, so the tests that only
compare against the restatement draw the stored (Montgomery) words at random
and run the reference on them with plain z and v (poly_ref.py)."""
import functools
import random

import numpy as np
import pytest

import halo2_amd as H
import pasta as P
import poly_ref as R

pytestmark = pytest.mark.gpu

# every n up to 130 (host wrappers), then the tile boundaries (runs of 8,
# tiles of 2^11 / 2^12) around every power of two up to 2^16, and 2^18 + 7
SMALL = list(range(1, 131))
LARGE = [(1 << k) + d for k in range(8, 17) for d in (-1, 0, 1)] + [(1 << 18) + 7]


def _dev(gpu_ctx, arr):
    import torch

    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(torch.device("cuda", gpu_ctx.device))


def _empty(gpu_ctx, rows):
    import torch

    return torch.empty((rows, 4), dtype=torch.int64, device=torch.device("cuda", gpu_ctx.device))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _scalar(r, v):
    return np.array(R.mont(r, v), dtype=np.uint64)


def _rand_raw(rng, r, n):
    return [rng.getrandbits(256) % r for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _pool(cid):
    """three random polynomials of the longest length, drawn once per field;
    the length sweeps take prefixes"""
    rng = random.Random(0xB00 + cid)
    return [_rand_raw(rng, P.CURVES[cid].r, max(LARGE)) for _ in range(3)]


def _check_witness(gpu_ctx, cid, polys_raw, sets, zs, v):
    """polys_raw: stored words as integers.  Runs the device witness and
    compares every row, its trailing zero and the batched evaluations."""
    import torch

    r = P.CURVES[cid].r
    n = len(polys_raw[0])
    d = [_dev(gpu_ctx, R.from_raw(p)) for p in polys_raw]
    out = _empty(gpu_ctx, len(sets) * n)
    out.fill_(-1)
    torch.cuda.synchronize()
    ev = gpu_ctx.multiopen_witness_device(cid, [t.data_ptr() for t in d], n, sets,
                                          np.array([R.mont(r, z) for z in zs], dtype=np.uint64), _scalar(r, v),
                                          out.data_ptr())
    rows = _host(out).reshape(len(sets), n, 4)
    for j, (s, z) in enumerate(zip(sets, zs)):
        q, e = R.gwc_witness([polys_raw[i] for i in s], z, v, r)
        assert np.array_equal(rows[j, :n - 1], R.from_raw(q)), (cid, n, j)
        assert not rows[j, n - 1].any(), (cid, n, j)
        assert R.raw_ints(ev[j:j + 1]) == [e], (cid, n, j)
    return ev


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_division_every_boundary(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(900 + cid)
    for n in SMALL:  # host wrapper, (n - 1) x 4 out
        a, z = _rand_raw(rng, r, n), rng.randrange(r)
        got = gpu_ctx.kate_division(cid, R.from_raw(a), _scalar(r, z))
        assert got.shape == (n - 1, 4)
        assert np.array_equal(got, R.from_raw(R.kate_division(a, z, r))), n
    for n in LARGE:  # device entry, S = 1, m = 1
        _check_witness(gpu_ctx, cid, [_pool(cid)[n % 3][:n]], [[0]], [rng.randrange(r)], rng.randrange(r))


@pytest.mark.parametrize("cid", [0, 1, 2])
@pytest.mark.parametrize("n", [257, 4097])
def test_adversarial_values(gpu_ctx, cid, n):
    r = P.CURVES[cid].r
    rng = random.Random(40 * n + cid)
    raw = lambda v: v * P.R_MONT % r  # noqa: E731  stored word of the plain value v
    polys = [_rand_raw(rng, r, n) for _ in range(24)]
    v = rng.randrange(r)
    for z in (0, 1, r - 1):
        _check_witness(gpu_ctx, cid, polys[:2], [[0, 1]], [z], v)
    top, zero = [raw(r - 1)] * n, [0] * n
    _check_witness(gpu_ctx, cid, [top, top], [[0, 1], [1]], [r - 1, rng.randrange(r)], r - 1)
    _check_witness(gpu_ctx, cid, [zero, polys[0]], [[0], [0, 1, 0]], [rng.randrange(r), rng.randrange(r)], v)
    for vv in (0, 1, r - 1):
        _check_witness(gpu_ctx, cid, polys[:3], [[0, 1, 2]], [rng.randrange(r)], vv)
    _check_witness(gpu_ctx, cid, polys[:2], [[0, 1, 0, 0]], [rng.randrange(r)], v)  # one polynomial listed twice
    _check_witness(gpu_ctx, cid, polys, [list(range(24))], [rng.randrange(r)], v)  # m = 24
    sets = [[5], [3, 9], list(range(7, 14)), list(range(23, -1, -1))]
    _check_witness(gpu_ctx, cid, polys, sets, [rng.randrange(r) for _ in sets], v)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_evaluation(gpu_ctx, cid):
    r = P.CURVES[cid].r
    rng = random.Random(1300 + cid)
    for n in SMALL + LARGE:
        polys = [p[:n] for p in _pool(cid)]
        d = [_dev(gpu_ctx, R.from_raw(p)) for p in polys]
        ptrs = [t.data_ptr() for t in d]
        idx = [0, 1, 2, 0, 0, 2, 1, 2, 1]
        pts = [0, 1, r - 1] + [rng.randrange(r) for _ in range(5)]
        pts.append(pts[3])  # polynomial 1 and polynomial 0 at the same point
        got = gpu_ctx.poly_eval_device(cid, ptrs, n, idx, np.array([R.mont(r, z) for z in pts], dtype=np.uint64))
        want = [R.eval_polynomial(polys[i], z, r) for i, z in zip(idx, pts)]
        assert R.raw_ints(got) == want, n
        if n <= 130:  # host wrapper
            one = gpu_ctx.eval_polynomial(cid, R.from_raw(polys[2]), _scalar(r, pts[5]))
            assert R.raw_ints(one.reshape(1, 4)) == [want[5]], n
        # a witness call's batched evaluation = sum_i v^{m-1-i} p_i(z)
        v, z = rng.randrange(r), pts[4]
        out = _empty(gpu_ctx, n)
        ev = gpu_ctx.multiopen_witness_device(cid, ptrs, n, [[2, 0, 1]], _scalar(r, z).reshape(1, 4), _scalar(r, v),
                                              out.data_ptr())
        vals = R.raw_ints(gpu_ctx.poly_eval_device(cid, ptrs, n, [2, 0, 1],
                                                   np.array([R.mont(r, z)] * 3, dtype=np.uint64)))
        assert R.raw_ints(ev) == [(vals[0] * v * v + vals[1] * v + vals[2]) % r], n


@pytest.mark.parametrize("k", [20, 22])
def test_large_sizes_by_identity(gpu_ctx, k):
    """batch(rho) - batch(z) == q(rho) (rho - z) for a random rho, every term
    evaluated on the device; at 2^20 one full quotient row against poly_ref."""
    import torch

    cid, n = H.BN254, 1 << k
    r = P.CURVES[cid].r
    rng = random.Random(k)
    d = [_empty(gpu_ctx, n) for _ in range(4)]
    for i, t in enumerate(d):
        gpu_ctx.synth_scalars(cid, 0x90 + i, 0, n, t.data_ptr())
    sets, zs, v, rho = [[0, 1, 2], [1, 3, 0]], [rng.randrange(r), rng.randrange(r)], rng.randrange(r), rng.randrange(r)
    out = _empty(gpu_ctx, 2 * n)
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in d]
    ev = R.from_array(r, gpu_ctx.multiopen_witness_device(
        cid, ptrs, n, sets, np.array([R.mont(r, z) for z in zs], dtype=np.uint64), _scalar(r, v), out.data_ptr()))
    rows = [out.data_ptr() + j * n * 32 for j in range(2)]
    idx = [0, 1, 2, 3, 4, 5]
    vals = R.from_array(r, gpu_ctx.poly_eval_device(cid, ptrs + rows, n, idx,
                                                    np.array([R.mont(r, rho)] * 6, dtype=np.uint64)))
    for j, (s, z) in enumerate(zip(sets, zs)):
        batch_rho = 0
        for i in s:
            batch_rho = (batch_rho * v + vals[i]) % r
        assert (batch_rho - ev[j]) % r == vals[4 + j] * (rho - z) % r, j
    if k == 20:
        polys = [R.raw_ints(_host(d[i])) for i in sets[1]]
        q = R.kate_division(R.batch_poly(polys, v, r), zs[1], r)
        row = _host(out).reshape(2, n, 4)[1]
        assert np.array_equal(row[:n - 1], R.from_raw(q))
        assert not row[n - 1].any()


def _open_case(gpu_ctx, cid, n, tau, rng):
    C = P.CURVES[cid]
    r = C.r
    pts, srs_arr = R.srs(cid, tau, n)
    srs = gpu_ctx.upload_bases(cid, srs_arr)
    polys = [[rng.randrange(r) for _ in range(n)] for _ in range(5)]
    arrs = [R.to_array(r, p) for p in polys]
    d = [_dev(gpu_ctx, a) for a in arrs]
    sets = [[0, 1, 2], [3], [4, 0, 2, 1]]
    zs, v = [rng.randrange(r) for _ in sets], rng.randrange(r)
    commits = [P.limbs_to_point(C, [int(x) for x in gpu_ctx.msm_resident(srs, 0, a)]) for a in arrs]
    w, ev = gpu_ctx.multiopen_open_device(cid, [t.data_ptr() for t in d], n, sets,
                                          np.array([R.mont(r, z) for z in zs], dtype=np.uint64), _scalar(r, v), srs)
    ev = R.from_array(r, ev)
    for j, (s, z) in enumerate(zip(sets, zs)):
        q, e = R.gwc_witness([polys[i] for i in s], z, v, r)
        assert ev[j] == e
        W = P.limbs_to_point(C, [int(x) for x in w[j]])
        assert W == C.mul(R.eval_polynomial(q, tau, r), C.gen) if any(q) else W is None, (n, j)
        # the relation the verifier's w, zw, f, e feed into the pairing
        lhs = C.add(C.mul((tau - z) % r, W) if W else None, C.mul(e, C.gen) if e else None)
        rhs = None
        for i in s:  # Horner in v over the commitments, the order of f
            rhs = C.add(C.mul(v, rhs) if rhs else None, commits[i])
        assert lhs == rhs, (n, j)
    srs.release()


@pytest.mark.parametrize("cid", [H.BN254, H.PALLAS])
def test_open_end_to_end(gpu_ctx, cid):
    rng = random.Random(60 + cid)
    tau = 0x1234567 + cid
    for n in (64, 1, 2):
        _open_case(gpu_ctx, cid, n, tau, rng)


def test_open_equals_witness_then_msm(gpu_ctx):
    import torch

    cid, n = H.BN254, 1 << 14
    r = P.CURVES[cid].r
    rng = random.Random(14)
    d_bases = torch.empty((n, 8), dtype=torch.int64, device=torch.device("cuda", gpu_ctx.device))
    gpu_ctx.synth_bases(cid, P.SEED_BASES, 0, n, d_bases.data_ptr())
    d = [_empty(gpu_ctx, n) for _ in range(3)]
    for i, t in enumerate(d):
        gpu_ctx.synth_scalars(cid, 0x40 + i, 0, n, t.data_ptr())
    torch.cuda.synchronize()
    srs = gpu_ctx.upload_bases(cid, d_bases=d_bases.data_ptr(), n=n)
    sets = [[0, 1, 2], [2], [1, 0]]
    zs = np.array([R.mont(r, rng.randrange(r)) for _ in sets], dtype=np.uint64)
    v = _scalar(r, rng.randrange(r))
    ptrs = [t.data_ptr() for t in d]
    w, ev = gpu_ctx.multiopen_open_device(cid, ptrs, n, sets, zs, v, srs)
    out = _empty(gpu_ctx, len(sets) * n)
    ev2 = gpu_ctx.multiopen_witness_device(cid, ptrs, n, sets, zs, v, out.data_ptr())
    assert np.array_equal(ev, ev2)
    for j in range(len(sets)):
        got = gpu_ctx.msm_resident_device(srs, 0, out.data_ptr() + j * n * 32, n)
        assert np.array_equal(w[j], got), j
        assert w[j].any()
    srs.release()


def test_argument_errors_on_a_live_context(gpu_ctx):
    cid = H.BN254
    r = P.CURVES[cid].r
    rng = random.Random(6)
    n = 300
    a = _rand_raw(rng, r, n)
    d = _dev(gpu_ctx, R.from_raw(a))
    out = _empty(gpu_ctx, n)
    z1, v = _scalar(r, 5).reshape(1, 4), _scalar(r, 7)
    srs = gpu_ctx.upload_bases(cid, R.srs(cid, 3, 4)[1])

    def code(fn):
        with pytest.raises(H.PmError) as e:
            fn()
        return int(str(e.value).split(":")[0].split()[-1])

    ptr = [d.data_ptr()]
    assert code(lambda: gpu_ctx.multiopen_witness_device(cid, ptr, 0, [[0]], z1, v, out.data_ptr())) == -1
    assert code(lambda: gpu_ctx.multiopen_witness_device(cid, ptr, n, [[]], z1, v, out.data_ptr())) == -1
    assert code(lambda: gpu_ctx.multiopen_witness_device(cid, ptr, n, [[1]], z1, v, out.data_ptr())) == -1
    assert code(lambda: gpu_ctx.poly_eval_device(cid, ptr, n, [1], z1)) == -1
    assert code(lambda: gpu_ctx.poly_eval_device(cid, ptr, 0, [0], z1)) == -1
    assert code(lambda: gpu_ctx.multiopen_open_device(cid, ptr, (1 << 26) + 1, [[0]], z1, v, srs)) == -4
    assert code(lambda: gpu_ctx.multiopen_witness_device(cid, ptr, (1 << 28) + 1, [[0]], z1, v, out.data_ptr())) == -4
    assert code(lambda: gpu_ctx.multiopen_open_device(cid, ptr, n, [[0]], z1, v, srs)) == -1  # SRS of 4 points
    # S == 0 and E == 0 succeed and write nothing
    assert gpu_ctx.poly_eval_device(cid, ptr, n, [], np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)
    assert gpu_ctx.multiopen_witness_device(cid, ptr, n, [], np.zeros((0, 4), dtype=np.uint64), v,
                                            out.data_ptr()).shape == (0, 4)
    srs.release()
    # the context still computes
    _check_witness(gpu_ctx, cid, [a], [[0]], [rng.randrange(r)], 1)
    got = gpu_ctx.poly_eval_device(cid, ptr, n, [0], z1)
    assert R.raw_ints(got) == [R.eval_polynomial(a, 5, r)]

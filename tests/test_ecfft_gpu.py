"""GPU tests of best_fft over curve points (pm_fft_points / pm_fft_points_device)
through halo2_amd.py, bit for bit:

  * every log_n = 0 .. 10 on the three curves, device and host-pointer entry,
    scale NULL / 1 / n^-1 / random, against pm_fft_points_host element for
    element (n = 1: no stage; 2: the multiplication-free stage only; 4: the
    first real twiddle; 512: one 256-lane block of butterflies; 1024: the first
    multi-block stage), log_n = 0 .. 3 against tests/ecfft_ref.py as well;
  * adversarial inputs at log_n = 3 and 10 through pin 1 (known discrete logs):
    equal inputs, a single input, identities, a = +-t in the last stage,
    scale = 0, a planted identity output;
  * 2^14 and 2^16 (BN254), 2^14 (Pallas, Vesta): forward then inverse returns
    the input, 256 sampled outputs against pin 1, one random linear combination
    of ALL outputs against pin 1;
  * pin 2 at 2^12 on BN254: MSM(coefficients, g) = MSM(evaluations, g_lagrange)
    through pm_bases_upload_device / pm_msm_resident, and a one-input
    pm_msm_resident_many against the new basis;
  * the twiddle cache across three roots on one context, and the context still
    serving pm_fft and pm_msm afterwards.
"""
import random

import numpy as np
import pytest

import ecfft_ref as E
import halo2_amd as H
import msm_ref
import ntt as N
import pasta as P

pytestmark = pytest.mark.gpu

HOST_THREADS = 8


def _dev(gpu_ctx, arr):
    import torch

    a = np.ascontiguousarray(arr, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(torch.device("cuda", gpu_ctx.device))


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _run_device(gpu_ctx, curve, pts, log_n, w, sc):
    d = _dev(gpu_ctx, pts)
    _host(d)  # the copy is done before the context's stream reads it
    gpu_ctx.fft_points_device(curve, d.data_ptr(), log_n, w, sc)
    return _host(d).reshape(-1, 8)


def _int_rows(arr, r):
    """(n, 4) u64 Montgomery scalars -> integers."""
    rinv = pow(P.R_MONT, -1, r)
    L = np.asarray(arr).astype(object)
    return [int(v) * rinv % r for v in (L[:, 0] + (L[:, 1] << 64) + (L[:, 2] << 128) + (L[:, 3] << 192))]


def _dlogs(curve, log_n, salt=0):
    C = P.CURVES[curve]
    return [P.synth_base_dlog(C, P.SEED_BASES + salt, 4096 * log_n + i) for i in range(1 << log_n)]


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_every_length_vs_host(gpu_ctx, curve):
    C = P.CURVES[curve]
    rng = random.Random(77 + curve)
    for log_n in range(0, 11):
        n = 1 << log_n
        a = _dlogs(curve, log_n)
        if n >= 4:
            a[n - 1] = 0      # an identity input
            a[2] = a[0]       # equal inputs in a later stage
        pts = E.dlog_points(curve, a)
        omega = E.root_of_unity(curve, log_n)
        w = E.scalar_limbs(curve, omega)
        for scale in (None, 1, pow(n, -1, C.r), rng.randrange(1, C.r)):
            sc = None if scale is None else E.scalar_limbs(curve, scale)
            want = H.fft_points_host(curve, pts, w, sc, threads=HOST_THREADS)
            assert np.array_equal(gpu_ctx.fft_points(curve, pts, w, sc), want), (log_n, scale, "host pointer")
            assert np.array_equal(_run_device(gpu_ctx, curve, pts, log_n, w, sc), want), (log_n, scale, "device")
            if log_n <= 3:
                ref = E.fft_points(curve, E.limbs_to_points(curve, pts), omega, log_n, scale)
                assert np.array_equal(want, E.points_to_limbs(curve, ref)), (log_n, scale, "restatement")


def _adversarial(curve, log_n):
    """name -> (dlogs, scale[, index of the planted identity output])"""
    C = P.CURVES[curve]
    r, n = C.r, 1 << log_n
    base = _dlogs(curve, log_n, salt=9)
    h = n // 2
    cases = {
        "all_equal": ([base[0]] * n, None),                       # a doubling in the first stage, identities after
        "single_at_0": ([base[0]] + [0] * (n - 1), None),
        "single_at_1": ([0, base[1]] + [0] * (n - 2), None),      # out[k] = [omega^k]P, -1 = r - 1 among them
        "all_identity": ([0] * n, 1),
        "interleaved": ([0 if i % 2 else base[i] for i in range(n)], None),
        "halves_equal": (base[:h] + base[:h], None),              # in[j] = in[j + n/2]: every first-stage pair doubles
        "halves_opposite": (base[:h] + [r - v for v in base[:h]], None),  # ... or cancels
        "scale_zero": (list(base), 0),
    }
    # a planted identity output (a_0 enters every output with coefficient 1).  The last stage pairs
    # outputs j and j + n/2: out[j + n/2] = O means a = t there (a' = a + t doubles), out[j] = O means a = -t
    omega = E.root_of_unity(curve, log_n)
    e = E.expected_dlogs(curve, base, omega, log_n)
    for name, k0 in (("planted_a_eq_t", n - 3), ("planted_a_eq_minus_t", 2)):
        planted = list(base)
        planted[0] = (planted[0] - e[k0]) % r
        cases[name] = (planted, pow(n, -1, r), k0)
    return omega, cases


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("log_n", [3, 10])
def test_adversarial_inputs_known_dlogs(gpu_ctx, curve, log_n):
    omega, cases = _adversarial(curve, log_n)
    w = E.scalar_limbs(curve, omega)
    for i, (name, (a, scale, *k0)) in enumerate(cases.items()):
        pts = E.dlog_points(curve, a)
        sc = None if scale is None else E.scalar_limbs(curve, scale)
        e = E.expected_dlogs(curve, a, omega, log_n, scale)
        want = E.dlog_points(curve, e)
        if name == "all_equal":
            assert e[0] != 0 and not any(e[1:])
        if name in ("all_identity", "scale_zero"):
            assert not want.any()
        if k0:
            assert e[k0[0]] == 0 and not want[k0[0]].any() and want[k0[0] ^ (1 << (log_n - 1))].any()
        got = gpu_ctx.fft_points(curve, pts, w, sc) if i % 2 else _run_device(gpu_ctx, curve, pts, log_n, w, sc)
        assert np.array_equal(got, want), name


@pytest.mark.parametrize("curve,log_n", [(2, 14), (2, 16), (0, 14), (1, 14)])
def test_large_round_trip_samples_and_combination(gpu_ctx, curve, log_n):
    C = P.CURVES[curve]
    r, n = C.r, 1 << log_n
    pts = msm_ref.synth_bases(curve, P.SEED_BASES, 0, n)                      # P_i = [a_i]G
    a = _int_rows(msm_ref.synth_scalars(curve, P.SEED_BASES, 0, n), r)
    omega = E.root_of_unity(curve, log_n)
    w = E.scalar_limbs(curve, omega)
    scale = random.Random(log_n + curve).randrange(1, r)
    sc = E.scalar_limbs(curve, scale)
    d = _dev(gpu_ctx, pts)
    _host(d)
    gpu_ctx.fft_points_device(curve, d.data_ptr(), log_n, w, sc)
    out = _host(d).reshape(-1, 8).copy()
    # pin 1 on 256 sampled outputs
    e = E.expected_dlogs(curve, a, omega, log_n, scale)
    rng = random.Random(5 * log_n + curve)
    ks = [0, 1, n // 2, n - 1] + [rng.randrange(n) for _ in range(252)]
    assert np.array_equal(out[ks], E.dlog_points(curve, [e[k] for k in ks]))
    # one random linear combination of all n outputs (a single C-port MSM) against [sum c_k e_k]G
    c = [rng.randrange(1, r) for _ in range(n)]
    cs = np.array([P.to_limbs(v * P.R_MONT % r) for v in c], dtype=np.uint64)
    comb = msm_ref.best_multiexp(curve, cs, out)
    assert np.array_equal(comb.reshape(1, 8), E.dlog_points(curve, [sum(x * y for x, y in zip(c, e)) % r]))
    # the inverse, undoing the scale with it: omega^-1 and (n scale)^-1
    back = E.scalar_limbs(curve, pow(n * scale, -1, r))
    gpu_ctx.fft_points_device(curve, d.data_ptr(), log_n, E.scalar_limbs(curve, pow(omega, -1, r)), back)
    assert np.array_equal(_host(d).reshape(-1, 8), pts)
    # ... and the plain pair: forward unscaled, inverse with n^-1
    gpu_ctx.fft_points_device(curve, d.data_ptr(), log_n, w)
    gpu_ctx.fft_points_device(curve, d.data_ptr(), log_n, E.scalar_limbs(curve, pow(omega, -1, r)),
                              E.scalar_limbs(curve, pow(n, -1, r)))
    assert np.array_equal(_host(d).reshape(-1, 8), pts)


def test_lagrange_basis_property(gpu_ctx):
    """Pin 2 at 2^12 on BN254: for a random p of degree < n, the MSM of its coefficients against g equals
    the MSM of its evaluations on the domain against g_lagrange = fft_points(g, omega^-1, n^-1)."""
    curve, log_n = 2, 12
    C = P.CURVES[curve]
    r, n = C.r, 1 << log_n
    g = msm_ref.synth_bases(curve, P.SEED_BASES, 0, n)
    omega = E.root_of_unity(curve, log_n)
    d_lag = _dev(gpu_ctx, g)
    d_g = _dev(gpu_ctx, g)
    _host(d_g)
    gpu_ctx.fft_points_device(curve, d_lag.data_ptr(), log_n, E.scalar_limbs(curve, pow(omega, -1, r)),
                              E.scalar_limbs(curve, pow(n, -1, r)))
    srs = gpu_ctx.upload_bases(curve, d_bases=d_g.data_ptr(), n=n)
    lag = gpu_ctx.upload_bases(curve, d_bases=d_lag.data_ptr(), n=n)
    rng = random.Random(4242)
    coeffs = [rng.randrange(r) for _ in range(n)]
    evals = N.serial_fft(list(coeffs), omega, log_n, r)
    to_arr = lambda vs: np.array([P.to_limbs(v * P.R_MONT % r) for v in vs], dtype=np.uint64)  # noqa: E731
    lhs = gpu_ctx.msm_resident(srs, 0, to_arr(coeffs))
    rhs = gpu_ctx.msm_resident(lag, 0, to_arr(evals))
    assert lhs.any() and np.array_equal(lhs, rhs)
    assert np.array_equal(lhs, msm_ref.best_multiexp(curve, to_arr(coeffs), g))
    # an instance commitment of one public input: [v] g_lagrange[0]
    v = rng.randrange(1, r)
    lag_host = _host(d_lag).reshape(-1, 8)
    got = gpu_ctx.msm_resident_many(lag, [1], to_arr([v]))
    assert np.array_equal(got[0], msm_ref.best_multiexp(curve, to_arr([v]), lag_host[:1], threads=1))
    # g_lagrange[0] = [n^-1 sum_j a_j]G
    a = _int_rows(msm_ref.synth_scalars(curve, P.SEED_BASES, 0, n), r)
    assert np.array_equal(lag_host[:1], E.dlog_points(curve, [sum(a) * pow(n, -1, r) % r]))


def test_twiddle_cache_and_context_reuse(gpu_ctx):
    curve, log_n = 2, 6
    C = P.CURVES[curve]
    r, n = C.r, 1 << log_n
    pts = E.dlog_points(curve, _dlogs(curve, log_n, salt=3))
    w1 = E.root_of_unity(curve, log_n)
    roots = [w1, pow(w1, -1, r), pow(w1, 3, r)]   # three roots: one more than the context caches
    want = [H.fft_points_host(curve, pts, E.scalar_limbs(curve, w), threads=HOST_THREADS) for w in roots]
    assert not np.array_equal(want[0], want[1])
    for i in (0, 1, 0, 2, 1, 0):
        assert np.array_equal(gpu_ctx.fft_points(curve, pts, E.scalar_limbs(curve, roots[i])), want[i]), i
    # another length and curve in between, then the first again
    w5 = E.scalar_limbs(0, E.root_of_unity(0, 5))
    p5 = E.dlog_points(0, _dlogs(0, 5))
    assert np.array_equal(gpu_ctx.fft_points(0, p5, w5), H.fft_points_host(0, p5, w5))
    assert np.array_equal(gpu_ctx.fft_points(curve, pts, E.scalar_limbs(curve, roots[0])), want[0])
    # the context still serves the scalar NTT and an MSM
    a = [random.Random(9).randrange(r) for _ in range(n)]
    arr = np.array([P.to_limbs(v * P.R_MONT % r) for v in a], dtype=np.uint64)
    got = gpu_ctx.fft(curve, arr, E.scalar_limbs(curve, w1))
    assert _int_rows(got, r) == N.serial_fft(list(a), w1, log_n, r)
    assert np.array_equal(gpu_ctx.msm(curve, arr, pts), msm_ref.best_multiexp(curve, arr, pts))


def test_errors_with_a_context(gpu_ctx):
    pts = E.dlog_points(2, _dlogs(2, 3))
    with pytest.raises(H.PmError, match="root of unity"):
        gpu_ctx.fft_points(2, pts, E.scalar_limbs(2, E.root_of_unity(2, 4)))
    with pytest.raises(H.PmError, match="curve"):
        gpu_ctx.fft_points(5, pts, E.scalar_limbs(2, E.root_of_unity(2, 3)))
    with pytest.raises(H.PmError, match="null"):
        gpu_ctx.fft_points_device(2, 0, 3, E.scalar_limbs(2, E.root_of_unity(2, 3)))

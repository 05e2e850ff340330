"""TEST INFRASTRUCTURE ONLY -- halo2's best_fft over curve points, restated over
``pasta.Curve`` (affine points, None the identity), and what the point
transform's tests share: roots of unity, the boundary's limb forms, and pin 1.

    out[k] = [scale] sum_j [omega^(jk)] in[j]

PARITY STATUS: unpinned by the reference (its halo2 fork is not vendored).  The
pins are (1) known discrete logs: with in[j] = [a_j]G the definition gives
out[k] = [scale NTT(a)_k]G, the scalar transform from oracle/ntt.py; (2) the
defining property of a Lagrange basis: MSM(coefficients of p, g) =
MSM(evaluations of p, fft_points(g, omega^-1, n^-1)).
"""
import numpy as np

import msm_ref
import ntt
import pasta as P

TWO_ADICITY = {0: 32, 1: 32, 2: 28}


def root_of_unity(curve, log_n):
    """A primitive 2^log_n-th root of unity of the curve's scalar field."""
    r = P.CURVES[curve].r
    if log_n == 0:
        return 1
    x = 2
    while True:
        w = pow(x, (r - 1) >> log_n, r)
        if pow(w, 1 << (log_n - 1), r) == r - 1:
            return w
        x += 1


def scalar_limbs(curve, v):
    """Integer -> (4,) u64 Montgomery words of the scalar field."""
    r = P.CURVES[curve].r
    return np.array(P.to_limbs(v % r * P.R_MONT % r), dtype=np.uint64)


def points_to_limbs(curve, pts):
    C = P.CURVES[curve]
    return np.array([P.point_to_limbs(C, q) for q in pts], dtype=np.uint64).reshape(-1, 8)


def limbs_to_points(curve, arr):
    C = P.CURVES[curve]
    return [P.limbs_to_point(C, [int(v) for v in row]) for row in np.asarray(arr).reshape(-1, 8)]


def fft_points(curve, pts, omega, log_n, scale=None):
    """best_fft's loop over points: bit reversal, then log_n stages of
    t = [w] b, b = a - t, a = a + t with w advanced by w_m; then [scale]."""
    C = P.CURVES[curve]
    a = list(pts)
    n = len(a)
    assert n == 1 << log_n
    for k in range(n):
        rk = ntt.bitreverse(k, log_n)
        if k < rk:
            a[k], a[rk] = a[rk], a[k]
    m = 1
    for _ in range(log_n):
        w_m = pow(omega, n // (2 * m), C.r)
        for k in range(0, n, 2 * m):
            w = 1
            for j in range(m):
                t = C.mul(w, a[k + j + m])
                a[k + j + m] = C.add(a[k + j], C.neg(t))
                a[k + j] = C.add(a[k + j], t)
                w = w * w_m % C.r
        m *= 2
    if scale is not None:
        a = [C.mul(scale, q) for q in a]
    return a


_G = {}
_DLOG = {}  # (curve, a) -> limbs: the tests ask for the same points again and again


def dlog_points(curve, dlogs):
    """[a]G for each a, (len, 8) u64 boundary limbs, through the C port (an n = 1 best_multiexp each)."""
    C = P.CURVES[curve]
    if curve not in _G:
        _G[curve] = np.array([P.point_to_limbs(C, C.gen)], dtype=np.uint64)
    out = np.zeros((len(dlogs), 8), dtype=np.uint64)
    for i, a in enumerate(dlogs):
        a %= C.r
        if a:
            if (curve, a) not in _DLOG:
                _DLOG[curve, a] = msm_ref.best_multiexp(curve, scalar_limbs(curve, a).reshape(1, 4), _G[curve],
                                                        threads=1)
            out[i] = _DLOG[curve, a]
    return out


def expected_dlogs(curve, dlogs, omega, log_n, scale=None):
    """Pin 1: the discrete logs of the outputs, scale * NTT(a)_k."""
    r = P.CURVES[curve].r
    e = ntt.serial_fft([a % r for a in dlogs], omega, log_n, r)
    return e if scale is None else [v * scale % r for v in e]

"""CPU tests of the point transform at the C-ABI boundary (no device): the three
entries are declared and exported; pm_fft_points_host against tests/ecfft_ref.py
element for element (log_n = 0 .. 8, three curves), against pin 1 (known
discrete logs) at 2^10, the same words on 1 and 4 threads; and every argument
error of the three entries (they check their arguments before they look at the
context, so a null context reaches each of them)."""
import ctypes

import numpy as np
import pytest

import ecfft_ref as E
import halo2_amd as H
import pasta as P

ENTRIES = ["pm_fft_points_device", "pm_fft_points", "pm_fft_points_host"]
PM_ERR_ARG, PM_ERR_UNSUPPORTED = -1, -4
u64p = ctypes.POINTER(ctypes.c_uint64)


def test_entries_declared_and_exported():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name
        assert getattr(H.lib(), name).argtypes, name
    txt = open(H.HEADER_PATH).read()
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4


def _dlogs(curve, log_n):
    C = P.CURVES[curve]
    n = 1 << log_n
    a = [P.synth_base_dlog(C, P.SEED_BASES, 1000 * log_n + i) for i in range(n)]
    if n >= 8:
        a[1] = 0            # an identity input
        a[3] = a[2]         # equal inputs: a doubling in the first stage
        a[5] = C.r - a[4]   # opposite inputs: an identity in the first stage
    return a


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_host_matches_the_restatement(curve):
    C = P.CURVES[curve]
    for log_n in range(0, 9):
        n = 1 << log_n
        a = _dlogs(curve, log_n)
        pts = E.dlog_points(curve, a)
        omega = E.root_of_unity(curve, log_n)
        for scale in (None, pow(n, -1, C.r)) if log_n in (0, 3, 8) else (None,):
            got = H.fft_points_host(curve, pts, E.scalar_limbs(curve, omega),
                                    None if scale is None else E.scalar_limbs(curve, scale))
            if log_n <= 5:   # the Python loop over points, element for element
                want = E.fft_points(curve, E.limbs_to_points(curve, pts), omega, log_n, scale)
                assert np.array_equal(got, E.points_to_limbs(curve, want)), (log_n, scale)
            # ... and pin 1 at every size (the restatement itself is pinned by it in test_ecfft_ref.py)
            want = E.dlog_points(curve, E.expected_dlogs(curve, a, omega, log_n, scale))
            assert np.array_equal(got, want), (log_n, scale)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_host_matches_the_restatement_6_to_8(curve):
    """Element for element against ecfft_ref.fft_points above 2^5 (the slow part of the Python loop)."""
    for log_n in (6, 7, 8):
        a = _dlogs(curve, log_n)
        pts = E.dlog_points(curve, a)
        omega = E.root_of_unity(curve, log_n)
        got = H.fft_points_host(curve, pts, E.scalar_limbs(curve, omega), threads=4)
        want = E.fft_points(curve, E.limbs_to_points(curve, pts), omega, log_n)
        assert np.array_equal(got, E.points_to_limbs(curve, want)), log_n


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_host_known_dlogs_2_10_and_threads(curve):
    C = P.CURVES[curve]
    log_n = 10
    a = _dlogs(curve, log_n)
    pts = E.dlog_points(curve, a)
    omega = pow(E.root_of_unity(curve, log_n), -1, C.r)
    scale = pow(1 << log_n, -1, C.r)
    w, sc = E.scalar_limbs(curve, omega), E.scalar_limbs(curve, scale)
    one = H.fft_points_host(curve, pts, w, sc, threads=1)
    four = H.fft_points_host(curve, pts, w, sc, threads=4)
    assert np.array_equal(one, four)
    assert np.array_equal(one, E.dlog_points(curve, E.expected_dlogs(curve, a, omega, log_n, scale)))


def test_host_edges():
    curve = 2
    C = P.CURVES[curve]
    pts = E.dlog_points(curve, _dlogs(curve, 3))
    w = E.scalar_limbs(curve, E.root_of_unity(curve, 3))
    zero = H.fft_points_host(curve, pts, w, np.zeros(4, np.uint64))
    assert not zero.any()
    ident = H.fft_points_host(curve, np.zeros((8, 8), np.uint64), w)
    assert not ident.any()
    # log_n = 0: [scale] in[0]
    got = H.fft_points_host(curve, pts[:1], E.scalar_limbs(curve, 1), E.scalar_limbs(curve, 12345))
    assert np.array_equal(got, E.points_to_limbs(curve, [C.mul(12345, E.limbs_to_points(curve, pts[:1])[0])]))
    assert np.array_equal(H.fft_points_host(curve, pts[:1], E.scalar_limbs(curve, 1)), pts[:1])


def _err(rc, code, word):
    assert rc == code
    msg = H.lib().pm_last_error()
    assert word in msg, msg


def _calls():
    """(name, call(curve, points, log_n, omega)) for the three entries, context null."""
    L = H.lib()
    return [
        ("device", lambda c, p, k, w: L.pm_fft_points_device(None, c, ctypes.c_void_p(0x1000) if p else None, k, w, None)),
        ("staged", lambda c, p, k, w: L.pm_fft_points(None, c, p, k, w, None)),
        ("host", lambda c, p, k, w: L.pm_fft_points_host(c, p, k, w, None, 1)),
    ]


@pytest.mark.parametrize("entry", [0, 1, 2])
def test_argument_errors(entry):
    name, call = _calls()[entry]
    pts = np.zeros((8, 8), np.uint64)
    p = pts.ctypes.data_as(u64p)
    for curve in (0, 1, 2):
        good = E.scalar_limbs(curve, E.root_of_unity(curve, 3)).ctypes.data_as(u64p)
        _err(call(curve, None, 3, good), PM_ERR_ARG, b"null")
        _err(call(curve, p, 3, None), PM_ERR_ARG, b"null")
        _err(call(curve, p, 27, good), PM_ERR_UNSUPPORTED, b"2^26")
        # omega^(n/2) != -1: a root of half the order, of twice the order, one, zero, a non-canonical word
        r = P.CURVES[curve].r
        for bad in (E.root_of_unity(curve, 2), E.root_of_unity(curve, 4), 1, 0):
            _err(call(curve, p, 3, E.scalar_limbs(curve, bad).ctypes.data_as(u64p)), PM_ERR_ARG, b"root of unity")
        noncanon = np.array(P.to_limbs(E.root_of_unity(curve, 3) * P.R_MONT % r + r), dtype=np.uint64)
        _err(call(curve, p, 3, noncanon.ctypes.data_as(u64p)), PM_ERR_ARG, b"root of unity")
        # n = 1: omega must be one
        _err(call(curve, p, 0, E.scalar_limbs(curve, r - 1).ctypes.data_as(u64p)), PM_ERR_ARG, b"root of unity")
        if name != "host":  # every argument in order: only the context is missing
            _err(call(curve, p, 3, good), PM_ERR_ARG, b"context")
            _err(call(curve, p, 0, E.scalar_limbs(curve, 1).ctypes.data_as(u64p)), PM_ERR_ARG, b"context")
    good = E.scalar_limbs(2, E.root_of_unity(2, 3)).ctypes.data_as(u64p)
    _err(call(7, p, 3, good), PM_ERR_ARG, b"curve")
    _err(call(-1, p, 3, good), PM_ERR_ARG, b"curve")
    assert not pts.any()   # nothing was written


def test_python_wrapper_shape_checks():
    w = E.scalar_limbs(2, 1)
    with pytest.raises(ValueError):
        H.fft_points_host(2, np.zeros((3, 8), np.uint64), w)
    with pytest.raises(ValueError):
        H.fft_points_host(2, np.zeros((0, 8), np.uint64), w)

"""CPU: argument handling of the pairing decider's C-ABI entries.  Every check
runs before the context is looked at, so each error is reached here with a null
context and no device."""
import ctypes

import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest

ARG, UNSUPPORTED = -1, -4
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)


def _p(a):
    return a.ctypes.data_as(_u64p)


def _create(g2, s_g2):
    h = ctypes.c_void_p()
    rc = H.lib().pm_pairing_create(None, _p(g2) if g2 is not None else None, _p(s_g2) if s_g2 is not None else None,
                                   ctypes.byref(h))
    return rc, h


@pytest.fixture(scope="module")
def host_pairing():
    return H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


def test_create_rejects_bad_g2_points():
    g2, s = U.g2_words(PR.G2), U.g2_words(U.s_g2())
    assert _create(None, s)[0] == ARG and _create(g2, None)[0] == ARG
    assert H.lib().pm_pairing_create(None, _p(g2), _p(s), None) == ARG
    off = g2.copy()
    off[8] ^= np.uint64(1)  # y.c0: off the twist
    for a, b in ((off, s), (g2, off)):
        rc, h = _create(a, b)
        assert rc == ARG and not h.value
        assert b"twist" in H.lib().pm_last_error()
    zero = np.zeros(16, dtype=np.uint64)
    assert _create(zero, s)[0] == ARG and _create(g2, zero)[0] == ARG
    assert b"identity" in H.lib().pm_last_error()
    big = g2.copy()
    big[3] = np.uint64(0xFFFFFFFFFFFFFFFF)  # x.c0 >= p
    assert _create(big, s)[0] == ARG


def test_create_rejects_a_point_outside_the_order_r_subgroup():
    # a point of the twist that is not in G2: x' = 1 + k u with x'^3 + b' a square
    Q = None
    k = 0
    while Q is None:
        k += 1
        x = (1, k)
        rhs = PR.f2_add(PR.f2_mul(x, PR.f2_mul(x, x)), PR.B2)
        # sqrt in Fp2 for p = 3 mod 4: a1 = rhs^((p-3)/4), alpha = a1 (a1 rhs), x0 = a1 rhs
        a1 = PR.f2_pow(rhs, (PR.P - 3) // 4)
        x0 = PR.f2_mul(a1, rhs)
        alpha = PR.f2_mul(a1, x0)
        if alpha == (PR.P - 1, 0):
            y = PR.f2_mul((0, 1), x0)
        else:
            y = PR.f2_mul(PR.f2_pow(PR.f2_add(PR.F2_ONE, alpha), (PR.P - 1) // 2), x0)
        if PR.f2_mul(y, y) == rhs and PR.g2_mul(PR.R, (x, y), reduce=False) is not None:
            Q = (x, y)
    assert PR.g2_on_curve(Q)
    rc, h = _create(U.g2_words(PR.G2), U.g2_words(Q))
    assert rc == ARG and b"order r" in H.lib().pm_last_error()


def test_info_and_release():
    assert H.lib().pm_pairing_info(None, None, None, None) == ARG
    assert H.lib().pm_pairing_release(None) == 0
    rc, h = _create(U.g2_words(PR.G2), U.g2_words(U.s_g2()))
    assert rc == 0 and h.value
    steps = ctypes.c_uint32(0)
    assert H.lib().pm_pairing_info(h, ctypes.byref(steps), None, None) == 0 and steps.value == 102
    assert H.lib().pm_pairing_release(h) == 0


@pytest.mark.parametrize("entry", ["pm_pairing_check_device", "pm_accum_decide_device"])
def test_device_entries_check_arguments_before_the_context(host_pairing, entry):
    f = getattr(H.lib(), entry)
    buf = np.zeros(64, dtype=np.uint64)
    p = ctypes.c_void_p(buf.ctypes.data)
    # B == 0 succeeds and writes nothing, whatever else is passed
    assert f(None, None, 0, None, None, None, None, None) == 0
    assert f(None, None, 1, p, None, p, None, None) == ARG  # null pm_pairing
    assert f(None, host_pairing.h, 1, None, None, p, None, None) == ARG  # null input
    assert f(None, host_pairing.h, 1, p, None, None, None, None) == ARG  # null out_ok
    assert f(None, host_pairing.h, (1 << 24) + 1, p, None, p, None, None) == UNSUPPORTED
    assert f(None, host_pairing.h, 1, p, None, p, None, None) == ARG  # null context, looked at last
    assert b"context" in H.lib().pm_last_error()
    assert not buf.any()


def test_host_pointer_and_host_entries(host_pairing):
    q = np.zeros((1, 4, 8), dtype=np.uint64)
    ok = np.full(2, 7, dtype=np.uint32)
    okp = ok.ctypes.data_as(_u32p)
    L = H.lib()
    assert L.pm_accum_decide(None, None, 0, None, None, None, None, None) == 0
    assert L.pm_accum_decide(None, None, 1, _p(q), None, okp, None, None) == ARG
    assert L.pm_accum_decide(None, host_pairing.h, 1, None, None, okp, None, None) == ARG
    assert L.pm_accum_decide(None, host_pairing.h, 1, _p(q), None, None, None, None) == ARG
    assert L.pm_accum_decide(None, host_pairing.h, 1, _p(q), None, okp, None, None) == ARG
    assert L.pm_accum_decide_host(None, 0, None, None, None, None, None) == 0
    assert L.pm_accum_decide_host(None, 1, _p(q), None, okp, None, None) == ARG
    assert L.pm_accum_decide_host(host_pairing.h, 1, None, None, okp, None, None) == ARG
    assert L.pm_accum_decide_host(host_pairing.h, 1, _p(q), None, None, None, None) == ARG
    assert list(ok) == [7, 7]
    # the all-identity quad is accepted; only out_ok[0] is written
    assert L.pm_accum_decide_host(host_pairing.h, 1, _p(q), None, okp, None, None) == 0
    assert list(ok) == [1, 7]

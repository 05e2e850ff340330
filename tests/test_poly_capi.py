"""CPU tests of the polynomial-opening entries at the C-ABI boundary (no
device): declared in the header, exported by the library, argument errors with
a null context, and the Python wrappers' shape checks (which run before the
library is called)."""
import ctypes

import numpy as np
import pytest

import halo2_amd as H

ENTRIES = ["pm_poly_eval_device", "pm_multiopen_witness_device", "pm_multiopen_open_device", "pm_eval_polynomial",
           "pm_kate_division"]
PM_ERR_ARG = -1


def test_entries_declared_and_exported():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name


def test_header_section_and_abi_version():
    txt = open(H.HEADER_PATH).read()
    assert "Polynomial openings" in txt
    assert "must not" in txt and "alias" in txt
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4


def _u64(*shape):
    return np.zeros(shape, dtype=np.uint64)


def test_null_context_is_an_argument_error():
    L = H.lib()
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    p64 = lambda a: a.ctypes.data_as(u64p)  # noqa: E731
    p32 = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    ptrs = (ctypes.c_void_p * 1)(0x1000)
    idx, offs = np.zeros(1, np.uint32), np.array([0, 1], np.uint32)
    z, v, out, w = _u64(1, 4), _u64(4), _u64(1, 4), _u64(1, 8)
    coeffs = _u64(4, 4)
    assert L.pm_poly_eval_device(None, 2, ptrs, 1, 4, p32(idx), p64(z), 1, p64(out)) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()
    assert L.pm_multiopen_witness_device(None, 2, ptrs, 1, 4, p32(offs), p32(idx), p64(z), p64(v), 1,
                                         ctypes.c_void_p(0x2000), p64(out)) == PM_ERR_ARG
    assert L.pm_multiopen_open_device(None, 2, ptrs, 1, 4, p32(offs), p32(idx), p64(z), p64(v), 1,
                                      ctypes.c_void_p(0x3000), p64(w), p64(out)) == PM_ERR_ARG
    assert L.pm_eval_polynomial(None, 2, p64(coeffs), 4, p64(v), p64(out)) == PM_ERR_ARG
    assert L.pm_kate_division(None, 2, p64(coeffs), 4, p64(v), p64(_u64(3, 4))) == PM_ERR_ARG


def _detached_context():
    """A Context object without a device context behind it: the wrappers'
    shape checks raise before any library call, so none is ever made."""
    ctx = object.__new__(H.Context)
    ctx.h = None
    return ctx


def test_wrappers_reject_mismatched_shapes():
    ctx = _detached_context()
    with pytest.raises(ValueError):  # 3 indices, 2 points
        ctx.poly_eval_device(2, [0x1000], 8, [0, 0, 0], _u64(2, 4))
    with pytest.raises(ValueError):  # 2 sets, 1 point
        ctx.multiopen_witness_device(2, [0x1000], 8, [[0], [0]], _u64(1, 4), _u64(4), 0x2000)
    with pytest.raises(ValueError):  # v is not one scalar
        ctx.multiopen_witness_device(2, [0x1000], 8, [[0]], _u64(1, 4), _u64(8), 0x2000)
    with pytest.raises(ValueError):  # 1 set, 3 points
        ctx.multiopen_open_device(2, [0x1000], 8, [[0]], _u64(3, 4), _u64(4), None)
    with pytest.raises(ValueError):  # point is not one scalar
        ctx.eval_polynomial(2, _u64(8, 4), _u64(2, 4))
    with pytest.raises(ValueError):  # coefficients are not rows of 4 words
        ctx.eval_polynomial(2, _u64(3, 3), _u64(4))
    with pytest.raises(ValueError):
        ctx.kate_division(2, _u64(8, 4), _u64(3))
    with pytest.raises(ValueError):
        ctx.kate_division(2, _u64(7), _u64(4))

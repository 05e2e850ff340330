"""CPU tests of the grand-product entries at the C-ABI boundary (no device):
declared in the header, exported by the library, argument errors with a null
context, and the Python wrappers' shape checks (which run before the library
is called)."""
import ctypes
import re

import numpy as np
import pytest

import halo2_amd as H

ENTRIES = ["pm_batch_invert_device", "pm_batch_invert", "pm_grand_product_device"]
PM_ERR_ARG = -1


def test_entries_declared_and_exported():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name


def test_header_constants_and_struct():
    txt = open(H.HEADER_PATH).read()
    for name, value in (("PM_GP_NONE", H.GP_NONE), ("PM_GP_OMEGA", H.GP_OMEGA), ("PM_GP_CHAIN", H.GP_CHAIN),
                        ("PM_GP_MAX_FACTORS", H.GP_MAX_FACTORS)):
        m = re.search(r"#define %s\s+(0x[0-9A-Fa-f]+|\d+)u?" % name, txt)
        assert m and int(m.group(1), 0) == value, name
    assert "typedef struct pm_gp_factor" in txt
    # x, y, b[4], g[4]: 72 bytes, the layout the kernels read as 18 words
    assert ctypes.sizeof(H.PmGpFactor) == 72
    assert (H.PmGpFactor.x.offset, H.PmGpFactor.y.offset, H.PmGpFactor.b.offset, H.PmGpFactor.g.offset) == (0, 4, 8, 40)


def test_header_section_and_abi_version():
    txt = open(H.HEADER_PATH).read()
    assert "Grand products" in txt
    section = txt[txt.index("Grand products"):txt.index("int pm_grand_product_device")]
    assert "must not alias" in section
    assert txt.index("Polynomial openings") < txt.index("Grand products")
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4


def _u64(*shape):
    return np.zeros(shape, dtype=np.uint64)


def test_null_context_is_an_argument_error():
    L = H.lib()
    u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)
    p64 = lambda a: a.ctypes.data_as(u64p)  # noqa: E731
    p32 = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    ptrs = (ctypes.c_void_p * 1)(0x1000)
    fac = (H.PmGpFactor * 1)()
    offs = np.array([0, 1], np.uint32)
    assert L.pm_batch_invert_device(None, 2, ctypes.c_void_p(0x1000), 4) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()
    assert L.pm_batch_invert(None, 2, p64(_u64(4, 4)), 4) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()
    assert L.pm_grand_product_device(None, 2, ptrs, 1, 4, fac, p32(offs), fac, p32(offs), 1, p64(_u64(4)),
                                     p64(_u64(4)), 4, 0, ctypes.c_void_p(0x2000), p64(_u64(1, 4))) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()


def _detached_context():
    """A Context object without a device context behind it: the wrappers'
    shape checks raise before any library call, so none is ever made."""
    ctx = object.__new__(H.Context)
    ctx.h = None
    return ctx


def test_wrappers_reject_bad_arguments():
    ctx = _detached_context()
    one, zero = _u64(4), None
    ok = ([(0, None, zero, one)], [(1, 0, one, one)])
    cols = [0x1000, 0x2000]

    def gp(sets=(ok,), n=8, omega=None, start=one, active=8, ptrs=cols):
        return ctx.grand_product_device(2, ptrs, n, list(sets), omega, start, active, 0x3000)

    with pytest.raises(ValueError):  # values are not rows of 4 words
        ctx.batch_invert(2, _u64(3, 3))
    with pytest.raises(ValueError):  # start is not one scalar
        gp(start=_u64(8))
    with pytest.raises(ValueError):  # omega is not one scalar
        gp(omega=_u64(3))
    with pytest.raises(ValueError):  # g is not one scalar
        gp(sets=[([(0, None, zero, _u64(2))], [])])
    with pytest.raises(ValueError):  # a factor is (x, y, b, g)
        gp(sets=[([(0, None, one)], [])])
    with pytest.raises(ValueError):  # x index >= C
        gp(sets=[([(2, None, zero, one)], [])])
    with pytest.raises(ValueError):  # y index >= C
        gp(sets=[([], [(0, 2, one, one)])])
    with pytest.raises(ValueError):  # any index with C == 0
        gp(sets=[([(0, None, zero, one)], [])], ptrs=[])
    with pytest.raises(ValueError):  # 17 factors in one list
        gp(sets=[([(0, None, zero, one)] * 17, [])])
    with pytest.raises(ValueError):  # active == 0
        gp(active=0)
    with pytest.raises(ValueError):  # active > n
        gp(active=9)
    with pytest.raises(ValueError):  # PM_GP_OMEGA without omega
        gp(sets=[([(0, H.GP_OMEGA, one, one)], [])])
    with pytest.raises(ValueError):  # no set
        gp(sets=[])

"""CPU tests of the lookup entries at the C-ABI boundary (no device): declared
in the header, exported by the library, every argument error (the entries
check their arguments before they look at the context, so a null context
reaches each of them), and the Python wrappers' shape checks (which run before
the library is called)."""
import ctypes
import re

import numpy as np
import pytest

import halo2_amd as H

ENTRIES = ["pm_lookup_compress_device", "pm_lookup_permute_device", "pm_lookup_permute"]
PM_ERR_ARG, PM_ERR_UNSUPPORTED = -1, -4
BN254 = 2

u64p, u32p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)


def test_entries_declared_and_exported():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name


def test_header_section_constants_and_abi_version():
    txt = open(H.HEADER_PATH).read()
    assert "Lookup permuted columns" in txt
    assert txt.index("Grand products") < txt.index("Lookup permuted columns") < txt.index("Extended-domain conversions")
    section = txt[txt.index("Lookup permuted columns"):txt.index("int pm_lookup_compress_device")]
    for phrase in ("may alias", "must not alias", "Context scratch", "2^28", "PM_LOOKUP_MAX_PAIRS", "PM_LOOKUP_MAX_COLS"):
        assert phrase in section, phrase
    for name, value in (("PM_LOOKUP_MAX_PAIRS", H.LOOKUP_MAX_PAIRS), ("PM_LOOKUP_MAX_COLS", H.LOOKUP_MAX_COLS),
                        ("PM_LOOKUP_TILE", H.LOOKUP_TILE), ("PM_LOOKUP_MERGE", H.LOOKUP_MERGE)):
        m = re.search(r"#define %s\s+(\d+)" % name, txt)
        assert m and int(m.group(1)) == value, name
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4


def _ptrs(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _err(rc, code, word):
    assert rc == code
    msg = H.lib().pm_last_error()
    assert word in msg, msg


def test_compress_argument_errors():
    L = H.lib()
    theta = np.zeros(4, np.uint64).ctypes.data_as(u64p)
    cols, out = _ptrs(0x1000, 0x2000), ctypes.c_void_p(0x3000)
    f = L.pm_lookup_compress_device
    _err(f(None, BN254, cols, 2, 8, theta, out), PM_ERR_ARG, b"context")
    _err(f(None, BN254, None, 2, 8, theta, out), PM_ERR_ARG, b"null")
    _err(f(None, BN254, cols, 2, 8, theta, None), PM_ERR_ARG, b"null")
    _err(f(None, BN254, cols, 2, 8, None, out), PM_ERR_ARG, b"theta")
    _err(f(None, BN254, cols, 1, 8, None, out), PM_ERR_ARG, b"context")  # one column: theta is not needed
    _err(f(None, 7, cols, 2, 8, theta, out), PM_ERR_ARG, b"curve")
    _err(f(None, BN254, cols, 2, 0, theta, out), PM_ERR_ARG, b"empty")
    _err(f(None, BN254, cols, 0, 8, theta, out), PM_ERR_ARG, b"no column")
    _err(f(None, BN254, _ptrs(0x1000, 0), 2, 8, theta, out), PM_ERR_ARG, b"null column")
    _err(f(None, BN254, cols, 2, (1 << 28) + 1, theta, out), PM_ERR_UNSUPPORTED, b"2^28")
    _err(f(None, BN254, cols, H.LOOKUP_MAX_COLS + 1, 8, theta, out), PM_ERR_UNSUPPORTED, b"65535")


def test_permute_device_argument_errors():
    L = H.lib()
    f = L.pm_lookup_permute_device
    st = np.zeros((2, 2), np.uint32).ctypes.data_as(u32p)
    a, s, oa, os_ = _ptrs(0x1000, 0x5000), _ptrs(0x2000, 0x6000), _ptrs(0x3000, 0x7000), _ptrs(0x4000, 0x8000)

    def call(ctx=None, curve=BN254, a=a, s=s, P=2, n=8, usable=7, oa=oa, os_=os_, st=st):
        return f(ctx, curve, a, s, P, n, usable, oa, os_, st)

    _err(call(), PM_ERR_ARG, b"context")
    for missing in ("a", "s", "oa", "os_", "st"):
        _err(call(**{missing: None}), PM_ERR_ARG, b"null")
    _err(call(curve=9), PM_ERR_ARG, b"curve")
    _err(call(n=0, usable=0), PM_ERR_ARG, b"empty")
    _err(call(usable=0), PM_ERR_ARG, b"usable")
    _err(call(usable=9), PM_ERR_ARG, b"usable")
    _err(call(P=0), PM_ERR_ARG, b"no pair")
    _err(call(a=_ptrs(0x1000, 0)), PM_ERR_ARG, b"null column")
    _err(call(os_=_ptrs(0x4000, 0)), PM_ERR_ARG, b"null column")
    _err(call(n=(1 << 28) + 1), PM_ERR_UNSUPPORTED, b"2^28")
    _err(call(P=H.LOOKUP_MAX_PAIRS + 1), PM_ERR_UNSUPPORTED, b"32767")
    # the two aliases the header allows, and a table shared by both pairs
    _err(call(oa=a, os_=s), PM_ERR_ARG, b"context")
    _err(call(s=_ptrs(0x2000, 0x2000)), PM_ERR_ARG, b"context")
    # ... and those it does not
    for bad in (dict(oa=s), dict(os_=a),                        # the other input of the pair
                dict(oa=_ptrs(0x3000, 0x3000)),                 # two outputs on one column
                dict(os_=oa),                                   # A' and S' of a pair on one column
                dict(oa=_ptrs(0x5000, 0x1000)),                 # the input of another pair
                dict(os_=_ptrs(0x4000, 0x3000)),                # the output of another pair
                dict(s=_ptrs(0x2000, 0x2000), os_=_ptrs(0x2000, 0x8000))):  # in place on a shared table
        _err(call(**bad), PM_ERR_ARG, b"aliases")


def test_permute_host_argument_errors():
    L = H.lib()
    f = L.pm_lookup_permute
    bufs = [np.zeros((8, 4), np.uint64) for _ in range(4)]
    a, s, oa, os_ = (b.ctypes.data_as(u64p) for b in bufs)
    st = np.zeros(2, np.uint32).ctypes.data_as(u32p)
    _err(f(None, BN254, a, s, 8, 7, oa, os_, st), PM_ERR_ARG, b"context")
    _err(f(None, BN254, a, s, 8, 7, a, s, st), PM_ERR_ARG, b"context")  # in place
    for k in range(5):
        args = [a, s, oa, os_, st]
        args[k] = None
        _err(f(None, BN254, args[0], args[1], 8, 7, args[2], args[3], args[4]), PM_ERR_ARG, b"null")
    _err(f(None, 5, a, s, 8, 7, oa, os_, st), PM_ERR_ARG, b"curve")
    _err(f(None, BN254, a, s, 0, 0, oa, os_, st), PM_ERR_ARG, b"empty")
    _err(f(None, BN254, a, s, 8, 0, oa, os_, st), PM_ERR_ARG, b"usable")
    _err(f(None, BN254, a, s, 8, 9, oa, os_, st), PM_ERR_ARG, b"usable")
    _err(f(None, BN254, a, s, (1 << 28) + 1, 7, oa, os_, st), PM_ERR_UNSUPPORTED, b"2^28")
    _err(f(None, BN254, a, s, 8, 7, s, os_, st), PM_ERR_ARG, b"aliases")
    _err(f(None, BN254, a, s, 8, 7, oa, a, st), PM_ERR_ARG, b"aliases")
    _err(f(None, BN254, a, s, 8, 7, oa, oa, st), PM_ERR_ARG, b"aliases")


def _detached_context():
    """A Context object without a device context behind it: the wrappers'
    shape checks raise before any library call, so none is ever made."""
    ctx = object.__new__(H.Context)
    ctx.h = None
    return ctx


def test_wrappers_reject_bad_arguments():
    ctx = _detached_context()
    one = np.zeros(4, np.uint64)

    def compress(cols=(0x1000, 0x2000), n=8, theta=one, out=0x3000):
        return ctx.lookup_compress_device(BN254, list(cols), n, theta, out)

    with pytest.raises(ValueError):  # no column
        compress(cols=())
    with pytest.raises(ValueError):  # n == 0
        compress(n=0)
    with pytest.raises(ValueError):  # n > 2^28
        compress(n=(1 << 28) + 1)
    with pytest.raises(ValueError):  # theta is not one scalar
        compress(theta=np.zeros(3, np.uint64))
    with pytest.raises(ValueError):  # two columns and no theta
        compress(theta=None)
    with pytest.raises(ValueError):  # null column
        compress(cols=(0x1000, 0))
    with pytest.raises(ValueError):  # null output
        compress(out=0)

    def permute(a=(0x1000,), s=(0x2000,), n=8, usable=7, oa=(0x3000,), os_=(0x4000,)):
        return ctx.lookup_permute_device(BN254, list(a), list(s), n, usable, list(oa), list(os_))

    with pytest.raises(ValueError):  # no pair
        permute(a=(), s=(), oa=(), os_=())
    with pytest.raises(ValueError):  # lists of different lengths
        permute(s=(0x2000, 0x6000))
    with pytest.raises(ValueError):  # n == 0
        permute(n=0, usable=0)
    with pytest.raises(ValueError):  # usable == 0
        permute(usable=0)
    with pytest.raises(ValueError):  # usable > n
        permute(usable=9)
    with pytest.raises(ValueError):  # null pointer
        permute(oa=(0,))
    with pytest.raises(ValueError):  # A' on the table
        permute(oa=(0x2000,))
    with pytest.raises(ValueError):  # S' on the input
        permute(os_=(0x1000,))
    with pytest.raises(ValueError):  # A' and S' on one column
        permute(os_=(0x3000,))
    with pytest.raises(ValueError):  # the output of another pair
        permute(a=(0x1000, 0x5000), s=(0x2000, 0x2000), oa=(0x3000, 0x3000), os_=(0x4000, 0x8000))

    with pytest.raises(ValueError):  # rows are not 4 words
        ctx.lookup_permute(BN254, np.zeros((3, 3), np.uint64), np.zeros((3, 3), np.uint64), 2)
    with pytest.raises(ValueError):  # columns of different lengths
        ctx.lookup_permute(BN254, np.zeros((3, 4), np.uint64), np.zeros((4, 4), np.uint64), 2)
    with pytest.raises(ValueError):  # usable > n
        ctx.lookup_permute(BN254, np.zeros((3, 4), np.uint64), np.zeros((3, 4), np.uint64), 4)

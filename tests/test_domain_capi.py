"""CPU tests of the extended-domain entries at the C-ABI boundary (no device):
declared in the header, exported by the library, the header's aliasing rules,
argument errors with a null context or domain, and the Python wrappers' shape
checks (which run before the library is called)."""
import ctypes

import numpy as np
import pytest

import halo2_amd as H

ENTRIES = ["pm_domain_create", "pm_domain_info", "pm_domain_release", "pm_coeff_to_extended_device",
           "pm_extended_to_coeff_device", "pm_divide_by_vanishing_device", "pm_fft_batch_device",
           "pm_coeff_to_extended", "pm_extended_to_coeff"]
PM_ERR_ARG = -1


def test_entries_declared_and_exported():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name


def test_header_section_and_abi_version():
    txt = open(H.HEADER_PATH).read()
    assert "Extended-domain conversions" in txt
    sec = txt[txt.index("Extended-domain conversions"):txt.index("Blake2b transcript replay")]
    assert "d_out[c] may equal d_in[c]" in sec
    assert "must not overlap d_in[c]" in sec
    assert "may overlap another column's" in sec
    assert "the input is left unchanged" in sec
    assert "#define PM_EXT_DIVIDE_VANISHING 1u" in sec
    assert "PM_ERR_UNSUPPORTED" in sec and "256 MiB" in sec
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4
    assert H.EXT_DIVIDE_VANISHING == 1


def _u64(*shape):
    return np.zeros(shape, dtype=np.uint64)


def test_null_context_or_domain_is_an_argument_error():
    L = H.lib()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    p64 = lambda a: a.ctypes.data_as(u64p)  # noqa: E731
    ptrs = (ctypes.c_void_p * 1)(0x1000)
    w, z, buf = _u64(4), _u64(4), _u64(4, 4)
    h = ctypes.c_void_p()
    live = ctypes.c_void_p(0x2000)  # never dereferenced: the other handle is null
    assert L.pm_domain_create(None, 2, 2, 4, p64(w), p64(z), ctypes.byref(h)) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()
    assert L.pm_domain_info(None, None, None, None, None) == PM_ERR_ARG
    assert L.pm_domain_release(None) == 0
    for ctx, dom in ((None, live), (live, None), (None, None)):
        assert L.pm_coeff_to_extended_device(ctx, dom, ptrs, ptrs, 1) == PM_ERR_ARG
        assert L.pm_extended_to_coeff_device(ctx, dom, ptrs, ptrs, 1, 1, 0) == PM_ERR_ARG
        assert L.pm_divide_by_vanishing_device(ctx, dom, ptrs, 1) == PM_ERR_ARG
        assert L.pm_coeff_to_extended(ctx, dom, p64(buf), p64(buf)) == PM_ERR_ARG
        assert L.pm_extended_to_coeff(ctx, dom, p64(buf), 1, 0, p64(buf)) == PM_ERR_ARG
    assert L.pm_fft_batch_device(None, 2, ptrs, 1, 2, p64(w), None) == PM_ERR_ARG
    assert b"null" in L.pm_last_error()


def _detached():
    """A Context and a Domain without device objects behind them: the
    wrappers' shape checks raise before any library call, so none is made."""
    ctx = object.__new__(H.Context)
    ctx.h = None
    dom = object.__new__(H.Domain)
    dom.h = None
    dom.curve, dom.k, dom.extended_k, dom.n, dom.N = 2, 3, 5, 8, 32
    return ctx, dom


def test_wrappers_reject_mismatched_shapes():
    ctx, dom = _detached()
    with pytest.raises(ValueError):  # 2 inputs, 1 output
        ctx.coeff_to_extended_device(dom, [0x1000, 0x2000], [0x3000])
    with pytest.raises(ValueError):  # null column pointer
        ctx.coeff_to_extended_device(dom, [0x1000], [0])
    with pytest.raises(ValueError):  # 1 input, 2 outputs
        ctx.extended_to_coeff_device(dom, [0x1000], [0x2000, 0x3000], 8)
    with pytest.raises(ValueError):  # keep = 0
        ctx.extended_to_coeff_device(dom, [0x1000], [0x2000], 0)
    with pytest.raises(ValueError):  # keep = N + 1
        ctx.extended_to_coeff_device(dom, [0x1000], [0x2000], 33)
    with pytest.raises(ValueError):
        ctx.divide_by_vanishing_device(dom, [0])
    with pytest.raises(ValueError):  # omega is not one scalar
        ctx.fft_batch_device(2, [0x1000], 4, _u64(8))
    with pytest.raises(ValueError):  # scale is not one scalar
        ctx.fft_batch_device(2, [0x1000], 4, _u64(4), scale=_u64(3))
    with pytest.raises(ValueError):
        ctx.fft_batch_device(2, [0x1000], 29, _u64(4))
    with pytest.raises(ValueError):  # n = 8 coefficients expected
        ctx.coeff_to_extended(dom, _u64(7, 4))
    with pytest.raises(ValueError):  # N = 32 evaluations expected
        ctx.extended_to_coeff(dom, _u64(8, 4))
    with pytest.raises(ValueError):
        ctx.extended_to_coeff(dom, _u64(32, 4), keep=0)
    with pytest.raises(ValueError):  # extended_k < k
        H.Domain(ctx, 2, 5, 4, _u64(4), _u64(4))
    with pytest.raises(ValueError):  # zeta is not one scalar
        H.Domain(ctx, 2, 3, 5, _u64(4), _u64(8))

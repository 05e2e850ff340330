"""CPU tests of the quotient-numerator entries at the C-ABI boundary (no
device): declared in the header, exported by the library and bound, the
header's rules, argument errors with a null context, domain or shape, and the
Python wrappers' checks (which run before the library is called)."""
import ctypes

import numpy as np
import pytest

import accum as A
import halo2_amd as H
import pasta as P
import quotient_ref as Q

ENTRIES = ["pm_quotient_create", "pm_quotient_info", "pm_quotient_release", "pm_quotient_device",
           "pm_quotient_eval_host"]
PM_ERR_ARG = -1


def test_entries_declared_exported_and_bound():
    syms = H.header_symbols()
    L = ctypes.CDLL(H.LIB_PATH)
    for name in ENTRIES:
        assert name in syms, name
        assert hasattr(L, name), name
        assert getattr(H.lib(), name).argtypes, name


def test_header_section_and_abi_version():
    txt = open(H.HEADER_PATH).read()
    assert "Quotient numerator on the extended domain" in txt
    sec = txt[txt.index("Quotient numerator on the extended domain"):txt.index("Blake2b transcript replay")]
    assert txt.index("Extended-domain conversions") < txt.index("Quotient numerator on the extended domain")
    assert "col[(j + rot 2^e) mod N]" in sec and "rot may be negative" in sec
    assert "d_out must not overlap any input column" in sec
    assert "#define PM_QUOT_DIVIDE_VANISHING 1u" in sec and "#define PM_QUOT_ACCUMULATE       2u" in sec
    assert "PM_ERR_UNSUPPORTED" in sec and "28 value slots" in sec and "65536 ops" in sec
    assert "#define PM_ABI_VERSION 4" in txt and H.abi_version() == 4
    assert (H.QUOT_DIVIDE_VANISHING, H.QUOT_ACCUMULATE) == (1, 2)
    assert [f[0] for f in H.PmQuotientColumns._fields_] == list(H.QUOT_GROUPS)
    fields = sec[sec.index("typedef struct pm_quotient_columns"):sec.index("} pm_quotient_columns")]
    order = [fields.index("* %s;" % g) for g in H.QUOT_GROUPS]
    assert order == sorted(order)


def test_null_arguments_are_argument_errors():
    L = H.lib()
    u64p = ctypes.POINTER(ctypes.c_uint64)
    ch = np.zeros(16, dtype=np.uint64).ctypes.data_as(u64p)
    live = ctypes.c_void_p(0x2000)  # never dereferenced: another argument is null
    ps = Q.product_shape(2, A.simple_example_shape(P.CURVES[2], 4))
    cols = H.PmQuotientColumns()
    h = ctypes.c_void_p(0x77)
    for ctx, dom, shape in ((None, live, ps.c), (live, None, ps.c), (live, live, None)):
        assert L.pm_quotient_create(ctx, dom, shape, ctypes.byref(h)) == PM_ERR_ARG
        assert b"null" in L.pm_last_error()
    assert L.pm_quotient_create(live, live, ps.c, None) == PM_ERR_ARG
    assert L.pm_quotient_info(None, None, None, None, None, None) == PM_ERR_ARG
    assert L.pm_quotient_release(None) == 0
    for ctx, q, c, chp, out in ((None, live, cols, ch, live), (live, None, cols, ch, live), (live, live, None, ch, live),
                                (live, live, cols, None, live), (live, live, cols, ch, None)):
        assert L.pm_quotient_device(ctx, q, c, chp, 0, out) == PM_ERR_ARG
        assert b"null" in L.pm_last_error()
    assert L.pm_quotient_eval_host(2, None, 0, None, None, None, None) == PM_ERR_ARG
    assert L.pm_quotient_eval_host(2, ps.c, 1, None, ch, ch, ch) == PM_ERR_ARG
    assert L.pm_quotient_eval_host(7, ps.c, 0, None, None, None, None) == PM_ERR_ARG
    assert b"curve" in L.pm_last_error()


def _detached():
    """A Context, a Domain and a Quotient without device objects behind them:
    the wrappers' checks raise before any library call, so none is made."""
    ctx = object.__new__(H.Context)
    ctx.h = None
    dom = object.__new__(H.Domain)
    dom.h = None
    dom.curve, dom.k, dom.extended_k, dom.n, dom.N = 2, 4, 6, 16, 64
    q = object.__new__(H.Quotient)
    q.h = None
    q.curve, q.N = 2, 64
    ps = Q.product_shape(2, A.simple_example_shape(P.CURVES[2], 4))
    q.counts = H.quotient_column_counts(ps)
    return ctx, dom, q, ps


def test_wrappers_reject_bad_arguments():
    ctx, dom, q, ps = _detached()
    assert q.counts == dict(advice=2, fixed=4, instance=1, sigma=4, perm_z=2, lookup_a=1, lookup_s=1, lookup_z=1)
    good = {g: [0x1000 * (i + 1) + 0x100000 * k for i in range(c)] for k, (g, c) in enumerate(q.counts.items())}
    ch = np.zeros((4, 4), dtype=np.uint64)
    with pytest.raises(ValueError):  # one advice column short
        ctx.quotient_device(q, dict(good, advice=good["advice"][:1]), ch, 0x9000000)
    with pytest.raises(ValueError):  # a group left out that the shape has
        ctx.quotient_device(q, {g: p for g, p in good.items() if g != "sigma"}, ch, 0x9000000)
    with pytest.raises(ValueError):  # a group the ABI does not know
        ctx.quotient_device(q, dict(good, extra=[0x1000]), ch, 0x9000000)
    with pytest.raises(ValueError):  # null column pointer
        ctx.quotient_device(q, dict(good, fixed=[0x1000, 0, 0x3000, 0x4000]), ch, 0x9000000)
    with pytest.raises(ValueError):  # three challenges
        ctx.quotient_device(q, good, np.zeros((3, 4), dtype=np.uint64), 0x9000000)
    with pytest.raises(ValueError):  # null output
        ctx.quotient_device(q, good, ch, 0)
    with pytest.raises(ValueError):  # the output is an input column
        ctx.quotient_device(q, good, ch, good["perm_z"][1])
    with pytest.raises(ValueError):  # shape.log_n != k
        dom.k = 5
        H.Quotient(ctx, dom, ps)
    with pytest.raises(ValueError):  # another curve
        dom.k, dom.curve = 4, 0
        H.Quotient(ctx, dom, ps)
    with pytest.raises(ValueError):  # challenges: 16 words per point
        H.quotient_eval_host(ps, np.zeros((1, ps.layout()[1], 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64),
                             np.zeros((1, 12), dtype=np.uint64))
    with pytest.raises(ValueError):  # one scalar short
        H.quotient_eval_host(ps, np.zeros((1, ps.layout()[1] - 1, 4), dtype=np.uint64),
                             np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 16), dtype=np.uint64))

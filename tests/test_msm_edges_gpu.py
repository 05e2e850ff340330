"""Adversarial scalars and bases (tests/msm_edge_util.py) on every large-n MSM
path, each result bit for bit against the C port of best_multiexp
(oracle/msm_ref.c) on the same host arrays and, as a point, against the
known-discrete-log answer (expected_by_dlog).  No expected value comes from the
library under test.

Paths (each test asserts the structural fact that proves the path was taken):

  sorting pipeline, raw bases     msm_device, set_small_msm(0): 2^14 + 5 (one
                                  point per sort thread), 2^18 + 5 (two), forced
                                  windows 13 and 20
  8-row resident table            2^18 + 11: device scalars; host scalars through
                                  the two-part split copy and the one-copy
                                  schedule; a prefix; an offset window (plain
                                  pipeline on row 0); the drop-in pm_msm through
                                  the warm cache
  4-row / 2-row resident table    2^20 + 3 / 2^22 + 3 (three-part copy)
  automatic fixed table           c = 16 at 2^18 + 5; c = 20 (8-byte sort
                                  entries) at 2^21 + 77

Inputs: one mixed array per path (random scalars and bases with every special
scalar, base transform and collision group planted at rows 0, n - 1 and both
sides of every sort-block and scalar-part boundary) and whole arrays of each
constant and of the all-ones digit pattern.  The synthetic bases come from the
device generator (pinned to msm_ref.synth_bases by
test_msm_gpu.test_synth_on_device_matches_oracle; the host one costs a scalar
multiplication per base); everything after that is built on the host and goes
up as host arrays.
"""
import numpy as np
import pytest

import halo2_amd as H
import msm_edge_util as E
import msm_ref
import pasta as P

pytestmark = pytest.mark.gpu

N_RAW_SMALL = (1 << 14) + 5
N_RAW = (1 << 18) + 5
N_ROWS8 = (1 << 18) + 11
N_ROWS4 = (1 << 20) + 3
N_ROWS2 = (1 << 22) + 3
N_FIXED20 = (1 << 21) + 77

_BASES = {}
_CASES = {}


def _synth_bases(ctx, curve, n):
    """Host copy of the first n synthetic bases (seed SEED_BASES), generated
    on the device; up to N_ROWS8 one array per curve serves every prefix."""
    import torch

    m = max(n, N_ROWS8)
    if (curve, m) not in _BASES:
        b = torch.empty((m, 8), dtype=torch.int64, device=torch.device("cuda", ctx.device))
        ctx.synth_bases(curve, P.SEED_BASES, 0, m, b.data_ptr())
        torch.cuda.synchronize()
        hb = b.cpu().numpy().view(np.uint64)
        if m > N_ROWS8:
            return hb[:n]
        hb.setflags(write=False)
        _BASES[(curve, m)] = hb
    return _BASES[(curve, m)][:n]


class Case:
    def __init__(self, curve, name, S, B, D):
        self.curve, self.name, self.S = curve, name, S
        self.want = msm_ref.best_multiexp(curve, S, B)          # the C port, on the same host arrays
        self.point = E.expected_by_dlog(curve, S, D)            # [sum s_i dlog_i] G
        S.setflags(write=False)

    def check(self, got, tag=""):
        assert np.array_equal(got, self.want), (self.name, tag)
        assert P.limbs_to_point(P.CURVES[self.curve], [int(x) for x in got]) == self.point, (self.name, tag)


class Inputs:
    """The mixed input of one path (and the whole-array scalars over its
    bases), with both references' answers computed once."""

    def __init__(self, ctx, curve, n, c, rows, table, whole):
        self.curve, self.n = curve, n
        S, B, D, self.planted = E.mixed_case(curve, n, c, rows, table, bases=_synth_bases(ctx, curve, n))
        kinds = {k for k, _, _ in self.planted}
        assert kinds >= set(E.GADGETS) | {f"group{g}" for g in E.GROUPS}
        assert {nm for _, _, nm in self.planted} >= {nm for nm, _ in E.special_scalars(curve, c, rows)}
        at = {r for _, rws, _ in self.planted for r in rws}
        assert all(b - 1 in at and b in at for b in E.boundaries(n, table) + [1, n - 1])
        self.B, self.D = B, D
        B.setflags(write=False)
        self.cases = [Case(curve, "mixed", S, B, D)]
        self.cases += [Case(curve, nm, E.whole_array_case(curve, n, nm, c), B, D) for nm in whole]
        self.mixed = self.cases[0]


def _inputs(ctx, curve, n, c, rows=1, table=False, whole=E.WHOLE_ARRAY_GPU, keep=True):
    key = (curve, n, c, rows, table, tuple(whole))
    if key in _CASES:
        return _CASES[key]
    inp = Inputs(ctx, curve, n, c, rows, table, whole)
    if keep:
        _CASES[key] = inp
    return inp


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to(torch.device("cuda", ctx.device))


# ------------------------------------------------ sorting pipeline, raw bases
@pytest.mark.parametrize("curve", [0, 2])
@pytest.mark.parametrize("n,ppt,c", [(N_RAW_SMALL, 1, 12), (N_RAW, 2, 16)])
def test_raw_pipeline(gpu_ctx, curve, n, ppt, c):
    """msm_device through the sorting pipeline (small-MSM path off) at the
    plan's automatic width: one point per sort thread, and the first size with
    two; canonical scalars give the same answer."""
    import pipeline_model as PM

    assert E.sort_ppt(n) == ppt and PM.make_plan(n)["c"] == c
    inp = _inputs(gpu_ctx, curve, n, c)
    b = _dev(gpu_ctx, inp.B)
    gpu_ctx.set_small_msm(0)
    try:
        for case in inp.cases:
            s = _dev(gpu_ctx, case.S)
            case.check(gpu_ctx.msm_device(curve, s.data_ptr(), b.data_ptr(), n))
        sc = _dev(gpu_ctx, E.canonical(curve, inp.mixed.S))
        inp.mixed.check(gpu_ctx.msm_device(curve, sc.data_ptr(), b.data_ptr(), n, canonical=True), "canonical")
    finally:
        gpu_ctx.set_small_msm(H.SMALL_MSM_DEFAULT)


@pytest.mark.parametrize("curve", [0, 2])
@pytest.mark.parametrize("c,W", [(13, 20), (20, 13)])
def test_raw_pipeline_forced_window(gpu_ctx, curve, c, W):
    """msm_device with a forced window of 13 (20 windows of 12-13 bits) and of
    20 (13 windows of 19-20 bits: 32-bit digit codes), digit patterns of that
    width."""
    n = N_RAW
    assert E.win_geom(c)[0] == W
    inp = _inputs(gpu_ctx, curve, n, c, whole=("const:r-1", "pattern:ones"))
    b = _dev(gpu_ctx, inp.B)
    gpu_ctx.set_small_msm(0)
    gpu_ctx.set_window(c)
    try:
        for case in inp.cases:
            s = _dev(gpu_ctx, case.S)
            case.check(gpu_ctx.msm_device(curve, s.data_ptr(), b.data_ptr(), n), c)
    finally:
        gpu_ctx.set_window(0)
        gpu_ctx.set_small_msm(H.SMALL_MSM_DEFAULT)


# ------------------------------------------------------ 8-row resident table
def _rows8(ctx, curve, whole=E.WHOLE_ARRAY_GPU):
    return _inputs(ctx, curve, N_ROWS8, 16, rows=8, table=True, whole=whole)


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_rows8_device_scalars(gpu_ctx, curve):
    """upload_bases + msm_resident_device on the 8-row table ([2^{32 j}] P);
    Vesta runs the mixed input only; canonical scalars give the same answer."""
    inp = _rows8(gpu_ctx, curve, whole=() if curve == 1 else E.WHOLE_ARRAY_GPU)
    rb = gpu_ctx.upload_bases(curve, inp.B)
    try:
        assert rb.rows == 8
        for case in inp.cases:
            s = _dev(gpu_ctx, case.S)
            case.check(gpu_ctx.msm_resident_device(rb, 0, s.data_ptr(), inp.n))
        sc = _dev(gpu_ctx, E.canonical(curve, inp.mixed.S))
        inp.mixed.check(gpu_ctx.msm_resident_device(rb, 0, sc.data_ptr(), inp.n, canonical=True), "canonical")
    finally:
        rb.release()


@pytest.mark.parametrize("curve", [0, 2])
@pytest.mark.parametrize("split", [-1, 0])
def test_rows8_host_scalars(gpu_ctx, curve, split):
    """msm_resident with host scalars on the 8-row table: split = -1 the
    two-part split copy (3/8 + 5/8, special rows on both sides of the cut),
    split = 0 the one-copy schedule (MSM_OPT_SPLIT_COPY = 0)."""
    inp = _rows8(gpu_ctx, curve)
    assert inp.n >= H.SPLIT_COPY_MIN_N and E.part_starts(inp.n, True) == [0, 106496, inp.n]
    at = {r for _, rws, _ in inp.planted for r in rws}
    assert {106495, 106496} <= at
    rb = gpu_ctx.upload_bases(curve, inp.B)
    gpu_ctx.set_msm_option(H.MSM_OPT_SPLIT_COPY, split)
    try:
        assert rb.rows == 8
        for case in inp.cases:
            case.check(gpu_ctx.msm_resident(rb, 0, case.S), split)
        inp.mixed.check(gpu_ctx.msm_resident(rb, 0, E.canonical(curve, inp.mixed.S), canonical=True), "canonical")
    finally:
        gpu_ctx.set_msm_option(H.MSM_OPT_SPLIT_COPY, -1)
        rb.release()


@pytest.mark.parametrize("curve", [0, 2])
def test_rows8_prefix_and_offset(gpu_ctx, curve):
    """The same table over its first n / 2 + 17 points and over a window at
    offset 5, device and host scalars.  Both run the plain pipeline on row 0
    of the table: the offset window by rule, the prefix because it is shorter
    than the row-table path's 2^18 points (resident_use_table in capi_internal.hpp; a
    prefix that stays on the row table: test_rows4)."""
    inp = _rows8(gpu_ctx, curve)
    n, S, B, D = inp.n, inp.mixed.S, inp.B, inp.D
    m = n // 2 + 17
    assert E.part_starts(m, True) == [0, m]   # below 2^18 points: no row-table path, no split copy
    pre = Case(curve, "prefix", S[:m].copy(), B[:m], D[:m])
    off = Case(curve, "offset", S[:m].copy(), B[5:5 + m], D[5:5 + m])
    rb = gpu_ctx.upload_bases(curve, B)
    try:
        assert rb.rows == 8
        s = _dev(gpu_ctx, S[:m])
        pre.check(gpu_ctx.msm_resident_device(rb, 0, s.data_ptr(), m), "device")
        pre.check(gpu_ctx.msm_resident(rb, 0, S[:m]), "host")
        off.check(gpu_ctx.msm_resident_device(rb, 5, s.data_ptr(), m), "device")
        off.check(gpu_ctx.msm_resident(rb, 5, S[:m]), "host")
    finally:
        rb.release()


@pytest.mark.parametrize("curve", [0, 2])
def test_rows8_dropin_warm_cache(curve):
    """pm_msm (host scalars + host bases) once the drop-in cache holds the set
    as a row table: the third call hits, and so does every later scalar set."""
    ctx = H.Context(0)
    try:
        inp = _rows8(ctx, curve)
        B = np.array(inp.B)
        for _ in range(3):
            inp.mixed.check(ctx.msm(curve, inp.mixed.S, B))
        st = ctx.dropin_stats()
        assert st["hits"] == 1 and st["misses"] == 2 and st["entries"] == 1
        for case in inp.cases[1:]:
            case.check(ctx.msm(curve, case.S, B), "warm")
        assert ctx.dropin_stats()["hits"] == len(inp.cases) and ctx.dropin_stats()["misses"] == 2
    finally:
        ctx.close()


# ----------------------------------------------- 4-row and 2-row resident tables
def test_rows4(gpu_ctx):
    """upload_bases at 2^20 + 3 keeps 4 rows ([2^{64 j}] P): device scalars and
    host scalars (two-part copy), and a prefix of just over half of the padded
    table, which stays on the row-table path; Pallas."""
    inp = _inputs(gpu_ctx, 0, N_ROWS4, 16, rows=4, table=True, whole=("const:r-1", "pattern:ones"), keep=False)
    rb = gpu_ctx.upload_bases(0, inp.B)
    try:
        assert rb.rows == 4 and len(E.part_starts(inp.n, True)) == 3
        for case in inp.cases:
            s = _dev(gpu_ctx, case.S)
            case.check(gpu_ctx.msm_resident_device(rb, 0, s.data_ptr(), inp.n), "device")
            case.check(gpu_ctx.msm_resident(rb, 0, case.S), "host")
        npad = (inp.n + E.SORT_B - 1) // E.SORT_B * E.SORT_B
        m = npad // 2 + 17
        assert m >= 1 << 18 and 2 * m >= npad   # resident_use_table: the row-table path
        pre = Case(0, "prefix", inp.mixed.S[:m].copy(), inp.B[:m], inp.D[:m])
        s = _dev(gpu_ctx, pre.S)
        pre.check(gpu_ctx.msm_resident_device(rb, 0, s.data_ptr(), m), "device")
        pre.check(gpu_ctx.msm_resident(rb, 0, pre.S), "host")
    finally:
        rb.release()


def test_rows2(gpu_ctx):
    """upload_bases at 2^22 + 3 keeps 2 rows ([2^{128}] P beside P): the mixed
    input with device scalars and with host scalars (three-part copy: special
    rows on both sides of the 1/4 and 5/8 cuts), Pallas."""
    inp = _inputs(gpu_ctx, 0, N_ROWS2, 16, rows=2, table=True, whole=(), keep=False)
    ps = E.part_starts(inp.n, True)
    assert ps == [0, 1 << 20, (5 << 19) + E.SORT_B, inp.n]
    at = {r for _, rws, _ in inp.planted for r in rws}
    assert all({p - 1, p} <= at for p in ps[1:3])
    rb = gpu_ctx.upload_bases(0, inp.B)
    try:
        assert rb.rows == 2
        s = _dev(gpu_ctx, inp.mixed.S)
        inp.mixed.check(gpu_ctx.msm_resident_device(rb, 0, s.data_ptr(), inp.n), "device")
        inp.mixed.check(gpu_ctx.msm_resident(rb, 0, inp.mixed.S), "host")
    finally:
        rb.release()


# ------------------------------------------------------- automatic fixed table
@pytest.mark.parametrize("curve", [0, 2])
def test_fixed_c16(gpu_ctx, curve):
    """fixed_bases(...) with the automatic width 16 at 2^18 + 5 (one table
    row per window, so the row patterns sit in single windows): device and
    host scalars, canonical scalars."""
    inp = _inputs(gpu_ctx, curve, N_RAW, 16, rows=16, table=True)
    fb = gpu_ctx.fixed_bases(curve, inp.B)
    try:
        assert fb.c == 16 and fb.windows == 16 and fb.n == inp.n
        for case in inp.cases:
            s = _dev(gpu_ctx, case.S)
            case.check(fb.msm_device(s.data_ptr(), inp.n), "device")
            case.check(fb.msm(case.S), "host")
        inp.mixed.check(fb.msm(E.canonical(curve, inp.mixed.S), canonical=True), "canonical")
    finally:
        fb.release()


def test_fixed_c20(gpu_ctx):
    """fixed_bases(...) past 2^21 points: automatic width 20, 13 windows,
    8-byte sort entries; the mixed input (digit patterns of width 20, also
    confined to each single window) with device and host scalars, Pallas."""
    inp = _inputs(gpu_ctx, 0, N_FIXED20, 20, rows=13, table=True, whole=(), keep=False)
    fb = gpu_ctx.fixed_bases(0, inp.B)
    try:
        assert fb.c == 20 and fb.windows == 13
        s = _dev(gpu_ctx, inp.mixed.S)
        inp.mixed.check(fb.msm_device(s.data_ptr(), inp.n), "device")
        inp.mixed.check(fb.msm(inp.mixed.S), "host")
    finally:
        fb.release()

"""Adversarial scalars and bases (tests/msm_short_edge_util.py) on the SHORT
MSM paths, each result bit for bit against the C port of best_multiexp
(oracle/msm_ref.c) on the same host arrays and, as a point, against the
known-discrete-log answer (expected_by_dlog).  No expected value comes from the
library under test.  The large-n paths: test_msm_edges_gpu.py.

Paths (each test asserts the structural fact that proves the path was taken:
the kernel stats of a timed run, or the window width of many_info()):

  k_small_fused                n = 1, 2, 16, 17, 32, all three curves: as many
                               mixed cases as it takes to plant every GLV
                               special scalar, the GLV collision (n = 2, 16, 32)
  k_small_table + k_small_sum  n = 33, 300, 2047 (kq = 1, 2, 8), all three curves
  k_small_table + k_small_sum_lanes   n = 2048, 4097, Pallas and BN254
      each through msm (host arrays), msm_device and msm_resident at an offset
      (bases in the R = 2^261 form), Montgomery and canonical scalars; on the
      table paths also whole arrays of r - 1 and of the all-8 halves, every
      base equal, and the GLV collision with phi(P) and with -phi(P)
  many-MSM, c = 7, 6, 5, 4     prefixes of 6000 / 8192 / 16384 / 32768 bases,
                               Pallas and BN254 (Vesta: c = 7): a call with
                               kq = 1 and one with kq > 1 that does not divide
                               W; host, device and canonical (some >= r) scalars
  many-MSM growth              c = 8 on 64 bases, then c = 6 on 8192
  many-MSM fallback            131073 bases: no table, one resident MSM each
  small-set drop-in cache      n = 5, 32, 64 through msm four times

The synthetic bases come from the device generator (pinned to
msm_ref.synth_bases by test_msm_gpu.test_synth_on_device_matches_oracle);
everything after that is built on the host and goes up as host arrays.
"""
import numpy as np
import pytest

import halo2_amd as H
import msm_edge_util as E
import msm_ref
import msm_short_edge_util as U
import pasta as P

pytestmark = pytest.mark.gpu

_BASES = {}
_DLOGS = {}


def _synth_bases(ctx, curve, n):
    """Host copies of the first n synthetic bases (seed SEED_BASES, generated
    on the device) and of their discrete logs."""
    import torch

    if curve not in _BASES or _BASES[curve].shape[0] < n:
        m = max(n, 32768)
        b = torch.empty((m, 8), dtype=torch.int64, device=torch.device("cuda", ctx.device))
        ctx.synth_bases(curve, P.SEED_BASES, 0, m, b.data_ptr())
        torch.cuda.synchronize()
        _BASES[curve] = b.cpu().numpy().view(np.uint64)
        _DLOGS[curve] = msm_ref.synth_scalars(curve, P.SEED_BASES, 0, m)
        _BASES[curve].setflags(write=False)
        _DLOGS[curve].setflags(write=False)
    return _BASES[curve][:n], _DLOGS[curve][:n]


def _dev(ctx, a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint64).view(np.int64)).to(torch.device("cuda", ctx.device))


def _above_r(curve, Sc):
    """Canonical scalars with j r added to row i (j = i mod 4) where that
    stays below 2^256: the same MSM."""
    r = P.CURVES[curve].r
    v = E.to_ints(Sc)
    return E.to_limbs([int(k) + (i & 3) * r if int(k) + (i & 3) * r < 1 << 256 else int(k) for i, k in enumerate(v)])


class Case:
    def __init__(self, curve, name, S, B, D):
        self.curve, self.name, self.S, self.B = curve, name, np.ascontiguousarray(S), np.ascontiguousarray(B)
        self.n = self.S.shape[0]
        self.want = msm_ref.best_multiexp(curve, self.S, self.B)      # the C port, on the same host arrays
        self.point = E.expected_by_dlog(curve, self.S, D)             # [sum s_i dlog_i] G
        self.Sc = E.canonical(curve, self.S)

    def check(self, got, tag=""):
        assert np.array_equal(got, self.want), (self.name, tag)
        assert P.limbs_to_point(P.CURVES[self.curve], [int(x) for x in got]) == self.point, (self.name, tag)


def _ran(ctx, path):
    fused, table, ssum = (ctx.kernel_stats(k)[0] for k in ("small_fused", "small_table", "small_sum"))
    return (fused == 1 and table == 0 and ssum == 0) if path == "fused" else (fused == 0 and table == 1 and ssum == 1)


FILL = 5   # rows in front of a case's bases in its resident set


def _run_entries(ctx, case, path, prove):
    """The case through msm (host scalars and bases), msm_device and
    msm_resident / msm_resident_device at offset FILL, Montgomery and
    canonical scalars.  prove: a timed run first, whose kernel stats show that
    `path` ran (the other runs wait on the completion flag, as untimed calls do)."""
    curve, n = case.curve, case.n
    assert U.small_geom(n)[0] == path
    ds, dsc, db = _dev(ctx, case.S), _dev(ctx, case.Sc), _dev(ctx, case.B)
    fill = _synth_bases(ctx, curve, FILL)[0]
    rb = ctx.upload_bases(curve, np.concatenate([fill, case.B]))
    try:
        if prove:
            ctx.set_timing(True)
            try:
                for f in (lambda: ctx.msm(curve, case.S, case.B), lambda: ctx.msm_device(curve, ds.data_ptr(), db.data_ptr(), n),
                          lambda: ctx.msm_resident(rb, FILL, case.S)):
                    ctx.dropin_clear()   # a small set seen twice would run on the many path
                    ctx.reset_stats()
                    case.check(f(), "timed")
                    assert _ran(ctx, path), (case.name, path)
            finally:
                ctx.set_timing(False)
        ctx.dropin_clear()
        case.check(ctx.msm(curve, case.S, case.B), "msm")
        ctx.dropin_clear()
        case.check(ctx.msm(curve, _above_r(curve, case.Sc), case.B, canonical=True), "msm canonical")
        case.check(ctx.msm_device(curve, ds.data_ptr(), db.data_ptr(), n), "device")
        case.check(ctx.msm_device(curve, dsc.data_ptr(), db.data_ptr(), n, canonical=True), "device canonical")
        case.check(ctx.msm_resident(rb, FILL, case.S), "resident")
        case.check(ctx.msm_resident(rb, FILL, case.Sc, canonical=True), "resident canonical")
        case.check(ctx.msm_resident_device(rb, FILL, ds.data_ptr(), n), "resident device")
    finally:
        rb.release()


def _mixed_cases(ctx, curve, n, path):
    B, D = _synth_bases(ctx, curve, n)
    names, out = set(), []
    for rot in U.covering_rots(curve, n, path):
        S, b, d, planted = U.short_mixed_case(curve, n, path, rot=rot, bases=B)
        names |= {nm for _, _, nm in planted}
        out.append((Case(curve, f"mixed{rot}", S, b, d), planted))
    assert names == {nm for nm, _, _ in U.glv_special_scalars(curve)}
    return out


def _collision_cases(ctx, curve, n):
    B, _ = _synth_bases(ctx, curve, n)
    out = []
    for pat in ("7..78", "8..8"):
        for negate in (False, True):
            c = Case(curve, f"collision:{pat}:{negate}", *U.glv_collision_case(curve, n, pat, negate, bases=B))
            assert (c.point is None) == negate and c.want.any() != negate
            out.append(c)
    return out


# ------------------------------------------------------------------ k_small_fused
@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 16, 17, 32])
def test_fused(gpu_ctx, curve, n):
    """n <= 32: one block per window (n = 32: exactly 64 terms), one quad per
    term.  Gadget pairs sit pow2(2 n) / 4 rows apart, so equal and opposite
    bases meet as raw affine points at the first tree level."""
    cases = _mixed_cases(gpu_ctx, curve, n, "fused")
    kinds = {k for _, pl in cases for k, _, _ in pl}
    assert n == 1 or kinds >= {"dup", "neg", "identity", "phi", "phi-neg", "phi2"}
    for i, (case, _) in enumerate(cases):
        _run_entries(gpu_ctx, case, "fused", prove=i == 0)
    if n in (2, 16, 32):
        for case in _collision_cases(gpu_ctx, curve, n):
            _run_entries(gpu_ctx, case, "fused", prove=False)


# ------------------------------------------------------- table + quads / lanes
def _table_path(ctx, curve, n, path, kq):
    assert U.small_geom(n)[:2] == (path, kq)
    cases = _mixed_cases(ctx, curve, n, path)
    for case, planted in cases:
        assert n == 33 or {k for k, _, _ in planted} >= set(U.SMALL_GADGETS) | {"run"}
    if n == 33:   # one pair per case (rows 0 and 32): between them every gadget
        assert {k for _, pl in cases for k, _, _ in pl} >= set(U.SMALL_GADGETS)
    for i, (case, _) in enumerate(cases):
        _run_entries(ctx, case, path, prove=i == 0)
    B0, D0 = _synth_bases(ctx, curve, n)
    whole = [Case(curve, nm, U.whole_array_case(curve, n, nm), B0, D0) for nm in ("const:r-1", "glv:+8..8,+8..8")]
    # every base equal, under the mixed scalars
    whole.append(Case(curve, "one base", cases[0][0].S, np.repeat(B0[:1], n, axis=0), np.repeat(D0[:1], n, axis=0)))
    for case in whole + _collision_cases(ctx, curve, n):
        _run_entries(ctx, case, path, prove=False)


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("n,kq", [(33, 1), (300, 2), (2047, 8)])
def test_table_quads(gpu_ctx, curve, n, kq):
    """k_small_table + k_small_sum: gadget pairs 64 terms apart, inside one
    quad's serial accumulation (kq > 1) and across the slice cuts; 2047 is the
    largest n below the lanes kernel."""
    _table_path(gpu_ctx, curve, n, "quads", kq)


@pytest.mark.parametrize("curve", [0, 2])
@pytest.mark.parametrize("n,kq", [(2048, 2), (4097, 5)])
def test_table_lanes(gpu_ctx, curve, n, kq):
    """k_small_table + k_small_sum_lanes (one-lane xyzz29_add): gadget pairs
    256 terms apart."""
    _table_path(gpu_ctx, curve, n, "lanes", kq)


# ------------------------------------------------------------------ many-MSM
class Batch:
    """One many-MSM call: its mixed cases and both references' answers."""

    def __init__(self, curve, c, ns, offs, B, D, seed=0):
        self.curve, self.ns, self.offs = curve, ns, offs
        self.S, self.planted = U.many_batch_case(curve, c, ns, offs, B, D, seed)
        self.B, self.D = B, D

    def references(self):
        """after the base set took its final form"""
        self.cases, s0 = [], 0
        for i, (n, o) in enumerate(zip(self.ns, self.offs)):
            self.cases.append(Case(self.curve, f"msm{i}", self.S[s0:s0 + n], self.B[o:o + n], self.D[o:o + n]))
            s0 += n
        self.Sc = _above_r(self.curve, E.canonical(self.curve, self.S))

    def check(self, got, tag):
        assert got.shape == (len(self.ns), 8)
        for i, case in enumerate(self.cases):
            case.check(got[i], tag)


@pytest.mark.parametrize("curve,nb,c", [(0, 6000, 7), (1, 6000, 7), (2, 6000, 7), (0, 8192, 6), (2, 8192, 6),
                                        (0, 16384, 5), (2, 16384, 5), (0, 32768, 4), (2, 32768, 4)])
def test_many_width(gpu_ctx, curve, nb, c):
    """The multiples table of a prefix that needs a window below 8 bits
    (digits that straddle two 32-bit words for c = 7, 6, 5; the carry window of
    c = 5; bits past 255 in the last window) and k_many_sum on it."""
    W, H_ = U.many_geom(c)
    assert U.many_pick_c(nb) == c
    b0, d0 = _synth_bases(gpu_ctx, curve, nb)
    B, D = b0.copy(), d0.copy()
    batches = [Batch(curve, c, *U.many_batch(nb, c, big), B, D, seed=17 * big) for big in (False, True)]
    kinds = set()
    for bt, big in zip(batches, (False, True)):
        bt.references()
        kq = U.many_kq(bt.ns, c)
        assert (kq > 1 and W % kq and kq < W) if big else kq == 1
        assert max(o + n for o, n in zip(bt.offs, bt.ns)) == nb and min(bt.ns) == 1 and max(bt.ns) >= 100
        kinds |= {k for _, k, _, _ in bt.planted}
        assert {nm for _, _, _, nm in bt.planted} >= {nm for nm, _ in U.many_special_scalars(curve, c)}
    assert kinds >= set(U.MANY_GADGETS) | ({"pow"} if W & (W - 1) else set())
    rb = gpu_ctx.upload_bases(curve, B)
    try:
        gpu_ctx.bases_many_prepare(rb, nb)
        assert rb.many_info() == (nb, c, nb * W * H_ * 128)
        for bt in batches:
            bt.check(gpu_ctx.msm_resident_many(rb, bt.ns, bt.S, offsets=bt.offs), "host")
            d = _dev(gpu_ctx, bt.S)
            bt.check(gpu_ctx.msm_resident_many_device(rb, bt.ns, d.data_ptr(), offsets=bt.offs), "device")
            bt.check(gpu_ctx.msm_resident_many(rb, bt.ns, bt.Sc, offsets=bt.offs, canonical=True), "canonical")
        assert rb.many_info()[:2] == (nb, c)
    finally:
        rb.release()   # a table is up to 2 GiB


def test_many_growth(gpu_ctx):
    """A first call within 64 bases builds the table at c = 8; a call reaching
    base 5000 rebuilds it for min(8192, the set) bases at c = 6; both calls
    repeated on the new table are still exact."""
    curve, nb = 0, 8192
    b0, d0 = _synth_bases(gpu_ctx, curve, nb)
    B, D = b0.copy(), d0.copy()
    first = Batch(curve, 8, [1, 7, 16, 31, 9], [0, 1, 8, 24, 55], B, D)
    second = Batch(curve, 6, [1, 300, 64, 600], [64, 100, 1000, 4400], B, D, seed=3)
    first.references()
    second.references()
    assert U.many_pick_c(64) == 8 and U.many_pick_c(8192) == 6
    rb = gpu_ctx.upload_bases(curve, B)
    try:
        assert rb.many_info() == (0, 0, 0)
        first.check(gpu_ctx.msm_resident_many(rb, first.ns, first.S, offsets=first.offs), "c = 8")
        assert rb.many_info()[:2] == (64, 8)
        second.check(gpu_ctx.msm_resident_many(rb, second.ns, second.S, offsets=second.offs), "c = 6")
        assert rb.many_info() == (8192, 6, 8192 * U.many_bytes_per_base(6))
        first.check(gpu_ctx.msm_resident_many(rb, first.ns, first.S, offsets=first.offs), "c = 8 inputs at c = 6")
        second.check(gpu_ctx.msm_resident_many(rb, second.ns, second.S, offsets=second.offs), "again")
        d = _dev(gpu_ctx, first.S)
        first.check(gpu_ctx.msm_resident_many_device(rb, first.ns, d.data_ptr(), offsets=first.offs), "device")
        assert rb.many_info()[:2] == (8192, 6)
    finally:
        rb.release()


def test_many_fallback(gpu_ctx):
    """131073 bases: one more than any multiples table holds.  A batch whose
    windows reach the last base gets no table (many_info() stays zero) and
    runs one resident MSM per entry: k_small_fused (n = 1), table + quads
    (n = 40) and the sorting pipeline (n = 20000), host and device scalars."""
    import pipeline_model as PM

    curve, nb = 0, 131073
    assert nb * U.many_bytes_per_base(4) > U.many_budget()[1] >= (nb - 1) * U.many_bytes_per_base(4)
    ns, offs = [1, 40, 20000, 1], [7, 100, nb - 20000, nb - 1]
    assert ns[2] > H.SMALL_MSM_DEFAULT and offs[2] + ns[2] == nb
    b0, d0 = _synth_bases(gpu_ctx, curve, nb)
    # the long window's rows are the set's first 20000 bases again (the
    # large-n generator numbers its dlogs from base 0)
    S2, B2, D2, planted = E.mixed_case(curve, ns[2], PM.make_plan(ns[2])["c"], bases=b0[:ns[2]])
    assert {k for k, _, _ in planted} >= set(E.GADGETS)
    B, D = b0.copy(), d0.copy()
    B[offs[2]:], D[offs[2]:] = B2, D2
    parts = [U.short_mixed_case(curve, 1, "fused", bases=B[7:8], dlogs=D[7:8]),
             U.short_mixed_case(curve, 40, "quads", bases=B[100:140], dlogs=D[100:140]),
             (S2, B2, D2, planted),
             U.short_mixed_case(curve, 1, "fused", rot=5, bases=B[nb - 1:], dlogs=D[nb - 1:])]
    for (s, b, d, _), n, o in zip(parts, ns, offs):
        B[o:o + n], D[o:o + n] = b, d
    cases = [Case(curve, f"msm{i}", p[0], B[o:o + n], D[o:o + n]) for i, (p, n, o) in enumerate(zip(parts, ns, offs))]
    S = np.concatenate([c.S for c in cases])
    rb = gpu_ctx.upload_bases(curve, B)
    try:
        got = gpu_ctx.msm_resident_many(rb, ns, S, offsets=offs)
        assert rb.many_info() == (0, 0, 0)
        d = _dev(gpu_ctx, S)
        got_d = gpu_ctx.msm_resident_many_device(rb, ns, d.data_ptr(), offsets=offs)
        got_c = gpu_ctx.msm_resident_many(rb, ns, E.canonical(curve, S), offsets=offs, canonical=True)
        assert rb.many_info() == (0, 0, 0)
        for i, case in enumerate(cases):
            case.check(got[i], "host")
            case.check(got_d[i], "device")
            case.check(got_c[i], "canonical")
        with pytest.raises(H.PmError):   # no table for this prefix
            gpu_ctx.bases_many_prepare(rb, nb)
    finally:
        rb.release()


# ----------------------------------------------------- small-set drop-in cache
@pytest.mark.parametrize("curve", [0, 2])
def test_small_set_dropin_cache_edges(curve):
    """msm (host arrays) four times with one small base set on a fresh
    context: first sighting on the small path, admission, then two hits: the
    last three run as one MSM of the many path at c = 8."""
    ctx = H.Context(0)
    try:
        for k, n in enumerate((5, 32, 64), 1):
            B, _ = _synth_bases(ctx, curve, n)
            path = U.small_geom(n)[0]
            S, b, d, planted = U.short_mixed_case(curve, n, path, rot=11 * k, bases=B)
            # five rows hold one pair (rows 0 and 4), the larger sets every gadget
            assert {kd for kd, _, _ in planted} >= ({"neg", "identity", "phi", "phi-neg"} if n >= 32 else {"phi"})
            case = Case(curve, f"n{n}", S, b, d)
            coll = Case(curve, f"collision{n}", *U.glv_collision_case(curve, n, "7..78", bases=B))
            assert np.array_equal(coll.B, U.glv_collision_case(curve, n, "8..8", bases=B)[1])
            coll2 = Case(curve, f"collision{n}b", U.glv_collision_case(curve, n, "8..8", bases=B)[0], coll.B,
                         U.glv_collision_case(curve, n, "8..8", bases=B)[2])
            ctx.set_timing(True)
            for i in range(4):
                ctx.reset_stats()
                if i < 3:
                    case.check(ctx.msm(curve, case.S, case.B), i)
                else:
                    case.check(ctx.msm(curve, _above_r(curve, case.Sc), case.B, canonical=True), "canonical")
                assert (ctx.kernel_stats("many_sum")[0] == 1) == (i > 0), (n, i)
                assert _ran(ctx, path) == (i == 0), (n, i)
            ctx.set_timing(False)
            st = ctx.dropin_small_stats()
            assert st["admitted"] == 2 * k - 1 and st["hits"] == 4 * k - 2 and st["entries"] == 2 * k - 1, st
            # a second set of the same size (the GLV collision's bases), new scalars on the hit
            coll.check(ctx.msm(curve, coll.S, coll.B), "first")
            coll.check(ctx.msm(curve, coll.S, coll.B), "admitted")
            coll2.check(ctx.msm(curve, coll2.S, coll2.B), "hit")
            coll.check(ctx.msm(curve, coll.S, coll.B), "hit")
            st = ctx.dropin_small_stats()
            assert st["admitted"] == 2 * k and st["hits"] == 4 * k and st["entries"] == 2 * k, st
        assert ctx.dropin_stats()["entries"] == 0   # the large-set cache is untouched
    finally:
        ctx.close()

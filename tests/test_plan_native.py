"""The Python mirrors of the drivers' host plans against the plans themselves.

The GPU edge tests place their inputs on boundaries computed by Python
restatements of the host planning (pipeline_model.make_plan, msm_edge_util,
msm_short_edge_util, accum_edge_util).  tests/native/plan_dump.cpp prints what
csrc/msm_plan.hpp and csrc/accum_plan.hpp compute (the functions the drivers
call), and every mirror and every hand-copied constant is compared with it
here: over n = 2^k, 2^k +- 1 for k = 0 .. 26, the sizes the GPU tests use,
every forced window in kMinC .. kMaxC, and for the accumulator B = 1 .. 4096
at the term counts of the shapes in shape_util, with the split and the terms
per lane automatic and forced.  No GPU."""
import functools

import pytest

import accum_edge_util as X
import msm_edge_util as E
import msm_short_edge_util as U
import pasta as P
import pipeline_model as M
import plan_native as N
import shape_util as S

MANY_PREFIX = U.MANY_PREFIX


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return N.build(tmp_path_factory)


@pytest.fixture(scope="module")
def consts(exe):
    return N.ask1(exe, "consts")


def sweep_sizes():
    ns = {(1 << k) + d for k in range(27) for d in (-1, 0, 1)}
    ns |= {(1 << 18) + 11, (1 << 21) + 77, (1 << 22) + 3}
    ns |= {E.SPLIT_COPY_MIN_N + d for d in (-1, 0, 1)}
    ns |= {n for n, _ in MANY_PREFIX}
    return sorted(n for n in ns if 1 <= n <= 1 << 26)


SIZES = sweep_sizes()


def test_constants(consts):
    """Every hand-copied or header-parsed Python constant is the code's."""
    k = consts
    assert (E.SORT_THREADS, E.SORT_PER_THREAD, E.SORT_B) == (k["kSortThreads"], k["kSortPerThread"], k["kSortB"])
    assert k["kSortB"] == k["kSortThreads"] * k["kSortPerThread"]
    assert (E.SPLIT_COPY_MIN_N, E.SPLIT_COPY3_MIN_N) == (k["kSplitCopyMinN"], k["kSplitCopy3MinN"])
    assert (U.SMALL_WIN, U.SMALL_FUSED_N, U.SMALL_QUADS) == (k["kSmallWin"], k["kSmallFusedN"], k["kSmallQuads"])
    assert (U.SMALL_SLICES, U.SMALL_LANES_T) == (k["kSmallSlices"], k["kSmallLanesT"])
    assert (U.MANY_QUADS, U.MANY_QUAD_BUDGET) == (k["kManyQuads"], k["kManyQuadBudget"])
    assert U.many_budget() == (k["kManyTabBudget"], k["kManyTabCap"])
    assert X.engine_constants() == {"kAccLaneBudget": k["kAccLaneBudget"], "kAccSumLanes": k["kAccSumLanes"]}
    assert M.K_TJOBS == k["kTJobs"]
    assert (k["kMinC"], k["kMaxC"], k["kAutoMaxC"], k["kL1"]) == (4, 20, 16, 4)   # make_plan's literals below
    assert k["kScanChunk"] == k["kScanThreads"] * k["kScanPerThread"] and k["kMaxParts"] == 3


def _plan_fields(p):
    W = p["W"]
    return dict(c=p["c"], W=W, widths=[p["base"] + (1 if w < p["extra"] else 0) for w in range(W)], K=p["K"],
                L1=p["L1"], log2L1=p["log2L1"], NB=p["NB"], M1=p["M1"], NB2=p["NB2"], chunk=p["chunk"],
                nthreads=p["nthreads"], cmax=p["cmax"])


def test_make_plan(exe, consts):
    cs = [0] + list(range(consts["kMinC"], consts["kMaxC"] + 1))
    cases = [(n, c) for n in SIZES for c in cs]
    got = N.ask(exe, ("msm %d %d 0" % nc for nc in cases))
    for (n, c), g in zip(cases, got):
        assert _plan_fields(g) == M.make_plan(n, c), (n, c)
    # windows outside [kMinC, kMaxC] are clamped alike
    for c in (1, 3, 21, 40):
        assert _plan_fields(N.ask1(exe, "msm 1000 %d 0" % c)) == M.make_plan(1000, c)
    # a forced chunk: the model takes it as given, the product as a lower bound
    for n in (1 << 10, (1 << 18) + 11):
        for ch in (64, 256, 4096):
            if ch >= M.make_plan(n)["chunk"]:
                assert _plan_fields(N.ask1(exe, "msm %d 0 %d" % (n, ch))) == M.make_plan(n, 0, ch)


def test_part_starts(exe):
    for n, a, b, c, d in zip(SIZES, N.ask(exe, ("parts %d 1 1 -1" % n for n in SIZES)),
                             N.ask(exe, ("parts %d 1 0 -1" % n for n in SIZES)),
                             N.ask(exe, ("parts %d 0 1 -1" % n for n in SIZES)),
                             N.ask(exe, ("parts %d 1 1 0" % n for n in SIZES))):
        assert a["pstart"] == E.part_starts(n, True) and a["nch"] == len(a["pstart"]) - 1, n
        for one in (b, c, d):   # device scalars, no table, the split switched off: one part
            assert one["pstart"] == E.part_starts(n, False) == [0, n], n


def test_sort_blocks(exe, consts):
    """sort_ppt / sort_block on every digit row the drivers sort: the raw
    pipeline's (n points) and a table's (padded rows; the split copy's parts),
    at the automatic and every forced window."""
    kB = consts["kSortB"]
    cs = [0] + list(range(consts["kMinC"], consts["kMaxC"] + 1))

    def check(g, n, table, split):
        ps = E.part_starts(n, split)
        assert g["nch"] == len(ps) - 1
        for ch, (c0, c1) in enumerate(zip(ps[:-1], ps[1:])):
            p = "p%d_" % ch
            stride = n if not table else max(kB, E._rnd(n)) if len(ps) == 2 else max(kB, E._rnd(c1 - c0))   # boundaries()
            assert (g[p + "c0"], g[p + "nc"], g[p + "stride"]) == (c0, c1 - c0, stride), (n, ch)
            assert g[p + "gm_ppt"] == E.sort_ppt(stride), (n, ch)
            assert g[p + "g_ppt"] * consts["kSortThreads"] == E.sort_block(stride), (n, ch)
            assert g[p + "gm_hsub"] * g[p + "g_ppt"] == g[p + "gm_ppt"]

    raw = [(n, c) for n in SIZES for c in cs]
    for (n, c), g in zip(raw, N.ask(exe, ("sort %d %d 0 0 1 0 -1 0 0" % nc for nc in raw))):
        check(g, n, False, False)
    tab = [(n, c, split) for n in SIZES for c in cs[1:] for split in (0, 1)]
    for (n, c, split), g in zip(tab, N.ask(exe, ("sort %d %d 0 1 1 %d -1 0 0" % t for t in tab))):
        check(g, n, True, bool(split))


def test_small_geom(exe):
    ns = [n for n in SIZES if n <= 1 << 20] + [16, 17, 33, 300, 2047, 2048, 4097]
    for n, g in zip(ns, N.ask(exe, ("small %d" % n for n in ns))):
        assert (g["path"], g["kq"], g["ns"]) == U.small_geom(n), n


def test_many_geometry(exe):
    for c in range(1, 21):
        g = N.ask1(exe, "manyc %d" % c)
        assert (g["W"], g["bytes_per_base"]) == (U.many_windows(c), U.many_bytes_per_base(c)), c
    ns = sorted(set(SIZES) | {n + d for n, _ in MANY_PREFIX for d in (-1, 0, 1)} |
                {4096, 4097, 7084, 7085, 12192, 12193, 20164, 20165, 131072, 131073})
    for n, g in zip(ns, N.ask(exe, ("many %d" % n for n in ns))):
        c = U.many_pick_c(n)
        assert (g["c"], g["W"], g["bytes_per_base"]) == (c, U.many_windows(c), U.many_bytes_per_base(c)), n
    # many_kq of a call's MSM lengths: the product sees their total entries
    calls = [([n], c) for n in SIZES if n <= 1 << 22 for c in range(4, 9)]
    calls += [(list(U.many_batch(nb, c, big)[0]), c) for nb, c in MANY_PREFIX for big in (False, True)]
    got = N.ask(exe, ("manykq %d" % (sum(ns_) * U.many_windows(c)) for ns_, c in calls))
    for (ns_, c), g in zip(calls, got):
        assert g["kq"] == U.many_kq(ns_, c), (sum(ns_), c)


@functools.lru_cache(maxsize=None)
def _shape_terms():
    """{(T, Tp, npair)} and the term plans of the shapes in shape_util (curve 0;
    the counts do not depend on the curve)."""
    C = P.CURVES[0]
    out = {}
    for name in sorted(S.ALL):
        sh = S.shape(0, name)
        out[name] = (sh, X.term_plan(C, sh, list(range(1, 8))))
    return out


def test_acc_path(exe, monkeypatch):
    triples = sorted({(pl.T, pl.Tp, pl.npair) for _, pl in _shape_terms().values()} | {(30, 21, 16)})
    k = X.engine_constants()
    monkeypatch.setattr(X, "engine_constants", lambda: k)   # acc_path parses the header on every call
    X_acc_path = X.acc_path
    modes = [(-1, -1)] + [(s, -1) for s in range(6)] + [(-1, 1), (-1, 2), (0, 1), (0, 2)]
    for T, Tp, npair in triples:
        qs = [(B, split, tpl) for B in range(1, 4097) for split, tpl in modes]
        got = N.ask(exe, ("acc %d %d %d %d %d %d -1" % (B, T, Tp, npair, split, tpl) for B, split, tpl in qs))
        for (B, split, tpl), g in zip(qs, got):
            want = X_acc_path(B, T, Tp, npair, split=split, tpl=tpl)
            have = dict(lgS=g["lgS"], quad_terms=bool(g["quad_terms"]), tpl=g["tpl"], pstep=g["pstep"], lgL=g["lgL"])
            assert have == want, (T, Tp, npair, B, split, tpl)
            assert g["lgT"] == (4 if want["quad_terms"] else want["lgS"])


def test_term_plans(exe):
    """acc_terms on the rotation sets of every shape in shape_util: slots in
    first-use order, the h_i, w, zw and e terms, and the two-term lanes' pairs
    are term_plan's."""
    kind = {"proof": 0, "fixed": 1, "sigma": 2}
    names, queries = [], []
    for name, (sh, pl) in _shape_terms().items():
        po = sh.point_offsets()
        sets = X._queries(sh)
        words = [sh.num_fixed_columns, len(sh.perm_columns), sh.quotient_degree, po["h"][0], po["W"][0], len(sets)]
        for _, qs in sets:
            words.append(len(qs))
            for ref, _, _ in qs:
                words += [3, 0, 0] if ref == "H" else [kind[ref[0]], ref[1], 0]
        names.append(name)
        queries.append("terms " + " ".join(str(w) for w in words))
    nf = lambda sh: sh.num_fixed_columns
    for name, g in zip(names, N.ask(exe, queries)):
        sh, pl = _shape_terms()[name]

        def src(t):
            k_, i = t["src"]
            if k_ == "proof":
                return i
            return (1 << 28) | {"fixed": i, "sigma": nf(sh) + i, "g1": nf(sh) + len(sh.perm_columns)}[k_]

        assert (g["T"], g["Tp"], g["nslots"], g["npair"]) == (pl.T, pl.Tp, pl.nslots, pl.npair), name
        assert g["h_slot0"] == pl.nslots - sh.quotient_degree
        assert g["termsrc"] == [src(t) for t in pl.terms], name
        pairs = g["pairs"]
        assert [(a, None if b == 0xFFFFFFFF else b) for a, b in zip(pairs[0::2], pairs[1::2])] == pl.pairs, name
        # the slot of every query, in set order (H: kSlotH)
        slot = {}
        for t, term in enumerate(pl.terms):
            for j, i, _ in term["queries"]:
                slot[(j, i)] = t
        want = [slot.get((j, i), 0xFFFF) for j, (_, qs) in enumerate(X._queries(sh)) for i in range(len(qs))]
        assert g["qprog"][0::2] == want, name


def test_reduce_plan(exe, consts):
    """The reduction's grids from make_plan's fields: Wr = W / rows bucket sets,
    NB2 + kTJobs bit-sum jobs and one more host term per set, a quad per
    4-bucket segment in blocks of 256 threads, kBitsSplitK / Wr blocks per job."""
    cases = []
    for n in SIZES[::3] + [(1 << 18) + 11, (1 << 22) + 3]:
        for c in [0] + list(range(consts["kMinC"], consts["kMaxC"] + 1)):
            cases.append((n, c, 0, 1, M.make_plan(n, c)))
            if c:
                pl = M.make_plan(max(consts["kSortB"], E._rnd(n)), c)
                cases += [(n, c, 1, rows, pl) for rows in (1, pl["W"])]
    got = N.ask(exe, ("reduce %d %d 0 %d %d" % t[:4] for t in cases))
    for (n, c, fixed, rows, pl), g in zip(cases, got):
        Wr = pl["W"] // rows
        want = dict(Wr=Wr, TOT=Wr * pl["NB"] + 1, NJ=pl["NB2"] + M.K_TJOBS, NQ=pl["NB2"] + M.K_TJOBS + 1,
                    seg_blocks=(4 * Wr * pl["M1"] + 255) // 256,
                    nsplit=max(1, min(consts["kMaxSplit"], consts["kBitsSplitK"] // Wr)))
        assert g == want, (n, c, fixed, rows)


def test_acc_ladder_and_scalar_block(exe, consts):
    """acc_path's ladder form (row-sliced waves up to kAccSlicedChains chains,
    the VK chains this call builds included) and k_acc_scalars' block: np as
    shape_util.facts restates it, the whole LDS cap as the request beside a
    split ladder."""
    cap = S.constants()["kAccScalarsLds"]
    T, Tp, npair = 30, 21, 16
    lim = consts["kAccSlicedChains"]
    qs = [(B, lad, nvk, row, tail) for B in (1, 16, 37, 38, 39, 256, 1024, 3000) for lad in (-1, 0, 1)
          for nvk in (0, 9) for row, tail in ((32 * 90, 2000), (32 * 300, 9000), (32 * 2000, 20000), (32 * 61, 500))]
    got = N.ask(exe, ("acc %d %d %d %d -1 -1 %d %d %d %d %d" % (B, T, Tp, npair, lad, nvk, row, tail, cap)
                      for B, lad, nvk, row, tail in qs))
    seen = set()
    for (B, lad, nvk, row, tail), g in zip(qs, got):
        split = X.acc_path(B, T, Tp, npair)["lgS"] > 0
        assert g["sliced"] == (0 if not split else lad if lad >= 0 else int(B * Tp + nvk <= lim)), (B, lad, nvk)
        np_ = min(16, (cap - tail) // row - 1)
        assert g["np"] == np_ and g["lds"] == max(row * (np_ + 1) + tail, cap if split else 0), (B, row, tail)
        seen.add((split, g["sliced"], np_ == 16))
    assert len(seen) == 6   # one-lane form; split with both ladders; full and short blocks
    assert (38 * Tp <= lim < 38 * Tp + 9) and 39 * Tp > lim   # B = 38: the VK chains tip it, 39: the proofs' alone

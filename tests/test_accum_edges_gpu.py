"""Adversarial proofs on the device paths of the batched multiopen
accumulator (pm_accum_batch*): the planted cases of tests/accum_edge_util.py
(what each reaches is shown on the model in test_accum_edges_oracle.py) run
through k_acc_termmul<1> / <2>, k_acc_termadd in its lane and quad forms under
both ladder modes, and k_acc_sum at every lane count and row step.

Every result is compared bit for bit with the C port (oracle/accum_ref.c) and
with [dlog]G for every proof, with accumulate_msm for a sample; statuses must
be 0.  Each test asserts on acc_path (the engine's thresholds, parsed from the
header) that the batch takes the path it means to hit.  Large batches are the
distinct proofs tiled with numpy, and a tiled batch must give identical rows
in every tile.

k_acc_termadd: no collision between partial sums is planted or claimed for
points of prime order (operands that meet hold digits at disjoint table
positions, so a collision needs the NAFs of the halves to contain those of a
lattice vector; the argument is in accum_edge_util's docstring and the model
shows none for these scalars), so that path is covered by
scalars (0, +-1, 2^i, lambda 2^i: inf + inf and inf + Q in the butterfly and a
sum of one table point; the NAF patterns and the lattice-cell corners: table
position 127) and by a VK term and a proof term holding the same point, not
by claimed doublings.

pm_accum_batch_proofs from bytes is out of scope: its challenges are hashed
from the points, so no coefficient can be planted."""
import functools

import numpy as np
import pytest

import accum as A
import accum_edge_util as X
import accum_ref as R
import accum_util as U
import halo2_amd as H
import pasta as P
import test_accum_edges_oracle as O

pytestmark = pytest.mark.gpu
CURVES = (0, 1, 2)
LOG_N = {0: 10, 1: 11, 2: 12}


@functools.lru_cache(maxsize=None)
def _case(kind, cid, shape):
    """The planted batch and its references, computed once: (case, product
    shape, packed inputs, C port quads / h_eval, [dlog]G quads)."""
    seed = 0x6E0 + 16 * cid
    if kind == "family":
        case = X.family_case(cid, shape, LOG_N[cid], seed)
    elif kind == "termadd":
        case = X.family_case(cid, shape, LOG_N[cid], seed + 1, names=X.TERMADD_NAMES)
    elif kind == "pairs":
        case = X.pattern_pairs_case(cid, shape, LOG_N[cid], seed + 2)
    elif kind == "two":
        case = X.two_term_case(cid, shape, LOG_N[cid], seed + 3)
    else:
        case = X.sum_case(cid, shape, LOG_N[cid], seed + 4)
    assert len(case.proofs) == case.enumerated
    ps = U.to_product_shape(cid, case.shape())
    arrs = case.pack()
    _, qc, hc, stc = R.accum_batch(cid, ps.c, *arrs, threads=8)
    assert not stc.any() and all(case.status(b) == 0 for b in range(len(case.proofs)))
    want = np.stack([case.expected_quad(b) for b in range(len(case.proofs))])
    assert np.array_equal(qc, want)
    return case, ps, arrs, qc, hc, want


def _geom(case):
    pl = case.plan(0)
    return pl.T, pl.Tp, pl.npair


def _run(ctx, kind, cid, shape, B=None, lo=0, hi=None, sample=(0,)):
    """One device call on proofs [lo, hi) of the case (tiled to B rows),
    checked against every reference -> the number of distinct proofs checked."""
    case, ps, arrs, qc, hc, want = _case(kind, cid, shape)
    hi = len(case.proofs) if hi is None else hi
    sub = [a[lo:hi] for a in arrs]
    n = hi - lo
    B = B or n
    quads, h, st = ctx.accum_batch_status(ps, *X.tile(sub, B))
    assert quads.shape == (B, 4, 8) and not st.any()
    ran = 0
    for i in range(n):
        nm = case.proofs[lo + i]["name"]
        assert np.array_equal(quads[i], qc[lo + i]), (kind, cid, nm)
        assert np.array_equal(quads[i], want[lo + i]), (kind, cid, nm)
        assert np.array_equal(h[i], hc[lo + i]), (kind, cid, nm)
        ran += 1
    for t0 in range(n, B, n):     # a tiled batch: every tile equals the first
        m = min(n, B - t0)
        assert np.array_equal(quads[t0:t0 + m], quads[:m]) and np.array_equal(h[t0:t0 + m], h[:m]), (kind, cid, t0)
    for i in sample:
        b = lo + (i % n)
        q, hh = A.pack_result(case.C, A.accumulate_msm(case.C, case.sh, case.oracle_proof(b)))
        assert np.array_equal(quads[b - lo], q) and np.array_equal(h[b - lo], hh), (kind, cid, b)
    assert ran == n
    return n


def _identity_rows_are_zero(kind, cid, shape, ctx):
    """Outputs that are the identity are stored as all zero words."""
    case, ps, arrs, qc, _, want = _case(kind, cid, shape)
    zero = [(b, o) for b in range(len(case.proofs)) for o in range(4) if not want[b, o].any()]
    assert len(zero) >= 2          # w of the adjacent pattern, e with ev = 0
    quads, _, _ = ctx.accum_batch_status(ps, *arrs)
    for b, o in zero:
        assert not quads[b, o].any(), (case.proofs[b]["name"], o)


@pytest.mark.parametrize("tpl", [1, 2])
@pytest.mark.parametrize("cid", CURVES)
def test_one_lane_windows(gpu_ctx, cid, tpl):
    """k_acc_termmul<Cv, 1> and <Cv, 2> (one-lane form forced, terms per lane
    forced): the scalar families on W_{S-2} (scalar_on_W: 0, +-1, the GLV
    specials, the base-8 patterns with the u = 8 arm, the NAF patterns, the
    lattice-cell corners), two base-8 patterns on the last zw pair, and the
    two-term collisions (madd's doubling and cancellation, cancellation in
    mid-chain with a restart, [m]P0 and +-phi(P0), an identity P0 or P1, a
    zero coefficient on a live point, the odd range's unpaired last term)."""
    shape = O.SHAPE_OF[cid]
    gpu_ctx.set_accum_split(0)
    gpu_ctx.set_accum_option(H.ACC_OPT_TERMS_PER_LANE, tpl)
    try:
        ran = want_n = 0
        for kind, shp in (("family", "simple"), ("pairs", shape), ("two", shape)):
            case = _case(kind, cid, shp)[0]
            p = X.acc_path(len(case.proofs), *_geom(case), split=0, tpl=tpl)
            assert (p["lgS"], p["tpl"], p["pstep"]) == (0, tpl, tpl)
            ran += _run(gpu_ctx, kind, cid, shp, sample=(0, 1, 2))
            want_n += case.enumerated
        assert ran == want_n
        two = _case("two", cid, shape)[0]
        assert any(t1 is None for _, t1 in two.plan(0).pairs)
    finally:
        gpu_ctx.set_accum_option(H.ACC_OPT_TERMS_PER_LANE, -1)
        gpu_ctx.set_accum_split(-1)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("cid", CURVES)
def test_term_additions(cid, mode):
    """k_acc_termadd in the lane form (2 .. 32 lanes per term, forced) and the
    quad form (automatic, B T <= 1024), tables built by both ladder forms (a
    fresh context per mode): the term-addition scalar family and the VK twin."""
    ctx = H.Context(0)
    try:
        ctx.set_accum_ladder(mode)
        case = _case("termadd", cid, "simple")[0]
        n, geom = len(case.proofs), _geom(case)
        assert any(pf["name"] == "vk twin" for pf in case.proofs)
        try:
            for lg in (1, 2, 3, 4, 5):
                p = X.acc_path(n, *geom, split=lg)
                assert p["lgS"] == lg and not p["quad_terms"]
                ctx.set_accum_split(lg)
                assert _run(ctx, "termadd", cid, "simple", sample=(lg,)) == n == case.enumerated
        finally:
            ctx.set_accum_split(-1)
        step = 1024 // geom[0]
        assert X.acc_path(step, *geom)["quad_terms"] and not X.acc_path(step + 1, *geom)["quad_terms"]
        ran = 0
        for lo in range(0, n, step):
            ran += _run(ctx, "termadd", cid, "simple", lo=lo, hi=min(n, lo + step), sample=())
        assert ran == n
    finally:
        ctx.close()


@pytest.mark.parametrize("lgL", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("cid", CURVES)
def test_sum_lanes(gpu_ctx, cid, lgL):
    """k_acc_sum with 2^lgL lanes per output (the batch size the model gives
    for it) after one-term lanes (row step 1) and two-term lanes (row step 2):
    equal products on w, zw and f (VK terms included) double in the loop and
    the butterfly, a ladder output meets an affine start (W_last = [2^i]
    W_prev at u = 2^i), +- patterns cancel, w = identity and e with ev = 0 are
    stored as zero words.  lgL <= 1 runs xyzz29_add, above it xyzz29_add_q."""
    shape = O.SHAPE_OF[(cid + 1) % 3]
    case = _case("sum", cid, shape)[0]
    geom = _geom(case)
    B = max(X.batch_for_lgL(lgL, *geom), len(case.proofs))
    gpu_ctx.set_accum_split(0)
    try:
        for tpl in (1, 2):
            p = X.acc_path(B, *geom, split=0, tpl=tpl)
            assert (p["lgL"], p["pstep"], p["lgS"]) == (lgL, tpl, 0), (B, p)
            gpu_ctx.set_accum_option(H.ACC_OPT_TERMS_PER_LANE, tpl)
            assert _run(gpu_ctx, "sum", cid, shape, B=B, sample=(lgL,)) == case.enumerated
        if lgL == 5:
            _identity_rows_are_zero("sum", cid, shape, gpu_ctx)
    finally:
        gpu_ctx.set_accum_option(H.ACC_OPT_TERMS_PER_LANE, -1)
        gpu_ctx.set_accum_split(-1)


@pytest.mark.parametrize("cid", CURVES)
def test_automatic_paths(gpu_ctx, cid):
    """The same planted batches under the automatic schedule (split form with
    the powers tables at these sizes): k_acc_termadd and k_acc_sum meet the
    identity points, zero coefficients and equal / opposite products."""
    for kind, shape in (("sum", O.SHAPE_OF[(cid + 1) % 3]), ("two", O.SHAPE_OF[cid])):
        case = _case(kind, cid, shape)[0]
        assert X.acc_path(len(case.proofs), *_geom(case))["lgS"] > 0
        assert _run(gpu_ctx, kind, cid, shape) == case.enumerated


def test_device_pointer_and_multi_entries(gpu_ctx):
    """The planted k_acc_sum batch (equal and cancelling products) through
    pm_accum_batch_device and pm_accum_batch_multi."""
    import torch

    cid, shape = 2, O.SHAPE_OF[0]
    case, ps, arrs, qc, hc, want = _case("sum", cid, shape)
    B = len(case.proofs)
    dev = torch.device("cuda", gpu_ctx.device)
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev) for a in arrs]
    dq = torch.zeros((B, 4, 8), dtype=torch.int64, device=dev)
    dh = torch.zeros((B, 4), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.accum_batch_device(ps, B, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), dq.data_ptr(), dh.data_ptr())
    assert np.array_equal(dq.cpu().numpy().view(np.uint64), qc) and np.array_equal(dq.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(dh.cpu().numpy().view(np.uint64), hc)
    extra = H.Context(0)
    try:
        ch, q, h, st = H.accum_batch_multi([gpu_ctx, extra], ps, arrs[0], arrs[1], challenges=arrs[2])
        assert np.array_equal(q, qc) and np.array_equal(q, want) and np.array_equal(h, hc) and not st.any()
    finally:
        extra.close()


# --------------------------------------------------------------- shape limits
def _accepted(ctx, cid, sh, B=2, seed=0x51):
    """B random proofs of the shape on the device == accumulate_msm."""
    C = P.CURVES[cid]
    proofs = [A.synth_proof(C, sh, seed, b) for b in range(B)]
    ps = U.to_product_shape(cid, sh)
    quads, h, st = ctx.accum_batch_status(ps, *A.pack_proofs(C, sh, proofs))
    assert not st.any()
    for b, pf in enumerate(proofs):
        q, hh = A.pack_result(C, A.accumulate_msm(C, sh, pf))
        assert np.array_equal(h[b], hh) and np.array_equal(quads[b], q), b
    return ps, proofs


def test_limit_expression_stack_16(gpu_ctx):
    """A right-nested Sum of 16 leaves (stack depth 16, the bound) is
    accepted: h_eval and the quad equal the oracle's."""
    _accepted(gpu_ctx, 2, O._limit_shape(2, gates=[O.nested_sum(16)]))


def test_limit_64_rotation_sets(gpu_ctx):
    _accepted(gpu_ctx, 2, O.many_rotations_shape(2, 64))


def test_limit_61_blinding_factors(gpu_ctx):
    _accepted(gpu_ctx, 2, O._limit_shape(2, blinding_factors=61))


def test_scalar_block_with_fewer_than_16_proofs_per_block(gpu_ctx):
    """A shape whose evaluation rows are large enough that k_acc_scalars takes
    fewer than 15 proofs per block (256 queries in one set: about 370 rows of
    32 B per proof in 152 KiB), in a batch of several blocks with a ragged
    last one: h_eval and every quad equal the C port for every proof, the
    Python oracle for three.  (The Lagrange quads beyond the block's proofs
    used to write into the rows of proofs 0, 1, ...: wrong h_eval and e.)"""
    C, sh, B = P.CURVES[0], O.big_set_shape(0, 256), 37
    proofs = [A.synth_proof(C, sh, 0x53, b) for b in range(B)]
    ps = U.to_product_shape(0, sh)
    arrs = A.pack_proofs(C, sh, proofs)
    # accum_device_impl's rows per proof (kAccXVals = 10, kAccStack = 16) and
    # its np <= kAccScalarsLds / row bytes - 1 (the constants' tail only lowers it)
    pl = X.term_plan(C, sh, proofs[0].challenges)
    nvals = 2 * sh.n_perm_sets + 1 + 5 * sh.num_lookups
    rows = sh.scalars_per_proof() + pl.T + 10 + nvals + 2 * (sh.blinding_factors + 3) + 16 + pl.nslots + \
        sh.quotient_degree
    assert 152 * 1024 // (32 * rows) - 1 <= 13
    _, qc, hc, stc = R.accum_batch(0, ps.c, *arrs, threads=8)
    quads, h, st = gpu_ctx.accum_batch_status(ps, *arrs)
    assert not st.any() and not stc.any()
    for b in range(B):
        assert np.array_equal(h[b], hc[b]) and np.array_equal(quads[b], qc[b]), b
    for b in (0, 1, B - 1):
        q, hh = A.pack_result(C, A.accumulate_msm(C, sh, proofs[b]))
        assert np.array_equal(h[b], hh) and np.array_equal(quads[b], q), b


def test_limit_256_queries_in_one_set(gpu_ctx):
    """256 queries in one rotation set are accepted and equal the oracle; 257
    are refused by pm_accum_batch (the layout call does not check it)."""
    _accepted(gpu_ctx, 2, O.big_set_shape(2, 256))
    sh = O.big_set_shape(2, 257)
    C = P.CURVES[2]
    proofs = [A.synth_proof(C, sh, 0x52, 0)]
    with pytest.raises(H.PmError, match="rotation set too large"):
        gpu_ctx.accum_batch(U.to_product_shape(2, sh), *A.pack_proofs(C, sh, proofs))

"""The accumulator path on the device across proof shapes: pm_accum_batch,
pm_transcript_batch, pm_accum_batch_transcript, pm_decode_proofs and
pm_accum_batch_proofs on the shape family of tests/shape_util.py.

The device code of this path is a program compiled from the caller's
pm_proof_shape, so each shape runs other code: another split of the Lagrange
denominators over the quad (acc_lagrange_q), another LDS layout and proofs per
block of k_acc_scalars, other rotation sets and term slots, another byte
stream with other squeeze offsets in k_transcript_s, other item offsets in
k_proof_decode.  What each shape reaches is asserted from facts() in
test_shapes_oracle.py.

Every expected value is an oracle's and none the library's: the C port
(oracle/accum_ref.c) for every proof, which test_shapes_oracle.py shows equal
to both Python restatements on these same batches (the references are built
once in shape_util and shared), [sum c_t a_t]G by the term plan for the first
and the last proof of a batch, and the Python transcript for every replay.
All comparisons are bit for bit."""
import numpy as np
import pytest

import accum as A
import accum_edge_util as X
import accum_util as U
import halo2_amd as H
import shape_util as S

pytestmark = pytest.mark.gpu
ALL_CURVES = ("bf0", "bf1", "bf2", "bf4", "bf6", "bf7", "bf61", "logn_max", "mixed", "consts")   # field-dependent chains


def _curves(name):
    return (0, 1, 2) if name in ALL_CURVES else (2,)


ACC_CASES = [(c, nm) for nm in list(S.DIRECTED) + list(S.WIDE) + sorted(S.EDGES) for c in _curves(nm)]


@pytest.fixture(scope="module")
def record_ctx():
    """A context whose transcript replay is the per-record kernel (k_transcript)."""
    ctx = H.Context(0)
    ctx.set_accum_option(H.ACC_OPT_TRANSCRIPT, 0)
    yield ctx
    ctx.close()


def _run_accum(ctx, cid, name, B):
    bt, ps, arrs, qc, hc, stc = S.reference(cid, name, B)
    assert not stc.any()
    quads, h, st = ctx.accum_batch_status(ps, *arrs)
    assert quads.shape == (B, 4, 8) and not st.any(), (name, B, st)
    for b in range(B):
        assert np.array_equal(h[b], hc[b]) and np.array_equal(quads[b], qc[b]), (name, B, b)
    for b in {0, B - 1}:
        assert np.array_equal(quads[b], bt.dlog_quad(b)), (name, B, b)


@pytest.mark.parametrize("cid,name", ACC_CASES)
def test_accumulator_with_caller_challenges(gpu_ctx, cid, name):
    """pm_accum_batch with distinct proofs at B = 1, B = np + 1 (a ragged
    second block of k_acc_scalars with one proof) and, for the wide shapes,
    B = 2 np (two full blocks), under the automatic schedule (the powers
    tables: 16 quads per term while B T <= 1024, which is every shape at B =
    1, else lanes); B = np + 1 again with the term kernels forced to the
    one-lane form (k_acc_termmul) and to 8 lanes per term (k_acc_termadd),
    which read the shape's term sources, ranks and pairs."""
    f = S.facts(S.shape(cid, name))
    n = f["np"]
    assert 1 <= n <= 16
    sizes = [1, n + 1] + ([2 * n] if name in S.WIDE else [])
    assert max(sizes) <= 33
    for B in sizes:
        p = f["path"](B)
        assert p["lgS"] >= 1 and p["quad_terms"] == (B * f["T"] <= 1024), (name, B, p)
        assert B > 1 or p["quad_terms"]
        _run_accum(gpu_ctx, cid, name, B)
    try:
        for lg in (0, 3):
            p = X.acc_path(n + 1, f["T"], f["Tp"], f["npair"], split=lg)
            assert p["lgS"] == lg and not p["quad_terms"] and (lg > 0 or p["tpl"] == 1)
            gpu_ctx.set_accum_split(lg)
            _run_accum(gpu_ctx, cid, name, n + 1)
    finally:
        gpu_ctx.set_accum_split(-1)


@pytest.mark.parametrize("cid,name", [(0, "gates_only"), (0, "bf1"), (1, "bf1"), (2, "bf1"), (2, "wide_np8_14")])
def test_scalar_block_values(gpu_ctx, cid, name):
    """theta, beta, gamma, y, v, u in {0, 1, r - 1}, x = 0, x^n = -1,
    evaluations all 0 / all r - 1: status 0 and the oracle's values.  x =
    omega^-i for every i <= bf + 1 (a denominator of every lane of the quad):
    PM_ACCUM_DENOM_ZERO for that proof alone, its neighbours bit-exact."""
    bt, names, ps, arrs, qc, hc, stc = S.scalar_block_reference(cid, name)
    quads, h, st = gpu_ctx.accum_batch_status(ps, *arrs)
    want = [bt.status(b) for b in range(bt.B)]
    assert st.tolist() == want == stc.tolist()
    assert want.count(A.STATUS_DENOM_ZERO) == bt.sh.blinding_factors + 2
    for b, nm in enumerate(names):
        if want[b]:
            continue                      # outputs unspecified
        assert np.array_equal(h[b], hc[b]) and np.array_equal(quads[b], qc[b]), nm
    assert not quads[names.index("x=0")][1].any()


def _tr_cases():
    out = []
    for nm in sorted(S.EDGES):
        out += [(c, nm) for c in (0, 1, 2)]
    for i, nm in enumerate(S.DIRECTED):
        out.append((i % 3, nm))
    return out


def _tr_id(case):
    cid, nm = case
    fits = S.facts(S.shape(cid, nm))["stream_fits"]
    return f"{cid}-{nm}-{'streamed' if fits else 'record_fallback_by_size'}"


TR_CASES = _tr_cases()


@pytest.mark.parametrize("case", TR_CASES, ids=[_tr_id(c) for c in TR_CASES])
def test_transcript(gpu_ctx, record_ctx, case):
    """pm_transcript_batch with B = 17 (two blocks, the second with one proof),
    proof 5 with an identity commitment (its streamed block falls back to the
    per-record replay): the streamed kernel where its plan fits LDS (the id
    says where it does not: the fallback by size) and the per-record kernel
    (PM_ACC_OPT_TRANSCRIPT = 0) both equal the Python transcript.  The edge
    shapes put each squeeze at a stream offset = 0, 1, 127 (mod 128)."""
    cid, name = case
    bt, ps, pts, scs, vk, ch, st = S.transcript_reference(cid, name, 17, 5)
    assert st[5] == 1 and st.sum() == 1
    for ctx in (gpu_ctx, record_ctx):
        got, gst = ctx.transcript_batch(ps, pts, scs, vk)
        assert np.array_equal(gst, st), name
        for b in range(17):
            assert np.array_equal(got[b], ch[b]), (name, b, ctx is record_ctx)


def test_transcript_cases_cover_both_plans():
    fits = {S.facts(S.shape(c, nm))["stream_fits"] for c, nm in TR_CASES}
    assert fits == {True, False}


BYTES_CASES = [(c, nm) for nm in list(S.DIRECTED) + list(S.WIDE) for c in ((0, 1, 2) if nm in ("bf0", "mixed") else (2,))]


@pytest.mark.parametrize("cid,name", BYTES_CASES)
def test_fused_and_from_bytes(gpu_ctx, cid, name):
    """B = 5 proofs, one with a point off the curve and one with a scalar = r:
    pm_decode_proofs equals the oracle's decode for all five; pm_accum_batch_proofs
    flags exactly those two and equals the oracle (challenges, quad, h_eval) on
    the other three; pm_accum_batch_transcript on the decoded inputs equals
    the oracle on the same three."""
    bt, ps, datas, inst, vk, out = S.bytes_reference(cid, name)
    bad = {S.BAD_POINT_AT: H.PROOF_BAD_POINT, S.BAD_SCALAR_AT: H.PROOF_BAD_SCALAR}
    good = [b for b in range(S.BYTES_B) if b not in bad]
    assert not out["status"][good].any()
    pts, scs, st = gpu_ctx.decode_proofs(ps, datas, inst)
    assert st.tolist() == [bad.get(b, 0) for b in range(S.BYTES_B)]
    assert np.array_equal(pts, out["points"]) and np.array_equal(scs, out["scalars"])
    quads, h, ch, st = gpu_ctx.accum_batch_proofs(ps, datas, inst, vk)
    assert np.array_equal(st, out["status"])
    for b, bit in bad.items():
        assert st[b] & (H.PROOF_BAD_POINT | H.PROOF_BAD_SCALAR) == bit
    for b in good:
        assert np.array_equal(ch[b], out["challenges"][b]) and np.array_equal(h[b], out["h_eval"][b]), (name, b)
        assert np.array_equal(quads[b], out["quads"][b]), (name, b)
    quads, h, ch, st = gpu_ctx.accum_batch_transcript(ps, out["points"], out["scalars"], vk)
    for b in good:
        assert st[b] == 0 and np.array_equal(ch[b], out["challenges"][b]), (name, b)
        assert np.array_equal(quads[b], out["quads"][b]) and np.array_equal(h[b], out["h_eval"][b]), (name, b)


@pytest.mark.parametrize("cid", [0, 1, 2])
def test_random_shapes(gpu_ctx, cid):
    """The generated shapes of test_shapes_oracle.test_random_shapes_agree (same
    seeds, where the C port is shown equal to the Python oracle on them): three
    proofs each, with caller challenges and from bytes."""
    import accum_ref as R
    import proof_bytes as PB

    shapes, _ = S.random_shapes(cid, 8, 0x5AFE + cid)
    for i, sh in enumerate(shapes):
        bt = S.Batch(cid, sh, 3, 0x4A + i)
        ps = U.to_product_shape(cid, sh)
        arrs = bt.pack()
        _, qc, hc, stc = R.accum_batch(cid, ps.c, *arrs, threads=4)
        quads, h, st = gpu_ctx.accum_batch_status(ps, *arrs)
        assert not st.any() and not stc.any()
        assert np.array_equal(quads, qc) and np.array_equal(h, hc), i
        assert np.array_equal(quads[0], bt.dlog_quad(0)), i
        _, vk = S.vk_repr(cid, f"random{i}")
        datas = [PB.serialize(bt.C, sh, bt.proof(b)) for b in range(3)]
        inst = np.ascontiguousarray(arrs[0][:, :sh.num_instance_columns])
        chc, qc, hc, stc = R.accum_batch(cid, ps.c, arrs[0], arrs[1], vk_repr=vk, threads=4)
        quads, h, ch, st = gpu_ctx.accum_batch_proofs(ps, datas, inst, vk)
        assert np.array_equal(st, stc) and not st.any(), i
        assert np.array_equal(ch, chc) and np.array_equal(quads, qc) and np.array_equal(h, hc), i


def test_zero_instance_columns_are_covered():
    ni = {S.shape(c, nm).num_instance_columns for c, nm in BYTES_CASES}
    assert 0 in ni and max(ni) > 0


def test_device_bounds(gpu_ctx):
    """A shape whose rows do not fit k_acc_scalars' LDS and a rotation set of
    257 queries are refused with PM_ERR_UNSUPPORTED before anything is
    launched; the same context then still computes a small case."""
    sh = S.shape(2, "past_lds")
    assert S.facts(sh)["np"] == 0 and S.legal(2, sh) == ""
    ps = U.to_product_shape(2, sh)
    with pytest.raises(H.PmError, match="pm error -4: .*too many evaluations / terms per proof"):
        gpu_ctx.accum_batch(ps, *S.Batch(2, sh, 1, 1).pack())
    _run_accum(gpu_ctx, 2, "mixed", 2)
    sh = S.set_size_shape(2, 257)
    assert S.legal(2, sh) == "set size"
    with pytest.raises(H.PmError, match="pm error -4: .*rotation set too large"):
        gpu_ctx.accum_batch(U.to_product_shape(2, sh), *S.Batch(2, sh, 1, 1).pack())
    _run_accum(gpu_ctx, 2, "mixed", 2)


def test_no_stale_state_between_shapes():
    """One context runs six shapes in turn, twice round, from proof bytes (the
    program, constants, VK words, the transcript's word table and the
    decoder's map are re-sent each time); every result equals the oracle's,
    and that of a fresh context."""
    names = [(2, "mixed"), (2, "gates_only"), (2, "sets64"), (0, "bf0"), (2, "lookups3"), (2, "perm_ragged")]
    good = [b for b in range(S.BYTES_B) if b not in (S.BAD_POINT_AT, S.BAD_SCALAR_AT)]
    fresh = []
    for cid, nm in names:
        _, ps, datas, inst, vk, _ = S.bytes_reference(cid, nm)
        ctx = H.Context(0)
        try:
            fresh.append(ctx.accum_batch_proofs(ps, datas, inst, vk))
        finally:
            ctx.close()
    one = H.Context(0)
    try:
        for rnd in range(2):
            for (cid, nm), want in zip(names, fresh):
                _, ps, datas, inst, vk, out = S.bytes_reference(cid, nm)
                quads, h, ch, st = one.accum_batch_proofs(ps, datas, inst, vk)
                assert np.array_equal(st, out["status"]) and np.array_equal(st, want[3]), (nm, rnd)
                for b in good:
                    assert np.array_equal(quads[b], out["quads"][b]) and np.array_equal(h[b], out["h_eval"][b]), (nm, rnd, b)
                    assert np.array_equal(ch[b], out["challenges"][b]), (nm, rnd, b)
                    assert np.array_equal(quads[b], want[0][b]) and np.array_equal(h[b], want[1][b]), (nm, rnd, b)
    finally:
        one.close()

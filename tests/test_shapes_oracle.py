"""CPU: the accumulator's references across proof shapes (tests/shape_util.py).

For every directed, wide and transcript-edge shape and for N_RANDOM random
shapes per curve, on all three curves: the literal and the MSM restatement of
the Python oracle agree, the C port (oracle/accum_ref.c: caller challenges,
replayed challenges, and from proof bytes) equals them bit for bit in
challenges, quads, h_eval and status, every quad is [sum c_t a_t]G by the
term plan, and the library's layout call equals the oracle's counts.  The
shapes with at most three proofs and with one proof per block of k_acc_scalars
(some 800 and 2000 evaluations) run on BN254 alone with one proof, against the
C port and [sum c_t a_t]G only: the two Python walks take seconds each there
and their field arithmetic is that of the other wide shape.

The coverage the family is for is asserted from facts(), not assumed; the
library's host validation is probed at every bound; the random generator must
keep at least half of its draws."""
import numpy as np
import pytest

import accum as A
import accum_ref as R
import accum_util as U
import halo2_amd as H
import pasta as P
import proof_bytes as PB
import shape_util as S
import transcript as T

CURVES = (0, 1, 2)
NAMES = list(S.DIRECTED) + list(S.WIDE) + list(S.EDGES)
N_RANDOM = 8


def _check_shape(cid, sh, name, bt, python=(0,)):
    """Every reference on the proofs of batch bt (Python on those in `python`)."""
    C = P.CURVES[cid]
    ps = U.to_product_shape(cid, sh)
    counts = (sh.points_per_proof(), sh.scalars_per_proof(), sh.num_sets())
    assert ps.layout() == counts and R.layout(ps.c) == counts
    assert H.proof_size(ps) == PB.proof_size(sh)
    arrs = bt.pack()
    _, q, h, st = R.accum_batch(cid, ps.c, *arrs, threads=4)
    for b in range(bt.B):
        assert st[b] == bt.status(b) == 0, (name, b)
        assert np.array_equal(q[b], bt.dlog_quad(b)), (name, b)
        if b in python:
            pf = bt.proof(b)
            r1, r2 = A.accumulate(C, sh, pf), A.accumulate_msm(C, sh, pf)
            assert r1 == r2, (name, b)
            qq, hh = A.pack_result(C, r2)
            assert np.array_equal(qq, q[b]) and np.array_equal(hh, h[b]), (name, b)
    # replayed challenges: the C port's own Blake2b against hashlib's
    vkr, vk = S.vk_repr(cid, name)
    ch, q2, h2, st2 = R.accum_batch(cid, ps.c, arrs[0], arrs[1], vk_repr=vk, threads=4)
    for b in range(bt.B):
        want, stw = T.replay_challenges(C, sh, bt.proof(b), vkr)
        assert stw == 0 and st2[b] == A.proof_status(C, sh, want), (name, b)
        assert np.array_equal(ch[b], S.limbs(C, want)), (name, b)
    # the same proofs from bytes: decode, replay, accumulate
    ni = sh.num_instance_columns
    buf = np.frombuffer(b"".join(PB.serialize(C, sh, bt.proof(b)) for b in range(bt.B)), dtype=np.uint8)
    out = R.batch_proofs(cid, ps.c, buf.reshape(bt.B, -1), np.ascontiguousarray(arrs[0][:, :ni]), vk_repr=vk, threads=4)
    assert np.array_equal(out["points"], arrs[0]) and np.array_equal(out["scalars"], arrs[1]) and not out["status"].any()
    assert np.array_equal(out["challenges"], ch) and np.array_equal(out["quads"], q2) and np.array_equal(out["h_eval"], h2)
    for b in python:
        pf = bt.proof(b)
        pf.challenges, _ = T.replay_challenges(C, sh, pf, vkr)
        qq, hh = A.pack_result(C, A.accumulate_msm(C, sh, pf))
        assert np.array_equal(qq, q2[b]) and np.array_equal(hh, h2[b]), (name, b)


@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("name", NAMES)
def test_references_agree(cid, name):
    sh = S.shape(cid, name)
    assert S.legal(cid, sh) == ""
    if name in S.HEAVY:
        # one curve, one proof, the C port and [sum c_t a_t]G (module docstring)
        if cid != 2:
            return
        bt, ps, arrs, q, h, st = S.reference(cid, name, 1)
        assert ps.layout() == (sh.points_per_proof(), sh.scalars_per_proof(), sh.num_sets())
        assert st[0] == bt.status(0) == 0 and np.array_equal(q[0], bt.dlog_quad(0))
        return
    bt = S.reference(cid, name, 2)[0]
    _check_shape(cid, sh, name, bt)


@pytest.mark.parametrize("cid", CURVES)
def test_random_shapes_agree(cid):
    """N_RANDOM generated shapes per curve through every reference; at most
    N_RANDOM redraws, so at least half of the generator's draws are kept."""
    shapes, redraws = S.random_shapes(cid, N_RANDOM, 0x5AFE + cid)
    assert len(shapes) == N_RANDOM and redraws <= N_RANDOM
    seen = set()
    for i, sh in enumerate(shapes):
        assert S.legal(cid, sh) == ""
        assert sh.points_per_proof() <= S.MAX_POINTS and sh.scalars_per_proof() <= S.MAX_EVALS
        _check_shape(cid, sh, f"random{i}", S.Batch(cid, sh, 2, 0x4A + i))
        f = S.facts(sh)
        seen.add((f["n_perm_sets"] > 0, f["num_lookups"] > 0, len(sh.gates) > 0))
    assert len(seen) >= 4       # the draws differ in structure, not only in size


def test_generator_counts_redraws():
    """A stream that must redraw says so: with the size bound at its minimum
    every larger draw is counted, none is dropped."""
    old = S.MAX_POINTS
    try:
        S.MAX_POINTS = 8
        shapes, redraws = S.random_shapes(2, 3, 7)
        assert len(shapes) == 3 and redraws > 0 and all(s.points_per_proof() <= 8 for s in shapes)
    finally:
        S.MAX_POINTS = old


def test_coverage():
    """Every fact the family is for, read off facts() of the named shapes."""
    F = {nm: S.facts(S.shape(2, nm)) for nm in NAMES}
    for nm, want in S.DIRECTED_FACTS.items():
        assert {k: F[nm][k] for k in want} == want, nm
    D = [F[nm] for nm in S.DIRECTED]
    assert {f["nd_mod3"] for f in D} == {0, 1, 2}
    assert {0, 1, 2, 4, 6, 7, 61} <= {f["bf"] for f in D}
    assert any(f["logn_short"] for f in D)
    assert {S.shape(2, nm).log_n for nm in S.DIRECTED} >= {2, 3}
    for cid in CURVES:
        sh = S.shape(cid, "logn_max")
        assert sh.log_n == S.TWO_ADICITY[cid] == A.two_adic(P.CURVES[cid].r)[2]
        assert pow(sh.omega, 1 << (sh.log_n - 1), P.CURVES[cid].r) == P.CURVES[cid].r - 1
    assert 8 <= F["wide_np8_14"]["np"] <= 14 and 1 <= F["wide_np3"]["np"] <= 3 and F["wide_np1"]["np"] == 1
    assert all(f["np"] == 16 for nm, f in F.items() if nm in S.DIRECTED and nm != "set256")
    assert S.facts(S.shape(2, "past_lds"))["np"] == 0
    assert {f["nsets"] for f in D} >= {1, 64}
    assert any(f["J"] == 0 for f in D) and any(f["J"] > 0 for f in D)
    assert {min(f["n_perm_sets"], 3) for f in D} == {0, 1, 2, 3}
    assert {min(f["num_lookups"], 3) for f in D} >= {0, 1, 3}
    assert max(f["stack"] for f in D) == 16 == S.constants()["kAccStack"]
    assert max(f["max_set"] for f in D) == 256 == S.constants()["kAccMaxPerSet"]
    sh = S.shape(2, "perm_chunk1")
    assert sh.perm_chunk_len == 1
    assert len(S.shape(2, "perm_ragged").perm_columns) % S.shape(2, "perm_ragged").perm_chunk_len == 1
    assert len(S.shape(2, "perm_exact").perm_columns) % S.shape(2, "perm_exact").perm_chunk_len == 0
    assert not S.shape(2, "no_gates").gates and not S.shape(2, "no_gates_lookup").gates
    assert {S.shape(2, nm).quotient_degree for nm in ("qd1", "qd24")} == {1, 24}
    sh = S.shape(2, "last_rot_queried")
    assert -(sh.blinding_factors + 1) in {rot for _, rot in sh.advice_queries} and sh.n_perm_sets > 1
    assert max(abs(rot) for _, rot in S.shape(2, "big_rotations").advice_queries) == (1 << 31) - 1
    assert len({rot for c, rot in S.shape(2, "one_col_many_rots").advice_queries if c == 0}) == 9
    sh = S.shape(2, "gates_only")                 # a VK column and a proof column in the one rotation set
    assert sh.fixed_queries and sh.advice_queries and F["gates_only"]["nsets"] == 1
    assert any(S.shape(2, nm).num_instance_columns == 0 for nm in S.DIRECTED)
    assert S.shape(2, "mixed").num_instance_columns and S.shape(2, "mixed").num_fixed_columns
    r = P.CURVES[2].r
    cs = []
    H.compile_expressions(S.shape(2, "consts").gates, cs)
    assert {c % r for c in cs} == {0, 1, r - 1}
    # the transcript: every squeeze at a full final block, one byte past it, one byte short
    got = set()
    for nm, pairs in S.EDGE_PAIRS.items():
        for k, res in pairs:
            assert F[nm]["L_mod"][k] == res, (nm, k)
            got.add((k, res))
    assert got == {(k, res) for k in range(7) for res in (0, 1, 127)}
    # both sides of the streamed plan's LDS bound
    assert {F[nm]["stream_fits"] for nm in S.EDGES} == {True, False}
    assert not F["sets64"]["stream_fits"] and F["mixed"]["stream_fits"]


def test_facts_restate_the_library():
    """facts()' counts against the library's layout call and the term plan."""
    import accum_edge_util as X

    for nm in ("mixed", "sets64", "lookups3", "wide_np8_14"):
        sh = S.shape(2, nm)
        f = S.facts(sh)
        bt = S.Batch(2, sh, 1, 1)
        pl = X.term_plan(P.CURVES[2], sh, bt.challenges[0])
        assert (f["T"], f["Tp"], f["npair"], f["nslots"], f["nsets"]) == (pl.T, pl.Tp, pl.npair, pl.nslots, pl.S), nm
        assert U.to_product_shape(2, sh).layout()[2] == f["nsets"]
        assert f["L"][6] == 33 + 65 * (sh.points_per_proof() - f["nsets"]) + 33 * sh.scalars_per_proof() + 7


def test_squeeze_offsets_are_the_oracles(monkeypatch):
    """facts()' L_k against the bytes the Python transcript really absorbs
    before each squeeze (counted in a subclass), on every edge shape and some
    directed ones: the residues asserted in test_coverage are those hashed."""
    made = []

    class Counting(T.Blake2bTranscript):
        def __init__(self, r):
            super().__init__(r)
            self.n, self.at = 0, []
            made.append(self)

        def common_point(self, pt, lookup_z=False):
            self.n += 65 if pt is not None else 0
            super().common_point(pt, lookup_z)

        def common_scalar(self, s):
            self.n += 33
            super().common_scalar(s)

        def squeeze_challenge(self):
            self.n += 1
            self.at.append(self.n)
            return super().squeeze_challenge()

    monkeypatch.setattr(T, "Blake2bTranscript", Counting)
    for nm in list(S.EDGES) + ["mixed", "lookups3", "perm_ragged", "sets64"]:
        sh = S.shape(1, nm)
        pf = S.Batch(1, sh, 1, 2).proof(0)
        got, _ = T.replay_challenges(P.CURVES[1], sh, pf, 12345)
        assert made[-1].at == S.facts(sh)["L"], nm
        monkeypatch.undo()          # the counting subclass hashed what the oracle hashes
        assert T.replay_challenges(P.CURVES[1], sh, pf, 12345)[0] == got
        monkeypatch.setattr(T, "Blake2bTranscript", Counting)


# --------------------------------------------------------------------- limits
def _layout(cid, sh):
    return U.to_product_shape(cid, sh).layout()


def test_limits_through_host_validation():
    """pm_shape_layout (acc_validate) refuses each shape one past a bound and
    accepts the bound itself."""
    c = 2
    _layout(c, S._bf_shape(c, 61))
    with pytest.raises(H.PmError, match="blinding_factors too large"):
        _layout(c, S._bf_shape(c, 62, 7))
    _layout(c, S.build(c, gates=[S.nested_sum(16)]))
    with pytest.raises(H.PmError, match="deeper than 16"):
        _layout(c, S.build(c, gates=[S.nested_sum(17)]))
    with pytest.raises(H.PmError, match="deeper than 16"):
        _layout(c, S.build(c, nl=1, lk_tab=[S.nested_sum(17)]))
    assert _layout(c, S.sets_shape(c, 64))[2] == 64
    with pytest.raises(H.PmError, match="too many rotation sets"):
        _layout(c, S.sets_shape(c, 65))
    ok = S._perm(c, 2, 1)
    _layout(c, ok)
    with pytest.raises(H.PmError, match="perm_chunk_len = 0"):
        _layout(c, S._perm(c, 2, 0))
    assert _layout(c, S.build(c, chunk=0))[0] == S.build(c, chunk=0).points_per_proof()   # chunk 0, no columns
    assert _layout(c, S.build(c, chunk=3)) == _layout(c, S.build(c, chunk=0))             # a chunk length alone adds nothing
    _layout(c, S.build(c, gates=[A.Const(1)], adv_q=[], na=0))                            # one expression, no column at all
    with pytest.raises(H.PmError, match="no expressions"):
        _layout(c, S.build(c, gates=[]))
    assert S.legal(c, S.build(c, gates=[])) == "no expressions"
    assert S.legal(c, S._perm(c, 2, 0)) and S.legal(c, S.sets_shape(c, 65)) and S.legal(c, S._bf_shape(c, 62, 7))
    assert S.legal(c, S.build(c, gates=[S.nested_sum(17)])) == "stack"


def test_oracle_accepts_empty_arguments():
    """The oracle on the shapes it used to refuse: perm_chunk_len = 0 without a
    permutation, no lookups, no instance / fixed columns, no gates."""
    sh = S.shape(0, "gates_only")
    assert sh.perm_chunk_len == 0 and sh.n_perm_sets == 0 and sh.scalar_offsets()["perm"][1] == 0
    d = A._split(sh, S.Batch(0, sh, 1, 3).proof(0))
    assert A.permutation_expressions(P.CURVES[0].r, sh, d, 1, 2, 3, 4, 5, 6) == []
    with pytest.raises(ValueError):
        S._perm(0, 2, 0).n_perm_sets


# ---------------------------------- the references the GPU module compares with
@pytest.mark.parametrize("cid,name", [(0, "gates_only"), (1, "bf1"), (2, "bf1"), (2, "wide_np8_14")])
def test_scalar_block_values_references(cid, name):
    """The special scalar-block values (shape_util.scalar_block_reference): the
    C port's status equals proof_status for every proof (a zero denominator
    for exactly the x = omega^-i), and its quads and h_eval equal both Python
    restatements for every clean proof (the wide shape: the x cases, u and v
    = 0, the evaluation cases and the plain one)."""
    assert name in S.SCALAR_BLOCK_SHAPES
    bt, names, ps, arrs, q, h, st = S.scalar_block_reference(cid, name)
    C, sh = bt.C, bt.sh
    assert bt.B <= 33 and len(set(names)) == bt.B
    poles = [b for b, nm in enumerate(names) if nm.startswith("x=omega^-")]
    assert len(poles) == sh.blinding_factors + 2
    ran = 0
    for b, nm in enumerate(names):
        assert st[b] == bt.status(b) == (A.STATUS_DENOM_ZERO if b in poles else 0), nm
        if b in poles:
            assert 0 < b < bt.B - 1 and b - 1 not in poles and b + 1 not in poles    # clean neighbours
            continue
        if name.startswith("wide") and not nm.startswith(("x", "u=0", "v=0", "evals", "plain")):
            continue
        pf = bt.proof(b)
        r1, r2 = A.accumulate(C, sh, pf), A.accumulate_msm(C, sh, pf)
        assert r1 == r2, nm
        qq, hh = A.pack_result(C, r2)
        assert np.array_equal(qq, q[b]) and np.array_equal(hh, h[b]), nm
        ran += 1
    assert ran >= 7
    b = names.index("x=0")
    assert not q[b][1].any()            # zw = [0]W: the identity, stored as zero words


BYTES_CASES = [(c, nm) for nm in list(S.DIRECTED) + list(S.WIDE) for c in ((0, 1, 2) if nm in ("bf0", "mixed") else (2,))]


@pytest.mark.parametrize("cid,name", BYTES_CASES)
def test_bytes_references(cid, name):
    """shape_util.bytes_reference: the C port's decode flags exactly the proof
    with the bad point and the one with the bad scalar, as the Python parser
    does; its decoded inputs equal the parser's; proof 0's challenges, quad
    and h_eval equal the Python replay and accumulator."""
    bt, ps, datas, inst, vk, out = S.bytes_reference(cid, name)
    C, sh = bt.C, bt.sh
    ni = sh.num_instance_columns
    vkr, _ = S.vk_repr(cid, name)
    for b, d in enumerate(datas):
        pts, scs, stp = PB.parse(C, sh, d, bt.proof(b).points[:ni])
        want = PB.STATUS_BAD_POINT if b == S.BAD_POINT_AT else PB.STATUS_BAD_SCALAR if b == S.BAD_SCALAR_AT else 0
        assert stp == want and out["status"][b] & (PB.STATUS_BAD_POINT | PB.STATUS_BAD_SCALAR) == want, b
        pp, ss, _ = A.pack_proofs(C, sh, [A.Proof(points=pts, scalars=scs, challenges=[0] * 7)])
        assert np.array_equal(out["points"][b], pp[0]) and np.array_equal(out["scalars"][b], ss[0]), b
        ch, stt = T.replay_challenges(C, sh, A.Proof(points=pts, scalars=scs, challenges=[]), vkr)
        assert np.array_equal(out["challenges"][b], S.limbs(C, ch)), b
        assert out["status"][b] == want | stt | A.proof_status(C, sh, ch), b
        if b == 0 and name not in S.HEAVY:
            qq, hh = A.pack_result(C, A.accumulate_msm(C, sh, A.Proof(points=pts, scalars=scs, challenges=ch)))
            assert np.array_equal(out["quads"][0], qq) and np.array_equal(out["h_eval"][0], hh)
    assert any(sh_.num_instance_columns == 0 for sh_ in (S.shape(2, nm) for _, nm in BYTES_CASES))


@pytest.mark.parametrize("cid", CURVES)
def test_transcript_references(cid):
    """shape_util.transcript_reference on an edge shape: the proof with the
    identity commitment is flagged (its record is skipped), the C port's
    replay equals hashlib's on all 17 proofs."""
    name = sorted(S.EDGES)[cid]
    bt, ps, pts, scs, vk, ch, st = S.transcript_reference(cid, name, 17, 5)
    assert st.tolist() == [T.STATUS_IDENTITY_SKIPPED if b == 5 else 0 for b in range(17)]
    chc, _, _, stc = R.accum_batch(cid, ps.c, pts, scs, vk_repr=vk, threads=4)
    assert np.array_equal(chc, ch) and np.array_equal(stc & 3, st)

"""GPU: the BN254 pairing decider (pm_accum_decide_device, pm_pairing_check_device,
pm_accum_decide) against the host form pm_accum_decide_host, bit for bit on
out_ok, out_status and out_gt, and against tests/pairing_ref.py directly.

Layout under test (pairing_plan.hpp): 6 lanes per item, 10 items per wave, one
wave per block, so P_wave = P_block = 10 and the batch sizes are
B in {1, 2, P_wave - 1, P_wave, P_wave + 1 (= P_block + 1), 2 P_block + 3}
   = {1, 2, 9, 10, 11, 23}.
Accepting and rejecting items alternate (pairing_util.batch), so neighbours in
one group of lanes, in one wave and across a wave boundary decide differently.
The expected decisions are pairing_util's, stated from the discrete logs."""
import re
import os

import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_WAVE = 10
P_BLOCK = 10
SIZES = sorted({1, 2, P_WAVE - 1, P_WAVE, P_WAVE + 1, P_BLOCK + 1, 2 * P_BLOCK + 3})
SENT32 = 0xA5A5A5A5
SENT64 = 0x5A5A5A5A5A5A5A5A


def test_sizes_follow_the_plan():
    src = open(os.path.join(ROOT, "halo2-aggregation_amd", "csrc", "pairing_plan.hpp")).read()
    g = int(re.search(r"constexpr int kPairG = (\d+);", src).group(1))
    wave = int(re.search(r"constexpr int kPairWave = (\d+);", src).group(1))
    assert re.search(r"constexpr int kPairBlock = kPairWave;", src)
    assert wave // g == P_WAVE == P_BLOCK
    assert SIZES == [1, 2, 9, 10, 11, 23]


@pytest.fixture(scope="module")
def pairings(gpu_ctx):
    g2 = U.g2_words(PR.G2)
    return {tau: H.Pairing(gpu_ctx, g2, U.g2_words(U.s_g2(tau))) for tau in (U.TAU, U.TAU2)}


@pytest.fixture(scope="module")
def batches(pairings):
    """per tau: the largest batch and the host form's answer for it, computed once"""
    out = {}
    for tau, pr in pairings.items():
        q, si, ok, st = U.batch(max(SIZES), tau)
        h_ok, h_st, h_gt = H.accum_decide_host(pr, q, si, want_gt=True)
        assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)
        out[tau] = (q, si, h_ok, h_st, h_gt)
    return out


def _dev(gpu_ctx, a):
    a = np.ascontiguousarray(a)
    v = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)
    return torch.from_numpy(v.copy()).to(torch.device("cuda", gpu_ctx.device))


def _out(gpu_ctx, n, dtype, sentinel, tail=8):
    """n words of output followed by `tail` sentinel words"""
    bits = 64 if dtype == torch.int64 else 32
    signed = sentinel - (1 << bits) if sentinel >> (bits - 1) else sentinel
    return torch.full((n + tail,), signed, dtype=dtype, device=torch.device("cuda", gpu_ctx.device))


def _run(gpu_ctx, pr, q, si, want_gt=True, pairs=False):
    B = q.shape[0]
    d_q, d_si = _dev(gpu_ctx, q), _dev(gpu_ctx, si)
    d_ok = _out(gpu_ctx, B, torch.int32, SENT32)
    d_st = _out(gpu_ctx, B, torch.int32, SENT32)
    d_gt = _out(gpu_ctx, 48 * B, torch.int64, SENT64)
    torch.cuda.synchronize()
    fn = gpu_ctx.pairing_check_device if pairs else gpu_ctx.accum_decide_device
    fn(pr, B, d_q.data_ptr(), d_ok.data_ptr(), d_status_in=d_si.data_ptr(), d_status=d_st.data_ptr(),
       d_gt=d_gt.data_ptr() if want_gt else 0)
    ok = d_ok.cpu().numpy().view(np.uint32)
    st = d_st.cpu().numpy().view(np.uint32)
    gt = d_gt.cpu().numpy().view(np.uint64)
    # a sentinel behind every output is intact, and the inputs are unchanged
    assert (ok[B:] == SENT32).all() and (st[B:] == SENT32).all() and (gt[48 * B:] == SENT64).all()
    if not want_gt:
        assert (gt == SENT64).all()
    assert np.array_equal(d_q.cpu().numpy().view(np.uint64), q) and np.array_equal(d_si.cpu().numpy().view(np.uint32), si)
    return ok[:B], st[:B], gt[:48 * B].reshape(B, 12, 4)


@pytest.mark.parametrize("B", SIZES)
def test_device_matches_host_form(gpu_ctx, pairings, batches, B):
    q, si, h_ok, h_st, h_gt = batches[U.TAU]
    ok, st, gt = _run(gpu_ctx, pairings[U.TAU], q[:B], si[:B])
    assert np.array_equal(ok, h_ok[:B]), (ok, h_ok[:B])
    assert np.array_equal(st, h_st[:B])
    assert np.array_equal(gt, h_gt[:B])
    ok2, st2, _ = _run(gpu_ctx, pairings[U.TAU], q[:B], si[:B], want_gt=False)
    assert np.array_equal(ok2, ok) and np.array_equal(st2, st)


def test_families_decide_as_constructed(gpu_ctx, pairings):
    fam = U.family()
    q = np.stack([f[1] for f in fam])
    si = np.array([f[2] for f in fam], dtype=np.uint32)
    ok, st, gt = _run(gpu_ctx, pairings[U.TAU], q, si)
    for f, o, s in zip(fam, ok, st):
        assert (int(o), int(s)) == (f[3], f[4]), f[0]
    names = [f[0] for f in fam]
    assert int(st[names.index("off_curve")]) == H.DECIDE_NOT_ON_CURVE == 8
    assert not gt[names.index("status_in")].any() and not gt[names.index("off_curve")].any()


def test_gt_matches_reference(gpu_ctx, pairings):
    """out_gt of 4 items against tests/pairing_ref.py itself"""
    fam = {f[0]: f for f in U.family()}
    pick = ["accept", "reject_d_plus_1", "zw_eq_f_reject", "w_inf_sum_not_inf"]
    q = np.stack([fam[n][1] for n in pick])
    _, _, gt = _run(gpu_ctx, pairings[U.TAU], q, np.zeros(4, dtype=np.uint32))
    for i, n in enumerate(pick):
        assert np.array_equal(gt[i], U.ref_gt_words(q[i])), n
    one = np.array(PR.gt_words(PR.F12_ONE), dtype=np.uint64).reshape(12, 4)
    assert np.array_equal(gt[0], one)


def test_two_pairings_alternate_on_one_context(gpu_ctx, pairings, batches):
    for tau in (U.TAU, U.TAU2, U.TAU, U.TAU2):
        q, si, h_ok, h_st, h_gt = batches[tau]
        ok, st, gt = _run(gpu_ctx, pairings[tau], q[:11], si[:11])
        assert np.array_equal(ok, h_ok[:11]) and np.array_equal(st, h_st[:11]) and np.array_equal(gt, h_gt[:11])
    # an item built for one tau is rejected under the other
    q, si, h_ok, _, _ = batches[U.TAU]
    ok, _, _ = _run(gpu_ctx, pairings[U.TAU2], q[:1], si[:1])
    assert h_ok[0] == 1 and ok[0] == 0


def test_pair_check_matches_decide(gpu_ctx, pairings, batches):
    """pm_pairing_check_device on (w, -(zw + f + e)) gives what pm_accum_decide_device gives on the quad"""
    q, si, h_ok, h_st, h_gt = batches[U.TAU]
    B = 11
    pairs = np.zeros((B, 2, 8), dtype=np.uint64)
    for i in range(B):
        pts = [U.ref_point(q[i, j]) for j in range(4)]
        ok_curve = all(PR.g1_on_curve(p) for p in pts)
        pairs[i, 0] = q[i, 0]
        if ok_curve:
            c = PR.g1_neg(PR.g1_add(PR.g1_add(pts[1], pts[2]), pts[3]))
            pairs[i, 1] = np.array(PR.g1_words(c), dtype=np.uint64)
        else:
            pairs[i, 1] = q[i, 2]  # the off-curve point stays in the pair
    ok, st, gt = _run(gpu_ctx, pairings[U.TAU], pairs, si[:B], pairs=True)
    assert np.array_equal(ok, h_ok[:B]) and np.array_equal(st, h_st[:B]) and np.array_equal(gt, h_gt[:B])


def test_host_pointer_form(gpu_ctx, pairings, batches):
    q, si, h_ok, h_st, h_gt = batches[U.TAU]
    ok, st, gt = gpu_ctx.accum_decide(pairings[U.TAU], q[:11], si[:11], want_gt=True)
    assert np.array_equal(ok, h_ok[:11]) and np.array_equal(st, h_st[:11]) and np.array_equal(gt, h_gt[:11])
    ok, st = gpu_ctx.accum_decide(pairings[U.TAU], q[:2])
    assert list(ok) == [1, 0]


def test_host_only_pairing_is_refused_by_device_entries(gpu_ctx):
    pr = H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2()))
    q, _, _, _ = U.batch(1)
    with pytest.raises(H.PmError, match="without a context"):
        gpu_ctx.accum_decide(pr, q)


def test_verify_proofs_device_chains_accumulator_and_decider(gpu_ctx, pairings):
    """Context.verify_proofs_device = pm_accum_batch_proofs_device then pm_accum_decide_device with the
    accumulator's status buffer as status in and out.  The synthetic proofs carry random W_j, so every
    proof is rejected; the decisions, status words and out_gt equal the host form's on the quads the
    accumulator wrote, and a proof with a corrupted scalar keeps its decoder status and is not evaluated."""
    import workloads as Wk

    B = 5
    shape = Wk.simple_example_shape(gpu_ctx, H.BN254, 14)
    batch = Wk.SyntheticBatch(gpu_ctx, shape, B, seed=0xDEC1)
    batch.to_proof_bytes(shape)
    # proof 2: its first scalar >= r (PM_PROOF_BAD_SCALAR)
    npts, nsc, nsets = shape.layout()
    off = 32 * (npts - nsets - shape.c.num_instance_columns)
    batch.proofs[2, off:off + 32] = 0xFF
    d_ok = _out(gpu_ctx, B, torch.int32, SENT32)
    d_gt = _out(gpu_ctx, 48 * B, torch.int64, SENT64)
    torch.cuda.synchronize()
    pr = pairings[U.TAU]
    gpu_ctx.verify_proofs_device(shape, pr, B, batch.vk_repr, batch.proofs.data_ptr(), batch.psize,
                                 batch.inst.data_ptr(), batch.challenges.data_ptr(), batch.quads.data_ptr(),
                                 batch.status.data_ptr(), d_ok.data_ptr(), d_h=batch.h_eval.data_ptr(),
                                 d_gt=d_gt.data_ptr())
    ok = d_ok.cpu().numpy().view(np.uint32)
    st = batch.status.cpu().numpy().view(np.uint32)
    gt = d_gt.cpu().numpy().view(np.uint64)
    quads = batch.quads.cpu().numpy().view(np.uint64)
    assert (ok[B:] == SENT32).all() and (gt[48 * B:] == SENT64).all()
    assert st[2] & H.PROOF_BAD_SCALAR and not st[[0, 1, 3, 4]].any()
    h_ok, h_st, h_gt = H.accum_decide_host(pr, quads, st, want_gt=True)
    assert np.array_equal(ok[:B], h_ok) and np.array_equal(st, h_st)
    assert np.array_equal(gt[:48 * B].reshape(B, 12, 4), h_gt)
    assert not ok[:B].any() and not h_gt[2].any() and h_gt[0].any()


# ---- end to end from proof bytes: valid proofs, as the accumulator writes their quads, are accepted
E2E_SEED = 0xE2E
E2E_LOGN = 10  # the smallest k of the existing proof-byte tests (test_decode_vs_oracle)


def _honest_proofs(B, tau):
    """B simple-example BN254 proofs whose W_j are the honest KZG witnesses for the SRS secret tau.
    Every point of a synthetic proof and of the synthetic VK has a known discrete log, and v, u are
    squeezed before the W_j are read, so: replay the transcript, take each rotation set's batched
    commitment discrete log F_j = sum_i v^(m-1-i) log(C_i) (H expanded as sum h_i xn^i) and
    evaluation e_j with the accumulator's own queries and coefficients (oracle/accum.py), and put
    W_j = [(F_j - e_j) / (tau - z_j)]G in the proof."""
    import accum as A
    import accum_util as AU
    import pasta as P
    import transcript as T

    C, sh, proofs = AU.make_case(2, "simple", E2E_LOGN, B, E2E_SEED)
    r = C.r
    assert r == PR.R
    vkr = T.vk_repr(r, b"pairing end to end")
    T.with_replayed_challenges(C, sh, proofs, vkr)
    po = sh.point_offsets()
    vk_seed = E2E_SEED ^ 0x7EC
    for b, pf in enumerate(proofs):
        dl = [P.synth_base_dlog(C, E2E_SEED, b * 4096 + i) for i in range(sh.points_per_proof())]
        x, v = pf.challenges[4], pf.challenges[5]
        d = A._split(sh, pf)
        _, xn, h_eval = A.scalar_block(C, sh, d, pf.challenges)

        def dlog(ref):
            if ref == A.H_POINT:
                return sum(dl[po["h"][0] + i] * pow(xn, i, r) for i in range(po["h"][1])) % r
            kind, i = ref
            if kind == "proof":
                return dl[i]
            return P.synth_base_dlog(C, vk_seed, i if kind == "fixed" else 1000 + i)

        sets = A.construct_intermediate_sets(A.build_queries(sh, d, h_eval))
        assert len(sets) == po["W"][1]
        for j, (rot, qs) in enumerate(sets):
            m = len(qs)
            F = sum(pow(v, m - 1 - i, r) * dlog(ref) for i, (ref, _, _) in enumerate(qs)) % r
            e = sum(pow(v, m - 1 - i, r) * ev for i, (_, _, ev) in enumerate(qs)) % r
            z = pow(sh.omega, rot % (1 << sh.log_n), r) * x % r
            pf.points[po["W"][0] + j] = C.mul(PR.honest_W(F, e, z, tau), C.gen)
        # the challenges do not depend on the W_j
        assert T.replay_challenges(C, sh, pf, vkr)[0] == pf.challenges
    return C, sh, proofs, vkr


def _verify_bytes(gpu_ctx, pr, ps, datas, inst, vk):
    """pm_accum_batch_proofs_device then pm_accum_decide_device on device buffers -> (ok, status, quads)"""
    B = len(datas)
    dev = torch.device("cuda", gpu_ctx.device)
    psize = H.proof_size(ps)
    buf = np.stack([np.frombuffer(d, dtype=np.uint8) for d in datas])
    assert buf.shape == (B, psize) and psize % 4 == 0
    d_pf = torch.from_numpy(buf.copy()).to(dev)
    d_in = _dev(gpu_ctx, inst)
    d_ch = torch.zeros((B, 7, 4), dtype=torch.int64, device=dev)
    d_q = torch.zeros((B, 4, 8), dtype=torch.int64, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_ok = _out(gpu_ctx, B, torch.int32, SENT32)
    torch.cuda.synchronize()
    gpu_ctx.accum_batch_proofs_device(ps, B, vk, d_pf.data_ptr(), psize, d_in.data_ptr(), d_ch.data_ptr(),
                                      d_q.data_ptr(), 0, d_st.data_ptr())
    gpu_ctx.accum_decide_device(pr, B, d_q.data_ptr(), d_ok.data_ptr(), d_status_in=d_st.data_ptr(),
                                d_status=d_st.data_ptr())
    ok = d_ok.cpu().numpy().view(np.uint32)
    assert (ok[B:] == SENT32).all()
    return ok[:B], d_st.cpu().numpy().view(np.uint32), d_q.cpu().numpy().view(np.uint64)


def test_end_to_end_from_proof_bytes(gpu_ctx, pairings):
    """B = 5 valid proofs from their bytes: all accepted.  Then the low byte of one evaluation of proof 2
    flipped and one W_j of proof 4 replaced: exactly those two rejected.  The host form agrees on the
    quads, and the quad of a valid proof is the oracle accumulator's."""
    import accum as A
    import accum_util as AU
    import pasta as P
    import proof_bytes as PB

    B = 5
    C, sh, proofs, vkr = _honest_proofs(B, U.TAU)
    ps = AU.to_product_shape(2, sh)
    ni = sh.num_instance_columns
    vk = np.array(A.to_limbs_mont(C.r, vkr), dtype=np.uint64)
    inst = np.array([[P.point_to_limbs(C, q) for q in pf.points[:ni]] for pf in proofs], dtype=np.uint64)
    datas = [PB.serialize(C, sh, pf) for pf in proofs]
    pr = pairings[U.TAU]

    ok, st, quads = _verify_bytes(gpu_ctx, pr, ps, datas, inst, vk)
    assert not st.any()
    assert list(ok) == [1] * B, list(ok)
    # as the accumulator writes it: the oracle's quad, bit for bit, and its e is the negated evaluation
    q0, _ = A.pack_result(C, A.accumulate_msm(C, sh, proofs[0]))
    assert np.array_equal(quads[0], q0)
    h_ok, h_st = H.accum_decide_host(pr, quads, st)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)
    # the same proofs under another SRS secret are all rejected
    ok2, _, _ = _verify_bytes(gpu_ctx, pairings[U.TAU2], ps, datas, inst, vk)
    assert not ok2.any()

    items = PB.proof_items(sh)
    bad = [bytearray(d) for d in datas]
    j_eval = next(j for j, (k, _) in enumerate(items) if k == "sc")
    bad[2][32 * j_eval] ^= 0x01  # low byte of the first evaluation of proof 2
    assert int.from_bytes(bad[2][32 * j_eval:32 * j_eval + 32], "little") < C.r
    j_w = next(j for j, (k, i) in enumerate(items) if k == "pt" and i == sh.point_offsets()["W"][0])
    bad[4][32 * j_w:32 * j_w + 32] = PB.encode_point(C, A.synth_point(C, 0xBAD, 4))  # W_0 of proof 4
    ok, st, quads = _verify_bytes(gpu_ctx, pr, ps, [bytes(d) for d in bad], inst, vk)
    assert not st.any()
    assert list(ok) == [1, 1, 0, 1, 0], list(ok)
    h_ok, h_st = H.accum_decide_host(pr, quads, st)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)

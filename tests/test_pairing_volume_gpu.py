"""GPU: the pairing decider past its residency limit, at every position of a
wave, and with other G2 arguments.

tests/test_pairing_gpu.py stops at B = 23, three one-wave blocks.  LDS allows 3
blocks of k_pairing_run per CU, so with B = 30 CUs + 11 items (7691 on 256 CUs,
770 blocks) blocks are co-resident on a CU, there are more blocks than CUs, and
a second round starts: the smallest batch that reaches all three.  Every item of
it is compared with the host form pm_accum_decide_host (pinned to the reference in
tests/test_pairing_host.py), and the decisions with the construction
(pairing_util.walk: B distinct items, one affine addition per point).

Times on one MI355X (pytest --durations, the walk and the host form's answer
are built once in a module fixture and counted with the first test that uses it):
    test_past_the_residency_limit      1.1 s fixture (walk of 7691 items, host form) + 0.8 s
    test_position_independence         0.4 s
    test_neighbours_at_infinity_...    0.1 s
    test_other_g2_arguments            0.5 s each of 4
    test_pairs_entry_at_volume         0.2 s
    the whole file                     6.7 s
"""
import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest
import test_pairing_gpu as TG
import torch

pytestmark = pytest.mark.gpu

P_BLOCK = TG.P_BLOCK
K_ALT = 0x5555555555555555555555555555555555555555555555555555555555555555 % PR.R   # 0101...
K_RUNS = 0x0000FFFFFFFF0000000000000000FFFF00000000FFFFFFFFFFFF000000000001 % PR.R  # long runs of ones and zeros
TAU3 = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % PR.R
ONE = np.array(PR.gt_words(PR.F12_ONE), dtype=np.uint64).reshape(12, 4)


@pytest.fixture(scope="module")
def pairing(gpu_ctx):
    return H.Pairing(gpu_ctx, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


@pytest.fixture(scope="module")
def cus(gpu_ctx):
    return torch.cuda.get_device_properties(gpu_ctx.device).multi_processor_count


@pytest.fixture(scope="module")
def volume(pairing, cus):
    """the walk of B = 30 CUs + 11 items and the host form's answer for every one of them"""
    B = 3 * P_BLOCK * cus + 11
    q, si, ok, st = U.walk(B)
    h_ok, h_st, h_gt = H.accum_decide_host(pairing, q, si, want_gt=True)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)
    return q, si, ok, st, h_gt


def test_past_the_residency_limit(gpu_ctx, pairing, cus, volume):
    """B = 30 CUs + 11: co-resident blocks, more blocks than CUs, a second round.  ok and status as
    constructed; ok, status and all 48 B words equal the host form's; sentinels and inputs intact
    (TG._run); the first and last item and the two around the end of the first round against
    pairing_ref."""
    q, si, ok, st, h_gt = volume
    B = q.shape[0]
    assert B == 30 * cus + 11 and (B + P_BLOCK - 1) // P_BLOCK > 3 * cus
    d_ok, d_st, d_gt = TG._run(gpu_ctx, pairing, q, si)
    assert np.array_equal(d_ok, ok), np.flatnonzero(d_ok != ok)[:10]
    assert np.array_equal(d_st, st), np.flatnonzero(d_st != st)[:10]
    bad = np.flatnonzero((d_gt != h_gt).reshape(B, -1).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:10])
    edge = 3 * cus * P_BLOCK   # the first item of the block after 3 blocks per CU
    for i in (0, edge - 1, edge, B - 1):
        assert st[i] == 0
        want = U.ref_gt_words(q[i])
        assert np.array_equal(d_gt[i], want), i
        assert np.array_equal(want, ONE) == bool(ok[i])
    assert ok[edge - 1] != ok[edge]


def test_position_independence(gpu_ctx, pairing):
    """an accepting and a rejecting item in all 10 group positions of a wave with the other as
    neighbour (B = 20), and alone in the last, partly filled block (B = 11): identical words"""
    fam = {f[0]: f for f in U.family()}
    acc, rej = fam["accept"][1], fam["reject_d_plus_1"][1]
    want = {1: U.ref_gt_words(acc), 0: U.ref_gt_words(rej)}
    assert np.array_equal(want[1], ONE) and not np.array_equal(want[0], ONE)
    # block 0: accept at even positions, block 1: at odd ones
    kind = np.array([(i + i // P_BLOCK + 1) % 2 for i in range(2 * P_BLOCK)])
    for item in (0, 1):
        assert sorted(i % P_BLOCK for i in np.flatnonzero(kind == item)) == list(range(P_BLOCK))
    q = np.stack([acc if k else rej for k in kind])
    ok, st, gt = TG._run(gpu_ctx, pairing, q, np.zeros(len(kind), dtype=np.uint32))
    assert np.array_equal(ok, kind) and not st.any()
    for i, k in enumerate(kind):
        assert np.array_equal(gt[i], want[int(k)]), i
    for last, other in ((acc, rej), (rej, acc)):
        q = np.stack([other] * P_BLOCK + [last])
        ok, st, gt = TG._run(gpu_ctx, pairing, q, np.zeros(P_BLOCK + 1, dtype=np.uint32))
        k = int(last is acc)
        assert list(ok) == [1 - k] * P_BLOCK + [k]
        assert np.array_equal(gt[P_BLOCK], want[k]) and all(np.array_equal(g, want[1 - k]) for g in gt[:P_BLOCK])


def test_neighbours_at_infinity_do_not_leak(gpu_ctx, pairing):
    """an item among nine that carry status_in != 0 (their flags put both points at infinity and
    their lines are 1) gives the words it gives alone, at each of the 10 positions"""
    fam = {f[0]: f for f in U.family()}
    for name in ("reject_d_plus_1", "zw_eq_f_accept"):
        item = fam[name][1]
        ok1, st1, gt1 = TG._run(gpu_ctx, pairing, item[None], np.zeros(1, dtype=np.uint32))
        assert ok1[0] == fam[name][3] and st1[0] == 0 and gt1[0].any()
        for pos in range(P_BLOCK):
            q = np.stack([fam["accept"][1]] * P_BLOCK)
            q[pos] = item
            si = np.full(P_BLOCK, 0x21, dtype=np.uint32)
            si[pos] = 0
            ok, st, gt = TG._run(gpu_ctx, pairing, q, si)
            assert np.array_equal(st, si) and ok[pos] == ok1[0] and not np.delete(ok, pos).any()
            assert np.array_equal(gt[pos], gt1[0]), (name, pos)
            assert not np.delete(gt, pos, axis=0).any()


@pytest.mark.parametrize("k,tau", [(K_ALT, U.TAU), (K_RUNS, U.TAU), (K_RUNS, TAU3), (1, TAU3)],
                         ids=["k_alt", "k_runs", "k_runs_tau3", "g2_tau3"])
def test_other_g2_arguments(gpu_ctx, pairing, k, tau):
    """(g2, s_g2) = ([k]G2, [k tau]G2): the product is the k-th power of the one under (G2, [tau]G2), so
    the decisions stand; the 204 line coefficients are all different"""
    g2, s_g2 = PR.g2_mul(k, PR.G2), PR.g2_mul(k * tau, PR.G2)
    pr = H.Pairing(gpu_ctx, U.g2_words(g2), U.g2_words(s_g2))
    q, si, ok, st = U.batch(23, tau)
    h_ok, h_st, h_gt = H.accum_decide_host(pr, q, si, want_gt=True)
    d_ok, d_st, d_gt = TG._run(gpu_ctx, pr, q, si)
    assert np.array_equal(d_ok, ok) and np.array_equal(d_st, st)
    assert np.array_equal(h_ok, ok) and np.array_equal(h_st, st)
    assert np.array_equal(d_gt, h_gt)
    for i in (0, 1):   # one accepted, one rejected: against pairing_ref with these G2 points
        w, zw, f, e = (U.ref_point(q[i, j]) for j in range(4))
        want = np.array(PR.gt_words(PR.accum_gt(w, zw, f, e, s_g2, g2)), dtype=np.uint64).reshape(12, 4)
        assert np.array_equal(d_gt[i], want), i
        assert np.array_equal(want, ONE) == bool(ok[i])
    assert ok[0] == 1 and ok[1] == 0 and st[0] == 0 and st[1] == 0
    if k != 1:
        # accepted under (G2, [tau]G2) and under ([k]G2, [k tau]G2); rejected under ([k]G2, [tau]G2)
        if tau == U.TAU:
            assert TG._run(gpu_ctx, pairing, q[:1], si[:1])[0][0] == 1
        mixed = H.Pairing(gpu_ctx, U.g2_words(g2), U.g2_words(U.s_g2(tau)))
        m_ok, m_st, m_gt = TG._run(gpu_ctx, mixed, q[:1], si[:1])
        assert m_ok[0] == 0 and m_st[0] == 0
        assert np.array_equal(m_gt, H.accum_decide_host(mixed, q[:1], si[:1], want_gt=True)[2])


def test_pairs_entry_at_volume(gpu_ctx, pairing, cus, volume):
    """pm_pairing_check_device on (w, -(zw + f + e)) of the walk's first 10 CUs + 11 items: the ok and
    out_gt of the quad entry"""
    q, si, ok, st, h_gt = volume
    B = P_BLOCK * cus + 11
    q, si = q[:B], si[:B]
    C = U.C
    pairs = np.zeros((B, 2, 8), dtype=np.uint64)
    pairs[:, 0] = q[:, 0]
    for i in range(B):
        if i == U.WALK_OFF_CURVE:
            pairs[i, 1] = q[i, 1]   # the point off the curve stays in the pair
            continue
        zw, f, e = (U.P.limbs_to_point(C, [int(v) for v in q[i, j]]) for j in (1, 2, 3))
        pairs[i, 1] = U.words(C.neg(C.add(C.add(zw, f), e)))
    q_ok, q_st, q_gt = TG._run(gpu_ctx, pairing, q, si)
    p_ok, p_st, p_gt = TG._run(gpu_ctx, pairing, pairs, si, pairs=True)
    assert np.array_equal(q_ok, ok[:B]) and np.array_equal(q_st, st[:B]) and np.array_equal(q_gt, h_gt[:B])
    assert np.array_equal(p_ok, q_ok) and np.array_equal(p_st, q_st)
    bad = np.flatnonzero((p_gt != q_gt).reshape(B, -1).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:10])

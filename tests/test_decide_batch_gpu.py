"""GPU: the batch decider (pm_accum_decide_batch_device, pm_accum_decide_batch,
pm_verify_proofs_batch_device) against the host form pm_accum_decide_batch_host
and against tests/decide_batch_util.py's expectations from the discrete logs:
ok, status, L and R bit for bit.

Geometry under test (pairing_batch_plan.hpp): 64 quads per block, at most kBatchKq
= 8 items per quad and slice, so one slice holds 512 items and B = 513 is the
first batch whose window sums are folded from two slices by ticket; a chunk is
2^16 items, crossed here at 64 through the PM_DECIDE_BATCH_CHUNK test hook.

Not reachable from a seed: a coefficient with all 128 bits set (2^-128 per draw).
The recoding's extremes (all ones, the carry out of the top nibble) are
exercised in tests/native/decide_batch_host.cpp only."""
import os
import re

import decide_batch_ref as BR
import decide_batch_util as D
import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT32 = 0xA5A5A5A5
SLICE = 8 * 64
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, SLICE, SLICE + 1]


def test_sizes_follow_the_plan():
    src = open(os.path.join(ROOT, "halo2-aggregation_amd", "csrc", "pairing_batch_plan.hpp")).read()
    quads = int(re.search(r"constexpr int kBatchQuads = (\d+);", src).group(1))
    kq = int(re.search(r"constexpr uint32_t kBatchKq = (\d+);", src).group(1))
    assert quads * kq == SLICE and SLICE + 1 in SIZES
    assert re.search(r"constexpr size_t kBatchChunk = size_t\(1\) << 16;", src)
    assert int(re.search(r"constexpr int kBatchWin = (\d+);", src).group(1)) == 33


@pytest.fixture(scope="module")
def pairing(gpu_ctx):
    return H.Pairing(gpu_ctx, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


@pytest.fixture(scope="module")
def pool():
    """the largest batch: accepting items over 16 types (64 pool points), one rejecting item near the
    end, computed once; a prefix of B <= 512 items is an accepting batch"""
    logs = D.with_bad(D.accepting(SLICE + 1), [SLICE])
    return logs, D.quads_from_logs(logs)


def _dev(gpu_ctx, a):
    a = np.ascontiguousarray(a)
    v = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32)
    return torch.from_numpy(v.copy()).to(torch.device("cuda", gpu_ctx.device))


def _out(gpu_ctx, n, tail=8):
    return torch.full((n + tail,), SENT32 - (1 << 32), dtype=torch.int32, device=torch.device("cuda", gpu_ctx.device))


def _run(gpu_ctx, pr, q, si=None, seed=D.SEED, locate=False, with_item=True):
    """-> dict(ok, pair, seed, status, item_ok); checks the sentinels and that the inputs are unchanged"""
    B = q.shape[0]
    d_q = _dev(gpu_ctx, q)
    d_si = _dev(gpu_ctx, si) if si is not None else None
    d_st, d_it = _out(gpu_ctx, B), _out(gpu_ctx, B)
    torch.cuda.synchronize()
    r = gpu_ctx.accum_decide_batch_device(pr, B, d_q.data_ptr(), d_status_in=d_si.data_ptr() if si is not None else 0,
                                          d_status=d_st.data_ptr(), seed=seed,
                                          d_item_ok=d_it.data_ptr() if with_item else 0, locate=locate)
    st = d_st.cpu().numpy().view(np.uint32)
    it = d_it.cpu().numpy().view(np.uint32)
    assert (st[B:] == SENT32).all() and (it[B:] == SENT32).all()
    assert np.array_equal(d_q.cpu().numpy().view(np.uint64).reshape(q.shape), q)
    if si is not None:
        assert np.array_equal(d_si.cpu().numpy().view(np.uint32), si)
    r["status"], r["item_ok"] = st[:B], it[:B]
    return r


@pytest.mark.parametrize("B", SIZES)
def test_device_matches_host_form_and_logs(gpu_ctx, pairing, pool, B):
    logs, quads = pool
    q = quads[:B]
    got = _run(gpu_ctx, pairing, q)
    ok, pair = D.expect(logs[:B], D.SEED)
    assert ok == (1 if B <= SLICE else 0)
    assert got["ok"] == ok and not got["status"].any() and got["seed"] == D.SEED
    assert np.array_equal(got["pair"], pair)
    host = H.accum_decide_batch_host(pairing, q, seed=D.SEED)
    assert host["ok"] == ok and np.array_equal(host["pair"], got["pair"]) and np.array_equal(host["status"], got["status"])
    assert (got["item_ok"] == SENT32).all()  # without PM_DECIDE_LOCATE the buffer keeps its sentinel


@pytest.mark.parametrize("B", [1, 2, 3, 17, 65])
def test_families(gpu_ctx, pairing, B):
    """identity w, identity sum, doubling in the three-point sum, off-curve, status_in: status words
    and sums equal the reference's, the decision and all words the host form's"""
    q, si, item_ok, item_st = D.family_batch(B)
    got = _run(gpu_ctx, pairing, q, si)
    host = H.accum_decide_batch_host(pairing, q, si, seed=D.SEED)
    assert np.array_equal(got["status"], item_st) and np.array_equal(host["status"], item_st)
    assert np.array_equal(got["pair"], host["pair"]) and got["ok"] == host["ok"] == (1 if item_ok.all() else 0)
    if B <= 17:
        _, L, R = BR.fold(q, si, D.SEED)
        assert np.array_equal(got["pair"], D.pair_words(L, R))


@pytest.mark.parametrize("chunk,B", [(64, 64), (64, 65), (64, 257), (128, 513)])
def test_chunked_batches(gpu_ctx, pairing, pool, chunk, B):
    """the chunk boundary (2^16 items; here through the test hook): one item just on each side of it,
    several chunks, and chunks that themselves take more than one quad round"""
    logs, quads = pool
    os.environ["PM_DECIDE_BATCH_CHUNK"] = str(chunk)
    try:
        got = _run(gpu_ctx, pairing, quads[:B])
    finally:
        del os.environ["PM_DECIDE_BATCH_CHUNK"]
    ok, pair = D.expect(logs[:B], D.SEED)
    assert got["ok"] == ok and np.array_equal(got["pair"], pair) and not got["status"].any()


def _seed_with(pred):
    for s in range(256):
        seed = bytes([s]) * 32
        if pred(seed):
            return seed
    raise AssertionError("no seed among 256 has the property")


def _equal_digit_window(seed):
    a, b = BR.digits(BR.coef(seed, 0)), BR.digits(BR.coef(seed, 1))
    return any(x == y != 0 for x, y in zip(a, b))


def test_adversarial_sums(gpu_ctx, pairing):
    r = D.R
    a, b, c = 424243, 777, 999
    seed = _seed_with(_equal_digit_window)  # a window in which items 0 and 1 take the same table entry
    r0, r1 = BR.coef(seed, 0), BR.coef(seed, 1)
    inv = pow(r1, -1, r)
    cases = {
        # r_0 w_0 = -r_1 w_1: L is the identity at the end of the Horner tail
        "sum_cancels": [(a, b, c, 5), ((-r0 * a * inv) % r, b, c, 6)],
        # w_1 = -w_0: in the window with equal digits the tree adds P and -P
        "tree_hits_identity": [(a, b, c, 5), (-a, b, c, 6)],
        # w_1 = w_0 (and equal C): in that window the tree's addition is a doubling
        "tree_doubles": [(a, b, c, 5), (a, b, c, 5)],
        # r_0 w_0 = r_1 w_1: the two terms of L are one point
        "terms_equal": [(a, b, c, 5), ((r0 * a * inv) % r, b, c, 6)],
        "every_w_identity": [(None, b + i, c, 5) for i in range(5)],
        "every_c_identity": [(a + i, b + i, c, -(b + i) - c) for i in range(5)],
        "everything_identity": [(None, None, None, None)] * 3,
    }
    for name, logs in cases.items():
        q = D.quads_from_logs(logs)
        got = _run(gpu_ctx, pairing, q, seed=seed)
        ok, pair = D.expect(logs, seed)
        assert np.array_equal(got["pair"], pair), name
        assert got["ok"] == ok and not got["status"].any(), name
        host = H.accum_decide_batch_host(pairing, q, seed=seed)
        assert host["ok"] == ok and np.array_equal(host["pair"], pair), name
    assert not _run(gpu_ctx, pairing, D.quads_from_logs(cases["sum_cancels"]), seed=seed)["pair"][0].any()
    assert D.expect(cases["everything_identity"], seed)[0] == 1
    assert D.expect(cases["every_w_identity"], seed)[0] == 0


def test_crafted_pair_on_the_device(gpu_ctx, pairing):
    logs = D.crafted_pair(5, 1, 3, D.SEED)
    q = D.quads_from_logs(logs)
    assert _run(gpu_ctx, pairing, q, seed=D.SEED)["ok"] == 1
    got = _run(gpu_ctx, pairing, q, seed=D.SEED2)
    assert got["ok"] == 0 and np.array_equal(got["pair"], D.expect(logs, D.SEED2)[1])


def test_off_curve_item_among_accepting_ones(gpu_ctx, pairing, pool):
    logs, quads = pool
    B, bad = 9, 4
    q = quads[:B].copy()
    q[bad, 2, 4] ^= np.uint64(2)  # y of f: no longer on the curve
    got = _run(gpu_ctx, pairing, q)
    assert got["ok"] == 0 and got["status"].tolist() == [8 if i == bad else 0 for i in range(B)]
    ok, pair = D.expect(logs[:B], D.SEED, skipped=(bad,))
    assert ok == 0 and np.array_equal(got["pair"], pair)  # L and R are the sums without the item
    host = H.accum_decide_batch_host(pairing, q, seed=D.SEED)
    assert host["ok"] == 0 and np.array_equal(host["pair"], pair) and np.array_equal(host["status"], got["status"])


def test_locate(gpu_ctx, pairing, pool):
    logs, quads = pool
    B, bad = 64, [0, 31, 63]
    q = D.quads_from_logs(D.with_bad(logs[:B], bad))
    got = _run(gpu_ctx, pairing, q, locate=True)
    assert got["ok"] == 0
    d_q, d_ok = _dev(gpu_ctx, q), _out(gpu_ctx, B)
    torch.cuda.synchronize()
    gpu_ctx.accum_decide_device(pairing, B, d_q.data_ptr(), d_ok.data_ptr())
    per_proof = d_ok.cpu().numpy().view(np.uint32)[:B]
    assert np.array_equal(got["item_ok"], per_proof)
    assert per_proof.tolist() == [0 if i in bad else 1 for i in range(B)]
    # an accepted batch: all ones; without the flag, or without the buffer, nothing is written
    got = _run(gpu_ctx, pairing, quads[:B], locate=True)
    assert got["ok"] == 1 and (got["item_ok"] == 1).all()
    assert (_run(gpu_ctx, pairing, q, locate=False)["item_ok"] == SENT32).all()
    assert _run(gpu_ctx, pairing, q, locate=True, with_item=False)["ok"] == 0


def test_host_pointer_form(gpu_ctx, pairing, pool):
    logs, quads = pool
    q, si, _, item_st = D.family_batch(17)
    dev = _run(gpu_ctx, pairing, q, si)
    got = gpu_ctx.accum_decide_batch(pairing, q, si, seed=D.SEED, locate=True)
    assert got["ok"] == dev["ok"] == 0 and np.array_equal(got["pair"], dev["pair"])
    assert np.array_equal(got["status"], dev["status"]) and got["seed"] == D.SEED
    per_ok, _ = H.accum_decide_host(pairing, q, si)
    assert np.array_equal(got["item_ok"], per_ok)
    got = gpu_ctx.accum_decide_batch(pairing, quads[:65])
    assert got["ok"] == 1 and len(got["seed"]) == 32 and "item_ok" not in got
    again = gpu_ctx.accum_decide_batch(pairing, quads[:65], seed=got["seed"])
    assert np.array_equal(again["pair"], got["pair"])


def test_null_seed_and_empty_batch(gpu_ctx, pairing, pool):
    _, quads = pool
    a = _run(gpu_ctx, pairing, quads[:5], seed=None)
    b = _run(gpu_ctx, pairing, quads[:5], seed=None)
    assert a["seed"] != b["seed"] and a["ok"] == b["ok"] == 1
    e = gpu_ctx.accum_decide_batch(pairing, np.zeros((0, 4, 8), dtype=np.uint64), seed=D.SEED)
    assert e["ok"] == 1 and not e["pair"].any()


def test_phases_appear_in_kernel_stats(gpu_ctx, pairing, pool):
    _, quads = pool
    gpu_ctx.set_timing(True)
    try:
        gpu_ctx.reset_stats()
        _run(gpu_ctx, pairing, quads[:65])
        stats = {n: gpu_ctx.kernel_stats(n) for n in ("decide_batch_prep", "decide_batch_sum")}
    finally:
        gpu_ctx.set_timing(False)
    for name, (calls, ms) in stats.items():
        assert calls == 1 and ms > 0, (name, calls, ms)


def test_end_to_end_from_proof_bytes(gpu_ctx, pairing):
    """the five honest simple-example proofs of tests/test_pairing_gpu.py through
    pm_verify_proofs_batch_device: accepted, the quads the oracle accumulator's; with one evaluation
    byte flipped the batch is rejected and PM_DECIDE_LOCATE names exactly that proof"""
    import accum as A
    import accum_util as AU
    import pasta as P
    import proof_bytes as PB
    import test_pairing_gpu as TP

    B = 5
    C, sh, proofs, vkr = TP._honest_proofs(B, U.TAU)
    ps = AU.to_product_shape(2, sh)
    ni = sh.num_instance_columns
    vk = np.array(A.to_limbs_mont(C.r, vkr), dtype=np.uint64)
    inst = np.array([[P.point_to_limbs(C, q) for q in pf.points[:ni]] for pf in proofs], dtype=np.uint64)
    datas = [PB.serialize(C, sh, pf) for pf in proofs]
    dev = torch.device("cuda", gpu_ctx.device)
    psize = H.proof_size(ps)

    def verify(datas, locate):
        buf = np.stack([np.frombuffer(d, dtype=np.uint8) for d in datas])
        d_pf = torch.from_numpy(buf.copy()).to(dev)
        d_in = _dev(gpu_ctx, inst)
        d_ch = torch.zeros((B, 7, 4), dtype=torch.int64, device=dev)
        d_q = torch.zeros((B, 4, 8), dtype=torch.int64, device=dev)
        d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
        d_it = _out(gpu_ctx, B)
        torch.cuda.synchronize()
        r = gpu_ctx.verify_proofs_batch_device(ps, pairing, B, vk, d_pf.data_ptr(), psize, d_in.data_ptr(),
                                               d_ch.data_ptr(), d_q.data_ptr(), d_st.data_ptr(), seed=D.SEED,
                                               d_item_ok=d_it.data_ptr(), locate=locate)
        it = d_it.cpu().numpy().view(np.uint32)
        assert (it[B:] == SENT32).all()
        return r, d_st.cpu().numpy().view(np.uint32), d_q.cpu().numpy().view(np.uint64), it[:B]

    r, st, quads, it = verify(datas, locate=False)
    assert r["ok"] == 1 and not st.any() and (it == SENT32).all()
    q0, _ = A.pack_result(C, A.accumulate_msm(C, sh, proofs[0]))
    assert np.array_equal(quads[0], q0)
    host = H.accum_decide_batch_host(pairing, quads, st, seed=D.SEED)
    assert host["ok"] == 1 and np.array_equal(host["pair"], r["pair"])

    items = PB.proof_items(sh)
    bad = [bytearray(d) for d in datas]
    j_eval = next(j for j, (k, _) in enumerate(items) if k == "sc")
    bad[2][32 * j_eval] ^= 0x01  # low byte of the first evaluation of proof 2
    assert int.from_bytes(bad[2][32 * j_eval:32 * j_eval + 32], "little") < C.r
    r, st, quads, it = verify([bytes(d) for d in bad], locate=True)
    assert r["ok"] == 0 and not st.any()
    assert it.tolist() == [1, 1, 0, 1, 1]

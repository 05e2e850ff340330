"""CPU: pm_accum_decide_batch_host, the host form of the batch decider (the
parity form of the device path and the CPU baseline), against
tests/decide_batch_ref.py: ok, every status word, L and R limb for limb, and
out_seed."""
import decide_batch_ref as BR
import decide_batch_util as D
import halo2_amd as H
import numpy as np
import pairing_ref as PR
import pairing_util as U
import pytest


@pytest.fixture(scope="module")
def pairing():
    return H.Pairing(None, U.g2_words(PR.G2), U.g2_words(U.s_g2()))


@pytest.mark.parametrize("B", [0, 1, 2, 3, 17])
def test_families_against_reference(pairing, B):
    """the families of pairing_util.family: identity w, identity sum, doubling in the sum,
    off-curve, status_in.  The sums are compared with the reference's; the decision with the
    reference's where it needs no pairing (a status is set), else with the per-item decisions:
    a batch of valid and invalid items is rejected, one of valid items accepted."""
    q, si, item_ok, item_st = D.family_batch(B)
    got = H.accum_decide_batch_host(pairing, q, si, seed=D.SEED)
    status, L, R = BR.fold(q, si, D.SEED)
    assert got["status"].tolist() == status == item_st.tolist()
    assert np.array_equal(got["pair"], D.pair_words(L, R))
    assert got["seed"] == D.SEED
    assert got["ok"] == (1 if item_ok.all() else 0)  # B = 0 and B = 1 (one accepting item): accepted


def test_accepting_subset_against_reference_pairing(pairing):
    fam = [f for f in U.family() if f[3] == 1 and f[2] == 0]
    q = np.stack([f[1] for f in fam])
    got = H.accum_decide_batch_host(pairing, q, seed=D.SEED)
    ok, status, L, R = BR.decide(q, None, D.SEED, U.s_g2())
    assert got["ok"] == ok == 1 and got["status"].tolist() == status
    assert np.array_equal(got["pair"], D.pair_words(L, R))


@pytest.mark.parametrize("pos", [0, 2, 4])
def test_one_bad_item_from_logs(pairing, pos):
    logs = D.with_bad(D.accepting(5), [pos])
    got = H.accum_decide_batch_host(pairing, D.quads_from_logs(logs), seed=D.SEED, locate=True)
    ok, pair = D.expect(logs, D.SEED)
    assert got["ok"] == ok == 0 and np.array_equal(got["pair"], pair)
    assert got["item_ok"].tolist() == [0 if i == pos else 1 for i in range(5)]


def test_crafted_pair(pairing):
    logs = D.crafted_pair(5, 1, 3, D.SEED)
    q = D.quads_from_logs(logs)
    a = H.accum_decide_batch_host(pairing, q, seed=D.SEED)
    b = H.accum_decide_batch_host(pairing, q, seed=D.SEED2)
    assert a["ok"] == 1 and b["ok"] == 0
    assert np.array_equal(a["pair"], D.expect(logs, D.SEED)[1])
    assert np.array_equal(b["pair"], D.expect(logs, D.SEED2)[1])


def test_pool_batch_with_equal_points(pairing):
    """65 items over 16 types: equal points meet in the buckets (the doubling branch)"""
    logs = D.accepting(65)
    got = H.accum_decide_batch_host(pairing, D.quads_from_logs(logs), seed=D.SEED, locate=True)
    ok, pair = D.expect(logs, D.SEED)
    assert got["ok"] == ok == 1 and np.array_equal(got["pair"], pair) and got["item_ok"].all()


def test_null_seed_draws_a_fresh_one(pairing):
    q = D.quads_from_logs(D.accepting(3))
    a = H.accum_decide_batch_host(pairing, q)
    b = H.accum_decide_batch_host(pairing, q)
    assert a["seed"] != b["seed"] and len(a["seed"]) == 32
    assert a["ok"] == 1 and b["ok"] == 1
    # the reported seed reproduces the result
    c = H.accum_decide_batch_host(pairing, q, seed=a["seed"])
    assert np.array_equal(c["pair"], a["pair"]) and c["ok"] == 1

"""CPU: tests/decide_batch_ref.py, the batch decider's definition on Python
integers, against itself: the coefficients against hashlib and pinned values,
the recoding, completeness, rejection with one bad item at each position, and
the crafted pair that documents why the seed must be fresh."""
import hashlib

import decide_batch_ref as BR
import decide_batch_util as D
import pairing_util as U
import pytest


def test_coefficients_against_hashlib():
    seed = D.SEED
    for i in (0, 1, 7, 2**32 + 5, 2**64 - 1):
        h = hashlib.blake2b(digest_size=64, person=b"pm-batch-decide" + b"\0")
        h.update(seed)
        h.update(i.to_bytes(8, "little"))
        assert BR.coef(seed, i) == int.from_bytes(h.digest()[:16], "little")
    # pinned: the personalisation, the input layout and the byte order
    assert BR.coef(seed, 0) == 0x8C0AFA9D4FCC8A90A5EDAA4407BEE311
    assert BR.coef(seed, 7) == 0x7F20C890BCA58AE45A221EEF282D2C2D
    assert BR.coef(D.SEED2, 0) != BR.coef(seed, 0)


def test_recoding():
    for r in (0, 1, 7, 8, 15, 16, 2**128 - 1, 2**127, 0x88888888888888888888888888888888,
              0x77777777777777777777777777777777, BR.coef(D.SEED, 3)):
        d = BR.digits(r)
        assert len(d) == 33 and all(-8 <= x <= 7 for x in d) and d[32] in (0, 1)
    assert BR.digits(2**128 - 1) == [-1] + [0] * 31 + [1]


def test_completeness_and_sums_from_logs():
    logs = D.accepting(5)
    ok, status, L, R = BR.decide(D.quads_from_logs(logs), None, D.SEED, U.s_g2())
    want_ok, want_pair = D.expect(logs, D.SEED)
    assert ok == 1 == want_ok and status == [0] * 5
    assert (D.pair_words(L, R) == want_pair).all()


@pytest.mark.parametrize("pos", range(5))
def test_one_bad_item_rejects(pos):
    logs = D.with_bad(D.accepting(5), [pos])
    ok, status, L, R = BR.decide(D.quads_from_logs(logs), None, D.SEED, U.s_g2())
    want_ok, want_pair = D.expect(logs, D.SEED)
    assert ok == 0 == want_ok and status == [0] * 5
    assert (D.pair_words(L, R) == want_pair).all()


def test_status_and_identity_items():
    fam = {f[0]: f for f in U.family()}
    names = ["accept", "off_curve", "status_in", "all_inf", "w_inf_sum_inf"]
    quads = [fam[n][1] for n in names]
    status_in = [fam[n][2] for n in names]
    status, L, R = BR.fold(quads, status_in, D.SEED)
    assert status == [0, 8, 0x13, 0, 0]
    # only "accept" contributes: the others have a status or identity bases
    st0, w, c = BR.item(quads[0])
    import pairing_ref as PR

    assert L == PR.g1_mul(BR.coef(D.SEED, 0), w) and R == PR.g1_mul(BR.coef(D.SEED, 0), c)
    # empty sums: accepted without a pairing's help (the product of nothing is 1)
    assert BR.decide([fam["all_inf"][1]], None, D.SEED, U.s_g2())[0] == 1


def test_crafted_pair_cancels_under_its_seed_only():
    """Items 1 and 3 are both invalid, the deviation of 3 being -r_1/r_3 times that of 1 under SEED:
    the batch is accepted under SEED and rejected under another seed.  This pins where r_i enters,
    and is why the seed must be fixed after the proofs and unknown to whoever made them."""
    logs = D.crafted_pair(5, 1, 3, D.SEED)
    assert D.deviation(logs[1]) != 0 and D.deviation(logs[3]) != 0
    q = D.quads_from_logs(logs)
    assert D.expect(logs, D.SEED)[0] == 1 and D.expect(logs, D.SEED2)[0] == 0
    assert BR.decide(q, None, D.SEED, U.s_g2())[0] == 1
    assert BR.decide(q, None, D.SEED2, U.s_g2())[0] == 0

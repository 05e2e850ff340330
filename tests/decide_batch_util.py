"""Batches for the batch decider's tests, built from known discrete logs (as
tests/pairing_util.py): an item is four logs (a, b, c, d) (None = identity), the
quad is ([a]G, [b]G, [c]G, [d]G), and everything expected is stated from the
logs, not computed by the code under test:

    L = [sum r_i a_i]G,   R = [-sum r_i (b_i + c_i + d_i)]G,
    ok  iff  every status is 0  and  sum r_i (a_i tau - b_i - c_i - d_i) = 0 mod r.

Large batches draw their points from a pool of at most 64 points (16 accepting
item types), so the Python set-up stays within seconds and equal points meet
each other in the sums."""
import decide_batch_ref as BR
import numpy as np
import pairing_util as U

R = U.C.r
TAU = U.TAU
SEED = bytes(range(32))
SEED2 = bytes(range(1, 33))

_W = {}


def words_of(k):
    """the ABI's 8 words of [k]G, cached (None or 0: the identity)"""
    k = 0 if k is None else k % R
    if k not in _W:
        _W[k] = U.words(U.pt(k))
    return _W[k]


def quads_from_logs(logs):
    return np.array([[words_of(k) for k in it] for it in logs], dtype=np.uint64).reshape(-1, 4, 8)


def lg(k):
    return 0 if k is None else k % R


def deviation(it, tau=TAU):
    a, b, c, d = (lg(k) for k in it)
    return (a * tau - b - c - d) % R


def expect(logs, seed, tau=TAU, skipped=()):
    """-> (ok, pair (2, 8) u64): skipped = indices of items with a non-zero status"""
    sa = sb = dev = 0
    for i, it in enumerate(logs):
        if i in skipped:
            continue
        r = BR.coef(seed, i)
        sa += r * lg(it[0])
        sb += r * (lg(it[1]) + lg(it[2]) + lg(it[3]))
        dev += r * deviation(it, tau)
    ok = 1 if (not skipped and dev % R == 0) else 0
    pair = np.array([U.words(U.pt(sa)), U.words(U.pt(-sb))], dtype=np.uint64)
    return ok, pair


def item_type(k, tau=TAU):
    """accepting item of type k: four pool points"""
    a, b, c = 1000003 + 17 * k, 2000003 + 29 * k, 3000017 + 31 * k
    return (a, b, c, U.solve_d(a, b, c, tau))


def accepting(B, tau=TAU, types=16):
    return [item_type(i % types, tau) for i in range(B)]


def with_bad(logs, at):
    """the items at `at` rejected: d + 1"""
    out = list(logs)
    for i in at:
        a, b, c, d = out[i]
        out[i] = (a, b, c, d + 1)
    return out


def crafted_pair(B, i, j, seed, tau=TAU):
    """all accepting but items i and j, whose deviations cancel under `seed`:
    dev_j = -(r_i / r_j) dev_i.  Accepted under `seed`, rejected under any other."""
    logs = accepting(B, tau)
    ri, rj = BR.coef(seed, i), BR.coef(seed, j)
    a, b, c, d = logs[i]
    logs[i] = (a, b, c, d - 12345)  # deviation +12345
    dj = (-ri * pow(rj, -1, R) * 12345) % R
    a, b, c, d = logs[j]
    logs[j] = (a, b, c, d - dj)
    return logs


def family_batch(B, tau=TAU):
    """B items cycling through pairing_util.family (identity w, identity sum, doubling in the
    sum, off-curve, status_in, ...) -> (quads, status_in, per-item ok, per-item status)"""
    fam = U.family(tau, 1) + U.family(tau, 2)
    pick = [fam[i % len(fam)] for i in range(B)]
    if B == 0:
        return (np.zeros((0, 4, 8), dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32),
                np.zeros(0, dtype=np.uint32))
    return (np.stack([p[1] for p in pick]), np.array([p[2] for p in pick], dtype=np.uint32),
            np.array([p[3] for p in pick], dtype=np.uint32), np.array([p[4] for p in pick], dtype=np.uint32))


def pair_words(L, Rp):
    import pairing_ref as PR

    return np.array([PR.g1_words(L), PR.g1_words(Rp)], dtype=np.uint64)

"""Items for the pairing decider's tests, built from known discrete logs: an
accumulator quad (w, zw, f, e) = ([a]G, [b]G, [c]G, [d]G) is accepted against
s_g2 = [tau]G2 iff a tau = b + c + d mod r.  Points come from oracle/pasta.py's
BN254; the expected decision of every family is stated here, not computed by
the code under test."""
import numpy as np
import pairing_ref as PR
import pasta as P

C = P.BN254
TAU = 0x1234567890ABCDEF1234567890ABCDEF
TAU2 = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0


def pt(k):
    """[k]G as oracle/pasta.py's point (None for the identity)"""
    k %= C.r
    return None if k == 0 else C.mul(k, C.gen)


def words(Pt):
    return [0] * 8 if Pt is None else [int(v) for v in P.point_to_limbs(C, Pt)]


def quad_words(w, zw, f, e):
    return np.array([words(w), words(zw), words(f), words(e)], dtype=np.uint64)


def solve_d(a, b, c, tau=TAU):
    return (a * tau - b - c) % C.r


def family(tau=TAU, seed=1):
    """[(name, quad (4, 8) u64, status_in, expect_ok, expect_status)]: the constructed families."""
    a, b, c = 55555 + seed, 777 + 3 * seed, 999 + 7 * seed
    d = solve_d(a, b, c, tau)
    items = []

    def add(name, q, ok, status_in=0, status=None):
        items.append((name, quad_words(*q), status_in, ok, status_in if status is None else status))

    add("accept", (pt(a), pt(b), pt(c), pt(d)), 1)
    add("reject_d_plus_1", (pt(a), pt(b), pt(c), pt(d + 1)), 0)
    add("w_inf_sum_inf", (None, pt(b), pt(c), pt(-b - c)), 1)
    add("w_inf_sum_not_inf", (None, pt(b), pt(c), pt(d)), 0)
    # zw = -f: the intermediate sum is the identity; then e alone must be [a tau]G
    add("zw_eq_neg_f_accept", (pt(a), pt(b), pt(-b), pt(a * tau)), 1)
    add("zw_eq_neg_f_reject", (pt(a), pt(b), pt(-b), pt(a * tau + 1)), 0)
    # zw = f: the first addition is a doubling
    add("zw_eq_f_accept", (pt(a), pt(b), pt(b), pt(a * tau - 2 * b)), 1)
    add("zw_eq_f_reject", (pt(a), pt(b), pt(b), pt(a * tau - 2 * b + 5)), 0)
    # zw + f = -e: the final sum is the identity while w is not
    add("sum_inf_w_not_inf", (pt(a), pt(b), pt(c), pt(-b - c)), 0)
    # zw + f = e: the second addition is a doubling
    b2 = (a * tau * pow(2, -1, C.r) - c) % C.r  # 2 (b2 + c) = a tau
    add("second_add_doubles_accept", (pt(a), pt(b2), pt(c), pt(b2 + c)), 1)
    add("second_add_doubles_reject", (pt(a), pt(b), pt(c), pt(b + c)), 0)
    add("all_inf", (None, None, None, None), 1)
    off = quad_words(pt(a), pt(b), pt(c), pt(d))
    off[2, 4] ^= np.uint64(2)  # y of f: no longer on the curve
    items.append(("off_curve", off, 0, 0, 8))
    add("status_in", (pt(a), pt(b), pt(c), pt(d)), 0, status_in=0x13)
    return items


def batch(B, tau=TAU):
    """B items cycling through the families with accepting and rejecting ones alternating
    -> (quads (B, 4, 8), status_in (B,), ok (B,), status (B,))."""
    fam = family(tau, 1) + family(tau, 2)
    acc = [f for f in fam if f[3] == 1]
    rej = [f for f in fam if f[3] == 0]
    pick = [(acc if i % 2 == 0 else rej)[(i // 2) % len(acc if i % 2 == 0 else rej)] for i in range(B)]
    return (np.stack([p[1] for p in pick]), np.array([p[2] for p in pick], dtype=np.uint32),
            np.array([p[3] for p in pick], dtype=np.uint32), np.array([p[4] for p in pick], dtype=np.uint32))


WALK_REJECT_EVERY = 3    # items i = 2 mod 3 carry the next item's e
WALK_STATUS_EVERY = 97   # items i = 96 mod 97 carry a non-zero status_in
WALK_OFF_CURVE = 4       # this item's zw is not on the curve


def walk(B, tau=TAU, a0=70001, b0=8101, c0=9203):
    """B distinct items from walks, no scalar multiplication per item:
    a_i = a0 + i, b_i = b0 + i, c_i = c0 + i, d_i = a_i tau - b_i - c_i, so w, zw and f advance
    by G and e by [tau - 2]G, one affine addition each.  Item i is accepted unless
      i = 2 mod 3: it carries d_(i+1) in place of d_i (off by tau - 2 != 0),
      i = 96 mod 97: status_in is non-zero (passed through, nothing evaluated),
      i = WALK_OFF_CURVE: the y of zw has a bit flipped (PM_DECIDE_NOT_ON_CURVE = 8).
    -> (quads (B, 4, 8), status_in (B,), ok (B,), status (B,)), stated from this construction."""
    assert (tau - 2) % C.r and B < WALK_STATUS_EVERY * 255
    step_e = pt(tau - 2)
    w, zw, f, e = pt(a0), pt(b0), pt(c0), pt(solve_d(a0, b0, c0, tau))
    q = np.zeros((B, 4, 8), dtype=np.uint64)
    si = np.zeros(B, dtype=np.uint32)
    ok = np.ones(B, dtype=np.uint32)
    for i in range(B):
        e_next = C.add(e, step_e)
        reject = i % WALK_REJECT_EVERY == WALK_REJECT_EVERY - 1
        q[i] = [words(w), words(zw), words(f), words(e_next if reject else e)]
        if reject:
            ok[i] = 0
        if i % WALK_STATUS_EVERY == WALK_STATUS_EVERY - 1:
            si[i], ok[i] = 0x10 + i // WALK_STATUS_EVERY, 0
        w, zw, f, e = C.add(w, C.gen), C.add(zw, C.gen), C.add(f, C.gen), e_next
    st = si.copy()
    if B > WALK_OFF_CURVE:
        assert ok[WALK_OFF_CURVE] == 1   # it would have been accepted
        q[WALK_OFF_CURVE, 1, 4] ^= np.uint64(2)
        ok[WALK_OFF_CURVE], st[WALK_OFF_CURVE] = 0, 8
    return q, si, ok, st


def g2_words(Q):
    return np.array(PR.g2_words(Q), dtype=np.uint64)


_S = {}


def s_g2(tau=TAU):
    if tau not in _S:
        _S[tau] = PR.g2_mul(tau, PR.G2)
    return _S[tau]


def ref_point(ws):
    """8 words -> pairing_ref's affine point (None for the identity)"""
    if not any(int(v) for v in ws):
        return None
    return (PR.words_fp(ws[:4]), PR.words_fp(ws[4:]))


def ref_gt_words(quad, tau=TAU):
    """pairing_ref's value for a quad, as the ABI's (12, 4) words"""
    w, zw, f, e = (ref_point(quad[i]) for i in range(4))
    return np.array(PR.gt_words(PR.accum_gt(w, zw, f, e, s_g2(tau))), dtype=np.uint64).reshape(12, 4)

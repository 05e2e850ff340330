"""The batch decider's definition on Python integers: one pairing
check for B accumulator quads by a random linear combination,

    L = sum r_i w_i,   R = sum r_i C_i,   C_i = -(zw_i + f_i + e_i),
    ok = [ every status is 0  and  e(L, s_g2) e(R, g2) == 1 ].

The tests pin pm_accum_decide_batch* by this file.  Points are
tests/pairing_ref.py's affine pairs (None = identity); quads are the ABI's
words."""
import hashlib
import struct

import pairing_ref as PR

PERSONAL = b"pm-batch-decide"  # hashlib pads it with zeros to 16 bytes
NOT_ON_CURVE = 8  # PM_DECIDE_NOT_ON_CURVE


def coef(seed, i):
    """r_i: the first 16 bytes, little-endian, of BLAKE2b-512(seed[32] || le64(i)); used as it comes."""
    assert len(seed) == 32
    h = hashlib.blake2b(bytes(seed) + struct.pack("<Q", i), digest_size=64, person=PERSONAL)
    return int.from_bytes(h.digest()[:16], "little")


def digits(r):
    """33 signed 4-bit digits in [-8, 7], sum d_w 16^w = r (the implementation's recoding)"""
    out, carry = [], 0
    for w in range(33):
        v = ((r >> (4 * w)) & 15) + carry
        carry = 1 if v >= 8 else 0
        out.append(v - 16 * carry)
    assert carry == 0 and sum(d << (4 * w) for w, d in enumerate(out)) == r
    return out


def point(ws):
    """8 words -> affine point, None for (0, 0); other words are taken mod p"""
    if not any(int(v) for v in ws):
        return None
    return (PR.words_fp(ws[:4]), PR.words_fp(ws[4:]))


def item(quad, status_in=0):
    """-> (status, w, C): a non-zero status_in passes through; an off-curve point gives
    NOT_ON_CURVE; with a non-zero status the item contributes nothing (w = C = None)."""
    if status_in:
        return status_in, None, None
    pts = [point(quad[k]) for k in range(4)]
    if not all(PR.g1_on_curve(p) for p in pts):
        return NOT_ON_CURVE, None, None
    return 0, pts[0], PR.g1_neg(PR.g1_add(PR.g1_add(pts[1], pts[2]), pts[3]))


def fold(quads, status_in, seed):
    """-> (status list, L, R) over the items with status 0"""
    L = R = None
    status = []
    for i, q in enumerate(quads):
        st, w, c = item(q, int(status_in[i]) if status_in is not None else 0)
        status.append(st)
        if st:
            continue
        r = coef(seed, i)
        L = PR.g1_add(L, PR.g1_mul(r, w))
        R = PR.g1_add(R, PR.g1_mul(r, c))
    return status, L, R


def decide(quads, status_in, seed, s_g2, g2=PR.G2):
    """-> (ok, status list, L, R); L = R = identity gives 1 (the empty product)"""
    status, L, R = fold(quads, status_in, seed)
    if any(status):
        return 0, status, L, R
    ok = 1 if PR.decide_gt(L, R, s_g2, g2) == PR.F12_ONE else 0
    return ok, status, L, R

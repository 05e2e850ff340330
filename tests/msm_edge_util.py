"""Adversarial MSM inputs with known answers (tests only, host only).

Builds on the synthetic inputs (msm_ref.synth_scalars / synth_bases: base i is
[a_i]G with a_i the synthetic scalar of seed SEED_BASES) and produces

    S      (n, 4) u64 scalars in MONTGOMERY form (canonical() converts),
    B      (n, 8) u64 affine Montgomery bases, (0, 0) = identity,
    dlogs  (n, 4) u64: the discrete log of base i, in Montgomery form like
           the output of msm_ref.synth_scalars (0 for an identity base),

so that sum_i s_i B_i = [sum_i s_i dlog_i] G (expected_by_dlog) whatever the
scalars are.  The special scalars are built in canonical form, always < r:

    constants   0, 1, r - 1, r - 2, (r - 1) / 2, (r + 1) / 2
    patterns    for a window width c (WinGeom of msm_kernels.hpp: W =
                ceil(256 / c) windows, width 256 / W + (w < 256 % W), offset
                w (256 / W) + min(w, 256 % W)) every window's raw digit is
                  half    2^(c_w - 1)      largest positive digit, no carry
                  half+1  2^(c_w - 1) + 1  smallest that goes negative, carries
                  half-1  2^(c_w - 1) - 1
                  ones    2^(c_w) - 1      the carry ripples through every
                                           window: each later one is code 0
                  alt     half / half+1 alternating by window
    row patterns  the same four digit values confined to the windows of one
                row of a row table (windows j W / rows .. (j + 1) W / rows - 1)
                over a random scalar; the window just below the row is set so
                that no carry enters (half, half-1) or one does (half+1, ones),
                and the carrying kinds pass theirs on to the row above
A pattern that is not < r loses top bits (never a reduction mod r): the low
windows keep their digits.

The base transforms (duplicate, negate, identity) and the special scalars are
planted into otherwise random inputs at rows 0 and n - 1 and on both sides of
every sort-block and scalar-part boundary of the pipeline (boundaries()), in
small gadgets: P P (equal pairs), P -P, P P -P, O with a special scalar beside
a zero scalar, and two special scalars on ordinary bases; groups of 2, 3, 64,
65 and 4097 equal (scalar, base) pairs land P + P in one bucket of every
window.  mixed_case() returns such an input with the list of what it planted.
"""
from __future__ import annotations

import numpy as np

import msm_ref
import pasta as P

M64 = (1 << 64) - 1
SORT_THREADS = 1024       # msm_plan.hpp kSortThreads
SORT_PER_THREAD = 8       # kSortPerThread
SORT_B = SORT_THREADS * SORT_PER_THREAD   # kSortB: fixed-base padding, part rounding
SPLIT_COPY_MIN_N = 1 << 18    # PM_SPLIT_COPY_MIN_N
SPLIT_COPY3_MIN_N = 1 << 21   # kSplitCopy3MinN
GROUPS = (2, 3, 64, 65, 4097)
PATTERN_KINDS = ("half", "half+1", "half-1", "ones")
CONSTANTS = ("zero", "one", "r-1", "r-2", "(r-1)/2", "(r+1)/2")


# ------------------------------------------------------------ limbs <-> ints
def to_ints(L):
    """(n, 4) u64 -> object array of Python ints."""
    L = np.asarray(L, dtype=np.uint64).reshape(-1, 4).astype(object)
    return L[:, 0] + (L[:, 1] << 64) + (L[:, 2] << 128) + (L[:, 3] << 192)


def to_limbs(vals):
    """iterable of ints -> (n, 4) u64."""
    v = np.asarray(list(vals), dtype=object).reshape(-1)
    out = np.empty((v.shape[0], 4), dtype=np.uint64)
    for k in range(4):
        out[:, k] = ((v >> (64 * k)) & M64).astype(np.uint64)
    return out


def montgomery(curve, S):
    """canonical (n, 4) -> Montgomery (n, 4)."""
    r = P.CURVES[curve].r
    return to_limbs(to_ints(S) * P.R_MONT % r)


def canonical(curve, S):
    """Montgomery (n, 4) -> canonical (n, 4)."""
    r = P.CURVES[curve].r
    return to_limbs(to_ints(S) * pow(P.R_MONT, -1, r) % r)


def expected_by_dlog(curve, S, dlogs, canonical=False):
    """[sum_i s_i dlog_i] G as an oracle point (None = identity): S (n, 4)
    Montgomery scalars (canonical with canonical=True), dlogs (n, 4)
    Montgomery.  known_dlog_point for arbitrary scalar and dlog lists."""
    C = P.CURVES[curve]
    S = np.asarray(S, dtype=np.uint64).reshape(-1, 4)
    D = np.asarray(dlogs, dtype=np.uint64).reshape(-1, 4)
    assert S.shape == D.shape
    tot = 0
    for k in range(0, S.shape[0], 1 << 16):
        tot += int(np.dot(to_ints(S[k:k + (1 << 16)]), to_ints(D[k:k + (1 << 16)])))
    rinv = pow(P.R_MONT, -1, C.r)
    tot = tot * rinv % C.r
    if not canonical:
        tot = tot * rinv % C.r
    return C.mul(tot, C.gen)


# --------------------------------------------------------------- window math
def win_geom(c):
    """(W, widths, offsets) of WinGeom<W> with W = ceil(256 / c)."""
    W = (256 + c - 1) // c
    base, extra = 256 // W, 256 % W
    widths = [base + (1 if w < extra else 0) for w in range(W)]
    offsets = [w * base + min(w, extra) for w in range(W)]
    return W, widths, offsets


def signed_digits(s, c, drop_carry_at=None):
    """signed_digit (msm_kernels.hpp) of canonical s over every window ->
    (digits, carries): digits[w] in [-2^(c_w - 1) + 1, 2^(c_w - 1)], carries[w]
    the carry OUT of window w.  drop_carry_at = w forgets the carry out of
    window w (a deliberately wrong recomputation, for the sensitivity tests)."""
    W, widths, offsets = win_geom(c)
    digits, carries, carry = [], [], 0
    for w in range(W):
        cw = widths[w]
        d = ((s >> offsets[w]) & ((1 << cw) - 1)) + carry
        if w != W - 1 and d > (1 << (cw - 1)):
            d -= 1 << cw
            carry = 1
        else:
            carry = 0
        digits.append(d)
        carries.append(carry)
        if w == drop_carry_at:
            carry = 0
    return digits, carries


def from_digits(digits, c):
    _, _, offsets = win_geom(c)
    return sum(d << o for d, o in zip(digits, offsets))


def clear_top(s, r):
    """s with top bits cleared until it is < r -> (s, bits kept)."""
    k = 256
    while s >= r:
        k -= 1
        s &= (1 << k) - 1
    return s, k


def _digit_value(kind, cw):
    return {"half": 1 << (cw - 1), "half+1": (1 << (cw - 1)) + 1, "half-1": (1 << (cw - 1)) - 1,
            "ones": (1 << cw) - 1}[kind]


def pattern_scalar(curve, c, kind, windows=None, fill=0):
    """Canonical scalar whose raw digit in every window of `windows` (all by
    default) is the `kind` value (kind "alt": half in even windows, half+1 in
    odd ones), the other bits those of `fill`; top bits cleared until < r."""
    r = P.CURVES[curve].r
    W, widths, offsets = win_geom(c)
    s = fill
    for w in (range(W) if windows is None else windows):
        k = kind if kind != "alt" else ("half", "half+1")[w & 1]
        s &= ~(((1 << widths[w]) - 1) << offsets[w])
        s |= _digit_value(k, widths[w]) << offsets[w]
    s, _ = clear_top(s & ((1 << 256) - 1), r)
    assert s < r
    return s


def row_windows(c, rows, j):
    W = win_geom(c)[0]
    assert rows >= 1 and W % rows == 0
    return list(range(j * W // rows, (j + 1) * W // rows))


def row_pattern_scalar(curve, c, rows, j, kind, seed=0xED6E):
    """`kind` in the windows of row j over a random scalar; the window below
    the row holds raw digit 1 (no carry enters) for half / half-1 and all
    ones (a carry enters) for half+1 / ones."""
    C = P.CURVES[curve]
    W, widths, offsets = win_geom(c)
    wins = row_windows(c, rows, j)
    fill = P.synth_scalar(seed + 131 * j + PATTERN_KINDS.index(kind), c, C.r, C.scalar_bits)
    if wins[0] > 0:
        b = wins[0] - 1
        fill &= ~(((1 << widths[b]) - 1) << offsets[b])
        fill |= (1 if kind in ("half", "half-1") else (1 << widths[b]) - 1) << offsets[b]
    return pattern_scalar(curve, c, kind, wins, fill)


def constant_scalar(curve, name):
    r = P.CURVES[curve].r
    return {"zero": 0, "one": 1, "r-1": r - 1, "r-2": r - 2, "(r-1)/2": (r - 1) // 2, "(r+1)/2": (r + 1) // 2}[name]


def special_scalars(curve, c, rows=1):
    """[(name, canonical int)]: constants, whole-scalar digit patterns of
    width c, and (rows > 1) the patterns confined to each row's windows."""
    out = [("const:" + k, constant_scalar(curve, k)) for k in CONSTANTS]
    out += [("pattern:" + k, pattern_scalar(curve, c, k)) for k in PATTERN_KINDS + ("alt",)]
    if rows > 1:
        for j in range(rows):
            out += [(f"row{j}:{k}", row_pattern_scalar(curve, c, rows, j, k)) for k in PATTERN_KINDS]
    r = P.CURVES[curve].r
    assert all(0 <= s < r for _, s in out)
    return out


# ------------------------------------------------------- pipeline boundaries
def _rnd(v):
    return (v + SORT_B - 1) // SORT_B * SORT_B


def part_starts(n, split):
    """pstart[] of msm_plan.hpp msm_parts: one part, or (split: host scalars on a row
    table) 3/8 + 5/8 from 2^18 points, 1/4 + 3/8 + 3/8 from 2^21."""
    if not split or n < SPLIT_COPY_MIN_N:
        return [0, n]
    if n >= SPLIT_COPY3_MIN_N:
        return [0, _rnd(n // 4), _rnd(n * 5 // 8), n]
    return [0, _rnd(n * 3 // 8), n]


def sort_ppt(stride):
    """Points per sort thread of a digit row of `stride` points (msm_plan.hpp
    sort_plan: the largest power of two <= 8 that leaves >= 128 blocks)."""
    ppt = 1
    while ppt < SORT_PER_THREAD and stride >= 256 * ppt * SORT_THREADS:
        ppt *= 2
    return ppt


def sort_block(stride):
    """Points per histogram block of that row: ppt x 1024, halved when the
    row has 128 <= blocks < 256 (hsub in sort_plan)."""
    ppt = sort_ppt(stride)
    nblk = (stride + ppt * SORT_THREADS - 1) // (ppt * SORT_THREADS)
    hsub = 2 if ppt >= 2 and 128 <= nblk < 256 else 1
    return ppt * SORT_THREADS // hsub


def boundaries(n, table=False):
    """Sorted rows b (0 < b < n) such that rows b - 1 and b lie on the two
    sides of a sort block or of a scalar part, for the raw pipeline (digit
    rows of n points) or, table=True, a fixed / row table (rows padded to
    kSortB, one part or the split copy's parts)."""
    out = set()
    for split in ((False, True) if table else (False,)):
        ps = part_starts(n, split)
        for c0, c1 in zip(ps[:-1], ps[1:]):
            if not table:
                stride = n
            elif len(ps) == 2:
                stride = max(SORT_B, _rnd(n))
            else:
                stride = max(SORT_B, _rnd(c1 - c0))
            blk = sort_block(stride)
            out.update(range(c0, c1, blk))
    return sorted(b for b in out if 0 < b < n)


# ------------------------------------------------------------- base transforms
def dup_base(B, dlogs, i, k):
    B[k] = B[i]
    dlogs[k] = dlogs[i]


def neg_base(curve, B, dlogs, i, src=None):
    """Row i becomes -(row src) (src = i by default): y -> p - y, dlog -> r - dlog."""
    C = P.CURVES[curve]
    src = i if src is None else src
    B[i, :4] = B[src, :4]
    y = P.from_limbs(B[src, 4:])
    d = P.from_limbs(dlogs[src])
    assert y != 0 and d != 0
    B[i, 4:] = np.array(P.to_limbs(C.p - y), dtype=np.uint64)
    dlogs[i] = np.array(P.to_limbs(C.r - d), dtype=np.uint64)


def identity_base(B, dlogs, i):
    B[i] = 0
    dlogs[i] = 0


# ------------------------------------------------------------------ the cases
def synth(curve, n, seed=0, bases=None):
    """Synthetic (S Montgomery, B, dlogs Montgomery) of n points.  `bases`:
    the (n, 8) synthetic bases of seed SEED_BASES ^ seed when the caller has
    them already (the host generator costs a scalar multiplication per base)."""
    S = msm_ref.synth_scalars(curve, P.SEED_SCALARS ^ seed, 0, n)
    if bases is None:
        B = msm_ref.synth_bases(curve, P.SEED_BASES ^ seed, 0, n)
    else:
        B = np.array(bases, dtype=np.uint64).reshape(n, 8)
    D = msm_ref.synth_scalars(curve, P.SEED_BASES ^ seed, 0, n)
    return S, B, D


GADGETS = ("special", "dup", "neg", "ppn", "identity")


def mixed_case(curve, n, c, rows=1, table=False, seed=0, bases=None):
    """Random scalars and bases with every special scalar and base transform
    planted at the rows described in the module docstring -> (S, B, dlogs,
    planted): planted is a list of (kind, rows, scalar name) where kind is a
    gadget of GADGETS or "group<g>"."""
    C = P.CURVES[curve]
    S, B, D = synth(curve, n, seed, bases)
    specials = special_scalars(curve, c, rows)
    mont = to_limbs([s * P.R_MONT % C.r for _, s in specials])
    used = np.zeros(n, dtype=bool)
    planted = []
    anchors = set(boundaries(n, table))
    if n >= 8:
        anchors.update((1, n - 1))
    # evenly spaced anchors where the boundaries alone are too few to show
    # every gadget with every special scalar (small n)
    want = min(len(GADGETS) * len(specials), n // 8)
    if len(anchors) < want:
        step = max(6, n // want)
        for a in range(5, n - 5, step):
            if not any(x in anchors for x in range(a - 4, a + 5)):
                anchors.add(a)
    for k, b in enumerate(sorted(anchors)):
        name = specials[k % len(specials)][0]
        sm = mont[k % len(specials)]
        kind = GADGETS[k % len(GADGETS)]
        if b == 1:
            kind = "special"
        elif b == n - 1:
            kind = "dup"
        if kind == "ppn" and (b < 2 or used[b - 2]):
            kind = "neg"
        rws = [b - 2, b - 1, b] if kind == "ppn" else [b - 1, b]
        if used[rws].any():
            continue
        used[rws] = True
        if kind == "special":   # two special scalars on ordinary bases
            S[b - 1] = sm
            S[b] = mont[(k + 1) % len(specials)]
        elif kind == "dup":     # P, P with equal scalars: P + P in every window's bucket
            dup_base(B, D, b - 1, b)
            S[b - 1] = S[b] = sm
        elif kind == "neg":     # P, -P with equal scalars: P + (-P) = O
            neg_base(curve, B, D, b, b - 1)
            S[b - 1] = S[b] = sm
        elif kind == "ppn":     # P, P, -P
            dup_base(B, D, b - 2, b - 1)
            neg_base(curve, B, D, b, b - 2)
            S[b - 2] = S[b - 1] = S[b] = sm
        else:                   # O with a special scalar, a zero scalar beside it
            identity_base(B, D, b - 1)
            S[b - 1] = sm
            S[b] = 0
        planted.append((kind, rws, name))
    # groups of equal (scalar, base) pairs in contiguous free rows, spread over the input
    free = np.flatnonzero(~used)
    sizes = []
    for g in GROUPS:   # as many of the groups as fit into 3/4 of the free rows
        if sum(sizes) + g <= len(free) * 3 // 4:
            sizes.append(g)
    gap = (len(free) - sum(sizes)) // (len(sizes) + 1)
    pos = gap
    for g in sizes:
        rws = free[pos:pos + g]
        assert len(rws) == g
        pos += g + gap
        B[rws] = B[rws[0]]
        D[rws] = D[rws[0]]
        S[rws] = S[rws[0]]
        used[rws] = True
        planted.append((f"group{g}", [int(x) for x in rws], "random"))
    return S, B, D, planted


def whole_array_case(curve, n, name, c):
    """Every scalar equal to one special value (name as in special_scalars:
    "const:..." or "pattern:...") -> Montgomery (n, 4)."""
    C = P.CURVES[curve]
    s = dict(special_scalars(curve, c))[name]
    return np.repeat(to_limbs([s * P.R_MONT % C.r]), n, axis=0)


WHOLE_ARRAY = tuple("const:" + k for k in CONSTANTS) + tuple("pattern:" + k for k in PATTERN_KINDS + ("alt",))
# the whole-array cases a mixed input cannot stand for (every point skipped
# or negated in a window): the constants and the all-ones pattern
WHOLE_ARRAY_GPU = tuple("const:" + k for k in CONSTANTS) + ("pattern:ones",)

"""A family of proof shapes for the accumulator path (tests only, host only).

pm_accum_batch*, pm_transcript_batch*, pm_decode_proofs* and
pm_accum_batch_proofs* run a program compiled from the caller's
pm_proof_shape: the query list and rotation sets, the term slots, the
expression byte code, the Lagrange batch size, the LDS layout of k_acc_scalars,
the byte stream and squeeze offsets of k_transcript_s, the item offsets of
k_proof_decode.  This module varies the SHAPE (the other edge modules vary the
data of two shapes):

  DIRECTED     named shapes, each the smallest that shows one fact (a residue
               of the Lagrange denominator split, a structural branch, a bound)
  WIDE         shapes whose rows in k_acc_scalars leave 8..14, <= 3 and one
               proof per block (the last that fits); PAST_LDS, the first
               past the bound
  EDGES        shapes that put a squeeze of the transcript at a stream offset
               = 0, 1 or 127 (mod 128), found by a search under the real rules
  random_shapes  a seeded generator of legal shapes (redraws are counted)
  facts(sh)    what the device code will do with the shape, restated from the
               headers: nd % 3, log_n < 3 nkmax, np, nsets, J, T, Tp, the
               accumulator path per batch size, L_k mod 128, whether the
               streamed transcript plan fits its LDS

Points of synthetic proofs come from a small pool of [a]G with known a (one
scalar multiplication per pool entry and curve, not per point), so every
output is also [sum c_t a_t]G through accum_edge_util.term_plan.
"""
from __future__ import annotations

import functools
import os
import random
import re
import zlib

import numpy as np

import accum as A
import accum_edge_util as X
import accum_ref as R
import accum_util as U
import halo2_amd as H
import pasta as P
import proof_bytes as PB
import transcript as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "halo2-aggregation_amd", "csrc")
TWO_ADICITY = {0: 32, 1: 32, 2: 28}
POOL = 48
MAX_POINTS, MAX_EVALS = 40, 60      # bounds of the random generator


# ------------------------------------------------------------ header constants
@functools.lru_cache(maxsize=None)
def constants():
    """The constants facts() restates, parsed from the headers (a product of
    integers after "NAME ="), so a moved threshold fails the tests."""
    want = {"accum_engine.hpp": ("kAccScalarsLds",),
            "accum_kernels.hpp": ("kAccXVals",),
            "accum_plan.hpp": ("kAccStack", "kAccMaxSets", "kAccMaxPerSet", "kAccMaxBlind"),
            "transcript_kernels.hpp": ("kTrSlots", "kTrChallenges")}
    out = {}
    for fn, names in want.items():
        txt = open(os.path.join(CSRC, fn)).read()
        for nm in names:
            m = re.search(r"\b%s = ([0-9][0-9 *]*)[;,]" % nm, txt)
            v = 1
            for f in m.group(1).split("*"):
                v *= int(f)
            out[nm] = v
    return out


# ------------------------------------------------------------------- building
def build(cid, *, log_n=4, bf=1, ni=0, na=1, nf=0, nl=0, chunk=0, qd=2, inst_q=(), adv_q=((0, 0),), fixed_q=(),
          perm=(), gates=None, lk_in=None, lk_tab=None):
    """An oracle ProofShape on curve cid with VK points from the pool."""
    C = P.CURVES[cid]
    if gates is None:
        gates = [A.Advice(0)]
    if lk_in is None:
        lk_in = [A.Advice(0)] if nl else []
    if lk_tab is None:
        lk_tab = [A.Advice(0)] if nl else []
    sh = A.ProofShape(log_n=log_n, blinding_factors=bf, num_instance_columns=ni, num_advice_columns=na,
                      num_fixed_columns=nf, num_lookups=nl, perm_chunk_len=chunk, quotient_degree=qd,
                      instance_queries=list(inst_q), advice_queries=list(adv_q), fixed_queries=list(fixed_q),
                      perm_columns=list(perm), gates=list(gates), lookup_inputs=list(lk_in),
                      lookup_tables=list(lk_tab), omega=A.domain_omega(C.r, log_n), delta=A.field_delta(C.r))
    return with_vk(cid, sh)


@functools.lru_cache(maxsize=None)
def pool(cid):
    """(dlogs, points, limbs (POOL, 8) u64) of the curve's point pool."""
    C = P.CURVES[cid]
    dl = [P.synth_base_dlog(C, 0x5A9E, i) for i in range(POOL)]
    pts = [C.mul(d, C.gen) for d in dl]
    return dl, pts, np.array([P.point_to_limbs(C, q) for q in pts], dtype=np.uint64)


def with_vk(cid, sh):
    """VK commitments from the pool; their dlogs in sh.vk_dlogs."""
    dl, pts, _ = pool(cid)
    nf, npc = sh.num_fixed_columns, len(sh.perm_columns)
    fi = [(7 * i + 3) % POOL for i in range(nf)]
    si = [(5 * k + 11) % POOL for k in range(npc)]
    sh.fixed_commitments = [pts[i] for i in fi]
    sh.sigma_commitments = [pts[i] for i in si]
    sh.vk_dlogs = {("fixed", i): dl[j] for i, j in enumerate(fi)}
    sh.vk_dlogs.update({("sigma", k): dl[j] for k, j in enumerate(si)})
    return sh


def legal(cid, sh):
    """The reason the C ABI refuses the shape (acc_validate and the device's
    set bounds restated), or the empty string when it accepts it."""
    k = constants()
    nps = sh.n_perm_sets if (sh.perm_chunk_len or not sh.perm_columns) else -1
    if nps < 0:
        return "perm_chunk_len = 0 with permutation columns"
    if sh.quotient_degree < 1:
        return "quotient_degree"
    if sh.blinding_factors > k["kAccMaxBlind"]:
        return "blinding_factors"
    if not 1 <= sh.log_n <= TWO_ADICITY[cid] or (1 << sh.log_n) < sh.blinding_factors + 3:
        return "log_n"
    for qs, n in ((sh.instance_queries, sh.num_instance_columns), (sh.advice_queries, sh.num_advice_columns),
                  (sh.fixed_queries, sh.num_fixed_columns)):
        if any(not 0 <= c < n for c, _ in qs):
            return "query column"
    lim = {A.KIND_ADVICE: len(sh.advice_queries), A.KIND_FIXED: len(sh.fixed_queries),
           A.KIND_INSTANCE: len(sh.instance_queries)}
    if any(q >= lim[kind] for kind, q in sh.perm_columns):
        return "permutation column"
    if len(sh.gates) + nps + 5 * sh.num_lookups == 0:
        return "no expressions"
    if max([stack_depth(e) for e in sh.gates + sh.lookup_inputs + sh.lookup_tables] or [0]) > k["kAccStack"]:
        return "stack"
    sets = X._queries(sh)
    if len(sets) > k["kAccMaxSets"]:
        return "rotation sets"
    if max(len(qs) for _, qs in sets) > k["kAccMaxPerSet"]:
        return "set size"
    return ""


def stack_depth(e):
    """The postfix stack depth of compile_expressions' code for e."""
    op = e[0]
    if op in ("const", "fixed", "advice", "instance"):
        return 1
    if op in ("neg", "scaled"):
        return stack_depth(e[1])
    return max(stack_depth(e[1]), 1 + stack_depth(e[2]))


# ---------------------------------------------------------------------- facts
def squeeze_offsets(sh):
    """The stream length at each of the seven squeezes, after its 0x00 byte
    (33-byte VK / scalar records, 65-byte point records, transcript.py order)."""
    nl, nps = sh.num_lookups, sh.n_perm_sets
    L = [33 + 65 * (sh.num_instance_columns + sh.num_advice_columns) + 1]
    L.append(L[-1] + 65 * 2 * nl + 1)
    L.append(L[-1] + 1)
    L.append(L[-1] + 65 * (nps + nl + 1) + 1)
    L.append(L[-1] + 65 * sh.quotient_degree + 1)
    L.append(L[-1] + 33 * sh.scalars_per_proof() + 1)
    L.append(L[-1] + 1)
    return L


def facts(sh):
    """What the device code does with the shape (see the module docstring);
    np = 0 means k_acc_scalars' rows do not fit (PM_ERR_UNSUPPORTED)."""
    k = constants()
    sets = X._queries(sh)
    setlen = [len(qs) for _, qs in sets]
    S, nq = len(sets), sum(setlen)
    refs = []
    for _, qs in sets:
        for ref, _, _ in qs:
            if ref != A.H_POINT and ref not in refs:
                refs.append(ref)
    qd, bf, nl, nps = sh.quotient_degree, sh.blinding_factors, sh.num_lookups, sh.n_perm_sets
    nslots = len(refs) + qd
    T = nslots + 2 * S + 1
    Tp = sum(1 for ref in refs if ref[0] == "proof") + qd + 2 * S
    npair = (nslots + 1) // 2 + 2 * ((S + 1) // 2) + 1
    # the wave-2 / wave-3 split of k_acc_scalars: sets [0, J) to wave 3
    J = acc = 0
    while J < S and 2 * (acc + setlen[J]) <= nq:
        acc += setlen[J]
        J += 1
    # acc_lagrange_q
    nd = bf + 2
    nkmax = (nd + 2) // 3
    # k_acc_scalars' LDS: rows per proof and the tail (constants, program)
    nsc, npc = sh.scalars_per_proof(), len(sh.perm_columns)
    nvals = (2 * nps + 1 if nps else 0) + 5 * nl
    rows = nsc + T + k["kAccXVals"] + nvals + 2 * (bf + 3) + k["kAccStack"] + nslots + qd
    consts = []
    ncode = sum(len(H.compile_expressions(ex, consts)) for ex in (sh.gates, sh.lookup_inputs, sh.lookup_tables))
    c_n29 = len(consts) + npc + S + (bf + 2) + 1 + (bf + 2)
    p_rank = ncode + npc + S + 2 * nq + T + Tp
    tail = 4 * (8 * (c_n29 + 1) + p_rank + T)
    lds = k["kAccScalarsLds"]
    np_ = 0 if tail + 2 * 32 * rows > lds else min(16, (lds - tail) // (32 * rows) - 1)
    # the transcript
    L = squeeze_offsets(sh)
    npts = sh.points_per_proof()
    slots, nch = k["kTrSlots"], k["kTrChallenges"]
    nw32, nblk, npr = (L[6] + 3) // 4, (L[6] + 127) // 128, npts - S
    oD = (3 * nw32 + npr + 1) & ~1
    oS = (oD + (slots + 1) * (16 * npts + 8 * nsc) + 1) & ~1
    total = oS + 2 * slots * 16 * nblk + 3 * 2 * slots * 16 + 2 * nch * slots * 8 + nch * slots * 16 + 1 + nch
    depth = max([stack_depth(e) for e in sh.gates + sh.lookup_inputs + sh.lookup_tables] or [0])
    return dict(bf=bf, nd_mod3=nd % 3, logn_short=sh.log_n < 3 * nkmax, np=np_, rows=rows, nsets=S, J=J, T=T, Tp=Tp,
                npair=npair, nslots=nslots, nq=nq, max_set=max(setlen), n_perm_sets=nps, num_lookups=nl,
                stack=depth, L=L, L_mod=[v % 128 for v in L], stream_fits=4 * total <= lds,
                path=lambda B: X.acc_path(B, T, Tp, npair))


# ------------------------------------------------------------ directed shapes
def _logn_for(bf):
    n = 2
    while (1 << n) < bf + 3:
        n += 1
    return n


def _bf_shape(cid, bf, log_n=None):
    """Two permutation sets (l_0, l_last, 1 - l_last - l_blind and the `last`
    rotation -(bf + 1) all enter h_eval and e) on the smallest domain."""
    return build(cid, log_n=log_n or _logn_for(bf), bf=bf, na=2, adv_q=[(0, 0), (1, 0)], chunk=1,
                 perm=[(A.KIND_ADVICE, 0), (A.KIND_ADVICE, 1)], gates=[A.Prod(A.Advice(0), A.Advice(1))])


def _perm(cid, ncols, chunk, **kw):
    return build(cid, na=ncols, adv_q=[(i, 0) for i in range(ncols)], chunk=chunk,
                 perm=[(A.KIND_ADVICE, i) for i in range(ncols)], **kw)


def _consts(cid):
    r = P.CURVES[cid].r
    a, b = A.Advice(0), A.Advice(1)
    gates = [A.Sum(A.Prod(a, A.Const(0)), A.Sum(A.Prod(b, A.Const(1)), A.Prod(a, A.Const(r - 1)))),
             A.Sum(A.Scaled(a, 0), A.Sum(A.Scaled(b, 1), A.Scaled(A.Prod(a, b), r - 1))),
             A.Const(r - 1), A.Const(0)]
    return build(cid, na=2, adv_q=[(0, 0), (1, 1)], gates=gates)


def _mixed(cid):
    """Instance, advice and fixed columns, all three kinds in the permutation
    (two sets), one lookup over two expressions, rotations -1 .. 2."""
    gates = [A.Prod(A.Fixed(0), A.Sum(A.Prod(A.Advice(0), A.Advice(1)), A.Neg(A.Instance(0)))),
             A.Sum(A.Scaled(A.Advice(2), 7), A.Neg(A.Instance(1)))]
    return build(cid, log_n=5, bf=2, ni=1, na=2, nf=1, nl=1, chunk=2, inst_q=[(0, 0), (0, -1)],
                 adv_q=[(0, 0), (1, 0), (0, 2)], fixed_q=[(0, 0)],
                 perm=[(A.KIND_INSTANCE, 0), (A.KIND_FIXED, 0), (A.KIND_ADVICE, 1)], gates=gates,
                 lk_in=[A.Prod(A.Fixed(0), A.Advice(0)), A.Instance(0)], lk_tab=[A.Fixed(0), A.Advice(2)])


def nested_sum(n, nq=1):
    """A right-nested Sum of n leaves: the postfix stack grows to n."""
    e = A.Advice(0)
    for i in range(n - 1):
        e = A.Sum(A.Advice(i % nq), e)
    return e


def sets_shape(cid, nrot):
    """nrot rotation sets: advice column 0 at nrot consecutive rotations around 0."""
    lo = -(nrot // 2) + 1
    return build(cid, log_n=7, adv_q=[(0, r) for r in range(lo, lo + nrot)])


def set_size_shape(cid, nq):
    """nq queries in the one rotation set (H, r and two advice columns again and again)."""
    return build(cid, na=2, adv_q=[(i % 2, 0) for i in range(nq - 2)])


BIG = (1 << 31) - 1
DIRECTED = {
    # acc_lagrange_q: nd = bf + 2 denominators over three lanes of a quad
    "bf0": lambda c: _bf_shape(c, 0),          # nd % 3 == 2, lane 3 owns none, log_n 2 < 3 nkmax
    "bf1": lambda c: _bf_shape(c, 1),          # nd % 3 == 0, log_n 2
    "bf2": lambda c: _bf_shape(c, 2),          # nd % 3 == 1, log_n 3 < 3 nkmax = 6
    "bf4": lambda c: _bf_shape(c, 4),          # nd % 3 == 0, log_n 3
    "bf6": lambda c: _bf_shape(c, 6),
    "bf7": lambda c: _bf_shape(c, 7),          # nd % 3 == 0 with three full rounds
    "bf61": lambda c: _bf_shape(c, 61),        # the cap, nd = 63
    "logn_max": lambda c: _bf_shape(c, 1, TWO_ADICITY[c]),
    # structural branches
    "gates_only": lambda c: build(c, na=1, nf=1, fixed_q=[(0, 0)], gates=[A.Prod(A.Fixed(0), A.Advice(0))]),
    "perm1": lambda c: _perm(c, 2, 2),                     # one set: no `last` query
    "perm_chunk1": lambda c: _perm(c, 3, 1),               # three sets of one column
    "perm_ragged": lambda c: _perm(c, 5, 2),               # 2 + 2 + 1
    "perm_exact": lambda c: _perm(c, 4, 2),
    "lookups3": lambda c: build(c, na=1, nf=1, nl=3, fixed_q=[(0, 0)], lk_tab=[A.Fixed(0)]),
    "no_gates": lambda c: _perm(c, 2, 2, gates=[]),
    "no_gates_lookup": lambda c: build(c, nl=1, gates=[]),
    "qd1": lambda c: _perm(c, 2, 1, qd=1),
    "qd24": lambda c: _perm(c, 2, 1, qd=24),
    "stack16": lambda c: build(c, na=3, adv_q=[(0, 0), (1, 0), (2, 1)], gates=[nested_sum(16, 3)]),
    "last_rot_queried": lambda c: build(c, bf=1, na=2, adv_q=[(0, 0), (1, 0), (0, -2)], chunk=1,
                                        perm=[(A.KIND_ADVICE, 0), (A.KIND_ADVICE, 1)]),
    "big_rotations": lambda c: build(c, na=2, adv_q=[(0, 0), (1, BIG), (0, -BIG), (1, 65537)],
                                     gates=[A.Sum(A.Advice(1), A.Advice(2))]),
    "sets64": lambda c: sets_shape(c, 64),
    "set256": lambda c: set_size_shape(c, 256),
    "consts": _consts,
    "one_col_many_rots": lambda c: build(c, adv_q=[(0, r) for r in (0, -4, 3, -1, 4, 1, -3, 2, -2)],
                                         gates=[A.Prod(A.Advice(1), A.Advice(8))]),
    "mixed": _mixed,
}
# the facts each directed shape must keep showing (asserted in test_shapes_oracle.py)
DIRECTED_FACTS = {
    "bf0": dict(bf=0, nd_mod3=2, logn_short=True), "bf1": dict(nd_mod3=0, logn_short=True),
    "bf2": dict(nd_mod3=1, logn_short=True), "bf4": dict(nd_mod3=0), "bf6": dict(nd_mod3=2),
    "bf7": dict(nd_mod3=0), "bf61": dict(bf=61, nd_mod3=0),
    "gates_only": dict(n_perm_sets=0, num_lookups=0, nsets=1, J=0), "perm1": dict(n_perm_sets=1),
    "perm_chunk1": dict(n_perm_sets=3), "perm_ragged": dict(n_perm_sets=3), "perm_exact": dict(n_perm_sets=2),
    "lookups3": dict(num_lookups=3, n_perm_sets=0), "stack16": dict(stack=16), "sets64": dict(nsets=64),
    "set256": dict(max_set=256, nsets=1),
}


def _wide(cid, nrot, per):
    """per queries at each of nrot rotations over four advice columns, two
    permutation sets and a lookup (every role of k_acc_scalars has work)."""
    lo = -(nrot // 2)
    adv = [(0, 0), (1, 0)] + [(i % 4, lo + j) for j in range(nrot) for i in range(per)]
    return build(cid, log_n=6, bf=2, na=4, nl=1, chunk=1, adv_q=adv, perm=[(A.KIND_ADVICE, 0), (A.KIND_ADVICE, 1)],
                 gates=[A.Prod(A.Advice(2), A.Advice(3))])


@functools.lru_cache(maxsize=None)
def _wide_params(kind):
    """The smallest `per` at which the wide shape of `kind` has the np it is
    for (searched on facts(), so a changed LDS layout moves it, not breaks it)."""
    if kind == "last_fit":      # one query per rotation less than the first shape past the bound
        nrot, per = _wide_params("past")
        return nrot, per - 1
    nrot = {"np8_14": 8, "np3": 16, "past": 32}[kind]
    for per in range(1, 257):
        n = facts(_wide(2, nrot, per))["np"]
        if (kind == "np8_14" and 8 <= n <= 14) or (kind == "np3" and 1 <= n <= 3) or (kind == "past" and n == 0):
            return nrot, per
    raise RuntimeError("no wide shape for " + kind)


WIDE = {"wide_np8_14": lambda c: _wide(c, *_wide_params("np8_14")),
        "wide_np3": lambda c: _wide(c, *_wide_params("np3")),
        "wide_np1": lambda c: _wide(c, *_wide_params("last_fit"))}
HEAVY = ("wide_np3", "wide_np1")    # 800 / 2000 evaluations: the Python walks take seconds per proof
PAST_LDS = {"past_lds": lambda c: _wide(c, *_wide_params("past"))}


# ------------------------------------------------------ transcript-edge shapes
def _edge_min_nsc(nl, nps):
    return 1 + 1 + nps + (3 * nps - 1 if nps else 0) + 5 * nl


def _edge_shape(cid, c0, nl, nps, qd, nsc):
    """c0 advice columns (most of them never queried: they are absorbed and
    nothing else), nl lookups, nps permutation sets of one column, qd quotient
    pieces and nsc evaluations in all."""
    extra = nsc - _edge_min_nsc(nl, nps)
    assert extra >= 0
    adv = [(0, 0)] + [((1 + i) % c0, i % 2) for i in range(extra)]
    return build(cid, na=c0, nl=nl, qd=qd, chunk=1 if nps else 0, adv_q=adv, perm=[(A.KIND_ADVICE, 0)] * nps)


@functools.lru_cache(maxsize=None)
def edge_params():
    """{(k, residue): (c0, nl, nps, qd, nsc)}: for each squeeze k and residue
    in (0, 1, 127) the cheapest legal shape (points + evaluations) of
    _edge_shape's family with L_k = residue (mod 128).  65 and 33 are units
    mod 128 (inverses 65 and 97), so one count is solved for, the others are
    enumerated."""
    def Ls(c0, nl, nps, qd, nsc):
        L = [34 + 65 * c0]
        L.append(L[-1] + 130 * nl + 1)
        L.append(L[-1] + 1)
        L.append(L[-1] + 65 * (nps + nl + 1) + 1)
        L.append(L[-1] + 65 * qd + 1)
        L.append(L[-1] + 33 * nsc + 1)
        L.append(L[-1] + 1)
        return L

    out = {}
    for k in range(7):
        for res in (0, 1, 127):
            best = None
            for nl in range(3):
                for nps in range(4):
                    for qd in range(1, 9):
                        lo = _edge_min_nsc(nl, nps)
                        if k <= 4:
                            c0 = 65 * (res - Ls(0, nl, nps, qd, lo)[k]) % 128 or 128
                            cands = [(c0, lo)]
                        else:
                            cands = []
                            for c0 in range(1, 5):
                                nsc = 97 * (res - Ls(c0, nl, nps, qd, 0)[k]) % 128
                                while nsc < lo:
                                    nsc += 128
                                cands.append((c0, nsc))
                        for c0, nsc in cands:
                            assert Ls(c0, nl, nps, qd, nsc)[k] % 128 == res
                            cost = c0 + 3 * nl + nps + qd + nsc
                            if best is None or cost < best[0]:
                                best = (cost, (c0, nl, nps, qd, nsc))
            out[(k, res)] = best[1]
    return out


def _edge_names():
    names = {}
    for (k, res), prm in sorted(edge_params().items()):
        names.setdefault("edge_" + "_".join(str(v) for v in prm), (prm, []))[1].append((k, res))
    return names


EDGE_PAIRS = {nm: pairs for nm, (_, pairs) in _edge_names().items()}          # name -> [(k, residue)]
EDGES = {nm: (lambda c, prm=prm: _edge_shape(c, *prm)) for nm, (prm, _) in _edge_names().items()}

ALL = {}
for _d in (DIRECTED, WIDE, EDGES):
    ALL.update(_d)


@functools.lru_cache(maxsize=None)
def shape(cid, name):
    """The named shape on curve cid (treat it as read-only: it is shared)."""
    return (ALL.get(name) or PAST_LDS[name])(cid)


# ------------------------------------------------------------ random shapes
def _random_expr(rng, leaves, depth):
    if depth == 0 or rng.random() < 0.3:
        return rng.choice(leaves)
    op = rng.randrange(5)
    if op == 0:
        return A.Neg(_random_expr(rng, leaves, depth - 1))
    if op == 1:
        return A.Scaled(_random_expr(rng, leaves, depth - 1), rng.choice((0, 1, 2, 3, 1 << 200)))
    f = A.Sum if op < 4 else A.Prod
    return f(_random_expr(rng, leaves, depth - 1), _random_expr(rng, leaves, depth - 1))


def _draw(cid, rng):
    log_n = rng.randrange(2, 9)
    bf = rng.randrange(0, min(12, (1 << log_n) - 3) + 1)
    ni, na, nf = rng.randrange(0, 3), rng.randrange(1, 5), rng.randrange(0, 4)
    nl, qd = rng.randrange(0, 3), rng.randrange(1, 5)
    rots = list(range(-3, 4))

    def qs(n, extra):
        return [(rng.randrange(n), rng.choice((0, 0, rng.choice(rots)))) for _ in range(rng.randrange(extra + 1))] if n else []

    inst_q, adv_q, fixed_q = qs(ni, 3), [(0, 0)] + qs(na, 8), qs(nf, 4)
    cand = [(A.KIND_INSTANCE, i) for i in range(len(inst_q))] + [(A.KIND_ADVICE, i) for i in range(len(adv_q))] + \
        [(A.KIND_FIXED, i) for i in range(len(fixed_q))]
    perm = [rng.choice(cand) for _ in range(rng.choice((0, 0, 1, 2, 3, 5, 7)))]
    chunk = rng.randrange(1, 4) if perm or rng.random() < 0.5 else 0
    leaves = [A.Instance(i) for i in range(len(inst_q))] + [A.Advice(i) for i in range(len(adv_q))] + \
        [A.Fixed(i) for i in range(len(fixed_q))] + [A.Const(rng.choice((0, 1, 5, P.CURVES[cid].r - 1)))]
    gates = [_random_expr(rng, leaves, 3) for _ in range(rng.randrange(0, 4))]
    nex = rng.randrange(1, 3)
    lk_in = [_random_expr(rng, leaves, 2) for _ in range(nex)] if nl else []
    lk_tab = [_random_expr(rng, leaves, 2) for _ in range(nex)] if nl else []
    return build(cid, log_n=log_n, bf=bf, ni=ni, na=na, nf=nf, nl=nl, chunk=chunk, qd=qd, inst_q=inst_q, adv_q=adv_q,
                 fixed_q=fixed_q, perm=perm, gates=gates, lk_in=lk_in, lk_tab=lk_tab)


def random_shapes(cid, n, seed):
    """n legal shapes of at most MAX_POINTS points and MAX_EVALS evaluations
    from one seeded stream -> (shapes, redraws).  A draw that is not legal (no
    expression at all) or too large is redrawn from the same stream and
    counted; none is dropped silently."""
    rng = random.Random(seed)
    out, redraws = [], 0
    while len(out) < n:
        sh = _draw(cid, rng)
        if legal(cid, sh) or sh.points_per_proof() > MAX_POINTS or sh.scalars_per_proof() > MAX_EVALS:
            redraws += 1
            continue
        out.append(sh)
    return out, redraws


# ------------------------------------------------------------ synthetic proofs
class Batch:
    """B distinct proofs of a shape: idx (B, npts) pool indices (-1: the
    identity), scalars / challenges as integers; the packed arrays on demand."""

    def __init__(self, cid, sh, B, seed):
        self.cid, self.C, self.sh, self.B = cid, P.CURVES[cid], sh, B
        r = self.C.r
        npts, nsc = sh.points_per_proof(), sh.scalars_per_proof()
        self.idx, self.scalars, self.challenges = [], [], []
        for b in range(B):      # a stream per proof: a smaller batch of the same seed is a prefix
            rng = random.Random(seed * 1000003 + b)
            self.idx.append([rng.randrange(POOL) for _ in range(npts)])
            self.scalars.append([rng.randrange(r) for _ in range(nsc)])
            self.challenges.append([rng.randrange(r) for _ in range(7)])

    def proof(self, b):
        pts = pool(self.cid)[1]
        return A.Proof(points=[pts[i] if i >= 0 else None for i in self.idx[b]], scalars=list(self.scalars[b]),
                       challenges=list(self.challenges[b]))

    def pack(self):
        """-> (points (B, npts, 8), scalars (B, nsc, 4), challenges (B, 7, 4)) u64 Montgomery."""
        r = self.C.r
        lim = np.concatenate([pool(self.cid)[2], np.zeros((1, 8), dtype=np.uint64)])     # [-1]: the identity
        pts = lim[np.array(self.idx, dtype=np.int64).reshape(self.B, -1)]
        scs = np.array([[P.to_limbs(s * P.R_MONT % r) for s in row] for row in self.scalars],
                       dtype=np.uint64).reshape(self.B, -1, 4)
        chs = np.array([[P.to_limbs(s * P.R_MONT % r) for s in row] for row in self.challenges], dtype=np.uint64)
        return np.ascontiguousarray(pts), scs, chs

    def status(self, b):
        return A.proof_status(self.C, self.sh, self.challenges[b])

    def dlog_quad(self, b):
        """[sum c_t a_t]G per output from accum_edge_util's term plan -> (4, 8) u64."""
        C, dl = self.C, pool(self.cid)[0]
        pl = X.term_plan(C, self.sh, self.challenges[b], self.scalars[b])
        out = dict.fromkeys(X.OUTPUTS, 0)
        for t in pl.terms:
            kind, i = t["src"]
            a = (dl[self.idx[b][i]] if self.idx[b][i] >= 0 else 0) if kind == "proof" else \
                1 if kind == "g1" else self.sh.vk_dlogs[t["src"]]
            out[t["out"]] = (out[t["out"]] + t["coef"] * a) % C.r
        return np.array([P.point_to_limbs(C, C.mul(out[o], C.gen) if out[o] else None) for o in X.OUTPUTS],
                        dtype=np.uint64)


def limbs(C, vals):
    return np.array([A.to_limbs_mont(C.r, v) for v in vals], dtype=np.uint64)


# ----------------------------------------------------------------- references
# Computed once per (curve, shape, batch) and shared by the CPU and the GPU
# module; a caller must not modify what these return.
def _seed(cid, name, salt):
    return (zlib.crc32(name.encode()) ^ (cid << 24) ^ salt) & 0x7FFFFFFF


def vk_repr(cid, name):
    C = P.CURVES[cid]
    vkr = T.vk_repr(C.r, b"shape:" + name.encode())
    return vkr, np.array(A.to_limbs_mont(C.r, vkr), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def reference(cid, name, B):
    """B distinct proofs with caller challenges -> (batch, product shape,
    packed inputs, the C port's quads / h_eval / status)."""
    sh = shape(cid, name)
    bt = Batch(cid, sh, B, _seed(cid, name, 0xACC))
    ps = U.to_product_shape(cid, sh)
    arrs = bt.pack()
    _, q, h, st = R.accum_batch(cid, ps.c, *arrs, threads=8)
    return bt, ps, arrs, q, h, st


@functools.lru_cache(maxsize=None)
def transcript_reference(cid, name, B, identity_at):
    """B distinct proofs, proof identity_at with the identity as its first
    absorbed commitment -> (batch, product shape, points, scalars, vk limbs,
    the Python oracle's challenges (B, 7, 4) and status (B,))."""
    sh = shape(cid, name)
    C = P.CURVES[cid]
    bt = Batch(cid, sh, B, _seed(cid, name, 0x7A))
    bt.idx[identity_at][0] = -1
    vkr, vk = vk_repr(cid, name)
    rows = [T.replay_challenges(C, sh, bt.proof(b), vkr) for b in range(B)]
    ch = np.stack([limbs(C, c) for c, _ in rows])
    st = np.array([s for _, s in rows], dtype=np.uint32)
    pts, scs, _ = bt.pack()
    return bt, U.to_product_shape(cid, sh), pts, scs, vk, ch, st


def _non_residue_x(C):
    x = 2
    while PB.sqrt_mod(x ** 3 + C.b, C.p) is not None:
        x += 1
    return x


BYTES_B, BAD_POINT_AT, BAD_SCALAR_AT = 5, 1, 3


@functools.lru_cache(maxsize=None)
def bytes_reference(cid, name):
    """BYTES_B serialized proofs, one with a point that is not on the curve
    (its last point item) and one with a scalar = r (its first scalar item) ->
    (batch, product shape, proof bytes, instance limbs, vk limbs, the C port's
    batch_proofs dict)."""
    sh = shape(cid, name)
    C = P.CURVES[cid]
    bt = Batch(cid, sh, BYTES_B, _seed(cid, name, 0xB17E5))
    datas = [bytearray(PB.serialize(C, sh, bt.proof(b))) for b in range(BYTES_B)]
    items = PB.proof_items(sh)
    jp = max(j for j, (k, _) in enumerate(items) if k == "pt")
    js = min(j for j, (k, _) in enumerate(items) if k == "sc")
    datas[BAD_POINT_AT][32 * jp:32 * jp + 32] = _non_residue_x(C).to_bytes(32, "little")
    datas[BAD_SCALAR_AT][32 * js:32 * js + 32] = C.r.to_bytes(32, "little")
    datas = [bytes(d) for d in datas]
    ni = sh.num_instance_columns
    inst = np.ascontiguousarray(bt.pack()[0][:, :ni])
    _, vk = vk_repr(cid, name)
    ps = U.to_product_shape(cid, sh)
    buf = np.frombuffer(b"".join(datas), dtype=np.uint8).reshape(BYTES_B, -1)
    out = R.batch_proofs(cid, ps.c, buf, inst, vk_repr=vk, threads=4)
    return bt, ps, datas, inst, vk, out


SCALAR_BLOCK_SHAPES = ("gates_only", "bf1", "wide_np8_14")     # gates only, nd % 3 == 0, wide


@functools.lru_cache(maxsize=None)
def scalar_block_reference(cid, name):
    """Distinct proofs of the shape, each with one special value in the scalar
    block: theta, beta, gamma, y, v, u in {0, 1, r - 1}; x = 0; x with x^n =
    -1; x = omega^-i for every i <= bf + 1 (a zero Lagrange denominator each,
    PM_ACCUM_DENOM_ZERO), placed between the others so that each has clean
    neighbours; evaluations all 0 and all r - 1; a plain proof last.
    -> (batch, names, product shape, packed inputs, the C port's quads /
    h_eval / status)."""
    sh = shape(cid, name)
    r = P.CURVES[cid].r
    edits = [(f"{nm}={vn}", ci, val) for ci, nm in ((0, "theta"), (1, "beta"), (2, "gamma"), (3, "y"), (5, "v"), (6, "u"))
             for vn, val in (("0", 0), ("1", 1), ("r-1", r - 1))]
    edits += [("x=0", 4, 0), ("x^n=-1", 4, A.domain_omega(r, sh.log_n + 1)), ("evals=0", -1, 0), ("evals=r-1", -1, r - 1),
              ("plain", None, None)]
    winv = pow(sh.omega, -1, r)
    poles = [(f"x=omega^-{i}", 4, pow(winv, i, r)) for i in range(sh.blinding_factors + 2)]
    order = []
    for i, e in enumerate(edits):
        order.append(e)
        if i < len(poles):
            order.append(poles[i])
    assert len(poles) <= len(edits)
    bt = Batch(cid, sh, len(order), _seed(cid, name, 0x5CB))
    for b, (_, ci, val) in enumerate(order):
        if ci is None:
            continue
        if ci < 0:
            bt.scalars[b] = [val] * len(bt.scalars[b])
        else:
            bt.challenges[b][ci] = val
    ps = U.to_product_shape(cid, sh)
    arrs = bt.pack()
    _, q, h, st = R.accum_batch(cid, ps.c, *arrs, threads=8)
    return bt, [nm for nm, _, _ in order], ps, arrs, q, h, st

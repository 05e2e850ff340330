"""CPU tests of the quotient program compiler: pm_quotient_eval_host runs the
program compiled from a pm_proof_shape with the host field code, and must equal
the y-fold of oracle/accum.py::scalar_block's expressions bit for bit, on the
three scalar fields and across the shape family of tests/shape_util.py."""
import functools

import numpy as np
import pytest

import accum as A
import halo2_amd as H
import pasta as P
import poly_ref as R
import quotient_ref as Q
import shape_util as S

PM_ERR_ARG, PM_ERR_UNSUPPORTED = -1, -4
POINTS = 8
RANDOM_SEED = 0x0E5
CURVES = [0, 1, 2]


def want_fold(C, sh, scalars, ch7):
    pf = A.Proof(points=[None] * sh.points_per_proof(), scalars=list(scalars), challenges=list(ch7))
    exprs = A.scalar_block(C, sh, A._split(sh, pf), ch7)[0]
    return Q.fold(exprs, ch7[3], C.r)


def check(cid, sh, rows):
    """rows: [(scalars, ch7)] -> the host program's results equal the oracle's folds"""
    C = P.CURVES[cid]
    r = C.r
    ps = Q.product_shape(cid, sh)
    sc = np.array([[R.mont(r, v) for v in s] for s, _ in rows], dtype=np.uint64)
    x = np.array([R.mont(r, ch[4]) for _, ch in rows], dtype=np.uint64)
    ch = np.array([[R.mont(r, v) for v in ch[:4]] for _, ch in rows], dtype=np.uint64).reshape(len(rows), 16)
    got = H.quotient_eval_host(ps, sc, x, ch)
    want = np.array([R.mont(r, want_fold(C, sh, s, c)) for s, c in rows], dtype=np.uint64)
    bad = [i for i in range(len(rows)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad


def batch_rows(cid, sh, seed, n=POINTS):
    bt = S.Batch(cid, sh, n, seed)
    return [(bt.scalars[b], bt.challenges[b]) for b in range(n)]


@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("name", ["simple", "rich"])
def test_oracle_shapes(cid, name):
    C = P.CURVES[cid]
    sh = (A.simple_example_shape if name == "simple" else A.rich_shape)(C, 10)
    proofs = [A.synth_proof(C, sh, 0x51 + cid, b) for b in range(POINTS)]
    check(cid, sh, [(pf.scalars, pf.challenges) for pf in proofs])


@functools.lru_cache(maxsize=None)
def accepted(cid):
    return tuple(nm for nm in sorted(S.ALL) if S.legal(cid, S.shape(cid, nm)) == "")


@pytest.mark.parametrize("cid", CURVES)
def test_every_named_shape(cid):
    names = accepted(cid)
    assert len(names) == len(S.ALL)  # the family holds legal shapes only; PAST_LDS is apart
    for nm in names:
        sh = S.shape(cid, nm)
        check(cid, sh, batch_rows(cid, sh, S._seed(cid, nm, 0x907)))


@pytest.mark.parametrize("cid", CURVES)
def test_random_shapes(cid):
    shapes, redraws = S.random_shapes(cid, 40, RANDOM_SEED + cid)
    assert len(shapes) == 40 and redraws >= 0
    for i, sh in enumerate(shapes):
        assert S.legal(cid, sh) == "", i
        check(cid, sh, batch_rows(cid, sh, 7000 + 41 * cid + i))


@pytest.mark.parametrize("cid", CURVES)
@pytest.mark.parametrize("name", ["gates_only", "no_gates", "no_gates_lookup", "perm1", "perm_chunk1", "mixed"])
def test_special_challenges(cid, name):
    """theta, beta, gamma, y in {0, 1, r - 1}, one at a time and all at once
    (y = 0: only the last expression survives), on a gates-only, a
    permutation-only and a lookups-only shape, one permutation set and three."""
    r = P.CURVES[cid].r
    sh = S.shape(cid, name)
    rows = []
    base = batch_rows(cid, sh, 0xC4 + cid, 13)
    k = 0
    for val in (0, 1, r - 1):
        for ci in range(4):
            s, ch = base[k]
            ch = list(ch)
            ch[ci] = val
            rows.append((s, ch))
            k += 1
    s, ch = base[12]
    rows.append((s, [0, 0, 0, 0] + list(ch[4:])))
    rows.append(([0] * len(s), ch))
    rows.append(([r - 1] * len(s), ch))
    check(cid, sh, rows)


def test_y_zero_keeps_the_last_expression_only():
    cid = 2
    C = P.CURVES[cid]
    sh = S.shape(cid, "mixed")
    s, ch = batch_rows(cid, sh, 99, 1)[0]
    ch = list(ch)
    ch[3] = 0
    pf = A.Proof(points=[None] * sh.points_per_proof(), scalars=list(s), challenges=ch)
    last = A.scalar_block(C, sh, A._split(sh, pf), ch)[0][-1]
    assert want_fold(C, sh, s, ch) == last
    check(cid, sh, [(s, ch)])


def test_no_expression_shape_is_an_argument_error():
    sh = S.build(2, gates=[])
    assert S.legal(2, sh) == "no expressions"
    ps = Q.product_shape(2, sh)
    z = np.zeros((1, 4), dtype=np.uint64)
    rc = H.lib().pm_quotient_eval_host(2, ps.c, 1, H._p(np.zeros((1, 2, 4), dtype=np.uint64)), H._p(z),
                                       H._p(np.zeros(16, dtype=np.uint64)), H._p(z))
    assert rc == PM_ERR_ARG and b"no expressions" in H.lib().pm_last_error()


def _leaning(op, n, left):
    e = A.Advice(0)
    for i in range(1, n):
        leaf = A.Advice(i % 3)
        e = op(e, leaf) if left else op(leaf, e)
    return e


@pytest.mark.parametrize("cid", CURVES)
def test_depth_16_expressions_are_accepted(cid):
    """Left- and right-leaning sums and products of 16 leaves (postfix stack
    depth 2 and 16, the validation's bound): both compile within the slot
    budget and evaluate to the oracle's value."""
    gates = [_leaning(op, 16, left) for op in (A.Sum, A.Prod) for left in (True, False)]
    assert sorted(S.stack_depth(g) for g in gates) == [2, 2, 16, 16]
    sh = S.build(cid, na=3, adv_q=[(0, 0), (1, 0), (2, 1)], gates=gates)
    assert S.legal(cid, sh) == ""
    check(cid, sh, batch_rows(cid, sh, 1600 + cid))
    # the deepest user of slots: a lookup holds its left side and both compressed sums around such an expression
    deep = [_leaning(A.Sum, 16, False), _leaning(A.Prod, 16, False)]
    lk = S.build(cid, na=3, nl=1, adv_q=[(0, 0), (1, 0), (2, 1)], gates=[], lk_in=deep, lk_tab=deep[::-1])
    assert S.legal(cid, lk) == ""
    check(cid, lk, batch_rows(cid, lk, 1650 + cid))
    deeper = S.build(cid, na=3, adv_q=[(0, 0), (1, 0), (2, 1)], gates=[_leaning(A.Sum, 17, False)])
    ps = Q.product_shape(cid, deeper)
    z = np.zeros((1, 4), dtype=np.uint64)  # depth 17: the shape validation's bound, not the slot budget
    rc = H.lib().pm_quotient_eval_host(cid, ps.c, 1, H._p(np.zeros((1, 5, 4), dtype=np.uint64)), H._p(z),
                                       H._p(np.zeros(16, dtype=np.uint64)), H._p(z))
    assert rc == PM_ERR_ARG and b"stack deeper than 16" in H.lib().pm_last_error()

"""CPU: the lazy bounds of k_pairing_run on tests/pairing_lazy_model.py, the
limb-level model of the kernel (no GPU).

The GPU tests compare the kernel's words with the host form and the reference;
they see about 40 distinct items whose intermediate values are effectively
random, so a bound crossed once in 10^4 items would pass them.  Here
  * the whole program runs on four constructed items and must give
    pairing_ref's 48 words bit for bit (so the model is pinned to the reference
    and a failing bound is not a model error), with every invariant asserted at
    every step;
  * every operation of the program runs on register states at the edge of the
    invariant (representatives v + j p below 3p, the largest Norm value below 3p,
    all low limbs 0x1FFFFFFF) and on random states drawn uniformly from [0, 3p),
    and must give pairing_ref's Fp12 operation mod p with outputs Norm and < 3p:
    the invariant is inductive;
  * f29_reduce3 for BN254 Fq is checked over every top limb;
  * two deliberately broken models (negation by 2p, no reduction after
    fold_xi's << 2) must raise.

Recorded maxima against the bounds the kernel states (asserted against the
bounds, not against these figures):

    value                 bound      whole program (4 items)   operations at the edge
    stored to LDS         < 3p       1.186884 p                1.206892 p computed (Frobenius); 3p - 1
                                                               where kOpConj passes an even coefficient on
    f29_reduce3 input     < 16p      9.000000 p                9.000000 p
    a b + u v             < 99 p^2   36.035249 p^2             38.777703 p^2 (Frobenius, stated 42 p^2);
                                                               kOpMul reaches its stated 27 p^2, a line 21 p^2
    f29_reduce3 output    < 3p       1.000000 p                1.000000109 p; over every top limb
                                                               (test_reduce3_every_top_limb) 1.000012067 p
The figures at whole multiples of p are zero coefficients in a non-canonical form (a coefficient
that is 0 mod p travels as p, 6p or 9p); the words at the end are the reference's all the same.

Run time of this file: 19 s on 8 cores of a build host (1.3 s per whole-program item, 3 to 4 s for
each of kOpMul, kOpLine and kOpFrob at the edge, 1.6 s for f29_reduce3 over 5.07e7 top limbs).
"""
import random

import numpy as np
import pairing_lazy_model as L
import pairing_ref as PR
import pairing_util as U
import plan_native as N
import pytest

P = PR.P
# the kernel's stated bounds, in units of p (a b + u v: of p^2)
BOUND = {"lds": 3, "reduce3_in": 16, "reduce3_out": 3, "prod": 99}
N_RANDOM = {"mul": 1200, "line": 1500, "frob": 300, "conj": 300, "scale_inv": 300}
SEEN = {}   # test -> maxima in units of p, printed as they are recorded (pytest -s shows them)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return L.Plan(N.ask1(N.build(tmp_path_factory), "pairing"))


@pytest.fixture(scope="module")
def lines(plan):
    return L.device_lines(plan, U.s_g2(), PR.G2)


def _record(name, m):
    mx = m.maxima()
    for k, v in m.mx.items():   # on the integers: 3p - 1 is below 3p, (3p - 1) / p as a float is not
        assert v < BOUND[k] * (P * P if k == "prod" else P), (name, k, mx[k])
    SEEN[name] = mx
    print("%s: %s" % (name, ", ".join("%s %.9f" % kv for kv in sorted(mx.items()))))


def test_constants_are_the_field():
    k = L.consts()
    assert L.val(k["P"]) == P and L.is_norm(k["P"])
    assert (P * k["INV"] + 1) % (1 << 29) == 0
    assert L.val(k["ONE"]) == L.R % P and L.val(k["TO256"]) == (1 << 256) % P
    assert L.val(k["R783"]) == pow(2, 783, P)
    assert L.val(k["K6"]) == 6 * P and L.val(k["K2"]) == 2 * P
    assert min(k["K6"][:8]) >= L.M29 and min(k["K2"][:8]) >= L.M29
    assert k["QMAGIC"] == (1 << 40) // (k["P"][8] + 1)
    assert L.R > 169 * P and L.MUL2_BOUND > 99 * P * P   # the header's 169 p and 99 p^2


def test_plan_query(plan):
    """the program, the schedule and the constants the model runs are pairing_plan.hpp's"""
    assert (plan.steps, plan.ops, plan.slots) == (102, 576, 8)
    codes = [w & 255 for w in plan.prog]
    op = plan.op
    assert [codes.count(op[n]) for n in ("kOpMul", "kOpLine", "kOpFrob", "kOpConj", "kOpScaleInv")] == [354, 204, 10, 7, 1]
    # a doubling per bit of 6x + 2 below the top one, an addition after each set bit, two Frobenius steps
    want = []
    for bit in bin(PR.LOOP)[3:]:
        want += [1] + ([0] if bit == "1" else [])
    assert plan.doubles == want + [0, 0]
    for j in (1, 2):
        for k in range(6):
            assert plan.frob[j - 1][k] == PR.f2_pow(PR.XI, k * (P**j - 1) // 6), (j, k)


# ---------------------------------------------------------------- the whole program
@pytest.mark.parametrize("name", ["accept", "reject_d_plus_1", "w_inf_sum_not_inf", "zw_eq_neg_f_accept"])
def test_whole_program(plan, lines, name):
    """k_pairing_run's model on one item: pairing_ref's words bit for bit, every invariant on the way"""
    fam = {f[0]: f for f in U.family()}
    _, quad, _, ok, _ = fam[name]
    w, zw, f, e = (U.ref_point(quad[i]) for i in range(4))
    A, C = w, PR.g1_neg(PR.g1_add(PR.g1_add(zw, f), e))   # what k_pairing_prep hands over
    m = L.Model(plan)
    got_ok, got = m.run(lines, A, C)
    assert np.array_equal(got, U.ref_gt_words(quad)), name
    assert got_ok == ok
    _record(name, m)


# ---------------------------------------------------------------- each operation at the edge
def edge_values(rng):
    """representatives below 3p: v + j p for v in {0, 1, p - 1, random}, the largest Norm value
    below 3p, and all eight low limbs 0x1FFFFFFF under the largest top limb that stays below 3p"""
    vs = []
    for v in (0, 1, P - 1, rng.randrange(P)):
        vs += [L.limbs(v + j * P) for j in range(3)]
    vs.append(L.limbs(3 * P - 1))
    top = (3 * P >> 232) - 1
    ones = [L.M29] * 8 + [top]
    assert L.val(ones) < 3 * P <= L.val([L.M29] * 8 + [top + 1])
    vs.append(ones)
    assert all(L.is_norm(a) and L.val(a) < 3 * P for a in vs)
    return vs


def rand_f(rng):
    return L.limbs(rng.randrange(3 * P))


def rand6(rng):
    return [(rand_f(rng), rand_f(rng)) for _ in range(6)]


def pick6(rng, vs):
    return [(rng.choice(vs), rng.choice(vs)) for _ in range(6)]


def check_mul(m, a6, b6):
    r = m.put(m.op_mul(a6, b6))
    assert L.decode(r) == L.from_f12(PR.f12_mul(L.to_f12(L.decode(a6)), L.to_f12(L.decode(b6))))


def check_line(m, f6, lc, xp, yp, inf):
    r = m.put(m.op_line(f6, lc, xp, yp, inf))
    lam, c = (L.from_mont(lc[0]), L.from_mont(lc[1])), (L.from_mont(lc[2]), L.from_mont(lc[3]))
    x, y = L.from_mont(xp), L.from_mont(yp)
    line = (((y, 0), PR.F2_ZERO, PR.F2_ZERO),
            (PR.f2_neg(PR.f2_scale(lam, x)), PR.F2_ZERO if inf else c, PR.F2_ZERO))
    assert L.decode(r) == L.from_f12(PR.f12_mul(L.to_f12(L.decode(f6)), line))


def check_frob(m, a6, j, by_power=False):
    r = m.put(m.op_frob(a6, j))
    a = L.decode(a6)
    want = [PR.f2_mul(PR.f2_conj(a[k]) if j & 1 else a[k], PR.f2_pow(PR.XI, k * (P**j - 1) // 6)) for k in range(6)]
    assert L.decode(r) == want
    if by_power:   # the definition itself: a^(p^j)
        assert want == L.from_f12(PR.f12_pow(L.to_f12(a), P**j))


def check_conj(m, a6, by_power=False):
    r = m.put(m.op_conj(a6))
    a = L.decode(a6)
    want = [PR.f2_neg(a[k]) if k & 1 else a[k] for k in range(6)]
    assert L.decode(r) == want
    if by_power:
        assert want == L.from_f12(PR.f12_pow(L.to_f12(a), P**6))


def check_scale_inv(m, a6, n):
    r = m.put(m.op_scale_inv(a6, n))
    ni = PR.f2_inv((L.from_mont(n[0]), L.from_mont(n[1])))
    assert L.decode(r) == [PR.f2_mul(a, ni) for a in L.decode(a6)]


def edges_mul(m, rng, n_random):
    vs = edge_values(rng)
    for pa in vs:
        for pb in vs:
            check_mul(m, [(pa, pa)] * 6, [(pb, pb)] * 6)
    for _ in range(100):
        check_mul(m, pick6(rng, vs), pick6(rng, vs))
    for _ in range(n_random):
        check_mul(m, rand6(rng), rand6(rng))


def edges_line(m, rng, n_random):
    vs = edge_values(rng)
    k = m.K
    c0, cm = L.limbs(0), L.limbs(P - 1)
    # x_P = 0: -x_P is 6p exactly
    assert L.val(m.negn(c0)) == 6 * P
    for lc in [[a, b, c, d] for a in (c0, cm) for b in (c0, cm) for c in (c0, cm) for d in (c0, cm)]:
        for xp in (c0, cm):
            for inf in (0, 1):
                for pf in vs:
                    check_line(m, [(pf, pf)] * 6, lc, xp, cm, inf)
    for _ in range(100):
        check_line(m, pick6(rng, vs), [rng.choice((c0, cm)) for _ in range(4)], rng.choice((c0, cm)), cm, rng.randrange(2))
    for _ in range(n_random):
        # as the kernel meets them: table and point canonical, the identity as (0, 1) with the flag
        inf = rng.randrange(4) == 0
        xp, yp = (c0, k["ONE"]) if inf else (L.limbs(rng.randrange(P)), L.limbs(rng.randrange(P)))
        check_line(m, rand6(rng), [L.limbs(rng.randrange(P)) for _ in range(4)], xp, yp, int(inf))


def edges_frob(m, rng, n_random):
    vs = edge_values(rng)
    for j in (1, 2):
        for i, pa in enumerate(vs):
            check_frob(m, [(pa, pa)] * 6, j, by_power=i in (3, 13))
        for i in range(40):
            check_frob(m, pick6(rng, vs), j, by_power=i == 0)
        for i in range(n_random):
            check_frob(m, rand6(rng), j, by_power=i < 3)


def edges_conj(m, rng, n_random):
    vs = edge_values(rng)
    for pa in vs:
        check_conj(m, [(pa, pa)] * 6)
    for i in range(n_random):
        check_conj(m, rand6(rng), by_power=i == 0)


def edges_scale_inv(m, rng, n_random):
    vs = edge_values(rng)
    for pa in vs:
        for pn in vs:
            check_scale_inv(m, [(pa, pa)] * 6, (pn, pn))
    for _ in range(100):
        check_scale_inv(m, pick6(rng, vs), (rng.choice(vs), rng.choice(vs)))
    for _ in range(n_random):
        check_scale_inv(m, rand6(rng), (rand_f(rng), rand_f(rng)))


EDGES = {"mul": edges_mul, "line": edges_line, "frob": edges_frob, "conj": edges_conj, "scale_inv": edges_scale_inv}


@pytest.mark.parametrize("op", sorted(EDGES))
def test_operation_at_the_edge_of_the_invariant(plan, op):
    m = L.Model(plan)
    EDGES[op](m, random.Random(0x10 + len(op)), N_RANDOM[op])
    _record("edge_" + op, m)


def test_final_conversion_takes_every_representative(plan):
    """an accepted proof ends at 1 mod p, as 1, p + 1 or 2p + 1 in Montgomery form depending on the
    path: f29_to_r256 gives the canonical words for every representative below 4p"""
    m = L.Model(plan)
    rng = random.Random(7)
    one = L.val(m.K["ONE"])
    for v in (0, 1, one, P - 1, rng.randrange(P), rng.randrange(P)):
        for j in range(4):
            assert m.to_r256(L.limbs(v + j * P)) == PR.fp_words(v * L.RINV % P), (v, j)
    assert m.to_r256(L.limbs(one + 2 * P)) == PR.fp_words(1)
    with pytest.raises(L.BoundError):
        m.to_r256(L.limbs(4 * P))


# ---------------------------------------------------------------- f29_reduce3, every top limb
def test_reduce3_every_top_limb():
    """a_8 = 0 .. 16 p_8 + 1 with the low 232 bits at 0 and at all ones, inputs below 16p.  numpy
    computes the magic multiply's q for every a_8; v - q p is increasing in v where q is constant, so
    the least and the greatest result of each run of equal q are taken exactly, on Python integers."""
    k = L.consts()
    p8, magic = k["P"][8], k["QMAGIC"]
    n = 16 * p8 + 2
    low1 = (1 << 232) - 1
    worst, count = 0, 0
    runs, run_lo, cur_q = [], 0, 0   # runs of equal q: (first a_8, last a_8, q)
    for start in range(0, n, 1 << 22):
        a8 = np.arange(start, min(n, start + (1 << 22)), dtype=np.uint64)
        q = ((a8 * np.uint64(magic)) >> np.uint64(40)).astype(np.int64)
        # the exact quotient by p_8 + 1, which the magic multiply may miss by one from below
        exact = (a8 // np.uint64(p8 + 1)).astype(np.int64)
        assert (q <= exact).all() and (exact - q <= 1).all()
        step = np.diff(np.concatenate(([cur_q], q)))
        assert (step >= 0).all()   # q never steps down
        for i in np.flatnonzero(step):
            runs.append((run_lo, start + int(i) - 1, cur_q))
            run_lo, cur_q = start + int(i), int(q[i])
        count += len(a8)
    runs.append((run_lo, n - 1, cur_q))
    assert count == n and sum(hi - lo + 1 for lo, hi, _ in runs) == n
    for lo, hi, q in runs:
        assert q == (lo * magic) >> 40 == (hi * magic) >> 40
        vmin = lo << 232
        if vmin >= 16 * P:
            continue
        vmax = min((hi << 232) + low1, 16 * P - 1)
        rmin, rmax = vmin - q * P, vmax - q * P
        assert 0 <= rmin and rmax < 3 * P, (lo, hi, q)
        worst = max(worst, rmax)
    SEEN["reduce3_every_top_limb"] = {"reduce3_out": worst / P}
    print("reduce3 over %d top limbs in %d runs of q: largest result %.9f p" % (n, len(runs), worst / P))
    assert worst / P < BOUND["reduce3_out"]
    # the model's limb-level reduce3 agrees with v - q p at the ends of every run
    m = L.Model.__new__(L.Model)
    m.K, m.PL, m.mx = k, k["P"], {"reduce3_in": 0, "reduce3_out": 0}
    for lo, hi, q in runs:
        for v in (lo << 232, min((hi << 232) + low1, 16 * P - 1)):
            if v < 16 * P:
                assert L.val(m.reduce3(L.limbs(v))) == v - q * P


# ---------------------------------------------------------------- the model can fail
def test_negation_by_2p_breaks_dominance(plan):
    """fq_negn with K2 in place of K6: a representative above 2p has a top limb K2's does not cover"""
    m = L.Model(plan, neg_const="K2")
    with pytest.raises(L.BoundError) as e:
        edges_mul(m, random.Random(1), 20)
    assert e.value.kind == "dominance"
    m = L.Model(plan, neg_const="K2")
    with pytest.raises(L.BoundError) as e:
        edges_conj(m, random.Random(2), 20)
    assert e.value.kind == "dominance"


def test_fold_xi_without_its_reduction_breaks_a_bound(plan):
    """fq2_fold_xi with 4 h left unreduced: 2 (4 h) + h + 6p - h' reaches 33p and limbs of 2^32"""
    kinds = set()
    for fn, seed in ((edges_mul, 3), (edges_line, 4)):
        m = L.Model(plan, fold_reduce_shift=False)
        with pytest.raises(L.BoundError) as e:
            fn(m, random.Random(seed), 20)
        kinds.add(e.value.kind)
    assert kinds <= {"limb", "reduce3_input"}, kinds


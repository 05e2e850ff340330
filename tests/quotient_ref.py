"""Reference of the quotient numerator on the extended domain (tests only):
for each extended row j it builds the `d` dictionary of oracle/accum.py from
integer columns, calls accum.scalar_block at x = X_j = zeta omega_e^j and
folds the returned expressions in y, without the division by x^n - 1.

A column's extended form is col[j] = p(X_j); a query (column, rot) at row j
reads col[(j + rot 2^e) mod N].  The domain is tests/domain_ref.Domain and the
shape's omega is set to the domain's (the two helpers may pick different
generators).  Values are plain integers mod r; the kernel is not linear, so the
device gets true Montgomery words (poly_ref.mont)."""
import dataclasses
import random

import numpy as np

import accum as A
import accum_util as U
import domain_ref as D
import pasta as P
import poly_ref as R

GROUPS = ("advice", "fixed", "instance", "sigma", "perm_z", "lookup_a", "lookup_s", "lookup_z")


def domain_for(cid, k, e):
    return D.Domain(P.CURVES[cid].r, k, k + e)


def on_domain(sh, dom):
    """the shape with the domain's k and omega"""
    assert sh.log_n == dom.k
    return dataclasses.replace(sh, omega=dom.omega)


def counts(sh):
    return dict(zip(GROUPS, (sh.num_advice_columns, sh.num_fixed_columns, sh.num_instance_columns, len(sh.perm_columns),
                             sh.n_perm_sets, sh.num_lookups, sh.num_lookups, sh.num_lookups)))


def random_columns(sh, N, r, seed):
    rng = random.Random(seed)
    return {g: [[rng.randrange(r) for _ in range(N)] for _ in range(c)] for g, c in counts(sh).items()}


def constant_columns(sh, N, value):
    return {g: [[value] * N for _ in range(c)] for g, c in counts(sh).items()}


def fold(exprs, y, r):
    h = exprs[0]
    for e in exprs[1:]:
        h = (h * y + e) % r
    return h


def evals_from(sh, read):
    """the d dictionary of accum.scalar_block; read(group, column, rot) -> the evaluation"""
    last = -(sh.blinding_factors + 1)
    return dict(
        inst_ev=[read("instance", c, rot) for c, rot in sh.instance_queries],
        adv_ev=[read("advice", c, rot) for c, rot in sh.advice_queries],
        fixed_ev=[read("fixed", c, rot) for c, rot in sh.fixed_queries],
        sigma_ev=[read("sigma", k, 0) for k in range(len(sh.perm_columns))],
        perm_sets=[dict(eval=read("perm_z", i, 0), next=read("perm_z", i, 1), last=read("perm_z", i, last))
                   for i in range(sh.n_perm_sets)],
        lookups=[dict(z=read("lookup_z", i, 0), z_w=read("lookup_z", i, 1), a=read("lookup_a", i, 0),
                      a_prev=read("lookup_a", i, -1), s=read("lookup_s", i, 0)) for i in range(sh.num_lookups)])


def expressions(C, sh, d, ch4, x):
    theta, beta, gamma, y = ch4
    return A.scalar_block(C, sh, d, [theta, beta, gamma, y, x, 0, 0])[0]


def row(C, sh, dom, cols, ch4, j, start=None):
    """out[j]; start: the value the fold starts from (PM_QUOT_ACCUMULATE)"""
    step = 1 << dom.e
    d = evals_from(sh, lambda g, c, rot: cols[g][c][(j + rot * step) % dom.N])
    x = dom.zeta * pow(dom.extended_omega, j, dom.r) % dom.r
    ex = expressions(C, sh, d, ch4, x)
    return fold(ex if start is None else [start] + ex, ch4[3], dom.r)


def numerator(C, sh, dom, cols, ch4, rows=None, start=None):
    rows = range(dom.N) if rows is None else rows
    return [row(C, sh, dom, cols, ch4, j, None if start is None else start[j]) for j in rows]


def mont_columns(r, cols):
    """{group: [(N, 4) u64 Montgomery]}"""
    return {g: [R.to_array(r, c) for c in cs] for g, cs in cols.items()}


def product_shape(cid, sh):
    """the halo2_amd.ProofShape of an oracle shape (VK points are not read by the quotient)"""
    if len(sh.fixed_commitments) != sh.num_fixed_columns or len(sh.sigma_commitments) != len(sh.perm_columns):
        sh = A.synth_vk_points(P.CURVES[cid], dataclasses.replace(sh))
    return U.to_product_shape(cid, sh)


def challenges_array(r, ch4):
    return np.array([R.mont(r, c) for c in ch4], dtype=np.uint64).reshape(4, 4)

"""Python big-int restatement of the prover's opening arithmetic, the reference
of tests/test_poly_*.py.  The halo2 fork's crates are not vendored under the
reference (its Cargo.toml:10-12 names them as git dependencies), so, as
oracle/ does for the verifier, the definitions are restated here from

  * halo2 `src/arithmetic.rs` [3P]: `eval_polynomial(poly, point)` and
    `kate_division(a, b)`, written as the same loops;
  * halo2 `src/poly/multiopen/gwc/prover.rs` [3P]: per rotation set,
    `poly_batch = poly_batch * v + query.poly`, `eval_batch = eval_batch * v +
    eval`, `poly_batch[0] -= eval_batch`, `witness = kate_division(poly_batch,
    z)`, `W = commit(witness)`.

Values are plain integers mod r unless a name says `mont`.  Division and the
batch are linear in the coefficients, so they may be fed Montgomery-form
coefficients (a R mod r) with plain z and v and return Montgomery-form
results; the large-size test uses that to skip 2^20 conversions."""
import numpy as np

import pasta as P


def eval_polynomial(poly, point, r):
    """arithmetic.rs eval_polynomial: rev().fold(0, |acc, c| acc * point + c)."""
    acc = 0
    for coeff in reversed(poly):
        acc = (acc * point + coeff) % r
    return acc


def kate_division(a, b, r):
    """arithmetic.rs kate_division: a(X) / (X - b), len(a) - 1 coefficients."""
    b = -b % r
    q = [0] * (len(a) - 1)
    tmp = 0
    for i, coeff in zip(range(len(q) - 1, -1, -1), reversed(a)):
        lead_coeff = (coeff - tmp) % r
        q[i] = lead_coeff
        tmp = lead_coeff * b % r
    return q


def batch_poly(polys, v, r):
    """gwc/prover.rs: poly_batch = poly_batch * v + query.poly, in query order."""
    acc = [0] * len(polys[0])
    for p in polys:
        acc = [(x * v + y) % r for x, y in zip(acc, p)]
    return acc


def gwc_witness(polys, z, v, r):
    """gwc/prover.rs, one rotation set: (witness polynomial, batched evaluation)."""
    poly_batch = batch_poly(polys, v, r)
    eval_batch = 0
    for p in polys:
        eval_batch = (eval_batch * v + eval_polynomial(p, z, r)) % r
    poly_batch[0] = (poly_batch[0] - eval_batch) % r
    return kate_division(poly_batch, z, r), eval_batch


def mont(r, v):
    return P.to_limbs(v * P.R_MONT % r)


def unmont(r, row):
    return P.from_limbs([int(x) for x in row]) * pow(P.R_MONT, -1, r) % r


def to_array(r, vals):
    """plain integers -> (n, 4) u64 Montgomery"""
    return np.array([mont(r, v) for v in vals], dtype=np.uint64).reshape(len(vals), 4)


def raw_ints(arr):
    """(n, 4) u64 -> the n 256-bit integers as stored (no Montgomery conversion)"""
    b = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def from_raw(vals):
    """n integers < 2^256 -> (n, 4) u64 as stored"""
    b = b"".join(v.to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype="<u8").reshape(len(vals), 4).astype(np.uint64)


def from_array(r, arr):
    rinv = pow(P.R_MONT, -1, r)
    return [v * rinv % r for v in raw_ints(arr)]


def srs(cid, tau, n):
    """G_t = [tau^t] G, t < n: (points, (n, 8) u64 affine Montgomery)"""
    C = P.CURVES[cid]
    pts, t = [], 1
    for _ in range(n):
        pts.append(C.mul(t, C.gen))
        t = t * tau % C.r
    return pts, np.array([P.point_to_limbs(C, q) for q in pts], dtype=np.uint64)

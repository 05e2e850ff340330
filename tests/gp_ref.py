"""Python big-int restatement of the prover's grand products, the reference of
tests/test_gp_*.py.  halo2's crates are not vendored under the reference (its
Cargo.toml:10-12 names them as git dependencies), so, as tests/poly_ref.py does
for the openings, the definitions are restated here from

  * ff `BatchInvert::batch_invert` [3P]: every non-zero element is replaced by
    its inverse, zeros are skipped and stay zero;
  * halo2 `src/plonk/permutation/prover.rs::commit` [3P]: per column chunk,
    modified_values *= beta * sigma + gamma + value, batch_invert, then
    modified_values *= delta^k beta omega^i + gamma + value, and
    z[0] = last_z, z[i + 1] = z[i] * modified_values[i];
  * halo2 `src/plonk/lookup/prover.rs::commit_product` [3P]: denominator
    (A' + beta)(S' + gamma), batch_invert, numerator (A + beta)(S + gamma),
    z[0] = 1, z[i + 1] = z[i] * ratio[i].

A factor is a tuple (x, y, b, g): one linear term f[i] = x[i] + b * y[i] + g per
row, x a column index or None (0), y a column index, OMEGA (the implicit column
omega^i) or None, b and g integers mod r.  Values are plain integers mod r;
products are not linear in the stored Montgomery words, so tests convert with
poly_ref.mont / to_array."""
import random

OMEGA = "omega"


def batch_invert(vals, r):
    """ff BatchInvert: a[i] <- a[i]^-1, zeros stay zero."""
    return [pow(v, r - 2, r) if v % r else 0 for v in vals]


def factor_row(cols, f, i, omega, r):
    x, y, b, g = f
    v = g
    if x is not None:
        v += cols[x][i]
    if y == OMEGA:
        v += b * pow(omega, i, r)
    elif y is not None:
        v += b * cols[y][i]
    return v % r


def list_rows(cols, factors, rows, omega, r):
    """the product of a factor list at rows [0, rows); an empty list gives 1"""
    out = [1] * rows
    for f in factors:
        x, y, b, g = f
        w = 1
        for i in range(rows):
            v = g
            if x is not None:
                v += cols[x][i]
            if y is not None:
                if y == OMEGA:
                    v += b * w
                    w = w * omega % r
                else:
                    v += b * cols[y][i]
            out[i] = out[i] * v % r
    return out


def grand_product_literal(cols, num, den, n, active, start, omega, r):
    """z[0] = start, z[i + 1] = z[i] * N[i] * inv0(D[i]) for i < active - 1,
    with one pow per row.  Returns (z[0 .. active), last)."""
    N = list_rows(cols, num, active - 1, omega, r)
    D = list_rows(cols, den, active - 1, omega, r)
    z = [start % r]
    for i in range(active - 1):
        z.append(z[i] * N[i] % r * pow(D[i], r - 2, r) % r)  # pow(0, r - 2) = 0
    return z, z[active - 1]


def grand_product_fast(cols, num, den, n, active, start, omega, r):
    """The same result with one pow: prefix products of N, prefix products of
    D with zeros counted as 1, one inverse of the total, and zeros from the
    first zero denominator on."""
    m = active - 1
    N = list_rows(cols, num, m, omega, r)
    D = list_rows(cols, den, m, omega, r)
    first_zero = next((i for i, d in enumerate(D) if d == 0), m)
    pd = [1] * (m + 1)  # pd[i] = prod_{j < i} D'[j]
    for i in range(m):
        pd[i + 1] = pd[i] * (D[i] or 1) % r
    inv = pow(pd[m], r - 2, r)
    ipd = [0] * (m + 1)  # ipd[i] = 1 / pd[i]
    for i in range(m, -1, -1):
        ipd[i] = inv
        if i:
            inv = inv * (D[i - 1] or 1) % r
    z, pn = [], start % r
    for i in range(active):
        z.append(pn * ipd[i] % r if i <= first_zero else 0)
        if i < m:
            pn = pn * N[i] % r
    return z, z[active - 1]


def grand_products(cols, sets, n, active, start, omega, r, chain=False, fn=grand_product_literal):
    """S sets (numerators, denominators); chained, set j starts from set
    j - 1's last.  Returns ([z_j], [last_j])."""
    zs, lasts, cur = [], [], start
    for num, den in sets:
        z, last = fn(cols, num, den, n, active, cur if chain else start, omega, r)
        zs.append(z)
        lasts.append(last)
        cur = last
    return zs, lasts


def permutation_sets(columns, sigmas, chunk_len, beta, gamma, delta, r):
    """permutation/prover.rs::commit: `columns` and `sigmas` are column indices
    (sigma_k holds the labels delta^k' omega^i' of the cell that (k, i) maps
    to); one set per chunk of chunk_len columns, to be run chained from 1."""
    sets = []
    for c0 in range(0, len(columns), chunk_len):
        num, den = [], []
        for k in range(c0, min(c0 + chunk_len, len(columns))):
            den.append((columns[k], sigmas[k], beta, gamma))
            num.append((columns[k], OMEGA, beta * pow(delta, k, r) % r, gamma))
        sets.append((num, den))
    return sets


def lookup_set(a, s, a_perm, s_perm, beta, gamma):
    """lookup/prover.rs::commit_product over the compressed input / table
    columns a, s and their permuted forms a_perm, s_perm (column indices)."""
    return ([(a, None, 0, beta), (s, None, 0, gamma)], [(a_perm, None, 0, beta), (s_perm, None, 0, gamma)])


def root_of_unity(r, order):
    assert (r - 1) % order == 0
    for g in range(2, 100):
        w = pow(g, (r - 1) // order, r)
        if pow(w, order // 2, r) != 1:
            return w
    raise AssertionError("no generator found")


def permutation_instance(r, ncols, n, seed, fixed_rows=()):
    """A random genuine permutation over ncols x n cells: values constant along
    its cycles, sigma columns holding the labels delta^k omega^i of each cell's
    image.  Returns (cols, value column indices, sigma column indices, omega,
    delta); cells in fixed_rows map to themselves."""
    rng = random.Random(seed)
    omega, delta = root_of_unity(r, n), 7
    cells = [(k, i) for k in range(ncols) for i in range(n) if i not in fixed_rows]
    image = list(cells)
    rng.shuffle(image)
    sigma = {c: c for c in ((k, i) for k in range(ncols) for i in range(n))}
    sigma.update(zip(cells, image))
    label = {(k, i): pow(delta, k, r) * pow(omega, i, r) % r for k in range(ncols) for i in range(n)}
    assert len(set(label.values())) == ncols * n  # pairwise distinct
    value, seen = {}, set()
    for c in sigma:
        if c in seen:
            continue
        v, d = rng.randrange(r), c
        while d not in seen:
            seen.add(d)
            value[d] = v
            d = sigma[d]
    cols = [[value[(k, i)] for i in range(n)] for k in range(ncols)]
    cols += [[label[sigma[(k, i)]] for i in range(n)] for k in range(ncols)]
    return cols, list(range(ncols)), list(range(ncols, 2 * ncols)), omega, delta

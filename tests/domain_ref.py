"""Python big-int restatement of halo2's extended-domain conversions, the
reference of tests/test_domain_*.py.  halo2's crates are not vendored under
the reference (its Cargo.toml:10-12 names them as git dependencies), so, as
tests/poly_ref.py and tests/gp_ref.py do, the definitions are restated here
from halo2 `src/poly/domain.rs` [3P], `EvaluationDomain`:

  * `new(j, k)`: extended_k is the smallest with 2^extended_k >= n *
    quotient_poly_degree (n = 2^k); extended_omega has order 2^extended_k and
    omega = extended_omega^(2^(extended_k - k)); g_coset = ZETA, a primitive
    cube root of unity, g_coset_inv = ZETA^2; t_evaluations holds the
    2^(extended_k - k) distinct values of (X^n - 1)^-1 on the coset,
    t[i] = (ZETA^n (extended_omega^n)^i - 1)^-1;
  * `distribute_powers_zeta(a, into_coset)` [3P]: a[i] times 1, g, g^2 for
    i mod 3 = 0, 1, 2, with g = ZETA into the coset and ZETA^2 out of it;
  * `coeff_to_extended(a)` [3P]: distribute into the coset, resize to
    2^extended_k with zeros, best_fft(extended_omega, extended_k);
  * `divide_by_vanishing_poly(h)` [3P]: h[j] *= t[j mod len(t)];
  * `extended_to_coeff(h)` [3P]: best_fft(extended_omega_inv, extended_k),
    times extended_ifft_divisor = 2^-extended_k, distribute out of the coset,
    truncate to n * quotient_poly_degree.

Values are integers mod r.  Every function is linear in its data, so tests may
feed Montgomery-form words (a R mod r) with plain roots and get Montgomery-form
results."""
import ntt as N


def root_of_unity(r, order):
    """an element of exact order `order` (a power of two, or 3)"""
    assert (r - 1) % order == 0
    for g in range(2, 100):
        w = pow(g, (r - 1) // order, r)
        if order == 1 or all(pow(w, order // q, r) != 1 for q in (2, 3) if order % q == 0):
            return w
    raise AssertionError("no generator found")


def cube_roots(r):
    """the two primitive cube roots of unity (zeta, zeta^2)"""
    z = root_of_unity(r, 3)
    return z, z * z % r


def extended_k_for(k, quotient_poly_degree):
    """EvaluationDomain::new: the smallest extended_k with 2^extended_k >= n * degree"""
    ek = k
    while (1 << ek) < (quotient_poly_degree << k):
        ek += 1
    return ek


class Domain:
    def __init__(self, r, k, extended_k, extended_omega=None, zeta=None):
        assert extended_k >= k >= 0
        self.r, self.k, self.extended_k = r, k, extended_k
        self.n, self.N, self.e = 1 << k, 1 << extended_k, extended_k - k
        self.extended_omega = root_of_unity(r, self.N) if extended_omega is None else extended_omega
        self.zeta = cube_roots(r)[0] if zeta is None else zeta
        assert self.zeta != 1 and pow(self.zeta, 3, r) == 1
        self.omega = pow(self.extended_omega, 1 << self.e, r)
        self.extended_omega_inv = pow(self.extended_omega, -1, r)
        self.g_coset, self.g_coset_inv = self.zeta, self.zeta * self.zeta % r
        self.extended_ifft_divisor = pow(self.N, -1, r)
        # t_evaluations [3P]: cur starts at ZETA^n and steps by extended_omega^n
        cur, step = pow(self.zeta, self.n, r), pow(self.extended_omega, self.n, r)
        self.t_evaluations = []
        for _ in range(1 << self.e):
            assert cur != 1
            self.t_evaluations.append(pow(cur - 1, -1, r))
            cur = cur * step % r

    def distribute_powers_zeta(self, a, into_coset):
        g = self.g_coset if into_coset else self.g_coset_inv
        mul = (1, g, g * g % self.r)
        return [v * mul[i % 3] % self.r for i, v in enumerate(a)]

    def coeff_to_extended(self, a):
        """|a| = n in halo2; up to N coefficients are taken here (the tests'
        products of degree >= n)"""
        assert len(a) <= self.N
        ext = self.distribute_powers_zeta(a, True) + [0] * (self.N - len(a))
        return N.serial_fft(ext, self.extended_omega, self.extended_k, self.r)

    def divide_by_vanishing_poly(self, h):
        assert len(h) == self.N
        t = self.t_evaluations
        return [v * t[j % len(t)] % self.r for j, v in enumerate(h)]

    def extended_to_coeff(self, h, keep=None):
        assert len(h) == self.N
        a = N.serial_fft(list(h), self.extended_omega_inv, self.extended_k, self.r)
        a = [v * self.extended_ifft_divisor % self.r for v in a]
        a = self.distribute_powers_zeta(a, False)
        return a[:self.N if keep is None else keep]

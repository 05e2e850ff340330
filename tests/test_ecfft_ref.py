"""tests/ecfft_ref.py (best_fft's loop over pasta.Curve points) against pin 1:
with in[j] = [a_j]G the outputs are [scale NTT(a)_k]G, the scalar transform
from oracle/ntt.py and the points from pasta.Curve.  log_n = 0 .. 6, three
curves; no GPU, no library."""
import pytest

import ecfft_ref as E
import ntt
import pasta as P


@pytest.mark.parametrize("curve", [0, 1, 2])
def test_roots_have_exact_order(curve):
    r = P.CURVES[curve].r
    for log_n in range(0, 12):
        w = E.root_of_unity(curve, log_n)
        assert pow(w, 1 << log_n, r) == 1
        assert log_n == 0 or pow(w, 1 << (log_n - 1), r) == r - 1


@pytest.mark.parametrize("curve", [0, 1, 2])
@pytest.mark.parametrize("log_n", range(0, 7))
def test_ref_matches_known_dlogs(curve, log_n):
    C = P.CURVES[curve]
    n = 1 << log_n
    a = [P.synth_base_dlog(C, P.SEED_BASES, 100 * log_n + i) for i in range(n)]
    if n >= 4:
        a[1] = 0            # an identity input
        a[3] = a[2]         # equal inputs
    pts = [C.mul(x, C.gen) for x in a]
    omega = E.root_of_unity(curve, log_n)
    scale = None if log_n % 2 else pow(n, -1, C.r)
    if log_n % 2 == 0:
        omega = pow(omega, -1, C.r)   # the inverse transform on even sizes
    got = E.fft_points(curve, pts, omega, log_n, scale)
    want = [C.mul(e, C.gen) for e in E.expected_dlogs(curve, a, omega, log_n, scale)]
    assert got == want


def test_ref_matches_the_definition():
    """The O(n^2) sum itself at n = 8 on BN254."""
    C = P.BN254
    a = [P.synth_base_dlog(C, P.SEED_BASES, i) for i in range(8)]
    pts = [C.mul(x, C.gen) for x in a]
    omega = E.root_of_unity(2, 3)
    got = E.fft_points(2, pts, omega, 3)
    for k in range(8):
        acc = None
        for j in range(8):
            acc = C.add(acc, C.mul(pow(omega, j * k, C.r), pts[j]))
        assert got[k] == acc
    assert got == [C.mul(e, C.gen) for e in ntt.dft(a, omega, C.r)]

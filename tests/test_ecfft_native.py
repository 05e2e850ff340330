"""The point transform's host form (ecfft_host.hpp) under g++ ASan + UBSan:
tests/native/ecfft_host_check.cpp, a stand-alone host program with its own main
(identity inputs, all-equal inputs, a single non-identity input, forward-then-
inverse round trips, a refused root; log_n = 0 .. 6, three curves, 1 and 3
threads), built by ``make -C halo2-aggregation_amd ecfft_asan`` and run there.
No GPU and no HIP library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "halo2-aggregation_amd")


def test_host_point_transform_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", PKG, "ecfft_asan"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-3000:]
    assert "ecfft_host_check: all checks passed" in r.stdout, out[-2000:]

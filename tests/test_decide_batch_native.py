"""The batch decider's host code (pairing_batch_plan.hpp, pairing_batch_host.hpp:
the coefficient derivation, the 128-bit recoding, the Horner tail and the host
fold): tests/native/decide_batch_host.cpp, a stand-alone host program with its
own main that recomputes what it checks naively, built with g++ ASan + UBSan by
``make -C halo2-aggregation_amd decide_batch_asan`` and run there.  No GPU and
no HIP library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "halo2-aggregation_amd")


def test_coefficients_recoding_horner_and_fold():
    r = subprocess.run(["make", "-s", "-C", PKG, "decide_batch_asan"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-3000:]
    assert "decide_batch_host: all checks passed" in r.stdout, out[-2000:]

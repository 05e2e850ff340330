"""The pairing decider's host code (pairing_host.hpp, pairing_plan.hpp: the Fp2 /
Fp12 tower, the G2 checks and line tables, the program on a dozen quads):
tests/native/pairing_host.cpp, a stand-alone host program with its own main that
recomputes what it checks naively, built with g++ ASan + UBSan by ``make -C
halo2-aggregation_amd pairing_asan`` and run there.  No GPU and no HIP library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "halo2-aggregation_amd")


def test_host_tower_tables_and_decider():
    r = subprocess.run(["make", "-s", "-C", PKG, "pairing_asan"], capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-3000:]
    assert "pairing_host: all checks passed" in r.stdout, out[-2000:]

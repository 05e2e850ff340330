"""Ownership of the device buffers (pm::Buf in runtime.hpp and the handles that
hold one): tests/native/buf_own.cpp, a stand-alone host program over a counting
hipMalloc / hipFree shim, built with g++ ASan + UBSan by ``make -C
halo2-aggregation_amd buf_own`` and run there.  No GPU and no HIP library:
move construction, move assignment onto a live buffer, growth, a reallocating
vector of twiddle slots and destruction must leave no allocation live and free
none twice."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "halo2-aggregation_amd")


def test_buffers_free_themselves_once():
    r = subprocess.run(["make", "-s", "-C", PKG, "buf_own"], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error:" not in out, out[-3000:]
    assert "buf_own: all checks passed" in r.stdout, out[-2000:]

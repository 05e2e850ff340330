"""CPU: csrc/quotient_plan.hpp (the compiler of the quotient numerator's
program) built for the host with g++ under the address and undefined-behaviour
sanitizers, and every program it emits for a few shapes walked by
tests/native/quotient_plan_check.cpp: indices in range, no slot read before it
is written, consistent Montgomery forms, counters equal to the ops."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "quotient_plan_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("quot") / "quotient_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", out, SRC], check=True)
    return out


def test_programs_are_well_formed(exe):
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.split("\n")[:-1]
    assert lines[-1] == "ok" and len(lines) == 6, res.stdout
    assert [ln.split(":")[0] for ln in lines[:-1]] == ["simple", "rich", "depth16_sums", "depth16_products",
                                                      "empty_lookup_lists"]

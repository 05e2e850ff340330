"""tests/native/plan_dump.cpp from Python: the host plans of the MSM and
accumulator drivers and of the pairing decider (csrc/msm_plan.hpp,
csrc/accum_plan.hpp, csrc/pairing_plan.hpp) asked of the compiled code
instead of read from its text.  build() compiles the program once per process with g++ (no HIP, no GPU); ask() sends queries and returns
one dict of fields per query."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_dump.cpp")
_EXE = {}


def build(tmp_path_factory):
    if "exe" not in _EXE:
        out = str(tmp_path_factory.mktemp("plan") / "plan_dump")
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", out, SRC], check=True)
        _EXE["exe"] = out
    return _EXE["exe"]


LISTS = ("pstart", "termsrc", "qprog", "pairs", "prog", "doubles", "frob")   # always lists, whatever their length


def _field(k, v):
    if k in LISTS:
        return [int(x) for x in v.split(",") if x]
    return int(v) if v.isdigit() else v


def ask(exe, queries):
    """queries: strings (see plan_dump.cpp) -> [dict of fields] in order."""
    queries = list(queries)
    r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-500:]
    rows = r.stdout.split("\n")[:-1]
    assert len(rows) == len(queries)
    return [{k: _field(k, v) for k, v in (f.split("=", 1) for f in row.split())} for row in rows]


def ask1(exe, query):
    return ask(exe, [query])[0]

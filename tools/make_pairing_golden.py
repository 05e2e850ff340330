#!/usr/bin/env python3
"""Writes tests/golden/pairing_bn254.json from tests/pairing_ref.py: e(G1, G2) and
three more pairings e([a]G1, [b]G2), each as the 12 Fp coefficients (hex,
canonical, tower order c0.c0.c0 .. c1.c2.c1).  tests/test_pairing_ref.py pins
pairing_ref by properties and compares it with this file."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairing_ref as PR  # noqa: E402

CASES = [(1, 1), (55555, 1), (777, 0x1234567890ABCDEF1234567890ABCDEF), (PR.R - 1, 999)]


def main():
    out = {"comment": "tools/make_pairing_golden.py: e([a]G1, [b]G2), coefficients c0.c0.c0 .. c1.c2.c1, canonical",
           "cases": []}
    for a, b in CASES:
        gt = PR.pairing(PR.g1_mul(a, PR.G1), PR.g2_mul(b, PR.G2))
        out["cases"].append({"a": hex(a), "b": hex(b), "gt": [hex(c) for c in PR.f12_flat(gt)]})
    path = os.path.join(ROOT, "tests", "golden", "pairing_bn254.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()

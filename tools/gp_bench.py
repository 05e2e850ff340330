"""Timing of the grand products (pm_grand_product_device) and the batch
inversion (pm_batch_invert_device) against the NTT of the same length and
field in the same process: BN254, device-resident columns.

Before any time is recorded every grand-product case is checked by the sampled
identity z[i+1] D[i] == z[i] N[i] (256 rows, the first and the last among
them, columns read back and N, D recomputed with Python integers), and the
inversion by a[i] a[i]^-1 == 1 on the same rows.

Timing as tools/poly_bench.py: every case is a synchronous library call, timed
with the host clock; all cases are warmed first, then ROUNDS rounds visit the
cases in turn, each round timing enough back-to-back calls to fill ~50 ms
(at least 3, so at least 21 timed calls per case).  The figure is the median
round.  Per-kernel times come from a separate pass with the context's event
timing on.

For the permutation chunk the HBM floor is recorded: (columns read + rows
written + the scratch rows written and read back) x 32 B x n over the 6.29 TB/s
a float4 copy measures on this part, and the kernels' share of it.

Writes profiles/gp/gp_bench.jsonl (one line per case, then the ratios)."""
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "halo2-aggregation_amd"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import halo2_amd as H  # noqa: E402
import workloads as Wk  # noqa: E402

CURVE = H.BN254
ROUNDS = int(os.environ.get("GP_BENCH_ROUNDS", "7"))
WINDOW_S = 0.05
HBM_BYTES_PER_S = 6.29e12
GP_KERNELS = ["poly_table", "gp_prep", "gp_local", "gp_carry", "gp_chain", "gp_sweep"]
NTT_KERNELS = ["ntt_cols", "ntt_mid", "ntt_rows"]
R_MONT = 1 << 256


def mont(r, v):
    v = v * R_MONT % r
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def rows_as_ints(t, idx, r):
    """plain integers of the rows idx of a device tensor of Montgomery scalars"""
    a = t[torch.as_tensor(idx, device=t.device)].cpu().numpy().view(np.uint64)
    rinv = pow(R_MONT, -1, r)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) * rinv % r for row in a]


def main():
    out_path = os.path.join(ROOT, "profiles", "gp", "gp_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("gp_bench needs a GPU")
    ctx = H.Context(0)
    r = H.SCALAR_MODULUS[CURVE]
    dev = torch.device("cuda", 0)
    beta, gamma, delta = 0x1234567, 0xABCDEF, 7

    def columns(k, count, seed):
        ts = [torch.empty((1 << k, 4), dtype=torch.int64, device=dev) for _ in range(count)]
        for i, t in enumerate(ts):
            ctx.synth_scalars(CURVE, seed + i, 0, 1 << k, t.data_ptr())
        return ts

    def perm_set():  # columns 0..2 values, 3..5 sigma
        num = [(k, H.GP_OMEGA, beta * pow(delta, k, r) % r, gamma) for k in range(3)]
        den = [(k, 3 + k, beta, gamma) for k in range(3)]
        return num, den

    def lookup_set():  # A, S, A', S'
        return [(0, None, 0, beta), (1, None, 0, gamma)], [(2, None, 0, beta), (3, None, 0, gamma)]

    def to_args(factors):
        return [(x, y, mont(r, b), mont(r, g)) for x, y, b, g in factors]

    def factor(f, vals, i, omega):
        x, y, b, g = f
        v = g + (vals[x] if x is not None else 0)
        if y == H.GP_OMEGA:
            v += b * pow(omega, i, r)
        elif y is not None:
            v += b * vals[y]
        return v % r

    def check_identity(cols, k, sets, omega, out):
        n = 1 << k
        rng = random.Random(k)
        idx = sorted({0, n - 2} | {rng.randrange(n - 1) for _ in range(254)})
        vals = [rows_as_ints(c, idx, r) for c in cols]
        z0, z1 = rows_as_ints(out, idx, r), rows_as_ints(out, [i + 1 for i in idx], r)
        num, den = sets
        for t, i in enumerate(idx):
            row = [v[t] for v in vals]
            N = D = 1
            for f in num:
                N = N * factor(f, row, i, omega) % r
            for f in den:
                D = D * factor(f, row, i, omega) % r
            assert D and z1[t] * D % r == z0[t] * N % r, ("identity", k, i)
        assert rows_as_ints(out, [0], r) == [1]

    def gp_case(cols, k, sets, omega, out):
        ptrs = [c.data_ptr() for c in cols]
        args = [(to_args(sets[0]), to_args(sets[1]))]
        w, one = mont(r, omega), mont(r, 1)
        fn = lambda: ctx.grand_product_device(CURVE, ptrs, 1 << k, args, w, one, 1 << k, out.data_ptr(),  # noqa: E731
                                              want_last=False)
        fn()
        check_identity(cols, k, sets, omega, out)
        return fn

    def invert_case(k, seed):
        src = columns(k, 1, seed)[0]
        work = src.clone()
        ctx.batch_invert_device(CURVE, work.data_ptr(), 1 << k)
        rng = random.Random(seed)
        idx = [0, (1 << k) - 1] + [rng.randrange(1 << k) for _ in range(254)]
        for a, b in zip(rows_as_ints(src, idx, r), rows_as_ints(work, idx, r)):
            assert a * b % r == 1, ("inverse", k)
        # inverting back and forth keeps the values generic
        return lambda: ctx.batch_invert_device(CURVE, work.data_ptr(), 1 << k)

    cases = []
    keep = []
    for k in (20, 23):
        omega = Wk.domain_omega(CURVE, k)
        cols = columns(k, 6, 0x100 * k)
        out = torch.empty((1 << k, 4), dtype=torch.int64, device=dev)
        fft = columns(k, 1, 0x100 * k + 0x40)[0]
        keep += [cols, out, fft]
        w = mont(r, omega)
        cases += [
            (f"fft_2^{k}", k, NTT_KERNELS,
             lambda fft=fft, k=k, w=w: ctx.fft_device(CURVE, fft.data_ptr(), k, w)),
            (f"batch_invert_2^{k}", k, GP_KERNELS, invert_case(k, 0x100 * k + 0x50)),
            (f"perm_chunk3_2^{k}", k, GP_KERNELS, gp_case(cols, k, perm_set(), omega, out)),
            (f"lookup_2^{k}", k, GP_KERNELS, gp_case(cols[:4], k, lookup_set(), omega, out)),
        ]
    torch.cuda.synchronize()

    reps = {}
    for name, _, _, fn in cases:  # warm-up, and the calls per window
        fn()
        fn()
        t = time.perf_counter()
        fn()
        reps[name] = max(3, int(WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    samples = {name: [] for name, _, _, _ in cases}
    for _ in range(ROUNDS):
        for name, _, _, fn in cases:
            t = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            samples[name].append((time.perf_counter() - t) / reps[name] * 1e3)
    kernels = {}
    ctx.set_timing(True)
    for name, _, names, fn in cases:
        ctx.reset_stats()
        for _ in range(5):
            fn()
        kernels[name] = {k: round(ctx.kernel_stats(k)[1] / 5, 4) for k in names if ctx.kernel_stats(k)[0]}
    ctx.set_timing(False)
    med = {name: statistics.median(s) for name, s in samples.items()}
    with open(out_path, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")

        for name, k, _, _ in cases:
            s = samples[name]
            rec = {"case": name, "curve": "bn254", "log_n": k, "calls_per_round": reps[name], "rounds": ROUNDS,
                   "wall_ms": round(med[name], 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4),
                   "kernels_ms": kernels[name], "kernels_sum_ms": round(sum(kernels[name].values()), 4)}
            if name.startswith("perm_chunk3"):
                # gp_local reads 6 columns for the denominators and 3 again for the numerators and
                # writes the PN and SD rows, gp_sweep reads both back and writes the z row
                rows = 9 + 2 + 2 + 1
                floor_ms = rows * 32 * (1 << k) / HBM_BYTES_PER_S * 1e3
                rec["hbm_rows_of_n"] = rows
                rec["hbm_floor_ms"] = round(floor_ms, 4)
                rec["floor_over_kernels"] = round(floor_ms / sum(kernels[name].values()), 4)
                # what no scheme can go below: every column once, the z row once
                rec["hbm_floor_ideal_ms"] = round(7 * 32 * (1 << k) / HBM_BYTES_PER_S * 1e3, 4)
            emit(rec)
        emit({"ratios_to_fft_same_length": {
            name: round(med[name] / med[f"fft_2^{k}"], 3) for name, k, _, _ in cases if not name.startswith("fft")},
            "targets": {"perm_chunk3_2^20": 2.0}})


if __name__ == "__main__":
    main()

"""Timing of the lookup argument's permuted columns (pm_lookup_permute_device,
pm_lookup_compress_device) against the NTT of the same length and field in the
same process: BN254, device-resident columns, n = usable.

Three key distributions, the extremes a prover meets: `distinct` (uniform
254-bit values, all different, the table a shuffle of the input), `range16`
(a 16-bit range table, uniform inputs: equal high words, massive duplicates)
and `equal` (one value everywhere).

Before any time is recorded every case is checked on its own output: A' is
ascending (the canonical values recomputed with Python integers: every row up
to 2^20, above that 64 windows of 4096 rows with the first and the last rows
among them), on every row A'[i] == S'[i] or A'[i] == A'[i-1], the status is ok,
and A' / S' have the field sums of A / S (a permutation keeps the sum; the
Montgomery form is linear, so the stored words are summed).

Timing as tools/gp_bench.py: every case is a synchronous library call, timed
with the host clock; all cases are warmed first, then ROUNDS rounds visit the
cases in turn, each round timing enough back-to-back calls to fill ~50 ms (at
least 3).  The figure is the median round, with min and max.  Per-kernel times
come from a separate pass with the context's event timing on.

The HBM floor of the call's own pass count is recorded: per column one tile
sort and ceil(log2(usable / tile)) merge passes of 64 B per key, and per pair
the pairing's 256 B per row (flags read 64, rows read 32 and write 64, scatter
reads 32 + 1 and writes up to 32, the row map 4 + 4 and the flag byte aside),
over the 6.29 TB/s a float4 copy measures on this part.

Writes profiles/lookup/lookup_bench.jsonl (one line per case, then the ratios)."""
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
ROUNDS = int(os.environ.get("LOOKUP_BENCH_ROUNDS", "7"))
WINDOW_S = 0.05
HBM_BYTES_PER_S = 6.29e12
LK_KERNELS = ["lk_tile_sort", "lk_merge", "lk_flags", "lk_carry", "lk_rows", "lk_scatter", "lk_compress"]
NTT_KERNELS = ["ntt_cols", "ntt_mid", "ntt_rows"]
R_MONT = 1 << 256
DISTRIBUTIONS = ("distinct", "range16", "equal")


def mont_rows(r, vals):
    b = b"".join((v * R_MONT % r).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype="<u8").reshape(len(vals), 4)


def stored_ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def field_sum(t, r):
    """sum of the stored 256-bit words of a device column, mod r"""
    a = t.cpu().numpy().view(np.uint32).astype(np.uint64)  # (n, 8) words, each column sum < 2^60
    return sum(int(c) << (32 * k) for k, c in enumerate(a.sum(axis=0))) % r


def main():
    out_path = os.path.join(ROOT, "profiles", "lookup", "lookup_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("lookup_bench needs a GPU")
    ctx = H.Context(0)
    r = H.SCALAR_MODULUS[CURVE]
    rinv = pow(R_MONT, -1, r)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0x10C)
    range_tab = torch.from_numpy(mont_rows(r, range(1 << 16)).view(np.int64).copy()).to(dev)

    def synth(n, seed):
        t = torch.empty((n, 4), dtype=torch.int64, device=dev)
        ctx.synth_scalars(CURVE, seed, 0, n, t.data_ptr())
        return t

    def pair(dist, n, seed):
        """(A, S): the compressed input and table columns of one lookup"""
        if dist == "distinct":
            s = synth(n, seed)
            return s[torch.randperm(n, device=dev, generator=gen)].contiguous(), s
        if dist == "range16":
            s = range_tab[torch.arange(n, device=dev) & 0xFFFF].contiguous()
            return range_tab[torch.randint(0, 1 << 16, (n,), device=dev, generator=gen)].contiguous(), s
        one = range_tab[7:8].expand(n, 4)
        return one.contiguous(), one.contiguous()

    def check(a, s, oa, os_, status, n):
        assert tuple(status) == (0, 0), ("status", tuple(status))
        ha, hs = oa.cpu().numpy().view(np.uint64), os_.cpu().numpy().view(np.uint64)
        first = (ha == hs).all(axis=1)
        repeated = np.concatenate([[False], (ha[1:] == ha[:-1]).all(axis=1)])
        assert (first | repeated).all(), "pairing property"
        assert field_sum(oa, r) == field_sum(a, r) and field_sum(os_, r) == field_sum(s, r), "multiset sum"
        if n <= 1 << 20:
            windows = [(0, n)]
        else:
            rng = random.Random(n)
            starts = [0, n - 4096] + [rng.randrange(n - 4096) for _ in range(62)]
            windows = [(lo, lo + 4096) for lo in starts]
        rows = 0
        for lo, hi in windows:
            v = [x * rinv % r for x in stored_ints(ha[lo:hi])]
            assert all(v[i] <= v[i + 1] for i in range(len(v) - 1)), ("sorted", lo)
            rows += hi - lo
        return rows

    cases, keep, meta = [], [], {}
    for k, P in ((20, 1), (23, 1), (20, 4)):
        n = 1 << k
        for dist in DISTRIBUTIONS:
            pairs = [pair(dist, n, 0x1000 * k + 0x10 * p + 1) for p in range(P)]
            outs = [(torch.empty_like(a), torch.empty_like(s)) for a, s in pairs]
            keep += [pairs, outs]
            args = ([a.data_ptr() for a, _ in pairs], [s.data_ptr() for _, s in pairs], n, n,
                    [o.data_ptr() for o, _ in outs], [o.data_ptr() for _, o in outs])
            fn = lambda args=args: ctx.lookup_permute_device(CURVE, *args)  # noqa: E731
            status = fn()
            checked = [check(a, s, oa, os_, status[p], n) for p, ((a, s), (oa, os_)) in enumerate(zip(pairs, outs))]
            name = f"permute_{dist}_2^{k}_P{P}"
            cases.append((name, k, LK_KERNELS, fn))
            meta[name] = {"pairs": P, "distribution": dist, "rows_checked_sorted": checked[0]}
    for k in (20, 23):
        n = 1 << k
        cols = [synth(n, 0x2000 * k + i) for i in range(3)]
        out = torch.empty_like(cols[0])
        fft = synth(n, 0x2000 * k + 0x40)
        keep += [cols, out, fft]
        theta = mont_rows(r, [0x1234567])[0].astype(np.uint64)
        w = mont_rows(r, [Wk.domain_omega(CURVE, k)])[0].astype(np.uint64)
        ptrs = [c.data_ptr() for c in cols]
        cases += [
            (f"fft_2^{k}", k, NTT_KERNELS, lambda fft=fft, k=k, w=w: ctx.fft_device(CURVE, fft.data_ptr(), k, w)),
            (f"compress_m3_2^{k}", k, LK_KERNELS,
             lambda ptrs=ptrs, n=n, theta=theta, out=out: ctx.lookup_compress_device(CURVE, ptrs, n, theta, out.data_ptr())),
        ]
        meta[f"fft_2^{k}"] = {}
        meta[f"compress_m3_2^{k}"] = {"columns": 3}
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
            rec.update(meta[name])
            if name.startswith("permute"):
                n, P = 1 << k, meta[name]["pairs"]
                sort_passes = 1 + max(0, k - (H.LOOKUP_TILE.bit_length() - 1))
                sort_ms = P * 2 * sort_passes * 64 * n / HBM_BYTES_PER_S * 1e3
                pair_ms = P * 256 * n / HBM_BYTES_PER_S * 1e3
                rec["sort_passes_per_column"] = sort_passes
                rec["hbm_floor_sort_ms"] = round(sort_ms, 4)
                rec["hbm_floor_ms"] = round(sort_ms + pair_ms, 4)
                rec["floor_over_kernels"] = round((sort_ms + pair_ms) / sum(kernels[name].values()), 4)
            elif name.startswith("compress"):
                rec["hbm_floor_ms"] = round(4 * 32 * (1 << k) / HBM_BYTES_PER_S * 1e3, 4)
            emit(rec)
        emit({"ratios_to_fft_same_length": {
            name: round(med[name] / med[f"fft_2^{k}"], 3) for name, k, _, _ in cases if not name.startswith("fft")}})


if __name__ == "__main__":
    main()

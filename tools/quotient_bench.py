"""Timing of the quotient numerator (pm_quotient_device, k_quot_eval) against
pm_fft_device at the extended length in the same process: BN254,
device-resident columns of uniform scalars.

Cases: the simple-example shape at k = 17 and k = 20 and the oracle's rich
shape at k = 17, all with e = 2, each with repeated leaves resident (the
default, when the program fits PM_QUOT_CACHE_SLOTS = 8 slots), with every use
loading (0) and with residency up to the kernel's slot budget (28).

Before any time is recorded every case is checked on the device: the call with
PM_QUOT_DIVIDE_VANISHING equals the plain call followed by
pm_divide_by_vanishing_device, and the variants of one shape agree.

Timing as tools/domain_bench.py: every case is a synchronous library call,
timed with the host clock; all cases are warmed first, then ROUNDS rounds visit
the cases in turn, each round timing enough back-to-back calls to fill ~50 ms
(at least 3).  The figure is the median round, with the rounds' min and max.
The kernel's own time comes from a separate pass with event timing on.

Models written with each record: the HBM floor, (loads_per_row + 1) rows of
N x 32 B at 6.29 TB/s, and the product model, products_per_row against the
NTT's ~10 products per element, scaled from the measured pm_fft_device.

Writes profiles/quotient/quotient_bench.jsonl."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "halo2-aggregation_amd"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import accum as A  # noqa: E402
import halo2_amd as H  # noqa: E402
import pasta as P  # noqa: E402
import workloads as Wk  # noqa: E402

CURVE = H.BN254
ROUNDS = int(os.environ.get("QUOTIENT_BENCH_ROUNDS", "7"))
WINDOW_S = 0.05
HBM_BYTES_PER_S = 6.29e12
NTT_PRODUCTS_PER_ELEMENT = 10
R_MONT = 1 << 256
VARIANTS = (("", None), ("_reload", "0"), ("_resident28", "28"))


def mont(r, v):
    v = v * R_MONT % r
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def shape_for(name, k):
    """simple: the product's workload shape; rich: the oracle's second shape.
    The quotient reads no VK commitment, so they are zeros."""
    if name == "simple":
        args = Wk.simple_example_args(CURVE, k)
    else:
        sh = A.rich_shape(P.CURVES[CURVE], k)
        args = dict(log_n=k, blinding_factors=sh.blinding_factors, num_instance_columns=sh.num_instance_columns,
                    num_advice_columns=sh.num_advice_columns, num_fixed_columns=sh.num_fixed_columns,
                    num_lookups=sh.num_lookups, perm_chunk_len=sh.perm_chunk_len, quotient_degree=sh.quotient_degree,
                    instance_queries=sh.instance_queries, advice_queries=sh.advice_queries,
                    fixed_queries=sh.fixed_queries, perm_columns=sh.perm_columns, gates=sh.gates,
                    lookup_inputs=sh.lookup_inputs, lookup_tables=sh.lookup_tables, omega=Wk.domain_omega(CURVE, k),
                    delta=Wk.field_delta(CURVE))
    return H.ProofShape(CURVE, g1=Wk.generator_limbs(CURVE),
                        fixed_commitments=np.zeros((args["num_fixed_columns"], 8), dtype=np.uint64),
                        sigma_commitments=np.zeros((len(args["perm_columns"]), 8), dtype=np.uint64), **args)


def main():
    out_path = os.path.join(ROOT, "profiles", "quotient", "quotient_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("quotient_bench needs a GPU")
    ctx = H.Context(0)
    r = H.SCALAR_MODULUS[CURVE]
    dev = torch.device("cuda", 0)
    zeta = next(z for z in (pow(g, (r - 1) // 3, r) for g in range(2, 50)) if z != 1)

    def column(rows, seed):
        t = torch.empty((rows, 4), dtype=torch.int64, device=dev)
        ctx.synth_scalars(CURVE, seed, 0, rows, t.data_ptr())
        return t

    cases, keep_alive, meta = [], [], {}

    def size(name, k, e):
        ek, N = k + e, 1 << (k + e)
        we = Wk.domain_omega(CURVE, ek)
        dom = ctx.domain(CURVE, k, ek, mont(r, we), mont(r, zeta))
        shape = shape_for(name, k)
        counts = H.quotient_column_counts(shape)
        cols = {g: [column(N, 0x10000 * ek + 0x100 * i + c) for c in range(n)] for i, (g, n) in enumerate(counts.items())}
        ptrs = {g: [t.data_ptr() for t in ts] for g, ts in cols.items()}
        ch = np.stack([mont(r, 0xC0FFEE + 7 * i) for i in range(4)])
        out = torch.empty((N, 4), dtype=torch.int64, device=dev)
        fft = column(N, 0x7F7 + ek)
        w = mont(r, we)
        tag = f"{name}_{k}->{ek}"
        first = None
        for suffix, slots in VARIANTS:
            if slots is None:
                os.environ.pop("PM_QUOT_CACHE_SLOTS", None)
            else:
                os.environ["PM_QUOT_CACHE_SLOTS"] = slots
            q = ctx.quotient(dom, shape)
            os.environ.pop("PM_QUOT_CACHE_SLOTS", None)
            info = q.info()
            # checks: the fused division against the two calls; the variants against each other
            plain = torch.empty((N, 4), dtype=torch.int64, device=dev)
            ctx.quotient_device(q, ptrs, ch, plain.data_ptr())
            ctx.quotient_device(q, ptrs, ch, out.data_ptr(), divide_vanishing=True)
            torch.cuda.synchronize()
            if first is None:
                first = plain.clone()
            assert torch.equal(plain, first), ("variants disagree", tag, suffix)
            ctx.divide_by_vanishing_device(dom, [plain.data_ptr()])
            torch.cuda.synchronize()
            assert torch.equal(plain, out), ("fused division", tag, suffix)
            del plain
            cases.append((f"quotient_{tag}{suffix}", tag,
                          lambda q=q: ctx.quotient_device(q, ptrs, ch, out.data_ptr(), divide_vanishing=True)))
            meta[f"quotient_{tag}{suffix}"] = dict(info, log_N=ek, shape=name, resident=slots or "8")
            keep_alive.append(q)
        cases.append((f"fft_{tag}", tag, lambda: ctx.fft_device(CURVE, fft.data_ptr(), ek, w)))
        meta[f"fft_{tag}"] = dict(log_N=ek)
        keep_alive.extend([dom, shape, cols, out, fft])

    size("simple", 17, 2)
    size("rich", 17, 2)
    size("simple", 20, 2)
    torch.cuda.synchronize()

    reps = {}
    for name, _, fn in cases:  # warm-up, and the calls per window
        fn()
        fn()
        t = time.perf_counter()
        fn()
        reps[name] = max(3, int(WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    samples = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, _, fn in cases:
            t = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            samples[name].append((time.perf_counter() - t) / reps[name] * 1e3)
    kernel_ms = {}
    ctx.set_timing(True)
    for name, _, fn in cases:
        if not name.startswith("quotient"):
            continue
        ctx.reset_stats()
        for _ in range(5):
            fn()
        kernel_ms[name] = round(ctx.kernel_stats("quot_eval")[1] / 5, 4)
    ctx.set_timing(False)
    med = {name: statistics.median(s) for name, s in samples.items()}
    with open(out_path, "w") as f:
        for name, tag, _ in cases:
            s = samples[name]
            rec = {"case": name, "curve": "bn254", "calls_per_round": reps[name], "rounds": ROUNDS,
                   "wall_ms": round(med[name], 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4)}
            rec.update(meta[name])
            if name in kernel_ms:
                N = 1 << rec["log_N"]
                fft_ms = med[f"fft_{tag}"]
                # + 1 product for the t[j mod 2^e] factor of the timed call
                products = rec["products_per_row"] + 1
                rec.update(kernel_ms=kernel_ms[name], fft_ms=round(fft_ms, 4), over_fft=round(med[name] / fft_ms, 3),
                           hbm_floor_ms=round((rec["loads_per_row"] + 1) * N * 32 / HBM_BYTES_PER_S * 1e3, 4),
                           product_model_ms=round(fft_ms * products / NTT_PRODUCTS_PER_ELEMENT, 4))
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Timing of the polynomial openings (pm_multiopen_witness_device,
pm_poly_eval_device, pm_multiopen_open_device) against the NTT of the same
length and field in the same process: BN254, device-resident inputs.

Every case is a synchronous library call (it returns after a stream
synchronise), timed with the host clock.  All cases are warmed first; then
ROUNDS rounds visit the cases in turn (so drift and other tenants hit every
case alike), each round timing enough back-to-back calls to fill ~50 ms.  The
figure is the median round, the spread its min / max.  Per-kernel times come
from a separate pass with the context's event timing on (events lengthen the
stream, so that pass feeds no wall figure).

Writes profiles/poly/poly_bench.jsonl (one line per case, then the ratios)."""
import json
import os
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
ROUNDS = int(os.environ.get("POLY_BENCH_ROUNDS", "7"))
WINDOW_S = 0.05
POLY_KERNELS = ["poly_table", "poly_div_local", "poly_div_carry", "poly_div_sweep", "poly_eval_part",
                "poly_eval_comb"]
NTT_KERNELS = ["ntt_cols", "ntt_mid", "ntt_rows"]
MSM_KERNELS = ["bases_r261", "sort_hist", "scan", "sort_coarse", "sort_fine", "accumulate", "fixup", "bucket_seg",
               "bucket_bits", "bits_combine", "host_tail", "small_fused", "small_table", "small_sum"]


def mont(r, v):
    v = v * (1 << 256) % r
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def main():
    out_path = os.path.join(ROOT, "profiles", "poly", "poly_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("poly_bench needs a GPU")
    ctx = H.Context(0)
    r = H.SCALAR_MODULUS[CURVE]
    dev = torch.device("cuda", 0)

    def polys(k, count, seed):
        ts = [torch.empty((1 << k, 4), dtype=torch.int64, device=dev) for _ in range(count)]
        for i, t in enumerate(ts):
            ctx.synth_scalars(CURVE, seed + i, 0, 1 << k, t.data_ptr())
        return ts

    p20 = polys(20, 24, 0x100)
    ptr20 = [t.data_ptr() for t in p20]
    out20 = torch.empty((4 << 20, 4), dtype=torch.int64, device=dev)
    fft20 = polys(20, 1, 0x200)[0]
    p23 = polys(23, 4, 0x300)
    ptr23 = [t.data_ptr() for t in p23]
    out23 = torch.empty((1 << 23, 4), dtype=torch.int64, device=dev)
    fft23 = polys(23, 1, 0x400)[0]
    bases = torch.empty((1 << 20, 8), dtype=torch.int64, device=dev)
    ctx.synth_bases(CURVE, 0xA11CE, 0, 1 << 20, bases.data_ptr())
    torch.cuda.synchronize()
    srs = ctx.upload_bases(CURVE, d_bases=bases.data_ptr(), n=1 << 20)
    z = [mont(r, 0x1234567 + 977 * j) for j in range(24)]
    v = mont(r, 0xABCDEF)
    w20, w23 = mont(r, Wk.domain_omega(CURVE, 20)), mont(r, Wk.domain_omega(CURVE, 23))
    sets4 = [[4 * j + i for i in range(4)] for j in range(4)]

    def witness(ptrs, n, m, out):
        return lambda: ctx.multiopen_witness_device(CURVE, ptrs, n, [list(range(m))], np.array(z[:1]), v,
                                                    out.data_ptr(), want_evals=False)

    cases = [
        ("fft_2^20", 20, NTT_KERNELS, lambda: ctx.fft_device(CURVE, fft20.data_ptr(), 20, w20)),
        ("witness_2^20_m1", 20, POLY_KERNELS, witness(ptr20, 1 << 20, 1, out20)),
        ("witness_2^20_m4", 20, POLY_KERNELS, witness(ptr20, 1 << 20, 4, out20)),
        ("witness_2^20_m24", 20, POLY_KERNELS, witness(ptr20, 1 << 20, 24, out20)),
        ("eval_2^20_E1", 20, POLY_KERNELS,
         lambda: ctx.poly_eval_device(CURVE, ptr20, 1 << 20, [0], np.array(z[:1]))),
        ("eval_2^20_E24", 20, POLY_KERNELS,
         lambda: ctx.poly_eval_device(CURVE, ptr20, 1 << 20, list(range(24)), np.array(z))),
        ("fft_2^23", 23, NTT_KERNELS, lambda: ctx.fft_device(CURVE, fft23.data_ptr(), 23, w23)),
        ("witness_2^23_m4", 23, POLY_KERNELS, witness(ptr23, 1 << 23, 4, out23)),
        ("witness_2^20_S4_m4", 20, POLY_KERNELS,
         lambda: ctx.multiopen_witness_device(CURVE, ptr20, 1 << 20, sets4, np.array(z[:4]), v, out20.data_ptr())),
        ("open_2^20_S4_m4", 20, POLY_KERNELS + MSM_KERNELS,
         lambda: ctx.multiopen_open_device(CURVE, ptr20, 1 << 20, sets4, np.array(z[:4]), v, srs)),
    ]
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
                   "kernels_ms": kernels[name]}
            if name.startswith("open"):
                poly = sum(v_ for k_, v_ in kernels[name].items() if k_ in POLY_KERNELS)
                msm = sum(v_ for k_, v_ in kernels[name].items() if k_ in MSM_KERNELS)
                rec["poly_kernels_ms"], rec["msm_kernels_ms"] = round(poly, 4), round(msm, 4)
                # the share pm_ctx_kernel_stats gives: MSM kernel time over all kernel time of the call
                rec["msm_share_of_kernels"] = round(msm / (msm + poly), 4)
                # and, from the walls alone, what the commits add to the stand-alone witness of the same shape
                rec["msm_share_by_wall_difference"] = round(1 - med["witness_2^20_S4_m4"] / med[name], 4)
            emit(rec)
        emit({"ratios_to_fft_same_length": {
            "witness_2^20_m1": round(med["witness_2^20_m1"] / med["fft_2^20"], 3),
            "witness_2^20_m4": round(med["witness_2^20_m4"] / med["fft_2^20"], 3),
            "witness_2^20_m24": round(med["witness_2^20_m24"] / med["fft_2^20"], 3),
            "eval_2^20_E1": round(med["eval_2^20_E1"] / med["fft_2^20"], 3),
            "eval_2^20_E24_per_pair": round(med["eval_2^20_E24"] / 24 / med["fft_2^20"], 3),
            "witness_2^23_m4": round(med["witness_2^23_m4"] / med["fft_2^23"], 3)},
            "targets": {"witness_2^20_m4": 2.0, "eval_2^20_E1": 1.0}})
    srs.release()


if __name__ == "__main__":
    main()

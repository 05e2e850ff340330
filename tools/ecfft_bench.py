"""Timing of best_fft over curve points (pm_fft_points_device): BN254,
device-resident points, log_n = 14, 17, 20, against two yardsticks taken in the
same process:

  * k_acc_termmul's terms per second at B = 4096 (the same one-term windowed GLV
    multiplication, two terms per lane there): terms x B over its kernel time
    from pm_ctx_kernel_stats.  The stage kernels at 2^20 should reach 0.75 of it.
  * pm_fft_points_host on 16 threads at 2^14, same input, checked equal.

Method as tools/poly_bench.py: every case is a synchronous library call timed
with the host clock; all cases are warmed, then ROUNDS rounds visit them in
turn, each round timing enough back-to-back calls to fill ~50 ms (at least
one); the figure is the median round with its min / max.  Per-kernel times
come from a separate pass with the context's event timing on.

Writes profiles/ecfft/ecfft_bench.jsonl."""
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
ROUNDS = int(os.environ.get("ECFFT_BENCH_ROUNDS", "5"))
LOGS = [int(x) for x in os.environ.get("ECFFT_BENCH_LOGS", "14,17,20").split(",")]
WINDOW_S = 0.05
KERNELS = ["ecfft_twiddles", "ecfft_bitrev", "ecfft_first", "ecfft_stage", "ecfft_scale"]
ACC_B = 4096
ACC_TERMS = 30  # terms per proof of the simple-example shape (accum_plan.hpp)
HOST_LOG, HOST_THREADS = 14, 16


def mont(r, v):
    v = v * (1 << 256) % r
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)], dtype=np.uint64)


def stage_multiplications(k):
    """Butterflies of stages 2 .. k whose twiddle is not 1 (those lanes multiply)."""
    n = 1 << k
    return sum(n // 2 - (n >> s) for s in range(2, k + 1))


def main():
    out_path = os.path.join(ROOT, "profiles", "ecfft", "ecfft_bench.jsonl")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("ecfft_bench needs a GPU")
    ctx = H.Context(0)
    r = H.SCALAR_MODULUS[CURVE]
    dev = torch.device("cuda", 0)
    kmax = max(LOGS + [HOST_LOG])
    src = torch.empty((1 << kmax, 8), dtype=torch.int64, device=dev)
    ctx.synth_bases(CURVE, 0xA11CE, 0, 1 << kmax, src.data_ptr())
    work = torch.empty_like(src)
    torch.cuda.synchronize()

    def case(k):
        w, sc = mont(r, pow(Wk.domain_omega(CURVE, k), -1, r)), mont(r, pow(1 << k, -1, r))

        def fn():  # g_lagrange of the first 2^k points (the copy is ~1 % of the call and is timed with it)
            work[:1 << k].copy_(src[:1 << k])
            torch.cuda.synchronize()
            ctx.fft_points_device(CURVE, work.data_ptr(), k, w, sc)
        return fn

    cases = [("fft_points_2^%d" % k, k, case(k)) for k in LOGS]
    reps = {}
    for name, _, fn in cases:
        fn()
        fn()
        t = time.perf_counter()
        fn()
        reps[name] = max(1, int(WINDOW_S / max(time.perf_counter() - t, 1e-6)))
    samples = {name: [] for name, _, _ in cases}
    for _ in range(ROUNDS):
        for name, _, fn in cases:
            t = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            samples[name].append((time.perf_counter() - t) / reps[name] * 1e3)
    kernels = {}
    ctx.set_timing(True)
    for name, _, fn in cases:
        ctx.reset_stats()
        for _ in range(3):
            fn()
        kernels[name] = {k: round(ctx.kernel_stats(k)[1] / 3, 4) for k in KERNELS if ctx.kernel_stats(k)[0]}
    # the yardstick: k_acc_termmul at B = 4096, same process
    shape = Wk.simple_example_shape(ctx, CURVE, 17)
    batch = Wk.SyntheticBatch(ctx, shape, ACC_B)
    batch.to_proof_bytes(shape)
    ctx.set_timing(False)
    for _ in range(3):
        batch.run_bytes(ctx, shape)
    ctx.set_timing(True)
    ctx.reset_stats()
    for _ in range(5):
        batch.run_bytes(ctx, shape)
    ctx.set_timing(False)
    tm_ms = ctx.kernel_stats("acc_termmul")[1] / 5
    tm_rate = ACC_TERMS * ACC_B / (tm_ms * 1e-3)
    # the CPU baseline, same input, checked equal
    k = HOST_LOG
    host_in = src[:1 << k].cpu().numpy().view(np.uint64)
    w, sc = mont(r, pow(Wk.domain_omega(CURVE, k), -1, r)), mont(r, pow(1 << k, -1, r))
    t = time.perf_counter()
    host_out = H.fft_points_host(CURVE, host_in, w, sc, threads=HOST_THREADS)
    host_ms = (time.perf_counter() - t) * 1e3
    work[:1 << k].copy_(src[:1 << k])
    torch.cuda.synchronize()
    ctx.fft_points_device(CURVE, work.data_ptr(), k, w, sc)
    torch.cuda.synchronize()
    equal = bool(np.array_equal(work[:1 << k].cpu().numpy().view(np.uint64), host_out))

    with open(out_path, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")

        rates = {}
        for name, k, _ in cases:
            s = samples[name]
            st = kernels[name].get("ecfft_stage", 0.0)
            rates[k] = stage_multiplications(k) / (st * 1e-3) if st else 0.0
            emit({"case": name, "curve": "bn254", "log_n": k, "calls_per_round": reps[name], "rounds": ROUNDS,
                  "wall_ms": round(statistics.median(s), 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4),
                  "kernels_ms": kernels[name], "stage_multiplications": stage_multiplications(k),
                  "stage_mul_per_s": round(rates[k], 1)})
        emit({"yardstick": "acc_termmul", "B": ACC_B, "terms_per_proof": ACC_TERMS, "kernel_ms": round(tm_ms, 4),
              "terms_per_s": round(tm_rate, 1),
              "stage_rate_over_termmul": {str(k): round(v / tm_rate, 4) for k, v in rates.items()},
              "target_at_2^20": 0.75})
        dev_ms = statistics.median(samples["fft_points_2^%d" % HOST_LOG]) if HOST_LOG in LOGS else None
        emit({"cpu_baseline": "pm_fft_points_host", "log_n": HOST_LOG, "threads": HOST_THREADS,
              "host_ms": round(host_ms, 2), "device_wall_ms": None if dev_ms is None else round(dev_ms, 4),
              "equal": equal,
              "k23_extrapolated_s": {"note": "n log n extrapolation from these sizes, not a measurement",
                                     "host": round(host_ms * (23 * 2 ** 23) / (k * 2 ** k) / 1e3, 1),
                                     "device": None if max(LOGS) < 20 else round(
                                         statistics.median(samples["fft_points_2^%d" % max(LOGS)])
                                         * (23 * 2 ** 23) / (max(LOGS) * 2 ** max(LOGS)) / 1e3, 2)}})
    if not equal:
        raise SystemExit("device and host transforms differ")


if __name__ == "__main__":
    main()

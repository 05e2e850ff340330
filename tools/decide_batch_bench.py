"""Timing of the batch decider (pm_accum_decide_batch_device: one pairing check
for B accumulator quads) against the per-proof decider on the same quads
(pm_accum_decide_device), its host form (pm_accum_decide_host, on the threads
the process is granted), the batch decider's own host form
(pm_accum_decide_batch_host, one thread) and the accumulator that feeds them
(pm_accum_batch_proofs_device on the simple-example batch of the same B),
B in {16, 256, 4096}.

The batch is accepting: 64 distinct quads built from known discrete logs
(a tau = b + c + d), tiled to B, under a fixed seed.  Before any time is recorded
the batch call's ok, status, L and R are compared with the host form's and with
the sums stated from the logs, and the per-proof decider's words with all ones.

Timing as tools/pairing_bench.py: every case is a synchronous library call timed
with the host clock; all cases are warmed first, then ROUNDS rounds visit the
cases in turn, each round timing enough back-to-back calls to fill ~50 ms (at
least 3).  The figure is the median round, with min and max.  The batch call's
phase split (prep kernel, table + sums, host Horner, host pairing) comes from a
separate pass with the context's timing on.

Writes profiles/pairing/decide_batch_bench.jsonl, or the path given as the first
argument (one line per case, then the ratios)."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "halo2-aggregation_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import decide_batch_util as D  # noqa: E402
import halo2_amd as H  # noqa: E402
import pairing_ref as PR  # noqa: E402
import pairing_util as U  # noqa: E402
import workloads as Wk  # noqa: E402

ROUNDS = int(os.environ.get("DECIDE_BATCH_BENCH_ROUNDS", "7"))
SIZES = [int(x) for x in os.environ.get("DECIDE_BATCH_BENCH_SIZES", "16,256,4096").split(",")]
WINDOW_S = 0.05
PHASES = ["decide_batch_prep", "decide_batch_sum", "decide_batch_horner", "decide_batch_pairing"]
ACCUM_LOGN = 17
DISTINCT = 64


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pairing", "decide_batch_bench.jsonl")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    if H.device_count() < 1:
        raise SystemExit("decide_batch_bench needs a GPU")
    ctx = H.Context(0)
    dev = torch.device("cuda", 0)
    pr = H.Pairing(ctx, U.g2_words(PR.G2), U.g2_words(U.s_g2()))
    shape = Wk.simple_example_shape(ctx, H.BN254, ACCUM_LOGN)
    seed = D.SEED

    cases, keep = [], []
    for B in SIZES:
        logs = D.accepting(B, types=DISTINCT)
        q = D.quads_from_logs(logs)
        d_q = torch.from_numpy(q.view(np.int64)).to(dev)
        d_ok = torch.zeros(B, dtype=torch.int32, device=dev)
        d_st = torch.zeros(B, dtype=torch.int32, device=dev)
        batch = Wk.SyntheticBatch(ctx, shape, B)
        batch.to_proof_bytes(shape)
        keep += [d_q, d_ok, d_st, batch]
        # results first: device == host form == the sums stated from the logs
        want_ok, want_pair = D.expect(logs, seed)
        host = H.accum_decide_batch_host(pr, q, seed=seed)
        got = ctx.accum_decide_batch_device(pr, B, d_q.data_ptr(), d_status=d_st.data_ptr(), seed=seed)
        assert want_ok == 1 and host["ok"] == 1 and got["ok"] == 1, "ok"
        assert np.array_equal(host["pair"], want_pair) and np.array_equal(got["pair"], want_pair), "L, R"
        assert not d_st.cpu().numpy().any() and not host["status"].any(), "status"
        ctx.accum_decide_device(pr, B, d_q.data_ptr(), d_ok.data_ptr())
        assert (d_ok.cpu().numpy() == 1).all(), "per-proof decider"
        cases.append((f"decide_batch_device_B{B}", B, PHASES,
                      lambda B=B, d_q=d_q: ctx.accum_decide_batch_device(pr, B, d_q.data_ptr(), seed=seed)))
        cases.append((f"decide_device_B{B}", B, [],
                      lambda B=B, d_q=d_q, d_ok=d_ok: ctx.accum_decide_device(pr, B, d_q.data_ptr(), d_ok.data_ptr())))
        cases.append((f"decide_host_B{B}", B, [], lambda q=q: H.accum_decide_host(pr, q)))
        cases.append((f"decide_batch_host_B{B}", B, [], lambda q=q: H.accum_decide_batch_host(pr, q, seed=seed)))
        cases.append((f"accum_proofs_device_B{B}", B, [], lambda batch=batch: batch.run_bytes(ctx, shape)))
    torch.cuda.synchronize()

    reps = {}
    for name, _, _, fn in cases:  # warm-up, and the calls per window
        fn()
        t = time.perf_counter()
        fn()
        one = max(time.perf_counter() - t, 1e-6)
        reps[name] = 1 if one > WINDOW_S else max(3, int(WINDOW_S / one))
    samples = {name: [] for name, _, _, _ in cases}
    for _ in range(ROUNDS):
        for name, _, _, fn in cases:
            t = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            samples[name].append((time.perf_counter() - t) / reps[name] * 1e3)
    phases = {}
    ctx.set_timing(True)
    for name, _, names, fn in cases:
        if not names:
            continue
        ctx.reset_stats()
        for _ in range(5):
            fn()
        phases[name] = {k: round(ctx.kernel_stats(k)[1] / 5, 4) for k in names if ctx.kernel_stats(k)[0]}
    ctx.set_timing(False)
    med = {name: statistics.median(s) for name, s in samples.items()}
    with open(out_path, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")

        for name, B, _, _ in cases:
            s = samples[name]
            rec = {"case": name, "B": B, "calls_per_round": reps[name], "rounds": ROUNDS,
                   "wall_ms": round(med[name], 4), "min_ms": round(min(s), 4), "max_ms": round(max(s), 4)}
            if name in phases:
                rec["phases_ms"] = phases[name]
            if name.startswith("decide_host"):
                rec["host_threads"] = min(16, len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16")))
            if name.startswith("accum"):
                rec["log_n"] = ACCUM_LOGN
            emit(rec)
        emit({"ratios": {
            f"B{B}": {"decide_over_batch": round(med[f"decide_device_B{B}"] / med[f"decide_batch_device_B{B}"], 2),
                      "host_per_proof_over_batch": round(med[f"decide_host_B{B}"] / med[f"decide_batch_device_B{B}"], 2),
                      "batch_over_accumulator": round(med[f"decide_batch_device_B{B}"] / med[f"accum_proofs_device_B{B}"], 3)}
            for B in SIZES}})
        faster = med["decide_batch_device_B%d" % max(SIZES)] < med["decide_device_B%d" % max(SIZES)]
        emit({"requirement": "batch call faster than pm_accum_decide_device at B = %d" % max(SIZES), "met": bool(faster)})


if __name__ == "__main__":
    main()

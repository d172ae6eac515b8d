"""Plain sumcheck: prover against verifier, same process, same resident tables: gkr_sumcheck_mle_batch_device alternating with
gkr_sumcheck_mle_verify_batch_device on

    headline   1024 x 2^20   (bench.py's step)
    lone          1 x 2^20
    small      4096 x 2^16

Per shape: the tables are filled on the device, one warm-up of each call, then --reps alternating repetitions; medians and
spread (interquartile range, min / max) of both, every timed verdict checked (all accepted).  The yardsticks:

  * the floor of a verify call: 32 * 2^n * batch bytes at the box's own read_GBps (gkr_ubench_ceilings, measured in this
    process before the first shape); the verify call is reported as a fraction of it, and so is the evaluation kernel alone
    when the kernel times of a rocprofv3 run of its own are given:

        python tools/bench_mle_verify.py --only headline --write-transcript T.npz
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mlev -- python tools/bench_mle_verify.py --trace-calls 5 --only headline --transcript T.npz
        python tools/bench_mle_verify.py --kernel-stats DIR/.../mlev_kernel_stats.csv --kernel-stats-calls 6

    (--write-transcript: prove the shape once, keep the transcript, nothing else.  --trace-calls N: no timing; one warm-up and N
    verify calls, N + 1 in the trace.  The prover launches k_eq_table and k_mle_fold_plan too, so the traced process reads the
    transcript of the same seed's tables from --transcript and never proves: the per-call kernel sums are the verifier's alone);
  * the same process's prove time for the same batch: by byte count alone (32 against 66 bytes per entry in the prover's default
    schedule) a verify should land near half of it; "verify_clearly_below_prove" says whether the verify median is below the
    prove median by more than the sum of the two interquartile ranges.

The result goes to profiles/r10/mle_verify.json (or --out)."""

import argparse
import csv
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gkr_amd import Context  # noqa: E402

SHAPES = {"headline": (20, 1024), "lone": (20, 1), "small": (16, 4096)}
EVAL_KERNELS = ("k_mle_eval_mfma", "k_mle_eval_small")
CALL_KERNELS = ("k_mle_eval", "k_eq_table", "k_mle_fold_plan", "k_verify_hash")


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms_per_call(path, calls):
    """-> (the evaluation kernel alone, every kernel of a verify call, per kernel) in ms per call, from a rocprofv3 --stats CSV."""
    ev, total, rows = 0.0, 0.0, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ms = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0) / 1e6 / calls
            if any(tag in name for tag in CALL_KERNELS):
                total += ms
                short = name.split("(")[0].split("::")[-1]
                rows[short] = rows.get(short, 0.0) + ms
            if any(tag in name for tag in EVAL_KERNELS):
                ev += ms
    return ev, total, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=sorted(SHAPES))
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--write-transcript", help="with --only: prove that shape, write its transcript to this .npz and stop")
    ap.add_argument("--transcript", help="with --trace-calls and --only: the transcript to verify (no prover call in the trace)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats CSV of a --trace-calls run of `headline`")
    ap.add_argument("--kernel-stats-calls", type=int, default=6, help="verify calls in that trace (--trace-calls + 1)")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r10", "mle_verify.json"))
    args = ap.parse_args()
    if args.reps < 20 and not args.trace_calls:
        ap.error("at least 20 repetitions")
    if (args.write_transcript or args.transcript) and not args.only:
        ap.error("a transcript belongs to one shape: --only")
    if args.trace_calls and not args.transcript:
        ap.error("--trace-calls verifies a transcript written before the trace: --transcript")
    result = {"tool": "tools/bench_mle_verify.py", "shapes": {}}
    bad = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        if not args.trace_calls and not args.write_transcript:
            result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for name, (n, batch) in SHAPES.items():
            if args.only and name != args.only:
                continue
            count = batch << n
            d = ctx.alloc(count * 32)
            try:
                ctx.fill_table(d, count, 0xC0FFEE + n)
                if args.trace_calls:
                    import numpy as np
                    with np.load(args.transcript) as z:
                        C, L, R = z["C"], z["L"], z["R"]
                else:
                    out = ctx.sumcheck_mle_batch_device(d, n, batch)
                    C, L, R = out
                if args.write_transcript:
                    import numpy as np
                    np.savez(args.write_transcript, C=C, L=L, R=R)
                    return 0
                verify = lambda: ctx.verify_sumcheck_batch_device(d, n, batch, C, L, R)   # noqa: E731
                accept = verify()[0]                                                      # (the warm-up)
                bad += int(not accept.all())
                if args.trace_calls:
                    for _ in range(args.trace_calls):
                        verify()
                    continue
                t_prove, t_verify = [], []
                for _ in range(args.reps):
                    ms, _ = timed(lambda: ctx.sumcheck_mle_batch_device(d, n, batch, out=out))
                    t_prove.append(ms)
                    ms, res = timed(verify)
                    t_verify.append(ms)
                    bad += int(not res[0].all())
            finally:
                ctx.free(d)
            p, v = spread(t_prove), spread(t_verify)
            floor_ms = 32.0 * count / (result["ceilings"]["read_GBps"] * 1e6)
            row = {"n": n, "batch": batch, "table_bytes": 32 * count, "prove": p, "verify": v, "floor_ms": floor_ms,
                   "floor_over_verify": floor_ms / v["median_ms"], "verify_over_prove": v["median_ms"] / p["median_ms"],
                   "verify_clearly_below_prove": p["median_ms"] - v["median_ms"] > p["iqr_ms"] + v["iqr_ms"],
                   "eval_kernel_ms_per_call": "not measured", "floor_over_eval_kernel": "not measured"}
            if name == "headline" and args.kernel_stats:
                ev, total, rows = kernel_ms_per_call(args.kernel_stats, args.kernel_stats_calls)
                row.update({"eval_kernel_ms_per_call": ev, "floor_over_eval_kernel": floor_ms / ev if ev else None,
                            "kernels_ms_per_call": rows, "all_kernels_ms_per_call": total})
            result["shapes"][name] = row
            print(name, json.dumps(row), flush=True)
    if args.trace_calls:
        return 1 if bad else 0
    result["rejected_or_failed"] = bad
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

"""Sumcheck over a sum of products of resident tables (gkr_sumcheck_sop_batch_device) at n = 20, batch in {1, 64}, three term
structures:

  * eq (A B - C):  4 tables, terms (0, 1, 2) and -(0, 3) -- the R1CS zero-check;
  * A B + C D:     4 tables, two terms of degree 2;
  * A B C:         one term of degree 3, beside gkr_sumcheck_product_batch_device at degree 3 on the SAME tables in the same
                   process -- the yardstick: the same transcript (checked: equal bytes) from the fused product kernels.

Per shape and structure: the tables are filled on the device, one warm-up of each call, then --reps alternating repetitions timed
on the host clock around calls that end in a device synchronise; medians and spread (interquartile range, min / max).  Every timed
output is checked: the first against verify_sumcheck_sop on every sumcheck and against mle_eval_batch_device on the same resident
tables, every later one for equality with the first.  Then --profile-reps calls under the context profile give the per-call kernel
times by name (sop_first, sop_fold_sum, sop_round) -- the pass / round split.  For the single term `sop_over_product` is the
ratio of the medians and `behind_by_iqrs` the difference of the medians in units of the larger of the two interquartile ranges.

Informational: no threshold.  Prints one JSON line; --out also writes it to a file."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gkr_amd import MODULUS, Context, from_limbs, verify_sumcheck_sop  # noqa: E402

STRUCTURES = [
    ("eq(AB-C)", 4, [(1, (0, 1, 2)), (MODULUS - 1, (0, 3))]),
    ("AB+CD", 4, [(1, (0, 1)), (1, (2, 3))]),
    ("ABC", 3, [(1, (0, 1, 2))]),
]


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def check(ctx, d, n, n_tables, terms, batch, out):
    """verify_sumcheck_sop on every sumcheck, and the evals against the evaluation kernel on the same tables."""
    C, L, R, E = out
    D = C.shape[2] - 1
    for b in range(batch):
        proof = [from_limbs(C[b, j])[D + 1 - int(L[b, j]):] for j in range(n)]
        if not verify_sumcheck_sop(proof, from_limbs(R[b]), from_limbs(E[b]), terms):
            return False
    return bool(np.array_equal(ctx.mle_eval_batch_device(d, n, batch * n_tables, np.repeat(R, n_tables, axis=0)), E.reshape(-1, 4)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    result = {"tool": "tools/bench_sop.py", "n": n, "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        for name, n_tables, terms in STRUCTURES:
            for batch in (1, 64):
                tables = batch * n_tables
                d = ctx.alloc((tables << n) * 32)
                try:
                    ctx.fill_table(d, tables << n, 0xC0FFEE + 1500 + 16 * n_tables + batch)
                    first = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)               # warm-up
                    ok = check(ctx, d, n, n_tables, terms, batch, first)
                    out = tuple(np.zeros_like(a) for a in first)
                    single = len(terms) == 1
                    if single:
                        product = ctx.sumcheck_product_batch_device(d, n, n_tables, batch)            # warm-up
                        ok = ok and all(a.tobytes() == b.tobytes() for a, b in zip(first, product))
                    t_sop, t_prod = [], []
                    for _ in range(args.reps):
                        ms, got = timed(lambda: ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch, out=out))
                        t_sop.append(ms)
                        ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first))
                        if single:
                            ms, _ = timed(lambda: ctx.sumcheck_product_batch_device(d, n, n_tables, batch, out=product))
                            t_prod.append(ms)
                    ctx.profile(1)
                    ctx.profile_reset()
                    for _ in range(args.profile_reps):
                        ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch, out=out)
                    kernels = {k: ctx.profile_get(k)["total_ms"] / args.profile_reps for k in ("sop_first", "sop_fold_sum", "sop_round")}
                    if single:
                        ctx.profile_reset()
                        for _ in range(args.profile_reps):
                            ctx.sumcheck_product_batch_device(d, n, n_tables, batch, out=product)
                        kernels.update({k: ctx.profile_get(k)["total_ms"] / args.profile_reps
                                        for k in ("product_first", "product_fold_sum", "product_round")})
                    ctx.profile(0)
                finally:
                    ctx.free(d)
                failed += int(not ok)
                s = spread(t_sop)
                pass_ms = kernels["sop_first"] + kernels["sop_fold_sum"]
                row = {"structure": name, "n_tables": n_tables, "n_terms": len(terms), "batch": batch, "checked": "ok" if ok else "FAILED",
                       "sop": s, "kernels_ms_per_call": kernels, "passes_ms_per_call": pass_ms,
                       "round_kernel_share_of_kernel_time": kernels["sop_round"] / (pass_ms + kernels["sop_round"]),
                       "table_bytes": tables * 32 * (1 << n)}
                if single:
                    p = spread(t_prod)
                    row["product"] = p
                    row["sop_over_product"] = s["median_ms"] / p["median_ms"]
                    row["behind_by_iqrs"] = (s["median_ms"] - p["median_ms"]) / max(s["iqr_ms"], p["iqr_ms"], 1e-9)
                result["shapes"].append(row)
    result["failed"] = failed
    line = json.dumps(result, sort_keys=True)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())

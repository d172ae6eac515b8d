"""Sumcheck over a sum of products of resident tables (gkr_sumcheck_sop_batch_device) at n = 20, batch in {1, 64} (--batches),
three term structures:

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

The verify leg, same process and tables (after tools/bench_product.py's): gkr_sumcheck_sop_verify_batch_device on the transcripts
just proved, alternating with a bare gkr_mle_eval_batch_device call on the same batch * n_tables tables with every point repeated
n_tables times -- the evaluation alone, every table on its own, the yardstick of what the verifier's one read of the tables should
cost.  Per call: host-clock medians and spread, the `mle_eval` (and `verify_hash`) entries of the context profile, and the
fraction of the box's read ceiling (gkr_ubench_ceilings, measured in this process) that the tables' batch * n_tables * 32 * 2^n
bytes reach in the call and in its `mle_eval` entry.  Checked: every transcript accepted, the values equal to the prover's and to
the bare evaluation's.  What the call costs above the bare evaluation is reported, not gated.

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


def verify_leg(ctx, d, n, n_tables, terms, batch, proved, args, ceil):
    C, L, R, E = proved
    tables = batch * n_tables
    points = np.ascontiguousarray(np.repeat(R, n_tables, axis=0))
    verify = lambda: ctx.verify_sumcheck_sop_batch_device(d, n, n_tables, terms, batch, C, L, R)
    bare = lambda: ctx.mle_eval_batch_device(d, n, tables, points)
    accepted = lambda res: bool(res[0].all()) and res[4].tobytes() == E.tobytes()
    ok = accepted(verify())                                                                    # warm-up
    ok = ok and bare().tobytes() == E.tobytes()
    t_verify, t_bare = [], []
    for _ in range(args.reps):
        ms, res = timed(verify)
        t_verify.append(ms)
        ok = ok and accepted(res)
        ms, got = timed(bare)
        t_bare.append(ms)
        ok = ok and got.tobytes() == E.tobytes()
    ctx.profile(1)
    entries = {}
    for name, call in (("verify", verify), ("bare", bare)):
        ctx.profile_reset()
        for _ in range(args.profile_reps):
            call()
        entries[name] = {k: ctx.profile_get(k)["total_ms"] / args.profile_reps for k in ("mle_eval", "verify_hash")}
    ctx.profile(0)
    v, b = spread(t_verify), spread(t_bare)
    floor_ms = tables * 32.0 * (1 << n) / (ceil["read_GBps"] * 1e6)
    return {"ok": ok, "verify": v, "bare_mle_eval": b, "table_bytes": tables * 32 * (1 << n), "read_floor_ms": floor_ms,
            "verify_profile_ms_per_call": entries["verify"], "bare_profile_ms_per_call": entries["bare"],
            "verify_call_fraction_of_read_ceiling": floor_ms / v["median_ms"], "bare_call_fraction_of_read_ceiling": floor_ms / b["median_ms"],
            "verify_mle_eval_fraction_of_read_ceiling": floor_ms / entries["verify"]["mle_eval"],
            "bare_mle_eval_fraction_of_read_ceiling": floor_ms / entries["bare"]["mle_eval"],
            "verify_minus_bare_ms": v["median_ms"] - b["median_ms"], "device_hashes": entries["verify"]["verify_hash"] > 0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-reps", type=int, default=5)
    ap.add_argument("--batches", default="1,64", help="batch sizes, comma-separated")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    result = {"tool": "tools/bench_sop.py", "n": n, "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for name, n_tables, terms in STRUCTURES:
            for batch in [int(b) for b in args.batches.split(",")]:
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
                    verify = verify_leg(ctx, d, n, n_tables, terms, batch, first, args, ceil)
                    ok = ok and verify.pop("ok")
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
                row["verify"] = verify
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

"""Sumcheck over a product of resident tables (gkr_sumcheck_product_batch_device) at n = 20, degree in {2, 3}, batch in {1, 64},
against two yardsticks taken in the same process on the same tables:

  * the plain per-round device-transcript sumcheck (gkr_sumcheck_mle_batch_device, GKR_TRANSCRIPT_DEVICE) of batch * degree
    tables of 2^20 entries -- the same table traffic and hash count without the products;
  * the box's own ceilings (gkr_ubench_ceilings): read GB/s and modular products per second.

Per shape: the tables are filled on the device, one warm-up of each call, then --reps alternating repetitions timed on the host
clock around calls that end in a device synchronise; medians and spread (interquartile range, min / max).  Every timed output is
checked: the first against verify_sumcheck_product on every sumcheck and against mle_eval_batch_device on the same resident
tables (the evals are the factors' values at the challenges), every later one for equality with the first.  Then --profile-reps
calls under the context profile give the per-call kernel times by name (product_first, product_fold_sum, product_round) and the
share of the round kernel -- the device hash, once per round on the critical path.

The verify leg, same process and tables: gkr_sumcheck_product_verify_batch_device on the transcripts just proved, alternating
with a bare gkr_mle_eval_batch_device call on the same batch * degree tables at the same points -- the evaluation alone, the
yardstick of what the verifier's table read should cost.  Per call: host-clock medians and spread, the `mle_eval` (and
`verify_hash`) entries of the context profile, and the fraction of the box's read ceiling that the tables' batch * degree * 32 *
2^n bytes reach in the call and in its `mle_eval` entry.  Checked: every transcript accepted, the values equal to the prover's.

Algorithmic counts per sumcheck (h = 2^(n-1)): modular products  h * c  in round 1 and  q * (2 d + c)  in a round that folds
(q = a quarter of its source tables; c = 3 at degree 2, 8 at degree 3: one per value at degree 2, a Montgomery and a lazy product
per value at degree 3), about  h * (2 d + 2 c)  in all; bytes  32 * d * 2^n  in round 1 and  6 q * 32  per factor and folding
round, about  4 * 32 * d * 2^n  in all.  `floor_ms` is the larger of bytes over read_GBps and products over modmul_per_sec, and
`bound` names it.

Prints one JSON line; --out also writes it to a file."""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gkr_amd import Context, from_limbs, verify_sumcheck_product  # noqa: E402
from gkr_amd import _native as N  # noqa: E402

COEFF_PRODUCTS = {1: 0, 2: 3, 3: 8}


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def check(ctx, d, n, degree, batch, out):
    """verify_sumcheck_product on every sumcheck, and the evals against the evaluation kernel on the same tables."""
    C, L, R, E = out
    for b in range(batch):
        proof = [from_limbs(C[b, j])[degree + 1 - int(L[b, j]):] for j in range(n)]
        if not verify_sumcheck_product(proof, from_limbs(R[b]), from_limbs(E[b]), degree):
            return False
    return bool(np.array_equal(ctx.mle_eval_batch_device(d, n, batch * degree, np.repeat(R, degree, axis=0)), E.reshape(-1, 4)))


def verify_leg(ctx, d, n, degree, batch, proved, args, ceil):
    C, L, R, E = proved
    tables = batch * degree
    points = np.ascontiguousarray(np.repeat(R, degree, axis=0))
    accepted = lambda res: bool(res[0].all()) and bool(np.array_equal(res[4], E))
    ok = accepted(ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R))      # warm-up
    ok = ok and bool(np.array_equal(ctx.mle_eval_batch_device(d, n, tables, points), E.reshape(-1, 4)))
    t_verify, t_bare = [], []
    for _ in range(args.reps):
        ms, res = timed(lambda: ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R))
        t_verify.append(ms)
        ok = ok and accepted(res)
        ms, _ = timed(lambda: ctx.mle_eval_batch_device(d, n, tables, points))
        t_bare.append(ms)
    ctx.profile(1)
    entries = {}
    for name, call in (("verify", lambda: ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R)),
                       ("bare", lambda: ctx.mle_eval_batch_device(d, n, tables, points))):
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


def counts(n, degree, batch):
    h, c = 1 << (n - 1), COEFF_PRODUCTS[degree]
    products = bytes_ = 0
    for rnd in range(n):
        items = (1 << n) >> (rnd + 1)
        products += items * (c if rnd == 0 else 2 * degree + c)
        bytes_ += 32 * degree * (2 * items if rnd == 0 else 6 * items)
    assert products <= h * (2 * degree + 2 * c)
    return batch * products, batch * bytes_


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-reps", type=int, default=5)
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out")
    args = ap.parse_args()
    n = args.n
    result = {"tool": "tools/bench_product.py", "n": n, "shapes": []}
    failed = 0
    with Context(0) as ctx:
        ctx.set_transcript(N.GKR_TRANSCRIPT_DEVICE)               # the plain leg's per-round device transcript; the product path ignores the mode
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for degree in (2, 3):
            for batch in (1, 64):
                tables = batch * degree
                d = ctx.alloc((tables << n) * 32)
                try:
                    ctx.fill_table(d, tables << n, 0xC0FFEE + 16 * degree + batch)
                    first = ctx.sumcheck_product_batch_device(d, n, degree, batch)                    # warm-up
                    ok = check(ctx, d, n, degree, batch, first)
                    out = tuple(np.zeros_like(a) for a in first)
                    plain = ctx.sumcheck_mle_batch_device(d, n, tables)                              # warm-up
                    t_prod, t_plain = [], []
                    for _ in range(args.reps):
                        ms, got = timed(lambda: ctx.sumcheck_product_batch_device(d, n, degree, batch, out=out))
                        t_prod.append(ms)
                        ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first))
                        ms, _ = timed(lambda: ctx.sumcheck_mle_batch_device(d, n, tables, out=plain))
                        t_plain.append(ms)
                    ctx.profile(1)
                    ctx.profile_reset()
                    for _ in range(args.profile_reps):
                        ctx.sumcheck_product_batch_device(d, n, degree, batch, out=out)
                    kernels = {k: ctx.profile_get(k)["total_ms"] / args.profile_reps for k in ("product_first", "product_fold_sum", "product_round")}
                    ctx.profile(0)
                    verify = verify_leg(ctx, d, n, degree, batch, first, args, ceil)
                    ok = ok and verify.pop("ok")
                finally:
                    ctx.free(d)
                failed += int(not ok)
                p, q = spread(t_prod), spread(t_plain)
                products, bytes_ = counts(n, degree, batch)
                mem_ms, alu_ms = bytes_ / (ceil["read_GBps"] * 1e6), products / ceil["modmul_per_sec"] * 1e3
                pass_ms = kernels["product_first"] + kernels["product_fold_sum"]
                row = {"degree": degree, "batch": batch, "checked": "ok" if ok else "FAILED", "product": p, "plain_device_transcript": q,
                       "product_over_plain": p["median_ms"] / q["median_ms"], "modular_products": products, "algorithmic_bytes": bytes_,
                       "floor_ms": max(mem_ms, alu_ms), "bound": "modmul" if alu_ms > mem_ms else "read bandwidth",
                       "bandwidth_floor_ms": mem_ms, "modmul_floor_ms": alu_ms, "kernels_ms_per_call": kernels,
                       "passes_fraction_of_modmul_ceiling": alu_ms / pass_ms, "passes_fraction_of_read_ceiling": mem_ms / pass_ms,
                       "call_fraction_of_modmul_ceiling": alu_ms / p["median_ms"],
                       "round_kernel_share_of_kernel_time": kernels["product_round"] / (pass_ms + kernels["product_round"])}
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

"""The fractional sum (gkr_fraction_sum_batch_device) at n = 20, batch in {1, 8, 64} (--batches), in one process.  The pairs are
filled on the device; before anything is timed (P, Q) of the first and the last pair is held to the tree of the downloaded
tables' Python integers, the end claims to gkr_mle_eval_batch_device, and the device verifier must accept; every timed call must
return the first call's bytes.  Then --reps alternating repetitions, everything reported as median and spread (interquartile
range, min / max):

  call        the whole call against gkr_grand_product_batch_device at the same (n, batch) on the first half of the same
              memory, alternating in this process (host clock around calls that end in a device synchronise);
  tree        the tree's launches alone (gkr_devtest_fraction_sum_tree under the context profile: device time of the `fs_tree`
              bracket) against 5 (2^n - 1) Montgomery products per pair at the box's product rate (gkr_ubench_ceilings, measured
              in this process), against the bytes of its four reads and two writes per node at the copy rate, and against
              launch_gp_tree (gkr_devtest_grand_product_tree, `gp_tree`) on batch tables of the same size;
  verify      gkr_fraction_sum_verify_batch_device against two bare gkr_mle_eval_batch_device calls (N's tables, then D's: the
              same bytes, each table at its pair's point).

Informational: no threshold.  Prints one JSON line; --out also writes it to a file."""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gkr_amd import MODULUS, Context, from_limbs  # noqa: E402
from gkr_amd import _native as N  # noqa: E402


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def compare(a, b):
    """a over b, and how far apart the medians are in units of the larger interquartile range."""
    return {"ratio": a["median_ms"] / b["median_ms"], "apart_by_iqrs": (a["median_ms"] - b["median_ms"]) / max(a["iqr_ms"], b["iqr_ms"], 1e-9)}


def tree_ms(ctx, symbol, label, d_tables, n, batch, d_layers):
    ctx.profile_reset()
    ctx._check(getattr(N.lib(), symbol)(ctx._h, d_tables, n, batch, d_layers))
    return ctx.profile_get(label)["total_ms"]


def python_root(ctx, d_tables, n, b):
    T = ctx.download(ctypes.c_void_p(d_tables.value + (64 << n) * b), (2 << n, 4))
    p, q = (np.array(from_limbs(T[h << n:(h + 1) << n]), dtype=object) for h in (0, 1))
    while len(p) > 1:
        h = len(p) // 2
        p, q = (p[:h] * q[h:] + p[h:] * q[:h]) % MODULUS, q[:h] * q[h:] % MODULUS
    return [int(p[0]), int(q[0])]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,8,64", help="batch sizes, comma-separated")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, pair = args.n, 64 << args.n
    result = {"tool": "tools/bench_fraction_sum.py", "n": n, "rounds": n * (n - 1) // 2 - 1, "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for batch in [int(b) for b in args.batches.split(",")]:
            total = 2 * batch * ((1 << n) - 1)
            d, lay, split = ctx.alloc(batch * pair), ctx.alloc(32 * total), ctx.alloc(batch * pair)
            try:
                ctx.fill_table(d, (2 * batch) << n, 0xF5AC + batch)
                run = lambda out=None: ctx.fraction_sum_batch_device(d, n, batch, out=out)
                run_gp = lambda out=None: ctx.grand_product_batch_device(d, n, batch, out=out)      # the first `batch` tables
                first, first_gp = run(), run_gp()                  # warm-up
                ok = all(from_limbs(first[0][b]) == python_root(ctx, d, n, b) for b in sorted({0, batch - 1}))
                verify = lambda: ctx.verify_fraction_sum_batch_device(d, n, batch, *first[1:6], sums=first[0])
                ok = ok and bool(verify()[0].all())
                # N's tables then D's with every pair's point: two bare evaluations of `batch` tables each
                T = ctx.download(d, (batch, 2, 1 << n, 4))
                ctx.upload(split, np.ascontiguousarray(T.transpose(1, 0, 2, 3)))
                del T
                half = ctypes.c_void_p(split.value + batch * (pair // 2))
                evaluate = lambda: (ctx.mle_eval_batch_device(split, n, batch, first[6]), ctx.mle_eval_batch_device(half, n, batch, first[6]))
                vn, vd = evaluate()
                ok = ok and vn.tobytes() == first[7][:, 0].tobytes() and vd.tobytes() == first[7][:, 1].tobytes()
                out, out_gp = tuple(np.zeros_like(a) for a in first), tuple(np.zeros_like(a) for a in first_gp)
                t_call, t_gp, t_verify, t_eval = [], [], [], []
                for _ in range(args.reps):
                    ms, got = timed(lambda: run(out))
                    t_call.append(ms)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first))
                    ms, got = timed(lambda: run_gp(out_gp))
                    t_gp.append(ms)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first_gp))
                    ms, got = timed(verify)
                    t_verify.append(ms)
                    ok = ok and bool(got[0].all())
                    t_eval.append(timed(evaluate)[0])
                ctx.profile(1)
                t_tree, t_gp_tree = [], []
                for _ in range(args.reps):
                    t_tree.append(tree_ms(ctx, "gkr_devtest_fraction_sum_tree", "fs_tree", d, n, batch, lay))
                    t_gp_tree.append(tree_ms(ctx, "gkr_devtest_grand_product_tree", "gp_tree", d, n, batch, lay))
                ctx.profile(0)
            finally:
                for p in (d, lay, split):
                    ctx.free(p)
            failed += int(not ok)
            call, gp, ver, ev, tree, gp_tree = (spread(t) for t in (t_call, t_gp, t_verify, t_eval, t_tree, t_gp_tree))
            montgomery_floor_ms = 5.0 * batch * ((1 << n) - 1) / ceil["modmul_per_sec"] * 1e3
            byte_floor_ms = batch * 6.0 * (32 << n) / (ceil["copy_GBps"] * 1e6)
            result["shapes"].append({
                "batch": batch, "checked": "ok" if ok else "FAILED", "pair_bytes": batch * pair,
                "call": call, "grand_product_call": gp, "call_over_grand_product": compare(call, gp),
                "tree": tree, "grand_product_tree": gp_tree, "tree_over_grand_product_tree": compare(tree, gp_tree),
                "tree_floors": {"montgomery_floor_ms": montgomery_floor_ms, "byte_floor_ms": byte_floor_ms,
                                "tree_over_montgomery_floor": tree["median_ms"] / montgomery_floor_ms,
                                "tree_over_byte_floor": tree["median_ms"] / byte_floor_ms},
                "verify": ver, "two_mle_evals": ev, "verify_over_two_mle_evals": compare(ver, ev)})
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

"""The zero-check eq(z, .) (A B - C) at n = 20, batch in {1, 64} (--batches), two ways in one process:

  * zerocheck:  gkr_sumcheck_zerocheck_batch_device on the three tables A, B, C and the point z -- eq(z, .) is never a table;
  * sop:        gkr_sumcheck_sop_batch_device on FOUR tables per sumcheck, table 0 = eq(z, .) built by gkr_eq_table_device (outside
                the timed region), terms (0, 1, 2) and -(0, 3) -- the path a caller had before, and the yardstick.

The tables are filled on the device (the same values in both layouts), the two transcripts are checked to be equal byte for byte
(coefficients, lengths, challenges, the tables' values, eq(z, r)) before anything is timed and after every timed call.  Then --reps
alternating repetitions are timed on the host clock around calls that end in a device synchronise, and --reps alternating calls under
the context profile give per call the kernel times by name (zc_first, zc_fold_sum, zc_round, zc_weights; sop_first, sop_fold_sum,
sop_round).  Everything is reported as median and spread (interquartile range, min / max).

Per batch, `passes` compares zc_first + zc_fold_sum with sop_first + sop_fold_sum and `call` the whole calls: the ratio of the
medians and `ahead_by_iqrs`, the difference of the medians (sop - zerocheck) in units of the larger of the two interquartile ranges.
The pass rates are set against the box's own ceilings (gkr_ubench_ceilings, measured in this process): table bytes the passes
touch per second against the read ceiling, field products per second against the product ceiling.

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
from gkr_amd import MODULUS, Context  # noqa: E402

TERMS = [(1, (0, 1)), (MODULUS - 1, (2,))]                        # A B - C over tables A, B, C
LIFTED = [(1, (0, 1, 2)), (MODULUS - 1, (0, 3))]                  # eq A B - eq C over tables eq, A, B, C
ZC_ENTRIES = ("zc_first", "zc_fold_sum", "zc_round", "zc_weights")
SOP_ENTRIES = ("sop_first", "sop_fold_sum", "sop_round")


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def same_transcript(sop, zc):
    return (all(a.tobytes() == b.tobytes() for a, b in zip(sop[:3], zc[:3])) and sop[3][:, 1:].tobytes() == zc[3].tobytes()
            and sop[3][:, 0].tobytes() == zc[4].tobytes())


def compare(a, b):
    """a, b: spreads of the zero-check and of the SOP path."""
    return {"zerocheck_over_sop": a["median_ms"] / b["median_ms"],
            "ahead_by_iqrs": (b["median_ms"] - a["median_ms"]) / max(a["iqr_ms"], b["iqr_ms"], 1e-9)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,64", help="batch sizes, comma-separated")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, size = args.n, 32 << args.n
    result = {"tool": "tools/bench_zerocheck.py", "n": n, "structure": "eq(AB-C)", "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for batch in [int(b) for b in args.batches.split(",")]:
            Z = np.random.default_rng(2000 + batch).integers(0, 1 << 63, size=(batch, n, 4), dtype=np.uint64)
            Z[:, :, 3] &= np.uint64((1 << 60) - 1)
            d_s, d_t = ctx.alloc(batch * 4 * size), ctx.alloc(batch * 3 * size)
            try:
                for b in range(batch):                            # the same A, B, C in both layouts
                    seed = 0xC0FFEE + 1700 + 64 * batch + b
                    ctx.fill_table(ctypes.c_void_p(d_s.value + (4 * b + 1) * size), 3 << n, seed)
                    ctx.fill_table(ctypes.c_void_p(d_t.value + 3 * b * size), 3 << n, seed)
                ctx.eq_table_device(Z, n, batch, d_s, stride=4 << n)
                run_zc = lambda out=None: ctx.sumcheck_zerocheck_batch_device(d_t, n, 3, TERMS, batch, Z, out=out)
                run_sop = lambda out=None: ctx.sumcheck_sop_batch_device(d_s, n, 4, LIFTED, batch, out=out)
                first_sop, first_zc = run_sop(), run_zc()         # warm-up
                ok = same_transcript(first_sop, first_zc)
                out_sop, out_zc = tuple(np.zeros_like(a) for a in first_sop), tuple(np.zeros_like(a) for a in first_zc)
                t_zc, t_sop = [], []
                for _ in range(args.reps):
                    ms, got = timed(lambda: run_zc(out_zc))
                    t_zc.append(ms)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first_zc))
                    ms, got = timed(lambda: run_sop(out_sop))
                    t_sop.append(ms)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first_sop))
                ctx.profile(1)
                samples = {k: [] for k in ZC_ENTRIES + SOP_ENTRIES}
                for _ in range(args.reps):
                    for run, out, names in ((run_zc, out_zc, ZC_ENTRIES), (run_sop, out_sop, SOP_ENTRIES)):
                        ctx.profile_reset()
                        run(out)
                        for k in names:
                            samples[k].append(ctx.profile_get(k)["total_ms"])
                ctx.profile(0)
                ok = ok and same_transcript(out_sop, out_zc)
            finally:
                ctx.free(d_s)
                ctx.free(d_t)
            failed += int(not ok)
            kernels = {k: spread(v) for k, v in samples.items()}
            zc_pass = spread([a + b for a, b in zip(samples["zc_first"], samples["zc_fold_sum"])])
            sop_pass = spread([a + b for a, b in zip(samples["sop_first"], samples["sop_fold_sum"])])
            zc, sop = spread(t_zc), spread(t_sop)
            # what the passes touch: round 1 reads every table; round j > 1 reads the source's 2^(n-j+2) entries and writes and re-reads
            # half of them (the algorithmic bytes of the Timed entries: 6 x 32 bytes per folded pair of pairs)
            pass_bytes = lambda tables: tables * 32.0 * ((1 << n) + sum(6.0 * ((1 << n) >> (r + 1)) for r in range(1, n)))
            # field products per index and round, a Montgomery product or a fold's fixed-multiplier product counted as 1 and an
            # unreduced multiply-add as 1/2: a fold is two products per index and table; the SOP path takes 4 x (1 + 1/2) for eq A B
            # and 3/2 for eq C, the zero-check 2 + 3/2 for A B and 2/2 for C
            idx = sum((1 << n) >> (r + 1) for r in range(n))
            fold_idx = idx - ((1 << n) >> 1)
            products = {"zerocheck": batch * (fold_idx * 6.0 + idx * 4.5), "sop": batch * (fold_idx * 8.0 + idx * 7.5)}
            rates = {}
            for name, tables, p in (("zerocheck", 3 * batch, zc_pass), ("sop", 4 * batch, sop_pass)):
                gbps = pass_bytes(tables) / (p["median_ms"] * 1e6)
                mps = products[name] / (p["median_ms"] * 1e-3)
                rates[name] = {"algorithmic_GBps": gbps, "fraction_of_read_ceiling": gbps / ceil["read_GBps"], "products_per_sec": mps,
                               "fraction_of_product_ceiling": mps / ceil["modmul_per_sec"]}
            result["shapes"].append({"batch": batch, "checked": "ok" if ok else "FAILED", "zerocheck": zc, "sop": sop, "call": compare(zc, sop),
                                     "kernels_ms_per_call": kernels, "zerocheck_passes": zc_pass, "sop_passes": sop_pass,
                                     "passes": compare(zc_pass, sop_pass), "pass_rates": rates,
                                     "table_bytes": {"zerocheck": 3 * batch * size, "sop": 4 * batch * size}})
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

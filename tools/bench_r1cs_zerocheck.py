"""The R1CS zero-check on the R1CS of bench.py's large_r1cs leg (synth.mimc7_demo_r1cs(65536): 262 144 constraints, n = 18), batch
in {1, 16} (--batches), the witnesses of a batch from different inputs:

  * prepare:     gkr_r1cs_rows_prepare (the CSR flattening on the host and its upload), once, host clock;
  * r1cs:        gkr_r1cs_zerocheck_batch_device on the resident witnesses -- the rows Az, Bz, Cz, the row check, the zero-check;
  * zerocheck:   gkr_sumcheck_zerocheck_batch_device on the tables gkr_r1cs_rows_device built from the same witnesses -- what a
                 caller who already held the tables would run; r1cs - zerocheck is what the rows cost a caller.

The two transcripts are checked to be equal byte for byte before anything is timed and after every timed call, and every witness
to satisfy the R1CS (first_bad).  Then --reps alternating repetitions on the host clock around calls that end in a device
synchronise, and --reps calls under the context profile for the kernel entries by name (r1cs_rows, r1cs_check, zc_first,
zc_fold_sum, zc_round, zc_weights).  Median and spread (interquartile range, min / max).

r1cs_rows is set against two floors from the box's own ceilings (gkr_ubench_ceilings, measured in this process): its algorithmic
bytes (8 + 32 per term, 32 per table entry) at the read rate, and its non-+-1 terms at the rate of modular products; and against
the zero-check's own passes (zc_first + zc_fold_sum) of the same call.

--long-row-ab: only r1cs_rows, on the chain (rows of 1 - 2 terms) and on the chain with one dense row of 4096 terms per 1024 rows
added (n = 19).  Run once per build of the library with another kR1csLongRow (GKR_AMD_LIB) to settle that constant.

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
from gkr_amd import MODULUS, Context, synth  # noqa: E402
from gkr_amd import _native as N  # noqa: E402
from gkr_amd.convert import R1cs  # noqa: E402
from gkr_amd.field import to_limbs  # noqa: E402

TERMS = [(1, (0, 1)), (MODULUS - 1, (2,))]
ENTRIES = ("r1cs_rows", "r1cs_check", "zc_first", "zc_fold_sum", "zc_round", "zc_weights")
NONE = 0xFFFFFFFF


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def witnesses(nrounds, batch):
    return np.stack([to_limbs(synth.mimc7_demo_witness(2 + b, 3 + b % 5, nrounds=nrounds)) for b in range(batch)])


def dense_rows_added(n_wires, cons, every=1024, length=4096):
    """One row of `length` terms (coefficients 2 .. 8: products) per `every` rows of the chain, appended; B and C stay short."""
    extra = [([((t % 7) + 2, (r * 8191 + t * 13) % n_wires) for t in range(length)], [(1, 0)], [(1, 1)]) for r in range(len(cons) // every)]
    return cons + extra


def rows_only(ctx, r1cs, W, reps):
    """r1cs_rows alone (no check pass), under the profile."""
    batch, nw = W.shape[0], W.shape[1]
    inf = r1cs.csr_info()
    d_w, d_t = ctx.alloc(W.nbytes), ctx.alloc(batch * 3 * (32 << inf["n"]))
    try:
        ctx.upload(d_w, W)
        with ctx.r1cs_rows(r1cs) as rows:
            ctx.r1cs_rows_device(rows, d_w, batch, d_t, check=False)      # warm-up
            ctx.profile(1)
            ms = []
            for _ in range(reps):
                ctx.profile_reset()
                ctx.r1cs_rows_device(rows, d_w, batch, d_t, check=False)
                ms.append(ctx.profile_get("r1cs_rows")["total_ms"])
            ctx.profile(0)
    finally:
        ctx.free(d_w)
        ctx.free(d_t)
    return {"batch": batch, "n": inf["n"], "n_terms": inf["n_terms"], "n_long_rows": inf["n_long_rows"], "r1cs_rows": spread(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nrounds", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16", help="batch sizes, comma-separated")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--long-row-ab", action="store_true")
    ap.add_argument("--label", default="", help="goes into the line (the build under test)")
    ap.add_argument("--out")
    args = ap.parse_args()
    nrounds = args.nrounds
    n_wires, cons = synth.mimc7_demo_constraints(nrounds)
    result = {"tool": "tools/bench_r1cs_zerocheck.py", "nrounds": nrounds, "library": os.path.relpath(N.LIB_PATH, REPO), "label": args.label}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        if args.long_row_ab:
            batch = max(int(b) for b in args.batches.split(","))
            W = witnesses(nrounds, batch)
            result["long_row_ab"] = {"chain": rows_only(ctx, R1cs.build(n_wires, 1, 1, 1, cons), W, args.reps),
                                     "chain_with_dense_rows": rows_only(ctx, R1cs.build(n_wires, 1, 1, 1, dense_rows_added(n_wires, cons)), W, args.reps)}
        else:
            ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
            r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
            inf = result["csr"] = r1cs.csr_info()
            n, size = inf["n"], 32 << inf["n"]
            used = [r1cs.csr(m)[1][:, 1] for m in range(3)]
            products = int(sum((u >= 2).sum() for u in used))     # the terms that take a product
            terms = sum(inf["n_terms"])
            ms, rows = timed(lambda: ctx.r1cs_rows(r1cs))
            result["prepare_ms"] = ms
            result["shapes"] = []
            for batch in [int(b) for b in args.batches.split(",")]:
                W = witnesses(nrounds, batch)
                Z = np.random.default_rng(1800 + batch).integers(0, 1 << 63, size=(batch, n, 4), dtype=np.uint64)
                Z[:, :, 3] &= np.uint64((1 << 60) - 1)
                d_w, d_t = ctx.alloc(W.nbytes), ctx.alloc(batch * 3 * size)
                try:
                    ctx.upload(d_w, W)
                    bad = ctx.r1cs_rows_device(rows, d_w, batch, d_t)
                    run_r1cs = lambda: ctx.r1cs_zerocheck_batch_device(rows, d_w, batch, Z)
                    run_zc = lambda: ctx.sumcheck_zerocheck_batch_device(d_t, n, 3, TERMS, batch, Z)
                    first_r1cs, first_zc = run_r1cs(), run_zc()      # warm-up
                    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a[:5], b[:5]))
                    ok = same(first_r1cs, first_zc) and (bad == NONE).all() and (first_r1cs[5] == NONE).all()
                    assert ok, "batch %d: the two transcripts differ, or a witness breaks a constraint -- nothing is timed" % batch
                    t_r1cs, t_zc = [], []
                    for _ in range(args.reps):
                        ms, got = timed(run_r1cs)
                        t_r1cs.append(ms)
                        ok = ok and same(got, first_zc)
                        ms, got = timed(run_zc)
                        t_zc.append(ms)
                        ok = ok and same(got, first_zc)
                    ctx.profile(1)
                    samples = {k: [] for k in ENTRIES}
                    for _ in range(args.reps):
                        ctx.profile_reset()
                        run_r1cs()
                        for k in ENTRIES:
                            samples[k].append(ctx.profile_get(k)["total_ms"])
                    ctx.profile(0)
                finally:
                    ctx.free(d_w)
                    ctx.free(d_t)
                failed += int(not ok)
                kernels = {k: spread(v) for k, v in samples.items()}
                passes = spread([a + b for a, b in zip(samples["zc_first"], samples["zc_fold_sum"])])
                a, b = spread(t_r1cs), spread(t_zc)
                rows_ms = kernels["r1cs_rows"]["median_ms"]
                row_bytes = batch * (40.0 * terms + 32.0 * 3 * (1 << n))
                check_bytes = batch * 3 * 32.0 * inf["n_constraints"]
                result["shapes"].append({
                    "batch": batch, "checked": "ok" if ok else "FAILED", "r1cs": a, "zerocheck_on_its_tables": b,
                    "rows_cost_a_caller_ms": a["median_ms"] - b["median_ms"],
                    "rows_cost_in_iqrs": (a["median_ms"] - b["median_ms"]) / max(a["iqr_ms"], b["iqr_ms"], 1e-9),
                    "kernels_ms_per_call": kernels, "zc_passes": passes,
                    "r1cs_rows_over_zc_passes": rows_ms / passes["median_ms"],
                    "r1cs_rows_floors": {"bytes": row_bytes, "byte_floor_ms": row_bytes / (ceil["read_GBps"] * 1e6),
                                         "algorithmic_GBps": row_bytes / (rows_ms * 1e6),
                                         "fraction_of_read_ceiling": row_bytes / (rows_ms * 1e6) / ceil["read_GBps"],
                                         "product_terms": batch * products, "product_floor_ms": batch * products / ceil["modmul_per_sec"] * 1e3,
                                         "gather_bytes_at_128B_lines": batch * 128.0 * terms,
                                         "gather_granularity_floor_ms": batch * (128.0 * terms + 8.0 * terms + 96.0 * (1 << n)) / (ceil["read_GBps"] * 1e6)},
                    "r1cs_check_floor_ms": check_bytes / (ceil["read_GBps"] * 1e6)})
            rows.close()
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

"""The R1CS inner sumcheck on the workload of tools/bench_r1cs_zerocheck.py (synth.mimc7_demo_r1cs(65536): 262 144 constraints,
n_x = 18, n_y = 19), and on a variant in which wire 0 additionally stands in every constraint of A (one column of 262 144
records beside columns of a handful), batch in {1, 16} (--batches):

  * cols_prepare: gkr_r1cs_cols_prepare (the column-major flattening on the host, the segment lists and the upload), host clock;
  * r1cs_cols / r1cs_cols_eq: the table T and the eq table in front of it, by name from the context profile, for every segment
    length of --segments (0 = no cut: a wave per long column) -- and the parent's r1cs_rows on the SAME R1CS in the same run,
    the same records gathered the other way; the calls alternate, --reps of each;
  * inner: gkr_r1cs_inner_batch_device beside gkr_sumcheck_product_batch_device on the tables it built (T from
    gkr_r1cs_cols_device, the padded witness beside it), alternating on the host clock: inner - product is the table's share.

Before anything is timed the tables of every segment length are checked to be equal byte for byte, and the inner call's
transcript to equal the product call's.  r1cs_cols is set against its algorithmic bytes (8 + 32 per record, 32 per table entry)
and against the same with the 32-byte gather counted as whole 128-byte lines, both at the box's own read rate
(gkr_ubench_ceilings, measured in this process).  Median and spread (interquartile range, min / max).

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
from gkr_amd import Context, synth  # noqa: E402
from gkr_amd import _native as N  # noqa: E402
from gkr_amd.convert import R1cs  # noqa: E402
from gkr_amd.field import to_limbs  # noqa: E402


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def random_elements(seed, shape):
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 60) - 1)
    return a


def measure(ctx, name, n_wires, cons, W_all, batches, segments, reps, ceil):
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    inf = r1cs.csc_info()
    n_x, n_y, terms = inf["n_x"], inf["n_y"], sum(inf["n_terms"])
    len_y = 1 << n_y
    out = {"workload": name, "csc": inf, "longest_column": [int(np.diff(r1cs.csc(m)[0].astype(np.int64)).max()) for m in range(3)], "shapes": []}
    prep = []
    for _ in range(3):
        ms, h = timed(lambda: ctx.r1cs_cols(r1cs))
        prep.append(ms)
        h.close()
    out["cols_prepare"] = spread(prep)
    ms, rows = timed(lambda: ctx.r1cs_rows(r1cs))
    out["rows_prepare_ms"] = ms
    handles = {s: ctx.r1cs_cols(r1cs, segment=s) for s in segments}
    default = ctx.r1cs_cols(r1cs)
    failed = 0
    try:
        for batch in batches:
            W = np.ascontiguousarray(W_all[:batch])
            X, RHO = random_elements(1900 + batch, (batch, n_x)), random_elements(1950 + batch, (batch, 3))
            d_w, d_rows = ctx.alloc(W.nbytes), ctx.alloc(batch * 3 * (32 << n_x))
            d_t, d_ref = ctx.alloc(batch * 2 * 32 * len_y), ctx.alloc(batch * 2 * 32 * len_y)
            try:
                ctx.upload(d_w, W)
                # the tables of every segment length are one table; the inner call is the product call on {T, w padded}
                ctx.r1cs_cols_device(default, X, RHO, batch, d_ref, stride=2 * len_y)
                pad = np.zeros((len_y, 4), dtype=np.uint64)
                for b in range(batch):
                    pad[:n_wires] = W[b]
                    ctx.upload(ctypes.c_void_p(d_ref.value + (2 * b + 1) * 32 * len_y), pad)
                ref = ctx.download(d_ref, (batch, 2, len_y, 4))
                ok = True
                for s, h in handles.items():
                    ctx.r1cs_cols_device(h, X, RHO, batch, d_t, stride=2 * len_y)
                    ok = ok and np.array_equal(ctx.download(d_t, (batch, 2, len_y, 4))[:, 0], ref[:, 0])
                run_inner = lambda: ctx.r1cs_inner_batch_device(default, d_w, batch, X, RHO)
                run_product = lambda: ctx.sumcheck_product_batch_device(d_ref, n_y, 2, batch)
                first = run_product()
                same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
                ok = ok and same(run_inner(), first)
                assert ok, "%s, batch %d: the tables or the transcripts differ -- nothing is timed" % (name, batch)
                ctx.r1cs_rows_device(rows, d_w, batch, d_rows, check=False)      # warm-up
                t_inner, t_product = [], []
                for _ in range(reps):
                    ms, got = timed(run_inner)
                    t_inner.append(ms)
                    ok = ok and same(got, first)
                    ms, got = timed(run_product)
                    t_product.append(ms)
                    ok = ok and same(got, first)
                ctx.profile(1)
                k_rows, k_cols, k_eq = [], {s: [] for s in segments}, []
                for _ in range(reps):
                    ctx.profile_reset()
                    ctx.r1cs_rows_device(rows, d_w, batch, d_rows, check=False)
                    k_rows.append(ctx.profile_get("r1cs_rows")["total_ms"])
                    for s, h in handles.items():
                        ctx.profile_reset()
                        ctx.r1cs_cols_device(h, X, RHO, batch, d_t, stride=2 * len_y)
                        k_cols[s].append(ctx.profile_get("r1cs_cols")["total_ms"])
                        if s == segments[0]:
                            k_eq.append(ctx.profile_get("r1cs_cols_eq")["total_ms"])
                ctx.profile(0)
            finally:
                for d in (d_w, d_rows, d_t, d_ref):
                    ctx.free(d)
            failed += int(not ok)
            a, b = spread(t_inner), spread(t_product)
            col_bytes = batch * (40.0 * terms + 32.0 * len_y)
            line_bytes = batch * (128.0 * terms + 8.0 * terms + 32.0 * len_y)
            out["shapes"].append({
                "batch": batch, "checked": "ok" if ok else "FAILED", "inner": a, "product_on_its_tables": b,
                "table_share_ms": a["median_ms"] - b["median_ms"],
                "table_share_in_iqrs": (a["median_ms"] - b["median_ms"]) / max(a["iqr_ms"], b["iqr_ms"], 1e-9),
                "r1cs_rows": spread(k_rows), "r1cs_cols_eq": spread(k_eq),
                "r1cs_cols_by_segment": {str(s): spread(v) for s, v in k_cols.items()},
                "r1cs_cols_floors": {"bytes": col_bytes, "byte_floor_ms": col_bytes / (ceil["read_GBps"] * 1e6),
                                     "gather_bytes_at_128B_lines": batch * 128.0 * terms,
                                     "gather_granularity_floor_ms": line_bytes / (ceil["read_GBps"] * 1e6)}})
    finally:
        rows.close()
        default.close()
        for h in handles.values():
            h.close()
    return out, failed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nrounds", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16", help="batch sizes, comma-separated")
    ap.add_argument("--segments", default="512,2048,8192,0", help="segment lengths, comma-separated; 0 = no cut")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--label", default="", help="goes into the line (the build under test)")
    ap.add_argument("--out")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    segments = [int(s) for s in args.segments.split(",")]
    n_wires, cons = synth.mimc7_demo_constraints(args.nrounds)
    wire0 = [(a + [(1, 0)], b, c) for a, b, c in cons]
    W = np.stack([to_limbs(synth.mimc7_demo_witness(2 + b, 3 + b % 5, nrounds=args.nrounds)) for b in range(max(batches))])
    result = {"tool": "tools/bench_r1cs_inner.py", "nrounds": args.nrounds, "library": os.path.relpath(N.LIB_PATH, REPO), "label": args.label,
              "default_segment": N.GKR_R1CS_COL_SEGMENT, "long_col": N.GKR_R1CS_LONG_COL, "workloads": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for name, system in (("chain", cons), ("chain_with_wire0_in_every_A", wire0)):
            out, bad = measure(ctx, name, n_wires, system, W, batches, segments, args.reps, ceil)
            result["workloads"].append(out)
            failed += bad
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

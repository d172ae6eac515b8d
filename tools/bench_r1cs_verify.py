"""The R1CS verifier on the workload of tools/bench_r1cs_inner.py (synth.mimc7_demo_r1cs(65536): 262 144 constraints, n = 18,
n_y = 19), one context, one rows handle, one cols handle, batch in {1, 16} (--batches), the witnesses of a batch from different
inputs:

  * matrix_evals against its composition: gkr_r1cs_matrix_evals_device beside the three public calls it fuses --
    gkr_eq_table_device(y) -> gkr_r1cs_rows_device (that table as the witness) -> gkr_mle_eval_batch_device(x) -- on the same
    points (the two provers' challenges), alternating on the host clock around calls that end in a device synchronise; the kernel
    entries of both by name from the context profile (r1cs_mat_eq, r1cs_mat; r1cs_rows, mle_eval);
  * verify against prove: gkr_r1cs_verify_batch_device with and without the witness beside gkr_r1cs_zerocheck_batch_device and
    gkr_r1cs_inner_batch_device on the same batch, host clock;
  * r1cs_rows (the zero-check's tables of the witnesses) and r1cs_cols (the inner sumcheck's table) by name from the same run, to
    set beside the earlier profile notes.

Before anything is timed the fused values are checked to equal the composition's byte for byte and every proof to be accepted;
both are checked again after every timed call.  Median and spread (interquartile range, min / max).  The line says whether the
fused pass is slower than the composition beyond the two interquartile ranges at either batch size.

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


def measure(ctx, r1cs, rows, cols, W, batch, reps):
    inf = rows.info()
    n, n_wires = inf["n"], inf["n_wires"]
    n_y = cols.info()["n_y"]
    Z, RHO = random_elements(2000 + batch, (batch, n)), random_elements(2050 + batch, (batch, 3))
    d_w, d_ey, d_t = ctx.alloc(W.nbytes), ctx.alloc((batch << n_y) * 32), ctx.alloc((batch * 3 << n) * 32)
    d_cols = ctx.alloc((batch << n_y) * 32)
    try:
        ctx.upload(d_w, W)
        prove_zc = lambda: ctx.r1cs_zerocheck_batch_device(rows, d_w, batch, Z)
        zc = prove_zc()
        prove_inner = lambda: ctx.r1cs_inner_batch_device(cols, d_w, batch, zc[2], RHO)
        inner = prove_inner()
        X, Y = zc[2], inner[2]
        X3 = np.ascontiguousarray(np.repeat(X.reshape(batch, 1, n, 4), 3, axis=1).reshape(batch * 3, n, 4))
        fused = lambda: ctx.r1cs_matrix_evals_device(rows, X, Y)

        def composition():
            ctx.eq_table_device(Y, n_y, batch, d_ey)
            ctx.r1cs_rows_device(rows, d_ey, batch, d_t, stride=1 << n_y, check=False)
            return ctx.mle_eval_batch_device(d_t, n, batch * 3, X3).reshape(batch, 3, 4)
        verify_w = lambda: ctx.verify_r1cs_batch_device(rows, batch, Z, zc[:4], RHO, inner, d_witness=d_w)
        verify = lambda: ctx.verify_r1cs_batch_device(rows, batch, Z, zc[:4], RHO, inner)
        want = composition()
        ok = fused().tobytes() == want.tobytes() and bool(verify_w()[0].all()) and bool(verify()[0].all())
        assert ok, "batch %d: the fused values differ from the composition's or a proof is rejected -- nothing is timed" % batch
        t = {k: [] for k in ("fused", "composition", "verify_with_witness", "verify", "prove_zerocheck", "prove_inner")}
        for _ in range(reps):
            ms, got = timed(fused)
            t["fused"].append(ms)
            ok = ok and got.tobytes() == want.tobytes()
            ms, got = timed(composition)
            t["composition"].append(ms)
            ok = ok and got.tobytes() == want.tobytes()
            ms, got = timed(verify_w)
            t["verify_with_witness"].append(ms)
            ok = ok and bool(got[0].all())
            ms, got = timed(verify)
            t["verify"].append(ms)
            ok = ok and bool(got[0].all())
            ms, got = timed(prove_zc)
            t["prove_zerocheck"].append(ms)
            ok = ok and got[0].tobytes() == zc[0].tobytes()
            ms, got = timed(prove_inner)
            t["prove_inner"].append(ms)
            ok = ok and got[0].tobytes() == inner[0].tobytes()
        ctx.profile(1)
        k = {name: [] for name in ("r1cs_mat_eq", "r1cs_mat", "composition_r1cs_rows", "composition_mle_eval", "r1cs_rows", "r1cs_cols", "r1cs_cols_eq")}
        for _ in range(reps):
            ctx.profile_reset()
            fused()
            for name in ("r1cs_mat_eq", "r1cs_mat"):
                k[name].append(ctx.profile_get(name)["total_ms"])
            ctx.profile_reset()
            composition()
            k["composition_r1cs_rows"].append(ctx.profile_get("r1cs_rows")["total_ms"])
            k["composition_mle_eval"].append(ctx.profile_get("mle_eval")["total_ms"])
            ctx.profile_reset()
            ctx.r1cs_rows_device(rows, d_w, batch, d_t, check=False)
            k["r1cs_rows"].append(ctx.profile_get("r1cs_rows")["total_ms"])
            ctx.profile_reset()
            ctx.r1cs_cols_device(cols, X, RHO, batch, d_cols)
            k["r1cs_cols"].append(ctx.profile_get("r1cs_cols")["total_ms"])
            k["r1cs_cols_eq"].append(ctx.profile_get("r1cs_cols_eq")["total_ms"])
        ctx.profile(0)
    finally:
        for d in (d_w, d_ey, d_t, d_cols):
            ctx.free(d)
    host = {name: spread(v) for name, v in t.items()}
    f, c = host["fused"], host["composition"]
    diff = f["median_ms"] - c["median_ms"]
    prove = host["prove_zerocheck"]["median_ms"] + host["prove_inner"]["median_ms"]
    return {"batch": batch, "checked": "ok" if ok else "FAILED", "host_clock": host, "kernels": {name: spread(v) for name, v in k.items()},
            "fused_minus_composition_ms": diff, "fused_slower_beyond_both_iqrs": bool(diff > f["iqr_ms"] + c["iqr_ms"]),
            "composition_over_fused": c["median_ms"] / f["median_ms"],
            "prove_both_calls_ms": prove, "verify_over_prove": host["verify"]["median_ms"] / prove,
            "verify_with_witness_over_prove": host["verify_with_witness"]["median_ms"] / prove,
            "bytes_not_written_or_reread": batch * 2.0 * 3.0 * 32.0 * (1 << n), "n_wires": n_wires}, int(not ok)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nrounds", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,16", help="batch sizes, comma-separated")
    ap.add_argument("--label", default="", help="goes into the line (the build under test)")
    ap.add_argument("--out")
    args = ap.parse_args()
    batches = [int(b) for b in args.batches.split(",")]
    n_wires, cons = synth.mimc7_demo_constraints(args.nrounds)
    W_all = np.stack([to_limbs(synth.mimc7_demo_witness(2 + b, 3 + b % 5, nrounds=args.nrounds)[:n_wires]) for b in range(max(batches))])
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    result = {"tool": "tools/bench_r1cs_verify.py", "nrounds": args.nrounds, "library": os.path.relpath(N.LIB_PATH, REPO), "label": args.label,
              "csr": r1cs.csr_info(), "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        with ctx.r1cs_rows(r1cs) as rows, ctx.r1cs_cols(r1cs) as cols:
            for batch in batches:
                out, bad = measure(ctx, r1cs, rows, cols, np.ascontiguousarray(W_all[:batch]), batch, args.reps)
                result["shapes"].append(out)
                failed += bad
    result["fused_slower_beyond_both_iqrs_anywhere"] = any(s["fused_slower_beyond_both_iqrs"] for s in result["shapes"])
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

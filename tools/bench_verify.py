"""Host verifier against device verifier, same process, same proofs: gkr_verify (threads = 0: every CPU the process may use)
alternating with gkr_verify_prepared on a warm handle, on

    wide      k = [18, 20, 20]  (synth.wide_circuit: what bench.py's wide_prove leg proves), one proof
    circom    the circom-shaped (20, 20) layer of synth.circom_shaped_layer as a one-layer circuit, one proof
    demo64    the demo circuit (three-input MiMC7 R1CS, compiled): its largest sub-circuit, the 64 proofs of bench.py's inputs

Per circuit: a warm-up of each, then --reps alternating repetitions; medians and spread (the interquartile range and min / max)
of both; gkr_verify_prepare timed once; a plain host-to-device upload of as many bytes as a gkr_verify_prepared call uploads,
timed the same way.  Every timed verdict of the device verifier is compared with the host's.  The result goes to
profiles/r07/verify_device.json (or --out).

The floor a gkr_verify_prepared call cannot beat = its upload at the measured upload rate + the sum of its kernels' times; the
kernel times come from a rocprofv3 run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o verify -- python tools/bench_verify.py --trace-calls 5 --only wide
    python tools/bench_verify.py --kernel-stats DIR/.../verify_kernel_stats.csv --kernel-stats-calls 6

(--trace-calls N: no timing, no host verifier; one warm-up and N gkr_verify_prepared calls, i.e. N + 1 calls in the trace.)

Where the challenge hashes run (context option verify_device_hash_min; -1: the context's host threads, 1: the device):

    --hash host | device   gkr_verify_prepared is timed under that setting
    --hash both            under both, alternating in the same repetitions ("gkr_verify_prepared" is the host setting, the path
                           without the option; "gkr_verify_prepared_device_hash" the device setting)
    --sweep                (needs --hash both) the demo circuit's proofs, tiled or cut to batch = 1, 2, 4, ... --sweep-max, both
                           settings alternating; per point medians and interquartile ranges, and from them the default
                           threshold: the smallest row count from which on, at EVERY larger point, the device median is below
                           the host median by more than the sum of the two interquartile ranges, rounded up to a power of two
                           (null: there is no such point -- the default is "never")
    --trace-calls N --trace-batch B   the demo circuit at batch B under --hash device|host, for a rocprofv3 run of its own

With --hash the result goes to profiles/r08/verify_device_hash.json."""

import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gkr_amd import Context, GKRCircuit, synth  # noqa: E402
from gkr_amd.dropin import verify_native  # noqa: E402
from gkr_amd.field import as_limbs  # noqa: E402

VERIFY_KERNELS = ("k_verify_", "k_eq_table", "k_check_canonical")


def workloads(only):
    if only in (None, "wide"):
        circuit, _, wit = synth.wide_circuit()
        yield "wide", circuit, np.ascontiguousarray(wit)
    if only in (None, "circom"):
        lay, _, W = synth.circom_shaped_layer(20, 20)
        yield "circom", GKRCircuit([lay], 20), np.ascontiguousarray(W[None])
    if only in (None, "demo64"):
        from gkr_amd.aggregate import ProvingStep
        step = ProvingStep(synth.mimc7_demo_r1cs())
        inputs = step.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(a, b)) for a, b in synth.demo_proof_inputs(64)]))
        j = max(range(len(step.circuits)), key=lambda i: sum(1 << k for k in step.circuits[i].get_k_list()))
        yield "demo64", step.circuits[j], np.ascontiguousarray(inputs[j])


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def upload_bytes(ks):
    """Bytes of one proof a gkr_verify_prepared call sends to the device: z, the challenges, d_coeffs, input_coeffs."""
    L = len(ks) - 1
    return 32 * (sum(ks) + sum(2 * ks[i + 1] for i in range(L)) + (1 << ks[0]) + (1 << ks[-1]))


def kernel_ms_per_call(path, calls):
    """Sum of the verifier's kernels in a rocprofv3 --stats CSV, per gkr_verify_prepared call."""
    total_ns, rows = 0.0, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            if any(tag in name for tag in VERIFY_KERNELS):
                total_ns += ns
                short = name.split("(")[0].split("::")[-1]
                rows[short] = rows.get(short, 0.0) + ns / 1e6 / calls
    return total_ns / 1e6 / calls, rows


def hash_settings(which):
    """[(key in the result, value of verify_device_hash_min or None: the library's default)]"""
    if which is None:
        return [("gkr_verify_prepared", None)]
    if which == "host":
        return [("gkr_verify_prepared", -1)]
    if which == "device":
        return [("gkr_verify_prepared_device_hash", 1)]
    return [("gkr_verify_prepared", -1), ("gkr_verify_prepared_device_hash", 1)]


def with_batch(arrs, batch):
    """The proofs of `arrs` tiled or cut to `batch` proofs."""
    B = arrs[0].shape[0]
    reps = -(-batch // B)
    return [np.ascontiguousarray(np.concatenate([a] * reps, axis=0)[:batch]) for a in arrs]


def derive_threshold(points):
    """points: [(rows, host spread, device spread)] ascending -> (threshold rows or None, the first row count of the winning tail)"""
    first = None
    for rows, h, d in reversed(points):
        if h["median_ms"] - d["median_ms"] > h["iqr_ms"] + d["iqr_ms"]:
            first = rows
        else:
            break
    if first is None:
        return None, None
    return 1 << (first - 1).bit_length(), first


def sweep(ctx, handle, circuit, arrs, args):
    rounds = arrs[0].shape[1]
    out, points = [], []
    mismatches = 0
    base = [verify_native(circuit, arrs, index=b, threads=0) for b in range(arrs[0].shape[0])]
    batch = 1
    while batch <= args.sweep_max:
        proofs = with_batch(arrs, batch)
        want = (base * (-(-batch // len(base))))[:batch]
        times = {-1: [], 1: []}
        for setting in (-1, 1):                                # (the warm-up of both)
            ctx.set_option("verify_device_hash_min", setting)
            mismatches += ctx.verify_batch(handle, proofs) != want
        for _ in range(args.reps):
            for setting in (-1, 1):
                ctx.set_option("verify_device_hash_min", setting)
                ms, got = timed(lambda: ctx.verify_batch(handle, proofs))
                times[setting].append(ms)
                mismatches += got != want
        ctx.set_option("verify_device_hash_min", 0)
        h, d = spread(times[-1]), spread(times[1])
        rows = batch * rounds
        point = {"batch": batch, "rows": rows, "host_hash": h, "device_hash": d,
                 "device_wins_beyond_spread": h["median_ms"] - d["median_ms"] > h["iqr_ms"] + d["iqr_ms"]}
        out.append(point)
        points.append((rows, h, d))
        print("sweep", json.dumps(point), flush=True)
        batch *= 2
    threshold, first = derive_threshold(points)
    return {"points": out, "rows_per_proof": rounds, "threshold_rows": threshold, "first_winning_rows": first,
            "rule": "smallest rows from which on every larger point has host median - device median > host IQR + device IQR; "
                    "rounded up to a power of two; null: never"}, mismatches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["wide", "circom", "demo64"])
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel stats CSV of a --trace-calls run of `wide`")
    ap.add_argument("--kernel-stats-calls", type=int, default=6, help="gkr_verify_prepared calls in that trace (--trace-calls + 1)")
    ap.add_argument("--hash", choices=["host", "device", "both"], help="where gkr_verify_prepared hashes (verify_device_hash_min = -1 / 1)")
    ap.add_argument("--sweep", action="store_true", help="batch sweep of the demo circuit under both settings (with --hash both)")
    ap.add_argument("--sweep-max", type=int, default=4096)
    ap.add_argument("--trace-batch", type=int, default=0, help="with --trace-calls: the demo circuit's proofs tiled or cut to this batch")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 20 and not args.trace_calls:
        ap.error("at least 20 repetitions")
    if args.sweep and args.hash != "both":
        ap.error("--sweep compares the two settings: --hash both")
    if args.trace_calls and args.hash == "both":
        ap.error("a trace is of one setting: --hash host or --hash device")
    if args.trace_batch:
        args.only = "demo64"
    if not args.out:
        args.out = os.path.join(REPO, "profiles", *(("r08", "verify_device_hash.json") if args.hash else ("r07", "verify_device.json")))
    settings = hash_settings(args.hash)
    result = {"tool": "tools/bench_verify.py", "host_threads": 0, "hash": args.hash, "circuits": {}}
    mismatches = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        for name, circuit, wit in workloads(args.only):
            ks = circuit.get_k_list()
            B = wit.shape[0]
            arrs = [a.copy() for a in ctx.prove_batch_raw(circuit, wit, all_arrays=True)]
            prepare_ms, handle = timed(lambda: ctx.prepare_verify(circuit))
            if args.trace_calls:
                if settings[0][1] is not None:
                    ctx.set_option("verify_device_hash_min", settings[0][1])
                proofs = with_batch(arrs, args.trace_batch) if args.trace_batch else arrs
                for _ in range(args.trace_calls + 1):
                    ctx.verify_batch(handle, proofs)
                handle.close()
                continue
            host = lambda: [verify_native(circuit, arrs, index=b, threads=0) for b in range(B)]   # noqa: E731

            def dev(setting):
                if setting is not None:
                    ctx.set_option("verify_device_hash_min", setting)
                return ctx.verify_batch(handle, arrs)
            want = host()
            for _, setting in settings:
                assert dev(setting) == want, (name, want)      # (the warm-up of all)
            t_host, t_devs = [], {key: [] for key, _ in settings}
            for _ in range(args.reps):
                ms, got = timed(host)
                t_host.append(ms)
                mismatches += got != want
                for key, setting in settings:
                    ms, got = timed(lambda: dev(setting))
                    t_devs[key].append(ms)
                    mismatches += got != want
            if args.hash:
                ctx.set_option("verify_device_hash_min", 0)
            t_dev = t_devs[settings[0][0]]
            sweep_result = None
            if args.sweep and name == "demo64":
                sweep_result, bad = sweep(ctx, handle, circuit, arrs, args)
                mismatches += bad
            handle.close()
            # a plain upload of the same bytes (pageable host memory, as the caller's proof buffers are)
            nbytes = upload_bytes(ks) * B
            blob = np.frombuffer(np.random.default_rng(1).bytes(nbytes), dtype=np.uint8)
            dptr = ctx.alloc(nbytes)
            ctx.upload(dptr, blob)
            t_up = []
            for _ in range(args.reps):
                ms, _ = timed(lambda: ctx.upload(dptr, blob))
                t_up.append(ms)
            ctx.free(dptr)
            h, d, u = spread(t_host), spread(t_dev), spread(t_up)
            row = {"k": ks, "batch": B, "all_accepted": all(v == (True, 0, 0) for v in want), "gkr_verify": h, "gkr_verify_prepared": d,
                   "gkr_verify_prepare_once_ms": prepare_ms, "upload_bytes": nbytes, "plain_upload": u,
                   "upload_GBps": nbytes / 1e6 / u["median_ms"], "host_over_device": h["median_ms"] / d["median_ms"],
                   "device_wins_beyond_spread": h["median_ms"] - d["median_ms"] > max(h["iqr_ms"], d["iqr_ms"]),
                   "kernel_ms_per_call": "not measured", "floor_ms": "not measured", "floor_over_measured": "not measured"}
            if name == "wide" and args.kernel_stats:
                km, rows = kernel_ms_per_call(args.kernel_stats, args.kernel_stats_calls)
                row.update({"kernel_ms_per_call": km, "kernels_ms": rows, "floor_ms": u["median_ms"] + km,
                            "floor_over_measured": (u["median_ms"] + km) / d["median_ms"]})
            for key, _ in settings[1:]:
                row[key] = spread(t_devs[key])
            if args.hash:
                row["rows"] = B * sum(2 * ks[i + 1] for i in range(len(ks) - 1))
                row[settings[0][0]] = d
                if settings[0][0] != "gkr_verify_prepared":   # (--hash device: the row's comparisons are of that setting)
                    del row["gkr_verify_prepared"]
            if sweep_result:
                result["demo_batch_sweep"] = sweep_result
            result["circuits"][name] = row
            print(name, json.dumps(row), flush=True)
    if args.trace_calls:
        return 0
    result["verdict_mismatches"] = int(mismatches)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    return 1 if mismatches else 0


if __name__ == "__main__":
    sys.exit(main())

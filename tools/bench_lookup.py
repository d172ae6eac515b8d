"""The lookup's preparation (gkr_lookup_multiplicities_device, the pair build of gkr_lookup_batch_device) at n_w = n_t = 20 (--n),
at batch 1 and at batch 16 with a shared table (--batches), in one process, for two witnesses: `uniform` (every entry drawn
uniformly from the table) and `repeated` (one table value in every entry: every lane on one counter).

Before anything is timed: the table's values are distinct, the device's multiplicities are numpy's count of the drawn indices, the
misses are none, the pair's entries are held to Python integers at both ends of both sides, the proofs have P = 0 and the device
verifier accepts them; every timed call must return the first call's bytes (the multiplicities) or sums (the proofs).  Then --reps
repetitions under the context profile, everything reported as median and spread (interquartile range, min / max) of device time:

  build       the index build (`lk_build`)                 count       the count (`lk_count`)
  mult        counters -> elements (`lk_mult`)              pair        the pair build (`lk_pair`)
  fraction_sum   gkr_fraction_sum_batch_device on the same pair (host clock, --fs-reps calls), the call the preparation stands in front of
  byte_floor  one read of W and T and one write of M, N and D at the box's copy rate (gkr_ubench_ceilings, measured in this process)

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
from gkr_amd import MODULUS, Context, from_limbs, to_limbs  # noqa: E402
from gkr_amd import _native as N  # noqa: E402


def spread(samples_ms):
    s = sorted(samples_ms)
    q = statistics.quantiles(s, n=4) if len(s) >= 4 else [s[0], s[len(s) // 2], s[-1]]
    return {"median_ms": statistics.median(s), "iqr_ms": q[2] - q[0], "min_ms": s[0], "max_ms": s[-1], "reps": len(s)}


def at(d, elements):
    return ctypes.c_void_p(d.value + 32 * elements)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fs-reps", type=int, default=3)
    ap.add_argument("--batches", default="1,16", help="batch sizes, comma-separated; above 1 the table is shared")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--out")
    args = ap.parse_args()
    n, size, L = args.n, 1 << args.n, args.n + 1
    result = {"tool": "tools/bench_lookup.py", "n_w": n, "n_t": n, "L": L, "shapes": []}
    failed = 0
    rng = np.random.default_rng(20261021)
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        for batch in [int(b) for b in args.batches.split(",")]:
            d_t, d_w, d_m, d_p = ctx.alloc(32 * size), ctx.alloc(32 * batch * size), ctx.alloc(32 * batch * size), ctx.alloc(64 * batch * (1 << L))
            try:
                ctx.fill_table(d_t, size, 0x100C + batch)
                T = ctx.download(d_t, (size, 4))
                distinct = len(np.unique(T.view([("", T.dtype)] * 4))) == size     # distinct values: the count of the drawn indices is M
                alphas = [int(x) for x in rng.integers(1, 1 << 62, size=batch)]    # (the table's values are 254-bit: none is that small)
                a_limbs = to_limbs(alphas)
                for witness in ("uniform", "repeated"):
                    ok = distinct
                    idx = rng.integers(0, size, size=(batch, size)) if witness == "uniform" else np.repeat(rng.integers(0, size, size=(batch, 1)), size, axis=1)
                    for b in range(batch):
                        ctx.upload(at(d_w, b * size), T[idx[b]])
                    want = np.stack([np.bincount(idx[b], minlength=size) for b in range(batch)]).astype(np.uint64)
                    count = lambda: ctx.lookup_multiplicities_device(d_w, n, d_t, n, True, batch, d_m)
                    missing, first = count()                       # warm-up
                    M = ctx.download(d_m, (batch, size, 4))
                    ok = ok and not missing.any() and (first == 0xFFFFFFFF).all() and np.array_equal(M[:, :, 0], want) and not M[:, :, 1:].any()
                    pair = lambda: ctx._check(N.lib().gkr_devtest_lookup_pair(ctx._h, d_w, n, d_t, n, 1, d_m, a_limbs.ctypes.data, batch, d_p))
                    pair()
                    for b in sorted({0, batch - 1}):               # both ends of both sides of the pair, on Python integers
                        for side, src, first_e in (("w", T[idx[b]], 0), ("t", T, size)):
                            for lo in (0, size - 4):
                                got_n = from_limbs(ctx.download(at(d_p, b * (2 << L) + first_e + lo), (4, 4)))
                                got_d = from_limbs(ctx.download(at(d_p, b * (2 << L) + (1 << L) + first_e + lo), (4, 4)))
                                vals = from_limbs(src[lo:lo + 4])
                                want_n = [1] * 4 if side == "w" else [(-int(m)) % MODULUS for m in want[b, lo:lo + 4]]
                                ok = ok and got_n == want_n and got_d == [(alphas[b] - v) % MODULUS for v in vals]
                    prove = lambda out=None: ctx.fraction_sum_batch_device(d_p, L, batch, out=out)
                    first_proof = prove()
                    whole = ctx.lookup_batch_device(d_w, n, d_t, n, True, d_m, alphas, batch)
                    ok = ok and all(a.tobytes() == b.tobytes() for a, b in zip(first_proof, whole))
                    ok = ok and not first_proof[0][:, 0].any() and bool(first_proof[0][:, 1].any(axis=-1).all())
                    ok = ok and bool(ctx.verify_lookup_batch_device(d_w, n, d_t, n, True, d_m, alphas, batch, *first_proof[1:6])[0].all())
                    t = {k: [] for k in ("lk_build", "lk_count", "lk_mult", "lk_pair")}
                    ctx.profile(1)
                    for _ in range(args.reps):
                        ctx.profile_reset()
                        count()
                        pair()
                        for k in t:
                            t[k].append(ctx.profile_get(k)["total_ms"])
                    ctx.profile(0)
                    ok = ok and np.array_equal(ctx.download(d_m, (batch, size, 4)), M)
                    t_fs, out = [], tuple(np.zeros_like(a) for a in first_proof)
                    for _ in range(args.fs_reps):
                        t0 = time.perf_counter()
                        got = prove(out)
                        t_fs.append((time.perf_counter() - t0) * 1e3)
                        ok = ok and np.array_equal(got[0], first_proof[0])
                    s = {k: spread(v) for k, v in t.items()}
                    fs = spread(t_fs)
                    prep = sum(s[k]["median_ms"] for k in s)
                    floor_bytes = 32.0 * size * (1 + batch) + 32.0 * batch * size + 64.0 * batch * (1 << L)    # read T, W; write M; write N, D
                    floor_ms = floor_bytes / (ceil["copy_GBps"] * 1e6)
                    result["shapes"].append({
                        "batch": batch, "witness": witness, "checked": "ok" if ok else "FAILED", "build": s["lk_build"], "count": s["lk_count"],
                        "mult": s["lk_mult"], "pair": s["lk_pair"], "preparation_ms": prep, "fraction_sum": fs,
                        "preparation_over_fraction_sum": prep / fs["median_ms"], "byte_floor_ms": floor_ms, "byte_floor_bytes": floor_bytes,
                        "preparation_over_byte_floor": prep / floor_ms})
                    failed += int(not ok)
            finally:
                for p in (d_t, d_w, d_m, d_p):
                    ctx.free(p)
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

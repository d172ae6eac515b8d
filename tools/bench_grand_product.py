"""The grand product (gkr_grand_product_batch_device) at n = 20, batch in {1, 64} (--batches), in one process.  The tables are
filled on the device; before anything is timed P is held to the product of the downloaded tables' Python integers (every table at
batch 1, the first and the last otherwise), every layer of sumcheck 0 to a direct zero-check call, and the device verifier must
accept; every timed call must return the first call's bytes.  Then --reps alternating repetitions, everything reported as median
and spread (interquartile range, min / max):

  tree        the tree's launches alone (gkr_devtest_grand_product_tree under the context profile: device time of the `gp_tree`
              bracket) against two floors of this box, measured in this process (gkr_ubench_ceilings): one read and one write of
              2^n * 32 bytes per table at the copy rate, and 2^n - 1 modular products per table at the product rate (a product
              of two canonical values is two of the rate's Montgomery products: both figures are given);
  other_tree  with --other-lib PATH: the same tree launches of ANOTHER build of the library (a second source state loaded beside
              this one: levels fused in registers at some depth), alternating with this build's on the same tables and checked to
              give the same bytes -- how the one-launch-per-level form was chosen over the fused ones (profiles/r27);
  sumchecks   the whole call minus its tree (host clock around calls that end in a device synchronise) against the sum of the
              zero-check calls on the same layers from this script (the levels come from the devtest tree; the points are the
              call's own), in the same run: the driver adds the host's tau, c and z between layers;
  verify      gkr_grand_product_verify_batch_device against a bare gkr_mle_eval_batch_device on the same tables and points.

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
from gkr_amd import MODULUS, Context, from_limbs, multi_hash  # noqa: E402
from gkr_amd import _native as N  # noqa: E402

TERMS = [(1, (0, 1))]


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


class OtherBuild:
    """Another build of the library beside this one, as far as the tree's launches go: a context of its own on the same device."""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.h = ctypes.c_void_p()
        self.lib.gkr_devtest_grand_product_tree.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
        self.lib.gkr_ctx_profile_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p] + [ctypes.c_void_p] * 3
        self.lib.gkr_ctx_destroy.argtypes = [ctypes.c_void_p]
        for fn in (self.lib.gkr_ctx_profile, self.lib.gkr_ctx_profile_reset):
            fn.argtypes = [ctypes.c_void_p] + ([ctypes.c_int] if fn is self.lib.gkr_ctx_profile else [])
        assert self.lib.gkr_ctx_create(ctypes.c_int(0), ctypes.byref(self.h)) == 0
        assert self.lib.gkr_ctx_profile(self.h, 1) == 0

    def tree_ms(self, d_tables, n, batch, d_layers):
        assert self.lib.gkr_ctx_profile_reset(self.h) == 0
        assert self.lib.gkr_devtest_grand_product_tree(self.h, d_tables, n, batch, d_layers) == 0
        launches, ms, nbytes = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double()
        assert self.lib.gkr_ctx_profile_get(self.h, b"gp_tree", ctypes.byref(launches), ctypes.byref(ms), ctypes.byref(nbytes)) == 0
        return ms.value

    def close(self):
        self.lib.gkr_ctx_destroy(self.h)


def tree_ms(ctx, d_tables, n, batch, d_layers):
    ctx.profile_reset()
    ctx._check(N.lib().gkr_devtest_grand_product_tree(ctx._h, d_tables, n, batch, d_layers))
    return ctx.profile_get("gp_tree")["total_ms"]


def python_product(ctx, d_tables, n, b):
    t = np.array(from_limbs(ctx.download(ctypes.c_void_p(d_tables.value + (32 << n) * b), (1 << n, 4))), dtype=object)
    while len(t) > 1:
        t = t[:len(t) // 2] * t[len(t) // 2:] % MODULUS
    return int(t[0])


def layer_points(out, n, batch):
    """z^(k) of every sumcheck for k = 2 .. n - 1 from the call's head, challenges and values (the chain of the header)."""
    H, R, E = out[1], out[4], out[5]
    zs = []
    for b in range(batch):
        z1 = multi_hash(from_limbs(H[b]), 0)
        zs.append([z1, multi_hash([z1], 0)])
    points = [zs]
    for k in range(2, n - 1):
        row = k * (k - 1) // 2 - 1
        zs = [[multi_hash(from_limbs(E[b, k - 2]), 0)] + from_limbs(R[b, row:row + k]) for b in range(batch)]
        points.append(zs)
    return points


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batches", default="1,64", help="batch sizes, comma-separated")
    ap.add_argument("--ceiling-bytes", type=int, default=2 << 30)
    ap.add_argument("--other-lib", help="another build of libgkr_amd.so whose tree launches are timed in alternation")
    ap.add_argument("--other-name", default="other", help="what the other build is, for the record")
    ap.add_argument("--out")
    args = ap.parse_args()
    n, size = args.n, 32 << args.n
    result = {"tool": "tools/bench_grand_product.py", "n": n, "rounds": n * (n - 1) // 2 - 1, "shapes": []}
    failed = 0
    with Context(0) as ctx:
        result["device"] = ctx.device_name()
        result["cpus"] = len(os.sched_getaffinity(0))
        geometry = np.zeros(n, dtype=np.uint32)
        ctx._check(N.lib().gkr_selftest_grand_product_geometry(n, geometry.ctypes.data))
        result["tree_blocks_per_level"] = [int(x) for x in geometry]
        ceil = result["ceilings"] = ctx.ceilings(args.ceiling_bytes)
        other = OtherBuild(args.other_lib) if args.other_lib else None
        for batch in [int(b) for b in args.batches.split(",")]:
            total = batch * ((1 << n) - 1)
            d, lay, lay2 = ctx.alloc(batch * size), ctx.alloc(32 * total), ctx.alloc(32 * total)
            try:
                ctx.fill_table(d, batch << n, 0xC0FFEE + batch)
                run = lambda out=None: ctx.grand_product_batch_device(d, n, batch, out=out)
                first = run()                                     # warm-up
                ok = all(from_limbs(first[0][b:b + 1])[0] == python_product(ctx, d, n, b) for b in sorted({0, batch - 1}))
                verify = lambda: ctx.verify_grand_product_batch_device(d, n, batch, *first[1:6], products=first[0])
                ok = ok and bool(verify()[0].all())
                evaluate = lambda: ctx.mle_eval_batch_device(d, n, batch, first[6])
                ok = ok and evaluate().tobytes() == first[7].tobytes()            # c_n = V~(z^(n)), from the evaluation alone
                ctx.profile(1)
                tree_ms(ctx, d, n, batch, lay)
                ctx.profile(0)
                points = layer_points(first, n, batch)
                src = lambda k: d if k + 1 == n else ctypes.c_void_p(lay.value + 32 * batch * ((1 << (k + 1)) - 1))
                layer_outs = [None] * n

                def layers():
                    for k in range(2, n):
                        layer_outs[k] = ctx.sumcheck_zerocheck_batch_device(src(k), k, 2, TERMS, batch, points[k - 2], out=layer_outs[k])
                layers()                                          # warm-up, and the check of every layer of every sumcheck
                for k in range(2, n):
                    row = k * (k - 1) // 2 - 1
                    ok = ok and layer_outs[k][0].tobytes() == first[2][:, row:row + k].tobytes() and layer_outs[k][2].tobytes() == first[4][:, row:row + k].tobytes()
                    ok = ok and layer_outs[k][3].tobytes() == first[5][:, k - 2].tobytes()
                out = tuple(np.zeros_like(a) for a in first)
                t_call, t_layers, t_verify, t_eval = [], [], [], []
                for _ in range(args.reps):
                    ms, got = timed(lambda: run(out))
                    t_call.append(ms)
                    ok = ok and all(np.array_equal(a, b) for a, b in zip(got, first))
                    t_layers.append(timed(layers)[0])
                    ms, got = timed(verify)
                    t_verify.append(ms)
                    ok = ok and bool(got[0].all())
                    t_eval.append(timed(evaluate)[0])
                ctx.profile(1)
                t_tree, t_other = [], []
                for _ in range(args.reps):
                    t_tree.append(tree_ms(ctx, d, n, batch, lay))
                    if other:
                        t_other.append(other.tree_ms(d, n, batch, lay2))
                ctx.profile(0)
                if other:                                         # the two builds' levels, byte for byte (a slice at a time)
                    step = 1 << 24
                    for at in range(0, total, step):
                        count = min(step, total - at)
                        a = ctx.download(ctypes.c_void_p(lay.value + 32 * at), (count, 4))
                        ok = ok and a.tobytes() == ctx.download(ctypes.c_void_p(lay2.value + 32 * at), (count, 4)).tobytes()
            finally:
                for p in (d, lay, lay2):
                    ctx.free(p)
            failed += int(not ok)
            tree, call, lays, ver, ev = spread(t_tree), spread(t_call), spread(t_layers), spread(t_verify), spread(t_eval)
            sumchecks = spread([c - tree["median_ms"] for c in t_call])
            byte_floor_ms = batch * 2.0 * size / (ceil["copy_GBps"] * 1e6)
            product_floor_ms = batch * ((1 << n) - 1) / ceil["modmul_per_sec"] * 1e3
            shape = {"batch": batch, "checked": "ok" if ok else "FAILED", "call": call, "tree": tree,
                     "tree_floors": {"byte_floor_ms": byte_floor_ms, "product_floor_ms": product_floor_ms, "montgomery_floor_ms": 2.0 * product_floor_ms,
                                     "tree_over_byte_floor": tree["median_ms"] / byte_floor_ms, "tree_over_product_floor": tree["median_ms"] / product_floor_ms,
                                     "tree_over_montgomery_floor": tree["median_ms"] / (2.0 * product_floor_ms)},
                     "sumchecks_of_the_call": sumchecks, "zerocheck_calls_on_the_layers": lays, "sumchecks_over_zerocheck_calls": compare(sumchecks, lays),
                     "verify": ver, "mle_eval": ev, "verify_over_mle_eval": compare(ver, ev), "table_bytes": batch * size}
            if other:
                shape["other_tree"] = dict(spread(t_other), name=args.other_name)
                shape["tree_over_other_tree"] = compare(tree, shape["other_tree"])
            result["shapes"].append(shape)
        if other:
            other.close()
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

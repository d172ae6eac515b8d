#!/usr/bin/env python3
"""Headline benchmark: BN254-Fr sumcheck field-ops/sec on 2^20-point multilinear tables (BASELINE.json metric,
configs[2]) and aggregated proofs/sec (configs[0] / configs[3]), one process per GPU.

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W [--mode mle|proofs|layer-split]

--mode mle (default): a step = one pass of the hot path over one batch: `--batch` (default 1024, 32 GiB of tables)
    independent 2^n-point multilinear sumchecks (prove_sumcheck, rust/src/gkr/sumcheck.rs:158-214), tables resident
    in HBM before the timed region, MiMC7 transcript included.  Independent sumchecks shard across ranks with no
    data-path collective (weak scaling: every rank proves its own batch).  The same line carries, on every rank's
    own share and MAX-reduced over ranks, `aggregated_proofs`: the R1CS of rust/t.circom (hand-written equivalent)
    compiled to its 12 layered circuits and proven for 3 and for 64 inputs (configs[0], configs[3]).
--mode proofs: configs[3] as its own timed workload: `--proofs` inputs of the demo circuit split over the ranks
    (strong scaling; no collective), a step = every rank proving its share of the inputs, all 12 sub-circuits.
--mode layer-split: configs[4]: ONE GKR layer (k_i = 24, k = 12: 2^24 gates, 2^24-point hypercube) split over the
    ranks by gates, two sum-over-ranks exchanges (RCCL all-reduce of limb-widened field elements) per sumcheck
    (gkr_sumcheck_layer_sharded); a step = one layer sumcheck; strong scaling.

--mode mle-split: BASELINE's "within one proof, disjoint hypercube halves shard across the GPUs": ONE 2^n-point table
    (--n 20, or 30) split over the ranks, one RCCL all-reduce per pass of up to five rounds + one gather per sumcheck
    (gkr_sumcheck_mle_sharded_dev); a step = --split-batch sumchecks; strong scaling.

field-ops: 5 (2^n - 1) per plain sumcheck, 25 (2^{2k} - 1) per layer sumcheck; algorithmic bytes 128 * 2^n
(SURVEY.md section 8d).

A plain run of --mode mle sets up, warms up, times the K steps and prints the headline line (the contract keys, the
step times); nothing else.  --full adds the rest: the timed steps with the per-kernel HIP events,
the check of the timed outputs, and every other leg (batch-1 latency, n16, configs[0] / [3] / [4], the wide layers,
the split legs on N > 1, large_r1cs, multi_device).  With --full the JSON line also carries
  roofline       the dominant kernel (k_mle_multifold_mfma, the fold pass) timed with HIP events on the library's
                 stream during the timed steps (profile level 2: only the bandwidth-bound kernels carry events)
  cpu_baseline   the plain-C oracle (oracle/c), one sumcheck per host core, on a bounded sample of the same
                 workload; rank 0, N = 1 only; plus cpu_ref_algo (the reference's term-list algorithm restated,
                 largest size under its time cap) and cpu_pipeline (the oracle proving the demo circuit)
The other modes run as they always did; --full changes nothing there.

--dump-outputs DIR: after the timed steps, rank 0 writes the arrays the timed path returned in its last step as
DIR/<name>.npy, float64 (see dump_outputs): --mode mle and mle-split coeffs / lengths / challenges (the C ABI's
C, L, R), layer-split the same for the layer sumcheck, proofs c<j>_<field> for sub-circuit j and every field of
gkr_proof_buf.  The inputs are seeded: the same arguments give the same arrays.
"""

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_GBPS = 8000.0   # MI355X HBM3E (MI355X_MICROARCH.md; measured copy ceiling 6.29 TB/s)
# The chip's rate of dependent 254-bit Montgomery products on v_mad_u64_u32 chains (16 waves per SIMD), as a CONSTANT: what
# gkr_ubench_ceilings measured on every box of rounds 3-6 (1.184 - 1.199 * 10^11).  The legs bound by it quote their fraction
# of this figure beside the fraction of what the box of the run itself measures, so that a slow box does not lower the bar.
PEAK_PRODUCTS_PER_SEC = 1.19e11


def usable_cpus():
    """Affinity mask capped by the cgroup CPU quota (the GPU box runs this in a container with cpu.max = 16 CPUs
    although 256 are visible)."""
    n = len(os.sched_getaffinity(0))
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p))))
    except Exception:
        pass
    return n


class World:
    """The ranks of this job: process group first, GPU second."""

    def __init__(self):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.size = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # test hooks (single-GPU boxes): several ranks on one device over gloo exercise the N > 1 code path
        self.backend = os.environ.get("GKR_BENCH_BACKEND", "nccl")
        if "GKR_BENCH_DEVICE" in os.environ:
            self.local_rank = int(os.environ["GKR_BENCH_DEVICE"])
        # GKR_BENCH_FORCE_GROUP=1: a process group (and with it RCCL) also for one rank, so that the exchange path of
        # --mode layer-split runs as it does on N GPUs (one MI355X is all a builder's box has)
        self.grouped = self.size > 1 or os.environ.get("GKR_BENCH_FORCE_GROUP") == "1"
        # eight ranks must never silently share one GPU: a rank's device is its LOCAL_RANK, and it has to exist
        # (device_count does not initialise the GPU).  Only the single-device test hook above may lift this.
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(self.size)) or self.size)
        if self.size > 1 and "GKR_BENCH_DEVICE" not in os.environ and torch.cuda.device_count() < local_world:
            raise SystemExit("bench.py: %d local ranks but %d visible device(s); one process per GPU is the contract "
                             "(GKR_BENCH_DEVICE=<id> with GKR_BENCH_BACKEND=gloo is the single-device test hook)"
                             % (local_world, torch.cuda.device_count()))
        if self.grouped:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29500")
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            if self.backend == "nccl":   # the process group comes first, the first GPU call after it
                dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank))
                torch.cuda.set_device(self.local_rank)
            else:
                dist.init_process_group(self.backend)
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (no GPU visible); there is no CPU fallback")
        self.device = "cuda" if self.backend == "nccl" else "cpu"

    def barrier(self, ctx=None):
        if self.grouped:
            self.dist.barrier()
        self.torch.cuda.synchronize()
        if ctx is not None:
            ctx.synchronize()

    def max_over_ranks(self, seconds):
        if self.size == 1:
            return seconds
        t = self.torch.tensor([seconds], dtype=self.torch.float64, device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def per_rank(self, value):
        """[value of rank 0, value of rank 1, ...] on every rank (one all-reduce of a vector with one slot per rank)."""
        if self.size == 1:
            return [value]
        t = self.torch.zeros(self.size, dtype=self.torch.float64, device=self.device)
        t[self.rank] = float(value)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return [float(x) for x in t.tolist()]

    def close(self):
        if self.grouped:
            self.dist.destroy_process_group()


def transcript_threads():
    """Host threads a context's transcript uses by default (gkr_capi.hip, default_host_threads): the rank's share of the
    usable CPUs, two (one, none) of them left to the runtime's own threads."""
    if os.environ.get("GKR_HOST_THREADS", "").isdigit() and int(os.environ["GKR_HOST_THREADS"]) >= 1:
        return int(os.environ["GKR_HOST_THREADS"])
    share = usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1") or 1))
    return max(1, min(64, share - 2 if share >= 6 else (share - 1 if share >= 3 else share)))


def transcript_floor(hashed_elements, vector_len, threads, achieved_ms):
    """The bound of a leg whose step time is the host's MiMC7 hashing: every round vector of every sumcheck is hashed
    once (Mimc7::multi_hash, sumcheck.rs:84,129,152: 91 rounds per element), the hashes of one sumcheck are a serial
    chain, those of different sumchecks are independent.  floor = hashed elements x the measured time per element on
    one thread (sixteen transcripts in IFMA lanes, measured now on this host) / threads."""
    import threading
    from gkr_amd.prover import host_hash_us
    lanes16, scalar = host_hash_us(vector_len)
    per_elem = (lanes16 if lanes16 > 0 else scalar) / vector_len
    floor_ms = hashed_elements * per_elem / threads / 1e3
    # The same micro-benchmark on ALL the leg's threads at once: what a thread's sixteen-lane hash takes while its neighbours
    # hash too (AVX-512 clocks, shared caches, the cgroup's quota) -- the rate the step can really draw on.  Beside, not
    # instead of, the one-thread figure `frac` is quoted against.
    loaded = []
    if lanes16 > 0 and threads > 1:
        gate = threading.Barrier(threads)

        def busy():
            gate.wait()
            mine = [host_hash_us(vector_len)[0] for _ in range(3)]
            loaded.append(statistics.median(mine))
        workers = [threading.Thread(target=busy) for _ in range(threads)]
        [w.start() for w in workers]
        [w.join() for w in workers]
    loaded_us = statistics.median(loaded) if loaded else None
    loaded_floor = hashed_elements * (loaded_us / vector_len) / threads / 1e3 if loaded_us else None
    return {"bound": "host transcript (MiMC7 hashing throughput of the host cores)", "hashed_elements_per_step": int(hashed_elements),
            "us_per_hash_16_lanes": lanes16, "us_per_hash_scalar": scalar, "vector_len_timed": vector_len, "threads": threads,
            "floor_ms": floor_ms, "achieved_ms": achieved_ms, "achieved_over_floor": achieved_ms / floor_ms if floor_ms else None,
            "frac": floor_ms / achieved_ms if achieved_ms else None,
            "us_per_hash_16_lanes_all_threads_hashing": loaded_us, "floor_ms_all_threads_hashing": loaded_floor,
            "frac_of_the_loaded_floor": loaded_floor / achieved_ms if loaded_floor and achieved_ms else None}


def guarded(fn, seconds):
    """fn() on a worker thread with a deadline -> (result, error text or None, still running)."""
    import threading
    box = {}

    def work():
        try:
            box["out"] = fn()
        except BaseException as e:   # noqa: BLE001 -- reported on the line
            box["err"] = "%s: %s" % (type(e).__name__, e)
    t = threading.Thread(target=work, daemon=True)
    t.start()
    t.join(seconds)
    if t.is_alive():
        return None, "no result after %d s (a rank may be stuck in a collective)" % seconds, True
    return box.get("out"), box.get("err"), False


def cgroup_cpu_stat():
    """nr_throttled / throttled_usec of this container's CPU controller ({} where there is none): spinning on more
    threads than the quota allows gets the whole process stopped for the rest of a 100 ms period."""
    out = {}
    for path in ("/sys/fs/cgroup/cpu.stat", "/sys/fs/cgroup/cpu/cpu.stat"):
        try:
            for line in open(path):
                k, v = line.split()
                out[k] = int(v)
            break
        except (OSError, ValueError):
            pass
    return out


LAST_THROTTLE = {}


def timed_steps(world, ctx, step, warmup, steps):
    """W untimed steps, then exactly K steps between barrier + synchronize on both sides; MAX over ranks."""
    import gc
    for _ in range(warmup):
        step()
    if ctx is not None:
        ctx.profile_reset()
    world.barrier(ctx)
    each = []
    before = cgroup_cpu_stat()
    gc.collect()
    gc.disable()      # a collection of the interpreter inside a 12 ms step is not the prover's time
    try:
        t0 = time.perf_counter()
        for _ in range(steps):
            t = time.perf_counter()
            step()
            each.append(time.perf_counter() - t)
        world.barrier(ctx)
        elapsed = time.perf_counter() - t0
    finally:
        gc.enable()
    after = cgroup_cpu_stat()
    LAST_THROTTLE.clear()
    LAST_THROTTLE.update({"throttled_periods": after.get("nr_throttled", 0) - before.get("nr_throttled", 0),
                          "throttled_ms": (after.get("throttled_usec", after.get("throttled_time", 0)) -
                                           before.get("throttled_usec", before.get("throttled_time", 0))) / 1e3})
    return world.max_over_ranks(elapsed), each


DUMP_LIMIT = 60 * 10**6   # bytes of all the arrays of one --dump-outputs together (under 64 MB with the .npy headers)


def dump_outputs(directory, arrays):
    """--dump-outputs: {name: array} of the last timed step -> directory/<name>.npy, float64.  A field element is four 64-bit
    limbs, which float64 cannot hold: an array of 64-bit integers is written as its 32-bit words (low word first, so its last
    axis doubles), every word exact in float64.  Should the arrays exceed DUMP_LIMIT, every array keeps the same evenly spaced
    entries of its first axis (the sumcheck or proof index, the same length in all of them) and rows.npy lists which."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype.kind in "ui" and a.dtype.itemsize == 8:
            a = a.view(np.uint32)
        out[name] = a.astype(np.float64)
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_LIMIT:
        rows = {a.shape[0] for a in out.values()}
        assert len(rows) == 1, "the arrays to sample do not share their first axis"
        rows = rows.pop()
        keep = np.unique(np.linspace(0, rows - 1, max(1, rows * DUMP_LIMIT // total - 1)).round().astype(np.int64))
        out = {name: a[keep] for name, a in out.items()}
        out["rows"] = keep.astype(np.float64)
    os.makedirs(directory, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(directory, name + ".npy"), a)


# ------------------------------------------------------------------------------------------------ what was timed is checked

def _sha(*arrays):
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def verify_mle_outputs(ctx, tables, n, batch, out, rank, sample=32, evaluations=2):
    """Checks the (C, L, R) arrays the LAST TIMED step produced, without the oracle:
      * against the committed digests of the reference-semantics transcripts (tests/golden/*.json, produced offline by
        tests/golden/make_config_hashes.py): the whole batch in one digest per rank, every table of rank 0 one by one,
        and rank 0's table 0 against config_hashes.json;
      * the verifier's relations (python/sumcheck.py:55-70) on `sample` sumchecks spread over the whole batch (all
        scheduling groups, first and last table included): g_1(0) + g_1(1) = the table's sum (recomputed here from the
        downloaded table), g_j(0) + g_j(1) = g_{j-1}(r_{j-1}), r_j = MiMC7(g_j); and for `evaluations` of them the
        final check g_n(r_n) = T(r_1 .. r_n), the table folded on the host in Python integers.
    -> (dict for the JSON line, ok)"""
    import numpy as np
    from gkr_amd import multi_hash, synth
    from gkr_amd.field import MODULUS as P, from_limbs
    C, L, R = out
    count = 1 << n
    res = {"checked": "the outputs of the last timed step"}
    ok = True
    gold = synth.bench_batch_digests()
    if gold and gold.get("n") == n:
        if gold.get("batch") == batch and str(rank) in gold["whole_batch_by_rank"]:
            res["whole_batch_digest"] = _sha(C, L, R) == gold["whole_batch_by_rank"][str(rank)]
            res["sumchecks_in_digest"] = batch
            ok &= res["whole_batch_digest"]
        if rank == 0 and batch <= len(gold["rank0_tables"]):
            bad = [b for b in range(batch) if _sha(C[b], L[b], R[b])[:16] != gold["rank0_tables"][b]]
            res["tables_matching_their_digest"] = batch - len(bad)
            if bad:
                res["first_mismatching_tables"] = bad[:8]
                ok = False
    if rank == 0:
        want = synth.golden_digest("mle", "n=%d,seed=%d" % (n, synth.bench_table_seed(0, 0)))
        if want is not None:
            res["table0_golden_digest"] = _sha(C[0], L[0], R[0]) == want
            ok &= res["table0_golden_digest"]
    # verifier relations
    picks = sorted({int(round(i * (batch - 1) / max(1, sample - 1))) for i in range(min(sample, batch))})
    evals = set(picks[:1] + picks[-1:]) if evaluations >= 2 else set(picks[:evaluations])
    failures = []
    for b in picks:
        t = ctx.download(ctypes.c_void_p(tables.value + b * count * 32), (count, 4))
        cols = t.view(np.uint32).reshape(count, 8).sum(axis=0, dtype=np.uint64)
        claim = sum(int(cols[j]) << (32 * j) for j in range(8)) % P
        rs = from_limbs(R[b])
        for j in range(n):
            ln = int(L[b, j])
            g = from_limbs(C[b, j])[2 - ln:]        # highest degree first
            at0 = g[-1]
            at1 = sum(g) % P
            if (at0 + at1) % P != claim:
                failures.append((b, j, "sum"))
                break
            if multi_hash(g) != rs[j]:
                failures.append((b, j, "challenge"))
                break
            claim = 0
            for c in g:                                  # Horner at r_j
                claim = (claim * rs[j] + c) % P
        else:
            if b in evals:
                vals = np.array(from_limbs(t), dtype=object)
                for j in range(n):
                    h = len(vals) // 2
                    vals = (vals[:h] + rs[j] * (vals[h:] - vals[:h])) % P
                if int(vals[0]) != claim:
                    failures.append((b, n, "final evaluation"))
    res["verifier_relations"] = {"sumchecks": len(picks), "tables": picks, "with_final_evaluation": sorted(evals), "failures": failures,
                                 "ok": not failures}
    ok &= not failures
    res["ok"] = bool(ok)
    return res, bool(ok)


def native_verify_all(circuits, outs, threads=None):
    """gkr_verify (the library's C++ verifier: python/gkr.py:202-231 + python/sumcheck.py:55-70 on the gkr_proof_buf) on EVERY
    proof of a timed step: outs[j] = the nine output arrays of circuit j (first axis = proof).  Small proofs are spread over a
    thread pool (ctypes releases the GIL), each verified single-threaded; a lone wide proof gets all the threads itself.
    -> {"proofs", "accepted", "rejected": [(circuit, proof, layer, check)], "ms"}"""
    from concurrent.futures import ThreadPoolExecutor
    from gkr_amd.dropin import verify_native
    threads = threads or max(1, usable_cpus() - 1)
    jobs = [(j, b) for j, arrs in enumerate(outs) for b in range(arrs[0].shape[0])]
    t0 = time.perf_counter()
    if len(jobs) <= 2:
        res = [verify_native(circuits[j], outs[j], index=b, threads=threads) for j, b in jobs]
    else:
        with ThreadPoolExecutor(threads) as pool:
            res = list(pool.map(lambda jb: verify_native(circuits[jb[0]], outs[jb[0]], index=jb[1], threads=1), jobs))
    bad = [(j, b, r[1], r[2]) for (j, b), r in zip(jobs, res) if not r[0]]
    return {"verifier": "gkr_verify (csrc/dropin.cpp) on every proof of the last timed step", "proofs": len(jobs), "accepted": len(jobs) - len(bad),
            "rejected": bad[:8], "ms": round((time.perf_counter() - t0) * 1e3, 2), "ok": not bad}


# ------------------------------------------------------------------------------------------------ mode: mle

def run_mle(args, world):
    from gkr_amd import Context, synth
    n, batch = args.n, args.batch
    count = 1 << n
    ctx = Context(world.local_rank)
    ctx.set_transcript(1 if args.transcript == "host" else 0)
    # (experiment: GKR_BENCH_ALIGN_LOG2=30 puts the tables on a 1 GiB boundary of the virtual address space inside a larger
    # allocation -- does the fold pass's bandwidth follow the alignment?  profiles/r03: it does not)
    align_log2 = int(os.environ.get("GKR_BENCH_ALIGN_LOG2", "0") or 0)
    raw_tables = ctx.alloc(batch * count * 32 + ((1 << align_log2) if align_log2 else 0))
    tables = ctypes.c_void_p((raw_tables.value + (1 << align_log2) - 1) >> align_log2 << align_log2) if align_log2 else raw_tables
    for b in range(batch):
        ctx.fill_table(ctypes.c_void_p(tables.value + b * count * 32), count, synth.bench_table_seed(world.rank, b))
    ctx.synchronize()
    # the box's own copy / product rates (~0.1 s)
    ceilings = ctx.ceilings() if (args.full and world.rank == 0 and not args.no_extras) else None
    outputs = [None]   # the proof arrays of the previous step are reused (no fresh pages inside the timed call)

    def step():
        outputs[0] = ctx.sumcheck_mle_batch_device(tables, n, batch, out=outputs[0])

    ctx.profile(2 if args.full and not args.no_profile else 0)   # on during warm-up too: the event pool is created lazily
    elapsed, each = timed_steps(world, ctx, step, args.warmup, args.steps)
    ctx.profile(False)
    if args.dump_outputs and world.rank == 0:
        dump_outputs(args.dump_outputs, dict(zip(("coeffs", "lengths", "challenges"), outputs[0])))
    ops_per_sumcheck = 5 * (count - 1)
    value = ops_per_sumcheck * batch * args.steps * world.size / elapsed
    line = None
    if world.rank == 0:
        line = {
            "metric": "BN254-Fr sumcheck field-ops/sec @ 2^20 vars",
            "value": value, "unit": "field-ops/s", "n_gpus": world.size, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u32x8 (BN254 Fr, 254-bit modular integers; the fold pass's constant-by-table products as exact i8 MFMA with i32 sums)",
            "data": "synthetic",
            "config": {"workload": "plain MLE sumcheck (prove_sumcheck), 2^%d points per table, BASELINE configs[2]" % n,
                       "log2_points": n, "batch_per_gpu": batch, "sumchecks_per_step": batch * world.size,
                       "transcript": "MiMC7-91 on %s, included in the timed region" % args.transcript,
                       "parallelism": "independent sumchecks per rank, no collective"},
            "sumchecks_per_sec": batch * args.steps * world.size / elapsed,
            "tables_device_address": hex(tables.value),
            "step_ms_each": [round(x * 1e3, 3) for x in each]}
    if not args.full:
        ctx.free(raw_tables)
        ctx.close()
        if line:
            emit(line)
        return
    verified, verified_ok = ({"skipped": "--no-verify"}, True) if args.no_verify else verify_mle_outputs(ctx, tables, n, batch, outputs[0], world.rank)
    ranks_failed = world.max_over_ranks(0.0 if verified_ok else 1.0)
    threads_per_rank = [int(x) for x in world.per_rank(transcript_threads())]
    step_ms_per_rank = [round(x, 3) for x in world.per_rank(sum(each) / max(1, len(each)) * 1e3)]

    names = ["mle_multifold", "mle_multifold_late", "mle_sub_sums", "mle_sub_reduce", "mle_pass_small", "mle_fold_plan",   # multi-round passes (default)
             "mle_fold_sum", "mle_sum_first", "mle_round_reduce", "mle_fold_sum_small", "mle_round_hash"]  # per-round paths
    prof = {k: ctx.profile_get(k) for k in names}
    if world.rank == 0:
        dom_name = "mle_multifold" if prof["mle_multifold"]["launches"] else "mle_fold_sum"
        dom = prof[dom_name]
        achieved = dom["bytes"] / (dom["total_ms"] * 1e-3) / 1e9 if dom["total_ms"] > 0 else 0.0
        kernel_ms_total = sum(v["total_ms"] for v in prof.values())
        scheduled_bytes = sum(v["bytes"] for v in prof.values())
        sumchecks = batch * args.steps
        line.update({
            "host_threads": {"usable_cpus": usable_cpus(), "GKR_HOST_THREADS": os.environ.get("GKR_HOST_THREADS"),
                             "LOCAL_WORLD_SIZE": os.environ.get("LOCAL_WORLD_SIZE"), "cgroup_throttling_in_timed_steps": dict(LAST_THROTTLE),
                             "transcript_threads_per_rank": threads_per_rank, "mean_step_ms_per_rank": step_ms_per_rank},
            "roofline": {
                "bound": "hbm", "kernel": "k_mle_multifold_mfma<5> (the 2^n -> 2^(n-5) fold pass)" if dom_name == "mle_multifold" else "k_" + dom_name,
                "achieved": achieved, "peak": PEAK_GBPS, "unit": "GB/s", "frac": achieved / PEAK_GBPS,
                "traffic": None, "launches": dom["launches"],
                "copy_GBps_measured": ceilings["copy_GBps"] if ceilings else None,
                "read_GBps_measured": ceilings["read_GBps"] if ceilings else None,
                "frac_of_copy": achieved / ceilings["copy_GBps"] if ceilings else None,
                "alu_products_per_sec_measured": ceilings["modmul_per_sec"] if ceilings else None,
                "avg_launch_us": (dom["total_ms"] * 1e3 / dom["launches"]) if dom["launches"] else None,
                "algorithmic_bytes_per_launch": (dom["bytes"] / dom["launches"]) if dom["launches"] else None,
                "bytes_rule": "fold pass binding J variables: (2^J + 1) * 32 B per output entry (reads 2^J source entries, "
                              "writes one), J = 5 on the large tables; k_mle_fold_sum: 192 B per output pair.  The later, small "
                              "fold passes run on their own stream beside other groups' streaming passes and are booked "
                              "separately (kernel_ms.mle_multifold_late): their elapsed time is not their own cost",
            },
            "verified": dict(verified, all_ranks_ok=ranks_failed == 0.0),
            # the step's other resource: the host hashes batch x n round vectors per step
            "host_transcript": transcript_floor(int(outputs[0][1].sum()), 2, transcript_threads(), elapsed / args.steps * 1e3),
            "kernel_ms": {k: round(v["total_ms"], 3) for k, v in prof.items() if v["launches"]},
            # every byte the schedule moves (pass 0 reads the tables once, every fold pass reads its source and writes
            # its output: ~66 * 2^n per sumcheck with five rounds per pass) over WALL time: the whole step as bandwidth
            "end_to_end_GBps": scheduled_bytes / elapsed / 1e9 if not args.no_profile else None,
            "scheduled_bytes_per_sumcheck": scheduled_bytes / sumchecks if sumchecks and not args.no_profile else None,
            # SURVEY 8d's per-round accounting (128 * 2^n bytes per sumcheck) over ALL kernel time of the step: the
            # multi-round schedule moves about half of that, so this figure is NOT a bandwidth and can exceed HBM's
            "survey_accounting_GBps": (128.0 * count * sumchecks) / (kernel_ms_total * 1e-3) / 1e9 if kernel_ms_total else None,
        })
        # which of the fold pass's placement-dependent bandwidth modes this process drew: the big launches one by one
        avg_bytes = dom["bytes"] / max(1, dom["launches"])
        big = [(ms, by) for ms, by in ctx.profile_samples("mle_multifold") if by >= 0.99 * avg_bytes]   # the 2^n -> 2^(n-5) launches
        if big:
            rates = sorted(by / (ms * 1e-3) / 1e9 for ms, by in big if ms > 0)
            line["roofline"]["first_fold_pass_GBps"] = {"min": rates[0], "median": statistics.median(rates), "max": rates[-1],
                                                        "launches": len(rates)}
            # The launches of a step go out in group order; a step's FIRST fold launch is the only one that has the chip to
            # itself (the later ones share it with earlier groups' late passes on the second stream, whose bytes are not booked
            # to this kernel): what round 2 called a placement lottery (profiles/r03/e_lottery_*: per-group medians 6.45, 6.0,
            # 6.0, 6.2 ... TB/s in every process, 6.5 - 6.6 for ALL groups with GKR_NO_LATE_STREAM=1)
            per_step = len(big) // max(1, args.steps)
            if per_step >= 1 and len(big) == per_step * args.steps:
                first = [by / (ms * 1e-3) / 1e9 for ms, by in big[::per_step] if ms > 0]
                if first:
                    line["roofline"]["first_fold_pass_GBps"]["unshared_median"] = statistics.median(first)
                    line["roofline"]["first_fold_pass_GBps"]["unshared_frac_of_peak"] = statistics.median(first) / PEAK_GBPS
        first = prof["mle_sub_sums"] if prof["mle_sub_sums"]["launches"] else prof["mle_sum_first"]
        if first["total_ms"] > 0:
            line["roofline"]["first_pass_GBps"] = first["bytes"] / (first["total_ms"] * 1e-3) / 1e9
        import glob
        # PMC passes are separate runs (counters slow the kernels 2.5x), never part of this run: the newest committed one
        for traffic_file in sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "*pmc_traffic.json")), reverse=True):
            rel = os.path.relpath(traffic_file, os.path.join(REPO, "profiles"))
            if dom_name == "mle_multifold":
                try:
                    tj = json.load(open(traffic_file))
                    if tj.get("batch") == batch and tj.get("n") == n:
                        var = tj["k_mle_multifold_mfma"].get("variants", {}).get("gkr::k_mle_multifold_mfma<5>")
                        per_launch = (var or tj["k_mle_multifold_mfma"])["per_launch_mean_bytes"]
                        # the counters' launches must be launches of this size (the group size is the library's choice)
                        if 0.9 < per_launch / avg_bytes < 1.2:
                            line["roofline"]["traffic"] = per_launch
                            line["roofline"]["traffic_source"] = ("profiles/%s: separate rocprofv3 --pmc passes of this command on "
                                                                  "an earlier box, NOT measured in this run" % rel)
                            break
                except Exception:
                    pass
    # single-sumcheck latency and the 2^16 size (configs[1]) on the same resident tables
    extras = {}
    if not args.no_extras:
        lat = []
        ctx.sumcheck_mle_batch_device(tables, n, 1)
        for _ in range(20):
            t = time.perf_counter()
            ctx.sumcheck_mle_batch_device(tables, n, 1)
            lat.append(time.perf_counter() - t)
        extras["latency_ms_batch1"] = statistics.median(lat) * 1e3
        extras["field_ops_per_sec_batch1"] = ops_per_sumcheck / statistics.median(lat)
        n16, b16 = 16, min(4096, batch * (count >> 16)) if n >= 16 else 0
        if b16:
            out16 = [None]

            def step16():
                out16[0] = ctx.sumcheck_mle_batch_device(tables, n16, b16, out=out16[0])
            for _ in range(2):
                step16()
            ctx.synchronize()
            t = time.perf_counter()
            for _ in range(5):
                step16()
            ctx.synchronize()
            dt = (time.perf_counter() - t) / 5
            extras["n16"] = {"workload": "BASELINE configs[1]: 2^16 points per table, batch %d" % b16,
                             "value": 5 * ((1 << 16) - 1) * b16 / dt, "unit": "field-ops/s", "ms_per_step": dt * 1e3}
            extras["n16"]["roofline"] = transcript_floor(int(out16[0][1].sum()), 2, transcript_threads(), dt * 1e3)
            extras["n16"]["roofline"]["hbm_GBps_whole_step"] = (66.0 * (1 << 16) * b16) / dt / 1e9   # ~66 * 2^n bytes per sumcheck over wall time
            gold = synth.bench_batch_digests()
            if gold and world.rank == 0 and n == gold.get("n") and b16 == gold.get("n16_tables") and not args.no_verify:
                extras["n16"]["whole_batch_digest"] = _sha(*out16[0]) == gold["n16_whole_batch_rank0"]
                verified_ok &= extras["n16"]["whole_batch_digest"]
    ctx.free(raw_tables)
    ctx.close()
    # second half of the metric: every rank proves its own share of the inputs; MAX over ranks
    proofs = None
    if args.proofs > 0:
        proofs = aggregated_proofs(world, args.proofs)
    layer24 = layer24_split = mle_split_out = wide20 = wide20_circom = wide_prove = None
    split_hung = split_failed = False
    if not args.no_extras and args.layer_k_i > 0:
        layer24 = layer_leg(world, args.layer_k_i, args.layer_k, steps=10, warmup=3, split=False, ceilings=ceilings)
        # a WIDE layer, the shape of a compiled R1CS's big layers (2^20 gates over 2^20 values; round 3 rejected it)
        wide20 = layer_leg(world, 20, 20, steps=5, warmup=2, split=False, ceilings=ceilings) if args.layer_k_i >= 20 else None
        wide20_circom = layer_leg(world, 20, 20, steps=5, warmup=2, split=False, ceilings=ceilings, shape="circom") if args.layer_k_i >= 20 else None
        wide_prove = wide_prove_leg(world) if args.layer_k_i >= 20 else None
        if world.size > 1:
            # configs[4] as BASELINE words it: the layer's gates split over the ranks, two RCCL all-reduces per sumcheck
            # (device exchange).  Under a watchdog: a rank stuck in a collective must not cost the whole line.
            def split_leg():
                world.torch.cuda.set_device(world.local_rank)
                if os.environ.get("GKR_BENCH_FAIL_SPLIT") == "1":     # (test hook: what a failing split leg does to the exit code)
                    raise RuntimeError("GKR_BENCH_FAIL_SPLIT=1")
                return layer_leg(world, args.layer_k_i, args.layer_k, steps=10, warmup=3, split=True, ceilings=ceilings)
            layer24_split, err, split_hung = guarded(split_leg, 180)
            if err:
                layer24_split = {"error": err}
            # and the metric's own path split the same way: one 2^n table over the ranks (gkr_sumcheck_mle_sharded_dev)
            if not split_hung and (world.size & (world.size - 1)) == 0:
                def mle_split():
                    world.torch.cuda.set_device(world.local_rank)
                    return mle_split_leg(world, args.n, 1, steps=10, warmup=3, ceilings=ceilings)
                mle_split_out, err, split_hung = guarded(mle_split, 180)
                if err:
                    mle_split_out = {"error": err}
    if world.rank == 0:
        line.update(extras)
        if layer24:
            line["layer24"] = layer24
            verified_ok &= layer24["matches_golden_digest"] is not False
        if wide20:
            line["wide20"] = wide20
            verified_ok &= wide20["matches_golden_digest"] is not False
        if wide20_circom:
            line["wide20_circom_shaped"] = wide20_circom
            verified_ok &= wide20_circom["matches_golden_digest"] is not False
        if wide_prove:
            line["wide_prove"] = wide_prove
            verified_ok &= wide_prove["matches_golden_digest"] is not False
        if layer24_split:
            line["layer24_split"] = layer24_split
            # (a WRONG transcript fails the run; a leg that could not run -- an exception or a rank stuck in its first real
            # multi-device collective -- is reported on the line and does not cost the headline its exit code)
            verified_ok &= layer24_split.get("matches_golden_digest") is not False
        if mle_split_out:
            line["mle_split"] = mle_split_out
            verified_ok &= mle_split_out.get("matches_golden_digest") is not False
        if world.size > 1:
            line["collective"] = collective_info(world)
            line["collective"]["note"] = ("the headline workload shards whole sumchecks over the ranks and needs no data-path collective; "
                                          "layer24_split and mle_split carry the exchanges of the two paths that have one")
        if proofs:
            line["aggregated_proofs"] = proofs
            verified_ok &= proofs.get("verified_ok", True)
        if world.size == 1 and not args.no_cpu_baseline:
            line["cpu_baseline"] = cpu_dense(n, args.cpu_seconds)
            line["cpu_ref_algo"] = cpu_ref_algo(args.ref_algo_seconds)
            line["cpu_pipeline"] = cpu_pipeline()
        # exit code: 1 = an output of a timed step failed its check; 4 = a split leg's collective did not return; 2 = a split leg
        # (the only legs with a real N > 1 data path) raised -- the line is still emitted and says which
        split_errors = {name: leg["error"] for name, leg in (("layer24_split", layer24_split), ("mle_split", mle_split_out))
                        if isinstance(leg, dict) and "error" in leg}
        wrong = not verified_ok or ranks_failed
        code = 1 if wrong else (4 if split_hung else (2 if split_errors else 0))
        why = ("WRONG RESULTS: an output of a timed step failed its check" if wrong else
               "a split leg's collective did not return (the headline above was timed and verified first)" if split_hung else
               "a split leg failed: " + "; ".join("%s: %s" % kv for kv in split_errors.items()) if split_errors else "ok")
        line["exit"] = {"code": code, "why": why[:400]}
        split_failed = bool(split_errors)
        emit(line)
    if split_hung:
        os._exit(4)    # a thread of this process sits in a collective that will not return: no orderly shutdown possible
    if not verified_ok or ranks_failed:
        raise SystemExit("WRONG RESULTS: the outputs of the timed steps failed their check (see \"verified\" / \"layer24\" / \"n16\")")
    if world.rank == 0 and split_failed:
        sys.stderr.write("bench.py: a split leg failed (see the line's `exit`)\n")
        raise SystemExit(2)


def aggregated_proofs(world, n_inputs):
    """"aggregated proofs/sec" on the circuit the reference's own test uses (aggregator.rs:441-457: t.circom with
    example/input{1,2,3}.json): its R1CS (hand-written equivalent, gkr_amd.synth) compiled to the 12 layered
    circuits, every (circuit, input) pair proven (gkr_prove_batch = prover::prove, prover.rs:6-96) -- for the three
    example inputs (configs[0]) and for `n_inputs` inputs split over the ranks (configs[3]).  One "proof" = one
    prover::prove call = one sub-circuit of one input.  Checked against the oracle in tests/test_gpu_circom_pipeline.py."""
    import numpy as np
    from gkr_amd import Context, parallel, synth
    from gkr_amd.aggregate import ProvingStep
    from gkr_amd.field import as_limbs
    t0 = time.perf_counter()
    r1cs = synth.mimc7_demo_r1cs()
    step = ProvingStep(r1cs)
    compile_ms = (time.perf_counter() - t0) * 1e3
    subs = len(step.circuits)
    cpus = max(1, usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))))
    threads = transcript_threads()   # (the library's own default: gkr_capi.hip, default_host_threads)
    ctx = Context(world.local_rank)
    out = {"circuit": "R1CS equivalent to rust/t.circom (MiMC7-91, 364 constraints) -> %d layered circuits, k lists %s"
                      % (subs, [c.get_k_list() for c in step.circuits]),
           "compile_ms": compile_ms, "proof": "one prover::prove call (one sub-circuit of one input)",
           "how": "gkr_prove_many: one call per proving step, one gkr_prove_batch per sub-circuit (the proofs of all inputs "
                  "advance together, one round trip per round), the %d sub-circuits in flight together on %d of the library's "
                  "own threads with child contexts (the reference's par_iter over the (circuit, input) pairs); threads that "
                  "wait, are done or have no item take pieces of the others' host work" % (subs, threads),
           "contexts": threads, "cpus_per_rank": cpus}

    def measure(witnesses, reps, ctx=ctx):
        inputs = step.inputs_for(np.stack([as_limbs(w) for w in witnesses])) if witnesses else None
        if inputs is not None:
            for _ in range(4):
                step.prove_raw_many(ctx, inputs, threads)     # warm-up: code objects, workspaces, circuit caches, the crew's threads
        world.barrier(ctx)
        each = []
        t = time.perf_counter()
        for _ in range(reps):
            t1 = time.perf_counter()
            if inputs is not None:
                step.prove_raw_many(ctx, inputs, threads)
            each.append(round((time.perf_counter() - t1) * 1e3, 3))
        world.barrier(ctx)
        return world.max_over_ranks((time.perf_counter() - t) / reps), each
    ex = [synth.mimc7_demo_witness(a, b) for a, b in synth.EXAMPLE_INPUTS]
    dt3, each3 = measure(ex if world.rank == 0 else [], 5)     # configs[0] is one rank's work
    def check(golden_rows, tag, sample=2):
        """The proofs of the LAST measured step (the prepared list's output buffers) against the committed digests of
        the CPU checker's proofs (tests/golden/proof_digests.json, made offline), every (input, sub-circuit) pair; and
        gkr_amd.verify on `sample` inputs' proofs.  -> dict for the line."""
        from gkr_amd import verify
        from gkr_amd.prover import _decode_proofs
        res = {"checked": "every proof of the last timed step: (sumcheck_proofs, sumcheck_r, q, z, r) digests; verifier on a sample"}
        bad, total, verified = [], 0, 0
        for j, (arrs, circuit) in enumerate(zip(step._prepared["outs"], step.circuits)):
            proofs = _decode_proofs(arrs, circuit.get_k_list())
            for i, pr in enumerate(proofs):
                total += 1
                dg = synth.proof_digest(pr.sumcheck_proofs, pr.sumcheck_r, pr.q, pr.z, pr.r)[:16]
                if golden_rows is not None and dg != golden_rows[i][j]:
                    bad.append((i, j))
                if i < sample or i == len(proofs) - 1:
                    verified += 1
                    if not verify(pr, circuit):
                        bad.append((i, j, "verifier"))
        native = native_verify_all(step.circuits, step._prepared["outs"])
        res.update({"proofs": total, "digests": "tests/golden/proof_digests.json[%s]" % tag if golden_rows is not None else None,
                    "mismatches": bad[:8], "python_verifier_accepts": verified, "gkr_verify": native, "ok": not bad and native["ok"]})
        return res
    golden = synth.proof_digests() if not os.environ.get("GKR_BENCH_NO_VERIFY") else None
    ver0 = check(golden["config0"]["digests"] if golden else None, "config0", sample=3) if world.rank == 0 and not os.environ.get("GKR_BENCH_NO_VERIFY") else None
    mine = parallel.shard_units(n_inputs, world.rank, world.size)
    dt, each = measure([synth.mimc7_demo_witness(a, b) for a, b in [synth.demo_proof_inputs(n_inputs)[i] for i in mine]], 5)
    # one more, untimed step with the library's thread accounts on: where the proving threads' time goes (own hashing pieces,
    # pieces of other contexts' work taken while waiting for the GPU, spinning with nothing to take, launches and set-up,
    # and what the threads without an item lent) -- rank 0's figures
    accounts = None
    if len(mine) and world.rank == 0:
        from gkr_amd import _native as N
        import ctypes
        lib = N.lib()
        acc_inputs = step.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(a, b)) for a, b in [synth.demo_proof_inputs(n_inputs)[i] for i in mine]]))
        step.prove_raw_many(ctx, acc_inputs, threads)   # (prepares the item list for these arrays: not part of the accounted step)
        lib.gkr_host_accounting(1)
        t1 = time.perf_counter()
        step.prove_raw_many(ctx, acc_inputs, threads)
        acc_ms = (time.perf_counter() - t1) * 1e3
        lib.gkr_host_accounting(0)
        buf = (ctypes.c_double * 28)()
        lib.gkr_host_accounting_read(buf, 28)
        own, helped, spin, rest, lent, lent_idle, calls, wake = [float(x) for x in buf[:8]]
        n_pieces, piece_us, pass_us = float(buf[8]), float(buf[9]), float(buf[10])
        lanes_hist = [int(buf[10 + n]) for n in range(1, 17)]
        thread_ms = threads * acc_ms
        accounts = {"step_ms": round(acc_ms, 3), "threads": threads, "proving_calls": int(calls),
                    "thread_ms": {"own_hashing_pieces": round(own / 1e3, 2), "others_pieces_while_waiting_for_the_gpu": round(helped / 1e3, 2),
                                  "spinning_on_the_gpu_nothing_to_take": round(spin / 1e3, 2), "launches_setup_copies": round(rest / 1e3, 2),
                                  "pieces_by_threads_without_an_item": round(lent / 1e3, 2), "those_threads_idle": round(lent_idle / 1e3, 2),
                                  "from_the_call_to_the_threads_first_item": round(wake / 1e3, 2)},
                    # the hashing pieces themselves: how full the sixteen IFMA lanes were, and what the threads' "piece" time is made of
                    "pieces": {"count": int(n_pieces), "transcripts_per_piece_histogram_1_to_16": lanes_hist,
                               "mean_transcripts_per_piece": round(sum((n + 1) * c for n, c in enumerate(lanes_hist)) / max(1.0, n_pieces), 2),
                               "ms_inside_the_pass_function_hashes_and_field_arithmetic": round(pass_us / 1e3, 2),
                               "ms_copying_round_vectors_out": round((piece_us - pass_us) / 1e3, 2),
                               "ms_posting_looking_for_and_waiting_for_pieces": round((own + helped + lent - piece_us) / 1e3, 2)},
                    "busy_fraction_of_threads_x_step": round((own + helped + rest + lent) / 1e3 / thread_ms, 3) if thread_ms else None,
                    "idle_fraction": round((spin + lent_idle) / 1e3 / thread_ms, 3) if thread_ms else None}
    ver3 = None
    if len(mine) and not os.environ.get("GKR_BENCH_NO_VERIFY"):
        rows = [golden["config3"]["digests"][i] for i in mine] if golden and golden["config3"]["inputs"] == n_inputs else None
        ver3 = check(rows, "config3")
    bad_ranks = world.max_over_ranks(1.0 if (ver3 and not ver3["ok"]) or (ver0 and not ver0["ok"]) else 0.0)
    out["config0_three_inputs"] = {"inputs": 3, "proofs": 3 * subs, "ms": dt3 * 1e3, "proofs_per_sec": 3 * subs / dt3, "ms_each": each3}
    out["config3"] = {"inputs": n_inputs, "inputs_per_rank": [len(parallel.shard_units(n_inputs, r, world.size)) for r in range(world.size)],
                      "proofs": n_inputs * subs, "ms": dt * 1e3, "proofs_per_sec": n_inputs * subs / dt, "inputs_per_sec": n_inputs / dt,
                      "ms_each_rank0": each}
    out["config3"]["host_thread_accounts"] = accounts
    # configs[3] the way the reference runs it: ONE host process whose par_iter fans prover::prove out
    # (aggregator.rs:350-355, 411-416) -- here over every device this process can see (gkr_ctx_create_multi: the items of a
    # gkr_prove_many call dealt over child contexts on all of them).  Only on the N = 1 line: with one rank per GPU the
    # ranks already hold a device each.
    if world.size == 1 and os.environ.get("GKR_BENCH_MULTI_DEVICE", "1") != "0":
        out["multi_device"] = multi_device_in_a_child(n_inputs)
    out["config0_three_inputs"]["verified"] = ver0
    out["config3"]["verified"] = dict(ver3 or {}, all_ranks_ok=bad_ranks == 0.0)
    out["verified_ok"] = bad_ranks == 0.0 and (ver0 is None or ver0["ok"]) and (ver3 is None or ver3["ok"])
    out["proofs_per_sec"] = out["config3"]["proofs_per_sec"]
    # The same pipeline on an R1CS of the size the reference is FOR (aggregating real circuits): 262 144 constraints -> 16
    # layered circuits with layers of 2^14 .. 2^16 values (round 3's boundary rejected them), one input, every rank alike;
    # every proof's arrays against the CPU checker's END-TO-END digests (its own restatement of convert.rs compiled the R1CS).
    if os.environ.get("GKR_BENCH_LARGE_R1CS", "1") != "0":
        gold = synth.large_r1cs_digests()
        nrounds = gold["nrounds"] if gold else 65536
        pair = tuple(gold["input"]) if gold else (2, 3)
        t0 = time.perf_counter()
        big_r1cs = synth.mimc7_demo_r1cs(nrounds=nrounds)       # (the fixture: Python writing 262 144 constraints + gkr_r1cs_build)
        big_synth_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        big = ProvingStep(big_r1cs)                             # gkr_r1cs_compile + the circuits' descriptions
        big_compile_ms = (time.perf_counter() - t0) * 1e3
        big_inputs = big.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(pair[0], pair[1], nrounds=nrounds))]))
        for _ in range(3):
            big.prove_raw_many(ctx, big_inputs, threads)
        world.barrier(ctx)
        each_big = []
        for _ in range(9):
            t1 = time.perf_counter()
            big.prove_raw_many(ctx, big_inputs, threads)
            each_big.append((time.perf_counter() - t1) * 1e3)
        world.barrier(ctx)
        dt_big = world.max_over_ranks(statistics.median(each_big) / 1e3)
        ks_big = [c.get_k_list() for c in big.circuits]
        bad_big = None
        if gold and not os.environ.get("GKR_BENCH_NO_VERIFY"):
            coeff_gold = gold.get("coeff_digests")
            bad_big = [j for j, (arrs, ks) in enumerate(zip(big._prepared["outs"], ks_big))
                       if j >= len(gold["digests"]) or ks != gold["k"][j] or synth.proof_arrays_digest(ks, *[a[0] for a in arrs[:7]]) != gold["digests"][j]
                       or (coeff_gold and synth.proof_coeffs_digest(arrs[7][0], arrs[8][0]) != coeff_gold[j])]
        big_native = native_verify_all(big.circuits, big._prepared["outs"]) if not os.environ.get("GKR_BENCH_NO_VERIFY") else None
        if big_native is not None and not big_native["ok"]:
            bad_big = (bad_big or []) + ["gkr_verify"]
        big_bad_ranks = world.max_over_ranks(1.0 if bad_big else 0.0)
        out["large_r1cs"] = {"constraints": 4 * nrounds, "sub_circuits": len(big.circuits), "k_lists": ks_big, "inputs": 1,
                             "compile_ms": big_compile_ms, "compile": "gkr_r1cs_compile (trees and groups on the host's threads) + reading the circuits out; the "
                             "fixture's own construction in Python (r1cs_synthesis_ms) is not the product's", "r1cs_synthesis_ms": big_synth_ms, "ms": dt_big * 1e3, "ms_each": [round(x, 3) for x in each_big],
                             "proofs_per_sec": len(big.circuits) / dt_big, "constraints_per_sec": 4 * nrounds / dt_big,
                             "verified": None if bad_big is None else {"digests": "tests/golden/large_r1cs_digests.json (compile and proofs by the CPU checker; d and input_func %s)" % ("included" if gold.get("coeff_digests") else "not covered"),
                                                                        "proofs": len(big.circuits), "mismatches": bad_big, "ok": not bad_big, "all_ranks_ok": big_bad_ranks == 0.0,
                                                                        "gkr_verify": big_native}}
        if bad_big or big_bad_ranks:
            out["verified_ok"] = False
        big.close()
    hashed = sum(int(arrs[1].sum()) for arrs in step._prepared["outs"])   # lengths of all round vectors of the last step
    out["config3"]["roofline"] = transcript_floor(hashed, 3, threads, dt * 1e3)
    ctx.close()
    step.close()
    return out


def multi_device_leg(n_inputs):
    """configs[3] through ONE process and gkr_ctx_create_multi over every visible device (the mode `multi-device` of this file:
    runs in a child of the default line).  -> the leg's dict."""
    import numpy as np
    import torch
    from gkr_amd import Context, synth
    from gkr_amd.aggregate import ProvingStep
    from gkr_amd.field import as_limbs
    from gkr_amd.prover import _decode_proofs
    devs = [int(os.environ["GKR_BENCH_DEVICE"])] if "GKR_BENCH_DEVICE" in os.environ else list(range(torch.cuda.device_count()))
    step = ProvingStep(synth.mimc7_demo_r1cs())
    subs = len(step.circuits)
    inputs = step.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(a, b)) for a, b in synth.demo_proof_inputs(n_inputs)]))
    # The same step through a plain context on devs[0] and through the multi-device context, ALTERNATING in this one process (a
    # fresh process proves ~5 % slower than the long-running one of the default line whatever the path -- same-box A/B
    # profiles/r06/a_multi_device_ab.txt -- so the comparison that says what gkr_ctx_create_multi costs is made here).
    direct_step = ProvingStep(synth.mimc7_demo_r1cs())
    direct_inputs = direct_step.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(a, b)) for a, b in synth.demo_proof_inputs(n_inputs)]))
    with Context(devs[0]) as one, Context(devices=devs) as mctx:
        for _ in range(20):
            direct_step.prove_raw_many(one, direct_inputs, 0)
            step.prove_raw_many(mctx, inputs, 0)
        each, each_direct = [], []
        for _ in range(10):
            t = time.perf_counter()
            direct_step.prove_raw_many(one, direct_inputs, 0)
            each_direct.append(round((time.perf_counter() - t) * 1e3, 3))
            t = time.perf_counter()
            step.prove_raw_many(mctx, inputs, 0)
            each.append(round((time.perf_counter() - t) * 1e3, 3))
        seen = mctx.device_count()
    direct_step.close()
    golden = synth.proof_digests()
    rows = golden["config3"]["digests"] if golden and golden["config3"]["inputs"] == n_inputs else None
    bad = total = 0
    for j, (arrs, circuit) in enumerate(zip(step._prepared["outs"], step.circuits)):
        for i, pr in enumerate(_decode_proofs(arrs, circuit.get_k_list())):
            total += 1
            if rows is not None and synth.proof_digest(pr.sumcheck_proofs, pr.sumcheck_r, pr.q, pr.z, pr.r)[:16] != rows[i][j]:
                bad += 1
    step.close()
    dt = statistics.median(each) / 1e3
    return {"how": "one process, gkr_ctx_create_multi(%s): one gkr_prove_many call per step deals the %d sub-circuits over child contexts "
                   "on every listed device (the reference: one process whose par_iter fans prover::prove out, aggregator.rs:350-355)" % (devs, subs),
            "devices_seen": seen, "device_ids": devs, "inputs": n_inputs, "proofs": n_inputs * subs, "ms": dt * 1e3,
            "proofs_per_sec": n_inputs * subs / dt, "ms_each": each,
            "direct_ms_same_process": statistics.median(each_direct), "direct_ms_each": each_direct,
            "ms_over_direct": dt * 1e3 / statistics.median(each_direct),
            "verified": {"proofs": total, "digests": "tests/golden/proof_digests.json[config3]" if rows is not None else None, "mismatches": bad, "ok": bad == 0}}


def multi_device_in_a_child(n_inputs):
    """The leg above in a CHILD process with a deadline: a path that has never met a second device (every builder's box had one)
    must not be able to fail or hang the line it rides on.  Its result -- or what went wrong -- is reported; the line's own
    verification does not depend on it."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", "multi-device", "--proofs", str(n_inputs)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    try:
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
        lines = [l for l in done.stdout.splitlines() if l.startswith("{")]
        if done.returncode == 0 and lines:
            return dict(json.loads(lines[-1]), isolated="ran in a child process of the bench: it cannot fail or hang the line")
        return {"error": "child exited %d: %s" % (done.returncode, (done.stderr or "")[-400:]), "isolated": True, "device_ids": None}
    except subprocess.TimeoutExpired:
        return {"error": "no result after 240 s (the child was ended)", "isolated": True, "device_ids": None}
    except Exception as e:   # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e), "isolated": True, "device_ids": None}


# ------------------------------------------------------------------------------------------------ mode: proofs

def run_proofs(args, world):
    import numpy as np
    from gkr_amd import Context, parallel, synth
    from gkr_amd.aggregate import ProvingStep
    from gkr_amd.field import as_limbs
    step_obj = ProvingStep(synth.mimc7_demo_r1cs())
    subs = len(step_obj.circuits)
    mine = parallel.shard_units(args.proofs, world.rank, world.size)
    cpus = max(1, usable_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", "1"))))
    threads = transcript_threads()   # (the library's own default: gkr_capi.hip, default_host_threads)
    ctx = Context(world.local_rank)
    inputs = step_obj.inputs_for(np.stack([as_limbs(synth.mimc7_demo_witness(2 + i, 3 + (i % 5))) for i in mine])) if len(mine) else None

    def step():
        if inputs is not None:
            step_obj.prove_raw_many(ctx, inputs, threads)
    elapsed, each = timed_steps(world, ctx, step, args.warmup, args.steps)
    if args.dump_outputs and world.rank == 0 and inputs is not None:
        from gkr_amd._native import ProofBuf
        fields = [f for f, _ in ProofBuf._fields_]
        dump_outputs(args.dump_outputs, {"c%d_%s" % (j, f): a for j, arrs in enumerate(step_obj._prepared["outs"]) for f, a in zip(fields, arrs)})
    # what was timed is checked on every rank: every proof of the last step through the library's verifier (gkr_verify)
    native = native_verify_all(step_obj.circuits, step_obj._prepared["outs"]) if inputs is not None and not args.no_verify else None
    bad_ranks = world.max_over_ranks(1.0 if native is not None and not native["ok"] else 0.0)
    hashed = sum(int(arrs[1].sum()) for arrs in step_obj._prepared["outs"]) if inputs is not None else 0
    if world.rank == 0:
        emit({
            "verified": {"ok": bad_ranks == 0.0, "all_ranks_ok": bad_ranks == 0.0, "gkr_verify_rank0": native},
            "roofline": transcript_floor(hashed, 3, threads, elapsed / args.steps * 1e3),
            "metric": "aggregated proofs/sec", "value": args.proofs * subs * args.steps / elapsed, "unit": "proofs/s",
            "n_gpus": world.size, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "u32x8 (BN254 Fr)", "data": "synthetic",
            "config": {"workload": "BASELINE configs[3]: %d inputs of the t.circom-equivalent R1CS, %d layered circuits each, "
                                   "inputs split over the ranks, no collective" % (args.proofs, subs),
                       "inputs_per_rank": [len(parallel.shard_units(args.proofs, r, world.size)) for r in range(world.size)],
                       "proof": "one prover::prove call (one sub-circuit of one input)",
                       "how": "gkr_prove_many, %d threads / child contexts per rank" % threads, "cpus_per_rank": cpus},
            "inputs_per_sec": args.proofs * args.steps / elapsed, "step_ms_each": [round(x * 1e3, 3) for x in each]})
    ctx.close()
    step_obj.close()
    if bad_ranks:
        raise SystemExit("WRONG RESULTS: gkr_verify rejected a proof of the last timed step")


# ------------------------------------------------------------------------------------------------ mode: layer-split

def layer_leg(world, k_i, k, steps, warmup, split, ceilings=None, shape="uniform", dump=None):
    """BASELINE configs[4]: ONE GKR layer sumcheck (prove_sumcheck_opt, sumcheck.rs:36-156) with 2^k_i random gates
    over a 2^k-entry next layer, gates and their sorted lists resident in HBM before the timed region, a step = one
    sumcheck (new z, W).  split: the gates are divided over the ranks (two sum-over-ranks exchanges per sumcheck);
    otherwise every rank proves the whole layer on its own (N = 1 work, MAX over ranks).  -> the dict of the JSON
    line (on rank 0; None elsewhere).  The transcript is compared with the committed digest of the reference-semantics
    transcript (tests/golden/config_hashes.json)."""
    import numpy as np
    from gkr_amd import Context, parallel, synth
    # shape "circom": the structure the reference's compiler emits (synth.circom_shaped_layer: runs of gates over runs of
    # values, two wires feeding most of the layer) instead of a uniform draw, which has no locality at all
    lay, z, W = synth.circom_shaped_layer(k_i, k) if shape == "circom" else synth.config5_layer(k_i, k)
    gt, l, r = lay.arrays()
    first, cnt = parallel.gate_range(k_i, world.rank, world.size) if split else (0, 1 << k_i)
    ctx = Context(world.local_rank)
    gates = parallel.ResidentGates(ctx, k_i, first, gt[first:first + cnt], l[first:first + cnt], r[first:first + cnt])
    coll = parallel.TorchCollective() if (split and world.grouped) else None
    exchange = coll.exchange() if coll else None   # one rank: the whole layer, no exchange
    result = [None]
    # W resident in HBM before the timed region, like the gates (inside prover::prove the next layer's values come from the
    # forward evaluation and never were host data); the split legs hand W over from the host as their entry points do
    d_W = None
    if not split:
        d_W = ctx.alloc(W.nbytes)
        ctx.upload(d_W, np.ascontiguousarray(W))

    def step():
        result[0] = gates.sumcheck_raw(k, z, W, exchange) if split else gates.sumcheck_raw_device_w(k, z, d_W)
    # the first sumcheck of a layer pays for the sort of its gates and the segment build as well (z- and W-independent, like
    # the reference's precomputed add_wire / mult_wire; once per circuit): timed on its own, outside the steps
    ctx.profile(1)
    ctx.profile_reset()
    ctx.synchronize()
    t_first = time.perf_counter()
    step()
    one_shot_ms = (time.perf_counter() - t_first) * 1e3
    sort_ms = ctx.profile_get("gate_lists")["total_ms"]
    # the steps on the line run WITHOUT the per-kernel events (a pair of event records around every timed launch leaves ~6 us of
    # idle device between two kernels of a chain: ~40 us of a 1.4 ms sumcheck); the kernels' own times come from a second pass
    # of the same steps with the events on
    ctx.profile(False)
    elapsed, each = timed_steps(world, ctx, step, warmup, steps)
    if dump and world.rank == 0:
        dump_outputs(dump, dict(zip(("coeffs", "lengths", "challenges"), result[0])))
    ctx.profile(1)
    ctx.profile_reset()
    for _ in range(steps):
        step()
    ctx.synchronize()
    ctx.profile(False)
    host_w_ms = None
    if not split and k >= 16:   # the PCIe-inclusive figure (W handed over in host memory every sumcheck): reported, never the value
        gates.sumcheck_raw(k, z, W, None)
        t_h = time.perf_counter()
        for _ in range(3):
            gates.sumcheck_raw(k, z, W, None)
        host_w_ms = (time.perf_counter() - t_h) / 3 * 1e3
    names = ["gate_lists", "eq_table_z", "gate_uv", "gate_rows", "gate_combine", "predicate_sorted", "layer_prod_pass"]
    prof = {n_: ctx.profile_get(n_) for n_ in names}
    exch = ctx.profile_get("exchange")
    own = ceilings or (ctx.ceilings(256 << 20) if world.rank == 0 else None)
    out = None
    if world.rank == 0:
        C, L, R = result[0]
        digest = synth.transcript_digest(C, L, R)
        want = synth.golden_digest("layer", ("circom-shaped," if shape == "circom" else "") + "k_i=%d,k=%d" % (k_i, k))
        N = 1 << (2 * k)
        # the passes over the gates -- for wide layers with the eq(z, .) table they gather from (built once per sumcheck: it
        # replaced a product per gate, so its time is the passes' time)
        passes = [n_ for n_ in ("eq_table_z", "gate_uv", "gate_rows", "gate_combine") if prof[n_]["launches"]]
        gate_ms = sum(prof[n_]["total_ms"] for n_ in passes) / steps
        # what a gate pass must do, whatever the schedule: one 254-bit product per gate (eq(z, g) times W[right] resp.
        # eq(u, left)); everything else a form spends (forming eq(z, g) from its two halves per gate, reductions) is
        # overhead against this count -- so the fraction compares forms fairly
        products = 2.0 * cnt
        rate = products / (gate_ms * 1e-3) if gate_ms else None
        peak = own["modmul_per_sec"] if own else None
        dense_accounting = 2 * k <= k_i + 2
        wide = k >= 13   # lane-group passes: the operand table (2^k x 32 B) no longer sits in LDS / L2 -- a gather per gate
        out = {
            # a layer with a gate for (nearly) every point of the 2^{2k} hypercube is priced by SURVEY 8d's dense accounting,
            # 25 (2^{2k} - 1) field-ops per sumcheck; a sparse (circom-shaped, wide) layer is proven in time linear in its GATES,
            # and 25 * 2^{2k} would be a number about nothing: gates/s there
            "metric": ("BN254-Fr GKR-layer sumcheck field-ops/sec @ 2^%d gates" if dense_accounting else "BN254-Fr GKR-layer sumcheck gates/sec @ 2^%d gates") % k_i,
            "value": (25 * (N - 1) if dense_accounting else (1 << k_i)) * steps / elapsed,
            "unit": "field-ops/s" if dense_accounting else "gates/s", "gates_per_sec": (1 << k_i) * steps / elapsed, "n_gpus": world.size if split else 1, "steps": steps, "warmup": warmup,
            "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "strong" if split else "weak", "vs_baseline": None,
            "dtype": "u32x8 (BN254 Fr)", "data": "synthetic",
            "config": {"workload": "%s: one GKR layer, k_i = %d, k = %d%s" % (
                           "BASELINE configs[4]" if (k_i, k) == (24, 12) else ("a WIDE layer, gates in the order and with the operand structure the reference's compiler emits (convert.rs:209-214, 278-343)"
                                                                                if shape == "circom" else "a WIDE layer, gates drawn uniformly (no locality: the worst case for the gathers)"),
                           k_i, k, ", gates split over the ranks, two sum-over-ranks exchanges of 2 * 2^k field elements per sumcheck" if split else
                           ", the whole layer on one GPU"),
                       "gates_per_rank": cnt, "gates": "gates and their sorted lists resident in HBM before the timed region (gkr_resident_layer_*: one circuit, a new z per sumcheck)",
                       "W": "handed over in host memory every sumcheck (the exchange entry points' form)" if split else "resident in HBM (gkr_resident_layer_sumcheck_wdev)"},
            "ms_per_step_with_W_from_host_memory": host_w_ms,
            "matches_golden_digest": None if want is None else digest == want, "transcript_sha256": digest,
            "one_shot_ms": one_shot_ms, "sort_ms": sort_ms,
            "one_shot_note": "the layer's FIRST sumcheck on this context: gate arrays already in HBM, but the counting sort of the gates, the segment "
                             "build (sort_ms: all their kernels, HIP events) and first-use allocations included; every later sumcheck is ms_per_step",
            "roofline": {"bound": "alu", "kernel": " + ".join("k_" + p_ for p_ in passes) + " (the two passes over this rank's gates: U, V before the b rounds; the row a_u, m_u before the c rounds)",
                         "achieved": rate, "peak": peak, "unit": "254-bit modular products/s",
                         "frac": rate / peak if rate and peak else None, "traffic": None,
                         "peak_fixed": PEAK_PRODUCTS_PER_SEC, "frac_of_fixed_peak": rate / PEAK_PRODUCTS_PER_SEC if rate else None,
                         "products_per_launch_pair": products, "gate_pass_ms_per_step": gate_ms,
                         "products_rule": "one product per gate and pass (2 per gate and sumcheck); peak = the chip-wide rate of dependent "
                                          "Montgomery products measured in this process (gkr_ubench_ceilings, 16 waves per SIMD)",
                         "hbm_bytes_per_gate_and_pass": 8, "note": ("not memory-bound: per gate one 8-byte list entry is streamed from HBM, the eq and W "
                                          "operands are gathers from L2-resident tables") if not wide else
                                         ("a WIDE layer's item passes are NOT bound by the products (frac above is what is left of the ALU): they are "
                                          "bound by the 128-byte lines their random 32-byte accesses move -- see `memory`")},
            # wide layers (k_next >= 13, kernels_wide.hip): per gate and pass one 8-byte packed entry streamed, eq(z, g) and the operand
            # gathered (32 B each, random), and per bucket two 32-byte outputs stored -- every one of the random accesses moves a
            # 128-byte line (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE per launch: profiles/r05/b_wide_gate_pass_pmc_*.txt)
            "memory": ({"bound": "hbm", "algorithmic_bytes_per_step": 2.0 * (cnt * (8 + 32 + 32) + (2 << k) * 32),
                        "achieved": 2.0 * (cnt * (8 + 32 + 32) + (2 << k) * 32) / (gate_ms * 1e-3) / 1e9 if gate_ms else None, "peak": PEAK_GBPS, "unit": "GB/s",
                        "frac": 2.0 * (cnt * (8 + 32 + 32) + (2 << k) * 32) / (gate_ms * 1e-3) / 1e9 / PEAK_GBPS if gate_ms else None,
                        "line_bytes_per_step_if_every_random_access_moves_128_B": 2.0 * (cnt * (8 + 128 + 128) + (2 << k) * 128),
                        "frac_in_lines": 2.0 * (cnt * (8 + 128 + 128) + (2 << k) * 128) / (gate_ms * 1e-3) / 1e9 / PEAK_GBPS if gate_ms else None,
                        "note": "uniform gates: every access is its own line (measured: 0.29 GB fetched + 0.12 GB written per pass at 2^20 gates); "
                                "compiler-shaped gates: runs of gates read runs of values, the lines are shared"} if wide else None),
            "product_pass_roofline": product_pass_roofline(k, prof["layer_prod_pass"]["total_ms"] / steps, peak),
            "exchange": {"calls_per_step": exch["launches"] / steps, "us_per_call": exch["total_ms"] * 1e3 / exch["launches"]} if exch["launches"] else None,
            "collective": collective_info(world, exchange, exch, steps) if split else None,
            "kernel_ms_per_step": {n_: prof[n_]["total_ms"] / steps for n_ in names if prof[n_]["launches"]},
            "kernel_ms_source": "HIP events around the launches in a second pass of the same %d steps (the timed steps run without them)" % steps,
            "step_ms_each": [round(x * 1e3, 3) for x in each]}
    if d_W is not None:
        ctx.free(d_W)
    gates.close()
    ctx.close()
    return out


def product_pass_roofline(k, prod_ms, peak_products_per_sec):
    """The bound of a layer sumcheck's PRODUCT passes (kernels.hip: both phases as sumchecks of W X + Y over three tables of 2^k
    entries, three rounds per pass).  Since round 5 the passes over tables of 2^15 (cross sums) / 2^17 (pending folds) entries and more run on the matrix cores
    (mfma_cross.h, mfma_fold.h: the 254-bit products as int8 digit-matrix products, exact), which leaves them bound by the
    bytes they move: a first pass reads its three tables once; a later pass folds the previous pass's three variables (reads
    three tables of 2^m entries, writes them an eighth as long) and reads the folded tables for its cross sums.  Below 2^17
    entries the passes stay on v_mad_u64_u32 and are latency chains between two hashes (a few us of work each).  `achieved`
    is all of those bytes over the elapsed time of ALL the passes' kernels -- the small ones included, which is why the
    fraction is low; the large kernels alone: profiles/r05 (k_prod_cross_mfma 96 MiB in 30 us at k = 20).  The modular-product
    count and the chip's measured rate of such products on the VALU -- the bound before round 5 -- stay beside it."""
    if not prod_ms:
        return None
    products = bytes_ = 0.0
    for _phase in range(2):
        m, jp, rem = k, 0, k
        while rem > 0:
            J = min(3, rem)
            bytes_ += 3.0 * 32.0 * (1 << m)                       # the tables as they stand: read once
            if jp:
                products += 3.0 * (1 << m)
                bytes_ += 3.0 * 32.0 * (1 << (m - jp))             # the folded tables: written
                if m >= 17:
                    bytes_ += 3.0 * 32.0 * (1 << (m - jp))         # ... and read again by the cross-sum kernel
            m -= jp
            products += float(1 << (m + J))
            jp, rem = J, rem - J
    rate = products / (prod_ms * 1e-3)
    gbps = bytes_ / (prod_ms * 1e-3) / 1e9
    return {"bound": "hbm", "kernel": "k_prod_cross_mfma (2^15 entries and more) + k_prod_fold_mfma (2^17 and more), k_prod_cross<8|32> below, k_prod_publish",
            "hbm_bytes_per_sumcheck": bytes_, "achieved": gbps, "peak": PEAK_GBPS, "unit": "GB/s", "frac": gbps / PEAK_GBPS,
            "ms_per_sumcheck": prod_ms,
            "modular_products_per_sumcheck": products, "modular_products_per_sec": rate,
            "valu_product_rate_of_the_chip": peak_products_per_sec,
            "frac_of_the_valu_product_rate": rate / peak_products_per_sec if peak_products_per_sec else None,
            "valu_product_rate_fixed": PEAK_PRODUCTS_PER_SEC, "frac_of_the_fixed_valu_product_rate": rate / PEAK_PRODUCTS_PER_SEC,
            "note": "elapsed time of the passes' kernels (HIP events); the hand-offs between them are the host transcript's"}


def wide_prove_leg(world, ks=(18, 20, 20), reps=5):
    """A whole proof (prover::prove, prover.rs:6-96) of a circuit with WIDE layers -- 2^18 gates over 2^20 values over a 2^20-value
    input layer (gkr_amd.synth.wide_circuit) -- on every rank alike; the proof's arrays against the committed digest of the CPU
    checker's proof (tests/golden/config_hashes.json["prove"]).  Round 3 rejected this circuit (k[i+1] > 14)."""
    from gkr_amd import Context, synth
    circuit, _, wit = synth.wide_circuit(ks)
    with Context(world.local_rank) as ctx:
        t = time.perf_counter()
        arrs = ctx.prove_batch_raw(circuit, wit, all_arrays=True)     # uploads and sorts the circuit
        first = time.perf_counter() - t
        each = []
        for _ in range(reps):
            t = time.perf_counter()
            ctx.prove_batch_raw(circuit, wit, out=arrs)              # circuit in the context's cache, proof buffers reused
            each.append((time.perf_counter() - t) * 1e3)
    digest = synth.proof_arrays_digest(list(ks), *[a[0] for a in arrs[:7]])
    want = synth.golden_digest("prove", "k=" + ",".join(map(str, ks)))
    # d and input_func (the device Moebius transform, copied to the reused buffers by the helper thread on every repetition)
    coeff_digest = synth.proof_coeffs_digest(arrs[7][0], arrs[8][0])
    want_coeffs = synth.golden_digest("prove_coeffs", "k=" + ",".join(map(str, ks)))
    dt = world.max_over_ranks(statistics.median(each) / 1e3)
    if world.rank != 0:
        return None
    native = native_verify_all([circuit], [arrs]) if not os.environ.get("GKR_BENCH_NO_VERIFY") else None
    return {"verified_by_gkr_verify": native,
            "workload": "gkr_prove of a circuit with k = %s (gates per layer 2^%d, 2^%d; input layer 2^%d values), one witness" % (list(ks), ks[0], ks[1], ks[-1]),
            "ms_per_proof": dt * 1e3, "ms_each": [round(x, 3) for x in each], "first_call_ms": first * 1e3,
            "first_call": "gate arrays uploaded, gate lists sorted, workspaces and proof buffers allocated",
            "matches_golden_digest": None if want is None else (digest == want and (want_coeffs is None or coeff_digest == want_coeffs) and (native is None or native["ok"])),
            "proof_sha256": digest, "d_and_input_func_sha256": coeff_digest,
            "digest_covers": "sumcheck_proofs, lengths, sumcheck_r, q, q lengths, z, r" + ("; d and input_func by their own digest" if want_coeffs else "; d and input_func NOT covered (no golden digest)"),
            "outputs_bytes": int(sum(a.nbytes for a in arrs))}


# ------------------------------------------------------------------------------------------------ mode: mle-split

def collective_info(world, exchange=None, exch_prof=None, steps=1):
    """What the ranks' collective really was, for the line of an N > 1 run: the backend and world size torch.distributed
    reports (not what --gpus said), and the exchanges of a step."""
    info = {"backend": world.dist.get_backend() if world.grouped else None,
            "world_size_seen": world.dist.get_world_size() if world.grouped else 1,
            "transport": type(exchange).__name__ if exchange is not None else None}
    if exch_prof and exch_prof["launches"]:
        info["exchanges_per_step"] = exch_prof["launches"] / steps
        info["us_per_exchange"] = exch_prof["total_ms"] * 1e3 / exch_prof["launches"]
    return info


def mle_split_leg(world, n, batch, steps, warmup, ceilings=None, dump=None):
    """ONE plain sumcheck (prove_sumcheck, sumcheck.rs:158-214) on a table of 2^n points split over the ranks
    (gkr_sumcheck_mle_sharded_dev): rank p holds the entries whose index bits log2 P .. 1 are p, every pass's sub-block
    sums cross the ranks in one all-reduce on the library's stream, the last entries are gathered and every rank ends
    with the whole transcript.  `batch` such tables per step (default 1).  Strong scaling.  The transcript is compared
    with the committed digest of the oracle's (tests/golden/config_hashes.json: n = 16, 20, 24, 27, 30)."""
    from gkr_amd import Context, parallel, synth
    P_ = world.size
    lp = P_.bit_length() - 1
    if (1 << lp) != P_:
        return {"skipped": "the split needs a power-of-two number of ranks"} if world.rank == 0 else None
    ctx = Context(world.local_rank)
    count = 1 << (n - lp)
    d = ctx.alloc(batch * count * 32)
    seed0 = synth.SEED + (1 if n == 16 else 2)
    for b in range(batch):
        ctx.fill_shard(ctypes.c_void_p(d.value + b * count * 32), n, lp, world.rank, seed0 + 1000 * b)
    ctx.synchronize()
    limbs = parallel.exchange_limbs_mle(n, lp, batch)
    if world.grouped and os.environ.get("GKR_BENCH_NATIVE_RCCL") == "1":
        # the collective the LIBRARY owns (csrc/exchange_rccl.cpp): torch only hands the 128-byte id round
        exchange = parallel.RcclExchange.from_torch_group(world.local_rank, limbs)
    else:
        exchange = parallel.TorchCollective().device_exchange(limbs) if world.grouped else parallel.NoExchange(ctx, limbs)
    result = [None]

    def step():
        result[0] = parallel.sumcheck_mle_sharded_raw(ctx, d, n, lp, world.rank, exchange, batch)
    ctx.profile(1)
    elapsed, each = timed_steps(world, ctx, step, warmup, steps)
    ctx.profile(False)
    if dump and world.rank == 0:
        dump_outputs(dump, dict(zip(("coeffs", "lengths", "challenges"), result[0][:3])))
    names = ["mle_multifold", "mle_sub_sums", "mle_sub_reduce", "mle_pass_small", "mle_fold_plan"]
    prof = {k: ctx.profile_get(k) for k in names}
    exch = ctx.profile_get("exchange")
    C, L, R, nx = result[0]
    digest = synth.transcript_digest(C[0], L[0], R[0])
    want = synth.golden_digest("mle", "n=%d,seed=%d" % (n, seed0))
    ok = (digest == want) if want is not None else None
    bad_ranks = world.max_over_ranks(1.0 if ok is False else 0.0)
    out = None
    if world.rank == 0:
        dom = prof["mle_multifold"] if prof["mle_multifold"]["launches"] else prof["mle_sub_sums"]
        achieved = dom["bytes"] / (dom["total_ms"] * 1e-3) / 1e9 if dom["total_ms"] > 0 else None
        out = {
            "metric": "BN254-Fr sumcheck field-ops/sec @ 2^%d vars, ONE table split over the ranks" % n,
            "value": 5 * ((1 << n) - 1) * batch * steps / elapsed, "unit": "field-ops/s", "n_gpus": world.size, "steps": steps,
            "warmup": warmup, "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "u32x8 (BN254 Fr)", "data": "synthetic",
            "config": {"workload": "plain MLE sumcheck, ONE table of 2^%d points split over %d rank(s) (%d table(s) per step): rank p "
                                   "holds the entries whose index bits log2 P .. 1 are p (2^%d entries = %.1f MiB per table and rank)"
                                   % (n, P_, batch, n - lp, count * 32 / 2**20),
                       "exchanges": "one in-place int64 SUM all-reduce per pass of <= 5 rounds (batch x (2^J + 2) x 8 limbs) + one gather "
                                    "of the 2^6 entries every shard has left; on the library's HIP stream"},
            "collective": dict(collective_info(world, exchange, exch, steps), exchanges_per_sumcheck=nx, rounds_per_sumcheck=n),
            "matches_golden_digest": ok, "all_ranks_match": bad_ranks == 0.0, "transcript_sha256": digest,
            "roofline": {"bound": "hbm", "kernel": "k_mle_multifold_mfma (the shard's first fold pass)" if prof["mle_multifold"]["launches"] else "k_mle_sub_sums",
                         "achieved": achieved, "peak": PEAK_GBPS, "unit": "GB/s", "frac": achieved / PEAK_GBPS if achieved else None, "traffic": None,
                         "copy_GBps_measured": ceilings["copy_GBps"] if ceilings else None,
                         "note": "at 2^20 points a shard is a few MiB: the step is the latency of its passes, exchanges and hashes, not bandwidth"},
            "kernel_ms_per_step": {k: v["total_ms"] / steps for k, v in prof.items() if v["launches"]},
            "host_threads": transcript_threads(),
            "step_ms_each": [round(x * 1e3, 3) for x in each]}
    ctx.free(d)
    if hasattr(exchange, "close"):
        exchange.close()
    ctx.close()
    return out


def run_mle_split(args, world):
    out = mle_split_leg(world, args.n, args.split_batch, args.steps, args.warmup, dump=args.dump_outputs)
    if world.rank == 0:
        emit(out)
        if out.get("matches_golden_digest") is False or out.get("all_ranks_match") is False:
            raise SystemExit("WRONG TRANSCRIPT")


def run_layer_split(args, world):
    out = layer_leg(world, args.k_i, args.k, args.steps, args.warmup, split=True, dump=args.dump_outputs)
    if world.rank == 0:
        emit(out)
        if out["matches_golden_digest"] is False:
            raise SystemExit("WRONG TRANSCRIPT")


# ------------------------------------------------------------------------------------------------ CPU legs (rank 0, N = 1)

def cpu_dense(n, seconds):
    """The oracle's dense C prover (a port of the reference algorithm's dense form; the reference itself is Rust and
    cannot be built here), throughput-fair: one whole sumcheck per host core, all cores busy."""
    import threading
    from oracle import cdense
    cores = min(cdense.max_threads(), usable_cpus())
    table = cdense.fill_table(1 << n, 0xC0FFEE + 2)
    cdense.sumcheck_mle_raw(table, n, 1)   # warm-up (constants, page faults)
    done = [0] * cores
    stop = time.perf_counter() + seconds

    def work(i):
        while time.perf_counter() < stop:
            cdense.sumcheck_mle_raw(table, n, 1)
            done[i] += 1
    t0 = time.perf_counter()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(cores)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    dt = time.perf_counter() - t0
    return {"value": sum(done) * 5 * ((1 << n) - 1) / dt, "unit": "field-ops/s", "cores": cores, "kind": "port",
            "sample": "%d 2^%d-point sumchecks (MiMC7 included) in %.1f s, one single-threaded sumcheck per core on %d cores"
                      % (sum(done), n, dt, cores)}


def cpu_ref_algo(cap_seconds):
    """The reference's ACTUAL algorithm (term lists, sumcheck.rs:36-156) as the oracle restates it in Python
    (oracle/termlist.py), at the largest size whose run stays under the cap -- size stated, nothing extrapolated.
    It documents the algorithmic gap (time grows ~16x per extra variable pair), not a speed to compare with."""
    import random
    from oracle import termlist
    from oracle.field import P
    best = None
    for k in range(1, 8):
        rng = random.Random(99 + k)
        k_i = k
        g = 1 << k_i
        gt = [rng.randint(0, 1) for _ in range(g)]
        l = [rng.randrange(1 << k) for _ in range(g)]
        r = [rng.randrange(1 << k) for _ in range(g)]
        layer = termlist.build_layer(k_i, k, gt, l, r)
        z = [rng.randrange(P) for _ in range(k_i)]
        w = termlist.get_multi_ext([rng.randrange(P) for _ in range(1 << k)], k)
        t = time.perf_counter()
        add_i = termlist.partial_eval_binary_form(layer.add, z)
        mult_i = termlist.partial_eval_binary_form(layer.mult, z)
        f1 = [termlist.extend_length(t_, 2 * k + 1) for t_ in w]
        f2 = termlist.modify_poly_from_k(w, k)
        termlist.prove_sumcheck_opt(layer.wire[0], layer.wire[1], add_i, mult_i, f1, f2, 2 * k)
        dt = time.perf_counter() - t
        if dt > cap_seconds:
            break
        best = {"v": 2 * k, "gates": g, "seconds": dt, "value": 25 * ((1 << (2 * k)) - 1) / dt}
        if dt * 16 > cap_seconds:
            break
    if best is None:
        return None
    return {"value": best["value"], "unit": "field-ops/s", "cores": 1, "kind": "port",
            "sample": "prove_sumcheck_opt term-list algorithm (pure-Python restatement of sumcheck.rs:36-156), largest layer under "
                      "%.0f s: v = %d variables, %d gates, %.2f s" % (cap_seconds, best["v"], best["gates"], best["seconds"])}


def cpu_pipeline():
    """The oracle proving the demo circuit's 12 sub-circuits for the three example inputs (dense C prover)."""
    from gkr_amd import synth
    from oracle import cdense
    from oracle import convert as oconv
    r = oconv.read_r1cs(synth.mimc7_demo_r1cs().serialize())
    t0 = time.perf_counter()
    proofs = 0
    for a, b in synth.EXAMPLE_INPUTS:
        for sub in oconv.convert_r1cs_wtns_gkr(r, synth.mimc7_demo_witness(a, b)):
            cdense.prove(sub["layers"], sub["input_values"])
            proofs += 1
    dt = time.perf_counter() - t0
    return {"value": proofs / dt, "unit": "proofs/s", "cores": min(cdense.max_threads(), usable_cpus()), "kind": "port",
            "sample": "%d proofs (3 example inputs x 12 sub-circuits of the t.circom-equivalent R1CS), compile included, %.2f s" % (proofs, dt)}


_REAL_STDOUT = None
DETAIL_PATH = os.environ.get("GKR_BENCH_DETAIL", os.path.join(REPO, "bench_detail.json"))
LINE_LIMIT = 6000   # bytes of the ONE stdout line (a 20 KB line was not parsed by the driver)

_CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
             "dtype", "data", "config")
_ROOFLINE = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_us", "algorithmic_bytes_per_launch",
             "launches", "copy_GBps_measured", "frac_of_copy", "traffic_source")
_CPU = ("value", "unit", "cores", "kind", "sample")


def _short(v, limit=200):
    """A scalar as it goes on the stdout line: floats to 6 significant digits, strings cut to `limit` characters."""
    if isinstance(v, float):
        return float("%.9g" % v)
    if isinstance(v, str) and len(v) > limit:
        return v[:limit - 3] + "..."
    return v


def _leg(v):
    """One secondary leg as {ms, ok, ...}: its step time, whether its outputs passed their check, its roofline fraction."""
    out = {}
    for k in ("ms_per_step", "ms", "ms_per_proof"):
        if isinstance(v.get(k), (int, float)):
            out["ms"] = _short(float(v[k]))
            break
    ok = v.get("matches_golden_digest", v.get("whole_batch_digest"))
    ver = v.get("verified")
    if ok is None and isinstance(ver, dict):
        ok = ver.get("ok")
    if "error" in v:
        ok, out["error"] = False, _short(str(v["error"]), 160)
    out["ok"] = ok
    for k in ("value", "proofs_per_sec", "compile_ms", "direct_ms_same_process", "ms_over_direct"):
        if isinstance(v.get(k), (int, float)):
            out[k] = _short(float(v[k]))
    if isinstance(v.get("unit"), str) and "value" in out:
        out["unit"] = v["unit"]
    r = v.get("roofline")
    if isinstance(r, dict) and isinstance(r.get("frac"), (int, float)):
        out["roofline_frac"] = _short(float(r["frac"]))
        out["bound"] = "host-hash" if str(r.get("bound")).startswith("host transcript") else _short(str(r.get("bound")), 24)
    return out


def compact_line(full):
    """The stdout line: the contract's keys, `roofline` and `cpu_baseline` with scalar fields only, `verified.ok`, and a flat
    `legs` summary {name: {ms, ok, ...}} of everything else; the whole of `full` goes to bench_detail.json and stderr."""
    line = {k: full[k] for k in _CONTRACT if k in full}
    if isinstance(line.get("dtype"), str):
        line["dtype"] = line["dtype"].split(" ")[0]
    line = {k: (_short(v) if not isinstance(v, dict) else {a: _short(b, 160) for a, b in v.items() if not isinstance(b, (dict, list))})
            for k, v in line.items()}
    if isinstance(full.get("roofline"), dict):
        line["roofline"] = {k: _short(full["roofline"].get(k), 120) for k in _ROOFLINE if k in full["roofline"]}
        line["roofline"].setdefault("traffic", None)
    if isinstance(full.get("cpu_baseline"), dict):
        line["cpu_baseline"] = {k: _short(full["cpu_baseline"].get(k), 160) for k in _CPU}
    ver = full.get("verified")
    if isinstance(ver, dict):
        line["verified"] = {k: ver[k] for k in ("ok", "all_ranks_ok", "tables_matching_their_digest", "whole_batch_digest") if k in ver}
    elif "matches_golden_digest" in full:
        line["verified"] = {"ok": full["matches_golden_digest"] is not False and full.get("all_ranks_match") is not False}
    legs = {}
    for name, v in full.items():
        if name in line or not isinstance(v, dict) or name in ("exit", "host_threads", "host_transcript", "kernel_ms", "collective",
                                                               "kernel_ms_per_step", "exchange", "memory", "product_pass_roofline"):
            continue
        if name == "aggregated_proofs":
            for sub, sv in v.items():
                if isinstance(sv, dict) and ("ms" in sv or "error" in sv):
                    legs[{"config0_three_inputs": "config0", "config3": "config3"}.get(sub, sub)] = _leg(sv)
        else:
            legs[name] = _leg(v)
    if legs:
        line["legs"] = legs
    for k in ("exchange", "collective"):
        if isinstance(full.get(k), dict):
            line[k] = {a: _short(b, 80) for a, b in full[k].items() if not isinstance(b, (dict, list))}
    if "exit" in full:
        line["exit"] = full["exit"]
    line["detail"] = os.path.basename(DETAIL_PATH)
    for drop in ("collective", "exchange", "legs"):       # (never reached with today's legs: ~3 KB)
        if len(json.dumps(line)) < LINE_LIMIT:
            break
        line.pop(drop, None)
    return line


def emit_raw(obj):
    """A child leg's result for its parent (bench.py --mode multi-device): the whole object on stdout, no detail file."""
    data = (json.dumps(obj) + "\n").encode()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, data)


def emit(obj):
    """The ONE JSON line of the contract, on the process's real stdout (see main): at most LINE_LIMIT bytes.  Every other
    figure of the run goes to bench_detail.json beside this file (GKR_BENCH_DETAIL overrides the path) and to stderr."""
    full = json.dumps(obj, indent=1)
    try:
        with open(DETAIL_PATH, "w") as f:
            f.write(full + "\n")
    except OSError as e:
        sys.stderr.write("bench.py: could not write %s (%s)\n" % (DETAIL_PATH, e))
    sys.stderr.write("bench.py detail (also in %s): %s\n" % (DETAIL_PATH, json.dumps(obj)))
    sys.stderr.flush()
    data = (json.dumps(compact_line(obj)) + "\n").encode()
    assert len(data) < LINE_LIMIT, len(data)
    if _REAL_STDOUT is None:
        sys.stdout.write(data.decode())
        sys.stdout.flush()
    else:
        while data:                      # (a pipe may take the line in pieces)
            data = data[os.write(_REAL_STDOUT, data):]


def visible_devices():
    """GPUs this process would see, counted in a CHILD process (counting must not initialise the GPU in a process that is
    about to start other programs; -1 when torch cannot say)."""
    import subprocess
    try:
        out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True,
                             text=True, timeout=600)
        return int(out.stdout.strip().splitlines()[-1])
    except Exception:
        return -1


def launch_ranks(n):
    """`python bench.py --gpus N` with no launcher around it: this process has not imported torch or touched the GPU; it
    starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py <the same arguments>` as a CHILD
    process (never an exec), relays rank 0's one JSON line to the real stdout and returns the child's exit code.  One
    process per GPU over RCCL -- the multi-GPU twin of the one process whose par_iter fans prover::prove out
    (rust/src/aggregator.rs:350-355, 411-416)."""
    import socket
    import subprocess
    test_hook = "GKR_BENCH_DEVICE" in os.environ   # several ranks on ONE device (gloo): single-GPU boxes exercising N > 1
    if not test_hook:
        seen = visible_devices()
        if 0 <= seen < n:
            sys.stderr.write("bench.py: --gpus %d but only %d device(s) visible (set GKR_BENCH_DEVICE=<id> and "
                             "GKR_BENCH_BACKEND=gloo to run the ranks on one device as a test)\n" % (n, seen))
            return 3
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=None, env=env, start_new_session=True)
    try:
        lines = 0
        relayed_exit = None
        for raw in child.stdout:
            if raw.lstrip().startswith(b"{") and lines == 0:
                try:
                    relayed_exit = json.loads(raw.decode()).get("exit", {}).get("code")
                except Exception:   # noqa: BLE001
                    pass
                os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, raw if raw.endswith(b"\n") else raw + b"\n")
                lines += 1
            else:
                sys.stderr.buffer.write(raw)
        rc = child.wait()
    except BaseException:
        import signal
        try:
            os.killpg(child.pid, signal.SIGTERM)   # exactly the process group started above
        except ProcessLookupError:
            pass
        raise
    if rc == 0 and lines != 1:
        sys.stderr.write("bench.py: the ranks exited 0 without a JSON line\n")
        return 5
    if rc != 0 and lines == 1 and relayed_exit in (2, 4) and os.environ.get("GKR_BENCH_LENIENT_EXIT") == "1":
        # Opt-in only: the line is out and says what happened (`exit`), a split leg failed (2) or hung (4) after the verified
        # headline.  By default that IS the run's exit code: a broken RCCL path must go red on the first multi-GPU box.
        sys.stderr.write("bench.py: a split leg failed after the verified headline (see the line's `exit`); GKR_BENCH_LENIENT_EXIT=1: exit code 0\n")
        return 0
    if rc == 0 and relayed_exit not in (None, 0):
        return int(relayed_exit)
    return rc


def main():
    # Libraries below write banners to stdout (RCCL: version / hostname lines at start-up and shutdown; gloo: "Rank n is
    # connected ..."): file descriptor 1 is pointed at stderr for the whole run and the JSON line goes to the saved one.
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["mle", "proofs", "layer-split", "mle-split", "multi-device"], default="mle")
    ap.add_argument("--split-batch", type=int, default=1, help="mle-split: tables per step, each split over all ranks")
    ap.add_argument("--n", "--log2-points", dest="n", type=int, default=20, help="log2 of the table size (--log2-points under torch.distributed.run, whose own parser claims --n)")
    ap.add_argument("--batch", type=int, default=1024, help="independent sumchecks per rank per step (32 GiB of tables)")
    ap.add_argument("--transcript", choices=["host", "device"], default="host",
                    help="where MiMC7 runs (host cores between launches, or one GPU lane per sumcheck)")
    ap.add_argument("--full", action="store_true",
                    help="mle mode: also the roofline, the check of the timed outputs, the CPU baselines and every other leg")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's output arrays as DIR/<name>.npy (float64)")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event timing")
    ap.add_argument("--no-extras", action="store_true", help="skip the batch-1 latency and the 2^16 leg")
    ap.add_argument("--proofs", type=int, default=64, help="inputs of the demo circuit (configs[3]); 0 = skip in mle mode")
    ap.add_argument("--k-i", type=int, default=24, help="layer-split: log2 gates")
    ap.add_argument("--k", type=int, default=12, help="layer-split: log2 entries of the next layer")
    ap.add_argument("--layer-k-i", type=int, default=24, help="mle mode: log2 gates of the configs[4] leg on the line (0 = skip)")
    ap.add_argument("--layer-k", type=int, default=12)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the check of the timed outputs (digests + verifier relations)")
    ap.add_argument("--cpu-seconds", type=float, default=4.0)
    ap.add_argument("--ref-algo-seconds", type=float, default=20.0)
    args = ap.parse_args()
    if args.mode == "multi-device":   # (the default line's multi_device leg, run as its child)
        emit_raw(multi_device_leg(args.proofs))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))
    world = World()
    if world.size != max(1, args.gpus) and world.size > 1:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d ranks" % (args.gpus, world.size))
    try:
        {"mle": run_mle, "proofs": run_proofs, "layer-split": run_layer_split, "mle-split": run_mle_split}[args.mode](args, world)
    finally:
        world.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Golden digests of the oracle's transcripts at BASELINE config sizes (too large to commit as vectors).

    python tests/golden/make_config_hashes.py      # rewrites tests/golden/config_hashes.json (~1 min of CPU)
    python tests/golden/make_config_hashes.py --bench-batch   # rewrites tests/golden/bench_batch_hashes.json (~6 min, 8 cores)
    python tests/golden/make_config_hashes.py --limits   # adds the size-limit workloads of tests/test_gpu_limits.py to
                                                          # config_hashes.json (~10 min on 8 cores, up to ~16 GiB of memory)

For each workload of gkr_amd.synth the C oracle (oracle/c, pinned against the reference-generated fixtures by
tests/test_oracle_*.py) produces the transcript; what is committed is sha256 over the raw output arrays
(coefficients | lengths | challenges, the C ABI's layout).  bench.py and tools/bench_layer.py compare the GPU
transcript of the workload they time against these digests without running the oracle.
"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from gkr_amd import synth  # noqa: E402
from oracle import cdense  # noqa: E402


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _bench_table_transcript(seed):
    """One table of bench.py's default workload: fill_table(2^20, seed) -> the oracle's (C, L, R) as bytes, and the
    transcripts of its sixteen 2^16-point slices (what the n16 leg proves on the same memory)."""
    table = cdense.fill_table(1 << 20, seed)
    C, L, R = cdense.sumcheck_mle_raw(table, 20, 1)
    slices = [cdense.sumcheck_mle_raw(table[j << 16:(j + 1) << 16], 16, 1) for j in range(16)]
    return seed, (C.tobytes(), L.tobytes(), R.tobytes()), [(c.tobytes(), l.tobytes(), r.tobytes()) for c, l, r in slices]


def bench_batch_digests(ranks=8, batch=1024, n16_tables=4096):
    """Digests of everything bench.py's default line times (gkr_amd.synth.bench_table_seed): per rank the whole batch of
    1024 x 2^20 transcripts (sha256 over the C | L | R output arrays as the C ABI lays them out for the batch), rank 0's
    tables one by one (first 16 hex digits), and rank 0's 4096 x 2^16 leg."""
    import multiprocessing
    seeds = sorted({synth.bench_table_seed(r, b) for r in range(ranks) for b in range(batch)})
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        done = {}
        n16 = {}
        for seed, t20, t16 in pool.imap_unordered(_bench_table_transcript, seeds, chunksize=4):
            done[seed] = t20
            if seed < synth.bench_table_seed(0, 0) + n16_tables // 16:
                n16[seed] = t16
    out = {"batch": batch, "n": 20, "whole_batch_by_rank": {}, "rank0_tables": [], "n16_whole_batch_rank0": None, "n16_tables": n16_tables}
    for r in range(ranks):
        hc, hl, hr = [], [], []
        for b in range(batch):
            c, l, rr = done[synth.bench_table_seed(r, b)]
            hc.append(c), hl.append(l), hr.append(rr)
        out["whole_batch_by_rank"][str(r)] = hashlib.sha256(b"".join(hc) + b"".join(hl) + b"".join(hr)).hexdigest()
    for b in range(batch):
        out["rank0_tables"].append(hashlib.sha256(b"".join(done[synth.bench_table_seed(0, b)])).hexdigest()[:16])
    hc, hl, hr = [], [], []
    for j in range(n16_tables):
        c, l, rr = n16[synth.bench_table_seed(0, j >> 4)][j & 15]
        hc.append(c), hl.append(l), hr.append(rr)
    out["n16_whole_batch_rank0"] = hashlib.sha256(b"".join(hc) + b"".join(hl) + b"".join(hr)).hexdigest()
    return out


def _demo_digests(pair):
    from oracle import convert as oconv
    a, b = pair
    r = _demo_digests.r1cs
    return [synth.proof_digest(p["sumcheck_proofs"], p["sumcheck_r"], p["q"], p["z"], p["r"])[:16]
            for p in (cdense.prove(sub["layers"], sub["input_values"]) for sub in oconv.convert_r1cs_wtns_gkr(r, synth.mimc7_demo_witness(a, b)))]


def proof_digests(n_inputs=64):
    """The CPU checker's proofs (oracle/convert.py + the dense C prover, both pinned by the reference's fixtures / the
    hand-derived circuits) of the demo circuit's 12 sub-circuits: configs[0]'s three example inputs and the 64 inputs of
    configs[3], one 16-hex-digit digest per (input, sub-circuit)."""
    from oracle import convert as oconv
    _demo_digests.r1cs = oconv.read_r1cs(synth.mimc7_demo_r1cs().serialize())
    # (serially: ~10 s; a process pool forked after the C checker's OpenMP runtime has started hangs)
    ex = [_demo_digests(p) for p in synth.EXAMPLE_INPUTS]
    many = [_demo_digests(p) for p in synth.demo_proof_inputs(n_inputs)]
    return {"what": "sha256[:16] of gkr_amd.synth.proof_digest over (sumcheck_proofs, sumcheck_r, q, z, r) per (input, sub-circuit)",
            "config0": {"inputs": [list(p) for p in synth.EXAMPLE_INPUTS], "digests": ex},
            "config3": {"inputs": n_inputs, "digests": many}}


def large_r1cs_digests(nrounds=65536, pair=(2, 3)):
    """A 262 144-constraint R1CS (gkr_amd.synth.mimc7_demo_r1cs with 65 536 rounds: the demo's constraint shapes, the
    constants repeating) through the CPU checker END TO END: oracle/convert.py's restatement of convert.rs compiles it into
    its layered circuits (layers of 2^14 .. 2^16 values), the linear-time C prover proves each for one witness; per sub-circuit
    the k list and the digest of the proof's arrays (gkr_amd.synth.proof_arrays_digest)."""
    import time
    from oracle import convert as oconv
    t = time.time()
    r = oconv.read_r1cs(synth.mimc7_demo_r1cs(nrounds=nrounds).serialize())
    subs = oconv.convert_r1cs_wtns_gkr(r, synth.mimc7_demo_witness(pair[0], pair[1], nrounds=nrounds))
    print("oracle compile: %.0f s, %d sub-circuits" % (time.time() - t, len(subs)), flush=True)
    out = {"what": "sha256 of gkr_amd.synth.proof_arrays_digest per sub-circuit; compile and proofs by the CPU checker",
           "nrounds": nrounds, "constraints": 4 * nrounds, "input": list(pair), "k": [], "digests": [], "coeff_digests": []}
    for sub in subs:
        layers = [(np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint32), np.asarray(c, dtype=np.uint32)) for a, b, c in sub["layers"]]
        ref = cdense.prove_raw(layers, cdense.to_limbs(sub["input_values"]))
        out["k"].append(list(sub["k"]))
        out["digests"].append(synth.proof_arrays_digest(list(sub["k"]), *synth.proof_arrays_from_checker(ref, list(sub["k"]))))
        out["coeff_digests"].append(synth.proof_coeffs_digest(cdense.mobius_raw(ref["values"][0], ref["k"][0]), cdense.mobius_raw(ref["values"][-1], ref["k"][-1])))
    return out


LIMIT_LAYERS = ((28, 12), (28, 14), (20, 24), (28, 24))   # GKR_MAX_K_I = 28, GKR_MAX_K_NEXT = 24 (include/gkr_amd.h)
LIMIT_PROOF = (18, 24, 24)
LIMIT_BATCH = (65535, (2, 14))   # gkr_sumcheck_mle_batch_device's cap on sumchecks per call, at two table sizes
LIMIT_PROOFS = 4096              # GKR_MAX_BATCH: proofs per gkr_prove_batch


def batch_table_seed(seed, j, n):
    """The seed with which oracle/c's fill_table(2^n, .) writes table j of fill_table(B * 2^n, seed) (entry i's limbs hash
    seed + (4 i + limb + 1) * 0x9E3779B97F4A7C15, so a slice is a fill of its own with the seed moved along)."""
    return (seed + 4 * (j << n) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def _mle_batch_part(args):
    n, seed, lo, hi = args
    cdense.lib().ogkr_set_threads(1)   # (one OpenMP thread per process: eight processes of eight spinning threads crawl)
    tables = cdense.fill_table((hi - lo) << n, batch_table_seed(seed, lo, n))
    out = [cdense.sumcheck_mle_raw(tables[(j << n):((j + 1) << n)], n, 1) for j in range(hi - lo)]
    return lo, [np.stack(x) for x in zip(*out)]


def mle_batch_digest(batch, n, seed):
    """sha256 over the (C | L | R) arrays of gkr_sumcheck_mle_batch_device on fill_table(batch * 2^n, seed), the C ABI's layout
    for the whole batch; each table's transcript by the C oracle, in spawned processes (one thread each)."""
    import multiprocessing
    C = np.zeros((batch, n, 2, 4), dtype=np.uint64)
    L = np.zeros((batch, n), dtype=np.uint32)
    R = np.zeros((batch, n, 4), dtype=np.uint64)
    step = 256
    parts = [(n, seed, lo, min(batch, lo + step)) for lo in range(0, batch, step)]
    with multiprocessing.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        for lo, (c, l, r) in pool.imap_unordered(_mle_batch_part, parts):
            C[lo:lo + len(c)], L[lo:lo + len(c)], R[lo:lo + len(c)] = c, l, r
    return digest(C, L, R)


def _proof_batch_part(args):
    lo, hi = args
    cdense.lib().ogkr_set_threads(1)
    circuit = synth.proof_batch_circuit()
    raw, ks = [lay.arrays() for lay in circuit.layer], synth.PROOF_BATCH_KS
    out = []
    for w in synth.proof_batch_witnesses(hi - lo, first=lo):
        ref = cdense.prove_raw(raw, w, 1)
        out.append(list(synth.proof_arrays_from_checker(ref, ks)) + [cdense.mobius_raw(ref["values"][0], ks[0]), cdense.mobius_raw(ref["values"][-1], ks[-1])])
    return lo, out


def proof_batch_digest(n_proofs):
    """gkr_amd.synth.proof_batch_digest of the C oracle's proofs of synth.proof_batch_circuit() for the first n_proofs witnesses
    of synth.proof_batch_witnesses, in spawned processes (one thread each)."""
    import multiprocessing
    proofs = [None] * n_proofs
    step = 128
    with multiprocessing.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        for lo, part in pool.imap_unordered(_proof_batch_part, [(lo, min(n_proofs, lo + step)) for lo in range(0, n_proofs, step)]):
            proofs[lo:lo + len(part)] = part
    return synth.proof_batch_digest(synth.PROOF_BATCH_KS, [np.stack(x) for x in zip(*proofs)])


def limits_digests(path):
    """The workloads of tests/test_gpu_limits.py, at the ABI's size limits: adds the keys the committed file lacks, writing
    it after each (the largest take minutes and up to ~16 GiB of host memory)."""
    import time
    cur = json.load(open(path))

    def put(kind, key, fn):
        if key in cur.setdefault(kind, {}):
            return
        t = time.time()
        cur[kind][key] = fn()
        with open(path, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")
        print("%s %s: %.0f s" % (kind, key, time.time() - t), flush=True)

    # (the batches first: their process pool is spawned before this process starts the oracle's OpenMP runtime)
    batch, ns = LIMIT_BATCH
    for n in ns:
        put("mle_batch", "batch=%d,n=%d,seed=%d" % (batch, n, synth.SEED + 11), lambda: mle_batch_digest(batch, n, synth.SEED + 11))
    put("prove_batch", "k=%s,proofs=%d" % (",".join(map(str, synth.PROOF_BATCH_KS)), LIMIT_PROOFS), lambda: proof_batch_digest(LIMIT_PROOFS))

    def mle_inplace(n):
        C, L, R = cdense.sumcheck_mle_inplace_raw(cdense.fill_table(1 << n, synth.SEED + 2), n)   # 2^29 points: 16 GiB
        return digest(C, L, R)
    put("mle", "n=29,seed=%d" % (synth.SEED + 2), lambda: mle_inplace(29))
    for k_i, k in LIMIT_LAYERS:
        def layer():
            lay, z, W = synth.config5_layer(k_i, k)
            return digest(*cdense.sumcheck_layer_lin_raw(k_i, k, lay.gate_type, lay.left, lay.right, z, W))
        put("layer", "k_i=%d,k=%d" % (k_i, k), layer)
    ks = LIMIT_PROOF
    key = "k=" + ",".join(map(str, ks))
    proof = {}

    def prove():
        circuit, raw, wit = synth.wide_circuit(ks)
        ref = cdense.prove_raw(raw, wit[0])
        proof["coeffs"] = synth.proof_coeffs_digest(cdense.mobius_raw(ref["values"][0], ks[0]), cdense.mobius_raw(ref["values"][-1], ks[-1]))
        return synth.proof_arrays_digest(list(ks), *synth.proof_arrays_from_checker(ref, list(ks)))
    put("prove", key, prove)
    if "coeffs" in proof:
        put("prove_coeffs", key, lambda: proof["coeffs"])


def main():
    if "--limits" in sys.argv:   # only the size-limit workloads (tests/test_gpu_limits.py), added to the committed file
        limits_digests(os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_hashes.json"))
        return
    if "--large-r1cs" in sys.argv:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "large_r1cs_digests.json")
        with open(path, "w") as f:
            json.dump(large_r1cs_digests(), f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", path)
        return
    if "--proofs" in sys.argv:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "proof_digests.json")
        with open(path, "w") as f:
            json.dump(proof_digests(), f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", path)
        return
    if "--circom-shaped" in sys.argv:   # only the compiler-shaped wide layer's digest, added to the committed file
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_hashes.json")
        cur = json.load(open(path))
        for k_i, k in ((20, 20),):
            lay, z, W = synth.circom_shaped_layer(k_i, k)
            C, L, R = cdense.sumcheck_layer_lin_raw(k_i, k, lay.gate_type, lay.left, lay.right, z, W)
            cur["layer"]["circom-shaped,k_i=%d,k=%d" % (k_i, k)] = digest(C, L, R)
        with open(path, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path)
        return
    if "--prove-coeffs" in sys.argv:   # only the d / input_func digests of the wide proof, added to the committed file
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_hashes.json")
        cur = json.load(open(path))
        cur["prove_coeffs"] = {}
        for ks in ((18, 20, 20),):
            circuit, raw, wit = synth.wide_circuit(ks)
            ref = cdense.prove_raw(raw, wit[0])
            assert cur["prove"]["k=" + ",".join(map(str, ks))] == synth.proof_arrays_digest(list(ks), *synth.proof_arrays_from_checker(ref, list(ks)))
            cur["prove_coeffs"]["k=" + ",".join(map(str, ks))] = synth.proof_coeffs_digest(cdense.mobius_raw(ref["values"][0], ks[0]), cdense.mobius_raw(ref["values"][-1], ks[-1]))
        with open(path, "w") as f:
            json.dump(cur, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path)
        return
    out = {"what": "sha256(coeffs | lens | challenges) of the C oracle's transcript; inputs: gkr_amd.synth", "layer": {}, "mle": {}}
    if "--bench-batch" in sys.argv:   # ~6 min on 8 cores: kept in its own file, regenerated only when asked
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_batch_hashes.json")
        with open(path, "w") as f:
            json.dump(bench_batch_digests(), f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", path)
        return
    for k_i, k in ((16, 8), (20, 10), (24, 12)):
        lay, z, W = synth.config5_layer(k_i, k)
        C, L, R = cdense.sumcheck_layer_raw(k_i, k, lay.gate_type, lay.left, lay.right, z, W)
        out["layer"]["k_i=%d,k=%d" % (k_i, k)] = digest(C, L, R)
    # a WIDE layer (2^20 gates over a next layer of 2^20 values: the shape of a compiled R1CS's big layers), by the linear-time
    # C prover -- the dense form cannot follow
    for k_i, k in ((20, 20),):
        lay, z, W = synth.config5_layer(k_i, k)
        C, L, R = cdense.sumcheck_layer_lin_raw(k_i, k, lay.gate_type, lay.left, lay.right, z, W)
        out["layer"]["k_i=%d,k=%d" % (k_i, k)] = digest(C, L, R)
    # a whole proof through wide layers (gkr_amd.synth.wide_circuit): the limb-only CPU prover on the linear-time layer form
    out["prove"] = {}
    for ks in ((18, 20, 20),):
        circuit, raw, wit = synth.wide_circuit(ks)
        ref = cdense.prove_raw(raw, wit[0])
        out["prove"]["k=" + ",".join(map(str, ks))] = synth.proof_arrays_digest(list(ks), *synth.proof_arrays_from_checker(ref, list(ks)))
        out["prove_coeffs"] = out.get("prove_coeffs", {})
        out["prove_coeffs"]["k=" + ",".join(map(str, ks))] = synth.proof_coeffs_digest(cdense.mobius_raw(ref["values"][0], ks[0]), cdense.mobius_raw(ref["values"][-1], ks[-1]))
    for n, seed in ((16, synth.SEED + 1), (20, synth.SEED + 2)):
        C, L, R = cdense.sumcheck_mle_raw(cdense.fill_table(1 << n, seed), n)
        out["mle"]["n=%d,seed=%d" % (n, seed)] = digest(C, L, R)
    # the tables bench.py --mode mle-split splits over the ranks (seed SEED + 2 at every size); 2^30 points = 32 GiB of
    # table: in place, only with --huge (kept from the committed file otherwise)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_hashes.json")
    try:
        old = json.load(open(path))["mle"]
    except (OSError, KeyError, ValueError):
        old = {}
    for n in (24, 27, 30):
        key = "n=%d,seed=%d" % (n, synth.SEED + 2)
        if n == 30 and "--huge" not in sys.argv:
            if key in old:
                out["mle"][key] = old[key]
            continue
        C, L, R = cdense.sumcheck_mle_inplace_raw(cdense.fill_table(1 << n, synth.SEED + 2), n)
        out["mle"][key] = digest(C, L, R)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "config_hashes.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()

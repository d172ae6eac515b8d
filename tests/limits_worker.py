"""Child process of tests/test_gpu_limits.py: one workload at a size limit of include/gkr_amd.h, in a process of its own
(tables of up to 32 GiB on the device, gate arrays and eq tables of several GiB on the host, none of it in the pytest
process).  Inputs come from the device's fill_table or gkr_amd.synth's seeds; outputs are compared bit for bit with the
committed digests of the C oracle's transcripts (tests/golden/config_hashes.json, tests/golden/make_config_hashes.py
--limits) or with the oracle itself.  Prints the workload's wall time and OK, or what did not match.

    python limits_worker.py mle <n> [option=value ...]   (option "transcript=device": the device transcript)
    python limits_worker.py mle-batch <n>
    python limits_worker.py prove-batch
    python limits_worker.py layer <k_i> <k>
    python limits_worker.py prove-wide
    python limits_worker.py layer-device-transcript <k_i> <k>"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gkr_amd import Context, synth  # noqa: E402
from gkr_amd import _native as N  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_config_hashes import LIMIT_PROOF, LIMIT_PROOFS  # noqa: E402

MAX_MLE_BATCH = 65535   # sumchecks per gkr_sumcheck_mle_batch_device call


def context(options):
    ctx = Context(0)
    for o in options:
        name, value = o.split("=")
        if name == "transcript":
            ctx.set_transcript({"device": N.GKR_TRANSCRIPT_DEVICE, "host": N.GKR_TRANSCRIPT_HOST}[value])
        else:
            ctx.set_option(name, int(value))
            assert ctx.get_option(name) == int(value), name
    return ctx


def expect(kind, key, got):
    want = synth.golden_digest(kind, key)
    if want is None:
        return "no committed digest %s / %s" % (kind, key)
    return None if got == want else "MISMATCH against the committed digest %s / %s" % (kind, key)


def mle(n, *options):
    # the table of config_hashes.json["mle"] (seed SEED + 2 at every size): 2^n points generated on the device
    count = 1 << n
    with context(options) as ctx:
        d = ctx.alloc(count * 32)
        try:
            ctx.fill_table(d, count, synth.SEED + 2)
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, 1)
        finally:
            ctx.free(d)
    return expect("mle", "n=%d,seed=%d" % (n, synth.SEED + 2), synth.transcript_digest(C[0], L[0], R[0]))


def mle_batch(n):
    # 65535 tables of 2^n points: ONE fill over all of them (table j is oracle/c's fill_table(2^n) with its seed moved along,
    # make_config_hashes.batch_table_seed), one call
    count = MAX_MLE_BATCH << n
    with Context(0) as ctx:
        d = ctx.alloc(count * 32)
        try:
            ctx.fill_table(d, count, synth.SEED + 11)
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, MAX_MLE_BATCH)
        finally:
            ctx.free(d)
    return expect("mle_batch", "batch=%d,n=%d,seed=%d" % (MAX_MLE_BATCH, n, synth.SEED + 11), synth.transcript_digest(C, L, R))


def prove_batch():
    from gkr_amd.dropin import verify_native
    circuit = synth.proof_batch_circuit()
    with Context(0) as ctx:
        arrs = ctx.prove_batch_raw(circuit, synth.proof_batch_witnesses(LIMIT_PROOFS), all_arrays=True)
    bad = expect("prove_batch", "k=%s,proofs=%d" % (",".join(map(str, synth.PROOF_BATCH_KS)), LIMIT_PROOFS),
                 synth.proof_batch_digest(synth.PROOF_BATCH_KS, arrs))
    for b in (0, 1, 2047, LIMIT_PROOFS - 1):
        if verify_native(circuit, arrs, index=b) != (True, 0, 0):
            bad = (bad or "") + " gkr_verify rejects proof %d" % b
    return bad


def layer(k_i, k):
    # config5_layer's default seed: the layers of config_hashes.json["layer"]
    lay, z, W = synth.config5_layer(k_i, k)
    with Context(0) as ctx:
        C, L, R = ctx.sumcheck_layer_raw(lay, k, z, W)
    return expect("layer", "k_i=%d,k=%d" % (k_i, k), synth.transcript_digest(C, L, R))


def prove_wide():
    # an input layer of 2^24 values: the Moebius transform of input_func and the line restriction at GKR_MAX_K_NEXT
    from gkr_amd.dropin import verify_native
    ks = list(LIMIT_PROOF)
    circuit, _, wit = synth.wide_circuit(ks)
    with Context(0) as ctx:
        arrs = ctx.prove_batch_raw(circuit, wit, all_arrays=True)
    key = "k=" + ",".join(map(str, ks))
    bad = expect("prove", key, synth.proof_arrays_digest(ks, *[a[0] for a in arrs[:7]]))
    bad = bad or expect("prove_coeffs", key, synth.proof_coeffs_digest(arrs[7][0], arrs[8][0]))
    if verify_native(circuit, arrs, index=0) != (True, 0, 0):
        bad = (bad or "") + " gkr_verify rejects the proof"
    return bad


def layer_device_transcript(k_i, k):
    # the device transcript's dense predicate tables: 2^(2k) cells each (2^28 at k = GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT)
    from oracle import cdense
    lay, z, W = synth.config5_layer(k_i, k)
    got = {}
    for mode in ("device", "host"):
        with context(["transcript=" + mode]) as ctx:
            got[mode] = ctx.sumcheck_layer_raw(lay, k, z, W)
    want = cdense.sumcheck_layer_lin_raw(k_i, k, lay.gate_type, lay.left, lay.right, z, W)
    for mode, g in got.items():
        if not all(np.array_equal(a, b) for a, b in zip(g, want)):
            return "MISMATCH: the %s transcript against the oracle" % mode
    return None


def main():
    what, args = sys.argv[1], sys.argv[2:]
    fn = {"mle": mle, "mle-batch": mle_batch, "prove-batch": prove_batch, "layer": layer, "prove-wide": prove_wide,
          "layer-device-transcript": layer_device_transcript}[what]
    args = [int(a) if a.isdigit() else a for a in args]
    t = time.time()
    bad = fn(*args)
    print("%s %s: %.1f s" % (what, " ".join(map(str, args)), time.time() - t))
    print(bad if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

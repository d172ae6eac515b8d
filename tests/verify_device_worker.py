"""Child process of tests/test_gpu_verify_device.py: the device verifier on the k = [18, 20, 20] circuit of synth.wide_circuit()
(gate arrays, eq tables and coefficient tables of tens of MiB each, none of it in the pytest process).  Every verdict is compared
with gkr_verify's on the same inputs.  Prints OK, or what did not match."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gkr_amd import Context, GKRCircuit, GkrError, Layer, synth  # noqa: E402
from gkr_amd import _native as N  # noqa: E402
from gkr_amd.dropin import verify_native  # noqa: E402
from gkr_amd.field import MODULUS  # noqa: E402


def main():
    circuit, raw, wit = synth.wide_circuit()
    ks = circuit.get_k_list()
    assert ks == [18, 20, 20], ks
    bad = []
    with Context(0) as ctx:
        arrs = [a.copy() for a in ctx.prove_batch_raw(circuit, np.ascontiguousarray(wit), all_arrays=True)]
        with ctx.prepare_verify(circuit) as handle:
            t0 = time.perf_counter()
            got = ctx.verify_batch(handle, arrs)
            print("device verify %.1f ms" % ((time.perf_counter() - t0) * 1e3))
            want = [verify_native(circuit, arrs, index=0)]
            print("accepts", got, want)
            if got != want or got != [(True, 0, 0)]:
                bad.append(("accept", got, want))
            # the last input coefficient: check 9 at layer 2
            flipped = [a.copy() for a in arrs]
            flipped[8][0, -1, 0] ^= np.uint64(1)
            got, want = ctx.verify_batch(handle, flipped), [verify_native(circuit, flipped, index=0)]
            print("input coefficient", got, want)
            if got != want or got != [(False, 2, 9)]:
                bad.append(("input coefficient", got, want))
            # the last input coefficient set to the modulus r: check 2 at layer 2, from the last thread of the canonical
            # scan's stride loop (2^20 coefficients over 2048 blocks)
            flipped = [a.copy() for a in arrs]
            flipped[8][0, -1] = [(MODULUS >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
            got, want = ctx.verify_batch(handle, flipped), [verify_native(circuit, flipped, index=0)]
            print("input coefficient = r", got, want)
            if got != want or got != [(False, 2, 2)]:
                bad.append(("input coefficient = r", got, want))
        # the last gate of the last layer with the other type: a second handle
        gt = raw[-1][0].copy()
        gt[-1] ^= 1
        wrong = GKRCircuit([Layer(ks[i], *raw[i]) for i in range(len(raw) - 1)] + [Layer(ks[-2], gt, raw[-1][1], raw[-1][2])], ks[-1])
        with ctx.prepare_verify(wrong) as handle:
            got, want = ctx.verify_batch(handle, arrs), [verify_native(wrong, arrs, index=0)]
            print("gate type", got, want)
            if got != want or got[0][0]:
                bad.append(("gate type", got, want))
        # a right operand of 2^20 at the last gate of layer 1: refused at prepare (the pack kernel's stride loop)
        right = raw[1][2].copy()
        right[-1] = 1 << ks[2]
        broken = GKRCircuit([Layer(ks[0], *raw[0]), Layer(ks[1], raw[1][0], raw[1][1], right)], ks[-1])
        try:
            ctx.prepare_verify(broken).close()
            status = 0
        except GkrError as e:
            status = e.status
        print("operand out of range", status)
        if status != N.GKR_ERR_INVALID:
            bad.append(("operand out of range", status, N.GKR_ERR_INVALID))
    print("MISMATCH %r" % bad if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

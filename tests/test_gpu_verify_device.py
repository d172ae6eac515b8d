"""The device verifier (gkr_verify_prepare / gkr_verify_prepared / gkr_verify_device; csrc/capi_verify.hip, kernels_verify.hip)
against the host verifier gkr_verify on the same inputs: every case asserts EQUALITY of the triple (accept, failed_layer,
failed_check) with dropin.verify_native, not just acceptance or rejection."""

import os
import subprocess
import sys

import numpy as np
import pytest

from gkr_amd import Context, GKRCircuit, GkrError, Layer, synth
from gkr_amd import _native as N
from gkr_amd.dropin import verify_device, verify_native
from gkr_amd.field import MODULUS
from helpers import ints, layers_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KS = [12, 14, 15, 13]
# the modulus r itself as limbs: the smallest non-canonical element (field.to_limbs reduces, so it cannot make one)
R_LIMBS = np.array([(MODULUS >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide(ctx):
    """synth.wide_circuit([12, 14, 15, 13], seed=4242), three proofs of it (raw arrays) and a handle."""
    circuit, layers, _ = synth.wide_circuit(KS, seed=4242)
    rng = np.random.default_rng(8)
    wit = np.ascontiguousarray(synth.rand_fr(rng, 3 << KS[-1]).reshape(3, 1 << KS[-1], 4))
    arrs = [a.copy() for a in ctx.prove_batch_raw(circuit, wit, all_arrays=True)]
    handle = ctx.prepare_verify(circuit)
    yield circuit, layers, arrs, handle
    handle.close()


def _host(circuit, arrs):
    return [verify_native(circuit, arrs, index=b, threads=0) for b in range(arrs[0].shape[0])]


def _circuit(layers, n_inputs):
    ks = [max(0, (len(l[0]) - 1).bit_length()) for l in layers] + [max(0, (n_inputs - 1).bit_length())]
    return GKRCircuit([Layer(ks[i], *layers[i]) for i in range(len(layers))], ks[-1])


def test_golden_circuits_are_accepted_and_a_handle_is_reused(ctx, gkr_cases):
    """Every circuit of tests/golden/gkr_circuits.json (k[0] = 0 among them), proven by ctx.prove: accepted, as the host
    verifier accepts it; a second call on the same handle -- with the proof twice in a batch -- gives the same."""
    for case in gkr_cases:
        circuit = _circuit(layers_of(case), len(case["inputs"]))
        proof = ctx.prove(circuit, ints(case["inputs"]))
        want = verify_native(circuit, proof)
        with ctx.prepare_verify(circuit) as handle:
            first = ctx.verify_batch(handle, proof)
            again = ctx.verify_batch(handle, [proof, proof])
        assert want == (True, 0, 0), (case["name"], want)
        assert first == [want], (case["name"], first)
        assert again == [want, want], (case["name"], again)


def test_tamper_matrix_in_a_batch_of_three(ctx, wide):
    """The tamper matrix of test_library_verifier_on_gpu_proofs_through_wide_layers applied to proof 1 only, the whole batch
    verified in one call: proof 1 carries the host's (layer, check), proofs 0 and 2 are accepted."""
    circuit, layers, arrs, handle = wide
    assert ctx.verify_batch(handle, arrs) == _host(circuit, arrs) == [(True, 0, 0)] * 3
    rows1 = 2 * KS[1]
    for name, arr, index, check, layer in (("round coefficient", 0, (1, rows1 + 5, 2, 0), 4, 1), ("challenge", 2, (1, 3, 0), 5, 0),
                                           ("q", 3, (1, KS[1] + 1 + 4, 0), 6, 1), ("r*", 6, (1, 2, 0), 7, 2), ("z", 5, (1, KS[0] + 1, 0), 8, 0),
                                           ("input_func", 8, (1, 77, 0), 9, 3)):
        bad = [a.copy() for a in arrs]
        bad[arr][index] ^= np.uint64(1)
        got, want = ctx.verify_batch(handle, bad), _host(circuit, bad)
        assert got == want, (name, got, want)
        assert got == [(True, 0, 0), (False, layer, check), (True, 0, 0)], (name, got)
    bad = [a.copy() for a in arrs]
    bad[5][1, 0, 0] = 1                                       # z[0][0] = 1
    got = ctx.verify_batch(handle, bad)
    assert got == _host(circuit, bad) and got[1] == (False, 0, 3), got
    # a flipped gate type: a second handle
    flipped = [(gt.copy(), l, r) for gt, l, r in layers]
    flipped[2][0][123] ^= 1
    wrong = GKRCircuit([Layer(KS[i], *flipped[i]) for i in range(3)], KS[-1])
    with ctx.prepare_verify(wrong) as other:
        got = ctx.verify_batch(other, arrs)
    assert got == _host(wrong, arrs), got
    assert not any(ok for ok, _, _ in got), got


def test_non_canonical_elements(ctx, wide):
    """One element of each of the proof's arrays set to the modulus r (proof 1 of the batch).  An element the verifier scans --
    round coefficients, challenges, q, the two coefficient tables -- is check 2 at the layer the host names.  The other arrays
    have no canonical scan of their own in gkr_verify, and the device verifier gives the host's verdict for them too: r* = r is
    not the hash (check 7), z[i+1][j] = r is not l(r*) (check 8), and a length whose low word is r's is out of range (check 1).
    The device computed eq tables and sums from these elements before any check ran: none of that garbage decides anything."""
    circuit, layers, arrs, handle = wide
    mod = R_LIMBS
    assert sum(int(x) << (64 * i) for i, x in enumerate(mod)) == MODULUS
    rows1 = 2 * KS[1]
    cases = (("round coefficient", 0, (1, rows1 + 7, 2), 2), ("round length", 1, (1, rows1 + 2), 1), ("challenge", 2, (1, 3), 2),
             ("challenge of the c-phase", 2, (1, rows1 + KS[2] + 1), 2), ("q", 3, (1, KS[1]), 2), ("q length", 4, (1, 1), 1),
             ("z", 5, (1, KS[0] + KS[1] + 2), 8), ("r*", 6, (1, 1), 7), ("D", 7, (1, 5), 2), ("input_func", 8, (1, 77), 2))
    for name, arr, index, check in cases:
        bad = [a.copy() for a in arrs]
        bad[arr][index] = mod if bad[arr].dtype == np.uint64 else np.uint32(mod[0] & np.uint64(0xFFFFFFFF))
        got, want = ctx.verify_batch(handle, bad), _host(circuit, bad)
        assert got == want, (name, got, want)
        assert got[0] == got[2] == (True, 0, 0) and not got[1][0] and got[1][2] == check, (name, got)


def test_verdicts_do_not_depend_on_the_chunking(ctx, wide):
    """verify_workspace_mb = 1: a proof of this circuit takes more than that, so every chunk is one proof."""
    circuit, layers, arrs, handle = wide
    bad = [a.copy() for a in arrs]
    bad[3][2, KS[1] + 1 + 4, 0] ^= np.uint64(1)               # q of layer 1, proof 2
    bad[7][0, 9] = R_LIMBS                                    # D, proof 0
    whole = ctx.verify_batch(handle, bad)
    ctx.set_option("verify_workspace_mb", 1)
    try:
        chunked = ctx.verify_batch(handle, bad)
    finally:
        ctx.set_option("verify_workspace_mb", 0)
    assert whole == chunked == _host(circuit, bad)
    assert whole == [(False, 0, 2), (True, 0, 0), (False, 1, 6)], whole


def test_an_operand_out_of_range_is_refused_at_prepare_time(ctx, wide):
    circuit, layers, arrs, handle = wide
    broken = [(gt.copy(), l.copy(), r) for gt, l, r in layers]
    broken[2][1][-7] = 1 << KS[3]                             # left = 2^k in the last layer
    with pytest.raises(GkrError) as e:
        ctx.prepare_verify(GKRCircuit([Layer(KS[i], *broken[i]) for i in range(3)], KS[-1]))
    assert e.value.status == N.GKR_ERR_INVALID
    broken[2][1][-7] = 0
    broken[2][0][5] = 2                                       # a gate type that is neither add nor mult
    with pytest.raises(GkrError) as e:
        ctx.prepare_verify(GKRCircuit([Layer(KS[i], *broken[i]) for i in range(3)], KS[-1]))
    assert e.value.status == N.GKR_ERR_INVALID
    assert ctx.verify_batch(handle, arrs) == [(True, 0, 0)] * 3        # the context is still usable


def test_large_circuit_in_a_worker():
    """tests/verify_device_worker.py: k = [18, 20, 20] accepted; the last input coefficient flipped is check 9 at layer 2; the
    last gate of the last layer flipped is rejected -- each equal to gkr_verify's verdict; the last input coefficient set to r is
    check 2; a right operand of 2^20 at the last gate of layer 1 is refused at prepare time."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "verify_device_worker.py")], env=dict(os.environ), capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_one_shot_calls_agree_with_the_handle(ctx, wide, gkr_cases):
    circuit, layers, arrs, handle = wide
    bad = [a.copy() for a in arrs]
    bad[2][1, 3, 0] ^= np.uint64(1)
    want = ctx.verify_batch(handle, bad)
    assert want == _host(circuit, bad)
    assert ctx.verify_batch(circuit, bad) == want             # gkr_verify_device
    assert verify_device(ctx, circuit, bad) == want
    assert verify_device(ctx, handle, bad, index=1) == want[1] == (False, 0, 5)
    case = gkr_cases[0]
    small = _circuit(layers_of(case), len(case["inputs"]))
    proof = ctx.prove(small, ints(case["inputs"]))
    assert verify_device(ctx, small, proof) == verify_native(small, proof) == (True, 0, 0)

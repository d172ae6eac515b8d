"""Exhaustive single-element tamper sweeps of the host verifiers, held to a closed-form model (tests/verify_sweeps.py).

Over all circuits of tests/golden/gkr_circuits.json, with the oracle's proofs: every field element of every array of the proof
is replaced, one at a time, by x + 1 mod r and by the modulus r, and every length by every value around its range.  gkr_verify
(csrc/dropin.cpp over csrc/verify_core.h) must give the model's verdict for each, and on x + 1 the verdict of the plain-integer
verifier (gkr_amd/verifier.py) as well.  A relation that skipped the last element of a table, the first slot of a round vector or
a layer's last challenge would accept a proof here that the model rejects.  No element is left out: the sweeps are counted against
the arrays' sizes."""

import pytest

from gkr_amd import Proof, verify
from gkr_amd.dropin import _arrays_of_proof, verify_native
from gkr_amd.prover import _decode_proofs
from helpers import ints, layers_of
from oracle import dense
from verify_sweeps import (ACCEPTED, COEFFS, FIELD_ARRAYS, LENS, NAMES, Q, Q_LEN, circuit_of, element_sweep, elements, length_cases,
                           length_sweep, q_grown_over_zeros)


@pytest.fixture(scope="module")
def proven(gkr_cases):
    """[(name, circuit, k list, the nine arrays of the oracle's proof, its elements)], computed once and never written to."""
    out = []
    for case in gkr_cases:
        layers, inputs = layers_of(case), ints(case["inputs"])
        ref = dense.prove(layers, inputs)
        circuit = circuit_of(layers, len(inputs))
        assert ref["k"] == circuit.get_k_list()
        proof = Proof(sumcheck_proofs=ref["sumcheck_proofs"], sumcheck_r=ref["sumcheck_r"], d=ref["d"], q=ref["q"], z=ref["z"], r=ref["r"],
                      depth=ref["depth"], input_func=ref["input_func"], k=ref["k"])
        arrs = _arrays_of_proof(proof)
        for a in arrs:
            a.setflags(write=False)
        assert verify_native(circuit, arrs) == ACCEPTED and verify(proof, circuit), case["name"]
        out.append((case["name"], circuit, ref["k"], arrs, elements(ref["k"], arrs)))
    assert len(out) == 25
    return out


def _host(circuit, bad):
    return [verify_native(circuit, bad, index=b) for b in range(bad[0].shape[0])]


def test_no_element_is_left_out(proven):
    """The element list has one entry per field element of the seven field arrays, each index once."""
    for name, circuit, ks, arrs, elems in proven:
        for a in FIELD_ARRAYS:
            mine = [e.index for e in elems if e.arr == a]
            n = sum(ks) if NAMES[a] == "z" else arrs[a][0].size // 4
            assert len(mine) == len(set(mine)) == n, (name, NAMES[a], len(mine), n)


def test_the_fixtures_reach_the_accept_branch_of_the_model(proven):
    """At least one unread round-vector slot and one unread q slot among the fixtures' proofs."""
    unread = [e for _, _, _, _, elems in proven for e in elems if not e.read]
    assert sum(e.arr == COEFFS for e in unread) >= 1
    assert sum(e.arr == Q for e in unread) >= 1


def test_plus_one_sweep(proven):
    """x + 1 mod r in every element: gkr_verify and verifier.verify agree, and accept exactly the elements no relation reads."""
    total = accepted = 0
    for name, circuit, ks, arrs, elems in proven:
        bad = element_sweep(arrs, elems, "plus1")
        native = _host(circuit, bad)
        plain = [verify(p, circuit) for p in _decode_proofs(bad, ks)]
        for el, got, py in zip(elems, native, plain):
            where = (name, NAMES[el.arr], el.index)
            assert got[0] == py, (where, got, py)
            assert got[0] == (not el.read), (where, got)
            assert got[0] or got[1] == el.layer, (where, got)
        total += len(elems)
        accepted += sum(g[0] for g in native)
    print("plus-one sweep: %d proofs, %d accepted" % (total, accepted))


def test_modulus_sweep(proven):
    """The modulus r in every element: the model's (accept, layer, check), exactly."""
    total = accepted = 0
    for name, circuit, ks, arrs, elems in proven:
        native = _host(circuit, element_sweep(arrs, elems, "mod"))
        for el, got in zip(elems, native):
            assert got == el.mod_verdict, (name, NAMES[el.arr], el.index, got, el.mod_verdict)
        total += len(elems)
        accepted += sum(g[0] for g in native)
    print("modulus sweep: %d proofs, %d accepted" % (total, accepted))


def test_length_sweep(proven):
    """Every sumcheck_len as 0..5 and every q_len as 0..7.  The verdicts are recorded for the device verifier to be compared
    with (test_gpu_verify_sweep.py).  Two things about them are closed-form: a length outside its range is check 1 at its own
    layer, and a q_len grown over zero leading slots names the same polynomial, so the proof stays accepted."""
    total, accepted = 0, []
    for name, circuit, ks, arrs, elems in proven:
        cases = length_cases(ks, arrs)
        native = _host(circuit, length_sweep(arrs, cases))
        layer_of_row = [i for i in range(len(ks) - 1) for _ in range(2 * ks[i + 1])]
        for case, got in zip(cases, native):
            arr, (at,), v = case
            layer = layer_of_row[at] if arr == LENS else at
            top = 3 if arr == LENS else ks[layer + 1] + 1
            if not 1 <= v <= top:
                assert got == (False, layer, 1), (name, case, got)
            if q_grown_over_zeros(ks, arrs, case):
                assert got == ACCEPTED, (name, case, got)
            assert got == ACCEPTED or (not got[0] and got[1] == layer and 1 <= got[2] <= 9), (name, case, got)
            if got[0]:
                accepted.append((name, NAMES[arr], at, v))
        total += len(cases)
    print("length sweep: %d proofs, accepted: %r" % (total, accepted))

"""The device verifier (gkr_verify_prepare / gkr_verify_prepared; csrc/capi_verify.hip, kernels_verify.hip, kernels_verify_hash.hip)
held to the host verifier gkr_verify, triple for triple (accept, failed_layer, failed_check), where a sum kernel being right
does not show it:

  A. the exhaustive single-element sweeps of tests/verify_sweeps.py (x + 1, the modulus r, every length) over every golden
     circuit, one batch per sweep, with the hashes on the device and on the host -- and against the closed-form model;
  B. a shape matrix at the launch boundaries of the kernels, the critical layer at index >= 1 (z[0] = 0 hides every gate of
     layer 0 but gate 0), with tampers at the first and last element of a block and of a table;
  C. the kernels that only detect -- k_verify_canonical, the range check of k_verify_pack, the validity of k_verify_hash -- over
     a matrix of values and positions;
  D. ragged chunks, workspaces reused between handles, and a batch beyond the 32768 proofs one chunk may hold.

The device verifier's own output is never the reference."""

import numpy as np
import pytest

from gkr_amd import Context, GKRCircuit, GkrError, Layer, synth, verify
from gkr_amd import _native as N
from gkr_amd.dropin import _arrays_of_proof, verify_native
from gkr_amd.field import MODULUS
from gkr_amd.prover import _decode_proofs
from helpers import ints, layers_of
from verify_sweeps import (ACCEPTED, CHALLENGES, COEFFS, D, INPUT, LENS, NAMES, Q, R_LIMBS, circuit_of, element_sweep, elements, length_cases,
                           length_sweep, limbs, positions, replicate, value)

pytestmark = pytest.mark.gpu
NON_CANONICAL = [MODULUS, MODULUS + 1, 1 << 254, (1 << 256) - 1]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _host(circuit, arrs):
    return [verify_native(circuit, arrs, index=b, threads=0) for b in range(arrs[0].shape[0])]


def _both(ctx, handle, arrs):
    """-> (verdicts with the hashes on the device, verdicts with the hashes on the host)"""
    try:
        ctx.set_option("verify_device_hash_min", 1)
        dev = ctx.verify_batch(handle, arrs)
        ctx.set_option("verify_device_hash_min", -1)
        host = ctx.verify_batch(handle, arrs)
    finally:
        ctx.set_option("verify_device_hash_min", 0)
    return dev, host


def _first_difference(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def _random_proofs(ctx, ks, seed, batch):
    """synth.wide_circuit(ks, seed) -- random gates --, `batch` random witnesses, their proofs as raw arrays."""
    circuit, raw, _ = synth.wide_circuit(ks, seed=seed)
    rng = np.random.default_rng(seed + 1)
    wit = np.ascontiguousarray(synth.rand_fr(rng, batch << ks[-1]).reshape(batch, 1 << ks[-1], 4))
    assert len({w.tobytes() for w in wit}) == batch
    arrs = [a.copy() for a in ctx.prove_batch_raw(circuit, wit, all_arrays=True)]
    return circuit, raw, arrs


def _with_gate_type_flipped(ks, raw, layer, gate):
    gt = raw[layer][0].copy()
    gt[gate] ^= 1
    return GKRCircuit([Layer(ks[i], gt if i == layer else raw[i][0], raw[i][1], raw[i][2]) for i in range(len(raw))], ks[-1])


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("case_index", range(25))
def test_exhaustive_sweeps_of_a_golden_circuit(ctx, gkr_cases, case_index):
    """One handle; per sweep ONE batch holding every tampered proof of the sweep, verified with the hashes on the device and on the
    host: each triple is gkr_verify's.  On x + 1 and on r it is the model's too (accepted iff no relation reads the element; on r
    the check code), so both verifiers skipping the same element would still fail here."""
    assert len(gkr_cases) == 25
    case = gkr_cases[case_index]
    circuit = circuit_of(layers_of(case), len(case["inputs"]))
    ks = circuit.get_k_list()
    arrs = _arrays_of_proof(ctx.prove(circuit, ints(case["inputs"])))
    elems = elements(ks, arrs)
    cases = length_cases(ks, arrs)
    with ctx.prepare_verify(circuit) as handle:
        for sweep, bad in (("plus1", element_sweep(arrs, elems, "plus1")), ("mod", element_sweep(arrs, elems, "mod")),
                           ("lengths", length_sweep(arrs, cases))):
            assert 1 <= bad[0].shape[0] <= 112, (case["name"], sweep, bad[0].shape[0])
            want = _host(circuit, bad)
            dev, host = _both(ctx, handle, bad)
            assert dev == want, (case["name"], sweep, "device hashes", _first_difference(dev, want))
            assert host == want, (case["name"], sweep, "host hashes", _first_difference(host, want))
            if sweep == "plus1":
                assert [w[0] for w in want] == [not e.read for e in elems], (case["name"], sweep)
            if sweep == "mod":
                assert want == [e.mod_verdict for e in elems], (case["name"], sweep)


# ---------------------------------------------------------------------------------------------------------------- B
# wiring pass: 256 gates a block -- one block up to k_i = 8, two at 9, the 1024-block cap (a thread takes several gates) from 19;
# a layer smaller than the chunk's largest leaves blocks idle ([2,11,3,10,2]); k_verify_reduce rows wider than a wave from
# k_i = 15; k_verify_mono_dot strides from k = 19; half tables of 0 variables at k <= 1, odd and even k; k_verify_pack strides
# beyond 2^19 gates.  (The canonical scan's stride loop starts at k = 20: tests/verify_device_worker.py.)
SHAPES = [[0, 1, 1], [1, 8, 3], [1, 9, 3], [2, 11, 3, 10, 2], [1, 15, 5], [1, 19, 4], [2, 3, 19]]


@pytest.mark.parametrize("ks", SHAPES, ids=lambda ks: "k" + "_".join(map(str, ks)))
def test_shapes_at_the_launch_boundaries(ctx, ks):
    L = len(ks) - 1
    batch = 2 if max(ks) >= 19 else 3
    circuit, raw, arrs = _random_proofs(ctx, ks, seed=7000 + sum(ks), batch=batch)
    n_in, n_d = 1 << ks[-1], 1 << ks[0]
    with ctx.prepare_verify(circuit) as handle:
        # correct proofs
        assert ctx.verify_batch(handle, arrs) == [ACCEPTED] * batch
        assert _host(circuit, arrs) == [ACCEPTED] * batch
        if sum(1 << k for k in ks) <= 1 << 12:                  # (the input layer counted: the plain-integer verifier walks its table)
            assert all(verify(p, circuit) for p in _decode_proofs(arrs, ks))
        # one batch of tampered copies of proof 0: input_coeffs + 1 and = r at the block and table boundaries, d_coeffs[last] = r
        at = positions(n_in)
        bad = replicate(arrs, 2 * len(at) + 1)
        want = []
        for e, p in enumerate(at):
            bad[INPUT][e, p] = limbs((value(bad[INPUT][e, p]) + 1) % MODULUS)
            bad[INPUT][len(at) + e, p] = R_LIMBS
        bad[D][2 * len(at), n_d - 1] = R_LIMBS
        want = [(False, L, 9)] * len(at) + [(False, L, 2)] * len(at) + [(False, 0, 2)]
        got = ctx.verify_batch(handle, bad)
        assert _host(circuit, bad) == want
        assert got == want, _first_difference(got, want)
    # a gate of the other type in a layer >= 1: eq(z_i, g) is non-zero for every g there, so every flip is a rejection
    for layer in range(1, L):
        for gate in positions(1 << ks[layer]):
            wrong = _with_gate_type_flipped(ks, raw, layer, gate)
            with ctx.prepare_verify(wrong) as other:
                got = ctx.verify_batch(other, arrs)
            want = _host(wrong, arrs)
            assert got == want, (layer, gate, got, want)
            assert not any(w[0] for w in want), (layer, gate, want)
    # ... and in layer 0 at a gate other than 0: eq(0, g) = 0, nobody can tell
    for gate in positions(1 << ks[0], (1, 3, -1)):
        if gate == 0:
            continue
        wrong = _with_gate_type_flipped(ks, raw, 0, gate)
        with ctx.prepare_verify(wrong) as other:
            got = ctx.verify_batch(other, arrs)
        assert got == _host(wrong, arrs) == [ACCEPTED] * batch, (gate, got)


# ---------------------------------------------------------------------------------------------------------------- C
KS_TABLES = [11, 3, 11]                                       # both coefficient tables have 2^11 entries
TABLE_POSITIONS = [0, 63, 64, 255, 256, (1 << 11) - 1]


@pytest.fixture(scope="module")
def tables(ctx):
    circuit, raw, arrs = _random_proofs(ctx, KS_TABLES, seed=5151, batch=3)
    handle = ctx.prepare_verify(circuit)
    assert ctx.verify_batch(handle, arrs) == _host(circuit, arrs) == [ACCEPTED] * 3
    yield circuit, arrs, handle
    handle.close()


@pytest.mark.parametrize("which", [D, INPUT], ids=["d_coeffs", "input_coeffs"])
def test_non_canonical_coefficients_at_block_and_wave_boundaries(ctx, tables, which):
    """r, r + 1, 2^254 and 2^256 - 1 at index 0, 63, 64, 255, 256 and last of a 2^11 table, in proof 1 of three: check 2 at the
    table's layer from k_verify_canonical's flag, the neighbours accepted."""
    circuit, arrs, handle = tables
    cases = [(v, p) for v in NON_CANONICAL for p in TABLE_POSITIONS]
    bad = [np.ascontiguousarray(np.concatenate([a] * len(cases), axis=0)) for a in arrs]
    for c, (v, p) in enumerate(cases):
        bad[which][3 * c + 1, p] = limbs(v)
    layer = 0 if which == D else len(KS_TABLES) - 1
    want = [ACCEPTED, (False, layer, 2), ACCEPTED] * len(cases)
    assert _host(circuit, bad) == want
    dev, host = _both(ctx, handle, bad)
    assert dev == want, _first_difference(dev, want)
    assert host == want, _first_difference(host, want)


def test_non_canonical_round_coefficients(ctx, tables):
    """The same values in used slots of round vectors: multi_hash_batch (k_verify_hash's own entry point) marks exactly those
    rows invalid, with a zero hash, and gives every other row the challenge the proof carries -- which gkr_verify has checked to
    be the row's hash; the verifier gives the host's check 2 at the row's layer."""
    circuit, arrs, handle = tables
    rounds = arrs[LENS].shape[1]
    rows0 = 2 * KS_TABLES[1]
    spots = []
    for row in (0, rows0 // 2, rows0 - 1, rows0, rounds - 1):
        ln = int(arrs[LENS][1, row])
        spots += [(row, 2), (row, 3 - ln)]                   # the constant term and the leading used slot
    cases = [(v, spot) for v in NON_CANONICAL for spot in sorted(set(spots))]
    bad = [np.ascontiguousarray(np.concatenate([a] * len(cases), axis=0)) for a in arrs]
    for c, (v, (row, t)) in enumerate(cases):
        bad[COEFFS][3 * c + 1, row, t] = limbs(v)
    got, valid = ctx.multi_hash_batch(bad[COEFFS].reshape(-1, 3, 4), bad[LENS].reshape(-1))
    want_valid = np.ones(len(valid), dtype=np.uint32)
    want_hash = bad[CHALLENGES].reshape(-1, 4).copy()
    for c, (v, (row, t)) in enumerate(cases):
        want_valid[(3 * c + 1) * rounds + row] = 0
        want_hash[(3 * c + 1) * rounds + row] = 0
    assert valid.tolist() == want_valid.tolist()
    assert np.array_equal(got, want_hash)
    want = []
    for v, (row, t) in cases:
        want += [ACCEPTED, (False, 0 if row < rows0 else 1, 2), ACCEPTED]
    assert _host(circuit, bad) == want
    dev, host = _both(ctx, handle, bad)
    assert dev == want, _first_difference(dev, want)
    assert host == want, _first_difference(host, want)


KS_PACK = [9, 3, 9, 4]                                        # first and last layer: 2^9 gates, two blocks of the pack kernel


def test_prepare_refuses_every_bad_gate(ctx):
    """Operands 2^k, 2^k + 1, 2^31, 2^31 | a valid index (bit 31 is the packed record's type bit) and 0xFFFFFFFF, left and right;
    types 2, 3, 0x80 and 0xFF; at gate 0, 255, 256 and last of the first and the last layer: GKR_ERR_INVALID each, and the
    context verifies a good batch afterwards."""
    circuit, raw, arrs = _random_proofs(ctx, KS_PACK, seed=909, batch=2)
    refused = 0
    for layer in (0, len(KS_PACK) - 2):
        k = KS_PACK[layer + 1]
        for gate in positions(1 << KS_PACK[layer]):
            edits = [(side, op) for side in (1, 2) for op in (1 << k, (1 << k) + 1, 1 << 31, (1 << 31) | ((1 << k) - 1), 0xFFFFFFFF)]
            edits += [(0, t) for t in (2, 3, 0x80, 0xFF)]
            for side, v in edits:
                broken = [[a.copy() for a in lay] for lay in raw]
                broken[layer][side][gate] = v
                assert int(broken[layer][side][gate]) == v
                with pytest.raises(GkrError) as e:
                    ctx.prepare_verify(GKRCircuit([Layer(KS_PACK[i], *broken[i]) for i in range(len(raw))], KS_PACK[-1]))
                assert e.value.status == N.GKR_ERR_INVALID, (layer, gate, side, v)
                refused += 1
    assert refused == 2 * 4 * 14
    with ctx.prepare_verify(circuit) as handle:
        assert ctx.verify_batch(handle, arrs) == _host(circuit, arrs) == [ACCEPTED] * 2


# ---------------------------------------------------------------------------------------------------------------- D
KS_SMALL = [3, 5, 6, 4]


@pytest.fixture(scope="module")
def small(ctx):
    circuit, raw, arrs = _random_proofs(ctx, KS_SMALL, seed=1718, batch=3)
    handle = ctx.prepare_verify(circuit)
    yield circuit, arrs, handle
    handle.close()


def _tiled(arrs, n):
    idx = np.arange(n) % arrs[0].shape[0]
    return [np.ascontiguousarray(a[idx]) for a in arrs]


def _tamper_four(ks, big, at):
    """A challenge, the last input coefficient, a q slot and a round length, one in each of the four proofs `at`."""
    big[CHALLENGES][at[0], 1, 0] ^= np.uint64(1)
    big[INPUT][at[1], -1, 0] ^= np.uint64(1)
    big[Q][at[2], ks[1], 0] ^= np.uint64(1)                   # the constant term of layer 0's q
    big[LENS][at[3], big[LENS].shape[1] - 1] = 4
    return big


def test_ragged_chunks(ctx, small):
    """127 proofs under verify_workspace_mb = 1: n chunks, 2 <= n < 127, the last one ragged; the first and last proof and the two
    in the middle tampered.  The verdicts are the host's, and those of the one-chunk run."""
    circuit, arrs, handle = small
    big = _tamper_four(KS_SMALL, _tiled(arrs, 127), (0, 63, 64, 126))
    want = _host(circuit, big)
    assert [i for i, w in enumerate(want) if not w[0]] == [0, 63, 64, 126]
    ctx.set_option("verify_workspace_mb", 1)
    ctx.set_option("verify_device_hash_min", 1)
    ctx.profile(1)
    try:
        ctx.profile_reset()
        chunked = ctx.verify_batch(handle, big)
        n = ctx.profile_get("verify_hash")["launches"]        # one launch per chunk
    finally:
        ctx.profile(0)
        ctx.set_option("verify_workspace_mb", 0)
        ctx.set_option("verify_device_hash_min", 0)
    assert 2 <= n < 127, n
    assert chunked == want, _first_difference(chunked, want)
    whole, _ = _both(ctx, handle, big)
    assert whole == want, _first_difference(whole, want)


def test_workspaces_are_reused_between_handles(ctx, small):
    """Handle A in a large batch, handle B (another k list) in a small one, A again in a small one, on one context: every
    workspace is laid out anew for each call."""
    circuit_a, arrs_a, handle_a = small
    circuit_b, raw_b, arrs_b = _random_proofs(ctx, [5, 3, 7], seed=2718, batch=2)
    large = _tamper_four(KS_SMALL, _tiled(arrs_a, 96), (0, 31, 32, 95))
    few_a = [a.copy() for a in arrs_a]
    few_a[Q][2, KS_SMALL[1], 0] ^= np.uint64(1)
    few_b = [a.copy() for a in arrs_b]
    few_b[INPUT][1, 100, 0] ^= np.uint64(1)
    with ctx.prepare_verify(circuit_b) as handle_b:
        for hash_min in (1, -1):
            ctx.set_option("verify_device_hash_min", hash_min)
            try:
                got = [ctx.verify_batch(handle_a, large), ctx.verify_batch(handle_b, few_b), ctx.verify_batch(handle_a, few_a)]
            finally:
                ctx.set_option("verify_device_hash_min", 0)
            assert got[0] == _host(circuit_a, large), hash_min
            assert got[1] == _host(circuit_b, few_b) == [ACCEPTED, (False, 2, 9)], (hash_min, got[1])
            assert got[2] == _host(circuit_a, few_a) == [ACCEPTED, ACCEPTED, (False, 0, 6)], (hash_min, got[2])


def test_more_proofs_than_one_chunk_may_hold(ctx):
    """40000 copies of one k = [1, 1] proof: a chunk holds at most 32768 proofs (the proof is a grid dimension), so proofs 32767
    and 32768 are the last of the first chunk and the first of the second.  Five distinct proofs, the host's verdict for each."""
    ks = [1, 1]
    circuit, raw, arrs = _random_proofs(ctx, ks, seed=4040, batch=1)
    at = (0, 32767, 32768, 39999)
    big = _tamper_four(ks, replicate(arrs, 40000), at)
    distinct = [0, 32767, 32768, 39999, 1]
    five = _host(circuit, [np.ascontiguousarray(a[distinct]) for a in big])
    assert five[4] == ACCEPTED and not any(w[0] for w in five[:4]), five
    want = [ACCEPTED] * 40000
    for i, w in zip(at, five):
        want[i] = w
    with ctx.prepare_verify(circuit) as handle:
        got = ctx.verify_batch(handle, big)
    assert got == want, _first_difference(got, want)

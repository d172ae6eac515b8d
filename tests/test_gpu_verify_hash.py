"""The verifier's challenge hashes on the device (k_verify_hash, csrc/kernels_verify_hash.hip).

A. gkr_mimc7_multi_hash_device against the host's gkr_mimc7_multi_hash, row for row: the exact 32 bytes and `valid`.  Eight
   lanes hash a row and eight rows share a wave, so the cases mix lengths 1, 2 and 3 and invalid rows inside one wave.
B. gkr_verify_prepared with verify_device_hash_min = 1 (device) and -1 (host) against gkr_verify (dropin.verify_native): equality
   of the triple (accept, failed_layer, failed_check) for every proof; the context's profile row "verify_hash" shows which side
   hashed."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GKRCircuit, Layer, synth
from gkr_amd import _native as N
from gkr_amd.dropin import verify_native
from gkr_amd.field import MODULUS
from helpers import ints, layers_of

pytestmark = pytest.mark.gpu
MASK64 = (1 << 64) - 1
ALL_ONES = (1 << 256) - 1
KS = [3, 5, 6, 4]
ROUNDS = 2 * sum(KS[1:])                                      # 30 round vectors per proof
LAST_ROWS = [2 * sum(KS[1:i + 2]) - 1 for i in range(3)]      # the rows r* of each layer hashes again: 9, 21, 29
EDGE = [0, 1, MODULUS - 1, 1 << 253, (1 << 253) + (1 << 32) - 1]   # the last two: canonical, long runs for the carry lookahead


def limbs(v):
    """Any 256-bit integer as four uint64 limbs, NOT reduced (field.to_limbs reduces: it cannot make a non-canonical element)."""
    return [(v >> (64 * i)) & MASK64 for i in range(4)]


R_LIMBS = np.array(limbs(MODULUS), dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- A
_host_cache = {}


def host_hash(values):
    """gkr_mimc7_multi_hash(values, key 0) on the host, as four limbs."""
    key = tuple(values)
    if key not in _host_cache:
        arr = np.array([limbs(v) for v in values], dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        rc = N.lib().gkr_mimc7_multi_hash(arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(values)), None,
                                          out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, rc
        _host_cache[key] = out
    return _host_cache[key]


def expected(slots, lens):
    """hash_piece's rule, row for row, with the host's hash."""
    want = np.zeros((len(lens), 4), dtype=np.uint64)
    valid = np.zeros(len(lens), dtype=np.uint32)
    for i, (row, ln) in enumerate(zip(slots, lens)):
        if 1 <= ln <= 3 and all(v < MODULUS for v in row[3 - ln:]):
            want[i] = host_hash(row[3 - ln:])
            valid[i] = 1
    return want, valid


def make_rows(n, seed):
    """n rows of three canonical slots: the edge values walk through the slots (so each meets every position and length), an
    all-zero row at index 5 of every 11, seeded random elements elsewhere."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        if i % 11 == 5:
            rows.append([0, 0, 0])
        elif i % 2 == 0:
            rows.append([EDGE[(i // 2 + t) % len(EDGE)] if (i // 2 + t) % 2 == 0 else rng.randrange(MODULUS) for t in range(3)])
        else:
            rows.append([rng.randrange(MODULUS) for _ in range(3)])
    return rows


def run(ctx, slots, lens):
    rows = np.array([[limbs(v) for v in row] for row in slots], dtype=np.uint64).reshape(len(slots), 3, 4)
    return ctx.multi_hash_batch(rows, np.array([ln & 0xFFFFFFFF for ln in lens], dtype=np.uint32))


def check(ctx, slots, lens, what):
    got, got_valid = run(ctx, slots, lens)
    want, want_valid = expected(slots, lens)
    assert got_valid.tolist() == want_valid.tolist(), (what, got_valid.tolist(), want_valid.tolist())
    bad = [i for i in range(len(lens)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, (what, "rows", bad[:8], "lens", [lens[i] for i in bad[:8]])
    return got, got_valid


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 513])
def test_mixed_lengths_in_every_wave(ctx, n):
    """len = i % 3 + 1: the eight groups of every wave run 1, 2 and 3 permutations side by side; n covers a lone group, a ragged
    wave, one wave and one more row, and several blocks."""
    slots = make_rows(n, seed=100 + n)
    lens = [i % 3 + 1 for i in range(n)]
    _, valid = check(ctx, slots, lens, "n = %d" % n)
    assert valid.all()


@pytest.mark.parametrize("ln", [1, 2, 3])
def test_uniform_lengths(ctx, ln):
    _, valid = check(ctx, make_rows(9, seed=7 + ln), [ln] * 9, "uniform length %d" % ln)
    assert valid.all()


def test_edge_values_alone_in_each_slot(ctx):
    """Every edge value as the only element, as the first of two and of three, and as the last of three."""
    slots, lens = [], []
    for v in EDGE:
        slots += [[5, 6, v], [9, v, 11], [v, 12, 13], [14, 15, v], [v, v, v]]
        lens += [1, 2, 3, 3, 3]
    slots.append([0, 0, 0])
    lens.append(3)
    _, valid = check(ctx, slots, lens, "edge values")
    assert valid.all()


def test_invalid_rows_leave_their_wave_alone(ctx):
    """Five kinds of malformed row -- len 0, 4, 2^31, a used slot equal to r, a used slot equal to 2^256 - 1 --, kind t at group
    positions 0, 3 and 7 of wave t and two of them in the ragged last wave: each has valid = 0 and a zero hash, and every other
    row of those waves carries the host's hash."""
    n = 8 * 5 + 5
    slots = make_rows(n, seed=31)
    lens = [i % 3 + 1 for i in range(n)]
    invalid = set()

    def spoil(i, kind):
        invalid.add(i)
        if kind < 3:
            lens[i] = (0, 4, 1 << 31)[kind]
        else:
            used = 3 - lens[i] + (i % lens[i])                # one of the row's used slots, not always the same one
            slots[i][used] = MODULUS if kind == 3 else ALL_ONES
    for kind in range(5):
        for pos in (0, 3, 7):
            spoil(8 * kind + pos, kind)
    spoil(40, 4)                                              # the ragged wave: its group 0 ...
    spoil(43, 1)                                              # ... and its group 3; row 44, its last, is valid
    got, valid = check(ctx, slots, lens, "invalid rows")
    assert [i for i in range(n) if not valid[i]] == sorted(invalid)
    assert not got[sorted(invalid)].any()
    assert valid[44] == 1


def test_an_unused_slot_is_never_looked_at(ctx):
    """len = 1 with 2^256 - 1 in both leading slots, len = 2 with r in the leading slot: valid, and the hash of the used slots
    only -- beside rows that use all three."""
    slots = make_rows(9, seed=77)
    lens = [3] * 9
    slots[2], lens[2] = [ALL_ONES, ALL_ONES, 12345], 1
    slots[6], lens[6] = [MODULUS, 7, MODULUS - 1], 2
    got, valid = check(ctx, slots, lens, "unused slots")
    assert valid.all()
    assert got[2].tobytes() == host_hash([12345]).tobytes() and got[6].tobytes() == host_hash([7, MODULUS - 1]).tobytes()


def test_more_rows_than_one_piece_of_the_workspace(ctx):
    """2^18 + 5 rows: the call works through its device workspace in pieces of 2^18 rows, and the second piece is a ragged
    wave.  The rows repeat a block of 513 (mixed lengths), so the host hashes 513 vectors, not 2^18."""
    base, n = 513, (1 << 18) + 5
    slots = make_rows(base, seed=9)
    lens = [i % 3 + 1 for i in range(base)]
    want, _ = expected(slots, lens)
    rows = np.array([[limbs(v) for v in row] for row in slots], dtype=np.uint64)
    idx = np.arange(n) % base
    got, valid = ctx.multi_hash_batch(rows[idx], np.array(lens, dtype=np.uint32)[idx])
    assert valid.all()
    assert np.array_equal(got, want[idx])


# ---------------------------------------------------------------------------------------------------------------- B
def _circuit(layers, n_inputs):
    ks = [max(0, (len(l[0]) - 1).bit_length()) for l in layers] + [max(0, (n_inputs - 1).bit_length())]
    return GKRCircuit([Layer(ks[i], *layers[i]) for i in range(len(layers))], ks[-1])


def _host(circuit, arrs):
    return [verify_native(circuit, arrs, index=b, threads=0) for b in range(arrs[0].shape[0])]


def _both(ctx, handle, proofs):
    """-> (verdicts with the hashes on the device, verdicts with the hashes on the host)"""
    try:
        ctx.set_option("verify_device_hash_min", 1)
        dev = ctx.verify_batch(handle, proofs)
        ctx.set_option("verify_device_hash_min", -1)
        host = ctx.verify_batch(handle, proofs)
    finally:
        ctx.set_option("verify_device_hash_min", 0)
    return dev, host


@pytest.fixture(scope="module")
def small(ctx):
    """synth.wide_circuit([3, 5, 6, 4]), three proofs of it (raw arrays) and a handle: 30 round vectors per proof, 90 per chunk --
    proofs straddle groups and waves."""
    circuit, layers, _ = synth.wide_circuit(KS, seed=1717)
    rng = np.random.default_rng(5)
    wit = np.ascontiguousarray(synth.rand_fr(rng, 3 << KS[-1]).reshape(3, 1 << KS[-1], 4))
    arrs = [a.copy() for a in ctx.prove_batch_raw(circuit, wit, all_arrays=True)]
    assert arrs[0].shape == (3, ROUNDS, 3, 4)
    handle = ctx.prepare_verify(circuit)
    yield circuit, arrs, handle
    handle.close()


def test_golden_circuits_on_both_sides(ctx, gkr_cases):
    """Every circuit of tests/golden/gkr_circuits.json (k[0] = 0 and one-row layers among them), as [proof] and [proof, proof]."""
    for case in gkr_cases:
        circuit = _circuit(layers_of(case), len(case["inputs"]))
        proof = ctx.prove(circuit, ints(case["inputs"]))
        want = verify_native(circuit, proof)
        with ctx.prepare_verify(circuit) as handle:
            for batch in ([proof], [proof, proof]):
                dev, host = _both(ctx, handle, batch)
                assert dev == host == [want] * len(batch), (case["name"], dev, host, want)


def _tampered(arrs):
    """(name, arrays) with proof 1 tampered, one case at a time."""
    def case(name, arr, index, value=None):
        bad = [a.copy() for a in arrs]
        if value is None:
            bad[arr][index] ^= bad[arr].dtype.type(1)
        else:
            bad[arr][index] = value
        return name, bad
    yield case("a round coefficient in a middle row", 0, (1, 14, 2, 0))
    yield case("a coefficient of a layer's last row", 0, (1, LAST_ROWS[1], 2, 0))
    yield case("a challenge", 2, (1, 3, 0))
    yield case("r*", 6, (1, 1, 0))
    yield case("a length set to 0", 1, (1, 12), 0)
    yield case("a length set to 4", 1, (1, 12), 4)
    yield case("a used coefficient set to r", 0, (1, 12, 2), R_LIMBS)
    two_long = np.flatnonzero(arrs[1][1] == 2)
    if len(two_long):
        yield case("an unused leading slot of a 2-long row set to r", 0, (1, int(two_long[0]), 0), R_LIMBS)


def test_tamper_matrix_on_both_sides(ctx, small):
    circuit, arrs, handle = small
    dev, host = _both(ctx, handle, arrs)
    assert dev == host == _host(circuit, arrs) == [(True, 0, 0)] * 3
    names = []
    for name, bad in _tampered(arrs):
        names.append(name)
        dev, host = _both(ctx, handle, bad)
        want = _host(circuit, bad)
        assert dev == want, (name, dev, want)
        assert host == want, (name, host, want)
        assert dev[0] == dev[2] == (True, 0, 0), (name, dev)
    assert len(names) >= 7


def test_more_than_one_chunk(ctx, small):
    """Forty copies of the batch (120 proofs, 3600 round vectors) under verify_workspace_mb = 1, which holds fewer than 120 proofs
    of this circuit: the chunks' boundaries fall inside waves of the hash launch.  One proof tampered in each part."""
    circuit, arrs, handle = small
    big = [np.ascontiguousarray(np.concatenate([a] * 40, axis=0)) for a in arrs]
    big[2][1, 3, 0] ^= np.uint64(1)                           # a challenge of proof 1
    big[1][118, 12] = 4                                       # a length of proof 118
    big[0][119, LAST_ROWS[2], 2, 0] ^= np.uint64(1)           # the row r* hashes, proof 119
    want = _host(circuit, big)
    assert [i for i, w in enumerate(want) if not w[0]] == [1, 118, 119]
    ctx.set_option("verify_workspace_mb", 1)
    ctx.profile(1)
    try:
        ctx.profile_reset()
        dev, host = _both(ctx, handle, big)
        launches = ctx.profile_get("verify_hash")["launches"]
    finally:
        ctx.profile(0)
        ctx.set_option("verify_workspace_mb", 0)
    assert dev == want and host == want
    assert launches >= 2, launches                            # one launch per chunk: the batch did take more than one
    whole, _ = _both(ctx, handle, big)                        # and in one chunk
    assert whole == want


def test_the_profile_shows_which_side_hashed(ctx, small):
    circuit, arrs, handle = small
    ctx.profile(1)
    try:
        ctx.profile_reset()
        ctx.set_option("verify_device_hash_min", 1)
        assert ctx.verify_batch(handle, arrs) == [(True, 0, 0)] * 3
        row = ctx.profile_get("verify_hash")
        assert row["launches"] >= 1 and row["bytes"] == 3 * ROUNDS * (96 + 4 + 36), row
        ctx.profile_reset()
        ctx.set_option("verify_device_hash_min", -1)
        assert ctx.verify_batch(handle, arrs) == [(True, 0, 0)] * 3
        assert ctx.profile_get("verify_hash")["launches"] == 0
    finally:
        ctx.profile(0)
        ctx.set_option("verify_device_hash_min", 0)


def test_the_threshold_counts_the_round_vectors_of_a_chunk(ctx, small):
    """verify_device_hash_min = n: a chunk of n round vectors and more hashes on the device, a smaller one on the host.  Three
    proofs are 90 vectors: 90 is the device, 91 the host."""
    circuit, arrs, handle = small
    ctx.profile(1)
    try:
        for setting, launches in ((90, 1), (91, 0), (3 * ROUNDS + 1000, 0)):
            ctx.profile_reset()
            ctx.set_option("verify_device_hash_min", setting)
            assert ctx.verify_batch(handle, arrs) == [(True, 0, 0)] * 3
            assert ctx.profile_get("verify_hash")["launches"] == launches, setting
    finally:
        ctx.profile(0)
        ctx.set_option("verify_device_hash_min", 0)

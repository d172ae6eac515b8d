"""gkr_fraction_sum_batch_device and its verifier (csrc/capi_fraction_sum.hip, csrc/kernels_fraction_sum.hip, csrc/tree_argument.h) bit
for bit against the C oracle's ogkr_fraction_sum (cdense.fraction_sum_raw; tests/test_oracle_fraction_sum_c.py holds it to the
integer model and to both integer verifiers) at the sizes tests/test_gpu_fraction_sum.py compares with nothing independent.  The
oracle runs the tree as a loop of products and sums and every layer as the EXPLICIT zero-check; it shares no code with the library,
so the layer kernel with its per-proof lambda at the layer geometries k = 13 .. 17, and the driver's own work there -- the level
offsets handed on as table bases, the row scatter into the proof's arrays, the tau and lambda chain -- are held to something
independent.

  a. the shape matrix (n, batch) = (16, 1), (17, 1), (17, 20), (18, 5): the launch geometry of the tree and of the top three layers
     asserted first; seven kinds of pair in turn; all eight output arrays; inputs unchanged; the device verifier's verdicts;
  b. every level of the tree at (17, 20), canaries on either side;
  c. tampered proofs with layers up to k = 15 in one batch at n = 16, verdicts from the closed form alone, under both hash sides,
     both evaluation kernels and one / several chunks of the verifier;
  d. the n = 5 sweep tiled over at least three chunks with a ragged last one, with and without claimed sums;
  e. the batch limit 65535 at n = 3 (chunks of 32768 and 32767);  f. the whole call with a pair 4 GiB into the tables.

Every chunking case asserts its chunk size through gkr_devtest_fraction_sum_chunk first.  The library's own output is never the
reference of a verdict or a value.  Each case prints the seconds the oracle and the device calls took (pytest -s shows them)."""

import random
import time

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, FRACTION_SUM, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR, fraction_sum,
                                head_root, make_tables, proof_arrays, rounds)
from fraction_sum_oracle import PAIR_KINDS, as_model, limb_pair, pick, zero_index
from fraction_sum_sweeps import ACCEPTED, _eq_weight, apply, check_cofactors, check_inputs, table_entries, tamperings
from oracle import cdense
from oracle.field import P
from product_shapes import product_geometry
from resident_tables import Resident, free_bytes
from test_fraction_sum_host import tree_geometry
from test_gpu_fraction_sum import CANARY, _assert_same, _batch_of, _level_offset, _model, _pair, _ptr_at, _raw

pytestmark = pytest.mark.gpu

# (n, batch, the kind of pair 0 -- pair b takes the b-th kind after it in PAIR_KINDS).  The batch-1 cases take pairs of distinct
# entries (random, padded): on a constant pair an operand read one entry off gives the same bytes.
MATRIX = [(16, 1, 0), (17, 1, 5), (17, 20, 0), (18, 5, 1)]
# (k, batch) -> (blocks per sumcheck, chunk) of round 0 of layer k's zero-check, which runs on tables of 2^k entries: what
# mle_blocks_per_table gives for items = 2^(k-1) pairs with the default items_per_block,
#   blocks = min(max(ceil(items / 1024), ceil(2048 / batch)), ceil(items / 256), 2048),   chunk = ceil(items / blocks) rounded up to 256.
# A retuned geometry has to fail the pin, not leave these cases running something else.
LAYER_GEOMETRY = {
    (13, 1): (16, 256), (14, 1): (32, 256),      # half a trip of the round kernel's 64-lane loop over the partials
    (15, 1): (64, 256),                          # exactly one trip
    (16, 1): (128, 256),                         # two trips
    (14, 20): (32, 256), (15, 20): (64, 256),
    (16, 20): (103, 512),                        # no power of two, 39 empty blocks
    (15, 5): (64, 256), (16, 5): (128, 256), (17, 5): (256, 256),
}
OPTIONS = ("mle_eval_mfma_min_n", "verify_device_hash_min", "verify_workspace_mb")
ZERO_Q = ("one_zero_denominator", "upper_zero")                    # Q = 0: proved all the same, ZERO_DENOMINATOR from the verifier


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _rule(k, batch):
    items = 1 << (k - 1)
    blocks = min(max(-(-items // 1024), -(-2048 // batch)), -(-items // 256), 2048)
    return blocks, (-(-items // blocks) + 255) // 256 * 256


def _chunk(ctx, n, batch):
    """gkr_devtest_fraction_sum_chunk: the proofs per chunk of the verifier under the context's options."""
    out = np.array([0, 0xDEAD], dtype=np.uint32)
    assert N.lib().gkr_devtest_fraction_sum_chunk(ctx._h, n, batch, out.ctypes.data) == N.GKR_OK
    assert out[1] == 0xDEAD                                        # one word, no more
    return int(out[0])


def _reset(ctx):
    for name in OPTIONS:
        ctx.set_option(name, 0)


def _kinds(batch, first):
    return [PAIR_KINDS[(first + b) % len(PAIR_KINDS)] for b in range(batch)]


def _seed(n, b):
    return 27000 + 101 * n + b


_oracle_cache, _seconds = {}, {}


def _oracle(key, T):
    """cdense.fraction_sum_raw(levels=True) of the (2, 2^n, 4) pair T, once per key; the seconds it took go to _seconds."""
    if key not in _oracle_cache:
        t0 = time.perf_counter()
        _oracle_cache[key] = cdense.fraction_sum_raw(T, T.shape[1].bit_length() - 1, levels=True)
        _seconds[key] = time.perf_counter() - t0
    return _oracle_cache[key]


def _matrix_tables(n, batch, first):
    return np.stack([limb_pair(kind, n, _seed(n, b)) for b, kind in enumerate(_kinds(batch, first))])


def _matrix_oracle(n, batch, first, T=None):
    """-> (the eight arrays stacked as the device returns them, [levels per pair], the oracle's seconds)."""
    kinds = _kinds(batch, first)
    if any((n, kind, _seed(n, b)) not in _oracle_cache for b, kind in enumerate(kinds)) and T is None:
        T = _matrix_tables(n, batch, first)
    raws = [_oracle((n, kind, _seed(n, b)), None if T is None else T[b]) for b, kind in enumerate(kinds)]
    want = tuple(np.stack([r[i] for r in raws]) for i in range(8))
    return want, [r[8] for r in raws], sum(_seconds[(n, kind, _seed(n, b))] for b, kind in enumerate(kinds))


def _verdicts(ctx, d, n, batch, H, C, L, R, E, sums):
    accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(d, n, batch, H, C, L, R, E, sums=sums)
    got = [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]
    assert list(accept) == [g == ACCEPTED for g in got]
    return got, out


def _first_difference(got, want, names):
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
    return None if at is None else (at, names[at], got[at], want[at])


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,first", MATRIX)
def test_shape_matrix_matches_the_c_oracle(ctx, n, batch, first):
    assert tree_geometry(n) == [max(1, (1 << k) // 256) for k in range(n)] and tree_geometry(n)[-3:] == [1 << (n - 11), 1 << (n - 10), 1 << (n - 9)]
    for k in (n - 1, n - 2, n - 3):
        assert product_geometry(k, batch)[0] == LAYER_GEOMETRY[(k, batch)] == _rule(k, batch), (k, batch)
    kinds = _kinds(batch, first)
    T = _matrix_tables(n, batch, first)
    if "one_zero_denominator" in kinds:                           # the zero sits in the last block of 256 of D's upper half
        t = T[kinds.index("one_zero_denominator")]
        assert not t[1, zero_index(n)].any() and zero_index(n) >> 8 == (1 << (n - 8)) - 1 and int((~t.any(axis=2)).sum()) == 1
    want, _, oracle_s = _matrix_oracle(n, batch, first, T)
    expect = [(ZERO_DENOMINATOR, 0, 0) if kind in ZERO_Q else ACCEPTED for kind in kinds]
    with Resident(ctx, T) as dev:
        t0 = time.perf_counter()
        got = ctx.fraction_sum_batch_device(dev.d, n, batch)
        prove_s = time.perf_counter() - t0
        dev.assert_unchanged((n, batch))
        _assert_same(got, want, (n, batch, kinds))
        t0 = time.perf_counter()
        for sums in (want[0], None):
            verdicts, out = _verdicts(ctx, dev.d, n, batch, *want[1:6], sums)
            assert verdicts == expect, (n, batch, kinds, verdicts)
            assert np.array_equal(out, want[0]), "out_sums are the oracle's (P, Q)"
        verify_s = time.perf_counter() - t0
        dev.assert_unchanged((n, batch, "verifier"))
    print("\ntiming (%d, %d): oracle %.2f s, device prover %.3f s, device verifier (twice) %.3f s" % (n, batch, oracle_s, prove_s, verify_s))


def test_the_shape_matrix_reaches_every_kind_of_pair_and_short_vectors():
    """(oracle only) every kind of pair occurs at a multi-block size; in the zero-bearing pairs a vector shorter than four occurs in
    the first layer (k = 2), in a layer strictly between, and in the last layer (k = n - 1), where the pair itself is read; full
    vectors occur too; a lookup's P is 0, a zero in D gives Q = 0."""
    seen, short, full = set(), set(), 0
    for n, batch, first in MATRIX:
        kinds = _kinds(batch, first)
        want, _, _ = _matrix_oracle(n, batch, first)
        seen |= set(kinds)
        for b, kind in enumerate(kinds):
            S, L = want[0][b], want[3][b]
            assert S[0].any() == (kind in ("random", "one_zero_denominator", "all_max")), (n, b, kind)     # P = 0: lookups, N = 0, a zero half
            assert S[1].any() == (kind not in ZERO_Q), (n, b, kind)
            full += bool((L == 4).all())
            if kind in ("zero_numerators", "one_zero_denominator", "upper_zero", "lookup", "padded"):
                for where, part in (("first", L[:2]), ("middle", L[2:rounds(n) - (n - 1)]), ("last", L[rounds(n) - (n - 1):])):
                    short |= {where} if (part < 4).any() else set()
            if kind == "upper_zero":
                assert (L == 1).all() and not want[2][b].any() and not want[1][b].any()
    assert seen == set(PAIR_KINDS) and full and short == {"first", "middle", "last"}, (seen, full, short)


# ---- b. every level of the tree -----------------------------------------------------------------------------------------------------------
def test_every_level_of_the_tree_matches_the_c_oracle(ctx):
    n, batch, first = MATRIX[2]
    assert (n, batch) == (17, 20) and tree_geometry(n) == [max(1, (1 << k) // 256) for k in range(n)]
    T = _matrix_tables(n, batch, first)
    _, levels, _ = _matrix_oracle(n, batch, first, T)
    total, pad = 2 * batch * ((1 << n) - 1), 64
    with Resident(ctx, T) as dev, Resident(ctx, np.tile(CANARY, (total + 2 * pad, 1))) as lay:
        assert N.lib().gkr_devtest_fraction_sum_tree(ctx._h, dev.d, n, batch, _ptr_at(lay.d, pad)) == N.GKR_OK
        dev.assert_unchanged((n, batch))
        got = ctx.download(lay.d, (total + 2 * pad, 4))
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all(), "canaries around the levels"
    for b in range(batch):
        for k in range(n):
            at, src = pad + _level_offset(k, batch, b), 2 * ((1 << k) - 1)
            assert np.array_equal(got[at:at + (2 << k)], levels[b][src:src + (2 << k)]), (n, batch, b, k)


# ---- c. tampered proofs with large layers ---------------------------------------------------------------------------------------------------
N_TAMPER = 16
TAMPER_ENTRIES = (0, (1 << 15) - 1, 1 << 15, (1 << 16) - 1)


def _tamper_cases(kind, seed):
    """-> (T (2, 2^16, 4), arrays, sums, [(name, what, closed-form verdict)]) for the oracle's proof of one pair."""
    n = N_TAMPER
    T = limb_pair(kind, n, seed)
    g = as_model(_oracle((n, kind, seed), T), n)
    check_cofactors(g, n)                                          # no rule of the sweep has an exception on this proof
    names = []
    for k in (2, 9, 15):
        for j in sorted({0, k // 2, k - 1}):
            vec = g["layers"][k - 2][0][j]
            names += ["layer %d round %d slot %d + 1" % (k, j, 4 - len(vec) + s) for s in range(len(vec))]
            names += ["layer %d challenge %d + 1" % (k, j), "layer %d length %d + 1" % (k, j), "layer %d length %d - 1" % (k, j)]
        names += ["layer %d value %d + 1" % (k, w) for w in range(4)]
    names += ["head %d + 1" % t for t in range(8)] + ["claimed sum 0 + 1", "claimed sum 1 + 1"]
    cases = pick(tamperings(g, n, True, False, length_steps=True), *names)
    for which in ("num", "den"):                                   # N~(z^(n)) or D~(z^(n)) moves by eq(z^(n), i), never zero at a hashed point
        for i in TAMPER_ENTRIES:
            assert _eq_weight(g["point"], i) != 0
            cases.append(("%s entry %d + 1" % (which, i), (which, i, "+1"), (EVALUATION, n, n)))
    return T, proof_arrays(g, n), list(g["sums"]), cases


def _proof_limbs(n, cases):
    """[(arrays of Python integers, sums)] -> (sums, H, C, L, R, E) limb arrays (elements taken as they are)."""
    B, R = len(cases), rounds(n)
    return (_raw([x for _, s in cases for x in s]).reshape(B, 2, 4), _raw([x for a, _ in cases for x in a[0]]).reshape(B, 8, 4),
            _raw([x for a, _ in cases for row in a[1] for x in row]).reshape(B, R, 4, 4),
            np.array([a[2] for a, _ in cases], dtype=np.int64).astype(np.uint32).reshape(B, R), _raw([x for a, _ in cases for x in a[3]]).reshape(B, R, 4),
            _raw([x for a, _ in cases for e in a[4] for x in e]).reshape(B, n - 2, 4, 4))


def _roots(proofs, want):
    """out_sums: the head's own root, zero where the proof fails SHAPE or NON_CANONICAL."""
    return cdense.to_limbs([x for (a, _), w in zip(proofs, want) for x in ((0, 0) if w[0] in (SHAPE, NON_CANONICAL) else head_root(a[0]))]).reshape(-1, 2, 4)


def test_tampered_proofs_with_large_layers_under_every_setting(ctx):
    """n = 16: the oracle's proofs of a random pair, a lookup's pair and a padded lookup's pair; the changes of
    fraction_sum_sweeps.tamperings at layers 2, 9 and 15 (rounds 0, k / 2 and k - 1: every used slot, the challenge, the length + 1
    and - 1; a0, a1, b0, b1), the eight head entries, claimed P and Q and the entries 0, 2^15 - 1, 2^15 and 2^16 - 1 of N and of D, in
    ONE batch with an honest proof first and last.  The verdicts are the closed form's; every combination of the hash side, the
    evaluation kernel (0: streaming at n = 16, 25: one block per table) and the verifier's workspace (1 MiB: at least three chunks)
    gives them."""
    n = N_TAMPER
    proofs, tables, want, names = [], [], [], []
    seeds = (("random", 27160), ("lookup", 27161), ("padded", 27162))
    for kind, seed in seeds:
        T, arrays, sums, cases = _tamper_cases(kind, seed)
        if not proofs:
            proofs, tables, want, names = [(arrays, sums)], [T], [ACCEPTED], [(kind, "honest")]
        for name, what, verdict in cases:
            if what[0] in ("num", "den"):
                t = T.copy()
                at = (int(what[0] == "den"), what[1])
                t[at] = cdense.to_limbs([cdense.from_limbs(T[at].reshape(1, 4))[0] + 1])[0]
                proofs.append((arrays, sums))
            else:
                t = T
                arr, _, _, s = apply(what, arrays, None, None, sums)
                proofs.append((arr, s))
            tables.append(t)
            want.append(verdict)
            names.append((kind, name))
    proofs.append((arrays, sums))
    tables.append(T)
    want.append(ACCEPTED)
    names.append((kind, "honest"))
    B = len(proofs)
    assert {w[0] for w in want} == {0, SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, FRACTION_SUM}
    assert {w[1] for w in want} >= {0, 2, 9, 15, 16} and want[0] == want[-1] == ACCEPTED
    sums, H, C, L, R, E = _proof_limbs(n, proofs)
    expect_out = _roots(proofs, want)
    verify_s = []
    with Resident(ctx, np.stack(tables)) as dev:
        try:
            for mb in (0, 1):
                for form in (0, 25):
                    for hash_min in (-1, 1):
                        ctx.set_option("verify_workspace_mb", mb)
                        ctx.set_option("mle_eval_mfma_min_n", form)
                        ctx.set_option("verify_device_hash_min", hash_min)
                        chunk = _chunk(ctx, n, B)
                        assert (chunk == B) if mb == 0 else (-(-B // chunk) >= 3), (mb, form, B, chunk)
                        t0 = time.perf_counter()
                        got, out = _verdicts(ctx, dev.d, n, B, H, C, L, R, E, sums)
                        verify_s.append(time.perf_counter() - t0)
                        assert _first_difference(got, want, names) is None, ((mb, form, hash_min, chunk), _first_difference(got, want, names))
                        assert np.array_equal(out, expect_out), (mb, form, hash_min)
                        assert not out[[w[0] == SHAPE for w in want]].any()
        finally:
            _reset(ctx)
        dev.assert_unchanged("tampered proofs")
    print("\ntiming tampered (16, %d): oracle %.2f s (three proofs), device verifier %.3f s (eight settings)"
          % (B, sum(_seconds[(n, kind, seed)] for kind, seed in seeds), sum(verify_s)))


# ---- d. chunks at small n -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_sums", [True, False])
def test_the_small_sweep_tiled_over_several_chunks(ctx, with_sums):
    """tests/test_gpu_fraction_sum.py's n = 5 sweep batch (every single-element change of the random pair's proof, an honest proof
    in front and behind, and the proof of another pair), repeated until verify_workspace_mb = 1 gives at least three chunks, a
    shorter last one and a chunk size that is no multiple of the pair's number of cases -- so chunk boundaries fall inside the
    runs at changing places.  Verdicts and out_sums position by position against the closed form."""
    n = 5
    num, den, g = _pair(n, "random") + (_model(n, "random"),)
    check_inputs(g, n, num, den)
    arrays = proof_arrays(g, n)
    honest = (arrays, num, den, list(g["sums"]))
    sweep = tamperings(g, n, with_sums, True, length_steps=True)
    cases = [honest] + [apply(what, arrays, num, den, g["sums"]) for _, what, _ in sweep] + [honest]
    want = [ACCEPTED] + [w for _, _, w in sweep] + [ACCEPTED]
    names = ["honest"] + [name for name, _, _ in sweep] + ["honest"]
    count = len(cases)
    cases.append((arrays,) + _pair(n, "lookup") + (list(g["sums"]),))
    want.append((EVALUATION, n, n))
    names.append("the proof of another pair")
    assert {w[0] for w in want} >= {0, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION} | ({FRACTION_SUM} if with_sums else set())
    one = _batch_of(n, cases)
    expect_one = _roots([(([h % P for h in c[0][0]],), None) for c in cases], want)     # (a head entry >= r: NON_CANONICAL, no root)
    try:
        ctx.set_option("verify_workspace_mb", 1)
        reps = 1
        while reps < 64:
            B = reps * len(cases)
            chunk = _chunk(ctx, n, B)
            if -(-B // chunk) >= 3 and B % chunk:
                break
            reps += 1
        assert -(-B // chunk) >= 3 and B % chunk and chunk % count and chunk % len(cases), (B, chunk, count)
        T, sums, H, C, L, R, E = (np.concatenate([a] * reps) for a in one)
        want, names, expect_out = want * reps, names * reps, np.concatenate([expect_one] * reps)
        with Resident(ctx, T) as dev:
            for mb in (1, 0):
                ctx.set_option("verify_workspace_mb", mb)
                assert (_chunk(ctx, n, B) == chunk) if mb else (_chunk(ctx, n, B) == B)
                got, out = _verdicts(ctx, dev.d, n, B, H, C, L, R, E, sums if with_sums else None)
                assert _first_difference(got, want, names) is None, (mb, B, chunk, _first_difference(got, want, names))
                assert np.array_equal(out, expect_out), (mb, int(np.argwhere((out != expect_out).any(axis=(1, 2)))[0]))
                assert not out[[w[0] in (SHAPE, NON_CANONICAL) for w in want]].any()
            dev.assert_unchanged("small sweep")
    finally:
        _reset(ctx)


# ---- e. the batch limit ---------------------------------------------------------------------------------------------------------------------
def test_the_batch_limit_of_65535_proofs(ctx):
    """n = 3, batch 65535 (a grid dimension of the tree's and of every layer's launches), seven distinct pairs in turn: 32768 mod 7
    = 1, so the verifier's chunk boundary (chunks of 32768 and 32767) falls inside a cycle.  The prover's arrays are the integer
    model's seven proofs, repeated; the verifier accepts all; then proofs 0, 32767, 32768 and 65534 are changed, one kind of
    change each, and exactly those get their closed-form verdicts."""
    n, batch = 3, 65535
    kinds = ["random", "lookup", "zero_numerators", "all_max", "random", "lookup", "zero_numerators"]
    pairs = [make_tables(kind, n, random.Random(27300 + i)) for i, kind in enumerate(kinds)]
    assert len({tuple(num + den) for num, den in pairs}) == 7 and 32768 % 7 == 1
    gs = [fraction_sum(num, den, n) for num, den in pairs]
    arrs = [proof_arrays(g, n) for g in gs]
    idx = np.arange(batch) % 7
    T7 = cdense.to_limbs([x for num, den in pairs for x in num + den]).reshape(7, 2, 1 << n, 4)
    seven = _proof_limbs(n, [(a, g["sums"]) for a, g in zip(arrs, gs)]) + (
        cdense.to_limbs([x for g in gs for x in g["point"]]).reshape(7, n, 4), cdense.to_limbs([x for g in gs for x in g["claim"]]).reshape(7, 2, 4))
    want = tuple(a[idx] for a in seven)
    assert _chunk(ctx, n, batch) == 32768 and batch - 32768 == 32767
    T = np.ascontiguousarray(T7[idx])
    with Resident(ctx, T) as dev:
        t0 = time.perf_counter()
        got = ctx.fraction_sum_batch_device(dev.d, n, batch)
        prove_s = time.perf_counter() - t0
        dev.assert_unchanged((n, batch))
        _assert_same(got, want, (n, batch))
        t0 = time.perf_counter()
        verdicts, out = _verdicts(ctx, dev.d, n, batch, *want[1:6], want[0])
        verify_s = time.perf_counter() - t0
        assert verdicts == [ACCEPTED] * batch and np.array_equal(out, want[0])
        sums, H, C, L, R, E = (a.copy() for a in want[:6])
        expect = [ACCEPTED] * batch
        i_num, i_den = table_entries(n)
        for b, name in ((0, "claimed sum 0 + 1"), (32767, "layer 2 challenge 1 + 1"), (32768, "layer 2 round 0 slot 3 + 1"), (65534, "den entry %d + 1" % i_den)):
            t = int(idx[b])
            _, what, verdict = pick(tamperings(gs[t], n, True, True), name)[0]
            arr, num, den, s = apply(what, arrs[t], pairs[t][0], pairs[t][1], gs[t]["sums"])
            s1, H1, C1, L1, R1, E1 = _proof_limbs(n, [(arr, s)])
            sums[b], H[b], C[b], L[b], R[b], E[b] = s1[0], H1[0], C1[0], L1[0], R1[0], E1[0]
            if what[0] == "den":
                assert _eq_weight(gs[t]["point"], what[1]) != 0
                dev.set_entry((b << (n + 1)) + (1 << n) + what[1], cdense.to_limbs([den[what[1]]])[0])
            expect[b] = verdict
        assert [expect[b][0] for b in (0, 32767, 32768, 65534)] == [FRACTION_SUM, CHALLENGE, ROUND_SUM, EVALUATION]
        verdicts, _ = _verdicts(ctx, dev.d, n, batch, H, C, L, R, E, sums)
        bad = [b for b in range(batch) if verdicts[b] != ACCEPTED]
        assert bad == [0, 32767, 32768, 65534] and [verdicts[b] for b in bad] == [expect[b] for b in bad], (bad, [verdicts[b] for b in bad])
    print("\ntiming (3, 65535): device prover %.3f s, device verifier %.3f s" % (prove_s, verify_s))


# ---- f. the whole call past 4 GiB -----------------------------------------------------------------------------------------------------------
def test_the_whole_call_with_a_pair_four_gib_into_the_tables(ctx):
    """n = 16, batch 1025: pair 1024 starts at byte 2^32 of the tables, its levels past byte 2^32 of the workspace, and its rows at
    proof 1024 of every output array.  Proofs 0 and 1024 are the oracle's on the downloaded pairs; the verifier accepts all 1025; one
    changed entry of D in pair 1024 fails proof 1024 alone, in the evaluation."""
    n, batch = 16, 1025
    size = 64 << n
    assert (batch - 1) * size == 1 << 32
    if free_bytes() < int(3.2 * batch * size):
        pytest.skip("not enough free device memory for 1025 pairs of 2^16 entries, their levels and the layers' workspace")
    d = ctx.alloc(batch * size)
    try:
        ctx.fill_table(d, batch << (n + 1), 4747)
        t0 = time.perf_counter()
        got = ctx.fraction_sum_batch_device(d, n, batch)
        prove_s = time.perf_counter() - t0
        point = None
        for b in (0, batch - 1):
            T = ctx.download(_ptr_at(d, b << (n + 1)), (2, 1 << n, 4))
            raw = _oracle(("4gib", b), T)
            _assert_same(tuple(a[b:b + 1] for a in got), tuple(a[None] for a in raw[:8]), (n, batch, b))
            point = cdense.from_limbs(raw[6])
        assert _chunk(ctx, n, batch) == batch                      # one chunk: the pair offset is the evaluation kernel's own
        t0 = time.perf_counter()
        verdicts, out = _verdicts(ctx, d, n, batch, *got[1:6], got[0])
        verify_s = time.perf_counter() - t0
        assert verdicts == [ACCEPTED] * batch and np.array_equal(out, got[0])
        index = 54321
        assert _eq_weight(point, index) != 0                      # the closed form: D~(z^(n)) moves by eq(z^(n), index)
        entry = cdense.from_limbs(T[1, index:index + 1])[0]
        ctx.upload(_ptr_at(d, ((batch - 1) << (n + 1)) + (1 << n) + index), cdense.to_limbs([entry + 1]))
        verdicts, _ = _verdicts(ctx, d, n, batch, *got[1:6], got[0])
        assert verdicts == [ACCEPTED] * (batch - 1) + [(EVALUATION, n, n)]
    finally:
        ctx.free(d)
    print("\ntiming (16, 1025): oracle %.2f s (two proofs), device prover %.3f s, device verifier %.3f s"
          % (_seconds[("4gib", 0)] + _seconds[("4gib", batch - 1)], prove_s, verify_s))

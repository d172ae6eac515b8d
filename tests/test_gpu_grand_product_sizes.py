"""gkr_grand_product_batch_device and its verifier (csrc/capi_grand_product.hip, csrc/kernels_grand_product.hip) bit for bit against
the C oracle's ogkr_grand_product (cdense.grand_product_raw; tests/test_oracle_grand_product_c.py holds it to the integer model and
to both integer verifiers) at the sizes tests/test_gpu_grand_product.py compares with nothing independent.  The oracle runs the
tree as a loop of products and every layer as the EXPLICIT zero-check; it shares no code with the library, so the zero-check's
launches at the layer geometries k = 13 .. 19 with two tables, and the driver's own work there -- the level offsets handed to the
zero-check as table bases, the row scatter into the proof's arrays, the tau chain -- are held to something independent.

  a. the shape matrix (n, batch) = (16, 1), (16, 20), (18, 5), (20, 1), (20, 4): the launch geometry of the tree and of the top three
     layers asserted first; six kinds of table in turn; all eight output arrays; inputs unchanged; the device verifier accepts;
  b. every level of the tree at (16, 20) and (20, 1), canaries on either side;
  c. tampered proofs with layers up to k = 15 in one batch at n = 16, verdicts from the closed form alone, under both hash sides,
     both evaluation kernels and one / several chunks of the verifier;
  d. the n = 5 sweep tiled over at least three chunks with a ragged last one, with and without claimed products;
  e. the batch limit 65535 at n = 3 (chunks of 32768 and 32767);  f. the whole call with a table 4 GiB into the tables.

Every chunking case asserts its chunk size through gkr_devtest_grand_product_chunk first.  The library's own output is never the
reference of a verdict or a value.  Each case prints the seconds the oracle and the device calls took (pytest -s shows them)."""

import random
import time

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from grand_product_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, KINDS, NON_CANONICAL, PRODUCT, ROUND_SUM, SHAPE, grand_product, make_table,
                                 proof_arrays, rounds)
from grand_product_oracle import TABLE_KINDS, as_model, limb_table, pick, zero_index
from grand_product_sweeps import _eq_weight, apply, tamperings
from oracle import cdense
from oracle.field import P
from product_shapes import product_geometry
from resident_tables import Resident, free_bytes
from test_gpu_grand_product import CANARY, _assert_same, _batch_of, _level_offset, _model, _ptr_at, _raw, _table
from test_grand_product_host import tree_geometry

pytestmark = pytest.mark.gpu

# (n, batch, the kind of table 0 -- table b takes the b-th kind after it in TABLE_KINDS).  The batch-1 cases take tables of
# distinct entries (one zero, random): on a constant table an operand read one entry off gives the same bytes.
MATRIX = [(16, 1, 4), (16, 20, 0), (18, 5, 1), (20, 1, 0), (20, 4, 3)]
# (k, batch) -> (blocks per sumcheck, chunk) of round 0 of layer k's zero-check, which runs on tables of 2^k entries: what
# mle_blocks_per_table gives for items = 2^(k-1) pairs with the default items_per_block,
#   blocks = min(max(ceil(items / 1024), ceil(2048 / batch)), ceil(items / 256), 2048),   chunk = ceil(items / blocks) rounded up to 256.
# A retuned geometry has to fail the pin, not leave these cases running something else.
LAYER_GEOMETRY = {
    (13, 1): (16, 256), (14, 1): (32, 256),      # half a trip of the round kernel's 64-lane loop over the partials
    (15, 1): (64, 256),                          # exactly one trip
    (13, 20): (16, 256), (14, 20): (32, 256), (15, 20): (64, 256),
    (15, 5): (64, 256), (16, 5): (128, 256), (17, 5): (256, 256),
    (17, 1): (256, 256), (18, 1): (512, 256), (19, 1): (1024, 256),
    (17, 4): (256, 256), (18, 4): (512, 256), (19, 4): (512, 512),     # the fill term 2048 / 4 caps the blocks: two pairs per thread
}
OPTIONS = ("mle_eval_mfma_min_n", "verify_device_hash_min", "verify_workspace_mb")


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
    """gkr_devtest_grand_product_chunk: the proofs per chunk of the verifier under the context's options."""
    out = np.array([0, 0xDEAD], dtype=np.uint32)
    assert N.lib().gkr_devtest_grand_product_chunk(ctx._h, n, batch, out.ctypes.data) == N.GKR_OK
    assert out[1] == 0xDEAD                                        # one word, no more
    return int(out[0])


def _reset(ctx):
    for name in OPTIONS:
        ctx.set_option(name, 0)


def _kinds(batch, first):
    return [TABLE_KINDS[(first + b) % len(TABLE_KINDS)] for b in range(batch)]


def _seed(n, b):
    return 26000 + 101 * n + b


_oracle_cache, _seconds = {}, {}


def _oracle(key, T):
    """cdense.grand_product_raw(levels=True) of the (2^n, 4) table T, once per key; the seconds it took go to _seconds."""
    if key not in _oracle_cache:
        t0 = time.perf_counter()
        _oracle_cache[key] = cdense.grand_product_raw(T, T.shape[0].bit_length() - 1, levels=True)
        _seconds[key] = time.perf_counter() - t0
    return _oracle_cache[key]


def _matrix_tables(n, batch, first):
    return np.stack([limb_table(kind, n, _seed(n, b)) for b, kind in enumerate(_kinds(batch, first))])


def _matrix_oracle(n, batch, first, T=None):
    """-> (the eight arrays stacked as the device returns them, [levels per table], the oracle's seconds)."""
    kinds = _kinds(batch, first)
    if any((n, kind, _seed(n, b)) not in _oracle_cache for b, kind in enumerate(kinds)) and T is None:
        T = _matrix_tables(n, batch, first)
    raws = [_oracle((n, kind, _seed(n, b)), None if T is None else T[b]) for b, kind in enumerate(kinds)]
    want = tuple(np.stack([r[i] for r in raws]) for i in range(8))
    return want, [r[8] for r in raws], sum(_seconds[(n, kind, _seed(n, b))] for b, kind in enumerate(kinds))


def _verdicts(ctx, d, n, batch, H, C, L, R, E, products):
    accept, layer, rnd, check, out = ctx.verify_grand_product_batch_device(d, n, batch, H, C, L, R, E, products=products)
    got = [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]
    assert list(accept) == [g == (0, 0, 0) for g in got]
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
    if "one_zero" in kinds:                                       # the zero sits in the last block of 256 of the upper half
        t = T[kinds.index("one_zero")]
        assert not t[zero_index(n)].any() and zero_index(n) >> 8 == (1 << (n - 8)) - 1 and int((~t.any(axis=1)).sum()) == 1
    want, _, oracle_s = _matrix_oracle(n, batch, first, T)
    with Resident(ctx, T) as dev:
        t0 = time.perf_counter()
        got = ctx.grand_product_batch_device(dev.d, n, batch)
        prove_s = time.perf_counter() - t0
        dev.assert_unchanged((n, batch))
        _assert_same(got, want, (n, batch, kinds))
        t0 = time.perf_counter()
        for products in (want[0], None):
            verdicts, out = _verdicts(ctx, dev.d, n, batch, *want[1:6], products)
            assert verdicts == [(0, 0, 0)] * batch, (n, batch, kinds, verdicts)
            assert np.array_equal(out, want[0]), "out_products are the oracle's P"
        verify_s = time.perf_counter() - t0
        dev.assert_unchanged((n, batch, "verifier"))
    print("\ntiming (%d, %d): oracle %.2f s, device prover %.3f s, device verifier (twice) %.3f s" % (n, batch, oracle_s, prove_s, verify_s))


def test_the_shape_matrix_reaches_every_kind_of_table_and_short_vectors():
    """(oracle only) every kind of table occurs, the zero-bearing ones at n = 16, 18 and 20; and in the zero-bearing tables a
    vector shorter than four occurs in the first layer (k = 2), in a layer strictly between, and in the last layer (k = n - 1),
    where the table itself is read; a table with one zero entry has full vectors too, and product zero."""
    seen, short = set(), set()
    for n, batch, first in MATRIX:
        kinds = _kinds(batch, first)
        want, _, _ = _matrix_oracle(n, batch, first)
        seen |= {(n, kind) for kind in kinds}
        for b, kind in enumerate(kinds):
            if kind not in ("one_zero", "upper_zero"):
                assert want[0][b].any() == (kind != "specials"), (n, b, kind)                              # (the patterns include 0)
                continue
            assert not want[0][b].any(), (n, b, kind)                                                      # P = 0
            L = want[3][b]
            for where, part in (("first", L[:2]), ("middle", L[2:rounds(n) - (n - 1)]), ("last", L[rounds(n) - (n - 1):])):
                short |= {where} if (part < 4).any() else set()
            if kind == "upper_zero":
                assert (L == 1).all() and not want[2][b].any() and not want[1][b].any()
            else:
                assert (L == 4).any()
    assert {kind for _, kind in seen} == set(TABLE_KINDS) and {n for n, kind in seen if kind in ("one_zero", "upper_zero")} == {16, 18, 20}
    assert short == {"first", "middle", "last"}, short


# ---- b. every level of the tree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,first", [m for m in MATRIX if m[:2] in ((16, 20), (20, 1))])
def test_every_level_of_the_tree_matches_the_c_oracle(ctx, n, batch, first):
    assert tree_geometry(n) == [max(1, (1 << k) // 256) for k in range(n)]
    T = _matrix_tables(n, batch, first)
    _, levels, _ = _matrix_oracle(n, batch, first, T)
    total, pad = batch * ((1 << n) - 1), 64
    with Resident(ctx, T) as dev, Resident(ctx, np.tile(CANARY, (total + 2 * pad, 1))) as lay:
        assert N.lib().gkr_devtest_grand_product_tree(ctx._h, dev.d, n, batch, _ptr_at(lay.d, pad)) == N.GKR_OK
        dev.assert_unchanged((n, batch))
        got = ctx.download(lay.d, (total + 2 * pad, 4))
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all(), "canaries around the levels"
    for b in range(batch):
        for k in range(n):
            at = pad + _level_offset(k, batch) + (b << k)
            assert np.array_equal(got[at:at + (1 << k)], levels[b][(1 << k) - 1:(2 << k) - 1]), (n, batch, b, k)


# ---- c. tampered proofs with large layers ---------------------------------------------------------------------------------------------------
N_TAMPER = 16


def _tamper_cases(kind, seed):
    """-> (T (2^16, 4), raw, arrays, product, [(name, what, closed-form verdict)]) for the oracle's proof of one table."""
    n = N_TAMPER
    T = limb_table(kind, n, seed)
    raw = _oracle((n, kind, seed), T)
    g = as_model(raw, n)
    names = []
    for k in (2, 9, 15):
        for j in sorted({0, k // 2, k - 1}):
            vec = g["layers"][k - 2][0][j]
            names += ["layer %d round %d slot %d" % (k, j, s) for s in range(len(vec))]                    # (s counts the used slots)
            names += ["layer %d challenge %d" % (k, j), "layer %d length %d + 1" % (k, j), "layer %d length %d - 1" % (k, j)]
        names += ["layer %d value 0" % k, "layer %d value 1" % k]
    names += ["head %d" % t for t in range(4)] + ["claimed product"]
    names += ["table entry %d" % i for i in (0, (1 << 15) - 1, 1 << 15, (1 << 16) - 1)]
    return T, raw, proof_arrays(g, n), g["product"], pick(tamperings(g, n, True, True), *names)


def _proof_limbs(n, cases):
    """[(arrays of Python integers, product)] -> (products, H, C, L, R, E) limb arrays (elements taken as they are)."""
    B, R = len(cases), rounds(n)
    return (_raw([p for _, p in cases]), _raw([x for a, _ in cases for x in a[0]]).reshape(B, 4, 4),
            _raw([x for a, _ in cases for row in a[1] for x in row]).reshape(B, R, 4, 4),
            np.array([a[2] for a, _ in cases], dtype=np.int64).astype(np.uint32).reshape(B, R), _raw([x for a, _ in cases for x in a[3]]).reshape(B, R, 4),
            _raw([x for a, _ in cases for e in a[4] for x in e]).reshape(B, n - 2, 2, 4))


def test_tampered_proofs_with_large_layers_under_every_setting(ctx):
    """n = 16: the oracle's proofs of a random table and of a table with one zero entry; the changes of
    grand_product_sweeps.tamperings at layers 2, 9 and 15 (rounds 0, k / 2 and k - 1: every used slot, the challenge, the length
    + 1 and - 1; a_k and b_k), the head, the claimed product and the table entries 0, 2^15 - 1, 2^15 and 2^16 - 1, in ONE batch with an
    honest proof first and last.  The verdicts are the closed form's; every combination of the hash side, the evaluation kernel
    (0: streaming at n = 16, 25: one block per table) and the verifier's workspace (1 MiB: at least three chunks) gives them."""
    n = N_TAMPER
    proofs, tables, want, names = [], [], [], []
    for kind, seed in (("random", 26160), ("one_zero", 26161)):
        T, _, arrays, product, cases = _tamper_cases(kind, seed)
        if not proofs:
            proofs, tables, want, names = [(arrays, product)], [T], [(0, 0, 0)], [(kind, "honest")]
        for name, what, verdict in cases:
            if what[0] == "table":
                t = T.copy()
                t[what[1]] = cdense.to_limbs([cdense.from_limbs(T[what[1]])[0] + 1])[0]
                proofs.append((arrays, product))
            else:
                t = T
                arr, _, prod = apply(what, arrays, None, product)
                proofs.append((arr, prod))
            tables.append(t)
            want.append(verdict)
            names.append((kind, name))
    proofs.append((arrays, product))
    tables.append(T)
    want.append((0, 0, 0))
    names.append((kind, "honest"))
    B = len(proofs)
    assert {w[0] for w in want} == {0, SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, PRODUCT}
    assert {w[1] for w in want} >= {0, 2, 9, 15, 16} and want[0] == want[-1] == (0, 0, 0)
    products, H, C, L, R, E = _proof_limbs(n, proofs)
    expect_out = cdense.to_limbs([0 if w[0] in (SHAPE, NON_CANONICAL) else a[0][0] * a[0][1] * a[0][2] * a[0][3] % P for (a, _), w in zip(proofs, want)])
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
                        got, out = _verdicts(ctx, dev.d, n, B, H, C, L, R, E, products)
                        verify_s.append(time.perf_counter() - t0)
                        assert _first_difference(got, want, names) is None, ((mb, form, hash_min, chunk), _first_difference(got, want, names))
                        assert np.array_equal(out, expect_out), (mb, form, hash_min)
        finally:
            _reset(ctx)
        dev.assert_unchanged("tampered proofs")
    print("\ntiming tampered (16, %d): oracle %.2f s (two proofs), device verifier %.3f s (eight settings)"
          % (B, _seconds[(n, "random", 26160)] + _seconds[(n, "one_zero", 26161)], sum(verify_s)))


# ---- d. chunks at small n -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_product", [True, False])
def test_the_small_sweep_tiled_over_several_chunks(ctx, with_product):
    """tests/test_gpu_grand_product.py's n = 5 sweep batch (every single-element change, all kinds of table, honest proofs around
    each table's changes, the proof of another table), repeated until verify_workspace_mb = 1 gives at least three chunks, a shorter
    last one and a chunk size that is no multiple of any table's number of cases -- so chunk boundaries fall inside the tables'
    runs at changing places.  Verdicts and out_products position by position against the closed form."""
    n = 5
    cases, want, names, counts = [], [], [], []
    for kind in KINDS:
        table, g = _table(n, kind), _model(n, kind)
        arrays = proof_arrays(g, n)
        honest = (arrays, table, g["product"])
        sweep = tamperings(g, n, with_product, True)
        cases += [honest] + [apply(what, arrays, table, g["product"]) for _, what, _ in sweep] + [honest]
        want += [(0, 0, 0)] + [w for _, _, w in sweep] + [(0, 0, 0)]
        names += [(kind, "honest")] + [(kind, name) for name, _, _ in sweep] + [(kind, "honest")]
        counts.append(len(sweep) + 2)
    cases.append((proof_arrays(_model(n, "random"), n), _table(n, "one_zero"), _model(n, "random")["product"]))
    want.append((EVALUATION, n, n))
    names.append(("random", "the proof of another table"))
    assert {w[0] for w in want} >= {0, SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION} | ({PRODUCT} if with_product else set())
    one = _batch_of(n, cases)
    expect_one = cdense.to_limbs([0 if w[0] in (SHAPE, NON_CANONICAL) else a[0][0] * a[0][1] * a[0][2] * a[0][3] % P for (a, _, _), w in zip(cases, want)])
    try:
        ctx.set_option("verify_workspace_mb", 1)
        reps = 1
        while reps < 16:
            B = reps * len(cases)
            chunk = _chunk(ctx, n, B)
            if -(-B // chunk) >= 3 and B % chunk:
                break
            reps += 1
        assert -(-B // chunk) >= 3 and B % chunk and all(chunk % c for c in counts) and chunk % len(cases), (B, chunk, counts)
        T, products, H, C, L, R, E = (np.concatenate([a] * reps) for a in one)
        want, names, expect_out = want * reps, names * reps, np.concatenate([expect_one] * reps)
        with Resident(ctx, T) as dev:
            for mb in (1, 0):
                ctx.set_option("verify_workspace_mb", mb)
                assert (_chunk(ctx, n, B) == chunk) if mb else (_chunk(ctx, n, B) == B)
                got, out = _verdicts(ctx, dev.d, n, B, H, C, L, R, E, products if with_product else None)
                assert _first_difference(got, want, names) is None, (mb, B, chunk, _first_difference(got, want, names))
                assert np.array_equal(out, expect_out), (mb, int(np.argwhere((out != expect_out).any(axis=1))[0]))
                assert not out[[w[0] == SHAPE for w in want]].any()
            dev.assert_unchanged("small sweep")
    finally:
        _reset(ctx)


# ---- e. the batch limit ---------------------------------------------------------------------------------------------------------------------
def test_the_batch_limit_of_65535_proofs(ctx):
    """n = 3, batch 65535 (a grid dimension of the tree's and of every layer's launches), seven distinct tables in turn: 32768 mod 7
    = 1, so the verifier's chunk boundary (chunks of 32768 and 32767) falls inside a cycle.  The prover's arrays are the integer
    model's seven proofs, repeated; the verifier accepts all; then proofs 0, 32767, 32768 and 65534 are changed, one kind of
    change each, and exactly those get their closed-form verdicts."""
    n, batch = 3, 65535
    kinds = ["random", "ones", "one_zero", "upper_zero", "all_max", "random", "one_zero"]
    tables = [make_table(kind, n, random.Random(26300 + i)) for i, kind in enumerate(kinds)]
    assert len({tuple(t) for t in tables}) == 7 and 32768 % 7 == 1
    gs = [grand_product(t, n) for t in tables]
    arrs = [proof_arrays(g, n) for g in gs]
    idx = np.arange(batch) % 7
    T7 = cdense.to_limbs([x for t in tables for x in t]).reshape(7, 1 << n, 4)
    seven = (cdense.to_limbs([g["product"] for g in gs]),) + _proof_limbs(n, [(a, g["product"]) for a, g in zip(arrs, gs)])[1:] + (
        cdense.to_limbs([x for g in gs for x in g["point"]]).reshape(7, n, 4), cdense.to_limbs([g["claim"] for g in gs]))
    want = tuple(a[idx] for a in seven)
    assert _chunk(ctx, n, batch) == 32768 and batch - 32768 == 32767
    T = np.ascontiguousarray(T7[idx])
    with Resident(ctx, T) as dev:
        got = ctx.grand_product_batch_device(dev.d, n, batch)
        dev.assert_unchanged((n, batch))
        _assert_same(got, want, (n, batch))
        verdicts, out = _verdicts(ctx, dev.d, n, batch, *want[1:6], want[0])
        assert verdicts == [(0, 0, 0)] * batch and np.array_equal(out, want[0])
        products, H, C, L, R, E = (a.copy() for a in want[:6])
        expect = [(0, 0, 0)] * batch
        for b, name in ((0, "claimed product"), (32767, "layer 2 challenge 1"), (32768, "layer 2 round 0 slot 0"), (65534, "table entry 5")):
            t = int(idx[b])
            _, what, verdict = pick(tamperings(gs[t], n, True, True), name)[0]
            arr, table, product = apply(what, arrs[t], tables[t], gs[t]["product"])
            p1, H1, C1, L1, R1, E1 = _proof_limbs(n, [(arr, product)])
            products[b], H[b], C[b], L[b], R[b], E[b] = p1[0], H1[0], C1[0], L1[0], R1[0], E1[0]
            if what[0] == "table":
                dev.set_entry((b << n) + what[1], cdense.to_limbs([table[what[1]]])[0])
            expect[b] = verdict
        assert [expect[b][0] for b in (0, 32767, 32768, 65534)] == [PRODUCT, CHALLENGE, ROUND_SUM, EVALUATION]
        verdicts, _ = _verdicts(ctx, dev.d, n, batch, H, C, L, R, E, products)
        bad = [b for b in range(batch) if verdicts[b] != (0, 0, 0)]
        assert bad == [0, 32767, 32768, 65534] and [verdicts[b] for b in bad] == [expect[b] for b in bad], (bad, [verdicts[b] for b in bad])


# ---- f. the whole call past 4 GiB -----------------------------------------------------------------------------------------------------------
def test_the_whole_call_with_a_table_four_gib_into_the_tables(ctx):
    """n = 16, batch 2049: table 2048 starts at byte 2^32 of the tables, its levels past byte 2^32 of the workspace, and its rows
    at proof 2048 of every output array.  Proofs 0 and 2048 are the oracle's on the downloaded tables; the verifier accepts all
    2049; one changed entry of table 2048 fails proof 2048 alone, in the evaluation."""
    n, batch = 16, 2049
    size = 32 << n
    assert (batch - 1) * size == 1 << 32
    if free_bytes() < int(3.2 * batch * size):
        pytest.skip("not enough free device memory for 2049 tables of 2^16 entries, their levels and the layers' workspace")
    d = ctx.alloc(batch * size)
    try:
        ctx.fill_table(d, batch << n, 4646)
        t0 = time.perf_counter()
        got = ctx.grand_product_batch_device(d, n, batch)
        prove_s = time.perf_counter() - t0
        point = None
        for b in (0, batch - 1):
            T = ctx.download(_ptr_at(d, b << n), (1 << n, 4))
            raw = _oracle(("4gib", b), T)
            _assert_same(tuple(a[b:b + 1] for a in got), tuple(a[None] for a in raw[:8]), (n, batch, b))
            point = cdense.from_limbs(raw[6])
        assert _chunk(ctx, n, batch) == batch                      # one chunk: the table offset is the evaluation kernel's own
        t0 = time.perf_counter()
        verdicts, out = _verdicts(ctx, d, n, batch, *got[1:6], got[0])
        verify_s = time.perf_counter() - t0
        assert verdicts == [(0, 0, 0)] * batch and np.array_equal(out, got[0])
        index = 54321
        assert _eq_weight(point, index) != 0                      # the closed form: V~(z^(n)) moves by eq(z^(n), index)
        entry = cdense.from_limbs(T[index])[0]
        ctx.upload(_ptr_at(d, ((batch - 1) << n) + index), cdense.to_limbs([entry + 1]))
        verdicts, _ = _verdicts(ctx, d, n, batch, *got[1:6], got[0])
        assert verdicts == [(0, 0, 0)] * (batch - 1) + [(EVALUATION, n, n)]
    finally:
        ctx.free(d)
    print("\ntiming (16, 2049): oracle %.2f s (two proofs), device prover %.3f s, device verifier %.3f s"
          % (_seconds[("4gib", 0)] + _seconds[("4gib", batch - 1)], prove_s, verify_s))

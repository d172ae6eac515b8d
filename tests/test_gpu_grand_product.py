"""gkr_grand_product_batch_device and its verifier (csrc/kernels_grand_product.hip, csrc/capi_grand_product.hip) on the device:

  a. the tree alone (gkr_devtest_grand_product_tree) bit for bit against numpy object arrays of Python integers, every level, at
     n = 3, 4, 5, on either side of the first n with a launch of more than one block (9, 10) and at n = 12, the launch geometry
     asserted first; batches of 1 and 3; all-max operands; canaries around the levels; a table 4 GiB into the tables;
  b. the whole call against the integer model (tests/grand_product_model.py), every output array, with the zero-bearing tables;
  c. every layer byte-equal to a direct gkr_sumcheck_zerocheck_batch_device call on that level of the devtest tree at the recorded
     z^(k), at n = 14 and 16;
  d. the device verifier: honest proofs accepted at every shape; the host sweep's tampered proofs at n = 4 and 5 in ONE batch with
     honest ones, under both hash sides, against the closed-form verdicts (tests/grand_product_sweeps.py); elements >= r;
  e. one size case, n = 20; f. one context for a zero-check, a grand product and the same zero-check again; g. the host-table forms.

The library's own output is never the reference of a verdict or a value."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from grand_product_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, KINDS, NON_CANONICAL, PRODUCT, ROUND_SUM, SHAPE, eq_point, grand_product,
                                 layer_row, make_table, model_verdict, product_tree_np, proof_arrays, rounds)
from grand_product_sweeps import apply, layers_of, tamperings
from oracle.mimc7 import multi_hash
from resident_tables import Resident, free_bytes
from test_grand_product_host import tree_geometry
from verify_sweeps import R_LIMBS, limbs

pytestmark = pytest.mark.gpu

# blocks of 256 threads per table of the launch of level k = 0 .. n - 1 (a thread per product): n = 9 is the last table whose every
# launch is one block, n = 10 the first whose top launch has two, n = 12 has launches of 2, 4 and 8 blocks
GEOMETRY = {3: [1] * 3, 4: [1] * 4, 5: [1] * 5, 9: [1] * 9, 10: [1] * 9 + [2], 12: [1] * 9 + [2, 4, 8]}
CANARY = np.array([0xC0DEC0DEC0DEC0DE, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
TERMS = [(1, (0, 1))]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_tables, _models = {}, {}


def _table(n, kind):
    """One table per (n, kind), the same in every test."""
    if (n, kind) not in _tables:
        _tables[(n, kind)] = make_table(kind, n, random.Random(7000 + 31 * n + KINDS.index(kind)))
    return _tables[(n, kind)]


def _model(n, kind):
    if (n, kind) not in _models:
        _models[(n, kind)] = grand_product(np.array(_table(n, kind), dtype=object), n, use_np=True)
    return _models[(n, kind)]


def _kinds(n, batch):
    row = ["one_zero", "upper_zero", ("random", "ones", "all_max")[n % 3]]
    return row if batch == 3 else [row[n % 3]]


def _level_offset(k, batch):
    return batch * ((1 << k) - 1)


def _ptr_at(d, elements):
    return ctypes.c_void_p(d.value + 32 * elements)


# ---- a. the tree alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", sorted(GEOMETRY))
def test_tree_matches_python_integers_at_every_level(ctx, n, batch):
    assert tree_geometry(n) == GEOMETRY[n], n
    kinds = ["all_max", "random", "one_zero"][:batch] if n % 2 else ["random", "all_max", "upper_zero"][:batch]
    tables = [_table(n, kind) for kind in kinds]
    T = to_limbs([x for t in tables for x in t]).reshape(batch, 1 << n, 4)
    total, pad = batch * ((1 << n) - 1), 64
    with Resident(ctx, T) as dev, Resident(ctx, np.tile(CANARY, (total + 2 * pad, 1))) as lay:
        rc = N.lib().gkr_devtest_grand_product_tree(ctx._h, dev.d, n, batch, _ptr_at(lay.d, pad))
        assert rc == N.GKR_OK, rc
        dev.assert_unchanged((n, batch))
        got = ctx.download(lay.d, (total + 2 * pad, 4))
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all(), "canaries around the levels"
    for b, table in enumerate(tables):
        levels = product_tree_np(np.array(table, dtype=object), n)
        for k in range(n):
            at = pad + _level_offset(k, batch) + (b << k)
            assert from_limbs(got[at:at + (1 << k)]) == [int(x) for x in levels[k]], (n, batch, b, k)


def test_tree_with_a_table_four_gib_into_the_tables(ctx):
    """n = 16, batch 2049: the last table starts at byte 2^32 of the tables and its level 15 past byte 2^32 of the levels; every
    offset is formed in 64 bits."""
    n, batch = 16, 2049
    size = 32 << n
    assert (batch - 1) * size == 1 << 32
    total = batch * ((1 << n) - 1)
    if free_bytes() < int(1.1 * (batch * size + 32 * total)):
        pytest.skip("not enough free device memory for 2049 tables of 2^16 entries and their levels")
    d, lay = ctx.alloc(batch * size), ctx.alloc(32 * (total + 128))
    try:
        ctx.fill_table(d, batch << n, 4242)
        ctx.upload(lay, np.tile(CANARY, (64, 1)))
        ctx.upload(_ptr_at(lay, 64 + total), np.tile(CANARY, (64, 1)))
        assert N.lib().gkr_devtest_grand_product_tree(ctx._h, d, n, batch, _ptr_at(lay, 64)) == N.GKR_OK
        assert (ctx.download(lay, (64, 4)) == CANARY).all() and (ctx.download(_ptr_at(lay, 64 + total), (64, 4)) == CANARY).all()
        for b in (0, batch - 1):
            table = np.array(from_limbs(ctx.download(_ptr_at(d, b << n), (1 << n, 4))), dtype=object)
            levels = product_tree_np(table, n)
            for k in (0, 1, 2, 3, 8, n - 2, n - 1):
                got = ctx.download(_ptr_at(lay, 64 + _level_offset(k, batch) + (b << k)), (1 << k, 4))
                assert from_limbs(got) == [int(x) for x in levels[k]], (b, k)
    finally:
        ctx.free(d)
        ctx.free(lay)


# ---- b. the whole call against the model --------------------------------------------------------------------------------------------------
def _model_arrays(n, kinds):
    """The model's proofs of the tables (n, kind) as the eight arrays of Context.grand_product_batch_device."""
    gs = [_model(n, kind) for kind in kinds]
    arrs = [proof_arrays(g, n) for g in gs]
    B, R = len(kinds), rounds(n)
    return (to_limbs([g["product"] for g in gs]), to_limbs([x for a in arrs for x in a[0]]).reshape(B, 4, 4),
            to_limbs([x for a in arrs for row in a[1] for x in row]).reshape(B, R, 4, 4), np.array([a[2] for a in arrs], dtype=np.uint32).reshape(B, R),
            to_limbs([x for a in arrs for x in a[3]]).reshape(B, R, 4), to_limbs([x for a in arrs for e in a[4] for x in e]).reshape(B, n - 2, 2, 4),
            to_limbs([x for g in gs for x in g["point"]]).reshape(B, n, 4), to_limbs([g["claim"] for g in gs]))


NAMES = ("products", "head", "coefficients", "lengths", "challenges", "values", "point", "claim")


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            pytest.fail("%s: %s differ first at %s: got %s, want %s" % (what, name, at, g[at[:-1]], w[at[:-1]]))


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [3, 4, 5, 8, 9, 10, 12])
def test_whole_call_matches_the_model_and_is_accepted(ctx, n, batch):
    kinds = _kinds(n, batch)
    T = to_limbs([x for kind in kinds for x in _table(n, kind)]).reshape(batch, 1 << n, 4)
    want = _model_arrays(n, kinds)
    with Resident(ctx, T) as dev:
        got = ctx.grand_product_batch_device(dev.d, n, batch)
        dev.assert_unchanged((n, batch))
        _assert_same(got, want, (n, batch, kinds))
        for products in (got[0], None):
            accept, layer, rnd, check, out = ctx.verify_grand_product_batch_device(dev.d, n, batch, *got[1:6], products=products)
            assert accept.all() and not layer.any() and not rnd.any() and not check.any(), (n, batch, kinds)
            assert np.array_equal(out, want[0])
    if "upper_zero" in kinds:                                      # every vector [0] with length 1, on the device as in the model
        b = kinds.index("upper_zero")
        assert (got[3][b] == 1).all() and not got[2][b].any() and not got[1][b].any() and not got[0][b].any()


# ---- c. every layer is the existing zero-check call on that level ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(14, 2), (16, 1)])
def test_layers_are_byte_equal_to_direct_zerocheck_calls(ctx, n, batch):
    size, total = 1 << n, batch * ((1 << n) - 1)
    d, lay = ctx.alloc(32 * batch * size), ctx.alloc(32 * total)
    try:
        ctx.fill_table(d, batch << n, 1600 + n)
        P8, H, C, L, R, E, Z, K = ctx.grand_product_batch_device(d, n, batch)
        assert N.lib().gkr_devtest_grand_product_tree(ctx._h, d, n, batch, lay) == N.GKR_OK
        for b in range(batch):
            table = np.array(from_limbs(ctx.download(_ptr_at(d, b << n), (size, 4))), dtype=object)
            levels = product_tree_np(table, n)
            assert from_limbs(P8[b:b + 1]) == [int(levels[0][0])] and from_limbs(H[b]) == [int(x) for x in levels[2]], b
        zs = []
        for b in range(batch):
            z1 = multi_hash(from_limbs(H[b]), 0)
            zs.append([z1, multi_hash([z1], 0)])
        for k in range(2, n):
            row = layer_row(k)
            src = d if k + 1 == n else _ptr_at(lay, _level_offset(k + 1, batch))
            Ck, Lk, Rk, Ek, Qk = ctx.sumcheck_zerocheck_batch_device(src, k, 2, TERMS, batch, zs)
            assert Ck.tobytes() == C[:, row:row + k].tobytes() and Lk.tobytes() == L[:, row:row + k].tobytes(), k
            assert Rk.tobytes() == R[:, row:row + k].tobytes() and Ek.tobytes() == E[:, k - 2].tobytes(), k
            nxt, claims = [], []
            for b in range(batch):
                rs, (a, bb) = from_limbs(Rk[b]), from_limbs(Ek[b])
                assert from_limbs(Qk[b:b + 1]) == [eq_point(zs[b], rs)], (k, b)
                tau = multi_hash([a, bb], 0)
                nxt.append([tau] + rs)
                claims.append((a + tau * (bb - a)) % P)
            zs = nxt
        assert from_limbs(Z.reshape(-1, 4)) == [x for z in zs for x in z] and from_limbs(K) == claims
        accept, _, _, check, _ = ctx.verify_grand_product_batch_device(d, n, batch, H, C, L, R, E, products=P8)
        assert accept.all() and not check.any()
    finally:
        ctx.free(d)
        ctx.free(lay)


# ---- d. the verifier ------------------------------------------------------------------------------------------------------------------------
def _raw(values):
    return np.array([limbs(v) for v in values], dtype=np.uint64).reshape(len(values), 4)


def _batch_of(n, cases):
    """cases: [(arrays, table, product)] of Python integers (not reduced) -> (T, products, H, C, L, R, E) limb arrays."""
    B, R = len(cases), rounds(n)
    return (_raw([x for _, t, _ in cases for x in t]).reshape(B, 1 << n, 4), _raw([p for _, _, p in cases]),
            _raw([x for a, _, _ in cases for x in a[0]]).reshape(B, 4, 4), _raw([x for a, _, _ in cases for row in a[1] for x in row]).reshape(B, R, 4, 4),
            np.array([a[2] for a, _, _ in cases], dtype=np.int64).astype(np.uint32).reshape(B, R), _raw([x for a, _, _ in cases for x in a[3]]).reshape(B, R, 4),
            _raw([x for a, _, _ in cases for e in a[4] for x in e]).reshape(B, n - 2, 2, 4))


@pytest.mark.parametrize("n", [4, 5])
def test_tamper_sweep_in_one_batch_under_both_hash_sides(ctx, n):
    """Every single-element change of the host sweep, of every kind of table, as ONE batch with an honest proof in front of and
    behind each table's changes; with claimed products and without; the round vectors hashed on the host threads and on the
    device.  Also a proof made from another table (EVALUATION) -- and, in the sweep itself, a wrong claimed product (PRODUCT)."""
    for with_product in (True, False):
        cases, want, names = [], [], []
        for kind in KINDS:
            table, g = _table(n, kind), _model(n, kind)
            arrays = proof_arrays(g, n)
            honest = (arrays, table, g["product"])
            sweep = tamperings(g, n, with_product, True)
            cases += [honest] + [apply(what, arrays, table, g["product"]) for _, what, _ in sweep] + [honest]
            want += [(0, 0, 0)] + [w for _, _, w in sweep] + [(0, 0, 0)]
            names += [(kind, "honest")] + [(kind, name) for name, _, _ in sweep] + [(kind, "honest")]
        cases.append((proof_arrays(_model(n, "random"), n), _table(n, "one_zero"), _model(n, "random")["product"]))
        want.append((EVALUATION, n, n))
        names.append(("random", "the proof of another table"))
        assert {w[0] for w in want} >= {0, SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION} | ({PRODUCT} if with_product else set())
        T, products, H, C, L, R, E = _batch_of(n, cases)
        with Resident(ctx, T) as dev:
            try:
                for hash_min in (-1, 1):
                    ctx.set_option("verify_device_hash_min", hash_min)
                    accept, layer, rnd, check, out = ctx.verify_grand_product_batch_device(dev.d, n, len(cases), H, C, L, R, E,
                                                                                           products=products if with_product else None)
                    got = [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]
                    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
                    assert diff is None, (n, with_product, hash_min, names[diff], got[diff], want[diff])
                    assert list(accept) == [w == (0, 0, 0) for w in want]
            finally:
                ctx.set_option("verify_device_hash_min", 0)


def test_elements_outside_the_field_and_the_order_of_the_form_checks(ctx):
    """r itself in every kind of element (an unused slot included: never read), one proof per case in one batch, the verdicts those of
    the integer model; out_products is zero exactly for the proofs that fail SHAPE or NON_CANONICAL."""
    n = 5
    table, g = _table(n, "random"), _model(n, "random")
    arrays = proof_arrays(g, n)
    short = next(row for row in range(rounds(n)) if arrays[2][row] < 4) if any(v < 4 for v in arrays[2]) else None

    def changed(**kw):
        head, C, L, R, E = list(arrays[0]), [list(c) for c in arrays[1]], list(arrays[2]), list(arrays[3]), [list(e) for e in arrays[4]]
        product = kw.pop("product", g["product"])
        for key, (at, v) in kw.items():
            if key == "head":
                head[at] = v
            elif key == "slot":
                C[at[0]][at[1]] = v
            elif key == "length":
                L[at] = v
            elif key == "r":
                R[at] = v
            else:
                E[at[0]][at[1]] = v
        return (head, C, L, R, E), table, product

    cases = [changed(), changed(head=(2, P)), changed(product=P)]
    for k in range(2, n):
        for j in range(k):
            cases += [changed(slot=((layer_row(k) + j, 3), P)), changed(r=(layer_row(k) + j, P + 5))]
        cases += [changed(value=((k - 2, 0), P)), changed(value=((k - 2, 1), (1 << 256) - 1))]
    cases += [changed(length=(rounds(n) - 1, 5), value=((0, 0), P)), changed(r=(rounds(n) - 1, P), value=((0, 0), P)),
              changed(r=(rounds(n) - 1, P), product=(g["product"] + 1) % P), changed(r=(0, (arrays[3][0] + 1) % P), product=(g["product"] + 1) % P),
              changed(length=(0, 0)), changed(length=(3, 77))]
    if short is not None:
        cases.append(changed(slot=((short, 0), P)))
    want = [model_verdict(a[0], layers_of(a, n), t, p) for a, t, p in cases]
    assert want[0] == (0, 0, 0) and want[1] == (NON_CANONICAL, 0, 0) == want[2] and want[-3 if short is not None else -2][0] == SHAPE
    assert (PRODUCT, 0, 0) in want and (NON_CANONICAL, n - 1, n - 1) in want and (short is None or want[-1] == (0, 0, 0))
    T, products, H, C, L, R, E = _batch_of(n, cases)
    with Resident(ctx, T) as dev:
        accept, layer, rnd, check, out = ctx.verify_grand_product_batch_device(dev.d, n, len(cases), H, C, L, R, E, products=products)
    assert [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)] == want
    form = np.array([w[0] in (SHAPE, NON_CANONICAL) for w in want])
    assert not out[form].any() and (out[~form] == to_limbs([g["product"]])[0]).all()


# ---- e. one size case -----------------------------------------------------------------------------------------------------------------------
def test_two_to_the_twenty(ctx):
    """n = 20, batch 1: 189 rounds over 18 layers; the device verifier accepts, P is the product of the downloaded table's Python
    integers, and one changed table entry is an EVALUATION failure."""
    n = 20
    d = ctx.alloc(32 << n)
    try:
        ctx.fill_table(d, 1 << n, 2020)
        out = ctx.grand_product_batch_device(d, n, 1)
        assert rounds(n) == 189 == out[2].shape[1]
        table = np.array(from_limbs(ctx.download(d, (1 << n, 4))), dtype=object)
        assert from_limbs(out[0]) == [int(product_tree_np(table, n)[0][0])]
        accept, layer, rnd, check, prod = ctx.verify_grand_product_batch_device(d, n, 1, *out[1:6], products=out[0])
        assert accept[0] and check[0] == 0 and np.array_equal(prod, out[0])
        ctx.upload(_ptr_at(d, 12345), to_limbs([int(table[12345]) + 1]))
        accept, layer, rnd, check, _ = ctx.verify_grand_product_batch_device(d, n, 1, *out[1:6], products=out[0])
        assert (bool(accept[0]), int(check[0]), int(layer[0]), int(rnd[0])) == (False, EVALUATION, n, n)
    finally:
        ctx.free(d)


# ---- f. context hygiene ---------------------------------------------------------------------------------------------------------------------
def test_a_zerocheck_is_unaffected_by_a_grand_product_on_the_same_context():
    n, batch, terms = 10, 3, [(1, (0, 1)), (P - 1, (2,))]
    rng = np.random.default_rng(99)
    Z = [[int(x) for x in rng.integers(1, 1 << 62, size=n)] for _ in range(batch)]
    with Context(0) as c:
        d, g = c.alloc(32 * batch * 3 << n), c.alloc(32 * batch << n)
        try:
            c.fill_table(d, batch * 3 << n, 11)
            c.fill_table(g, batch << n, 12)
            before = c.sumcheck_zerocheck_batch_device(d, n, 3, terms, batch, Z)
            first = c.grand_product_batch_device(g, n, batch)
            after = c.sumcheck_zerocheck_batch_device(d, n, 3, terms, batch, Z)
            again = c.grand_product_batch_device(g, n, batch)
        finally:
            c.free(d)
            c.free(g)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


# ---- g. the host-table forms ----------------------------------------------------------------------------------------------------------------
def test_host_table_forms(ctx):
    n = 5
    for kind in ("random", "one_zero"):
        table, g = _table(n, kind), _model(n, kind)
        product, head, layers, point, claim = ctx.prove_grand_product(table, n)
        assert (product, head, layers, point, claim) == (g["product"], g["head"], g["layers"], g["point"], g["claim"]), kind
        assert ctx.verify_grand_product(table, head, layers, product) == (0, 0, 0) == ctx.verify_grand_product(table, head, layers)
        assert ctx.verify_grand_product(table, head, layers, (product + 1) % P) == (PRODUCT, 0, 0)
        other = list(table)
        other[7] = (other[7] + 1) % P
        assert ctx.verify_grand_product(other, head, layers, product) == (EVALUATION, n, n)
        proof, r, ab = layers[1]
        bad = layers[:1] + [(proof, r, ((ab[0] + 1) % P, ab[1]))] + layers[2:]
        assert ctx.verify_grand_product(table, head, bad, product) == model_verdict(head, bad, table, product) == (FINAL_CLAIM, 3, 3)
    raw = np.ascontiguousarray(to_limbs(_table(n, "random")))
    raw[9] = R_LIMBS
    with pytest.raises(GkrError) as e:
        ctx.prove_grand_product(raw, n)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL

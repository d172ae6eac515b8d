"""gkr_fraction_sum_batch_device and its verifier (csrc/kernels_fraction_sum.hip, csrc/capi_fraction_sum.hip) on the device:

  a. the tree alone (gkr_devtest_fraction_sum_tree) bit for bit against Python integers, every level, at n = 3, 4, 5 with batches
     of 1 and 3 and on either side of the first two-block launch (n = 9, 10) with batch 2, the launch geometry asserted first;
     canaries around the caller's buffer; one pair 4 GiB into the tables allocation;
  b. the whole call against the integer model (tests/fraction_sum_model.py), every output byte, n = 3 .. 8 x all kinds x batch 1
     and 3, a batch member against the same pair proved alone (the per-proof lambda), and the verifier on what was proved;
  c. the multi-block sizes n = 17 with batch 1 and 20: the geometries asserted, the tree against numpy integers, the head and the
     chain against the model's host steps, EVERY layer byte-equal to a direct gkr_sumcheck_zerocheck_batch_device call with batch 1
     on that pair's level with that pair's lambda_k and z^(k), the end claims against the numpy extension;
  d. the device verifier: the host sweep's tampered proofs at n = 4 and 5 in ONE batch per size under both hash sides against the
     closed-form verdicts (tests/fraction_sum_sweeps.py); three chunks for a batch of 7 with a tampered proof in each chunk and at
     each chunk edge; claimed sums given, absent and wrong; a zero denominator; out_sums;
  e. one context for a zero-check, a grand product and a fractional sum, interleaved;  f. the host-table forms.

The library's own output is never the reference of a verdict or a value."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, FRACTION_SUM, KINDS, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR,
                                eq_point, fraction_sum, fraction_tree_np, head_chain, head_root, layer_row, layer_terms, make_tables, mle_np,
                                model_verdict, next_chain, proof_arrays, rounds)
from fraction_sum_sweeps import ACCEPTED, apply, check_inputs, layers_of, tamperings
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from resident_tables import Resident
from test_fraction_sum_host import tree_geometry
from verify_sweeps import R_LIMBS, limbs

pytestmark = pytest.mark.gpu

# blocks of 256 threads per pair of the launch of level k = 0 .. n - 1 (a thread per node): n = 9 is the last size whose every
# launch is one block, n = 10 the first whose top launch has two
GEOMETRY = {3: [1] * 3, 4: [1] * 4, 5: [1] * 5, 9: [1] * 9, 10: [1] * 9 + [2]}
CANARY = np.array([0xC0DEC0DEC0DEC0DE, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_pairs, _models = {}, {}


def _pair(n, kind):
    """One pair (N, D) per (n, kind), the same in every test."""
    if (n, kind) not in _pairs:
        _pairs[(n, kind)] = make_tables(kind, n, random.Random(9000 + 37 * n + KINDS.index(kind)))
    return _pairs[(n, kind)]


def _model(n, kind):
    if (n, kind) not in _models:
        num, den = _pair(n, kind)
        _models[(n, kind)] = fraction_sum(np.array(num, dtype=object), np.array(den, dtype=object), n, use_np=True)
    return _models[(n, kind)]


def _level_offset(k, batch, b=0):
    return 2 * batch * ((1 << k) - 1) + (b << (k + 1))


def _ptr_at(d, elements):
    return ctypes.c_void_p(d.value + 32 * elements)


def _pair_limbs(pairs, n):
    """[(N, D)] -> (batch, 2, 2^n, 4) limbs: the device's layout."""
    return to_limbs([x for num, den in pairs for x in list(num) + list(den)]).reshape(len(pairs), 2, 1 << n, 4)


def _assert_levels(got, pairs, n, batch, pad=0):
    for b, (num, den) in enumerate(pairs):
        levels = fraction_tree_np(np.array(num, dtype=object), np.array(den, dtype=object), n)
        for k in range(n):
            at = pad + _level_offset(k, batch, b)
            assert from_limbs(got[at:at + (2 << k)]) == [int(x) for x in levels[k][0]] + [int(x) for x in levels[k][1]], (n, batch, b, k)


# ---- a. the tree alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(3, 1), (3, 3), (4, 1), (4, 3), (5, 1), (5, 3), (9, 2), (10, 2)])
def test_tree_matches_python_integers_at_every_level(ctx, n, batch):
    assert tree_geometry(n) == GEOMETRY[n], n
    kinds = (["all_max", "random", "one_zero_denominator"] if n % 2 else ["random", "all_max", "lookup"])[:batch]
    pairs = [_pair(n, kind) for kind in kinds]
    total, pad = 2 * batch * ((1 << n) - 1), 64
    with Resident(ctx, _pair_limbs(pairs, n)) as dev, Resident(ctx, np.tile(CANARY, (total + 2 * pad, 1))) as lay:
        rc = N.lib().gkr_devtest_fraction_sum_tree(ctx._h, dev.d, n, batch, _ptr_at(lay.d, pad))
        assert rc == N.GKR_OK, rc
        dev.assert_unchanged((n, batch))
        got = ctx.download(lay.d, (total + 2 * pad, 4))
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all(), "canaries around the levels"
    _assert_levels(got, pairs, n, batch, pad)


def test_tree_with_a_pair_four_gib_into_the_tables_allocation(ctx):
    """n = 10: the pair starts at byte 2^32 of its allocation; every offset is formed in 64 bits."""
    n, pad = 10, 64
    pair = _pair(n, "random")
    total = 2 * ((1 << n) - 1)
    d, lay = ctx.alloc((1 << 32) + (64 << n)), ctx.alloc(32 * (total + 2 * pad))
    try:
        at = ctypes.c_void_p(d.value + (1 << 32))
        ctx.upload(at, _pair_limbs([pair], n))
        ctx.upload(lay, np.tile(CANARY, (total + 2 * pad, 1)))
        assert N.lib().gkr_devtest_fraction_sum_tree(ctx._h, at, n, 1, _ptr_at(lay, pad)) == N.GKR_OK
        got = ctx.download(lay, (total + 2 * pad, 4))
    finally:
        ctx.free(d)
        ctx.free(lay)
    assert (got[:pad] == CANARY).all() and (got[pad + total:] == CANARY).all()
    _assert_levels(got, [pair], n, 1, pad)


# ---- b. the whole call against the model --------------------------------------------------------------------------------------------------
NAMES = ("sums", "head", "coefficients", "lengths", "challenges", "values", "point", "claims")


def _model_arrays(n, kinds):
    """The model's proofs of the pairs (n, kind) as the eight arrays of Context.fraction_sum_batch_device."""
    gs = [_model(n, kind) for kind in kinds]
    arrs = [proof_arrays(g, n) for g in gs]
    B, R = len(kinds), rounds(n)
    return (to_limbs([x for g in gs for x in g["sums"]]).reshape(B, 2, 4), to_limbs([x for a in arrs for x in a[0]]).reshape(B, 8, 4),
            to_limbs([x for a in arrs for row in a[1] for x in row]).reshape(B, R, 4, 4), np.array([a[2] for a in arrs], dtype=np.uint32).reshape(B, R),
            to_limbs([x for a in arrs for x in a[3]]).reshape(B, R, 4), to_limbs([x for a in arrs for e in a[4] for x in e]).reshape(B, n - 2, 4, 4),
            to_limbs([x for g in gs for x in g["point"]]).reshape(B, n, 4), to_limbs([x for g in gs for x in g["claim"]]).reshape(B, 2, 4))


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = tuple(int(x) for x in np.argwhere(g != w)[0])
            pytest.fail("%s: %s differ first at %s: got %s, want %s" % (what, name, at, g[at[:-1]], w[at[:-1]]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [3, 4, 5, 6, 7, 8])
def test_whole_call_matches_the_model_and_is_verified(ctx, n, kind):
    """Batch 1, then batch 3 with this pair in front of two pairs of other kinds: every output byte the model's; member 0 of the
    batch byte-equal to the pair proved alone (a coefficient shared by the batch fails here: every proof has a lambda of its own);
    the verifier accepts what was proved -- and rejects a zero denominator, which the prover proves all the same."""
    i = KINDS.index(kind)
    alone = None
    for kinds in ([kind], [kind, KINDS[(i + 1) % 5], KINDS[(i + 3) % 5]]):
        batch = len(kinds)
        want = _model_arrays(n, kinds)
        with Resident(ctx, _pair_limbs([_pair(n, k) for k in kinds], n)) as dev:
            got = ctx.fraction_sum_batch_device(dev.d, n, batch)
            dev.assert_unchanged((n, kinds))
            _assert_same(got, want, (n, kinds))
            verdicts = [(ZERO_DENOMINATOR, 0, 0) if k == "one_zero_denominator" else ACCEPTED for k in kinds]
            for sums in (got[0], None):
                accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(dev.d, n, batch, *got[1:6], sums=sums)
                assert [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)] == verdicts, (n, kinds)
                assert list(accept) == [v == ACCEPTED for v in verdicts] and np.array_equal(out, want[0])
        if alone is None:
            alone = got
        else:
            assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(alone, got)), "a batch member against the pair proved alone"
    if kind == "lookup":
        assert not got[0][0, 0].any() and got[0][0, 1].any()       # P = 0, Q != 0: the lookup holds


# ---- c. multi-block sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,pairs", [(1, (0,)), (20, (0, 9, 19))])
def test_multi_block_layers_are_byte_equal_to_direct_zerocheck_calls(ctx, batch, pairs):
    """n = 17: the top layer k = 16 runs 128 blocks per sumcheck at batch 1 (the round kernel's wave loop makes two full trips) and
    103 blocks with a chunk of 512 at batch 20.  The Python model is too slow here and the zero-check is pinned to its C oracle, so:
    the tree against numpy integers, the head and the chain against the model's host steps, every layer of the pairs `pairs`
    against the direct zero-check call on that pair's level, the end claims against the numpy extension."""
    n = 17
    assert tuple(product_geometry(16, batch)[:2]) == PRODUCT_GEOMETRY[(16, batch)]
    size, total = 2 << n, 2 * batch * ((1 << n) - 1)
    d, lay = ctx.alloc(32 * batch * size), ctx.alloc(32 * total)
    try:
        ctx.fill_table(d, batch * size, 1700 + batch)
        S, H, C, L, R, E, Z, K = ctx.fraction_sum_batch_device(d, n, batch)
        assert N.lib().gkr_devtest_fraction_sum_tree(ctx._h, d, n, batch, lay) == N.GKR_OK
        for b in pairs:
            T = ctx.download(_ptr_at(d, b * size), (size, 4))
            num, den = (np.array(from_limbs(T[h << n:(h + 1) << n]), dtype=object) for h in (0, 1))
            levels = fraction_tree_np(num, den, n)
            for k in range(n):
                got = from_limbs(ctx.download(_ptr_at(lay, _level_offset(k, batch, b)), (2 << k, 4)))
                assert got == [int(x) for x in levels[k][0]] + [int(x) for x in levels[k][1]], (b, k)
            head = from_limbs(H[b])
            assert head == [int(x) for x in levels[2][0]] + [int(x) for x in levels[2][1]] and tuple(from_limbs(S[b])) == head_root(head), b
            z, lam, cp, cq = head_chain(head)
            for k in range(2, n):
                row = layer_row(k)
                src = _ptr_at(d, b * size) if k + 1 == n else _ptr_at(lay, _level_offset(k + 1, batch, b))
                Ck, Lk, Rk, Ek, Qk = ctx.sumcheck_zerocheck_batch_device(src, k, 4, layer_terms(lam), 1, [z])
                assert Ck[0].tobytes() == C[b, row:row + k].tobytes() and Lk[0].tobytes() == L[b, row:row + k].tobytes(), (b, k)
                assert Rk[0].tobytes() == R[b, row:row + k].tobytes() and Ek[0].tobytes() == E[b, k - 2].tobytes(), (b, k)
                rs, vals = from_limbs(Rk[0]), from_limbs(Ek[0])
                assert from_limbs(Qk) == [eq_point(z, rs)], (b, k)
                z, lam, cp, cq = next_chain(vals, rs)
            assert from_limbs(Z[b]) == z and from_limbs(K[b]) == [cp, cq], b
            assert (cp, cq) == (mle_np(num, z), mle_np(den, z)), b
        accept, _, _, check, out = ctx.verify_fraction_sum_batch_device(d, n, batch, H, C, L, R, E, sums=S)
        assert accept.all() and not check.any() and np.array_equal(out, S)
    finally:
        ctx.free(d)
        ctx.free(lay)


# ---- d. the verifier ------------------------------------------------------------------------------------------------------------------------
def _raw(values):
    return np.array([limbs(v) for v in values], dtype=np.uint64).reshape(len(values), 4)


def _batch_of(n, cases):
    """cases: [(arrays, num, den, sums)] of Python integers (not reduced) -> (T, sums, H, C, L, R, E) limb arrays."""
    B, R = len(cases), rounds(n)
    return (_raw([x for _, num, den, _ in cases for x in list(num) + list(den)]).reshape(B, 2, 1 << n, 4),
            _raw([x for _, _, _, s in cases for x in s]).reshape(B, 2, 4), _raw([x for a, _, _, _ in cases for x in a[0]]).reshape(B, 8, 4),
            _raw([x for a, _, _, _ in cases for row in a[1] for x in row]).reshape(B, R, 4, 4),
            np.array([a[2] for a, _, _, _ in cases], dtype=np.int64).astype(np.uint32).reshape(B, R),
            _raw([x for a, _, _, _ in cases for x in a[3]]).reshape(B, R, 4), _raw([x for a, _, _, _ in cases for e in a[4] for x in e]).reshape(B, n - 2, 4, 4))


def _verdicts(check, layer, rnd):
    return [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]


@pytest.mark.parametrize("n", [4, 5])
def test_tamper_sweep_in_one_batch_under_both_hash_sides(ctx, n):
    """Every single-element change of the host sweep as ONE batch with an honest proof in front and behind, with claimed sums and
    without; the round vectors hashed on the device (verify_device_hash_min = 1) and on the host threads (a value above the row
    count).  out_sums is zero exactly for the proofs that fail SHAPE or NON_CANONICAL."""
    num, den, g = _pair(n, "random") + (_model(n, "random"),)
    check_inputs(g, n, num, den)
    arrays = proof_arrays(g, n)
    honest = (arrays, num, den, list(g["sums"]))
    for with_sums in (True, False):
        sweep = tamperings(g, n, with_sums, True)
        cases = [honest] + [apply(what, arrays, num, den, g["sums"]) for _, what, _ in sweep] + [honest]
        want = [ACCEPTED] + [w for _, _, w in sweep] + [ACCEPTED]
        names = ["honest"] + [name for name, _, _ in sweep] + ["honest"]
        assert {w[0] for w in want} >= {0, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION} | ({FRACTION_SUM} if with_sums else set())
        T, sums, H, C, L, R, E = _batch_of(n, cases)
        with Resident(ctx, T) as dev:
            try:
                for hash_min in (1, len(cases) * rounds(n) + 1):
                    ctx.set_option("verify_device_hash_min", hash_min)
                    accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(dev.d, n, len(cases), H, C, L, R, E,
                                                                                          sums=sums if with_sums else None)
                    got = _verdicts(check, layer, rnd)
                    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
                    assert diff is None, (n, with_sums, hash_min, names[diff], got[diff], want[diff])
                    assert list(accept) == [w == ACCEPTED for w in want]
                    form = np.array([w[0] in (SHAPE, NON_CANONICAL) for w in want])
                    roots = to_limbs([x for (a, _, _, _), f in zip(cases, form) if not f for x in head_root([v % P for v in a[0]])]).reshape(-1, 2, 4)
                    assert not out[form].any() and np.array_equal(out[~form], roots)
            finally:
                ctx.set_option("verify_device_hash_min", 0)


def test_three_chunks_with_a_tampered_proof_in_each_and_at_each_edge(ctx):
    """verify_workspace_mb = 1 at n = 23 holds three proofs per chunk (asserted first): a batch of 7 runs as chunks of 3, 3 and 1.
    Device-proved proofs; one element changed in proofs 0, 2, 3, 5 and 6 -- both edges of both full chunks and the ragged last
    one -- each with the verdict of its position's rule; proofs 1 and 4 stay honest.  The same verdicts in one chunk."""
    n, batch = 23, 7
    size = 2 << n
    d = ctx.alloc(32 * batch * size)
    try:
        ctx.fill_table(d, batch * size, 2323)
        S, H, C, L, R, E, Z, K = ctx.fraction_sum_batch_device(d, n, batch)
        assert (L == 4).all()                                      # every slot is used
        assert from_limbs(E[5, 9 - 2])[3] != 0                     # the cofactor of the value changed below: b1 of proof 5, layer 9
        H, C, L, R, E = (a.copy() for a in (H, C, L, R, E))
        want = [ACCEPTED] * batch
        row = layer_row(11) + 4
        R[0, row] = to_limbs([(from_limbs(R[0, row:row + 1])[0] + 1) % P])[0]
        want[0] = (CHALLENGE, 11, 4)
        C[2, row, 2] = to_limbs([(from_limbs(C[2, row, 2:3])[0] + 1) % P])[0]
        want[2] = (ROUND_SUM, 11, 4)
        L[3, layer_row(22) + 21] = 5
        want[3] = (SHAPE, 22, 21)
        E[5, 9 - 2, 0] = to_limbs([(from_limbs(E[5, 9 - 2, 0:1])[0] + 1) % P])[0]
        want[5] = (FINAL_CLAIM, 9, 9)
        H[6, 7] = R_LIMBS
        want[6] = (NON_CANONICAL, 0, 0)
        out = np.zeros(1, dtype=np.uint32)
        try:
            for mb, chunk in ((1, 3), (0, batch)):
                ctx.set_option("verify_workspace_mb", mb)
                assert N.lib().gkr_devtest_fraction_sum_chunk(ctx._h, n, batch, out.ctypes.data) == N.GKR_OK and out[0] == chunk, (mb, out[0])
                accept, layer, rnd, check, sums = ctx.verify_fraction_sum_batch_device(d, n, batch, H, C, L, R, E, sums=S)
                assert _verdicts(check, layer, rnd) == want, mb
                assert list(accept) == [w == ACCEPTED for w in want]
                assert np.array_equal(sums[:3], S[:3]) and np.array_equal(sums[4:6], S[4:6]) and not sums[3].any() and not sums[6].any()
        finally:
            ctx.set_option("verify_workspace_mb", 0)
    finally:
        ctx.free(d)


def test_claimed_sums_given_absent_and_wrong_and_a_zero_denominator(ctx):
    n = 5
    kinds = ["random", "lookup", "one_zero_denominator", "random", "random", "zero_numerators"]
    gs = [_model(n, k) for k in kinds]
    cases = [(proof_arrays(g, n),) + _pair(n, k) + (list(g["sums"]),) for g, k in zip(gs, kinds)]
    cases[3][3][0] = (cases[3][3][0] + 1) % P                      # a wrong P
    cases[4][3][1] = (cases[4][3][1] + 1) % P                      # a wrong Q
    cases[2][3][0] = (cases[2][3][0] + 1) % P                      # Q = 0 is reported before a wrong claim
    want = [ACCEPTED, ACCEPTED, (ZERO_DENOMINATOR, 0, 0), (FRACTION_SUM, 0, 0), (FRACTION_SUM, 0, 0), ACCEPTED]
    assert want == [model_verdict(a[0], layers_of(a, n), num, den, s) for a, num, den, s in cases]
    T, sums, H, C, L, R, E = _batch_of(n, cases)
    roots = to_limbs([x for g in gs for x in g["sums"]]).reshape(len(kinds), 2, 4)
    with Resident(ctx, T) as dev:
        accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(dev.d, n, len(cases), H, C, L, R, E, sums=sums)
        assert _verdicts(check, layer, rnd) == want and np.array_equal(out, roots)
        accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(dev.d, n, len(cases), H, C, L, R, E, sums=None)
        assert _verdicts(check, layer, rnd) == [ACCEPTED, ACCEPTED, (ZERO_DENOMINATOR, 0, 0)] + [ACCEPTED] * 3 and np.array_equal(out, roots)
        assert list(accept) == [True, True, False, True, True, True]
        # the proof of another pair: the chain holds, the evaluation does not
        other = _batch_of(n, [(cases[0][0],) + _pair(n, "lookup") + (cases[0][3],)])
    with Resident(ctx, other[0]) as dev:
        accept, layer, rnd, check, out = ctx.verify_fraction_sum_batch_device(dev.d, n, 1, *other[2:], sums=other[1])
        assert _verdicts(check, layer, rnd) == [(EVALUATION, n, n)] and not accept[0]


# ---- e. context isolation -----------------------------------------------------------------------------------------------------------------
def test_a_zerocheck_a_grand_product_and_a_fraction_sum_share_one_context():
    """Interleaved on one context, each call is byte-equal to its run on a fresh context."""
    n, batch, terms = 10, 3, [(1, (0, 1)), (P - 1, (2,))]
    rng = np.random.default_rng(101)
    Z = [[int(x) for x in rng.integers(1, 1 << 62, size=n)] for _ in range(batch)]

    def run(c, which):
        d = c.alloc(32 * batch * 3 << n)
        try:
            out = {}
            for w in which:
                c.fill_table(d, batch * 3 << n, 11 + "zgf".index(w))
                if w == "z":
                    out[w] = c.sumcheck_zerocheck_batch_device(d, n, 3, terms, batch, Z)
                elif w == "g":
                    out[w] = c.grand_product_batch_device(d, n, batch)
                else:
                    out[w] = c.fraction_sum_batch_device(d, n, batch)
            return out
        finally:
            c.free(d)

    fresh = {}
    for w in "zgf":
        with Context(0) as c:
            fresh.update(run(c, w))
    with Context(0) as c:
        for order in ("zgf", "fzg", "gfz"):
            got = run(c, order)
            for w in order:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[w], fresh[w])), (order, w)


# ---- f. the host-table forms ----------------------------------------------------------------------------------------------------------------
def test_host_table_forms(ctx):
    n = 5
    for kind in ("random", "lookup"):
        (num, den), g = _pair(n, kind), _model(n, kind)
        sums, head, layers, point, claims = ctx.prove_fraction_sum(num, den, n)
        assert (sums, head, layers, point, claims) == (g["sums"], g["head"], g["layers"], g["point"], g["claim"]), kind
        assert ctx.verify_fraction_sum(num, den, head, layers, sums) == ACCEPTED == ctx.verify_fraction_sum(num, den, head, layers)
        assert ctx.verify_fraction_sum(num, den, head, layers, (sums[0], (sums[1] + 1) % P)) == (FRACTION_SUM, 0, 0)
        other = list(den)
        other[7] = (other[7] + 1) % P
        assert ctx.verify_fraction_sum(num, other, head, layers, sums) == (EVALUATION, n, n)
        proof, r, vals = layers[1]
        bad = layers[:1] + [(proof, r, (vals[0], vals[1], (vals[2] + 1) % P, vals[3]))] + layers[2:]
        assert ctx.verify_fraction_sum(num, den, head, bad, sums) == model_verdict(head, bad, num, den, sums) == (FINAL_CLAIM, 3, 3)
    (num, den), g = _pair(n, "one_zero_denominator"), _model(n, "one_zero_denominator")
    sums, head, layers, _, _ = ctx.prove_fraction_sum(num, den, n)
    assert sums == g["sums"] and sums[1] == 0 and ctx.verify_fraction_sum(num, den, head, layers, sums) == (ZERO_DENOMINATOR, 0, 0)
    raw = np.ascontiguousarray(to_limbs(_pair(n, "random")[1]))
    raw[9] = R_LIMBS
    with pytest.raises(GkrError) as e:
        ctx.prove_fraction_sum(_pair(n, "random")[0], raw, n)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL

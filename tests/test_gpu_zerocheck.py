"""gkr_sumcheck_zerocheck_batch_device / gkr_sumcheck_zerocheck / gkr_eq_table_device (csrc/kernels_zerocheck.hip,
csrc/capi_zerocheck.hip) through the C ABI, bit-exact against the implicit integer model of tests/zerocheck_model.py -- which
tests/test_zerocheck_host.py holds against the sum-of-products model on the materialised eq table and against the reference's own
eq(AB-C) fixtures -- and byte for byte against gkr_sumcheck_sop_batch_device on the tables plus the device-built eq table.

  a. the shape matrix against the model: n x the five structures x batch, a point of its own per sumcheck, inputs unmodified;
  b. byte equality with the SOP path on the device, the multi-block geometries included;
  c. gkr_eq_table_device alone: both kernels of launch_eq_table, strided output, the gaps untouched;
  d. special points and inputs: boolean z, a satisfied zero-check, cancelling terms, coefficients 0, 1, r - 1;
  e. the batch limit and offsets past 4 GiB;
  f. the transcripts through gkr_sumcheck_sop_verify_batch_device;
  g. one context for the plain, the product, the SOP and this path.

n = 8 .. 10 straddle the weight split: with eight free variables or fewer a round takes E_hi = [1] and a short E_lo, from nine on
E_hi has 2^(free - 8) entries (round 1 has n - 1 free variables, so n = 9 is the last shape without and n = 10 the first with an
E_hi table in round 1; every larger n passes through the change of form on its way down)."""

import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import mle_eval, verify_sumcheck_zerocheck
from oracle.mimc7 import multi_hash
from product_model import factor
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from sop_model import STRUCTURES, limbs_to_object
from zerocheck_model import (eq_table, eq_table_np, lift_terms, zc_degree, zerocheck_claim_np, zerocheck_sumcheck,
                             zerocheck_sumcheck_np)

pytestmark = pytest.mark.gpu

SHAPE_N = [2, 3, 5, 8, 9, 10, 11, 13]
ZC_STRUCTURES = [s for s in STRUCTURES if s[0] in ("AB-C", "5AB+7BC+11A", "AA+3B", "AB-AB", "AB-AC")]
MIX = ["random", "indep_first", "all_max", "indep_last", "specials", "bits", "indep_middle", "constant"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _structure(name):
    return next(s for s in STRUCTURES if s[0] == name)


def _decode(C, L, R, E, Q, b, D):
    n = L.shape[1]
    proof = [from_limbs(C[b, j])[D + 1 - int(L[b, j]):] for j in range(n)]
    assert all(not C[b, j, :D + 1 - int(L[b, j])].any() for j in range(n)), "unused slots hold zero"
    return proof, from_limbs(R[b]), from_limbs(E[b]), from_limbs(Q[b:b + 1])[0]


def _limbs(groups):
    return np.concatenate([to_limbs(t) for g in groups for t in g])


def _z_limbs(zs):
    return to_limbs([x for z in zs for x in z]).reshape(len(zs), len(zs[0]), 4)


def _run(ctx, groups, n, terms, zs):
    """groups[b][m]: table m of sumcheck b, zs[b] its point -> [(proof, r, evals, eq_r)]; the inputs are downloaded afterwards and
    must be what was uploaded."""
    T = _limbs(groups)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        out = ctx.sumcheck_zerocheck_batch_device(d, n, len(groups[0]), terms, len(groups), _z_limbs(zs))
        assert np.array_equal(ctx.download(d, T.shape), T), "the inputs are not modified"
    finally:
        ctx.free(d)
    return [_decode(*out, b, zc_degree(terms)) for b in range(len(groups))]


def _model(tables, terms, z, n):
    if n < 8:
        return zerocheck_sumcheck(tables, terms, z, n)
    return zerocheck_sumcheck_np(np.array(tables, dtype=object), terms, z, n)


def _random_limbs(rng, count):
    T = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    T[:, 3] &= np.uint64((1 << 60) - 1)                           # below 2^252: canonical
    return T


def _random_point(rng, n):
    return [rng.randrange(P) for _ in range(n)]


# ---- the reference's fixtures through both entry points ---------------------------------------------------------------------------------
def test_golden_fixtures_of_the_reference_python_prover(ctx):
    cases = [c for c in load_golden("sop_sumcheck.json")["cases"] if c["z"]]
    assert len(cases) == 2
    for c in cases:
        n, z = c["n"], [int(x) for x in c["z"]]
        tables = [[int(x) for x in t] for t in c["tables"]][1:]
        terms = [(int(k), tuple(i - 1 for i in idx[1:])) for k, idx in c["terms"]]
        want = ([[int(x) for x in g] for g in c["proof"]], [int(x) for x in c["r"]])
        proof, r, evals, eq_r = ctx.prove_zerocheck(tables, terms, z, n)              # the host form
        assert (proof, r) == want, n
        assert evals == [mle_eval(t, r) for t in tables] and eq_r == mle_eval(eq_table(z), r)
        assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, int(c["claim"]))
        assert _run(ctx, [tables], n, terms, [z]) == [(proof, r, evals, eq_r)]        # the resident form


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("structure", ZC_STRUCTURES, ids=[s[0] for s in ZC_STRUCTURES])
@pytest.mark.parametrize("n", SHAPE_N)
def test_shapes_match_the_model(ctx, n, structure, batch):
    name, n_tables, terms = structure
    rng = random.Random(7100 + 97 * n + 7 * len(name) + batch)
    groups = [[factor(MIX[(n + 3 * b + 5 * m + n_tables) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(batch)]
    zs = [_random_point(rng, n) for _ in range(batch)]
    assert len({tuple(z) for z in zs}) == batch
    assert _run(ctx, groups, n, terms, zs) == [_model(g, terms, z, n) for g, z in zip(groups, zs)]


# ---- b. byte equality with the SOP path on the device -----------------------------------------------------------------------------------
def _both_paths(ctx, T, n, terms, Z):
    """T: (batch, M, 2^n, 4) limbs, Z: (batch, n, 4) limbs -> (the SOP path's (C, L, R, E) on M + 1 tables per sumcheck with slot 0
    filled by gkr_eq_table_device and the lifted terms, the zero-check's (C, L, R, E, Q) on a copy of tables 1 .. M)."""
    batch, M = T.shape[:2]
    S = np.zeros((batch, M + 1, 1 << n, 4), dtype=np.uint64)
    S[:, 1:] = T
    d_s, d_t = ctx.alloc(S.nbytes), ctx.alloc(T.nbytes)
    try:
        ctx.upload(d_s, S)
        ctx.upload(d_t, T)
        ctx.eq_table_device(Z, n, batch, d_s, stride=(M + 1) << n)
        sop = ctx.sumcheck_sop_batch_device(d_s, n, M + 1, lift_terms(terms), batch)
        zc = ctx.sumcheck_zerocheck_batch_device(d_t, n, M, terms, batch, Z)
    finally:
        ctx.free(d_s)
        ctx.free(d_t)
    return sop, zc


def _assert_bytes_equal(sop, zc, where):
    for name, s, z in zip(("coeffs", "len", "r"), sop[:3], zc[:3]):
        assert s.shape == z.shape and s.dtype == z.dtype and s.tobytes() == z.tobytes(), (name, where)
    assert sop[3][:, 1:].tobytes() == zc[3].tobytes(), ("evals", where)
    assert sop[3][:, 0].tobytes() == zc[4].tobytes(), ("eq", where)


@pytest.mark.parametrize("structure", ZC_STRUCTURES, ids=[s[0] for s in ZC_STRUCTURES])
@pytest.mark.parametrize("n", SHAPE_N)
def test_bytes_equal_the_sop_path_with_the_device_built_eq_table(ctx, n, structure):
    name, n_tables, terms = structure
    batch = 3
    rng = random.Random(7300 + 89 * n + len(name))
    groups = [[factor(MIX[(n + 5 * b + 3 * m) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(batch)]
    zs = [_random_point(rng, n), [rng.randrange(2) for _ in range(n)], [(0, 1, rng.randrange(P))[(j + n) % 3] for j in range(n)]]
    sop, zc = _both_paths(ctx, _limbs(groups).reshape(batch, n_tables, 1 << n, 4), n, terms, _z_limbs(zs))
    _assert_bytes_equal(sop, zc, (n, name))


@pytest.mark.parametrize("n,batch,structure", [(16, 1, "AB-C"), (16, 20, "5AB+7BC+11A"), (20, 1, "AB-C")])
def test_bytes_equal_the_sop_path_at_multi_block_shapes(ctx, n, batch, structure):
    """(16, 1): 128 blocks; (16, 20): 103 blocks of which 64 work, chunk 512 (two trips of a thread's loop, two E_hi entries per
    block; the eq tables go through the staging buffer in two chunks); (20, 1): the cap of 2048 blocks (the eq table is written in
    place)."""
    assert tuple(product_geometry(n, batch)[:2]) == PRODUCT_GEOMETRY[(n, batch)]
    _, n_tables, terms = _structure(structure)
    g = np.random.default_rng(1700 + n + batch)
    T = _random_limbs(g, batch * n_tables << n).reshape(batch, n_tables, 1 << n, 4)
    Z = _random_limbs(g, batch * n).reshape(batch, n, 4)
    Z[0, 1], Z[0, n - 1] = 0, to_limbs([1])[0]                    # a zero and a one among the first point's entries
    sop, zc = _both_paths(ctx, T, n, terms, Z)
    _assert_bytes_equal(sop, zc, (n, batch))
    assert (zc[1] == zc_degree(terms) + 1).all()
    # the proven sum of the first and the last sumcheck, entry by entry
    for b in {0, batch - 1}:
        tables, z = limbs_to_object(T[b]), from_limbs(Z[b])
        proof, r, evals, eq_r = _decode(*zc, b, zc_degree(terms))
        assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, zerocheck_claim_np(tables, terms, z)), b
        eq_want = 1
        for zj, rj in zip(z, r):
            eq_want = eq_want * (zj * rj + (1 - zj) * (1 - rj)) % P
        assert eq_r == eq_want


# ---- c. gkr_eq_table_device alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 7, 13, 14, 16])
def test_eq_table_device(ctx, n):
    """Batch 3 with a stride above 2^n (the gaps keep what they held), then the dense layout.  n >= 14: k_eq_table_split."""
    batch, size = 3, 1 << n
    stride = size + 5
    rng = random.Random(7500 + n)
    zs = [_random_point(rng, n), [rng.randrange(2) for _ in range(n)], [(rng.randrange(P), 1, 0)[j % 3] for j in range(n)]]
    fill = np.full((batch * stride, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d = ctx.alloc(fill.nbytes)
    try:
        ctx.upload(d, fill)
        ctx.eq_table_device(zs, n, batch, d, stride=stride)
        strided = ctx.download(d, fill.shape).reshape(batch, stride, 4)
        ctx.upload(d, fill)
        ctx.eq_table_device(_z_limbs(zs), n, batch, d)
        dense = ctx.download(d, fill.shape)
    finally:
        ctx.free(d)
    assert (strided[:, size:] == fill[0]).all() and (dense[batch * size:] == fill[0]).all()
    assert np.array_equal(strided[:, :size].reshape(-1, 4), dense[:batch * size])
    for b, z in enumerate(zs):
        got = limbs_to_object(strided[b, :size])
        assert int(got.sum()) % P == 1
        if n < 16:
            assert got.tolist() == eq_table(z), b
        else:
            want = eq_table_np(z)
            sample = np.r_[0:size:257, size - 1]
            assert got[sample].tolist() == want[sample].tolist(), b
    assert int(limbs_to_object(strided[1, :size])[int("".join(map(str, zs[1])), 2)]) == 1     # a boolean point: the indicator


def test_a_z_entry_or_a_coefficient_that_is_not_canonical_is_refused(ctx):
    n, terms = 2, [(1, (0,))]
    bad = np.full((1, 1, 4), (1 << 64) - 1, dtype=np.uint64)
    Z = np.concatenate([_z_limbs([[3]]), bad], axis=1)
    tables = to_limbs([0, 1, 2, 3])
    d = ctx.alloc(tables.nbytes)
    try:
        ctx.upload(d, tables)
        with pytest.raises(GkrError) as e:
            ctx.sumcheck_zerocheck_batch_device(d, n, 1, terms, 1, Z)
        assert e.value.status == N.GKR_ERR_NON_CANONICAL
        with pytest.raises(GkrError) as e:
            ctx.eq_table_device(Z, n, 1, d)
        assert e.value.status == N.GKR_ERR_NON_CANONICAL
        assert np.array_equal(ctx.download(d, tables.shape), tables)
        arr = (N.SopTerm * 1)()
        arr[0].degree = 1
        C, L, R = np.zeros((n, 3, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros((n, 4), dtype=np.uint64)
        z_ok = _z_limbs([[3, 5]])
        rc = N.lib().gkr_sumcheck_zerocheck_batch_device(ctx._h, d, n, 1, ctypes.cast(arr, ctypes.c_void_p), _ptr(bad), 1, 1, _ptr(z_ok), _ptr(C),
                                                         _ptr(L), _ptr(R), None, None)
        assert rc == N.GKR_ERR_NON_CANONICAL and not C.any() and not L.any() and not R.any()
        # NULL coefficients are all ones, NULL evals and eq are not written
        assert N.lib().gkr_sumcheck_zerocheck_batch_device(ctx._h, d, n, 1, ctypes.cast(arr, ctypes.c_void_p), None, 1, 1, _ptr(z_ok), _ptr(C),
                                                           _ptr(L), _ptr(R), None, None) == 0
    finally:
        ctx.free(d)
    want = zerocheck_sumcheck([[0, 1, 2, 3]], terms, [3, 5], n)
    assert [from_limbs(C[j])[3 - int(L[j]):] for j in range(n)] == want[0] and from_limbs(R) == want[1]
    assert ctx.prove_zerocheck([tables], terms, [3, 5], n) == want
    tables[3] = bad[0, 0]
    with pytest.raises(GkrError) as e:
        ctx.prove_zerocheck([tables], terms, [3, 5], n)                                # the host form: a table entry >= r
    assert e.value.status == N.GKR_ERR_NON_CANONICAL


# ---- d. special points and inputs -------------------------------------------------------------------------------------------------------
def _bits(x, n):
    return [(x >> (n - 1 - j)) & 1 for j in range(n)]


def test_boolean_points_pick_single_entries(ctx):
    """n = 9, C = A o B except at one index x*: a boolean z = x* gives the claim g(x*), any other boolean z the claim 0; z all
    zero, all one and mixed with field elements against the model."""
    n = 9
    _, n_tables, terms = _structure("AB-C")
    rng = random.Random(7700)
    A, B = factor("random", n, rng), factor("random", n, rng)
    x_star = 0b101100111
    C = [a * b % P for a, b in zip(A, B)]
    C[x_star] = (C[x_star] + 12345) % P
    zs = [_bits(x_star, n), [0] * n, [1] * n, _bits(x_star ^ 1, n), _bits(x_star ^ (1 << (n - 1)), n),
          [(0, 1, rng.randrange(P))[j % 3] for j in range(n)]]
    got = _run(ctx, [[A, B, C]] * len(zs), n, terms, zs)
    assert got == [_model([A, B, C], terms, z, n) for z in zs]
    claims = [(2 * proof[0][-1] + sum(proof[0][:-1])) % P for proof, _, _, _ in got]
    assert claims[0] == (P - 12345) % P == (A[x_star] * B[x_star] - C[x_star]) % P
    assert claims[1:5] == [0] * 4
    for (proof, r, evals, eq_r), z, claim in zip(got, zs, claims):
        assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, claim)
        assert proof != [[0]] * n                                 # (g is not identically zero: only the SUM vanishes)


@pytest.mark.parametrize("n", [3, 10])
def test_a_satisfied_zero_check_and_terms_that_cancel(ctx, n):
    """C = A o B everywhere: the claim is zero and so are g_1(0) and g_1(1) one by one -- but the round vectors are NOT [0]: A~ B~ - C~
    vanishes on the cube, not as a polynomial (g_1 is a multiple of X (1 - X)), and the SOP path on the materialised eq table, to
    which this path is byte-equal, writes four coefficients too.  Every vector is [0] with length 1 where g IS the zero polynomial:
    A B - A B, and a satisfied LINEAR relation A - A' with A' = A (a multilinear extension is determined by its table)."""
    rng = random.Random(7800 + n)
    A, B = factor("random", n, rng), factor("random", n, rng)
    C = [a * b % P for a, b in zip(A, B)]
    zs = [_random_point(rng, n), [1] * n]
    zero = [[0]] * n, [multi_hash([0], 0)] * n
    _, _, terms = _structure("AB-C")
    got = _run(ctx, [[A, B, C]] * 2, n, terms, zs)
    assert got == [_model([A, B, C], terms, z, n) for z in zs]
    for (proof, r, evals, eq_r), z in zip(got, zs):
        assert proof[0][-1] == 0 and sum(proof[0]) % P == 0 and len(proof[0]) == 4          # g_1(0) = 0, g_1(1) = 0, g_1 != 0
        assert evals == [mle_eval(t, r) for t in (A, B, C)] and eq_r == mle_eval(eq_table(z), r)
        assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, 0)
    # g identically zero: every vector [0] with length 1
    for tables, terms in (([A, B], _structure("AB-AB")[2]), ([A, list(A)], [(1, (0,)), (P - 1, (1,))])):
        got = _run(ctx, [tables] * 2, n, terms, zs)
        for (proof, r, evals, eq_r), z in zip(got, zs):
            assert (proof, r) == zero
            assert evals == [mle_eval(t, r) for t in tables] and eq_r == mle_eval(eq_table(z), r)
            assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, 0)


def test_a_zero_table_in_the_middle_sumcheck_in_both_transcript_modes():
    """A B - A C at batch 3 with A the zero table in the middle sumcheck: its round vectors are all [0], its neighbours' are not.
    n = 2 (the first pass and one fold, a chunk below 256 entries), 9 and 10 (round 1 without and with an E_hi table; one block and
    two blocks per sumcheck in round 1)."""
    _, n_tables, terms = _structure("AB-AC")
    with Context(0) as c:
        for mode in (N.GKR_TRANSCRIPT_HOST, N.GKR_TRANSCRIPT_DEVICE):
            c.set_transcript(mode)
            for n in (2, 9, 10):
                rng = random.Random(7600 + n)
                groups = [[factor("zero" if (b, m) == (1, 0) else "random", n, rng) for m in range(n_tables)] for b in range(3)]
                zs = [_random_point(rng, n) for _ in range(3)]
                got = _run(c, groups, n, terms, zs)
                assert got == [_model(g, terms, z, n) for g, z in zip(groups, zs)], (mode, n)
                assert got[1][0] == [[0]] * n and got[1][1] == [multi_hash([0], 0)] * n
                assert all(len(v) == 4 for b in (0, 2) for v in got[b][0])


@pytest.mark.parametrize("n", [4, 10])
def test_coefficients_zero_one_and_r_minus_one(ctx, n):
    terms = [(0, (0, 1)), (1, (1, 2)), (P - 1, (0,))]
    rng = random.Random(7900 + n)
    groups = [[factor(MIX[(b + 3 * m) % len(MIX)], n, rng) for m in range(3)] for b in range(2)]
    zs = [_random_point(rng, n) for _ in range(2)]
    assert _run(ctx, groups, n, terms, zs) == [_model(g, terms, z, n) for g, z in zip(groups, zs)]
    # inner degree 1 alone: rows of three slots
    terms = [(P - 1, (0,)), (7, (1,))]
    assert _run(ctx, [g[:2] for g in groups], n, terms, zs) == [_model(g[:2], terms, z, n) for g, z in zip(groups, zs)]


# ---- e. large batches and offsets -------------------------------------------------------------------------------------------------------
def test_batch_limit(ctx):
    n, n_tables, batch = 2, 2, 65535
    terms = [(1, (0, 0)), (3, (1,)), (P - 2, (0, 1))]
    g = np.random.default_rng(65535)
    T = _random_limbs(g, batch * n_tables << n)
    Z = _random_limbs(g, batch * n).reshape(batch, n, 4)
    Z[1::4, 0], Z[2::4, 1] = 0, to_limbs([1])[0]
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        C, L, R, E, Q = ctx.sumcheck_zerocheck_batch_device(d, n, n_tables, terms, batch, Z)
    finally:
        ctx.free(d)
    tables = limbs_to_object(T).reshape(batch, n_tables, 1 << n)
    z = limbs_to_object(Z)
    for b in [0, 1, 2, batch // 2, batch - 1] + list(range(511, batch, 2048)):
        assert _decode(C, L, R, E, Q, b, 3) == zerocheck_sumcheck(list(tables[b]), terms, [int(x) for x in z[b]], n), b
    # every sumcheck: the first round's sum is the entry-by-entry claim, round 2's sum is round 1's value at its challenge, and
    # the last relation holds with eq(z, r) in O(n)
    c, r, e, q = limbs_to_object(C), limbs_to_object(R), limbs_to_object(E), limbs_to_object(Q)
    at_r = (((c[:, :, 0] * r + c[:, :, 1]) * r + c[:, :, 2]) * r + c[:, :, 3]) % P
    sums = (c[:, :, 0] + c[:, :, 1] + c[:, :, 2] + 2 * c[:, :, 3]) % P
    assert (sums[:, 1] == at_r[:, 0]).all()
    assert (q == ((z[:, 0] * r[:, 0] + (1 - z[:, 0]) * (1 - r[:, 0])) * (z[:, 1] * r[:, 1] + (1 - z[:, 1]) * (1 - r[:, 1]))) % P).all()
    assert (at_r[:, 1] == q * (e[:, 0] * e[:, 0] + 3 * e[:, 1] + (P - 2) * e[:, 0] * e[:, 1]) % P).all()
    eq = np.stack([(1 - z[:, 0]) * (1 - z[:, 1]), (1 - z[:, 0]) * z[:, 1], z[:, 0] * (1 - z[:, 1]), z[:, 0] * z[:, 1]], axis=1) % P
    g_x = (tables[:, 0] * tables[:, 0] + 3 * tables[:, 1] + (P - 2) * tables[:, 0] * tables[:, 1]) % P
    assert (sums[:, 0] == (eq * g_x).sum(axis=1) % P).all()


def test_offsets_past_four_gib(ctx):
    """n = 16, 3 tables, batch 700, tables from gkr_device_fill_table: the last sumcheck's tables start at byte 2097 * 2^21 > 2^32.
    Its row must be byte-equal to the same sumcheck run alone at batch 1 from its offset pointer."""
    import torch
    n, n_tables, batch = 16, 3, 700
    _, _, terms = _structure("AB-C")
    size = 32 << n
    assert (batch - 1) * n_tables * size >= 1 << 32
    if torch.cuda.mem_get_info()[0] < int(1.75 * batch * n_tables * size):
        pytest.skip("not enough free device memory for 2100 tables of 2^16 entries")
    Z = _random_limbs(np.random.default_rng(700), batch * n).reshape(batch, n, 4)
    d = ctx.alloc(batch * n_tables * size)
    try:
        ctx.fill_table(d, batch * n_tables << n, 20261019)
        last = ctypes.c_void_p(d.value + (batch - 1) * n_tables * size)
        full = ctx.sumcheck_zerocheck_batch_device(d, n, n_tables, terms, batch, Z)
        alone = ctx.sumcheck_zerocheck_batch_device(last, n, n_tables, terms, 1, Z[batch - 1:])
        first = ctx.sumcheck_zerocheck_batch_device(d, n, n_tables, terms, 1, Z[:1])
        tables = limbs_to_object(ctx.download(last, (n_tables << n, 4))).reshape(n_tables, 1 << n)
    finally:
        ctx.free(d)
    for name, f, a, a0 in zip(("coeffs", "len", "r", "evals", "eq"), full, alone, first):
        assert f[batch - 1:].tobytes() == a.tobytes(), name
        assert f[:1].tobytes() == a0.tobytes(), name
    assert full[0][batch - 1].tobytes() != full[0][0].tobytes()
    z = from_limbs(Z[batch - 1])
    proof, r, evals, eq_r = _decode(*alone, 0, 3)
    assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, zerocheck_claim_np(tables, terms, z))
    # every row: lengths, and the challenge chain's last relation (vectorised)
    assert (full[1] == 4).all()
    c, rr = limbs_to_object(full[0][:, n - 1]), limbs_to_object(full[2][:, n - 1])
    e, q = limbs_to_object(full[3]), limbs_to_object(full[4])
    at_r = (((c[:, 0] * rr + c[:, 1]) * rr + c[:, 2]) * rr + c[:, 3]) % P
    assert (at_r == q * (e[:, 0] * e[:, 1] - e[:, 2]) % P).all()


# ---- f. through the existing verifier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 13])
def test_transcripts_pass_the_sop_verifier_on_the_device_built_eq_table(ctx, n):
    _, n_tables, terms = _structure("5AB+7BC+11A")
    lifted = lift_terms(terms)
    batch, M = 3, n_tables + 1
    g = np.random.default_rng(8100 + n)
    T = _random_limbs(g, batch * n_tables << n).reshape(batch, n_tables, 1 << n, 4)
    Z = _random_limbs(g, batch * n).reshape(batch, n, 4)
    Z[1] = _z_limbs([[j % 2 for j in range(n)]])[0]               # one boolean point
    S = np.zeros((batch, M, 1 << n, 4), dtype=np.uint64)
    S[:, 1:] = T
    claims = to_limbs([zerocheck_claim_np(limbs_to_object(T[b]), terms, from_limbs(Z[b])) for b in range(batch)])
    d_s, d_t = ctx.alloc(S.nbytes), ctx.alloc(T.nbytes)
    try:
        ctx.upload(d_s, S)
        ctx.upload(d_t, T)
        ctx.eq_table_device(Z, n, batch, d_s, stride=M << n)
        C, L, R, E, Q = ctx.sumcheck_zerocheck_batch_device(d_t, n, n_tables, terms, batch, Z)
        accept, rnd, check, out_claims, out_evals = ctx.verify_sumcheck_sop_batch_device(d_s, n, M, lifted, batch, C, L, R, claims)
        assert accept.all() and (check == N.GKR_VERIFY_OK).all()
        assert np.array_equal(out_claims, claims)
        assert np.array_equal(out_evals[:, 1:], E) and np.array_equal(out_evals[:, 0], Q)
        # one entry of table B of sumcheck 1 changed (at the index its boolean point selects: the sum moves)
        x = int("".join(str(j % 2) for j in range(n)), 2)
        entry = ctypes.c_void_p(d_s.value + 32 * (((1 * M + 2) << n) + x))
        ctx.upload(entry, to_limbs([(from_limbs(T[1, 1, x:x + 1])[0] + 1) % P]))
        accept, rnd, check, _, _ = ctx.verify_sumcheck_sop_batch_device(d_s, n, M, lifted, batch, C, L, R, claims)
        assert accept.tolist() == [True, False, True]
        assert int(check[1]) == N.GKR_VERIFY_EVALUATION and int(rnd[1]) == n
    finally:
        ctx.free(d_s)
        ctx.free(d_t)


# ---- g. one context for four paths ------------------------------------------------------------------------------------------------------
def test_context_reuse_with_the_plain_the_product_and_the_sop_path():
    n, batch = 10, 3
    _, n_tables, terms = _structure("5AB+7BC+11A")
    rng = random.Random(8300)
    groups = [[factor(MIX[(b + 3 * m) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(batch)]
    zs = [_random_point(rng, n) for _ in range(batch)]
    Z = _z_limbs(zs)
    want = [_model(g, terms, z, n) for g, z in zip(groups, zs)]
    T = _limbs(groups)
    calls = (lambda c, d: c.sumcheck_mle_batch_device(d, n, batch * n_tables),
             lambda c, d: c.sumcheck_product_batch_device(d, n, 3, batch),
             lambda c, d: c.sumcheck_sop_batch_device(d, n, n_tables, terms, batch),
             lambda c, d: c.sumcheck_zerocheck_batch_device(d, n, n_tables, terms, batch, Z))

    def alone(call, mode):                                        # one path on a context of its own
        with Context(0) as c:
            c.set_transcript(mode)
            d = c.alloc(T.nbytes)
            try:
                c.upload(d, T)
                return calls[call](c, d)
            finally:
                c.free(d)

    with Context(0) as c:
        d = c.alloc(T.nbytes)
        try:
            c.upload(d, T)
            for mode in (N.GKR_TRANSCRIPT_HOST, N.GKR_TRANSCRIPT_DEVICE):
                ref = [alone(call, mode) for call in range(4)]
                assert [_decode(*ref[3], b, 3) for b in range(batch)] == want, mode
                c.set_transcript(mode)
                order = (3, 0, 3, 2, 1, 3, 2, 0, 1, 3)
                for call in order:
                    got = calls[call](c, d)
                    assert len(got) == len(ref[call]) and all(np.array_equal(a, b) for a, b in zip(got, ref[call])), (mode, call)
            assert np.array_equal(c.download(d, T.shape), T)
        finally:
            c.free(d)

"""gkr_sumcheck_sop_batch_device / gkr_sumcheck_sop (csrc/kernels_sop.hip, csrc/capi_sop.hip) through the C ABI, bit-exact against
the dense integer model of tests/sop_model.py -- which tests/test_sop_host.py holds against the term-list prover on add_poly of
scaled mult_poly term lists, against the product model and against the reference's own Python prover.

  a. the shape matrix: n x the six structures x batch, factor kinds mixed per table;
  b. one term of coefficient 1 against gkr_sumcheck_product_batch_device, byte for byte;
  c. cancellation across terms;
  d. bookkeeping: mixed degrees, squares and cubes, shared tables, 8 terms over 8 tables, coefficients, term_coeffs = NULL;
  e. the batch limit and offsets past 4 GiB;
  f. multi-block shapes (tests/product_shapes.py's geometry), every sumcheck through the host verifier with an independently
     summed claim and the device's own evaluations;
  g. one context for the plain, the product and this path, inputs unmodified."""

import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import mle_eval, verify_sumcheck_sop
from oracle.mimc7 import multi_hash
from product_model import factor, product_sumcheck
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from sop_model import (STRUCTURES, constant_tables_transcript, limbs_to_object, sop_claim_np, sop_degree, sop_eval, sop_sumcheck,
                       sop_sumcheck_np)
from sop_terms import BOOKKEEPING

pytestmark = pytest.mark.gpu

SHAPE_N = [2, 3, 5, 8, 9, 10, 11, 13]  # n = 9 .. 13: the first shapes with 2 .. 16 blocks per sumcheck in the value pass
MIX = ["random", "indep_first", "all_max", "indep_last", "specials", "bits", "indep_middle", "constant"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def _decode(C, L, R, E, b, degree):
    n = L.shape[1]
    proof = [from_limbs(C[b, j])[degree + 1 - int(L[b, j]):] for j in range(n)]
    assert all(not C[b, j, :degree + 1 - int(L[b, j])].any() for j in range(n)), "unused slots hold zero"
    return proof, from_limbs(R[b]), from_limbs(E[b])


def _limbs(groups):
    return np.concatenate([to_limbs(t) for g in groups for t in g])


def _run(ctx, groups, n, terms):
    """groups[b][m]: table m of sumcheck b (lists of 2^n ints) -> [(proof, r, evals)] through the resident-table entry point."""
    T = _limbs(groups)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        out = ctx.sumcheck_sop_batch_device(d, n, len(groups[0]), terms, len(groups))
    finally:
        ctx.free(d)
    return [_decode(*out, b, sop_degree(terms)) for b in range(len(groups))]


def _model(tables, terms, n):
    """The model's transcript of one sumcheck (the vectorised form from 2^8 entries on; test_sop_host.py holds the two equal)."""
    if n < 8:
        return sop_sumcheck(tables, terms, n)
    return sop_sumcheck_np(np.array(tables, dtype=object), terms, n)


# ---- the golden fixtures through both entry points --------------------------------------------------------------------------------------
def test_golden_fixtures_of_the_reference_python_prover(ctx):
    for c in load_golden("sop_sumcheck.json")["cases"]:
        tables = [[int(x) for x in t] for t in c["tables"]]
        terms = [(int(k), tuple(idx)) for k, idx in c["terms"]]
        want = ([[int(x) for x in g] for g in c["proof"]], [int(x) for x in c["r"]])
        proof, r, evals = ctx.prove_sumcheck_sop(tables, terms, c["n"])               # the host form
        assert (proof, r) == want, (c["name"], c["n"])
        assert evals == [mle_eval(t, r) for t in tables]
        assert verify_sumcheck_sop(proof, r, evals, terms, int(c["claim"]))
        assert _run(ctx, [tables], c["n"], terms) == [(proof, r, evals)]              # the resident form


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("structure", STRUCTURES, ids=[s[0] for s in STRUCTURES])
@pytest.mark.parametrize("n", SHAPE_N)
def test_shapes_match_the_model(ctx, n, structure, batch):
    name, n_tables, terms = structure
    rng = random.Random(5100 + 97 * n + 7 * len(name) + batch)
    groups = [[factor(MIX[(n + 3 * b + 5 * m + n_tables) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(batch)]
    assert _run(ctx, groups, n, terms) == [_model(g, terms, n) for g in groups]


# ---- b. one term against the product path -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 7, 12])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_one_term_is_the_product_path_byte_for_byte(ctx, n, degree):
    kinds = ["random", "zero", "indep_last", "constant", "bits", "indep_first", "all_max"]
    rng = random.Random(700 + 10 * n + degree)
    batch = len(kinds)
    groups = [[factor(kinds[b] if f == (b % degree) else ("random", "indep_last", "constant")[(b + f) % 3], n, rng) for f in range(degree)]
              for b in range(batch)]
    T = _limbs(groups)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        want = ctx.sumcheck_product_batch_device(d, n, degree, batch)
        got = ctx.sumcheck_sop_batch_device(d, n, degree, [(1, tuple(range(degree)))], batch)
    finally:
        ctx.free(d)
    for name, g, w in zip(("coeffs", "len", "r", "evals"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, n, degree)
    assert [_decode(*got, b, degree) for b in range(batch)] == [product_sumcheck(g, n) for g in groups]
    assert (got[1][1] == 1).all() and not got[0][1].any()                            # the zero factor's sumcheck: every vector [0]
    assert (got[1] < degree + 1).any()


# ---- c. cancellation across terms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 10])
def test_terms_that_cancel(ctx, n):
    rng = random.Random(900 + n)
    A, B, C = (factor("random", n, rng) for _ in range(3))
    k = rng.randrange(1, P)
    # A B - A B: every vector [0]
    terms = [(1, (0, 1)), (P - 1, (0, 1))]
    (proof, r, evals), = _run(ctx, [[A, B]], n, terms)
    assert proof == [[0]] * n and r == [multi_hash([0], 0)] * n
    assert evals == [mle_eval(A, r), mle_eval(B, r)]
    # A B - A B' with B' = B + k: g = -k A, every vector has at most two coefficients
    terms = [(1, (0, 1)), (P - 1, (0, 2))]
    groups = [[A, B, [(x + k) % P for x in B]]]
    got = _run(ctx, groups, n, terms)
    assert got == [_model(groups[0], terms, n)]
    assert all(len(g) <= 2 for g in got[0][0]) and any(len(g) == 2 for g in got[0][0])
    assert got[0][0] == _model([A], [(P - k, (0,))], n)[0]
    # A B C - A B C' with C' = C + k: the degree-3 coefficient cancels, the degree-2 one does not (g = -k A B)
    terms = [(1, (0, 1, 2)), (P - 1, (0, 1, 3))]
    groups = [[A, B, C, [(x + k) % P for x in C]]]
    got = _run(ctx, groups, n, terms)
    assert got == [_model(groups[0], terms, n)]
    assert all(len(g) == 3 for g in got[0][0])
    assert got[0][0] == _model([A, B], [(P - k, (0, 1))], n)[0]


def test_a_zero_table_in_the_middle_sumcheck_in_both_transcript_modes():
    """A B C - A D at batch 3 with A the zero table in the middle sumcheck: its round vectors are all [0], its neighbours' are not.
    n = 2 (the first pass and one fold, a chunk below 256 entries), 9 and 10 (one block and two blocks per sumcheck in round 1)."""
    _, n_tables, terms = next(s for s in STRUCTURES if s[0] == "ABC-AD")
    with Context(0) as c:
        for mode in (N.GKR_TRANSCRIPT_HOST, N.GKR_TRANSCRIPT_DEVICE):
            c.set_transcript(mode)
            for n in (2, 9, 10):
                rng = random.Random(1000 + n)
                groups = [[factor("zero" if (b, m) == (1, 0) else "random", n, rng) for m in range(n_tables)] for b in range(3)]
                got = _run(c, groups, n, terms)
                assert got == [_model(g, terms, n) for g in groups], (mode, n)
                assert got[1][0] == [[0]] * n and got[1][1] == [multi_hash([0], 0)] * n
                assert all(len(v) == 4 for b in (0, 2) for v in got[b][0])


# ---- d. bookkeeping ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 10])
@pytest.mark.parametrize("name", list(BOOKKEEPING))
def test_bookkeeping(ctx, name, n):
    n_tables, terms = BOOKKEEPING[name]
    assert {i for _, idx in terms for i in idx} == set(range(n_tables))
    rng = random.Random(1100 + n + len(name))
    groups = [[factor(MIX[(b + 3 * m) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(2)]
    assert _run(ctx, groups, n, terms) == [_model(g, terms, n) for g in groups]


def test_null_coefficients_are_all_ones_and_null_evals(ctx):
    n, n_tables, batch = 10, 3, 2
    spec = [(0, 1, 2), (1, 2), (0,)]
    terms = [(1, idx) for idx in spec]
    rng = random.Random(1212)
    groups = [[factor("random", n, rng) for _ in range(n_tables)] for _ in range(batch)]
    T = _limbs(groups)
    arr = (N.SopTerm * len(spec))()
    for k, idx in enumerate(spec):
        arr[k].degree = len(idx)
        for j, i in enumerate(idx):
            arr[k].table[j] = i
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
        C2, L2, R2 = np.zeros_like(C), np.zeros_like(L), np.zeros_like(R)
        assert N.lib().gkr_sumcheck_sop_batch_device(ctx._h, d, n, n_tables, ctypes.cast(arr, ctypes.c_void_p), None, len(spec), batch, _ptr(C2),
                                                     _ptr(L2), _ptr(R2), None) == 0
        again = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch, out=(C2, L2, R2, np.zeros_like(E)))
    finally:
        ctx.free(d)
    assert np.array_equal(C, C2) and np.array_equal(L, L2) and np.array_equal(R, R2)
    assert again[0] is C2 and np.array_equal(again[3], E)
    assert [_decode(C, L, R, E, b, 3) for b in range(batch)] == [_model(g, terms, n) for g in groups]


def test_a_coefficient_or_a_host_table_entry_that_is_not_canonical_is_refused(ctx):
    from gkr_amd import GkrError
    n, terms = 2, [(1, (0,))]
    not_canonical = np.full((1, 4), (1 << 64) - 1, dtype=np.uint64)
    arr = (N.SopTerm * 1)()
    arr[0].degree = 1
    tables = to_limbs([0, 1, 2, 3])
    C, L, R = np.zeros((n, 2, 4), dtype=np.uint64), np.zeros(n, dtype=np.uint32), np.zeros((n, 4), dtype=np.uint64)
    rc = N.lib().gkr_sumcheck_sop(ctx._h, _ptr(tables), n, 1, ctypes.cast(arr, ctypes.c_void_p), _ptr(not_canonical), 1, _ptr(C), _ptr(L), _ptr(R), None)
    assert rc == N.GKR_ERR_NON_CANONICAL and not C.any() and not L.any() and not R.any()
    assert ctx.prove_sumcheck_sop([tables], terms, n) == sop_sumcheck([[0, 1, 2, 3]], terms, n)      # the same tables are fine
    tables[3] = not_canonical[0]
    with pytest.raises(GkrError) as e:
        ctx.prove_sumcheck_sop([tables], terms, n)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL


# ---- e. large batches and offsets -------------------------------------------------------------------------------------------------------
def _random_limbs(rng, count):
    T = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64)
    T[:, 3] &= np.uint64((1 << 60) - 1)                           # below 2^252: canonical
    return T


def test_batch_limit(ctx):
    n, n_tables, batch = 2, 2, 65535
    terms = [(1, (0, 0)), (3, (1,)), (P - 2, (0, 1))]
    T = _random_limbs(np.random.default_rng(65535), batch * n_tables << n)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
    finally:
        ctx.free(d)
    tables = limbs_to_object(T).reshape(batch, n_tables, 1 << n)
    for b in [0, batch // 2, batch - 1] + list(range(511, batch, 1024)):
        assert _decode(C, L, R, E, b, 2) == sop_sumcheck(list(tables[b]), terms, n), b
    # every challenge is the hash of its row (the verifier's hash kernel, one call), every last relation holds, every round's sum
    # is the value of the round before at its challenge
    H, valid = ctx.multi_hash_batch(C.reshape(-1, 3, 4), L.reshape(-1))
    assert valid.all() and np.array_equal(H, R.reshape(-1, 4))
    assert (L == 3).all()
    c = limbs_to_object(C)                                        # (batch, n, 3)
    r, e = limbs_to_object(R), limbs_to_object(E)
    at_r = ((c[:, :, 0] * r + c[:, :, 1]) * r + c[:, :, 2]) % P
    sums = (c[:, :, 0] + c[:, :, 1] + 2 * c[:, :, 2]) % P
    assert (sums[:, 1] == at_r[:, 0]).all()
    assert (at_r[:, 1] == (e[:, 0] * e[:, 0] + 3 * e[:, 1] + (P - 2) * e[:, 0] * e[:, 1]) % P).all()
    claims = (tables[:, 0] * tables[:, 0] + 3 * tables[:, 1] + (P - 2) * tables[:, 0] * tables[:, 1]).sum(axis=1) % P
    assert (sums[:, 0] == claims).all()


def test_offsets_past_four_gib(ctx):
    """n = 16, 3 tables, batch 684: 2052 tables of 2 MiB; the last sumcheck's tables start at byte 2049 * 2^21 > 2^32.  Sumchecks
    0 .. 682 are constant tables with a value of their own each (the transcript is closed-form, and a table read at a wrapped
    offset would show); the last one is random."""
    n, n_tables, batch = 16, 3, 684
    _, _, terms = next(s for s in STRUCTURES if s[0] == "5AB+7BC+11A")
    size = 32 << n
    assert (batch - 1) * n_tables * size >= 1 << 32                # the last sumcheck's first byte
    if _free_bytes() < int(1.75 * batch * n_tables * size):
        pytest.skip("not enough free device memory for 2052 tables of 2^16 entries")
    values = [((t + 1) * 0x9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251F86C6A11D0C18E95) % P for t in range((batch - 1) * n_tables)]
    vl = to_limbs(values)
    last = _random_limbs(np.random.default_rng(4096), n_tables << n)
    d = ctx.alloc(batch * n_tables * size)
    try:
        per = 64                                                  # tables per upload (128 MiB)
        for t0 in range(0, len(values), per):
            ctx.upload(ctypes.c_void_p(d.value + t0 * size), np.repeat(vl[t0:t0 + per], 1 << n, axis=0))
        ctx.upload(ctypes.c_void_p(d.value + len(values) * size), last)
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
        points = np.repeat(R[batch - 1:], n_tables, axis=0)
        dev_evals = ctx.mle_eval_batch_device(ctypes.c_void_p(d.value + len(values) * size), n, n_tables, points)
    finally:
        ctx.free(d)
    # the constant sumchecks: [2^(n-1-j) g(values)], one coefficient, in every round; evals = the values
    assert (L[:batch - 1] == 1).all() and not C[:batch - 1, :, :2].any()
    g = [sop_eval(values[b * n_tables:(b + 1) * n_tables], terms) for b in range(batch - 1)]
    want = to_limbs([(1 << (n - 1 - j)) * gb % P for gb in g for j in range(n)]).reshape(batch - 1, n, 4)
    assert np.array_equal(C[:batch - 1, :, 2], want)
    assert np.array_equal(E[:batch - 1].reshape(-1, 4), vl)
    H, valid = ctx.multi_hash_batch(C.reshape(-1, 3, 4), L.reshape(-1))
    assert valid.all() and np.array_equal(H, R.reshape(-1, 4))
    for b in (0, 341, batch - 2):
        assert _decode(C, L, R, E, b, 2) == constant_tables_transcript(values[b * n_tables:(b + 1) * n_tables], terms, n), b
    # the last one
    tables = limbs_to_object(last).reshape(n_tables, 1 << n)
    proof, r, evals = _decode(C, L, R, E, batch - 1, 2)
    assert (proof, r, evals) == sop_sumcheck_np(tables, terms, n)
    assert verify_sumcheck_sop(proof, r, evals, terms, sop_claim_np(tables, terms))
    assert np.array_equal(dev_evals, E[batch - 1])


# ---- f. multi-block shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,structure,modelled", [(16, 1, "ABC-AD", (0,)), (16, 20, "5AB+7BC+11A", (0, 19)), (20, 1, "ABC-AD", ())])
def test_multi_block_shapes(ctx, n, batch, structure, modelled):
    """(16, 1): 128 blocks, two trips of the round kernel's wave loop; (16, 20): 103 blocks of which 64 work, chunk 512; (20, 1): the
    cap of 2048 blocks, 32 trips.  The sumchecks in `modelled` against the model (at 2^20 entries the model takes too long); every
    sumcheck through the host verifier with a claim summed entry by entry and the evaluations gkr_mle_eval_batch_device computes."""
    assert tuple(product_geometry(n, batch)[:2]) == PRODUCT_GEOMETRY[(n, batch)]
    _, n_tables, terms = next(s for s in STRUCTURES if s[0] == structure)
    T = _random_limbs(np.random.default_rng(1600 + n + batch), batch * n_tables << n)
    T = T.reshape(batch, n_tables, 1 << n, 4)
    T[batch - 1, 0, 1::2] = T[batch - 1, 0, 0::2]                 # table 0 of the last sumcheck ignores x_n ...
    T[0, n_tables - 1, 1 << (n - 1):] = T[0, n_tables - 1, :1 << (n - 1)]   # ... and the last table of the first one x_1
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
        dev_evals = ctx.mle_eval_batch_device(d, n, batch * n_tables, np.repeat(R, n_tables, axis=0))
    finally:
        ctx.free(d)
    assert np.array_equal(dev_evals.reshape(batch, n_tables, 4), E)
    D = sop_degree(terms)
    for b in range(batch):
        tables = limbs_to_object(T[b])
        proof, r, evals = _decode(C, L, R, E, b, D)
        assert verify_sumcheck_sop(proof, r, evals, terms, sop_claim_np(tables, terms)), b
        if b in modelled:
            assert (proof, r, evals) == sop_sumcheck_np(tables, terms, n), b


# ---- g. one context for three paths -------------------------------------------------------------------------------------------------------
def test_context_reuse_with_the_plain_and_the_product_path():
    n, batch = 10, 3
    _, n_tables, terms = next(s for s in STRUCTURES if s[0] == "ABC-AD")
    rng = random.Random(1300)
    groups = [[factor(MIX[(b + 3 * m) % len(MIX)], n, rng) for m in range(n_tables)] for b in range(batch)]
    want = [_model(g, terms, n) for g in groups]
    T = _limbs(groups)
    lib = N.lib()
    lib.gkr_device_tables_differ.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
    with Context(0) as c:
        d, copy = c.alloc(T.nbytes), c.alloc(T.nbytes)
        try:
            c.upload(d, T)
            c.upload(copy, T)
            for mode in (N.GKR_TRANSCRIPT_HOST, N.GKR_TRANSCRIPT_DEVICE):
                c.set_transcript(mode)
                plain = c.sumcheck_mle_batch_device(d, n, batch * n_tables)
                product = c.sumcheck_product_batch_device(d, n, 2, batch * 2)         # the same memory as 6 pairs of tables
                sop = c.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
                assert [_decode(*sop, b, 3) for b in range(batch)] == want, mode
                product2 = c.sumcheck_product_batch_device(d, n, 2, batch * 2)        # ... and the other order
                plain2 = c.sumcheck_mle_batch_device(d, n, batch * n_tables)
                sop2 = c.sumcheck_sop_batch_device(d, n, n_tables, terms, batch)
                for a, b in zip(plain + product + sop, plain2 + product2 + sop2):
                    assert np.array_equal(a, b), mode
            differ = ctypes.c_uint32(7)
            assert lib.gkr_device_tables_differ(c._h, d, copy, T.shape[0], ctypes.byref(differ)) == 0 and differ.value == 0
        finally:
            c.free(d)
            c.free(copy)

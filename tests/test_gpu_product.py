"""gkr_sumcheck_product_batch_device / gkr_sumcheck_product (csrc/kernels_product.hip, csrc/capi_product.hip) through the C ABI,
bit-exact against the dense integer model of tests/product_model.py -- which tests/test_product_host.py holds against the
reference's own Python prover and against the term-list prover on mult_poly term lists."""

import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import mle_eval, verify_sumcheck_product
from product_model import constant_tables_transcript, factor, product_sumcheck

pytestmark = pytest.mark.gpu

SHAPE_N = [2, 3, 6, 7, 9, 10, 13]      # half a table: below one wave, one wave (n = 7), one 256-chunk (n = 9), several blocks
MIX = ["random", "indep_first", "all_max", "indep_last", "specials", "bits", "indep_middle", "random"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _decode(C, L, R, E, b, degree):
    n = L.shape[1]
    proof = [from_limbs(C[b, j])[degree + 1 - int(L[b, j]):] for j in range(n)]
    assert all(not C[b, j, :degree + 1 - int(L[b, j])].any() for j in range(n)), "unused slots hold zero"
    return proof, from_limbs(R[b]), from_limbs(E[b])


def _run(ctx, groups, n, degree):
    """groups[b][f]: factor f of sumcheck b (lists of 2^n ints) -> [(proof, r, evals)] through the resident-table entry point."""
    T = np.concatenate([to_limbs(t) for g in groups for t in g])
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        out = ctx.sumcheck_product_batch_device(d, n, degree, len(groups))
    finally:
        ctx.free(d)
    return [_decode(*out, b, degree) for b in range(len(groups))]


_shape_cache = {}


def _shape(n, degree, batch):
    """The factors of a shape (kinds that move with the sumcheck, the factor and n) and the model's transcripts, computed once."""
    key = (n, degree, batch)
    if key not in _shape_cache:
        rng = random.Random(4100 + 97 * n + 7 * degree + batch)
        groups = [[factor(MIX[(n + 3 * b + 5 * f + degree) % len(MIX)], n, rng) for f in range(degree)] for b in range(batch)]
        _shape_cache[key] = (groups, [product_sumcheck(g, n) for g in groups])
    return _shape_cache[key]


def test_golden_fixtures_of_the_reference_python_prover(ctx):
    for c in load_golden("product_sumcheck.json")["cases"]:
        tables = [[int(x) for x in t] for t in c["tables"]]
        want = ([[int(x) for x in g] for g in c["proof"]], [int(x) for x in c["r"]])
        proof, r, evals = ctx.prove_sumcheck_product(tables, c["n"])                 # the host form
        assert (proof, r) == want, (c["n"], c["degree"])
        assert evals == [mle_eval(t, r) for t in tables]
        assert verify_sumcheck_product(proof, r, evals, c["degree"], int(c["claim"]))
        assert _run(ctx, [tables], c["n"], c["degree"]) == [(proof, r, evals)]       # the resident form


def test_golden_plain_transcripts_at_degree_one(ctx, mle_cases):
    assert len(mle_cases) == 9
    for c in mle_cases:
        table = [int(x) for x in c["table"]]
        proof, r, evals = ctx.prove_sumcheck_product([table], c["n"])
        assert proof == [[int(x) for x in g] for g in c["proof"]] and r == [int(x) for x in c["r"]], c["n"]
        assert evals == [mle_eval(table, r)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("n", SHAPE_N)
def test_shapes_match_the_model(ctx, n, degree, batch):
    groups, want = _shape(n, degree, batch)
    assert _run(ctx, groups, n, degree) == want


def test_the_shape_matrix_reaches_short_vectors_in_every_kind_of_round():
    """(model only) lengths below degree + 1 occur in first, middle and last rounds of the matrix above, at every degree."""
    for degree in (1, 2, 3):
        where = set()
        for n in SHAPE_N:
            for batch in (1, 3):
                for proof, _, _ in _shape(n, degree, batch)[1]:
                    where |= {("first" if j == 0 else "last" if j == n - 1 else "middle") for j, g in enumerate(proof) if len(g) < degree + 1}
        assert where == {"first", "middle", "last"}, (degree, where)


@pytest.mark.parametrize("n", [3, 10])
def test_a_zero_factor_gives_zero_vectors_of_length_one(ctx, n):
    rng = random.Random(300 + n)
    for degree in (1, 2, 3):
        groups = [[factor("zero" if f == at else ("random", "indep_last", "bits")[(f + at) % 3], n, rng) for f in range(degree)]
                  for at in range(degree)]
        got = _run(ctx, groups, n, degree)
        for at, (proof, r, evals) in enumerate(got):
            assert proof == [[0]] * n and evals[at] == 0, (degree, at)
        assert got == [product_sumcheck(g, n) for g in groups]


def _free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def test_term_bound_with_all_max_factors():
    """The most products one thread adds into a Lazy17 between two reductions.  A thread visits ceil(chunk / 256) table pairs,
    chunk = the 256-multiple above items / blocks, and mle_blocks_per_table gives items / 1024 blocks up to kMaxBlocksPerTable =
    2048: four pairs per thread for every half table up to 2^21 entries, doubling with each doubling of the table from there.
    The largest half the ABI admits with products in play is 2^28 (degree 2, n = 29, batch 1: 2 * 2^29 = 2^30 values): 2048
    blocks, chunk 2^17, 512 products of (p - 1)^2 per thread and accumulator (the accumulator's seventeenth limb is in use from
    the 24th on), 256 threads per Acc<9> block sum and 2048 partials per Acc<10> total -- each count at its maximum.
    Constant tables: the expected transcript is the model's closed form (tests/test_product_host.py ties it to the model)."""
    n, degree = 29, 2
    size = 32 << n
    if _free_bytes() < int(2.75 * degree * size):                # the tables, half of them again as workspace, and headroom
        pytest.skip("not enough free device memory for two 2^29-entry tables")
    block = np.tile(to_limbs([P - 1]), (1 << 22, 1))             # 128 MiB of p - 1
    with Context(0) as c:                                        # (its own context: the 16 GiB of workspace go with it)
        d = c.alloc(degree * size)
        try:
            for off in range(0, degree * size, block.nbytes):
                c.upload(ctypes.c_void_p(d.value + off), block)
            out = c.sumcheck_product_batch_device(d, n, degree, 1)
        finally:
            c.free(d)
    assert _decode(*out, 0, degree) == constant_tables_transcript([P - 1] * degree, n)


def test_evals_bind_to_the_tables_and_inputs_stay_unchanged(ctx):
    n, degree, batch = 10, 3, 3
    groups, want = _shape(n, degree, batch)
    T = np.concatenate([to_limbs(t) for g in groups for t in g])
    lib = N.lib()
    d, copy = ctx.alloc(T.nbytes), ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        ctx.upload(copy, T)
        C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
        differ = ctypes.c_uint32(7)
        lib.gkr_device_tables_differ.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
        assert lib.gkr_device_tables_differ(ctx._h, d, copy, T.shape[0], ctypes.byref(differ)) == 0 and differ.value == 0
        for b in range(batch):
            proof, r, evals = _decode(C, L, R, E, b, degree)
            assert (proof, r, evals) == want[b]
            assert evals == [mle_eval(t, r) for t in groups[b]]
        # the degree factors of one sumcheck are a batch of degree tables at the same point
        points = np.repeat(R, degree, axis=0)
        assert np.array_equal(ctx.mle_eval_batch_device(d, n, batch * degree, points), E.reshape(batch * degree, 4))
        # out_evals = NULL
        C2, L2, R2 = np.zeros_like(C), np.zeros_like(L), np.zeros_like(R)
        assert lib.gkr_sumcheck_product_batch_device(ctx._h, d, n, degree, batch, _ptr(C2), _ptr(L2), _ptr(R2), None) == 0
        assert np.array_equal(C, C2) and np.array_equal(L, L2) and np.array_equal(R, R2)
        # out=: the arrays of the earlier call are written into
        again = ctx.sumcheck_product_batch_device(d, n, degree, batch, out=(C2, L2, R2, np.zeros_like(E)))
        assert again[0] is C2 and np.array_equal(again[3], E)
    finally:
        ctx.free(d)
        ctx.free(copy)


def test_batch_limit(ctx):
    n, degree, batch = 2, 2, 65535
    rng = np.random.default_rng(65535)
    T = rng.integers(0, 1 << 63, size=(batch * degree << n, 4), dtype=np.uint64)
    T[:, 3] &= np.uint64((1 << 60) - 1)                           # below 2^252: canonical
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
    finally:
        ctx.free(d)
    tables = T.reshape(batch, degree, 1 << n, 4)
    for b in (0, batch // 2, batch - 1):
        assert _decode(C, L, R, E, b, degree) == product_sumcheck([from_limbs(t) for t in tables[b]], n), b
    vals = np.array(from_limbs(C.reshape(-1, 4)), dtype=object).reshape(batch, n, degree + 1)
    rs = np.array(from_limbs(R.reshape(-1, 4)), dtype=object).reshape(batch, n)
    es = np.array(from_limbs(E.reshape(-1, 4)), dtype=object).reshape(batch, degree)
    # (131070 round vectors: hashed in one call of the verifier's hash kernel, not one by one on the host)
    H, valid = ctx.multi_hash_batch(C.reshape(-1, degree + 1, 4), L.reshape(-1))
    assert valid.all()
    hs = np.array(from_limbs(H), dtype=object).reshape(batch, n)
    for b in range(batch):
        proof = [list(vals[b, j, degree + 1 - int(L[b, j]):]) for j in range(n)]
        assert verify_sumcheck_product(proof, list(rs[b]), list(es[b]), degree, hashes=list(hs[b])), b
        if b in (0, batch // 2, batch - 1):
            assert verify_sumcheck_product(proof, list(rs[b]), list(es[b]), degree), b


def test_offsets_past_four_gib(ctx):
    """n = 16, degree 3, batch 683: 2049 tables of 2 MiB; the last sumcheck's last factor starts at byte 2^32, and every
    offset is formed as (b * degree + f) << n."""
    n, degree, batch = 16, 3, 683
    size = 32 << n
    assert (batch * degree - 1) * size >= 1 << 32                # the last factor's first byte
    if _free_bytes() < int(1.75 * batch * degree * size):
        pytest.skip("not enough free device memory for 2049 tables of 2^16 entries")
    d = ctx.alloc(batch * degree * size)
    try:
        for t in range(batch * degree):
            ctx.fill_table(ctypes.c_void_p(d.value + t * size), 1 << n, 5000 + t)
        C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
        ends = {b: [from_limbs(ctx.download(ctypes.c_void_p(d.value + (b * degree + f) * size), (1 << n, 4))) for f in range(degree)]
                for b in (0, batch - 1)}
    finally:
        ctx.free(d)
    assert ends[0][0] != ends[batch - 1][0]
    for b, tables in ends.items():
        assert _decode(C, L, R, E, b, degree) == product_sumcheck(tables, n), b
    for b in range(batch):
        proof, r, evals = _decode(C, L, R, E, b, degree)
        assert verify_sumcheck_product(proof, r, evals, degree), b


def test_result_depends_on_neither_the_transcript_mode_nor_an_earlier_plain_sumcheck():
    n, degree, batch = 10, 3, 3
    groups, want = _shape(n, degree, batch)
    T = np.concatenate([to_limbs(t) for g in groups for t in g])
    with Context(0) as c:
        d = c.alloc(T.nbytes)
        try:
            c.upload(d, T)
            for mode in (N.GKR_TRANSCRIPT_HOST, N.GKR_TRANSCRIPT_DEVICE, N.GKR_TRANSCRIPT_HOST):
                c.set_transcript(mode)
                plain = c.sumcheck_mle_batch_device(d, n, batch * degree)            # the plain path's workspaces, same context
                out = c.sumcheck_product_batch_device(d, n, degree, batch)
                assert [_decode(*out, b, degree) for b in range(batch)] == want, mode
                again = c.sumcheck_mle_batch_device(d, n, batch * degree)            # ... and the plain path after the product's
                assert all(np.array_equal(a, b) for a, b in zip(plain, again)), mode
        finally:
            c.free(d)

"""gkr_sumcheck_sop_verify_batch_device / gkr_sumcheck_sop_verify (csrc/capi_mle_verify.hip, kernels_mle_eval.hip,
kernels_verify_hash.hip):

  a. transcripts proved on the device are accepted -- the golden cases and a shape matrix; the values the verifier computes are the
     prover's out_evals;
  b. the evaluation of a sumcheck's tables at their one shared point against the evaluation of every table on its own;
  c. the exhaustive single-element tamper sweep of tests/sop_verify_sweeps.py, one batch per transcript, against the closed-form
     model (which test_sop_verify_host.py holds to the four checks on Python integers);
  d. the verifier given other terms than the prover's;
  e. one term gives the product verifier's outputs byte for byte;
  f. verdicts and values depend neither on where the hashes ran, nor on the chunking, nor on the evaluation kernel;
  g. the chunk cap that keeps the table index inside a grid dimension;
  h. a table that starts 4 GiB into the tables.

The verifier's own output is never the reference."""

import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from product_model import factor
from product_verify_sweeps import cases as product_cases
from sop_model import STRUCTURES, sop_claim, sop_degree, sop_eval, sop_sumcheck
from sop_verify_sweeps import (ACCEPTED, CHALLENGE, EVALUATION, NON_CANONICAL, ROUND_SUM, SHAPE, arrays_of, assert_sweep_is_sharp,
                               assert_sweep_reaches_short_rows, build_batch, cases, point_sees, table_verdicts)
from verify_sweeps import R_LIMBS, limbs, value

pytestmark = pytest.mark.gpu
OPTIONS = ("mle_eval_mfma_min_n", "verify_device_hash_min", "verify_workspace_mb")
BOTH_HASH_SIDES = ((0, -1, 0), (0, 1, 0))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sop_cases():
    cases_ = load_golden("sop_sumcheck.json")["cases"]
    assert len(cases_) == 5
    return [{"name": c["name"], "n": c["n"], "terms": [(int(k), tuple(idx)) for k, idx in c["terms"]],
             "tables": [[int(x) for x in t] for t in c["tables"]], "proof": [[int(x) for x in g] for g in c["proof"]],
             "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases_]


def _triples(result):
    return [(bool(a), int(r), int(c)) for a, r, c in zip(result[0], result[1], result[2])]


def _first_difference(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def _reset(ctx):
    for name in OPTIONS:
        ctx.set_option(name, 0)


def _structure(name):
    return next((m, terms) for s, m, terms in STRUCTURES if s == name)


class Resident:
    """Tables (any shape (.., 4) of uint64 limbs) in device memory for the length of a `with`."""

    def __init__(self, ctx, T):
        self.ctx, self.T = ctx, np.ascontiguousarray(T)

    def __enter__(self):
        self.d = self.ctx.alloc(self.T.nbytes)
        try:
            self.ctx.upload(self.d, self.T)
        except Exception:
            self.ctx.free(self.d)
            raise
        return self.d

    def __exit__(self, *a):
        self.ctx.free(self.d)


def _limbs_of_tables(tables):
    return np.concatenate([to_limbs(t) for t in tables])


def _random_tables(count, n, seed):
    """count tables of 2^n canonical values (below 2^252) as limbs: every table different."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 1 << 63, size=(count << n, 4), dtype=np.uint64)
    T[:, 3] &= np.uint64((1 << 60) - 1)
    return T


# ---- a. proved on the device and accepted ---------------------------------------------------------------------------------------------
def test_golden_cases_proved_on_the_device_are_accepted(ctx, sop_cases):
    for c in sop_cases:
        n, terms, tables = c["n"], c["terms"], c["tables"]
        M = len(tables)
        with Resident(ctx, _limbs_of_tables(tables)) as d:
            C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, 1)
            assert from_limbs(R[0]) == c["r"]
            claim = to_limbs([c["claim"]])
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, 1, C, L, R, claims=claim)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[3], claim) and res[4].tobytes() == E.tobytes()
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, 1, C, L, R)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[3], claim) and res[4].tobytes() == E.tobytes()
        # the host-table entry point on the reference's own transcript
        assert ctx.verify_sumcheck_sop(tables, terms, c["proof"], c["r"], claim=c["claim"]) == ACCEPTED
        assert ctx.verify_sumcheck_sop(tables, terms, c["proof"], c["r"]) == ACCEPTED
        assert ctx.verify_sumcheck_sop(tables, terms, c["proof"], c["r"], claim=(c["claim"] + 1) % P) == (False, 0, ROUND_SUM)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("structure", STRUCTURES, ids=[s[0] for s in STRUCTURES])
@pytest.mark.parametrize("n", [2, 3, 8, 11, 12, 13, 16])
def test_shapes_proved_on_the_device_are_accepted(ctx, n, structure, batch):
    """n = 12 and 13 straddle the default switch between the one-block and the streaming evaluation kernel; n = 11 runs with
    mle_eval_mfma_min_n = 11, the streaming kernel's smallest table (one E_up entry per point).  Every table of every sumcheck
    is different, so a table evaluated at another sumcheck's point (batch 3 with three tables: a wrong blockIdx / G) gives
    another value than the prover's."""
    name, M, terms = structure
    T = _random_tables(batch * M, n, 16100 + 97 * n + 7 * len(name) + batch)
    try:
        if n == 11:
            ctx.set_option("mle_eval_mfma_min_n", 11)
        with Resident(ctx, T) as d:
            C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, batch)
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, R)
            assert _triples(res) == [ACCEPTED] * batch
            assert res[4].shape == (batch, M, 4) and res[4].tobytes() == E.tobytes()      # the prover's out_evals
            proved = res[3]
            if name in ("AB-AB",):
                assert not proved.any()
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, R, claims=proved)
            assert _triples(res) == [ACCEPTED] * batch and res[4].tobytes() == E.tobytes()
    finally:
        _reset(ctx)


# ---- b. the grouped evaluation against the ungrouped one -------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 5, 8])
@pytest.mark.parametrize("n", [5, 11, 12, 13, 16])
def test_grouped_evaluation_is_the_ungrouped_one_bit_for_bit(ctx, n, M):
    """out_evals (M tables per point, the point's weights built once) against gkr_mle_eval_batch_device on the same resident tables
    with each point repeated M times (every table on its own).  n = 11 with mle_eval_mfma_min_n = 11, 13 and 16: the streaming
    kernel; n = 5 and 12: one block per table."""
    batch = 3
    terms = [(1, (m,)) for m in range(M)]                                    # the sum of the tables: any structure does
    T = _random_tables(batch * M, n, 16300 + 10 * n + M)
    try:
        if n == 11:
            ctx.set_option("mle_eval_mfma_min_n", 11)
        with Resident(ctx, T) as d:
            C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, batch)
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, R)
            points = np.ascontiguousarray(np.repeat(R, M, axis=0))
            assert points.shape == (batch * M, n, 4)
            alone = ctx.mle_eval_batch_device(d, n, batch * M, points)
        assert _triples(res) == [ACCEPTED] * batch
        assert res[4].reshape(batch * M, 4).tobytes() == alone.tobytes()
        assert alone.tobytes() == E.tobytes()
        assert len({bytes(x) for x in alone}) == batch * M                   # (all different: a mixed-up table or point would show)
    finally:
        _reset(ctx)


# ---- c. the exhaustive sweep --------------------------------------------------------------------------------------------------------------
def _run_sweep(ctx, tables, n, terms, proof, r, evals, claim, with_claim, positions=None, settings=((0, 0, 0),), rows=None, launches=None):
    """One batch: every case of the transcript's sweep.  settings: (mle_eval_mfma_min_n, verify_device_hash_min,
    verify_workspace_mb).  rows: keep the slot, r and len cases of these rows only.  launches: a list that receives the
    evaluation's launch count of every call (the context is profiling).  -> (sweep, L, results)."""
    M, D = 1 + max(m for _, idx in terms for m in idx), sop_degree(terms)
    C, L, R = arrays_of(proof, r, D)
    assert point_sees(R, range(1 << n) if positions is None else positions)
    sweep = cases(C, L, R, evals, terms, with_claim, table_positions=positions)
    if rows is not None:
        sweep = [c for c in sweep if c.what in ("honest", "claim", "table") or c.index[0] in rows]
    T1 = (tables if isinstance(tables, np.ndarray) else _limbs_of_tables(tables)).reshape(M, 1 << n, 4)
    T, Cb, Lb, Rb, cl = build_batch(T1, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
    want = [c.verdict for c in sweep]
    results = []
    with Resident(ctx, T) as d:
        try:
            for form, hash_min, mb in settings:
                ctx.set_option("mle_eval_mfma_min_n", form)
                ctx.set_option("verify_device_hash_min", hash_min)
                ctx.set_option("verify_workspace_mb", mb)
                if launches is not None:
                    ctx.profile_reset()
                res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, len(sweep), Cb, Lb, Rb, claims=cl)
                if launches is not None:
                    launches.append(ctx.profile_get("mle_eval")["launches"])
                diff = _first_difference(_triples(res), want)
                assert diff is None, (n, terms, with_claim, (form, hash_min, mb), sweep[diff[0]], diff)
                results.append(res)
        finally:
            _reset(ctx)
    for res in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(res, results[0]))     # values and sums too
    # out_evals / out_claims: zero exactly for the transcripts that fail checks 1 and 2
    bad = np.array([v[2] in (SHAPE, NON_CANONICAL) for v in want])
    assert not results[0][4][bad].any() and not results[0][3][bad].any()
    assert np.array_equal(results[0][4][0], to_limbs(evals)) and np.array_equal(results[0][4][-1], to_limbs(evals))   # the honest copies
    return sweep, L, results


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_the_golden_cases(ctx, sop_cases, with_claim):
    for c in sop_cases:
        proof, r, evals = sop_sumcheck(c["tables"], c["terms"], c["n"])
        assert proof == c["proof"] and r == c["r"]
        sweep, _, _ = _run_sweep(ctx, c["tables"], c["n"], c["terms"], proof, r, evals, c["claim"], with_claim, settings=BOTH_HASH_SIDES)
        assert_sweep_is_sharp(sweep, evals)


def _proved_on_the_device(ctx, tables, n, terms):
    """-> (proof, r, evals) of one sumcheck as the device proves it."""
    D = sop_degree(terms)
    with Resident(ctx, _limbs_of_tables(tables)) as d:
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, len(tables), terms, 1)
    proof = [from_limbs(C[0, j])[D + 1 - int(L[0, j]):] for j in range(n)]
    return proof, from_limbs(R[0]), from_limbs(E[0])


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
@pytest.mark.parametrize("structure", STRUCTURES, ids=[s[0] for s in STRUCTURES])
def test_tamper_sweep_over_a_device_proved_transcript(ctx, structure, with_claim):
    """n = 4, random tables, hashes on the host and on the device.  Without cancellation the sweep is sharp (a condition on the
    inputs, asserted); AB-AB accepts every change of a table."""
    name, M, terms = structure
    n = 4
    rng = random.Random(16400 + len(name))
    tables = [factor("random", n, rng) for _ in range(M)]
    proof, r, evals = _proved_on_the_device(ctx, tables, n, terms)
    sweep, _, _ = _run_sweep(ctx, tables, n, terms, proof, r, evals, sop_claim(tables, terms), with_claim, settings=BOTH_HASH_SIDES)
    if name == "AB-AB":
        assert proof == [[0]] * n and all(table_verdicts(sweep, m) == {ACCEPTED} for m in range(M))
    else:
        assert_sweep_is_sharp(sweep, evals)


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_behind_a_zero_cofactor(ctx, with_claim):
    """AB - AC with B == C: every vector [0]; a change of A is accepted (its cofactor e_B - e_C is zero), one of B or C is seen."""
    M, terms = _structure("AB-AC")
    n = 4
    rng = random.Random(16450)
    tables = [factor("random", n, rng) for _ in range(2)]
    tables.append(list(tables[1]))
    proof, r, evals = _proved_on_the_device(ctx, tables, n, terms)
    assert proof == [[0]] * n and evals[0] != 0 and evals[1] == evals[2]
    sweep, _, _ = _run_sweep(ctx, tables, n, terms, proof, r, evals, 0, with_claim, settings=BOTH_HASH_SIDES)
    assert table_verdicts(sweep, 0) == {ACCEPTED}
    assert table_verdicts(sweep, 1) == table_verdicts(sweep, 2) == {(False, n, EVALUATION)}


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
@pytest.mark.parametrize("kinds", [("indep_middle", "random", "random"), ("random", "indep_last", "indep_last"),
                                   ("indep_first", "indep_first", "indep_first")], ids=["A", "B_and_C_last", "all_first"])
def test_tamper_sweep_over_transcripts_with_short_rows(ctx, kinds, with_claim):
    """AB - C with tables that ignore a variable: rows shorter than D + 1 in a middle, the last and the first round -- every unused
    slot changed (never read: accepted), every longer length (CHALLENGE), every shorter one."""
    M, terms = _structure("AB-C")
    n = 4
    rng = random.Random(16480 + len(kinds[0]))
    tables = [factor(k, n, rng) for k in kinds]
    proof, r, evals = _proved_on_the_device(ctx, tables, n, terms)
    assert (proof, r, evals) == sop_sumcheck(tables, terms, n)
    sweep, L, _ = _run_sweep(ctx, tables, n, terms, proof, r, evals, sop_claim(tables, terms), with_claim, settings=BOTH_HASH_SIDES)
    assert_sweep_is_sharp(sweep, evals)
    assert_sweep_reaches_short_rows(sweep, L, 2)


# ---- d. other terms than the prover's -----------------------------------------------------------------------------------------------------
def test_the_verifier_given_other_terms_than_the_provers(ctx):
    """5AB + 7BC + 11A at n = 8: the transcript is checked against the terms the VERIFIER is given.  Coefficient c_k + 1 moves the
    sum by prod_j e_t(k,j) (non-zero here, asserted); a swapped table index moves it too; a coefficient equal to the modulus is
    GKR_ERR_NON_CANONICAL."""
    M, terms = _structure("5AB+7BC+11A")
    n = 8
    T = _random_tables(M, n, 16500)
    with Resident(ctx, T) as d:
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, 1)
        evals = from_limbs(E[0])
        assert _triples(ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, 1, C, L, R)) == [ACCEPTED]
        for k, (c, idx) in enumerate(terms):
            moved = 1
            for m in idx:
                moved = moved * evals[m] % P
            assert moved != 0
            other = list(terms)
            other[k] = ((c + 1) % P, idx)
            assert _triples(ctx.verify_sumcheck_sop_batch_device(d, n, M, other, 1, C, L, R)) == [(False, n, EVALUATION)], k
        for other in ([(5, (0, 2)), (7, (1, 2)), (11, (0,))], [(5, (0, 1)), (7, (1, 2)), (11, (1,))], [(5, (0, 1)), (7, (2, 2)), (11, (0,))],
                      [(7, (0, 1)), (5, (1, 2)), (11, (0,))]):
            assert sop_eval(evals, other) != sop_eval(evals, terms)
            assert _triples(ctx.verify_sumcheck_sop_batch_device(d, n, M, other, 1, C, L, R)) == [(False, n, EVALUATION)], other
        same = [(7, (2, 1)), (11, (0,)), (5, (1, 0))]                        # the same polynomial written differently
        assert _triples(ctx.verify_sumcheck_sop_batch_device(d, n, M, same, 1, C, L, R)) == [ACCEPTED]
        # a coefficient equal to the modulus: the call fails, nothing is written
        arr, coeffs, _ = Context._sop_terms(terms, M)
        coeffs[1] = R_LIMBS
        accept, rnd, check = np.full(1, 7, dtype=np.int32), np.full(1, 9, dtype=np.uint32), np.full(1, 9, dtype=np.uint32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = N.lib().gkr_sumcheck_sop_verify_batch_device(ctx._h, d, n, M, ctypes.cast(arr, ctypes.c_void_p), ptr(coeffs), len(terms), 1, None,
                                                          ptr(C), ptr(L), ptr(R), ptr(accept), ptr(rnd), ptr(check), None, None)
        assert rc == N.GKR_ERR_NON_CANONICAL and (int(accept[0]), int(rnd[0]), int(check[0])) == (7, 9, 9)
    # the host form: the same for a coefficient, and for a table entry
    tables = [from_limbs(T[m << n:(m + 1) << n]) for m in range(M)]
    proof = [from_limbs(C[0, j])[3 - int(L[0, j]):] for j in range(n)]
    assert ctx.verify_sumcheck_sop(tables, terms, proof, from_limbs(R[0])) == ACCEPTED
    Th = T.copy()
    a1, r1, c1 = ctypes.c_int(7), ctypes.c_uint32(9), ctypes.c_uint32(9)
    out = (ctypes.byref(a1), ctypes.byref(r1), ctypes.byref(c1))
    rc = N.lib().gkr_sumcheck_sop_verify(ctx._h, ptr(Th), n, M, ctypes.cast(arr, ctypes.c_void_p), ptr(coeffs), len(terms), None, ptr(C[0]),
                                         ptr(L[0]), ptr(R[0]), *out)
    assert rc == N.GKR_ERR_NON_CANONICAL and (a1.value, r1.value, c1.value) == (7, 9, 9)
    arr, coeffs, _ = Context._sop_terms(terms, M)
    Th[(M << n) - 1] = R_LIMBS
    rc = N.lib().gkr_sumcheck_sop_verify(ctx._h, ptr(Th), n, M, ctypes.cast(arr, ctypes.c_void_p), ptr(coeffs), len(terms), None, ptr(C[0]),
                                         ptr(L[0]), ptr(R[0]), *out)
    assert rc == N.GKR_ERR_NON_CANONICAL and (a1.value, r1.value, c1.value) == (7, 9, 9)
    rc = N.lib().gkr_sumcheck_sop_verify(ctx._h, ptr(T), n, M, ctypes.cast(arr, ctypes.c_void_p), ptr(coeffs), len(terms), None, ptr(C[0]),
                                         ptr(L[0]), ptr(R[0]), *out)
    assert rc == 0 and (a1.value, r1.value, c1.value) == (1, 0, 0)


# ---- e. one term is the product verifier --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_one_term_gives_the_product_verifiers_outputs_byte_for_byte(ctx, degree, with_claim):
    """The product sweep's batch (honest and tampered copies of every kind) through both entry points on the same arrays."""
    n = 4
    terms = [(1, tuple(range(degree)))]
    rng = random.Random(16600 + degree)
    tables = [factor(k, n, rng) for k in ("random", "indep_last", "random")[:degree]]
    proof, r, evals = _proved_on_the_device(ctx, tables, n, terms)
    C, L, R = arrays_of(proof, r, degree)
    sweep = product_cases(C, L, R, evals, with_claim)
    claim = to_limbs([sop_claim(tables, terms)])[0] if with_claim else None
    T, Cb, Lb, Rb, cl = build_batch(_limbs_of_tables(tables).reshape(degree, 1 << n, 4), C, L, R, claim, sweep)
    with Resident(ctx, T) as d:
        want = ctx.verify_sumcheck_product_batch_device(d, n, degree, len(sweep), Cb, Lb, Rb, claims=cl)
        got = ctx.verify_sumcheck_sop_batch_device(d, n, degree, terms, len(sweep), Cb, Lb, Rb, claims=cl)
    assert _triples(want) == [c.verdict for c in sweep]
    assert {v[2] for v in _triples(want)} >= {0, SHAPE, NON_CANONICAL, CHALLENGE, EVALUATION}
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes()


# ---- f. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [11, 13])
def test_options_do_not_move_verdicts(ctx, n):
    """ABC - AD (four tables): honest and tampered copies of one transcript in one batch -- tampers of every kind at three rounds,
    table entries at entry 0, at the last entry and in two other of the streaming kernel's 32 source streams, in every table.
    mle_eval_mfma_min_n = 11 (the streaming kernel) against 24 (one block per table), hashes on the host and on the device,
    verify_workspace_mb = 1 against the default: with the streaming kernel a sumcheck's share of the workspace is about 150 KB, so
    1 MiB holds 7 of them and the batch is several chunks (the launch count of the evaluation says so).  All results identical."""
    M, terms = _structure("ABC-AD")
    count = 1 << n
    T = _random_tables(M, n, 16700 + n)
    with Resident(ctx, T) as d:
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, 1)
        proved = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, 1, C, L, R)[3]
    S = count >> 5
    positions = [0, 5 * S + 1, 17 * S + S - 1, count - 1]
    proof = [from_limbs(C[0, j])[4 - int(L[0, j]):] for j in range(n)]
    evals = from_limbs(E[0])
    settings = [(form, hash_min, mb) for form in (11, 24) for hash_min in (-1, 1) for mb in (0, 1)]
    chunks = []
    try:
        ctx.profile(True)
        sweep, _, results = _run_sweep(ctx, T, n, terms, proof, from_limbs(R[0]), evals, value(proved[0]), True, positions=positions,
                                       settings=settings, rows={0, n // 2, n - 1}, launches=chunks)
    finally:
        ctx.profile(False)
        _reset(ctx)
    assert_sweep_is_sharp(sweep, evals)
    assert {c.verdict[2] for c in sweep} >= {0, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, EVALUATION}
    assert len(results) == len(chunks) == 8 and len(sweep) > 14
    for i, (form, hash_min, mb) in enumerate(settings):
        if mb == 0:
            assert chunks[i] == 1, (settings[i], chunks)
        elif form == 11:
            assert chunks[i] == -(-len(sweep) // 7) > 1, (settings[i], chunks, len(sweep))
    assert results[0][4][0].tobytes() == E[0].tobytes()


# ---- g. the chunk cap -----------------------------------------------------------------------------------------------------------------------
def test_chunk_cap_keeps_the_table_index_inside_the_grid(ctx):
    """n = 2, AB - C, batch = 65535: the workspace is no limit, so a chunk is 32768 / 3 = 10922 sumchecks -- no multiple of
    anything -- and the batch is seven chunks.  Every 997th transcript has one challenge + 1."""
    M, terms = _structure("AB-C")
    n, batch = 2, 65535
    T = _random_tables(batch * M, n, 16800)
    with Resident(ctx, T) as d:
        C, L, R, E = ctx.sumcheck_sop_batch_device(d, n, M, terms, batch)
        Rb = R.copy()
        want = [ACCEPTED] * batch
        for b in range(0, batch, 997):
            j = (b // 997) % n
            Rb[b, j] = limbs((value(R[b, j]) + 1) % P)
            want[b] = (False, j, CHALLENGE)
        try:
            ctx.profile(True)
            ctx.profile_reset()
            res = ctx.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, Rb)
            launches = ctx.profile_get("mle_eval")["launches"]
        finally:
            ctx.profile(False)
    assert launches == 7
    diff = _first_difference(_triples(res), want)
    assert diff is None, diff
    assert want.count(ACCEPTED) == batch - 66
    # the values of the untouched transcripts are the prover's, across every chunk boundary
    ok = np.array([w == ACCEPTED for w in want])
    assert res[4][ok].tobytes() == E[ok].tobytes()


# ---- h. offsets past 4 GiB --------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def test_offsets_past_four_gib():
    """AB - C, n = 24, batch 3: nine tables of 512 MiB; the last sumcheck's last table starts at byte 2^32.  Filled table by table
    as test_gpu_product_verify.py::test_offsets_past_four_gib fills its tables; proved on the device, accepted; then the last entry
    of the last table changed."""
    M, terms = _structure("AB-C")
    n, batch = 24, 3
    size = 32 << n
    assert (batch * M - 1) * size == 1 << 32
    if _free_bytes() < int(1.75 * batch * M * size):
        pytest.skip("not enough free device memory for nine tables of 2^24 entries")
    with Context(0) as c:                                         # (its own context: the prover's workspace goes with it)
        try:
            d = c.alloc(batch * M * size)
        except Exception as e:                                     # the allocation is refused
            pytest.skip("nine tables of 2^24 entries could not be allocated: %s" % e)
        try:
            for t in range(batch * M):
                c.fill_table(ctypes.c_void_p(d.value + t * size), 1 << n, 9100 + t)
            C, L, R, E = c.sumcheck_sop_batch_device(d, n, M, terms, batch)
            res = c.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, R)
            assert _triples(res) == [ACCEPTED] * batch and res[4].tobytes() == E.tobytes()
            at = ctypes.c_void_p(d.value + batch * M * size - 32)
            old = c.download(at, (1, 4))
            c.upload(at, limbs((value(old[0]) + 1) % P)[None])
            res = c.verify_sumcheck_sop_batch_device(d, n, M, terms, batch, C, L, R)
            assert _triples(res) == [ACCEPTED] * (batch - 1) + [(False, n, EVALUATION)]
            keep = np.ones((batch, M), dtype=bool)
            keep[batch - 1, M - 1] = False
            assert np.array_equal(res[4][keep], E[keep]) and not np.array_equal(res[4][batch - 1, M - 1], E[batch - 1, M - 1])
        finally:
            c.free(d)

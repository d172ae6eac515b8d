"""gkr_sumcheck_product_verify_batch_device / gkr_sumcheck_product_verify (csrc/capi_mle_verify.hip, kernels_mle_eval.hip,
kernels_verify_hash.hip):

  a. transcripts proved on the device are accepted -- the golden cases and a shape matrix; the values the verifier computes are the
     prover's out_evals, the proven sums are the tables' own;
  b. the exhaustive single-element tamper sweep of tests/product_verify_sweeps.py, one batch per transcript, against the
     closed-form model (which test_product_verify_host.py holds to the four checks on Python integers);
  c. degree 1 gives the plain verifier's verdicts on the same tables and arrays;
  d. verdicts and values depend neither on where the hashes ran, nor on the chunking, nor on the evaluation kernel;
  e. the four-slot hash kernel at its launch boundaries;
  f. a factor that starts 4 GiB into the tables;
  g. the host-table entry point.

The verifier's own output is never the reference."""

import ctypes
import random

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from mle_verify_sweeps import arrays_of as plain_arrays_of, build_batch as plain_build_batch, cases as plain_cases
from product_model import factor, product_sumcheck
from product_verify_sweeps import (ACCEPTED, CHALLENGE, EVALUATION, NON_CANONICAL, ROUND_SUM, SHAPE, arrays_of, assert_sweep_is_sharp,
                                   assert_sweep_reaches_short_rows, build_batch, cases, point_sees)
from verify_sweeps import R_LIMBS, limbs, value

pytestmark = pytest.mark.gpu
OPTIONS = ("mle_eval_mfma_min_n", "verify_device_hash_min", "verify_workspace_mb")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def product_cases():
    cases_ = load_golden("product_sumcheck.json")["cases"]
    assert len(cases_) == 7
    return [{"n": c["n"], "degree": c["degree"], "tables": [[int(x) for x in t] for t in c["tables"]],
             "proof": [[int(x) for x in g] for g in c["proof"]], "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases_]


def _triples(result):
    return [(bool(a), int(r), int(c)) for a, r, c in zip(result[0], result[1], result[2])]


def _first_difference(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def _reset(ctx):
    for name in OPTIONS:
        ctx.set_option(name, 0)


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


def _limbs_of_groups(groups):
    """groups[b][f]: lists of ints -> (batch * degree * 2^n, 4) limbs in the ABI's order."""
    return np.concatenate([to_limbs(t) for g in groups for t in g])


def _sum_of_products(group):
    total = 0
    for xs in zip(*group):
        v = 1
        for x in xs:
            v = v * x % P
        total += v
    return total % P


def _random_tables(count, n, seed):
    """count tables of 2^n canonical values (below 2^252) as limbs, and as Python integers."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 1 << 63, size=(count << n, 4), dtype=np.uint64)
    T[:, 3] &= np.uint64((1 << 60) - 1)
    return T


# ---- a. proved on the device and accepted ---------------------------------------------------------------------------------------------
def test_golden_cases_proved_on_the_device_are_accepted(ctx, product_cases):
    for c in product_cases:
        n, degree, tables = c["n"], c["degree"], c["tables"]
        with Resident(ctx, _limbs_of_groups([tables])) as d:
            C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, 1)
            assert from_limbs(R[0]) == c["r"]
            claim = to_limbs([c["claim"]])
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, 1, C, L, R, claims=claim)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[3], claim) and np.array_equal(res[4], E)
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, 1, C, L, R)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[3], claim) and np.array_equal(res[4], E)
        # the host-table entry point on the reference's own transcript
        assert ctx.verify_sumcheck_product(tables, c["proof"], c["r"], claim=c["claim"]) == ACCEPTED
        assert ctx.verify_sumcheck_product(tables, c["proof"], c["r"]) == ACCEPTED
        assert ctx.verify_sumcheck_product(tables, c["proof"], c["r"], claim=(c["claim"] + 1) % P) == (False, 0, ROUND_SUM)


MIX = ["random", "indep_first", "all_max", "indep_last", "specials", "bits", "indep_middle", "constant"]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("n", [2, 3, 8, 11, 12, 13, 16])
def test_shapes_proved_on_the_device_are_accepted(ctx, n, degree, batch):
    """n = 12 and 13 straddle the default switch between the one-block and the streaming evaluation kernel; n = 11 runs with
    mle_eval_mfma_min_n = 11, the streaming kernel's smallest table.  Up to n = 8 the factors are of mixed kinds (rows of
    every length), above they are random."""
    if n <= 8:
        rng = random.Random(6100 + 97 * n + 7 * degree + batch)
        groups = [[factor(MIX[(n + 3 * b + 5 * f + degree) % len(MIX)], n, rng) for f in range(degree)] for b in range(batch)]
        T = _limbs_of_groups(groups)
    else:
        T = _random_tables(batch * degree, n, 7000 + 97 * n + 7 * degree + batch)
        flat = from_limbs(T)
        groups = [[flat[(b * degree + f) << n:(b * degree + f + 1) << n] for f in range(degree)] for b in range(batch)]
    sums = to_limbs([_sum_of_products(g) for g in groups])
    try:
        if n == 11:
            ctx.set_option("mle_eval_mfma_min_n", 11)
        with Resident(ctx, T) as d:
            C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R)
            assert _triples(res) == [ACCEPTED] * batch
            assert np.array_equal(res[4], E)                                 # the prover's out_evals
            assert np.array_equal(res[3], sums)                              # the model's sums
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R, claims=sums)
            assert _triples(res) == [ACCEPTED] * batch and np.array_equal(res[4], E)
    finally:
        _reset(ctx)


# ---- b. the exhaustive sweep --------------------------------------------------------------------------------------------------------------
def _run_sweep(ctx, tables, n, degree, proof, r, evals, claim, with_claim, sharp, positions=None, settings=((0, 0, 0),)):
    """One batch: every case of the transcript's sweep.  settings: (mle_eval_mfma_min_n, verify_device_hash_min, verify_workspace_mb)."""
    C, L, R = arrays_of(proof, r, degree)
    assert point_sees(R, range(1 << n) if positions is None else positions)
    sweep = cases(C, L, R, evals, with_claim, table_positions=positions)
    if sharp:
        assert_sweep_is_sharp(sweep, evals)
    T1 = _limbs_of_groups([tables]).reshape(degree, 1 << n, 4)
    T, Cb, Lb, Rb, cl = build_batch(T1, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
    want = [c.verdict for c in sweep]
    results = []
    with Resident(ctx, T) as d:
        try:
            for form, hash_min, mb in settings:
                ctx.set_option("mle_eval_mfma_min_n", form)
                ctx.set_option("verify_device_hash_min", hash_min)
                ctx.set_option("verify_workspace_mb", mb)
                res = ctx.verify_sumcheck_product_batch_device(d, n, degree, len(sweep), Cb, Lb, Rb, claims=cl)
                diff = _first_difference(_triples(res), want)
                assert diff is None, (n, degree, with_claim, (form, hash_min, mb), sweep[diff[0]], diff)
                results.append(res)
        finally:
            _reset(ctx)
    for res in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(res, results[0]))     # values and sums too
    # out_evals / out_claims: zero exactly for the transcripts that fail checks 1 and 2
    bad = np.array([v[2] in (SHAPE, NON_CANONICAL) for v in want])
    assert not results[0][4][bad].any() and not results[0][3][bad].any()
    assert np.array_equal(results[0][4][0], to_limbs(evals)) and np.array_equal(results[0][4][-1], to_limbs(evals))   # the honest copies
    return sweep, L


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_the_golden_cases(ctx, product_cases, with_claim):
    for c in product_cases:
        proof, r, evals = product_sumcheck(c["tables"], c["n"])
        assert proof == c["proof"] and r == c["r"]
        _run_sweep(ctx, c["tables"], c["n"], c["degree"], proof, r, evals, c["claim"], with_claim, sharp=True,
                   settings=((0, -1, 0), (0, 1, 0)))


LENGTH_RULE_COMBOS = [["constant"], ["constant", "indep_last"], ["indep_middle", "bits", "indep_last"], ["constant", "constant", "indep_first"],
                      ["indep_last", "random"]]


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_transcripts_with_short_rows(ctx, with_claim):
    """Constant, indep_last and bits factors: rows shorter than degree + 1 in first, middle and last rounds -- every unused slot
    changed (never read: accepted), every longer length (CHALLENGE), every shorter one -- with the hashes on the host and on the
    device (rows of two slots repacked for the three-slot kernel, rows of four for the four-slot one)."""
    n = 4
    lengths = set()
    for ci, combo in enumerate(LENGTH_RULE_COMBOS):
        rng = random.Random(8200 + ci)
        tables = [factor(k, n, rng) for k in combo]
        assert all(any(t) for t in tables)
        proof, r, evals = product_sumcheck(tables, n)
        claim = _sum_of_products(tables)
        sweep, L = _run_sweep(ctx, tables, n, len(combo), proof, r, evals, claim, with_claim, sharp=True, settings=((0, -1, 0), (0, 1, 0)))
        assert_sweep_reaches_short_rows(sweep, L, len(combo))
        lengths |= {(len(combo), int(x)) for x in L}
    assert {(3, 1), (3, 2), (3, 3), (3, 4), (2, 1), (2, 2), (2, 3), (1, 1)} <= lengths, lengths


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_a_zero_factor_transcript(ctx, with_claim):
    """Every vector [0]: no special case.  A change of the zero factor is seen; a change of another factor hides behind it."""
    n, degree = 3, 3
    rng = random.Random(8300)
    tables = [factor(k, n, rng) for k in ("random", "zero", "bits")]
    proof, r, evals = product_sumcheck(tables, n)
    assert proof == [[0]] * n and evals[1] == 0
    sweep, _ = _run_sweep(ctx, tables, n, degree, proof, r, evals, 0, with_claim, sharp=False, settings=((0, -1, 0), (0, 1, 0)))
    seen = {f: {c.verdict for c in sweep if c.what == "table" and c.index[0] == f} for f in range(degree)}
    assert seen == {0: {ACCEPTED}, 1: {(False, n, EVALUATION)}, 2: {ACCEPTED}}


# ---- c. degree 1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_degree_one_gives_the_plain_verifiers_verdicts(ctx, mle_cases, with_claim):
    assert len(mle_cases) == 9
    for case in mle_cases:
        n, table = case["n"], [int(x) for x in case["table"]]
        C, L, R = plain_arrays_of([[int(x) for x in g] for g in case["proof"]], [int(x) for x in case["r"]])
        sweep = plain_cases(C, L, R, with_claim)
        T, Cb, Lb, Rb, cl = plain_build_batch(to_limbs(table), C, L, R, to_limbs([sum(table)])[0] if with_claim else None, sweep)
        with Resident(ctx, T) as d:
            plain = ctx.verify_sumcheck_batch_device(d, n, len(sweep), Cb, Lb, Rb, claims=cl)
            ours = ctx.verify_sumcheck_product_batch_device(d, n, 1, len(sweep), Cb, Lb, Rb, claims=cl)
        assert _triples(ours) == _triples(plain) == [c.verdict for c in sweep], n
        assert np.array_equal(ours[3], plain[3])


# ---- d. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [9, 20])
def test_chunk_boundaries_fall_between_sumchecks(ctx, batch):
    """n = 13, degree 3: a sumcheck's share of the workspace is about 110 KB, so verify_workspace_mb = 1 holds 9 of them: the
    batch of 9 is one chunk under both settings, the batch of 20 is three (the launch count of the evaluation says so).  The
    last factor of ONE sumcheck tampered, for every sumcheck in turn -- the ones just before and just after a boundary among
    them: only that verdict flips, under both settings, and every value but that factor's stays."""
    n, degree = 13, 3
    count = 1 << n
    T = _random_tables(batch * degree, n, 5150 + batch)
    with Resident(ctx, T) as d:
        try:
            C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
            ctx.profile(True)
            chunks = {}
            honest = {}
            for mb in (0, 1):
                ctx.set_option("verify_workspace_mb", mb)
                ctx.profile_reset()
                honest[mb] = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R)
                chunks[mb] = ctx.profile_get("mle_eval")["launches"]
                assert _triples(honest[mb]) == [ACCEPTED] * batch and np.array_equal(honest[mb][4], E)
            ctx.profile(False)
            assert chunks[0] == 1 and chunks[1] == (3 if batch == 20 else 1), chunks
            assert all(np.array_equal(a, b) for a, b in zip(honest[0], honest[1]))
            for b in range(batch):
                at = ctypes.c_void_p(d.value + (((b * degree + degree - 1) << n) + count - 1) * 32)
                old = ctx.download(at, (1, 4))
                ctx.upload(at, limbs((value(old[0]) + 1) % P)[None])
                want = [ACCEPTED] * batch
                want[b] = (False, n, EVALUATION)
                keep = np.ones((batch, degree), dtype=bool)
                keep[b, degree - 1] = False
                for mb in (0, 1):
                    ctx.set_option("verify_workspace_mb", mb)
                    res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R)
                    assert _triples(res) == want, (b, mb)
                    assert np.array_equal(res[4][keep], E[keep]) and not np.array_equal(res[4][b, degree - 1], E[b, degree - 1])
                ctx.upload(at, old)
        finally:
            ctx.profile(False)
            _reset(ctx)


@pytest.mark.parametrize("n", [11, 13])
def test_either_evaluation_kernel_and_either_hash_side_give_the_same(ctx, n):
    """mle_eval_mfma_min_n = 11 (the streaming kernel) against 24 (one block per table), hashes on the host and on the device:
    tampers of every kind at three rounds, table entries at entry 0, at the last entry and in two other of the streaming
    kernel's 32 source streams, in every factor."""
    degree, count = 3, 1 << n
    T = _random_tables(degree, n, 4400 + n)
    flat = from_limbs(T)
    tables = [flat[f << n:(f + 1) << n] for f in range(degree)]
    with Resident(ctx, T) as d:
        C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, 1)
    S = count >> 5
    positions = [0, 5 * S + 1, 17 * S + S - 1, count - 1]
    rows = {0, n // 2, n - 1}
    C1, L1, R1, evals = C[0], L[0], R[0], from_limbs(E[0])
    assert point_sees(R1, positions)
    full = cases(C1, L1, R1, evals, True, table_positions=positions)
    assert_sweep_is_sharp(full, evals)
    sweep = [c for c in full if c.what in ("honest", "claim", "table") or c.index[0] in rows]
    claim = _sum_of_products(tables)
    Tb, Cb, Lb, Rb, cl = build_batch(T.reshape(degree, count, 4), C1, L1, R1, to_limbs([claim])[0], sweep)
    want = [c.verdict for c in sweep]
    assert {v[2] for v in want} >= {0, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, EVALUATION}
    results = []
    with Resident(ctx, Tb) as d:
        try:
            for form in (11, 24):
                for hash_min in (-1, 1):
                    ctx.set_option("mle_eval_mfma_min_n", form)
                    ctx.set_option("verify_device_hash_min", hash_min)
                    res = ctx.verify_sumcheck_product_batch_device(d, n, degree, len(sweep), Cb, Lb, Rb, claims=cl)
                    diff = _first_difference(_triples(res), want)
                    assert diff is None, (form, hash_min, sweep[diff[0]], diff)
                    results.append(res)
        finally:
            _reset(ctx)
    for res in results[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(res, results[0]))
    assert np.array_equal(results[0][4][0], E[0]) and np.array_equal(results[0][3][0], to_limbs([claim])[0])


# ---- e. the four-slot hash kernel at its launch boundaries ------------------------------------------------------------------------------------
# kinds per sumcheck whose transcripts have rows of length 4, 3, 2, 1 (random factors depend on every variable, constant ones on none)
BY_LENGTH = [["random", "random", "random"], ["constant", "random", "random"], ["constant", "constant", "random"],
             ["constant", "constant", "constant"]]


def _expected(batch, shape, non_canonical):
    """Verdicts of honest transcripts with these (transcript, row) tampers: shape comes first, then canonical, each at its first row."""
    want = []
    for b in range(batch):
        sh = [j for t, j in shape if t == b]
        nc = [j for t, j in non_canonical if t == b]
        want.append((False, min(sh), SHAPE) if sh else (False, min(nc), NON_CANONICAL) if nc else ACCEPTED)
    return want


@pytest.mark.parametrize("n,batch", [(2, 1), (7, 1), (2, 4), (3, 3), (13, 5)], ids=["2rows", "7rows", "8rows", "9rows", "65rows"])
def test_four_slot_hash_kernel_boundaries(ctx, n, batch):
    """Degree 3 with the hashes forced onto the device: k_verify_hash<4>, eight rows per wave.  batch * n = 2 (the fewest the ABI
    admits: n >= 2), 7, 8, 9 and 65 rows -- part of a wave, a whole one, one row and one row past eight blocks' worth;
    lengths 1 .. 4 mixed inside one wave (the 8-row case); then, in one call, a non-canonical UNUSED leading slot (accepted, its neighbours
    unaffected), a non-canonical used slot, and the lengths 0 and 5, each in another transcript or row."""
    degree, W = 3, 4
    rng = random.Random(8800 + 10 * n + batch)
    groups = [[factor(k, n, rng) for k in BY_LENGTH[(b + (0 if batch > 1 else 1)) % 4]] for b in range(batch)]
    with Resident(ctx, _limbs_of_groups(groups)) as d:
        try:
            ctx.set_option("verify_device_hash_min", 1)
            ctx.profile(True)
            ctx.profile_reset()
            C, L, R, E = ctx.sumcheck_product_batch_device(d, n, degree, batch)
            flat = L.reshape(-1)
            assert flat.shape[0] == batch * n
            assert any(int(x) < W for x in flat)
            if batch >= 4:                                                   # 8 rows: all four lengths in the one wave; 65 rows:
                mixed = 4 if flat.shape[0] == 8 else 2                       # a transcript's 13 rows are of one length, a wave spans two
                assert any(len(set(flat[a:a + 8].tolist())) >= mixed for a in range(0, flat.shape[0], 8)), "lengths mixed inside one wave"
                assert set(flat.tolist()) == {1, 2, 3, 4}
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, C, L, R)
            assert ctx.profile_get("verify_hash")["launches"] == 1           # the kernel ran
            assert _triples(res) == [ACCEPTED] * batch and np.array_equal(res[4], E)
            # the tampers, each in another transcript where there are several, each in another row where there is one
            short = [(b, j) for b in range(batch) for j in range(n) if L[b, j] < W]
            b0, j0 = short[0]
            others = [b for b in range(batch) if b != b0] or [b0]
            (b1, j1), (b2, j2), (b3, j3) = [(others[i % len(others)], (j0 + 1 + i) % n) for i in range(3)]
            assert (b2, j2) != (b3, j3)
            Cb, Lb = C.copy(), L.copy()
            Cb[b0, j0, 0] = limbs((1 << 256) - 1)                            # an unused leading slot: never read
            Cb[b1, j1, W - 1] = R_LIMBS                                      # a used slot (the last one always is)
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, Cb, Lb, R)
            want = _expected(batch, shape=[], non_canonical=[(b1, j1)])
            assert _triples(res) == want, ((b0, j0), (b1, j1))
            Lb[b2, j2], Lb[b3, j3] = 0, 5
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, Cb, Lb, R)
            want = _expected(batch, shape=[(b2, j2), (b3, j3)], non_canonical=[(b1, j1)])
            assert _triples(res) == want, ((b0, j0), (b1, j1), (b2, j2), (b3, j3))
            if batch > 3:
                assert want[b0] == ACCEPTED and want.count(ACCEPTED) == batch - 3
            ok = np.array([w == ACCEPTED for w in want])
            assert np.array_equal(res[4][ok], E[ok]) and not res[4][~ok].any()
            # the unused slot alone: accepted, and every other transcript with it
            Cb, Lb = C.copy(), L.copy()
            Cb[b0, j0, 0] = R_LIMBS
            res = ctx.verify_sumcheck_product_batch_device(d, n, degree, batch, Cb, Lb, R)
            assert _triples(res) == [ACCEPTED] * batch and np.array_equal(res[4], E)
        finally:
            ctx.profile(False)
            _reset(ctx)


# ---- f. offsets past 4 GiB --------------------------------------------------------------------------------------------------------------------
def _free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


def test_offsets_past_four_gib(ctx):
    """n = 26, degree 3, batch 1: three tables of 2 GiB; the third factor starts at byte 2^32.  Filled table by table as
    test_gpu_product.py::test_offsets_past_four_gib fills its tables; proved on the device, accepted; then the last entry of
    the last factor changed."""
    n, degree = 26, 3
    size = 32 << n
    assert (degree - 1) * size == 1 << 32
    if _free_bytes() < int(1.75 * degree * size):
        pytest.skip("not enough free device memory for three tables of 2^26 entries")
    with Context(0) as c:                                         # (its own context: the 3 GiB of the prover's workspace go with it)
        d = c.alloc(degree * size)
        try:
            for t in range(degree):
                c.fill_table(ctypes.c_void_p(d.value + t * size), 1 << n, 9000 + t)
            C, L, R, E = c.sumcheck_product_batch_device(d, n, degree, 1)
            res = c.verify_sumcheck_product_batch_device(d, n, degree, 1, C, L, R)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[4], E)
            at = ctypes.c_void_p(d.value + degree * size - 32)
            old = c.download(at, (1, 4))
            c.upload(at, limbs((value(old[0]) + 1) % P)[None])
            res = c.verify_sumcheck_product_batch_device(d, n, degree, 1, C, L, R)
            assert _triples(res) == [(False, n, EVALUATION)]
            assert np.array_equal(res[4][0, :2], E[0, :2]) and not np.array_equal(res[4][0, 2], E[0, 2])
        finally:
            c.free(d)


# ---- g. the host form ---------------------------------------------------------------------------------------------------------------------------
def test_host_form(ctx):
    n, degree = 5, 3
    rng = random.Random(77)
    tables = [factor(k, n, rng) for k in ("random", "indep_last", "specials")]
    proof, r, evals = product_sumcheck(tables, n)
    claim = _sum_of_products(tables)
    assert ctx.verify_sumcheck_product(tables, proof, r, claim=claim) == ACCEPTED
    assert ctx.verify_sumcheck_product(tables, proof, r) == ACCEPTED
    assert ctx.verify_sumcheck_product(tables, proof, [r[0]] + [(r[1] + 1) % P] + r[2:]) == (False, 1, CHALLENGE)
    bad = [list(t) for t in tables]
    bad[2][7] = (bad[2][7] + 1) % P
    assert ctx.verify_sumcheck_product(bad, proof, r, claim=claim) == (False, n, EVALUATION)
    # a table entry = r: GKR_ERR_NON_CANONICAL, nothing written, inputs unchanged
    T = _limbs_of_groups([tables])
    C, L, R = arrays_of(proof, r, degree)
    T[(2 << n) - 1] = R_LIMBS
    before = [a.copy() for a in (T, C, L, R)]
    accept, rnd, check = ctypes.c_int(7), ctypes.c_uint32(9), ctypes.c_uint32(9)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = N.lib().gkr_sumcheck_product_verify(ctx._h, ptr(T), n, degree, None, ptr(C), ptr(L), ptr(R), ctypes.byref(accept), ctypes.byref(rnd),
                                             ctypes.byref(check))
    assert rc == N.GKR_ERR_NON_CANONICAL and (accept.value, rnd.value, check.value) == (7, 9, 9)
    assert all(np.array_equal(a, b) for a, b in zip((T, C, L, R), before))
    T[(2 << n) - 1] = to_limbs([tables[1][-1]])[0]
    rc = N.lib().gkr_sumcheck_product_verify(ctx._h, ptr(T), n, degree, None, ptr(C), ptr(L), ptr(R), ctypes.byref(accept), ctypes.byref(rnd),
                                             ctypes.byref(check))
    assert rc == 0 and (accept.value, rnd.value, check.value) == (1, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip((C, L, R), before[1:]))

"""gkr_sumcheck_mle_verify_batch_device / gkr_sumcheck_mle_verify (csrc/capi_mle_verify.hip, kernels_mle_eval.hip):

  a. honest transcripts of the device prover are accepted -- they are pinned to the oracle by test_gpu_parity.py, so acceptance is
     an exact-equality check of T(r) -- with the table's sum as the claim and without a claim;
  b. the exhaustive single-element tamper sweep of tests/mle_verify_sweeps.py over the nine golden cases, tampered and honest
     transcripts mixed in one batch, against the closed-form model (which test_mle_verify_host.py holds to the relations on
     Python integers);
  c. the same verdicts with the hashes on the host and on the device, in several chunks, and with either evaluation kernel;
  d. one table at n = 28 and at n = 30 in a child process (tests/mle_verify_worker.py).

The verifier's own output is never the reference."""

import os
import subprocess
import sys
import time

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from mle_verify_sweeps import (ACCEPTED, CHALLENGE, EVALUATION, LENGTH_RULE_TABLES, ROUND_SUM, arrays_of, assert_sweep_reaches_short_rows,
                               build_batch, cases, eq_weight)
from verify_sweeps import limbs, value

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _triples(result):
    accept, rnd, check, _ = result
    return [(bool(a), int(r), int(c)) for a, r, c in zip(accept, rnd, check)]


def _first_difference(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def _verify_tables(ctx, T, n, C, L, R, claims=None):
    """Upload tables (B, 2^n, 4), verify, free."""
    B = T.shape[0]
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        return ctx.verify_sumcheck_batch_device(d, n, B, C, L, R, claims=claims)
    finally:
        ctx.free(d)


# ---- a. honest transcripts -------------------------------------------------------------------------------------------------------
def test_golden_cases_proved_on_the_device_are_accepted(ctx, mle_cases):
    for case in mle_cases:
        n, table = case["n"], [int(x) for x in case["table"]]
        T = to_limbs(table)
        d = ctx.alloc(T.nbytes)
        try:
            ctx.upload(d, T)
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, 1)
            assert from_limbs(R[0]) == [int(x) for x in case["r"]]
            total = to_limbs([sum(table)])
            assert _triples(ctx.verify_sumcheck_batch_device(d, n, 1, C, L, R, claims=total)) == [ACCEPTED]
            res = ctx.verify_sumcheck_batch_device(d, n, 1, C, L, R)
            assert _triples(res) == [ACCEPTED] and np.array_equal(res[3], total)
        finally:
            ctx.free(d)
        # the host-table entry point on what prove_sumcheck returns
        proof, r = ctx.prove_sumcheck(table, n)
        assert ctx.verify_sumcheck(table, proof, r, claim=sum(table) % P) == ACCEPTED
        assert ctx.verify_sumcheck(table, proof, r) == ACCEPTED
        assert ctx.verify_sumcheck(table, proof, r, claim=(sum(table) + 1) % P) == (False, 0, ROUND_SUM)


@pytest.mark.parametrize("batch", [1, 3, 9])
@pytest.mark.parametrize("n", [11, 13, 16, 20])
def test_device_filled_tables_are_accepted(ctx, n, batch):
    """fill_table's tables, `batch` of them in one fill; both evaluation kernels up to n = 16 (one block per table walks the whole
    table: not at 2^20 entries), the default one at n = 20.  The proven sums returned without a claim are accepted as claims."""
    count = batch << n
    d = ctx.alloc(count * 32)
    try:
        ctx.fill_table(d, count, 0xC0FFEE + 100 * n + batch)
        C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
        for form in ([0, 11, 31] if n <= 16 else [0]):
            ctx.set_option("mle_eval_mfma_min_n", form)
            res = ctx.verify_sumcheck_batch_device(d, n, batch, C, L, R)
            assert _triples(res) == [ACCEPTED] * batch, (n, batch, form)
            assert _triples(ctx.verify_sumcheck_batch_device(d, n, batch, C, L, R, claims=res[3])) == [ACCEPTED] * batch
        if n <= 13 and batch == 3:                                           # the proven sum IS the table's sum
            host = ctx.download(d, (count, 4))
            sums = [sum(from_limbs(host[b << n:(b + 1) << n])) % P for b in range(batch)]
            assert from_limbs(res[3]) == sums
    finally:
        ctx.set_option("mle_eval_mfma_min_n", 0)
        ctx.free(d)


def test_length_rule_tables_are_accepted(ctx):
    """The tables of test_mle_length_rule_edge_cases and test_mle_last_variable_dependence_on_streamed_tables: rows of length 1."""
    n13 = 13
    pairs = [(i >> 1) * 7919 + 3 for i in range(1 << n13)]
    one_pair = list(pairs)
    one_pair[5431] += 1
    last = list(pairs)
    last[-1] = 12345
    tables = [([5] * 16, 4), ([i >> 1 for i in range(32)], 5), ([0] * 8, 3), ([1, 1, 2, 2], 2), ([3, 4, 3, 4, 3, 4, 3, 4], 3), ([P - 1] * 64, 6),
              (pairs, n13), (one_pair, n13), (last, n13), ([9] * (1 << n13), n13)]
    short_rows = 0
    for t, n in tables:
        proof, r = ctx.prove_sumcheck(t, n)
        short_rows += sum(len(g) == 1 for g in proof)
        for form in ([0] if n < 11 else [11, 31]):
            ctx.set_option("mle_eval_mfma_min_n", form)
            try:
                assert ctx.verify_sumcheck(t, proof, r, claim=sum(t) % P) == ACCEPTED, (n, form)
                assert ctx.verify_sumcheck(t, proof, r) == ACCEPTED, (n, form)
            finally:
                ctx.set_option("mle_eval_mfma_min_n", 0)
    assert short_rows > 0


# ---- b. the exhaustive sweep -------------------------------------------------------------------------------------------------------
def _golden_sweep(case, with_claim):
    n, table = case["n"], [int(x) for x in case["table"]]
    proof, r = [[int(x) for x in g] for g in case["proof"]], [int(x) for x in case["r"]]
    assert all(eq_weight(r, i) != 0 for i in range(1 << n))                  # no table entry is invisible at this point
    C, L, R = arrays_of(proof, r)
    sweep = cases(C, L, R, with_claim)
    claim = to_limbs([sum(table)])[0] if with_claim else None
    return n, sweep, build_batch(to_limbs(table), C, L, R, claim, sweep)


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_the_golden_cases(ctx, mle_cases, with_claim):
    for ci, case in enumerate(mle_cases):
        n, sweep, (T, C, L, R, cl) = _golden_sweep(case, with_claim)
        got = _triples(_verify_tables(ctx, T, n, C, L, R, claims=cl))
        want = [c.verdict for c in sweep]
        diff = _first_difference(got, want)
        assert diff is None, (ci, n, sweep[diff[0]], diff)


@pytest.mark.parametrize("with_claim", [True, False], ids=["claim", "no_claim"])
def test_tamper_sweep_over_transcripts_with_rows_of_length_one(ctx, with_claim):
    """The golden rows all have two coefficients.  The length-rule tables' transcripts (the oracle's prover) have rows of length 1:
    the full sweep over them, batched, holds every unused slot changed (never read: accepted) and every length 1 -> 2 (CHALLENGE),
    with the hashes on the host and on the device (where the two-slot rows are repacked for the three-slot kernel).  A table of
    pairs at n = 13 takes the same cases through the streaming kernel and through more round vectors than one hash block holds."""
    from oracle import cdense
    n13 = 13
    jobs = [(t, None) for t in LENGTH_RULE_TABLES]
    jobs.append(([(i >> 1) * 7919 + 3 for i in range(1 << n13)], [0, 1, 63, 64, 255, 256, (1 << n13) - 2, (1 << n13) - 1]))
    for table, positions in jobs:
        n = len(table).bit_length() - 1
        T1 = to_limbs(table)
        C, L, R = cdense.sumcheck_mle_raw(T1, n)
        r = from_limbs(R)
        assert all(eq_weight(r, i) != 0 for i in (positions if positions is not None else range(1 << n)))
        sweep = cases(C, L, R, with_claim, table_positions=positions)
        assert_sweep_reaches_short_rows(sweep, L)
        T, Cb, Lb, Rb, cl = build_batch(T1, C, L, R, to_limbs([sum(table)])[0] if with_claim else None, sweep)
        want = [c.verdict for c in sweep]
        d = ctx.alloc(T.nbytes)
        try:
            ctx.upload(d, T)
            for hash_min in (-1, 1):
                ctx.set_option("verify_device_hash_min", hash_min)
                got = _triples(ctx.verify_sumcheck_batch_device(d, n, len(sweep), Cb, Lb, Rb, claims=cl))
                diff = _first_difference(got, want)
                assert diff is None, (n, hash_min, sweep[diff[0]], diff)
        finally:
            ctx.set_option("verify_device_hash_min", 0)
            ctx.free(d)


# ---- c. settings ---------------------------------------------------------------------------------------------------------------------
def test_verdicts_do_not_depend_on_where_the_hashes_ran_or_on_the_chunking(ctx, mle_cases):
    """The largest golden sweep, four times over (more tables than one chunk of verify_workspace_mb = 1 holds), with the hashes on
    the host and on the device."""
    case = max(mle_cases, key=lambda c: c["n"])
    n, sweep, (T, C, L, R, cl) = _golden_sweep(case, True)
    rep = 4
    T, C, L, R, cl = (np.ascontiguousarray(np.concatenate([a] * rep)) for a in (T, C, L, R, cl))
    want = [c.verdict for c in sweep] * rep
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        for hash_min in (-1, 1):
            for mb in (0, 1):
                ctx.set_option("verify_device_hash_min", hash_min)
                ctx.set_option("verify_workspace_mb", mb)
                got = _triples(ctx.verify_sumcheck_batch_device(d, n, T.shape[0], C, L, R, claims=cl))
                assert _first_difference(got, want) is None, (hash_min, mb, _first_difference(got, want))
    finally:
        ctx.set_option("verify_device_hash_min", 0)
        ctx.set_option("verify_workspace_mb", 0)
        ctx.free(d)


@pytest.mark.parametrize("n", [11, 13])
def test_tampers_on_streamed_tables_under_every_setting(ctx, n):
    """Tables large enough for the streaming kernel (device-filled, proven here): every kind of tampering at the first, a middle
    and the last round, table entries at the ends of the table and of its streams and wave tiles; verify_workspace_mb = 1 holds
    fewer of these tables than the batch has, so the batch spans several chunks.  Every combination of hash side, chunking and
    evaluation kernel gives the model's verdicts."""
    count = 1 << n
    d1 = ctx.alloc(count * 32)
    try:
        ctx.fill_table(d1, count, 0xABCD00 + n)
        C, L, R = ctx.sumcheck_mle_batch_device(d1, n, 1)
        table = ctx.download(d1, (count, 4))
    finally:
        ctx.free(d1)
    r = from_limbs(R[0])
    S = count >> 5
    positions = sorted({0, 1, 63, 64, 255, 256, S - 1, S, 31 * S, count - 65, count - 1})
    assert all(eq_weight(r, i) != 0 for i in positions)
    rows = sorted({0, 1, 5, n // 2, n - 2, n - 1})
    sweep = [c for c in cases(C[0], L[0], R[0], True, table_positions=positions) if c.what in ("honest", "claim", "table") or c.index[0] in rows]
    T, Cb, Lb, Rb, cl = build_batch(table, C[0], L[0], R[0], to_limbs([sum(from_limbs(table))])[0], sweep)
    want = [c.verdict for c in sweep]
    assert {v[2] for v in want} >= {0, 1, 2, ROUND_SUM, CHALLENGE, EVALUATION}
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        for form in (11, 31):
            for hash_min in (-1, 1):
                for mb in (0, 1):
                    ctx.set_option("mle_eval_mfma_min_n", form)
                    ctx.set_option("verify_device_hash_min", hash_min)
                    ctx.set_option("verify_workspace_mb", mb)
                    got = _triples(ctx.verify_sumcheck_batch_device(d, n, len(sweep), Cb, Lb, Rb, claims=cl))
                    diff = _first_difference(got, want)
                    assert diff is None, (form, hash_min, mb, sweep[diff[0]], diff)
    finally:
        for name in ("mle_eval_mfma_min_n", "verify_device_hash_min", "verify_workspace_mb"):
            ctx.set_option(name, 0)
        ctx.free(d)


# ---- d. limits -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [28, 30])
def test_one_table_at_the_largest_sizes(n):
    t = time.time()
    try:
        out = subprocess.run([sys.executable, os.path.join(HERE, "mle_verify_worker.py"), str(n)], capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired as e:                   # a child that hung: start nothing more on the card either
        pytest.exit("mle_verify_worker.py %d did not end within %d s:\n%s" % (n, e.timeout, e.stdout), returncode=3)
    print("\nmle_verify_worker %d: %.1f s (child)\n%s" % (n, time.time() - t, out.stdout))
    if out.returncode < 0 or out.returncode in (134, 139):   # a child that faulted or aborted: start nothing more on the card
        pytest.exit("mle_verify_worker.py %d ended by a signal (%d):\n%s" % (n, out.returncode, out.stdout + out.stderr[-4000:]), returncode=3)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr

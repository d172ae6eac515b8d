"""The sumcheck over a product of tables (include/gkr_amd.h, gkr_sumcheck_product*) as far as no device is needed: the symbols,
the argument checks that run before a device is touched, the dense integer model (tests/product_model.py) against the
reference's own Python prover (tests/golden/product_sumcheck.json), against the plain sumcheck's model at degree 1 and against
the term-list prover on mult_poly term lists, and the host verifier gkr_amd.verifier.verify_sumcheck_product."""

import ctypes
import os
import random
import re

import pytest

import gkr_amd
from conftest import load_golden
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P
from gkr_amd.prover import Context
from gkr_amd.verifier import mle_eval, verify_sumcheck_product
from oracle import dense, termlist
from oracle.mimc7 import multi_hash
from product_model import KINDS, constant_tables_transcript, factor, product_sumcheck, product_term_list

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_sumcheck_product_batch_device", "gkr_sumcheck_product"]


@pytest.fixture(scope="module")
def product_cases():
    cases = load_golden("product_sumcheck.json")["cases"]
    assert [(c["n"], c["degree"]) for c in cases] == [(2, 2), (3, 2), (4, 2), (5, 2), (2, 3), (3, 3), (4, 3)]
    return [{"n": c["n"], "degree": c["degree"], "tables": [[int(x) for x in t] for t in c["tables"]],
             "proof": [[int(x) for x in g] for g in c["proof"]], "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases]


def test_both_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+GKR_PRODUCT_MAX_DEGREE\s+3\b", header)
    assert callable(Context.sumcheck_product_batch_device) and callable(Context.prove_sumcheck_product)
    assert callable(gkr_amd.prove_sumcheck_product)
    assert "prove_sumcheck_product" in gkr_amd.__all__ and "verify_sumcheck_product" in gkr_amd.__all__


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    bd = lib.gkr_sumcheck_product_batch_device
    good = [fake, fake, 3, 2, 1, fake, fake, fake, fake]          # ctx, tables, n, degree, batch, coeffs, len, r, evals
    for at in (0, 1, 5, 6, 7):
        args = list(good)
        args[at] = None
        assert bd(*args) == INVALID, at
    for at, bad in ((3, 0), (3, 4), (3, -1), (2, 1), (2, 31), (2, 0), (4, 0), (4, 65536), (4, -1)):
        args = list(good)
        args[at] = bad
        assert bd(*args) == INVALID, (at, bad)
    # batch * degree * 2^n <= 2^30 values: every shape one step over the cap
    for n, degree, batch in ((30, 2, 1), (29, 3, 1), (28, 3, 2), (20, 1, 1025), (16, 3, 5462), (2, 3, 65535 * 4096)):
        args = list(good)
        args[2], args[3], args[4] = n, degree, batch
        assert bd(*args) == INVALID, (n, degree, batch)
    host = lib.gkr_sumcheck_product
    good = [fake, fake, 3, 2, fake, fake, fake, fake]             # ctx, tables, n, degree, coeffs, len, r, evals
    for at in (0, 1, 4, 5, 6):
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    for at, bad in ((3, 0), (3, 4), (2, 1), (2, 31), (2, 30)):    # (n = 30 with two tables is over the cap)
        args = list(good)
        args[at] = bad
        assert host(*args) == INVALID, (at, bad)
    assert not any(word)                                         # nothing was written


def test_model_matches_the_reference_python_prover(product_cases):
    for c in product_cases:
        proof, r, evals = product_sumcheck(c["tables"], c["n"])
        assert proof == c["proof"] and r == c["r"], (c["n"], c["degree"])
        assert evals == [mle_eval(t, r) for t in c["tables"]]
        assert all(len(g) == c["degree"] + 1 for g in proof)      # random tables: full length in every round


def test_model_at_degree_one_is_the_plain_sumcheck(mle_cases):
    assert len(mle_cases) == 9
    for c in mle_cases:
        table = [int(x) for x in c["table"]]
        proof, r, evals = product_sumcheck([table], c["n"])
        assert (proof, r) == dense.sumcheck_mle(table, c["n"])
        assert proof == [[int(x) for x in g] for g in c["proof"]] and r == [int(x) for x in c["r"]]
        assert evals == [mle_eval(table, r)]


def test_model_matches_the_term_list_prover_on_mult_poly():
    """prove_sumcheck (oracle/termlist.py) on g = mult_poly of the factors' extensions, n 2..4, degree 2..3, every kind of factor
    next to every other.  A tuple is skipped only when a factor is the zero table (g is then the empty term list)."""
    rng = random.Random(20261018)
    kinds = KINDS                                                # (a 0/1-valued table is the zero table now and then)
    ran = skipped = 0
    short = set()
    for n in (2, 3, 4):
        for degree in (2, 3):
            combos = [[kinds[(a + i * (b + 1)) % len(kinds)] for i in range(degree)] for a in range(len(kinds)) for b in range(len(kinds))]
            for combo in combos:
                tables = [factor(k, n, rng) for k in combo]
                if any(not any(t) for t in tables):
                    skipped += 1
                    continue
                proof, r, _ = product_sumcheck(tables, n)
                assert (proof, r) == termlist.prove_sumcheck(product_term_list(tables, n), n), (n, combo)
                ran += 1
                short |= {(0 if j == 0 else 2 if j == n - 1 else 1) for j, g in enumerate(proof) if len(g) < degree + 1}
    assert ran >= 300 and skipped <= 0.05 * (ran + skipped), (ran, skipped)
    assert short == {0, 1, 2}                                    # short vectors in first, middle and last rounds


def test_zero_factor_and_constant_tables_in_the_model():
    rng = random.Random(5)
    for n in (2, 4):
        for degree in (1, 2, 3):
            for at in range(degree):
                tables = [factor("zero" if f == at else "random", n, rng) for f in range(degree)]
                proof, r, evals = product_sumcheck(tables, n)
                assert proof == [[0]] * n and evals[at] == 0
            values = [P - 1] * degree
            assert product_sumcheck([[v] * (1 << n) for v in values], n) == constant_tables_transcript(values, n)


def _fixture_transcripts(product_cases):
    for c in product_cases:
        proof, r, evals = product_sumcheck(c["tables"], c["n"])
        yield c, proof, r, evals
    rng = random.Random(77)
    for combo in (["indep_first", "random"], ["indep_middle", "bits", "indep_last"], ["constant", "indep_last"]):
        tables = [factor(k, 4, rng) for k in combo]               # transcripts with short round vectors
        claim = sum(eval_prod(tables, i) for i in range(16)) % P
        proof, r, evals = product_sumcheck(tables, 4)
        yield {"degree": len(combo), "claim": claim}, proof, r, evals


def eval_prod(tables, i):
    v = 1
    for t in tables:
        v = v * t[i] % P
    return v


def test_host_verifier_accepts_the_fixtures_and_rejects_every_single_change(product_cases):
    seen_short = False
    for c, proof, r, evals in _fixture_transcripts(product_cases):
        d, claim = c["degree"], c["claim"]
        assert verify_sumcheck_product(proof, r, evals, d, claim) and verify_sumcheck_product(proof, r, evals, d)
        seen_short |= any(len(g) < d + 1 for g in proof)
        for j, g in enumerate(proof):
            for k in range(len(g)):
                bad = [list(x) for x in proof]
                bad[j][k] = (g[k] + 1) % P
                assert not verify_sumcheck_product(bad, r, evals, d, claim), (j, k)
                assert not verify_sumcheck_product(bad, r, evals, d), (j, k)
            hashes = [multi_hash(x, 0) for x in proof]            # the caller's own hashes stand in for the verifier's
            assert verify_sumcheck_product(proof, r, evals, d, claim, hashes=hashes)
            hashes[j] = (hashes[j] + 1) % P
            assert not verify_sumcheck_product(proof, r, evals, d, claim, hashes=hashes), j
            assert not verify_sumcheck_product(proof, r, evals, d, claim, hashes=hashes[:-1])
            bad_r = list(r)
            bad_r[j] = (r[j] + 1) % P
            assert not verify_sumcheck_product(proof, bad_r, evals, d, claim), j
            for bad_g in ([], [0] * (d + 2 - len(g)) + list(g)):   # lengths 0 and degree + 2 (the same polynomial, zero-padded)
                bad = [list(x) for x in proof]
                bad[j] = bad_g
                assert not verify_sumcheck_product(bad, r, evals, d, claim), (j, len(bad_g))
        for f in range(d):
            bad_e = list(evals)
            bad_e[f] = (evals[f] + 1) % P
            assert not verify_sumcheck_product(proof, r, bad_e, d, claim), f
        assert not verify_sumcheck_product(proof, r, evals, d, (claim + 1) % P)
        assert not verify_sumcheck_product(proof, r, evals[:-1], d, claim) and not verify_sumcheck_product(proof[:-1], r, evals, d, claim)
    assert seen_short

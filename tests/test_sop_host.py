"""The sumcheck over a sum of products of tables (include/gkr_amd.h, gkr_sumcheck_sop*) as far as no device is needed: the
symbols, the argument checks that run before a device is touched, the dense integer model (tests/sop_model.py) against the
term-list prover on add_poly of scaled mult_poly term lists, against the product model with one term, against the reference's own
Python prover (tests/golden/sop_sumcheck.json), and the host verifier gkr_amd.verifier.verify_sumcheck_sop."""

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
from gkr_amd.verifier import mle_eval, verify_sumcheck_sop
from oracle import termlist
from product_model import KINDS, factor, product_sumcheck
from sop_model import STRUCTURES, constant_tables_transcript, sop_claim, sop_degree, sop_eval, sop_sumcheck, sop_term_list

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_sumcheck_sop_batch_device", "gkr_sumcheck_sop"]


def test_both_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"#define\s+GKR_SOP_MAX_TABLES\s+8\b", header) and re.search(r"#define\s+GKR_SOP_MAX_TERMS\s+8\b", header)
    assert (N.GKR_SOP_MAX_TABLES, N.GKR_SOP_MAX_TERMS) == (8, 8) and ctypes.sizeof(N.SopTerm) == 4
    assert callable(Context.sumcheck_sop_batch_device) and callable(Context.prove_sumcheck_sop)
    assert callable(gkr_amd.prove_sumcheck_sop) and callable(gkr_amd.verify_sumcheck_sop)
    assert "prove_sumcheck_sop" in gkr_amd.__all__ and "verify_sumcheck_sop" in gkr_amd.__all__


def _terms(spec):
    arr = (N.SopTerm * len(spec))()
    for k, (degree, idx) in enumerate(spec):
        arr[k].degree = degree
        for j, i in enumerate(idx):
            arr[k].table[j] = i
    return arr


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    ok_terms = _terms([(2, (0, 1)), (1, (2,))])

    def tp(arr):
        return ctypes.cast(arr, ctypes.c_void_p)

    bd = lib.gkr_sumcheck_sop_batch_device
    # ctx, tables, n, n_tables, terms, coeffs, n_terms, batch, out_coeffs, out_len, out_r, out_evals
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, 1, fake, fake, fake, fake]
    for at in (0, 1, 4, 8, 9, 10):
        args = list(good)
        args[at] = None
        assert bd(*args) == INVALID, at
    for at, bad in ((7, 0), (7, 65536), (7, -1), (2, 1), (2, 31), (2, 0), (2, -1), (3, 0), (3, 9), (3, -1), (6, 0), (6, 9), (6, -1)):
        args = list(good)
        args[at] = bad
        assert bd(*args) == INVALID, (at, bad)
    eight = [(1, (m,)) for m in range(8)]
    for spec, n_tables in (([(0, ()), (1, (0,))], 1), ([(4, (0, 0, 0))], 1), ([(255, (0, 0, 0))], 1),      # a term degree outside 1 .. 3
                           ([(2, (0, 3)), (1, (1,)), (1, (2,))], 3), ([(3, (0, 1, 8))] + eight, 8),         # a table index >= n_tables
                           ([(2, (0, 1))], 3), ([(3, (0, 0, 0)), (1, (2,))], 3), (eight[:7], 8)):            # a table no term references
        arr = _terms(spec[:8])
        args = list(good)
        args[3], args[4], args[6] = n_tables, tp(arr), len(spec[:8])
        assert bd(*args) == INVALID, (spec, n_tables)
    # batch * n_tables * 2^n <= 2^30 values: every shape one step over the cap (and the shape at the cap passes these checks:
    # it is not tried, it would reach the context)
    for n, n_tables, batch in ((30, 2, 1), (28, 5, 1), (27, 8, 2), (20, 1, 1025), (16, 3, 5462), (10, 8, 65535 * 4)):
        arr = _terms([(1, (m,)) for m in range(n_tables)])
        args = list(good)
        args[2], args[3], args[4], args[6], args[7] = n, n_tables, tp(arr), n_tables, batch
        assert bd(*args) == INVALID, (n, n_tables, batch)
    host = lib.gkr_sumcheck_sop
    # ctx, tables, n, n_tables, terms, coeffs, n_terms, out_coeffs, out_len, out_r, out_evals
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, fake, fake, fake, fake]
    for at in (0, 1, 4, 7, 8, 9):
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    for at, bad in ((2, 1), (2, 31), (3, 0), (3, 9), (6, 0), (6, 9), (3, 2), (3, 4)):    # (n_tables 2: index 2 is out; 4: table 3 unused)
        args = list(good)
        args[at] = bad
        assert host(*args) == INVALID, (at, bad)
    arr = _terms([(1, (0,)), (1, (1,))])
    args = list(good)
    args[2], args[3], args[4] = 30, 2, tp(arr)                                          # 2 * 2^30 values
    assert host(*args) == INVALID
    assert not any(word)                                                                # nothing was written


def _trials(name, n_tables, n, rng):
    """The tables of a structure's trials: the kinds rotate through the tables so that every kind stands everywhere, and the
    last trial has two tables equal (one table alone: the trial repeats)."""
    for a in range(len(KINDS)):
        yield [factor(KINDS[(a + 3 * m) % len(KINDS)], n, rng) for m in range(n_tables)]
    tables = [factor("random", n, rng) for _ in range(n_tables)]
    tables[-1] = list(tables[-2]) if n_tables > 1 else tables[-1]
    yield tables


def test_model_matches_the_term_list_prover_on_add_poly_of_scaled_products():
    """prove_sumcheck (oracle/termlist.py) on g = add_poly over k of c_k mult_poly(..), n = 2, 3 for every structure and n = 4
    for those of <= 3 tables and degree <= 2.  Where g is the empty term list (the reference panics) the model's transcript is
    all [0]; no case is skipped."""
    rng = random.Random(20261019)
    ran = empty = 0
    short = set()
    for n in (2, 3, 4):
        for name, n_tables, terms in STRUCTURES:
            if n == 4 and (n_tables > 3 or sop_degree(terms) > 2):
                continue
            for tables in _trials(name, n_tables, n, rng):
                proof, r, evals = sop_sumcheck(tables, terms, n)
                g = sop_term_list(tables, terms, n)
                if not g:
                    assert proof == [[0]] * n, (name, n)
                    empty += 1
                else:
                    assert (proof, r) == termlist.prove_sumcheck(g, n), (name, n)
                    ran += 1
                    short |= {(0 if j == 0 else 2 if j == n - 1 else 1) for j, v in enumerate(proof) if len(v) < sop_degree(terms) + 1}
                assert evals == [mle_eval(t, r) for t in tables]
    assert ran >= 100 and empty >= 10, (ran, empty)               # AB-AB is always empty, AB-AC with B = C once per n
    assert short == {0, 1, 2}                                     # short vectors in first, middle and last rounds


def test_one_term_of_coefficient_one_is_the_product_model():
    rng = random.Random(20261020)
    kinds = KINDS + ["zero"]
    ran = 0
    for n in (2, 3, 4):
        for degree in (1, 2, 3):
            for a in range(len(kinds)):
                tables = [factor(kinds[(a + 4 * f) % len(kinds)], n, rng) for f in range(degree)]
                assert sop_sumcheck(tables, [(1, tuple(range(degree)))], n) == product_sumcheck(tables, n), (n, degree, a)
                ran += 1
    assert ran == 81


def test_the_vectorised_model_is_the_model():
    """sop_model.sop_sumcheck_np / sop_claim_np (object arrays; what the GPU tests use from 2^8 entries on) against the plain lists."""
    import numpy as np
    from gkr_amd.field import to_limbs
    from sop_model import limbs_to_object, sop_claim_np, sop_sumcheck_np
    rng = random.Random(20261021)
    for name, n_tables, terms in STRUCTURES:
        for n in (2, 3, 6):
            tables = [factor(KINDS[(n + 3 * m + len(name)) % len(KINDS)], n, rng) for m in range(n_tables)]
            arr = limbs_to_object(np.stack([to_limbs(t) for t in tables]))
            assert arr.shape == (n_tables, 1 << n) and arr.tolist() == tables
            assert sop_sumcheck_np(arr, terms, n) == sop_sumcheck(tables, terms, n), (name, n)
            assert sop_claim_np(arr, terms) == sop_claim(tables, terms), (name, n)


def test_constant_tables_in_the_model():
    for name, n_tables, terms in STRUCTURES:
        values = [P - 1 - m for m in range(n_tables)]
        assert sop_sumcheck([[v] * 8 for v in values], terms, 3) == constant_tables_transcript(values, terms, 3), name


@pytest.fixture(scope="module")
def sop_cases():
    cases = load_golden("sop_sumcheck.json")["cases"]
    assert [(c["name"], c["n"]) for c in cases] == [("AB-C", 2), ("AB-C", 3), ("AB-C", 4), ("eq(AB-C)", 2), ("eq(AB-C)", 3)]
    return [{"name": c["name"], "n": c["n"], "terms": [(int(k), tuple(idx)) for k, idx in c["terms"]],
             "z": [int(x) for x in c["z"]] if c["z"] else None, "tables": [[int(x) for x in t] for t in c["tables"]],
             "proof": [[int(x) for x in g] for g in c["proof"]], "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases]


def test_model_matches_the_reference_python_prover(sop_cases):
    for c in sop_cases:
        proof, r, evals = sop_sumcheck(c["tables"], c["terms"], c["n"])
        assert proof == c["proof"] and r == c["r"], (c["name"], c["n"])
        assert evals == [mle_eval(t, r) for t in c["tables"]]
        assert sop_claim(c["tables"], c["terms"]) == c["claim"]
        assert verify_sumcheck_sop(proof, r, evals, c["terms"], c["claim"])
        if c["z"]:                                                # table 0 is eq(z, .): its entries sum to one, each is a product
            n, z = c["n"], c["z"]
            assert sum(c["tables"][0]) % P == 1
            assert c["tables"][0][1] == (z[n - 1] * _prod((1 - zj) % P for zj in z[:n - 1])) % P


def _prod(xs):
    v = 1
    for x in xs:
        v = v * x % P
    return v


def test_host_verifier_accepts_the_model_and_rejects_every_single_change():
    rng = random.Random(606)
    n = 3
    for name in ("ABC-AD", "5AB+7BC+11A"):
        _, n_tables, terms = next(s for s in STRUCTURES if s[0] == name)
        tables = [factor("random", n, rng) for _ in range(n_tables)]
        claim = sop_claim(tables, terms)
        proof, r, _ = sop_sumcheck(tables, terms, n)
        evals = [mle_eval(t, r) for t in tables]
        assert verify_sumcheck_sop(proof, r, evals, terms, claim) and verify_sumcheck_sop(proof, r, evals, terms)
        for j, g in enumerate(proof):
            for k in range(len(g)):
                bad = [list(x) for x in proof]
                bad[j][k] = (g[k] + 1) % P
                assert not verify_sumcheck_sop(bad, r, evals, terms, claim), (j, k)
                assert not verify_sumcheck_sop(bad, r, evals, terms), (j, k)
            bad_r = list(r)
            bad_r[j] = (r[j] + 1) % P
            assert not verify_sumcheck_sop(proof, bad_r, evals, terms, claim), j
            assert len(g) > 1
            bad = [list(x) for x in proof]
            bad[j] = g[1:]                                        # a dropped leading slot
            assert not verify_sumcheck_sop(bad, r, evals, terms, claim), j
            bad[j] = [0] * (sop_degree(terms) + 2 - len(g)) + list(g)   # D + 2 slots (the same polynomial, zero-padded)
            assert not verify_sumcheck_sop(bad, r, evals, terms, claim), j
        for m in range(n_tables):
            bad_e = list(evals)
            bad_e[m] = (evals[m] + 1) % P
            # (the change shows unless every term with table m has a zero coefficient or a zero among its other factors)
            assert sop_eval(bad_e, terms) != sop_eval(evals, terms)
            assert not verify_sumcheck_sop(proof, r, bad_e, terms, claim), m
        assert not verify_sumcheck_sop(proof, r, evals, terms, (claim + 1) % P)
        assert not verify_sumcheck_sop(proof[:-1], r, evals, terms, claim)
        assert not verify_sumcheck_sop(proof, r, evals[:-1], terms, claim)     # an index of the terms has no eval
    # an eval whose change cannot show: its only term has a zero coefficient
    terms = [(1, (0, 1)), (0, (2,))]
    tables = [factor("random", n, rng) for _ in range(3)]
    proof, r, evals = sop_sumcheck(tables, terms, n)
    assert verify_sumcheck_sop(proof, r, evals, terms)
    assert verify_sumcheck_sop(proof, r, evals[:2] + [(evals[2] + 1) % P], terms)
    assert not verify_sumcheck_sop(proof, r, [(evals[0] + 1) % P] + evals[1:], terms)

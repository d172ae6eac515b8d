"""The product sumcheck's verifier (include/gkr_amd.h, gkr_sumcheck_product_verify*) as far as no device is needed: the symbols,
the argument checks that run before a device is touched, and the closed-form verdict model of tests/product_verify_sweeps.py
against the four checks evaluated one after the other on Python integers -- on the dense model's transcripts
(tests/product_model.py) of every kind of factor, on the reference's own transcripts (tests/golden/product_sumcheck.json) next
to gkr_amd.verifier, and at degree 1 against the plain sumcheck's model (tests/mle_verify_sweeps.py)."""

import ctypes
import os
import random
import re

import pytest

import gkr_amd
import mle_verify_sweeps as plain
from conftest import load_golden
from gkr_amd import _native as N
from gkr_amd import multi_hash
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.prover import Context
from gkr_amd.verifier import mle_eval, verify_sumcheck_product
from product_model import KINDS, factor, product_sumcheck
from product_verify_sweeps import (ACCEPTED, EVALUATION, arrays_of, assert_sweep_is_sharp, assert_sweep_reaches_short_rows, build_batch, cases,
                                   point_sees, reference_verdict, rounds_of)
from verify_sweeps import value

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_sumcheck_product_verify_batch_device", "gkr_sumcheck_product_verify"]

_hashes = {}


def cached_hash(g, key=0):
    k = (tuple(g), key)
    if k not in _hashes:
        _hashes[k] = multi_hash(list(g), key)
    return _hashes[k]


def test_both_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert header.index("gkr_sumcheck_product(") < header.index("gkr_sumcheck_product_verify_batch_device(") < header.index("gkr_mle_eval_batch_device(")
    assert callable(Context.verify_sumcheck_product_batch_device) and callable(Context.verify_sumcheck_product)
    assert "verify_sumcheck_product" in gkr_amd.__all__ and "Context" in gkr_amd.__all__
    assert "verify_sumcheck_product" in Context.prove_sumcheck_product.__doc__
    assert "verify_sumcheck_product_batch_device" in verify_sumcheck_product.__doc__


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    accept, rnd, check = ctypes.c_int(7), ctypes.c_uint32(9), ctypes.c_uint32(9)
    out = [ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check)]
    INVALID = N.GKR_ERR_INVALID
    vb = lib.gkr_sumcheck_product_verify_batch_device
    # ctx, tables, n, degree, batch, claims, coeffs, len, r, accept, failed_round, failed_check, out_claims, out_evals
    good = [fake, fake, 3, 2, 1, fake, fake, fake, fake] + out + [fake, fake]
    for at in (0, 1, 6, 7, 8, 9):                                # ctx, tables, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert vb(*args) == INVALID, at
    for at, bad in ((3, 0), (3, 4), (3, -1), (2, 1), (2, 31), (2, 0), (2, -1), (4, 0), (4, 65536), (4, -1)):
        args = list(good)
        args[at] = bad
        assert vb(*args) == INVALID, (at, bad)
    # batch * degree * 2^n <= 2^30 values: every shape one step over the cap (test_product_host.py's list)
    for n, degree, batch in ((30, 2, 1), (29, 3, 1), (28, 3, 2), (20, 1, 1025), (16, 3, 5462), (2, 3, 65535 * 4096)):
        args = list(good)
        args[2], args[3], args[4] = n, degree, batch
        assert vb(*args) == INVALID, (n, degree, batch)
    host = lib.gkr_sumcheck_product_verify
    good = [fake, fake, 3, 2, fake, fake, fake, fake] + out    # ctx, tables, n, degree, claim, coeffs, len, r, accept, round, check
    for at in (0, 1, 5, 6, 7, 8):                                # ctx, tables, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    for at, bad in ((3, 0), (3, 4), (3, -1), (2, 1), (2, 0), (2, 31), (2, 30)):   # (n = 30 with two tables is over the cap)
        args = list(good)
        args[at] = bad
        assert host(*args) == INVALID, (at, bad)
    args = list(good)
    args[2], args[3] = 29, 3
    assert host(*args) == INVALID
    assert not any(word) and (accept.value, rnd.value, check.value) == (7, 9, 9)          # nothing was written


# ---- the closed-form verdict model ---------------------------------------------------------------------------------------------------
COMBOS = {
    1: [["random"], ["constant"], ["indep_last"], ["bits"], ["zero"], ["indep_first"]],
    2: [["random", "constant"], ["indep_last", "bits"], ["indep_first", "specials"], ["zero", "random"], ["constant", "indep_last"],
        ["indep_middle", "all_max"]],
    3: [["random", "indep_last", "bits"], ["constant", "constant", "indep_middle"], ["all_max", "random", "indep_first"],
        ["random", "zero", "bits"], ["indep_last", "constant", "indep_last"]],
}


def _sweep_against_the_relations(tables, n, degree, proof, r, evals, claim, sharp):
    """Every case of the sweep, with and without a claim: the model's triple equals reference_verdict's."""
    C, L, R = arrays_of(proof, r, degree)
    T = to_limbs([x for t in tables for x in t]).reshape(degree, 1 << n, 4)
    assert point_sees(R, range(1 << n))
    short = any(int(x) < degree + 1 for x in L)
    for with_claim in (True, False):
        sweep = cases(C, L, R, evals, with_claim)
        assert {c.what for c in sweep} == {"honest", "slot", "r", "len", "table"} | ({"claim"} if with_claim else set())
        if sharp:
            assert_sweep_is_sharp(sweep, evals)
        if short:
            assert_sweep_reaches_short_rows(sweep, L, degree)
        Tb, Cb, Lb, Rb, cl = build_batch(T, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
        for e, c in enumerate(sweep):
            cl_e = value(cl[e]) if with_claim else None
            tab_e = [from_limbs(Tb[e, f]) for f in range(degree)]
            assert reference_verdict(tab_e, Cb[e], Lb[e], Rb[e], cl_e, cached_hash) == c.verdict, (n, degree, with_claim, c)
        assert sweep[0].verdict == ACCEPTED and sweep[-1].verdict == ACCEPTED
    return short


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_verdict_model_against_the_relations_on_model_transcripts(degree):
    """n in 2 .. 4, every combination of COMBOS: constant, indep_last, bits and zero factors among them (all of
    product_model.KINDS occur), so rows of every length, and the zero-factor transcripts whose other factors' entries are
    invisible."""
    assert {k for d in COMBOS for combo in COMBOS[d] for k in combo} == set(KINDS) | {"zero"}
    short = zero = 0
    for n in (2, 3, 4):
        for ci, combo in enumerate(COMBOS[degree]):
            rng = random.Random(9100 + 100 * n + 10 * degree + ci)
            tables = [factor(k, n, rng) for k in combo]
            has_zero = any(not any(t) for t in tables)
            assert has_zero == ("zero" in combo), "a bits factor came out as the zero table: another seed"
            proof, r, evals = product_sumcheck(tables, n)
            claim = sum(_prod(tables, i) for i in range(1 << n)) % P
            if has_zero:
                assert proof == [[0]] * n and claim == 0
            short += _sweep_against_the_relations(tables, n, degree, proof, r, evals, claim, sharp=not has_zero)
            zero += has_zero
    assert short and zero == 3


def _prod(tables, i):
    v = 1
    for t in tables:
        v = v * t[i] % P
    return v


def test_zero_factor_hides_the_other_factors_entries():
    """(model) in a zero-factor transcript a change of the ZERO factor is seen, a change of any other factor is accepted."""
    rng = random.Random(31)
    n, degree = 3, 3
    tables = [factor(k, n, rng) for k in ("random", "zero", "bits")]
    proof, r, evals = product_sumcheck(tables, n)
    C, L, R = arrays_of(proof, r, degree)
    sweep = cases(C, L, R, evals, True)
    by_factor = {f: {c.verdict for c in sweep if c.what == "table" and c.index[0] == f} for f in range(degree)}
    assert by_factor == {0: {ACCEPTED}, 1: {(False, n, EVALUATION)}, 2: {ACCEPTED}}


@pytest.fixture(scope="module")
def product_cases():
    cases_ = load_golden("product_sumcheck.json")["cases"]
    assert [(c["n"], c["degree"]) for c in cases_] == [(2, 2), (3, 2), (4, 2), (5, 2), (2, 3), (3, 3), (4, 3)]
    return [{"n": c["n"], "degree": c["degree"], "tables": [[int(x) for x in t] for t in c["tables"]],
             "proof": [[int(x) for x in g] for g in c["proof"]], "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases_]


def test_reference_verdict_on_the_golden_cases_agrees_with_the_host_verifier(product_cases):
    """The reference's own transcripts are accepted; over the sweep, wherever the tampered transcript is still well-formed, the
    accept bit equals verifier.verify_sumcheck_product on the values mle_eval gives for the (tampered) tables."""
    for c in product_cases:
        n, degree, tables = c["n"], c["degree"], c["tables"]
        C, L, R = arrays_of(c["proof"], c["r"], degree)
        evals = [mle_eval(t, c["r"]) for t in tables]
        assert reference_verdict(tables, C, L, R, c["claim"], cached_hash) == ACCEPTED
        assert reference_verdict(tables, C, L, R, None, cached_hash) == ACCEPTED
        assert verify_sumcheck_product(c["proof"], c["r"], evals, degree, c["claim"])
        T = to_limbs([x for t in tables for x in t]).reshape(degree, 1 << n, 4)
        positions = sorted({0, 1, (1 << n) // 2, (1 << n) - 1})
        assert point_sees(R, positions)
        for with_claim in (True, False):
            sweep = cases(C, L, R, evals, with_claim, table_positions=positions)
            assert_sweep_is_sharp(sweep, evals)
            Tb, Cb, Lb, Rb, cl = build_batch(T, C, L, R, to_limbs([c["claim"]])[0] if with_claim else None, sweep)
            compared = 0
            for e, case in enumerate(sweep):
                cl_e = value(cl[e]) if with_claim else None
                tab_e = [from_limbs(Tb[e, f]) for f in range(degree)]
                got = reference_verdict(tab_e, Cb[e], Lb[e], Rb[e], cl_e, cached_hash)
                assert got == case.verdict, (n, degree, with_claim, case)
                if got[2] not in (1, 2):                                    # well-formed: the host verifier can read it
                    r_e = from_limbs(Rb[e])
                    ev_e = [mle_eval(t, r_e) for t in tab_e]
                    assert verify_sumcheck_product(rounds_of(Cb[e], Lb[e]), r_e, ev_e, degree, cl_e) == got[0], (n, degree, case)
                    compared += 1
            assert compared > len(sweep) // 2


def test_degree_one_is_the_plain_verifiers_model(mle_cases):
    """Degree 1 IS the plain sumcheck: on the nine golden plain transcripts and their sweeps (mle_verify_sweeps.cases), this
    file's reference_verdict equals mle_verify_sweeps.reference_verdict, and this file's sweep gives the same verdicts."""
    assert len(mle_cases) == 9
    for case in mle_cases:
        n, table = case["n"], [int(x) for x in case["table"]]
        proof, r = [[int(x) for x in g] for g in case["proof"]], [int(x) for x in case["r"]]
        C, L, R = plain.arrays_of(proof, r)
        C1, L1, R1 = arrays_of(proof, r, 1)
        assert (C == C1).all() and (L == L1).all() and (R == R1).all()
        claim = sum(table) % P
        for with_claim in (True, False):
            sweep = plain.cases(C, L, R, with_claim)
            Tb, Cb, Lb, Rb, cl = plain.build_batch(to_limbs(table), C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
            for e, c in enumerate(sweep):
                cl_e = value(cl[e]) if with_claim else None
                tab_e = from_limbs(Tb[e])
                want = plain.reference_verdict(tab_e, Cb[e], Lb[e], Rb[e], cl_e, cached_hash)
                assert reference_verdict([tab_e], Cb[e], Lb[e], Rb[e], cl_e, cached_hash) == want == c.verdict, (n, with_claim, c)
            ours = cases(C, L, R, [mle_eval(table, r)], with_claim)
            assert [(c.what, c.verdict) for c in ours if c.what != "table"] == [(c.what, c.verdict) for c in sweep if c.what != "table"]
            assert [c.verdict for c in ours if c.what == "table"] == [c.verdict for c in sweep if c.what == "table"]

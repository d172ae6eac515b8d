"""The sum-of-products sumcheck's verifier (include/gkr_amd.h, gkr_sumcheck_sop_verify*) as far as no device is needed: the
symbols, the argument checks that run before a device is touched, and the closed-form verdict model of tests/sop_verify_sweeps.py
against the four checks evaluated one after the other on Python integers -- on the dense model's transcripts (tests/sop_model.py)
of the six shared structures, with one term against the product verifier's model (tests/product_verify_sweeps.py), next to
gkr_amd.verifier.verify_sumcheck_sop, and on the reference's own transcripts (tests/golden/sop_sumcheck.json)."""

import ctypes
import os
import random
import re

import pytest

import product_verify_sweeps as product
from conftest import load_golden
from gkr_amd import _native as N
from gkr_amd import multi_hash
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.prover import Context
from gkr_amd.verifier import mle_eval, verify_sumcheck_sop
from product_model import factor, product_sumcheck
from sop_model import STRUCTURES, sop_claim, sop_degree, sop_eval, sop_sumcheck
from sop_verify_sweeps import (ACCEPTED, EVALUATION, ROUND_SUM, arrays_of, assert_sweep_is_sharp, assert_sweep_reaches_short_rows, build_batch,
                               cases, point_sees, reference_verdict, rounds_of, table_verdicts)
from verify_sweeps import value

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_sumcheck_sop_verify_batch_device", "gkr_sumcheck_sop_verify"]
NO_CANCELLATION = ("AB-C", "ABC-AD", "5AB+7BC+11A", "AA+3B")

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
    assert header.index("gkr_sumcheck_sop(") < header.index("gkr_sumcheck_sop_verify_batch_device(") < header.index("gkr_mle_eval_batch_device(")
    assert callable(Context.verify_sumcheck_sop_batch_device) and callable(Context.verify_sumcheck_sop)
    assert "verify_sumcheck_sop" in Context.prove_sumcheck_sop.__doc__
    assert "verify_sumcheck_sop_batch_device" in verify_sumcheck_sop.__doc__
    assert "sum-of-products" in re.search(r"GKR_VERIFY_EVALUATION = 10[^\n]*\n[^\n]*", header).group(0)


def _terms(spec):
    arr = (N.SopTerm * len(spec))()
    for k, (degree, idx) in enumerate(spec):
        arr[k].degree = degree
        for j, i in enumerate(idx):
            arr[k].table[j] = i
    return arr


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device pointer that is never dereferenced.  The
    verifier refuses exactly what the prover refuses (test_sop_host.py's list)."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    accept, rnd, check = ctypes.c_int(7), ctypes.c_uint32(9), ctypes.c_uint32(9)
    out = [ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check)]
    INVALID = N.GKR_ERR_INVALID
    ok_terms = _terms([(2, (0, 1)), (1, (2,))])

    def tp(arr):
        return ctypes.cast(arr, ctypes.c_void_p)

    vb = lib.gkr_sumcheck_sop_verify_batch_device
    # 0 ctx, 1 tables, 2 n, 3 n_tables, 4 terms, 5 term_coeffs, 6 n_terms, 7 batch, 8 claims, 9 coeffs, 10 len, 11 r, 12 accept,
    # 13 failed_round, 14 failed_check, 15 out_claims, 16 out_evals
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, 1, fake, fake, fake, fake] + out + [fake, fake]
    for at in (0, 1, 4, 9, 10, 11, 12):                          # ctx, tables, terms, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert vb(*args) == INVALID, at
    for at, bad in ((7, 0), (7, 65536), (7, -1), (2, 1), (2, 31), (2, 0), (2, -1), (3, 0), (3, 9), (3, -1), (6, 0), (6, 9), (6, -1)):
        args = list(good)
        args[at] = bad
        assert vb(*args) == INVALID, (at, bad)
    eight = [(1, (m,)) for m in range(8)]
    for spec, n_tables in (([(0, ()), (1, (0,))], 1), ([(4, (0, 0, 0))], 1), ([(255, (0, 0, 0))], 1),      # a term degree outside 1 .. 3
                           ([(2, (0, 3)), (1, (1,)), (1, (2,))], 3), ([(3, (0, 1, 8))] + eight, 8),         # a table index >= n_tables
                           ([(2, (0, 1))], 3), ([(3, (0, 0, 0)), (1, (2,))], 3), (eight[:7], 8)):            # a table no term references
        arr = _terms(spec[:8])
        args = list(good)
        args[3], args[4], args[6] = n_tables, tp(arr), len(spec[:8])
        assert vb(*args) == INVALID, (spec, n_tables)
    # batch * n_tables * 2^n <= 2^30 values: every shape one step over the cap
    for n, n_tables, batch in ((30, 2, 1), (28, 5, 1), (27, 8, 2), (20, 1, 1025), (16, 3, 5462), (10, 8, 65535 * 4)):
        arr = _terms([(1, (m,)) for m in range(n_tables)])
        args = list(good)
        args[2], args[3], args[4], args[6], args[7] = n, n_tables, tp(arr), n_tables, batch
        assert vb(*args) == INVALID, (n, n_tables, batch)
    host = lib.gkr_sumcheck_sop_verify
    # 0 ctx, 1 tables, 2 n, 3 n_tables, 4 terms, 5 term_coeffs, 6 n_terms, 7 claim, 8 coeffs, 9 len, 10 r, 11 accept, 12 round, 13 check
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, fake, fake, fake, fake] + out
    for at in (0, 1, 4, 8, 9, 10, 11):                           # ctx, tables, terms, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    for at, bad in ((2, 1), (2, 31), (2, 0), (3, 0), (3, 9), (6, 0), (6, 9), (3, 2), (3, 4)):   # (n_tables 2: index 2 is out; 4: table 3 unused)
        args = list(good)
        args[at] = bad
        assert host(*args) == INVALID, (at, bad)
    for spec, n_tables in (([(0, ()), (1, (0,))], 1), ([(4, (0, 0, 0))], 1)):
        arr = _terms(spec)
        args = list(good)
        args[3], args[4], args[6] = n_tables, tp(arr), len(spec)
        assert host(*args) == INVALID, spec
    arr = _terms([(1, (0,)), (1, (1,))])
    args = list(good)
    args[2], args[3], args[4] = 30, 2, tp(arr)                   # 2 * 2^30 values
    assert host(*args) == INVALID
    assert not any(word) and (accept.value, rnd.value, check.value) == (7, 9, 9)          # nothing was written


# ---- the closed-form verdict model ---------------------------------------------------------------------------------------------------
def _structure(name):
    return next((m, terms) for s, m, terms in STRUCTURES if s == name)


def _tables_for(name, n, variant, rng):
    """variant 0: random tables.  1: tables that ignore a variable (short rows): every table the same variable, rotating with n.
    AB-AC in variant 1 has B == C (g identically zero)."""
    M, _ = _structure(name)
    if variant == 0:
        return [factor("random", n, rng) for _ in range(M)]
    kind = ("indep_first", "indep_middle", "indep_last")[n % 3]
    tables = [factor(kind, n, rng) for _ in range(M)]
    if name == "AB-AC":
        tables[2] = list(tables[1])
    return tables


def _sweep_against_the_relations(name, tables, n, with_claim):
    """Every case of the sweep: the model's triple equals reference_verdict's; and wherever the tampered transcript is still
    well-formed, the accept bit equals verifier.verify_sumcheck_sop on the values mle_eval gives for the (tampered) tables."""
    M, terms = _structure(name)
    D = sop_degree(terms)
    proof, r, evals = sop_sumcheck(tables, terms, n)
    claim = sop_claim(tables, terms)
    C, L, R = arrays_of(proof, r, D)
    assert point_sees(R, range(1 << n))
    sweep = cases(C, L, R, evals, terms, with_claim)
    assert {c.what for c in sweep} == {"honest", "slot", "r", "len", "table"} | ({"claim"} if with_claim else set())
    assert sweep[0].verdict == ACCEPTED and sweep[-1].verdict == ACCEPTED
    T = to_limbs([x for t in tables for x in t]).reshape(M, 1 << n, 4)
    Tb, Cb, Lb, Rb, cl = build_batch(T, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
    compared = 0
    for e, c in enumerate(sweep):
        cl_e = value(cl[e]) if with_claim else None
        tab_e = [from_limbs(Tb[e, m]) for m in range(M)]
        got = reference_verdict(tab_e, terms, Cb[e], Lb[e], Rb[e], cl_e, cached_hash)
        assert got == c.verdict, (name, n, with_claim, c)
        if got[2] not in (1, 2):                                             # well-formed: the host verifier can read it
            r_e = from_limbs(Rb[e])
            ev_e = [mle_eval(t, r_e) for t in tab_e]
            assert verify_sumcheck_sop(rounds_of(Cb[e], Lb[e]), r_e, ev_e, terms, cl_e) == got[0], (name, n, c)
            compared += 1
    assert compared > len(sweep) // 2
    return sweep, L, evals, proof


@pytest.mark.parametrize("name", [s[0] for s in STRUCTURES])
def test_verdict_model_against_the_relations_on_model_transcripts(name):
    """The six structures at n = 2, 3, 4, with and without claim, on random tables and on tables that ignore a variable (rows
    shorter than D + 1).  Sharpness is a condition on the inputs (seeds chosen for which it holds): without cancellation every
    value at the challenges is non-zero, every table change is seen and no shortened row drops coefficients that sum to zero;
    AB-AB accepts every table change; AB-AC with B == C accepts the changes of A and sees those of B and of C."""
    M, terms = _structure(name)
    D = sop_degree(terms)
    short = 0
    for n in (2, 3, 4):
        for variant in (0, 1):
            rng = random.Random(16000 + 100 * n + 10 * variant + len(name))
            tables = _tables_for(name, n, variant, rng)
            for with_claim in (True, False):
                sweep, L, evals, proof = _sweep_against_the_relations(name, tables, n, with_claim)
                if any(int(x) < D + 1 for x in L):
                    assert_sweep_reaches_short_rows(sweep, L, D)
                    short += 1
                if name in NO_CANCELLATION or (name == "AB-AC" and variant == 0):
                    assert_sweep_is_sharp(sweep, evals)
                elif name == "AB-AB":
                    assert proof == [[0]] * n
                    assert all(table_verdicts(sweep, m) == {ACCEPTED} for m in range(M))
                else:                                                        # AB-AC with B == C: A's cofactor e_B - e_C is zero
                    assert proof == [[0]] * n and evals[0] != 0
                    assert table_verdicts(sweep, 0) == {ACCEPTED}
                    assert table_verdicts(sweep, 1) == table_verdicts(sweep, 2) == {(False, n, EVALUATION)}
    assert short >= 6                                                        # every n in the variable-ignoring variant, both claims


def test_squares_follow_from_the_one_rule():
    """AA + 3B: a change w of e_A moves the sum by w (2 e_A + w), of e_B by 3 w -- both seen; with e_A chosen as -w / 2 the
    change of A would hide, which the rule (not a derivative) gets right."""
    _, terms = _structure("AA+3B")
    w = 12345
    e_a = (P - w) * pow(2, P - 2, P) % P
    assert sop_eval([(e_a + w) % P, 7], terms) == sop_eval([e_a, 7], terms)
    assert sop_eval([(e_a + w + 1) % P, 7], terms) != sop_eval([e_a, 7], terms)


def _key(c):
    """A case as plain Python values (its new element is an array of limbs)."""
    return c.what, c.index, c.new if c.new is None or isinstance(c.new, (int, str)) else tuple(int(x) for x in c.new), c.verdict, c.dropped


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_one_term_of_coefficient_one_is_the_product_verifiers_model(degree):
    """With one term of coefficient 1 over distinct tables the case list and the verdicts are product_verify_sweeps.cases' --
    zero-factor transcripts included (a change behind the zero factor is accepted by both)."""
    terms = [(1, tuple(range(degree)))]
    ran = 0
    for n in (2, 3, 4):
        for kinds in (["random"] * degree, ["indep_last", "random", "bits"][:degree], ["zero", "random", "constant"][:degree]):
            rng = random.Random(16500 + 10 * n + degree)
            tables = [factor(k, n, rng) for k in kinds]
            proof, r, evals = product_sumcheck(tables, n)
            assert sop_sumcheck(tables, terms, n) == (proof, r, evals)
            C, L, R = arrays_of(proof, r, degree)
            assert point_sees(R, range(1 << n))
            for with_claim in (True, False):
                assert [_key(c) for c in cases(C, L, R, evals, terms, with_claim)] == [_key(c) for c in product.cases(C, L, R, evals, with_claim)]
                ran += 1
    assert ran == 18


@pytest.fixture(scope="module")
def sop_cases():
    cases_ = load_golden("sop_sumcheck.json")["cases"]
    assert len(cases_) == 5
    return [{"name": c["name"], "n": c["n"], "terms": [(int(k), tuple(idx)) for k, idx in c["terms"]],
             "tables": [[int(x) for x in t] for t in c["tables"]], "proof": [[int(x) for x in g] for g in c["proof"]],
             "r": [int(x) for x in c["r"]], "claim": int(c["claim"])} for c in cases_]


def test_golden_transcripts_are_accepted_and_rejected_with_another_claim(sop_cases):
    for c in sop_cases:
        C, L, R = arrays_of(c["proof"], c["r"], sop_degree(c["terms"]))
        assert reference_verdict(c["tables"], c["terms"], C, L, R, c["claim"], cached_hash) == ACCEPTED
        assert reference_verdict(c["tables"], c["terms"], C, L, R, None, cached_hash) == ACCEPTED
        assert reference_verdict(c["tables"], c["terms"], C, L, R, (c["claim"] + 1) % P, cached_hash) == (False, 0, ROUND_SUM)
        evals = [mle_eval(t, c["r"]) for t in c["tables"]]
        for with_claim in (True, False):
            sweep = cases(C, L, R, evals, c["terms"], with_claim)
            assert_sweep_is_sharp(sweep, evals)

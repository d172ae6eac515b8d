"""The zero-check sumcheck (include/gkr_amd.h, gkr_sumcheck_zerocheck*, gkr_eq_table_device) as far as no device is needed: the
symbols, the argument checks that run before a device is touched, the implicit integer model (tests/zerocheck_model.py) against
the sum-of-products model on the materialised eq table, the reference's own eq(AB-C) fixtures (tests/golden/sop_sumcheck.json)
and the host verifier gkr_amd.verifier.verify_sumcheck_zerocheck."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import gkr_amd
from conftest import load_golden
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, to_limbs
from gkr_amd.prover import Context
from gkr_amd.verifier import mle_eval, verify_sumcheck_sop, verify_sumcheck_zerocheck
from product_model import KINDS, factor
from sop_model import STRUCTURES, limbs_to_object, sop_sumcheck
from zerocheck_model import (eq_table, eq_table_np, lift_terms, zc_degree, zerocheck_claim, zerocheck_claim_np, zerocheck_eval,
                             zerocheck_sumcheck, zerocheck_sumcheck_np)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_sumcheck_zerocheck_batch_device", "gkr_sumcheck_zerocheck", "gkr_eq_table_device"]
ZC_STRUCTURES = [s for s in STRUCTURES if s[0] in ("AB-C", "5AB+7BC+11A", "AA+3B", "AB-AB", "AB-AC")]


def test_the_three_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("sumcheck_zerocheck_batch_device", "prove_zerocheck", "eq_table_device"):
        assert callable(getattr(Context, name)), name
    assert callable(gkr_amd.prove_zerocheck) and callable(gkr_amd.verify_sumcheck_zerocheck)
    assert "prove_zerocheck" in gkr_amd.__all__ and "verify_sumcheck_zerocheck" in gkr_amd.__all__


def _terms(spec):
    arr = (N.SopTerm * len(spec))()
    for k, (degree, idx) in enumerate(spec):
        arr[k].degree = degree
        for j, i in enumerate(idx):
            arr[k].table[j] = i
    return arr


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    ok_terms = _terms([(2, (0, 1)), (1, (2,))])

    def tp(arr):
        return ctypes.cast(arr, ctypes.c_void_p)

    bd = lib.gkr_sumcheck_zerocheck_batch_device
    # ctx, tables, n, n_tables, terms, coeffs, n_terms, batch, z, out_coeffs, out_len, out_r, out_evals, out_eq
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, 1, fake, fake, fake, fake, fake, fake]
    for at in (0, 1, 4, 8, 9, 10, 11):                             # (8: NULL z)
        args = list(good)
        args[at] = None
        assert bd(*args) == INVALID, at
    for at, bad in ((7, 0), (7, 65536), (7, -1), (2, 1), (2, 31), (2, 0), (2, -1), (3, 0), (3, 9), (3, -1), (6, 0), (6, 9), (6, -1)):
        args = list(good)
        args[at] = bad
        assert bd(*args) == INVALID, (at, bad)
    eight = [(1, (m,)) for m in range(8)]
    for spec, n_tables in (([(0, ()), (1, (0,))], 1), ([(4, (0, 0, 0))], 1), ([(255, (0, 0, 0))], 1),      # a term degree outside 1 .. 3
                           ([(3, (0, 0, 0))], 1), ([(3, (0, 1, 2))], 3), ([(2, (0, 1)), (3, (0, 1, 2))], 3),  # A TERM OF DEGREE 3
                           ([(2, (0, 3)), (1, (1,)), (1, (2,))], 3), ([(2, (0, 8))] + eight, 8),            # a table index >= n_tables
                           ([(2, (0, 1))], 3), ([(2, (0, 0)), (1, (2,))], 3), (eight[:7], 8)):               # a table no term references
        arr = _terms(spec[:8])
        args = list(good)
        args[3], args[4], args[6] = n_tables, tp(arr), len(spec[:8])
        assert bd(*args) == INVALID, (spec, n_tables)
    # batch * n_tables * 2^n <= 2^30 values: the SOP prover's shapes one step over the cap
    for n, n_tables, batch in ((30, 2, 1), (28, 5, 1), (27, 8, 2), (20, 1, 1025), (16, 3, 5462), (10, 8, 65535 * 4)):
        arr = _terms([(1, (m,)) for m in range(n_tables)])
        args = list(good)
        args[2], args[3], args[4], args[6], args[7] = n, n_tables, tp(arr), n_tables, batch
        assert bd(*args) == INVALID, (n, n_tables, batch)
    host = lib.gkr_sumcheck_zerocheck
    # ctx, tables, n, n_tables, terms, coeffs, n_terms, z, out_coeffs, out_len, out_r, out_evals, out_eq
    good = [fake, fake, 3, 3, tp(ok_terms), None, 2, fake, fake, fake, fake, fake, fake]
    for at in (0, 1, 4, 7, 8, 9, 10):                              # (7: NULL z)
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    for at, bad in ((2, 1), (2, 31), (3, 0), (3, 9), (6, 0), (6, 9), (3, 2), (3, 4)):    # (n_tables 2: index 2 is out; 4: table 3 unused)
        args = list(good)
        args[at] = bad
        assert host(*args) == INVALID, (at, bad)
    args = list(good)
    args[4] = tp(_terms([(3, (0, 1, 2)), (1, (2,))]))                                   # a term of degree 3
    assert host(*args) == INVALID
    arr = _terms([(1, (0,)), (1, (1,))])
    args = list(good)
    args[2], args[3], args[4] = 30, 2, tp(arr)                                          # 2 * 2^30 values
    assert host(*args) == INVALID
    eq = lib.gkr_eq_table_device
    # ctx, z, n, batch, d_out, stride_elements
    good = [fake, fake, 3, 2, fake, 8]
    for at in (0, 1, 4):
        args = list(good)
        args[at] = None
        assert eq(*args) == INVALID, at
    for at, bad in ((2, 0), (2, -1), (2, 31), (3, 0), (3, -1), (3, 65536), (5, 7), (5, 0)):
        args = list(good)
        args[at] = bad
        assert eq(*args) == INVALID, (at, bad)
    assert not any(word)                                                                # nothing was written


def _points(n, rng):
    """(name, z): random, all zero, all one, mixed 0/1, mixed 0/1/random."""
    yield "random", [rng.randrange(P) for _ in range(n)]
    yield "zeros", [0] * n
    yield "ones", [1] * n
    yield "boolean", [(j + 1) % 2 for j in range(n)]
    yield "boolean2", [rng.randrange(2) for _ in range(n)]
    yield "mixed", [(0, 1, rng.randrange(P))[(j + n) % 3] for j in range(n)]
    yield "mixed2", [(rng.randrange(P), 1, 0)[j % 3] for j in range(n)]


def test_eq_table_is_the_product_of_its_factors():
    rng = random.Random(17001)
    for n in (1, 2, 5):
        z = [rng.randrange(P) for _ in range(n)]
        e = eq_table(z)
        assert len(e) == 1 << n and sum(e) % P == 1
        for i in range(1 << n):
            v = 1
            for j in range(n):
                v = v * (z[j] if (i >> (n - 1 - j)) & 1 else 1 - z[j]) % P
            assert e[i] == v
        assert eq_table_np(z).tolist() == e
    assert eq_table([]) == [1]
    assert eq_table([1, 0, 1]) == [0, 0, 0, 0, 0, 1, 0, 0]        # a boolean point: the indicator of its index, MSB first


def test_model_is_the_sop_model_on_the_materialised_eq_table():
    """Every structure of inner degree <= 2, n = 2 .. 4, every factor kind in every table, the seven points: proof, r, the
    tables' evals and eq_r (= the eq table's eval) are sop_sumcheck's on [eq_table(z)] + tables with the lifted terms; the claim
    g_1(0) + g_1(1) is the entry-by-entry sum."""
    rng = random.Random(20261101)
    assert [s[0] for s in ZC_STRUCTURES] == ["AB-C", "5AB+7BC+11A", "AA+3B", "AB-AB", "AB-AC"]
    ran, zero, short = 0, 0, set()
    for n in (2, 3, 4):
        for name, n_tables, terms in ZC_STRUCTURES:
            lifted = lift_terms(terms)
            assert all(idx[0] == 0 and min(idx[1:]) >= 1 for _, idx in lifted) and zc_degree(terms) == max(len(i) for _, i in lifted)
            for a in range(len(KINDS)):
                tables = [factor(KINDS[(a + 3 * m) % len(KINDS)], n, rng) for m in range(n_tables)]
                for pname, z in _points(n, rng):
                    proof, r, evals, eq_r = zerocheck_sumcheck(tables, terms, z, n)
                    want = sop_sumcheck([eq_table(z)] + tables, lifted, n)
                    assert (proof, r, [eq_r] + evals) == want, (name, n, a, pname)
                    claim = zerocheck_claim(tables, terms, z)
                    assert (2 * proof[0][-1] + sum(proof[0][:-1])) % P == claim, (name, n, a, pname)
                    assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, claim)
                    ran += 1
                    zero += proof == [[0]] * n
                    short |= {len(g) for g in proof}
    assert ran == 3 * 5 * 8 * 7 and zero >= 3 * 8 * 7               # AB-AB is identically zero at every point
    assert short == {1, 2, 3, 4}


def test_the_vectorised_model_is_the_model():
    rng = random.Random(20261102)
    for name, n_tables, terms in ZC_STRUCTURES:
        for n in (2, 3, 6):
            tables = [factor(KINDS[(n + 3 * m + len(name)) % len(KINDS)], n, rng) for m in range(n_tables)]
            arr = limbs_to_object(np.stack([to_limbs(t) for t in tables]))
            for pname, z in list(_points(n, rng))[::3]:
                assert zerocheck_sumcheck_np(arr, terms, z, n) == zerocheck_sumcheck(tables, terms, z, n), (name, n, pname)
                assert zerocheck_claim_np(arr, terms, z) == zerocheck_claim(tables, terms, z), (name, n, pname)


def test_reference_fixtures_from_the_tables_and_z_alone():
    """The two eq(AB-C) cases of the reference's own Python prover record z: their table 0 is eq_table(z) (which pins the variable
    order of the eq table to the reference), and the implicit model reproduces them from tables 1 .. 3 and z."""
    cases = [c for c in load_golden("sop_sumcheck.json")["cases"] if c["z"]]
    assert [(c["name"], c["n"]) for c in cases] == [("eq(AB-C)", 2), ("eq(AB-C)", 3)]
    for c in cases:
        n, z = c["n"], [int(x) for x in c["z"]]
        tables = [[int(x) for x in t] for t in c["tables"]]
        lifted = [(int(k), tuple(idx)) for k, idx in c["terms"]]
        terms = [(k, tuple(i - 1 for i in idx[1:])) for k, idx in lifted]
        assert all(idx[0] == 0 for _, idx in lifted) and lift_terms(terms) == lifted
        assert tables[0] == eq_table(z)
        proof, r, evals, eq_r = zerocheck_sumcheck(tables[1:], terms, z, n)
        assert proof == [[int(x) for x in g] for g in c["proof"]] and r == [int(x) for x in c["r"]], n
        assert evals == [mle_eval(t, r) for t in tables[1:]] and eq_r == mle_eval(tables[0], r)
        assert zerocheck_claim(tables[1:], terms, z) == int(c["claim"])
        assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, int(c["claim"]))
        assert verify_sumcheck_sop(proof, r, [eq_r] + evals, lifted, int(c["claim"]))


def test_host_verifier_accepts_the_model_and_rejects_every_single_change():
    rng = random.Random(707)
    n = 3
    for name in ("AB-C", "5AB+7BC+11A"):
        _, n_tables, terms = next(s for s in STRUCTURES if s[0] == name)
        tables = [factor("random", n, rng) for _ in range(n_tables)]
        for pname, z in _points(n, rng):
            claim = zerocheck_claim(tables, terms, z)
            proof, r, evals, eq_r = zerocheck_sumcheck(tables, terms, z, n)
            ok = lambda **kw: verify_sumcheck_zerocheck(kw.get("proof", proof), kw.get("r", r), kw.get("evals", evals), terms,
                                                        kw.get("z", z), kw.get("claim", claim))
            assert ok() and ok(claim=None)
            assert proof[-1] != [0] and eq_r != 0 and zerocheck_eval(evals, terms, eq_r) != 0, pname   # (so that every change below shows)
            for j, g in enumerate(proof):
                for k in range(len(g)):
                    bad = [list(x) for x in proof]
                    bad[j][k] = (g[k] + 1) % P
                    assert not ok(proof=bad) and not ok(proof=bad, claim=None), (pname, j, k)
                bad_r = list(r)
                bad_r[j] = (r[j] + 1) % P
                assert not ok(r=bad_r), (pname, j)
                bad_z = list(z)
                bad_z[j] = (z[j] + 1) % P
                assert not ok(z=bad_z), (pname, j)
            for m in range(n_tables):
                bad_e = list(evals)
                bad_e[m] = (evals[m] + 1) % P
                assert zerocheck_eval(bad_e, terms, eq_r) != zerocheck_eval(evals, terms, eq_r)
                assert not ok(evals=bad_e), (pname, m)
            assert not ok(claim=(claim + 1) % P)
            assert not ok(proof=proof[:-1]) and not ok(z=z[:-1]) and not ok(evals=evals[:-1])
            assert not ok(proof=[[0] * (zc_degree(terms) + 2 - len(proof[0])) + proof[0]] + proof[1:])   # D + 2 slots
    assert not verify_sumcheck_zerocheck(proof, r, evals + [0], [(1, (0, 1, 2)), (1, (3,))], z)           # a term of three tables

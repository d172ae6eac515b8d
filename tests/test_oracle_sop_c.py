"""ogkr_sumcheck_sop and ogkr_sumcheck_zerocheck (oracle/c/ogkr.c; cdense.sumcheck_sop_raw, cdense.sumcheck_zerocheck_raw), the C
twins of tests/sop_model.py and tests/zerocheck_model.py that the GPU suite compares the sum-of-products and the zero-check kernels
with at sizes the Python models cannot reach.  The zero-check oracle is EXPLICIT (it writes eq(z, .) out as a table of 2^n entries
and runs the SOP oracle on it); the model and the library are implicit.  What holds the two:

  a. sop_model.sop_sumcheck for n = 2 .. 6: the six STRUCTURES and the five bookkeeping term lists, every factor kind in turn;
  b. the reference's own Python prover (tests/golden/sop_sumcheck.json), the eq (AB - C) cases through both oracles;
  c. ogkr_sumcheck_product, byte for byte, with one term of coefficient 1 at degree 1 .. 3;
  d. zerocheck_model.zerocheck_sumcheck for n = 2 .. 6: the five structures x random, boolean, mixed and z_j = 1/2 points;
  e. at n = 16, where only the C side is fast: the vectorised models, the host verifiers with a claim summed entry by entry, the
     same bytes under 1, 3 and all usable threads;
  f. bad shapes are errors;
  g. a stand-alone program (oracle/c/sop_selfcheck.c) built with the C file under ASan + UBSan, run as a child process."""

import os
import random
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd.verifier import mle_eval, verify_sumcheck_sop, verify_sumcheck_zerocheck
from oracle import cdense
from oracle.field import P
from product_model import KINDS, factor
from sop_model import STRUCTURES, limbs_to_object, sop_claim_np, sop_degree, sop_sumcheck, sop_sumcheck_np
from sop_terms import BOOKKEEPING
from zerocheck_model import (eq_table, zc_degree, zerocheck_claim_np, zerocheck_sumcheck, zerocheck_sumcheck_np)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KINDS = KINDS + ["zero"]
HALF = (P + 1) // 2
TERM_LISTS = [(name, M, terms) for name, M, terms in STRUCTURES] + [(name, M, terms) for name, (M, terms) in BOOKKEEPING.items()]
ZC_STRUCTURES = [s for s in STRUCTURES if s[0] in ("AB-C", "5AB+7BC+11A", "AA+3B", "AB-AB", "AB-AC")]


def _limbs(tables):
    return np.concatenate([cdense.to_limbs(t) for t in tables])


def _rows(C, L, what):
    """The used slots of every row, as integers; the unused ones must hold zero."""
    slots = C.shape[1]
    rows = [cdense.from_limbs(C[j]) for j in range(C.shape[0])]
    for j, row in enumerate(rows):
        assert 1 <= int(L[j]) <= slots and not any(row[:slots - int(L[j])]), ("unused slots hold zero", what, j)
    return [row[slots - int(L[j]):] for j, row in enumerate(rows)]


def _assert_sop_equals(tables, terms, n, want, what):
    M, D = len(tables), sop_degree(terms)
    C, L, R, E = cdense.sumcheck_sop_raw(_limbs(tables), n, M, terms)
    assert C.shape == (n, D + 1, 4) and L.shape == (n,) and R.shape == (n, 4) and E.shape == (M, 4)
    proof, r, evals = want
    assert _rows(C, L, what) == proof, what
    assert cdense.from_limbs(R) == r, what
    if evals is not None:
        assert cdense.from_limbs(E) == evals, what
    return E


def _assert_zerocheck_equals(tables, terms, z, n, want, what):
    M, D = len(tables), zc_degree(terms)
    C, L, R, E, Q = cdense.sumcheck_zerocheck_raw(_limbs(tables), n, M, terms, cdense.to_limbs(z))
    assert C.shape == (n, D + 1, 4) and L.shape == (n,) and R.shape == (n, 4) and E.shape == (M, 4) and Q.shape == (4,)
    proof, r, evals, eq_r = want
    assert _rows(C, L, what) == proof, what
    assert cdense.from_limbs(R) == r, what
    if evals is not None:
        assert cdense.from_limbs(E) == evals, what
    if eq_r is not None:
        assert cdense.from_limbs(Q) == [eq_r], what
    return E, Q


def _closed_form_eq(z, r):
    v = 1
    for zj, rj in zip(z, r):
        v = v * (zj * rj + (1 - zj) * (1 - rj)) % P
    return v


# ---- a. the SOP oracle against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,M,terms", TERM_LISTS, ids=[t[0] for t in TERM_LISTS])
def test_sop_equals_the_model_for_every_factor_kind(name, M, terms):
    """Kind ci sits at table (ci + n) % M, the other tables take the kinds that follow it: every table position of every term list
    sees several kinds, and every kind (the zero table included) occurs in every term list at every n."""
    D = sop_degree(terms)
    short_first = short_last = full = 0
    for n in range(2, 7):
        for ci, kind in enumerate(ALL_KINDS):
            rng = random.Random(11000 + 100 * n + ci + len(name))
            at = (ci + n) % M
            kinds = [kind if m == at else ALL_KINDS[(ci + 3 * (m - at) + n) % len(ALL_KINDS)] for m in range(M)]
            tables = [factor(k, n, rng) for k in kinds]
            want = sop_sumcheck(tables, terms, n)
            _assert_sop_equals(tables, terms, n, want, (name, n, kinds))
            short_first += len(want[0][0]) < D + 1
            short_last += len(want[0][-1]) < D + 1
            full += all(len(g) == D + 1 for g in want[0])
    assert short_first and short_last                              # the length rule was in play at both ends ...
    assert full or name == "AB-AB"                                 # ... and not everywhere


def test_sop_of_cancelling_terms_is_all_zero_vectors():
    from oracle.mimc7 import multi_hash
    rng = random.Random(11900)
    for n in (2, 5):
        tables = [factor("random", n, rng) for _ in range(2)]
        C, L, R, E = cdense.sumcheck_sop_raw(_limbs(tables), n, 2, [(1, (0, 1)), (P - 1, (0, 1))])
        assert (L == 1).all() and not C.any() and cdense.from_limbs(R) == [multi_hash([0], 0)] * n
        assert cdense.from_limbs(E) == [mle_eval(t, cdense.from_limbs(R)) for t in tables]


# ---- b. the reference's Python prover ---------------------------------------------------------------------------------------------------
def test_both_oracles_reproduce_the_reference_python_prover():
    cases = load_golden("sop_sumcheck.json")["cases"]
    assert len(cases) == 5 and sum(1 for c in cases if c["z"]) == 2
    for c in cases:
        n = c["n"]
        tables = [[int(x) for x in t] for t in c["tables"]]
        terms = [(int(k), tuple(idx)) for k, idx in c["terms"]]
        proof, r = [[int(x) for x in g] for g in c["proof"]], [int(x) for x in c["r"]]
        E = _assert_sop_equals(tables, terms, n, (proof, r, None), (c["name"], n))
        evals = cdense.from_limbs(E)
        assert evals == [mle_eval(t, r) for t in tables]
        assert verify_sumcheck_sop(proof, r, evals, terms, int(c["claim"]))
        if c["z"]:                                                 # eq (A B - C): the zero-check oracle from tables 1 .. 3 and z alone
            z = [int(x) for x in c["z"]]
            assert tables[0] == eq_table(z)
            inner = [(k, tuple(i - 1 for i in idx[1:])) for k, idx in terms]
            assert all(idx[0] == 0 for _, idx in terms)
            _assert_zerocheck_equals(tables[1:], inner, z, n, (proof, r, evals[1:], evals[0]), ("zero-check", n))
            assert verify_sumcheck_zerocheck(proof, r, evals[1:], inner, z, int(c["claim"]))


# ---- c. one term against the product oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_one_term_of_coefficient_one_is_the_product_oracle_byte_for_byte(degree):
    terms = [(1, tuple(range(degree)))]
    short = 0
    for n in list(range(2, 7)) + [12]:
        for ci, kind in enumerate(ALL_KINDS if n < 12 else ["random", "indep_last"]):
            rng = random.Random(12000 + 100 * n + 10 * degree + ci)
            tables = [factor(kind if f == ci % degree else ALL_KINDS[(ci + 2 * f + n) % len(ALL_KINDS)], n, rng) for f in range(degree)]
            T = _limbs(tables)
            got = cdense.sumcheck_sop_raw(T, n, degree, terms)
            want = cdense.sumcheck_product_raw(T, n, degree)
            for what, g, w in zip(("coeffs", "len", "r", "evals"), got, want):
                assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, n, degree, kind)
            short += int((got[1] < degree + 1).any())
    assert short


# ---- d. the zero-check oracle against the implicit model --------------------------------------------------------------------------------
def _points(n, rng):
    """name -> (z, the round whose vector z_j = 1/2 shortens or None)."""
    out = {"random": ([rng.randrange(P) for _ in range(n)], None),
           "boolean": ([rng.randrange(2) for _ in range(n)], None),
           "mixed": ([(0, 1, rng.randrange(P))[(j + n) % 3] for j in range(n)], None)}
    for where, j in (("first", 0), ("middle", n // 2), ("last", n - 1)):
        z = [rng.randrange(P) for _ in range(n)]
        z[j] = HALF
        out["half at the %s index" % where] = (z, j)
    return out


@pytest.mark.parametrize("structure", ZC_STRUCTURES, ids=[s[0] for s in ZC_STRUCTURES])
def test_zerocheck_equals_the_model(structure):
    name, M, terms = structure
    D = zc_degree(terms)
    for n in range(2, 7):
        rng = random.Random(13000 + 100 * n + len(name))
        for pi, (point, (z, half_at)) in enumerate(_points(n, rng).items()):
            # 1/2: random tables, so that h_j has its full degree and the linear factor alone shortens the vector
            kinds = ["random"] * M if half_at is not None else [ALL_KINDS[(pi + 3 * m + n) % len(ALL_KINDS)] for m in range(M)]
            tables = [factor(k, n, rng) for k in kinds]
            want = zerocheck_sumcheck(tables, terms, z, n)
            if half_at is not None:                                # (on the model first)
                assert (2 * z[half_at] - 1) % P == 0
                lengths = [len(g) for g in want[0]]
                if name == "AB-AB":
                    assert want[0] == [[0]] * n
                else:
                    assert lengths[half_at] == D and want[0][half_at][0] != 0, (name, n, point, lengths)
                    assert all(l == D + 1 for j, l in enumerate(lengths) if j != half_at), (name, n, point, lengths)
            _assert_zerocheck_equals(tables, terms, z, n, want, (name, n, point, kinds))
            assert want[3] == _closed_form_eq(z, want[1])


# ---- e. a size only the C side reaches --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_sop():
    n = 16
    _, M, terms = next(s for s in STRUCTURES if s[0] == "ABC-AD")
    T = cdense.fill_table(M << n, 1604).reshape(M, 1 << n, 4)
    T[3, 1::2] = T[3, 0::2]                                        # D ignores x_n: the last vector loses nothing (A B C has degree 3)
    T[1, 1 << (n - 1):] = T[1, :1 << (n - 1)]                      # B ignores x_1: round 0 has degree 2
    return n, M, terms, T, cdense.sumcheck_sop_raw(T, n, M, terms)


@pytest.fixture(scope="module")
def large_zerocheck():
    n = 16
    _, M, terms = next(s for s in STRUCTURES if s[0] == "5AB+7BC+11A")
    T = cdense.fill_table(M << n, 1605).reshape(M, 1 << n, 4)
    z = cdense.from_limbs(cdense.fill_table(n, 1606))
    z[3], z[5], z[9] = HALF, 0, 1
    Z = cdense.to_limbs(z)
    return n, M, terms, T, z, cdense.sumcheck_zerocheck_raw(T, n, M, terms, Z)


def test_sop_at_a_size_only_the_c_side_reaches(large_sop):
    n, M, terms, T, (C, L, R, E) = large_sop
    tables = limbs_to_object(T)
    proof, r, evals = _rows(C, L, "n = 16"), cdense.from_limbs(R), cdense.from_limbs(E)
    assert (proof, r, evals) == sop_sumcheck_np(tables, terms, n)
    assert [len(g) for g in proof] == [3] + [4] * (n - 1)
    assert verify_sumcheck_sop(proof, r, evals, terms, sop_claim_np(tables, terms))
    assert not verify_sumcheck_sop(proof, r, evals, terms, (sop_claim_np(tables, terms) + 1) % P)


def test_zerocheck_at_a_size_only_the_c_side_reaches(large_zerocheck):
    n, M, terms, T, z, (C, L, R, E, Q) = large_zerocheck
    tables = limbs_to_object(T)
    proof, r, evals, eq_r = _rows(C, L, "n = 16"), cdense.from_limbs(R), cdense.from_limbs(E), cdense.from_limbs(Q)[0]
    assert (proof, r, evals, eq_r) == zerocheck_sumcheck_np(tables, terms, z, n)
    assert [len(g) for g in proof] == [4, 4, 4, 3] + [4] * (n - 4)                      # z_4 = 1/2
    assert eq_r == _closed_form_eq(z, r)
    claim = zerocheck_claim_np(tables, terms, z)
    assert verify_sumcheck_zerocheck(proof, r, evals, terms, z, claim)
    assert not verify_sumcheck_zerocheck(proof, r, evals, terms, z, (claim + 1) % P)


def test_the_results_do_not_depend_on_the_thread_count(large_sop, large_zerocheck):
    n, M, terms, T, want = large_sop
    for threads in (1, 3, cdense.usable_threads()):
        got = cdense.sumcheck_sop_raw(T, n, M, terms, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), threads
    n, M, terms, T, z, want = large_zerocheck
    for threads in (1, 3, cdense.usable_threads()):
        got = cdense.sumcheck_zerocheck_raw(T, n, M, terms, cdense.to_limbs(z), threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), threads


# ---- f. bad shapes ----------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_are_errors():
    T = cdense.fill_table(9 << 4, 1)
    ab = [(1, (0, 1))]
    Z = cdense.fill_table(4, 2)
    cdense.sumcheck_sop_raw(T[:2 << 4], 4, 2, ab)                                        # (the good shape next to them)
    cdense.sumcheck_zerocheck_raw(T[:2 << 4], 4, 2, ab, Z)
    for n, M, terms in ((1, 2, ab), (4, 0, ab), (4, 9, ab), (4, 2, []), (4, 2, [(1, (0, 1, 1, 0))]), (4, 2, [(1, ())]), (4, 2, [(1, (0, 2))]),
                        (4, 2, [(1, (0,))] * 9)):
        with pytest.raises(ValueError):
            cdense.sumcheck_sop_raw(T[:M << n], n, M, terms)
    with pytest.raises(ValueError):
        cdense.sumcheck_sop_raw(T[:5], 2, 2, ab)
    for n, M, terms, z in ((1, 2, ab, Z[:1]), (4, 0, ab, Z), (4, 9, ab, Z), (4, 2, [], Z), (4, 3, [(1, (0, 1, 2))], Z), (4, 2, [(1, (0, 2))], Z),
                           (4, 2, ab, Z[:3])):
        with pytest.raises(ValueError):
            cdense.sumcheck_zerocheck_raw(T[:M << n], n, M, terms, z)
    not_canonical = Z.copy()
    not_canonical[2] = (1 << 64) - 1
    with pytest.raises(ValueError):
        cdense.sumcheck_zerocheck_raw(T[:2 << 4], 4, 2, ab, not_canonical)


# ---- g. under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """`make -C oracle/c sop_selfcheck`: n = 2 .. 10, both oracles, 1 and 4 threads give equal bytes, one term equals
    ogkr_sumcheck_product, the zero-check equals the SOP oracle on an eq table the program builds; no sanitizer report.  A child
    process: nothing is loaded into this one."""
    exe = str(tmp_path / "sop_selfcheck")
    build = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "c"), "sop_selfcheck", "OUT=" + exe], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "sop_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

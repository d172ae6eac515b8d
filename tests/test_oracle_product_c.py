"""ogkr_sumcheck_product (oracle/c/ogkr.c, cdense.sumcheck_product_raw), the C twin of tests/product_model.py that the GPU suite
compares the product sumcheck's kernels with at sizes the Python model cannot reach.  What holds it:

  a. the model, for every ordered pair of factor kinds (degree 3: every pair with a third factor drawn by a fixed seed), n = 2..6;
  b. the reference's own Python prover (tests/golden/product_sumcheck.json);
  c. the older, independent C function ogkr_sumcheck_mle at degree 1, n = 12 and 16;
  d. at n = 16, degree 3, where only the C side is fast: the host verifier, the sum of products and an integer fold;
  e. the same bytes with 1, 3 and all usable threads;
  f. a stand-alone program (oracle/c/product_selfcheck.c) built with the C file under ASan + UBSan, run as a child process."""

import os
import random
import subprocess

import numpy as np
import pytest

from conftest import load_golden
from gkr_amd.verifier import mle_eval, verify_sumcheck_product
from oracle import cdense
from oracle.field import P
from product_model import KINDS, factor, product_sumcheck

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KINDS = KINDS + ["zero"]


def _limbs(tables):
    return np.concatenate([cdense.to_limbs(t) for t in tables])


def _assert_equals_model(tables, n, want=None, what=None):
    d = len(tables)
    C, L, R, E = cdense.sumcheck_product_raw(_limbs(tables), n, d)
    assert C.shape == (n, d + 1, 4) and L.shape == (n,) and R.shape == (n, 4) and E.shape == (d, 4)
    proof, r, evals = want if want is not None else product_sumcheck(tables, n)
    assert [int(x) for x in L] == [len(g) for g in proof], what
    for j in range(n):
        row = cdense.from_limbs(C[j])
        assert not any(row[:d + 1 - len(proof[j])]), ("unused slots hold zero", what, j)
        assert row[d + 1 - len(proof[j]):] == proof[j], (what, j)
    assert cdense.from_limbs(R) == r, what
    if evals is not None:
        assert cdense.from_limbs(E) == evals, what
    return E


def _kind_choices(degree):
    """Ordered choices of factor kinds: all of them at degree 1 and 2; at degree 3 every ordered pair, in each of the three
    position pairs in turn, with the remaining factor's kind drawn by a fixed seed (9^3 = 729 triples times five n is too much)."""
    if degree == 1:
        return [[k] for k in ALL_KINDS]
    pairs = [[a, b] for a in ALL_KINDS for b in ALL_KINDS]
    if degree == 2:
        return pairs
    rng = random.Random(31415)
    out = []
    for i, (a, b) in enumerate(pairs):
        third = ALL_KINDS[rng.randrange(len(ALL_KINDS))]
        out.append([[a, b, third], [a, third, b], [third, a, b]][i % 3])
    return out


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_equals_the_model_for_every_pair_of_factor_kinds(degree):
    choices = _kind_choices(degree)
    if degree >= 2:
        seen = {(c[i], c[j]) for c in choices for i in range(degree) for j in range(i + 1, degree)}
        assert seen == {(a, b) for a in ALL_KINDS for b in ALL_KINDS}
    short_first = short_last = zero = 0
    for n in range(2, 7):
        for ci, kinds in enumerate(choices):
            rng = random.Random(9000 + 1000 * degree + 100 * n + ci)
            tables = [factor(k, n, rng) for k in kinds]
            want = product_sumcheck(tables, n)
            _assert_equals_model(tables, n, want, (n, kinds))
            short_first += len(want[0][0]) < degree + 1
            short_last += len(want[0][-1]) < degree + 1
            zero += "zero" in kinds and want[0] == [[0]] * n
    assert short_first and short_last and zero          # the length rules and the zero-factor rule were in play


def test_equals_the_reference_python_prover():
    cases = load_golden("product_sumcheck.json")["cases"]
    assert len(cases) == 7
    for c in cases:
        tables = [[int(x) for x in t] for t in c["tables"]]
        proof, r = [[int(x) for x in g] for g in c["proof"]], [int(x) for x in c["r"]]
        E = _assert_equals_model(tables, c["n"], (proof, r, None), (c["n"], c["degree"]))
        assert cdense.from_limbs(E) == [mle_eval(t, r) for t in tables]
        assert verify_sumcheck_product(proof, r, cdense.from_limbs(E), c["degree"], int(c["claim"]))


@pytest.mark.parametrize("n", [12, 16])
def test_degree_one_equals_the_plain_c_sumcheck(n):
    T = cdense.fill_table(1 << n, 1200 + n)
    C, L, R, E = cdense.sumcheck_product_raw(T, n, 1)
    c2, l2, r2 = cdense.sumcheck_mle_raw(T, n)
    assert np.array_equal(C, c2) and np.array_equal(L, l2) and np.array_equal(R, r2)
    assert (L == 2).all()
    # ... and on a table that ignores x_n and x_1: lengths 1 in the first and the last round
    T[1::2] = T[0::2]
    T[1 << (n - 1):] = T[:1 << (n - 1)]
    C, L, R, E = cdense.sumcheck_product_raw(T, n, 1)
    c2, l2, r2 = cdense.sumcheck_mle_raw(T, n)
    assert np.array_equal(C, c2) and np.array_equal(L, l2) and np.array_equal(R, r2)
    assert L[0] == 1 and L[-1] == 1 and (L[1:-1] == 2).all()


@pytest.fixture(scope="module")
def large():
    n, degree = 16, 3
    T = cdense.fill_table(degree << n, 1603)
    return n, degree, T, cdense.sumcheck_product_raw(T, n, degree)


def test_a_size_only_the_c_side_reaches(large):
    """n = 16, degree 3, random tables: the transcript passes the host verifier with the claim and the evals computed here
    on Python integers (sum of products; an integer fold at the transcript's challenges)."""
    n, degree, T, (C, L, R, E) = large
    flat = cdense.from_limbs(T)
    tables = [flat[f << n:(f + 1) << n] for f in range(degree)]
    claim = sum(a * b % P * c for a, b, c in zip(*tables)) % P
    assert (L == degree + 1).all()
    proof = [cdense.from_limbs(C[j]) for j in range(n)]
    r = cdense.from_limbs(R)
    evals = [mle_eval(t, r) for t in tables]
    assert cdense.from_limbs(E) == evals
    assert verify_sumcheck_product(proof, r, evals, degree, claim)
    assert not verify_sumcheck_product(proof, r, evals, degree, (claim + 1) % P)


def test_the_result_does_not_depend_on_the_thread_count(large):
    n, degree, T, want = large
    for threads in (1, 3, cdense.usable_threads()):
        got = cdense.sumcheck_product_raw(T, n, degree, threads=threads)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), threads


def test_bad_shapes_are_errors():
    T = cdense.fill_table(4 << 4, 1)
    for n, degree in ((1, 1), (4, 4)):
        with pytest.raises(ValueError):
            cdense.sumcheck_product_raw(T[:degree << n], n, degree)
    with pytest.raises(ValueError):
        cdense.sumcheck_product_raw(T[:5], 2, 1)


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """`make -C oracle/c product_selfcheck`: n = 2..10, degree 1..3, 1 and 4 threads give equal bytes, degree 1 equals
    ogkr_sumcheck_mle; no sanitizer report.  A child process: nothing is loaded into this one."""
    exe = str(tmp_path / "product_selfcheck")
    build = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "c"), "product_selfcheck", "OUT=" + exe], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "product_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

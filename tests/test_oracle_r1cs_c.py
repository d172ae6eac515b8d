"""ogkr_r1cs_rows, ogkr_r1cs_cols and ogkr_r1cs_matrix_evals (oracle/c/ogkr.c; cdense.r1cs_rows_raw, r1cs_cols_raw,
r1cs_matrix_evals_raw), the C twins of tests/r1cs_rows_model.rows, tests/r1cs_cols_model.cols_table and verifier.r1cs_matrix_evals
that tests/test_gpu_r1cs_sizes.py compares the R1CS kernels with at sizes the Python models cannot reach.  They loop over the flat
records as they stand (no CSR, no column-major form, no pool, no case for 1 and r - 1).  What holds them:

  a. the three Python models, value for value, for n and n_y from 2 to 9: empty rows, zero coefficients, repeated wires, rows and
     columns longer than 32 and 64, the four coefficient mixes of the R1CS tests, random and boolean points, rho among 0, 1, r - 1
     and random;
  b. mimc91 and the five-constraint system: ogkr_sumcheck_zerocheck and ogkr_sumcheck_product on the oracle's tables give proofs
     that verifier.verify_r1cs accepts, and refuses after a change;
  c. at n_x = n_y = 16, on a system of tests/r1cs_systems.py, two identities in Python integers that tie the three together:
     <T, w> = sum_m rho_m sum_i eq(x, i) (M_m w)[i], and matrix_evals(x, y)[m] = the extension at y of the cols table with rho the
     m-th unit vector; the witness of r1cs_systems satisfies its system, and the library reads the arrays as the oracle does;
  d. thread counts 1 and 3 give the same bytes; e. every bad shape is an error;
  f. a stand-alone program (oracle/c/r1cs_selfcheck.c) built with the C file under ASan + UBSan, run as a child process."""

import os
import random
import subprocess

import numpy as np
import pytest

from gkr_amd import synth
from gkr_amd.verifier import R1CS_ZEROCHECK_TERMS, mle_eval, r1cs_matrix_evals, verify_r1cs
from oracle import cdense
from oracle.field import P
from r1cs_cols_model import cols_table, eq_table, n_y_of
from r1cs_rows_model import first_bad, rows, table_log2
from r1cs_systems import COEFF_MIX, LONG, NO_BAD, SEG, build_r1cs, constraints_of, flatten, generate, random_constraints, witness
import r1cs_systems

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO_KINDS = ["zero", "one", "minus_one", "random"]


def _rho(kind, rng):
    return {"zero": 0, "one": 1, "minus_one": P - 1}.get(kind, rng.randrange(P))


def _point(rng, n, boolean):
    return [rng.randrange(2) if boolean else rng.randrange(P) for _ in range(n)]


def _three(counts, wires, coeffs, n_wires, w, n, x, rho, y, threads=0):
    """The three oracle calls as integers: (rows [Az, Bz, Cz], T, [A~, B~, C~])."""
    n_y = len(y)
    r = cdense.r1cs_rows_raw(counts, wires, coeffs, n_wires, cdense.to_limbs(w), n, threads=threads)
    t = cdense.r1cs_cols_raw(counts, wires, coeffs, n_wires, cdense.to_limbs(x), cdense.to_limbs(rho), n_y, threads=threads)
    m = cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, n_wires, cdense.to_limbs(x), cdense.to_limbs(y), threads=threads)
    return [cdense.from_limbs(r[k]) for k in range(3)], cdense.from_limbs(t), cdense.from_limbs(m)


# ---- a. the Python models ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", COEFF_MIX)
def test_the_three_functions_equal_the_python_models(kind):
    """Every (n, n_y) in 2 .. 9 squared, each with one size: full tables, one entry past half (padding), or the smallest count that
    gives this n; rows of up to 4 or up to 70 terms; the points boolean or random and the weights cycling with the case."""
    longest_row = longest_col = case = 0
    for n in range(2, 10):
        for n_y in range(2, 10):
            case += 1
            rng = random.Random(31000 + 100 * n + 10 * n_y + len(kind))
            n_constraints = (1 << n, (1 << n - 1) + 1, 1 if n == 2 else (1 << n - 1) + 1)[case % 3]
            n_wires = ((1 << n_y - 1) + 1, 1 << n_y, 1 if n_y == 2 else (1 << n_y - 1) + 1)[(case // 3) % 3]
            assert table_log2(n_constraints) == n and n_y_of(n_wires) == n_y
            cons = random_constraints(rng, n_constraints, n_wires, kind, longest=70 if case % 4 == 0 else 4, zeros=case % 2 == 0)
            flat = flatten(cons)
            w = [rng.randrange(P) for _ in range(n_wires)]
            x, y = _point(rng, n, case % 3 == 1), _point(rng, n_y, case % 5 == 1)
            rho = [_rho(RHO_KINDS[(case + m) % 4], rng) for m in range(3)]
            got_rows, got_t, got_m = _three(*flat, n_wires, w, n, x, rho, y)
            assert got_rows == rows(cons, w, n), (n, n_y)
            assert got_t == cols_table(cons, n_wires, x, rho, n_y), (n, n_y)
            assert got_m == r1cs_matrix_evals(cons, x, y), (n, n_y)
            assert not any(got_t[n_wires:]) and not any(v for t in got_rows for v in t[n_constraints:])
            longest_row = max(longest_row, max(len(lc) for con in cons for lc in con))
            in_a = np.repeat(np.arange(len(flat[0])) % 3, flat[0]) == 0
            longest_col = max(longest_col, int(np.bincount(flat[1][in_a], minlength=1).max()))
    assert longest_row > 64 and longest_col > 64


def test_empty_rows_zero_coefficients_and_repeated_wires():
    """Written out: an empty A, a zero coefficient beside a non-zero one on the same wire, wire 1 three times in one combination."""
    cons = [([], [(0, 1), (5, 1)], [(2, 1), (3, 1), (P - 1, 1)]), ([(7, 0)], [], [(0, 2)])]
    w = [1, 10, 100]
    got_rows, got_t, got_m = _three(*flatten(cons), 3, w, 2, [0, 0], [1, 1, 1], [0, 1])       # row 0, wire 1
    assert got_rows == [[0, 7, 0, 0], [50, 0, 0, 0], [40, 0, 0, 0]] == rows(cons, w, 2)
    assert got_t == [0, 9, 0, 0] == cols_table(cons, 3, [0, 0], [1, 1, 1], 2)
    assert got_m == [0, 5, 4] == r1cs_matrix_evals(cons, [0, 0], [0, 1])


# ---- b. proofs from the oracle alone, through the Python verifier ---------------------------------------------------------------------------
def _five():
    cons = [([(1, 1)], [(1, 2)], [(1, 3)]), ([(1, 3), (5, 0)], [(P - 1, 1)], [(1, 4)]), ([(2, 4)], [(1, 4), (1, 1)], [(1, 5)]),
            ([(1, 5)], [(1, 0)], [(1, 5)]), ([(1, 0)], [(7, 0)], [(7, 0)])]
    x, y = 11, 13
    w3 = x * y % P
    w4 = (w3 + 5) * (P - x) % P
    return 6, cons, [1, x, y, w3, w4, 2 * w4 * (w4 + x) % P]


def _mimc91():
    n_wires, cons = synth.mimc7_demo_constraints(91)
    return n_wires, cons, synth.mimc7_demo_witness(3, 4, nrounds=91)


def _used(C, L):
    width = C.shape[1]
    return [cdense.from_limbs(C[j])[width - int(L[j]):] for j in range(C.shape[0])]


def _oracle_proof(cons, n_wires, w, z, rho):
    """The two sumchecks from the oracle alone: the zero-check on ogkr_r1cs_rows' tables, the product at degree 2 on
    {ogkr_r1cs_cols' table at the zero-check's challenges, the witness zero-padded}."""
    n, n_y = table_log2(len(cons)), n_y_of(n_wires)
    flat = flatten(cons)
    tables = cdense.r1cs_rows_raw(*flat, n_wires, cdense.to_limbs(w), n)
    CX, LX, RX, EX, _ = cdense.sumcheck_zerocheck_raw(tables, n, 3, R1CS_ZEROCHECK_TERMS, cdense.to_limbs(z))
    pair = np.zeros((2, 1 << n_y, 4), dtype=np.uint64)
    pair[0] = cdense.r1cs_cols_raw(*flat, n_wires, RX, cdense.to_limbs(rho), n_y)
    pair[1, :n_wires] = cdense.to_limbs(w)
    CY, LY, RY, EY = cdense.sumcheck_product_raw(pair, n_y, 2)
    return _used(CX, LX), cdense.from_limbs(RX), cdense.from_limbs(EX), _used(CY, LY), cdense.from_limbs(RY), cdense.from_limbs(EY)


@pytest.mark.parametrize("system", [_five, _mimc91], ids=["five", "mimc91"])
def test_oracle_proofs_pass_the_python_verifier_and_tampered_ones_do_not(system):
    n_wires, cons, w = system()
    rng = random.Random(32000 + n_wires)
    n = table_log2(len(cons))
    z, rho = _point(rng, n, False), [rng.randrange(1, P) for _ in range(3)]
    assert first_bad(cons, w, n) is None
    proof = _oracle_proof(cons, n_wires, w, z, rho)
    assert verify_r1cs(cons, z, rho, *proof) == (0, 0, 0)
    assert verify_r1cs(cons, z, rho, *proof, witness=w) == (0, 0, 0)
    n_y = n_y_of(n_wires)
    # a changed coefficient of the last round vector of either sumcheck, changed evaluations, another matrix, another witness
    gx, rx, ex, gy, ry, ey = proof
    bumped = [g[:] for g in gx]
    bumped[-1][-1] = (bumped[-1][-1] + 1) % P
    assert verify_r1cs(cons, z, rho, bumped, rx, ex, gy, ry, ey)[0] == 1
    assert verify_r1cs(cons, z, rho, gx, rx, [ex[0], ex[1], (ex[2] + 1) % P], gy, ry, ey)[0] == 1
    bumped = [g[:] for g in gy]
    bumped[0][-1] = (bumped[0][-1] + 1) % P
    assert verify_r1cs(cons, z, rho, gx, rx, ex, bumped, ry, ey)[0] == 2
    other = [tuple([((c + 1) % P, k) for c, k in lc] if i == len(cons) - 1 and m == 2 else lc for m, lc in enumerate(con)) for i, con in enumerate(cons)]
    assert verify_r1cs(other, z, rho, *proof)[::2] == (3, 11)                     # GKR_VERIFY_MATRIX
    w2 = w[:]
    w2[n_wires - 1] = (w2[n_wires - 1] + 1) % P
    assert verify_r1cs(cons, z, rho, *proof, witness=w2) == (4, n_y, 12)          # GKR_VERIFY_WITNESS
    # a broken witness: the oracle's zero-check claims something else than zero, and the verifier says so in round 0
    assert first_bad(cons, w2, n) is not None
    broken = _oracle_proof(cons, n_wires, w2, z, rho)
    g0 = broken[0][0]
    assert (sum(g0) + g0[-1]) % P != 0
    assert verify_r1cs(cons, z, rho, *broken)[:2] == (1, 0)


# ---- c. n_x = n_y = 16 ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    system = generate(1 << 16, 1 << 16, 1616)
    return system, witness(system, "random", 1617)


def test_two_identities_tie_the_three_functions_together_at_2_to_the_16(large):
    system, w_limbs = large
    n = n_y = 16
    rng = random.Random(33000)
    x, y, rho = _point(rng, n, False), _point(rng, n_y, False), [rng.randrange(P) for _ in range(3)]
    X, Y = cdense.to_limbs(x), cdense.to_limbs(y)
    tables = cdense.r1cs_rows_raw(*system.flat(), system.n_wires, w_limbs, n)
    T = cdense.r1cs_cols_raw(*system.flat(), system.n_wires, X, cdense.to_limbs(rho), n_y)
    w, t = cdense.from_limbs(w_limbs), cdense.from_limbs(T)
    e = eq_table(x)
    weighted = 0
    for m in range(3):
        weighted += rho[m] * sum(a * b for a, b in zip(e, cdense.from_limbs(tables[m])))
    assert sum(a * b for a, b in zip(t, w)) % P == weighted % P
    evals = cdense.from_limbs(cdense.r1cs_matrix_evals_raw(*system.flat(), system.n_wires, X, Y))
    for m in range(3):
        unit = cdense.to_limbs([int(k == m) for k in range(3)])
        assert evals[m] == mle_eval(cdense.from_limbs(cdense.r1cs_cols_raw(*system.flat(), system.n_wires, X, unit, n_y)), y), m
    assert all(evals)


def test_the_array_built_system_is_what_it_claims_and_its_witness_satisfies_it(large):
    """The properties tests/test_gpu_r1cs_sizes.py relies on, from the library's own csr_info / csc_info; the library's export of
    the built system is the arrays; first_bad from the oracle: none for the witness, the row of a changed output wire otherwise."""
    system, w_limbs = large
    r1cs = build_r1cs(*system.flat(), system.n_wires)
    csr, csc = r1cs.csr_info(), r1cs.csc_info()
    long_rows = system.long_rows()
    assert csr["n"] == 16 and csc["n_y"] == 16 and csr["n_constraints"] == 1 << 16 and csr["n_wires"] == 1 << 16
    assert csr["n_long_rows"] == [len(l) for l in long_rows] and csr["n_terms"] == system.nonzero_terms().sum(axis=0).tolist()
    assert len(long_rows[0]) > len(long_rows[1]) > 20 and len(long_rows[2]) == 0
    assert int(long_rows[0][-1]) == (1 << 16) - 1 and int(system.counts[-3]) > 4096           # the last row, several thousand terms
    assert system.column_lengths(0) == [1 << 16] * 3 and (1 << 16) // SEG == 32
    for m in range(3):
        col_ptr, terms, long_cols, _ = r1cs.csc(m)
        assert int(col_ptr[1]) == 1 << 16 and np.array_equal(terms[:1 << 16, 0], np.arange(1 << 16, dtype=np.uint32))
        assert len(long_cols) == csc["n_long_cols"][m]
    counts, wires, coeffs = (np.zeros_like(a) for a in system.flat())
    from gkr_amd import _native as N
    assert N.lib().gkr_r1cs_export(r1cs._h, cdense._p(counts), cdense._p(wires), cdense._p(coeffs)) == 0
    assert np.array_equal(counts, system.counts) and np.array_equal(wires, system.wires) and np.array_equal(coeffs, system.coeffs)
    # +-1 dominate
    ones = (system.coeffs == cdense.to_limbs([1])[0]).all(axis=1) | (system.coeffs == cdense.to_limbs([P - 1])[0]).all(axis=1)
    assert 0.75 < ones.mean() < 0.97 and (system.coeffs == cdense.to_limbs([P - 2])[0]).all(axis=1).sum() > 600
    tables = cdense.r1cs_rows_raw(*system.flat(), system.n_wires, w_limbs, 16)
    assert r1cs_systems.first_bad(tables, 1 << 16) == NO_BAD
    for wire, row in ((system.n_wires - 1, (1 << 16) - 1), (system.n_in + 2567, 2567)):
        broken = w_limbs.copy()
        broken[wire, 0] ^= np.uint64(1)
        assert r1cs_systems.first_bad(cdense.r1cs_rows_raw(*system.flat(), system.n_wires, broken, 16), 1 << 16) == row
    # the integer model on the first 300 constraints
    cons = constraints_of(*system.flat(), 300)
    w = cdense.from_limbs(w_limbs)
    assert [cdense.from_limbs(tables[m, :300]) for m in range(3)] == [t[:300] for t in rows(cons, w, 9)]
    assert LONG == 32


# ---- d. thread counts -------------------------------------------------------------------------------------------------------------------
def test_the_results_do_not_depend_on_the_thread_count(large):
    system, w_limbs = large
    X, Y, rho = cdense.fill_table(16, 34000), cdense.fill_table(16, 34001), cdense.fill_table(3, 34002)
    want = None
    for threads in (1, 3, cdense.usable_threads()):
        got = (cdense.r1cs_rows_raw(*system.flat(), system.n_wires, w_limbs, 16, threads=threads),
               cdense.r1cs_cols_raw(*system.flat(), system.n_wires, X, rho, 16, threads=threads),
               cdense.r1cs_matrix_evals_raw(*system.flat(), system.n_wires, X, Y, threads=threads))
        want = want or got
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), threads


# ---- e. bad shapes ----------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_are_errors():
    cons = [([(1, 0)], [(2, 1)], [(3, 2)]), ([(4, 3)], [(5, 0)], [(6, 1)]), ([(7, 2)], [(8, 3)], [(9, 0)])]
    counts, wires, coeffs = flatten(cons)
    W, X, Y, rho = cdense.fill_table(4, 1), cdense.fill_table(2, 2), cdense.fill_table(2, 3), cdense.fill_table(3, 4)
    cdense.r1cs_rows_raw(counts, wires, coeffs, 4, W, 2)                                     # (the good shape next to them)
    cdense.r1cs_cols_raw(counts, wires, coeffs, 4, X, rho, 2)
    cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, 4, X, Y)
    big = np.full(4, (1 << 64) - 1, dtype=np.uint64)
    bad_coeffs = coeffs.copy()
    bad_coeffs[4] = big
    bad_w, bad_x, bad_rho = W.copy(), X.copy(), rho.copy()
    bad_w[3], bad_x[1], bad_rho[2] = big, big, big
    calls = [lambda: cdense.r1cs_rows_raw(counts, wires, coeffs, 4, W, 1),                   # n_constraints > 2^n
             lambda: cdense.r1cs_rows_raw(counts, wires, coeffs, 3, W[:3], 2),               # a wire >= n_wires
             lambda: cdense.r1cs_rows_raw(counts, wires, bad_coeffs, 4, W, 2),
             lambda: cdense.r1cs_rows_raw(counts, wires, coeffs, 4, bad_w, 2),
             lambda: cdense.r1cs_rows_raw(counts, wires, coeffs, 4, W[:3], 2),               # a witness of another length
             lambda: cdense.r1cs_rows_raw(counts[:8], wires, coeffs, 4, W, 2),               # counts that do not match
             lambda: cdense.r1cs_rows_raw(counts, wires[:8], coeffs, 4, W, 2),
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 4, X[:1], rho, 2),          # n_constraints > 2^n_x
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 4, X, rho, 1),              # n_wires > 2^n_y
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 3, X, rho, 2),
             lambda: cdense.r1cs_cols_raw(counts, wires, bad_coeffs, 4, X, rho, 2),
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 4, bad_x, rho, 2),
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 4, X, bad_rho, 2),
             lambda: cdense.r1cs_cols_raw(counts, wires, coeffs, 4, X, rho[:2], 2),
             lambda: cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, 4, X[:1], Y),
             lambda: cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, 4, X, Y[:1]),
             lambda: cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, 3, X, Y),
             lambda: cdense.r1cs_matrix_evals_raw(counts, wires, bad_coeffs, 4, X, Y),
             lambda: cdense.r1cs_matrix_evals_raw(counts, wires, coeffs, 4, bad_x, Y),
             lambda: cdense.fr_mul_many(W, X)]
    for at, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was accepted" % at)
    # the return value itself: -1, not another error
    import ctypes
    out = np.zeros((3 << 2, 4), dtype=np.uint64)
    fn = cdense.lib().ogkr_r1cs_rows
    fn.restype = ctypes.c_int
    args = lambda n_wires, n: (ctypes.c_size_t(3), ctypes.c_uint32(n_wires), cdense._p(counts), cdense._p(wires), cdense._p(coeffs), cdense._p(W), ctypes.c_int(n),
                               cdense._p(out), ctypes.c_int(1))
    assert fn(*args(4, 2)) == 0 and fn(*args(4, 1)) == -1 and fn(*args(3, 2)) == -1


def test_the_vector_product_and_sum_equal_the_scalar_ones():
    a, b = cdense.fill_table(50, 5), cdense.fill_table(50, 6)
    a[0], b[0], a[1] = cdense.to_limbs([P - 1, P - 1, 0])
    ia, ib = cdense.from_limbs(a), cdense.from_limbs(b)
    assert cdense.from_limbs(cdense.fr_mul_many(a, b)) == [x * y % P for x, y in zip(ia, ib)]
    assert cdense.from_limbs(cdense.fr_add_many(a, b)) == [(x + y) % P for x, y in zip(ia, ib)]


# ---- f. under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """`make -C oracle/c r1cs_selfcheck`: n and n_y from 2 to 9, the three functions with 1 and 4 threads give equal bytes, the two
    identities with eq tables the program builds entry by entry, zero padding, the refusals; no sanitizer report.  A child
    process: nothing is loaded into this one."""
    exe = str(tmp_path / "r1cs_selfcheck")
    build = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "c"), "r1cs_selfcheck", "OUT=" + exe], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "r1cs_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

"""The R1CS inner sumcheck (include/gkr_amd.h, gkr_r1cs_csc_* / gkr_r1cs_cols_* / gkr_r1cs_inner*) as far as no device is needed:
the symbols, the column-major flattening of csrc/r1cs.cpp against its restatement in tests/r1cs_cols_model.py and against the CSR
form, the identity  sum_y T(y) w(y) = sum_m rho_m Mz_m~(rx)  and  T~(ry) = sum_m rho_m M_m~(rx, ry)  on integers, the host verifier
verify_r1cs_inner on the product model's transcripts, the argument checks that return before a device is touched, and a
stand-alone program under AddressSanitizer and UBSan (a child process: no sanitizer goes near code loaded into python)."""

import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import gkr_amd
from gkr_amd import _native as N
from gkr_amd import synth
from gkr_amd.convert import R1cs
from gkr_amd.field import MODULUS as P
from gkr_amd.prover import Context, GkrError, R1csCols
from gkr_amd.verifier import mle_eval, r1cs_matrix_evals, verify_r1cs_inner
from product_model import product_sumcheck
from r1cs_cols_model import LONG_COL, cols_table, csc, eq_table, n_y_of
from r1cs_rows_model import csr, rows, table_log2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_r1cs_csc_info", "gkr_r1cs_csc_export", "gkr_r1cs_cols_prepare", "gkr_r1cs_cols_prepare_segment", "gkr_r1cs_cols_info",
         "gkr_r1cs_cols_free", "gkr_r1cs_cols_device", "gkr_r1cs_inner_batch_device", "gkr_r1cs_inner"]


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    kernels = open(os.path.join(REPO, "gkr_amd", "csrc", "kernels.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("r1cs_cols", "r1cs_cols_device", "r1cs_inner_batch_device", "prove_r1cs_inner"):
        assert callable(getattr(Context, name)), name
    for name in ("info", "close", "__enter__", "__exit__"):
        assert callable(getattr(R1csCols, name)), name
    assert callable(R1cs.csc) and callable(R1cs.csc_info) and callable(gkr_amd.prove_r1cs_inner)
    for name in ("prove_r1cs_inner", "R1csCols", "verify_r1cs_inner", "r1cs_matrix_evals"):
        assert name in gkr_amd.__all__, name
    assert int(re.search(r"#define\s+GKR_R1CS_LONG_COL\s+(\d+)", header).group(1)) == LONG_COL == N.GKR_R1CS_LONG_COL
    assert re.search(r"kR1csLongCol = %d;" % LONG_COL, kernels)
    segment = int(re.search(r"#define\s+GKR_R1CS_COL_SEGMENT\s+(\d+)", header).group(1))
    assert segment == N.GKR_R1CS_COL_SEGMENT and re.search(r"kR1csColSegment = %d;" % segment, kernels)
    assert ctypes.sizeof(N.R1csCscInfo) == 16 + 8 * 8                      # three uint32 and padding, then eight size_t


def _assert_csc_is_the_model(r1cs, constraints, n_wires):
    mats, pool = csc(constraints, n_wires)
    csr_mats, csr_pool = csr(constraints)
    inf = r1cs.csc_info()
    cinf = r1cs.csr_info()
    assert inf["n_constraints"] == len(constraints) and inf["n_x"] == table_log2(len(constraints)) == cinf["n"]
    assert inf["n_y"] == n_y_of(n_wires) and inf["n_wires"] == n_wires and inf["n_pool"] == len(pool) == cinf["n_pool"]
    assert inf["n_terms"] == cinf["n_terms"]
    for m in range(3):
        col_ptr, terms, long_cols, got_pool = r1cs.csc(m)
        want_ptr, want_terms, want_long = mats[m]
        assert col_ptr.dtype == np.uint32 and terms.dtype == np.uint32 and long_cols.dtype == np.uint32
        assert col_ptr.tolist() == want_ptr and len(col_ptr) == n_wires + 1, m
        assert [tuple(t) for t in terms.tolist()] == want_terms, m
        assert long_cols.tolist() == want_long, m
        assert got_pool == pool == csr_pool == r1cs.csr(m)[3] and got_pool[:2] == [1, P - 1], m
        assert inf["n_terms"][m] == len(want_terms) and inf["n_long_cols"][m] == len(want_long)
        # the CSC records re-sorted by (row, CSR order) are the CSR records: within a row the CSR order is the order of the
        # record's position in its column list only per wire, so rebuild the rows from the CSR walk and compare as multisets per
        # row AND as the exact sequence through the stable inverse sort
        row_ptr, csr_terms, _, _ = r1cs.csr(m)
        tagged = []
        for y in range(n_wires):
            for t in range(int(col_ptr[y]), int(col_ptr[y + 1])):
                tagged.append((int(terms[t][0]), y, int(terms[t][1])))
        position = {}                                                     # (row, wire) -> the CSR positions of that wire in that row, in order
        for i in range(len(constraints)):
            for t in range(int(row_ptr[i]), int(row_ptr[i + 1])):
                position.setdefault((i, int(csr_terms[t][0])), []).append(t)
        back = [None] * len(csr_terms)
        seen = {}
        for row, y, c in tagged:                                          # a column's records of one row keep the CSR order
            k = seen.get((row, y), 0)
            seen[(row, y)] = k + 1
            back[position[(row, y)][k]] = (y, c)
        assert back == [tuple(t) for t in csr_terms.tolist()], m
        for y in range(n_wires):                                          # ascending rows within a column
            col_rows = terms[int(col_ptr[y]):int(col_ptr[y + 1]), 0].tolist()
            assert col_rows == sorted(col_rows), (m, y)
    return mats, pool


def test_csc_of_the_mimc_chains():
    for nr, style in ((3, "plain"), (91, "negated")):
        n_wires, cons = synth.mimc7_demo_constraints(nr, style)
        mats, pool = _assert_csc_is_the_model(synth.mimc7_demo_r1cs(nr, style), cons, n_wires)
        assert sum(len(m[1]) for m in mats) == sum(len(lc) for con in cons for lc in con)   # no zero coefficient in the chains


def _hand_built():
    """Eight wires (a power of two), 33 constraints.  Wire 0 stands in every constraint of A, B and C: columns of 33 records, long
    in all three.  Wire 1: the first 32 constraints of A (exactly LONG_COL records: short) and all 33 of B with a repeat in row 7
    (34 records).  Wire 2 twice in row 5 of A.  Zero coefficients on wires 3 and 6 are dropped (wire 6 appears nowhere else: an
    empty column), wire 7 is unused."""
    cons = []
    for i in range(33):
        a = [(1, 0)] + ([((P - 1, 5 + i)[i % 2], 1)] if i < 32 else []) + [(0, 3)]
        b = [(P - 1, 0), (7, 1)] + ([(9, 1)] if i == 7 else [])
        c = [(0, 6), (3 + i % 2, 0), (1, 4 + i % 2)]
        if i == 5:
            a += [(11, 2), (1, 3), (12, 2)]
        cons.append((a, b, c))
    return 8, cons


def test_csc_of_a_hand_built_system():
    nw, cons = _hand_built()
    r1cs = R1cs.build(nw, 1, 1, 1, cons)
    mats, pool = _assert_csc_is_the_model(r1cs, cons, nw)
    lens = [[m[0][y + 1] - m[0][y] for y in range(nw)] for m in mats]
    assert lens[0] == [33, LONG_COL, 2, 1, 0, 0, 0, 0] and lens[1] == [33, LONG_COL + 2, 0, 0, 0, 0, 0, 0]
    assert lens[2] == [33, 0, 0, 0, 17, 16, 0, 0]
    assert [m[2] for m in mats] == [[0], [0, 1], [0]]                    # exactly 32 records: not long; 33: long
    assert mats[0][1][33 + 32:33 + 34] == [(5, pool.index(11)), (5, pool.index(12))]   # the repeated wire: two records, one row, CSR order
    assert mats[1][1][33 + 7:33 + 9] == [(7, pool.index(7)), (7, pool.index(9))]
    assert r1cs.csc_info()["n_y"] == 3 and r1cs.csc_info()["n_x"] == 6


def test_csc_of_one_wire_and_sizes():
    cons = [([(1, 0)], [(2, 0), (P - 1, 0)], [(i + 3, 0)]) for i in range(5)]
    r1cs = R1cs.build(1, 1, 0, 0, cons)
    mats, pool = _assert_csc_is_the_model(r1cs, cons, 1)
    assert r1cs.csc_info() == dict(n_x=3, n_y=2, n_wires=1, n_constraints=5, n_terms=[5, 10, 5], n_long_cols=[0, 0, 0], n_pool=8)
    assert mats[1][0] == [0, 10] and mats[1][1][:2] == [(0, pool.index(2)), (0, 1)]
    for n_wires, n_y in ((2, 2), (4, 2), (5, 3), (256, 8), (257, 9)):
        assert n_y_of(n_wires) == n_y
        assert R1cs.build(n_wires, 1, 1, 1, [([(1, n_wires - 1)], [], [])]).csc_info()["n_y"] == n_y


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    good = synth.mimc7_demo_r1cs(3)
    info = N.R1csCscInfo()
    assert lib.gkr_r1cs_csc_info(None, ctypes.byref(info)) == INVALID and lib.gkr_r1cs_csc_info(good._h, None) == INVALID
    empty = R1cs.build(4, 1, 1, 1, [])
    no_wires = R1cs.build(0, 0, 0, 0, [([], [], [])])
    for bad in (empty, no_wires):
        assert lib.gkr_r1cs_csc_info(bad._h, ctypes.byref(info)) == INVALID
        assert lib.gkr_r1cs_csc_export(bad._h, 0, None, None, None, None) == INVALID
        with pytest.raises(GkrError) as e:
            bad.csc_info()
        assert e.value.status == INVALID
    for matrix in (-1, 3, 255):
        assert lib.gkr_r1cs_csc_export(good._h, matrix, None, None, None, None) == INVALID
    assert lib.gkr_r1cs_csc_export(None, 0, None, None, None, None) == INVALID
    assert lib.gkr_r1cs_csc_export(good._h, 2, None, None, None, None) == 0              # every output may be NULL
    with pytest.raises(GkrError):
        good.csc(3)
    out = ctypes.c_void_p()
    for prep, extra in ((lib.gkr_r1cs_cols_prepare, ()), (lib.gkr_r1cs_cols_prepare_segment, (2048,))):
        assert prep(None, good._h, *extra, ctypes.byref(out)) == INVALID and prep(fake, None, *extra, ctypes.byref(out)) == INVALID
        assert prep(fake, good._h, *extra, None) == INVALID
        assert prep(fake, empty._h, *extra, ctypes.byref(out)) == INVALID and not out.value   # refused by the info call, before the context
    assert lib.gkr_r1cs_cols_prepare_segment(fake, good._h, 63, ctypes.byref(out)) == INVALID  # a segment below a wave's width
    assert lib.gkr_r1cs_cols_info(None, ctypes.byref(info)) == INVALID
    lib.gkr_r1cs_cols_free(None)                                                          # a no-op
    # without a device there is no handle, so only the NULLs are reached here (the rest: tests/test_gpu_r1cs_inner.py)
    assert lib.gkr_r1cs_cols_device(None, fake, fake, fake, 1, fake, 16) == INVALID
    assert lib.gkr_r1cs_cols_device(fake, None, fake, fake, 1, fake, 16) == INVALID
    assert lib.gkr_r1cs_inner_batch_device(None, fake, fake, 16, 1, fake, fake, fake, fake, fake, None) == INVALID
    assert lib.gkr_r1cs_inner_batch_device(fake, None, fake, 16, 1, fake, fake, fake, fake, fake, None) == INVALID
    # ctx, r1cs, witness, n_witness, x, rho, out_coeffs, out_len, out_r, out_evals
    host = lib.gkr_r1cs_inner
    ok = [fake, good._h, fake, 15, fake, fake, fake, fake, fake, None]
    for at in (0, 1, 2, 4, 5, 6, 7, 8):
        args = list(ok)
        args[at] = None
        assert host(*args) == INVALID, at
    args = list(ok)
    args[3] = 14                                                                          # n_witness < n_wires = 15
    assert host(*args) == INVALID
    args[1], args[3] = empty._h, 15
    assert host(*args) == INVALID
    assert not any(word)                                                                  # nothing was written


def _random_system(rng, n_constraints, n_wires):
    def lc():
        return [((1, P - 1, rng.randrange(P), 0)[rng.randrange(4)], rng.randrange(n_wires)) for _ in range(rng.randrange(4))]
    return [(lc(), lc(), lc()) for _ in range(n_constraints)]


@pytest.mark.parametrize("n_x", [2, 3, 4])
@pytest.mark.parametrize("n_y", [2, 3, 4])
def test_the_identity_of_the_inner_sumcheck_on_integers(n_x, n_y):
    """For random and boolean rx, a satisfied-looking and an arbitrary ("broken") witness -- the identity holds for EVERY witness:
    sum_y T(y) w(y) == sum_m rho_m rows(..)[m]~(rx), and sum_m rho_m M_m~(rx, ry) == T~(ry); a boolean rx picks row i:
    T == sum_m rho_m (row i of M_m)."""
    rng = random.Random(1900 + 10 * n_x + n_y)
    n_constraints = (1 << n_x) - (1 if n_x > 2 else 0)
    n_wires = (1 << n_y) - (n_y % 2)
    assert table_log2(n_constraints) == n_x and n_y_of(n_wires) == n_y
    cons = _random_system(rng, n_constraints, n_wires)
    for boolean in (False, True):
        rx = [rng.randrange(2) if boolean else rng.randrange(P) for _ in range(n_x)]
        for witness in ("ones", "random"):
            w = [1] * n_wires if witness == "ones" else [rng.randrange(P) for _ in range(n_wires)]
            rho = [rng.randrange(P) for _ in range(3)]
            T = cols_table(cons, n_wires, rx, rho, n_y)
            assert not any(T[n_wires:])
            tabs = rows(cons, w, n_x)
            want = sum(r * mle_eval(t, rx) for r, t in zip(rho, tabs)) % P
            assert sum(t * v for t, v in zip(T, w)) % P == want
            ry = [rng.randrange(P) for _ in range(n_y)]
            assert sum(r * v for r, v in zip(rho, r1cs_matrix_evals(cons, rx, ry))) % P == mle_eval(T, ry)
            if boolean:
                i = int("".join(str(b) for b in rx), 2)
                row = [0] * (1 << n_y)
                if i < n_constraints:
                    for m in range(3):
                        for c, y in cons[i][m]:
                            row[y] = (row[y] + rho[m] * c) % P
                assert T == row and eq_table(rx)[i] == 1


def test_verify_r1cs_inner_accepts_the_models_transcripts_and_rejects_single_changes():
    rng = random.Random(1950)
    n_wires, cons = synth.mimc7_demo_constraints(4)
    n_x, n_y = 4, n_y_of(n_wires)
    good = synth.mimc7_demo_witness(2, 3, nrounds=4)
    broken = list(good)
    broken[9] = (broken[9] + 1) % P
    for w in (good, broken):
        rx = [rng.randrange(P) for _ in range(n_x)]
        rho = [rng.randrange(1, P) for _ in range(3)]
        claims = [mle_eval(t, rx) for t in rows(cons, w, n_x)]
        T = cols_table(cons, n_wires, rx, rho, n_y)
        wp = list(w) + [0] * ((1 << n_y) - n_wires)
        proof, r, evals = product_sumcheck([T, wp], n_y)
        left = verify_r1cs_inner(cons, rx, rho, claims, proof, r, evals)
        assert left == (r, mle_eval(wp, r)) and left[1] == evals[1]
        # one rho
        for m in range(3):
            bad = list(rho)
            bad[m] = (bad[m] + 1) % P
            assert verify_r1cs_inner(cons, rx, bad, claims, proof, r, evals) is None
        # one claim
        for m in range(3):
            bad = list(claims)
            bad[m] = (bad[m] + 1) % P
            assert verify_r1cs_inner(cons, rx, rho, bad, proof, r, evals) is None
        # one matrix coefficient (the round checks still pass: the last check against the public matrices fails)
        for m in range(3):
            i = next(k for k, con in enumerate(cons) if con[m])
            other = [tuple(list(lc) for lc in con) for con in cons]
            c, y = other[i][m][0]
            other[i][m][0] = ((c + 1) % P, y)
            assert verify_r1cs_inner(other, rx, rho, claims, proof, r, evals) is None
        # one transcript slot, one challenge, evals[0], evals[1]
        for j in range(n_y):
            for k in range(len(proof[j])):
                bad = [list(g) for g in proof]
                bad[j][k] = (bad[j][k] + 1) % P
                assert verify_r1cs_inner(cons, rx, rho, claims, bad, r, evals) is None
            bad = list(r)
            bad[j] = (bad[j] + 1) % P
            assert verify_r1cs_inner(cons, rx, rho, claims, proof, bad, evals) is None
        for k in range(2):
            bad = list(evals)
            bad[k] = (bad[k] + 1) % P
            assert verify_r1cs_inner(cons, rx, rho, claims, proof, r, bad) is None
        assert verify_r1cs_inner(cons, rx, rho[:2], claims, proof, r, evals) is None
        assert verify_r1cs_inner(cons, rx[:3], rho, claims, proof, r, evals) is None     # too few row variables for the constraints


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """tests/r1cs_csc_selfcheck.cpp with csrc/r1cs.cpp: the hand-built system and a one-wire system through gkr_r1cs_build, the three
    matrices' columns against the CSR export, every array at its exact size and NULL for every optional output; no sanitizer
    report.  A child process: nothing is loaded into this one."""
    exe = str(tmp_path / "r1cs_csc_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-pthread",
                            os.path.join(REPO, "tests", "r1cs_csc_selfcheck.cpp"), os.path.join(REPO, "gkr_amd", "csrc", "r1cs.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "r1cs_csc_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

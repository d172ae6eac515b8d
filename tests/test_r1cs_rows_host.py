"""The R1CS zero-check (include/gkr_amd.h, gkr_r1cs_csr_* / gkr_r1cs_rows_* / gkr_r1cs_zerocheck*) as far as no device is needed:
the symbols, the CSR flattening of csrc/r1cs.cpp against its restatement in tests/r1cs_rows_model.py, the sizes, the argument
checks that return before a device is touched, the integer model of the tables under the zero-check's model and host verifier,
and a stand-alone program under AddressSanitizer and UBSan (a child process: no sanitizer goes near code loaded into python).

Not reached here: GKR_ERR_UNSUPPORTED (more than 2^32 - 1 terms in one matrix) and n > GKR_MAX_MLE_N (more than 2^30
constraints) need an R1CS of more than a hundred GiB of host memory."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import gkr_amd
from gkr_amd import _native as N
from gkr_amd import synth
from gkr_amd.convert import R1cs
from gkr_amd.field import MODULUS as P
from gkr_amd.prover import Context, GkrError, R1csRows
from gkr_amd.verifier import R1CS_ZEROCHECK_TERMS, verify_sumcheck_zerocheck
from r1cs_rows_model import LONG_ROW, csr, first_bad, rows, table_log2
from zerocheck_model import zerocheck_claim, zerocheck_sumcheck

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_r1cs_csr_info", "gkr_r1cs_csr_export", "gkr_r1cs_rows_prepare", "gkr_r1cs_rows_info", "gkr_r1cs_rows_free",
         "gkr_r1cs_rows_device", "gkr_r1cs_zerocheck_batch_device", "gkr_r1cs_zerocheck"]


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("r1cs_rows", "r1cs_rows_device", "r1cs_zerocheck_batch_device", "prove_r1cs_zerocheck"):
        assert callable(getattr(Context, name)), name
    for name in ("info", "close", "__enter__", "__exit__"):
        assert callable(getattr(R1csRows, name)), name
    assert callable(R1cs.csr) and callable(R1cs.csr_info) and callable(gkr_amd.prove_r1cs_zerocheck)
    assert "prove_r1cs_zerocheck" in gkr_amd.__all__
    assert R1CS_ZEROCHECK_TERMS == [(1, (0, 1)), (P - 1, (2,))]
    assert int(re.search(r"#define\s+GKR_R1CS_LONG_ROW\s+(\d+)", header).group(1)) == LONG_ROW == N.GKR_R1CS_LONG_ROW
    assert re.search(r"kR1csLongRow = %d;" % LONG_ROW, open(os.path.join(REPO, "gkr_amd", "csrc", "kernels.h")).read())


def _assert_csr_is_the_model(r1cs, constraints):
    mats, pool = csr(constraints)
    inf = r1cs.csr_info()
    assert inf["n_constraints"] == len(constraints) and inf["n"] == table_log2(len(constraints)) and inf["n_pool"] == len(pool)
    for m in range(3):
        row_ptr, terms, long_rows, got_pool = r1cs.csr(m)
        want_ptr, want_terms, want_long = mats[m]
        assert row_ptr.dtype == np.uint32 and terms.dtype == np.uint32 and long_rows.dtype == np.uint32
        assert row_ptr.tolist() == want_ptr, m
        assert [tuple(t) for t in terms.tolist()] == want_terms, m
        assert long_rows.tolist() == want_long, m
        assert got_pool == pool and got_pool[:2] == [1, P - 1], m
        assert inf["n_terms"][m] == len(want_terms) and inf["n_long_rows"][m] == len(want_long)
    return mats, pool


def test_csr_of_the_mimc_chain():
    n_wires, cons = synth.mimc7_demo_constraints(3)
    mats, pool = _assert_csr_is_the_model(synth.mimc7_demo_r1cs(3), cons)
    assert len(pool) == 4 and not any(m[2] for m in mats)         # 1, r - 1 and the round constants of rounds 2 and 3


def test_csr_of_the_negated_chain_has_one_pool_of_one_minus_one_and_the_round_constants():
    n_wires, cons = synth.mimc7_demo_constraints(91, "negated")
    r1cs = synth.mimc7_demo_r1cs(91, "negated")
    assert r1cs.constraints() == cons
    mats, pool = _assert_csr_is_the_model(r1cs, cons)
    used = {c for m in mats for _, c in m[1]}
    assert {0, 1} <= used and len(pool) > 80 and used == set(range(len(pool)))


def _hand_built():
    """Row 0: an empty A.  Row 1: a zero coefficient (dropped) and a wire repeated.  Rows 2, 3: LONG_ROW and LONG_ROW + 1 terms
    in B (the second one alone is long; the zero coefficient in front of row 2's terms does not count).  Row 4: all three empty."""
    nw = 11
    long_a = [(0, 4)] + [((5 + t) if t % 3 else P - 1, (3 * t) % nw) for t in range(LONG_ROW)]
    long_b = [((7 + t) if t % 4 else 1, (5 * t + 1) % nw) for t in range(LONG_ROW + 1)]
    cons = [([], [(1, 1)], [(P - 2, 2)]),
            ([(3, 2), (0, 5), (3, 2), (P - 1, 2)], [(1, 0)], [(0, 7)]),
            ([(1, 1)], long_a, [(1, 3)]),
            ([(2, 1)], long_b, [(1, 3), (1, 3)]),
            ([], [], [])]
    return nw, cons


def test_csr_of_a_hand_built_system():
    nw, cons = _hand_built()
    r1cs = R1cs.build(nw, 1, 1, 1, cons)
    mats, pool = _assert_csr_is_the_model(r1cs, cons)
    assert mats[0][0][:2] == [0, 0] and mats[0][0][2] == 3        # the empty A; the zero coefficient is gone, the repeated wire stays
    assert mats[0][1][:3] == [(2, pool.index(3)), (2, pool.index(3)), (2, 1)]
    assert mats[1][0][3] - mats[1][0][2] == LONG_ROW and mats[1][0][4] - mats[1][0][3] == LONG_ROW + 1
    assert mats[1][2] == [3] and mats[0][2] == [] and mats[2][2] == []
    assert mats[2][0] == [0, 1, 1, 2, 4, 4]                       # C of row 1 was the zero coefficient alone: an empty row
    assert pool[2] == P - 2                                       # first appearance: row 0's C comes before row 1's A


@pytest.mark.parametrize("n_constraints,n", [(1, 2), (2, 2), (4, 2), (5, 3), (256, 8), (257, 9)])
def test_sizes_from_csr_info(n_constraints, n):
    cons = [([(1, i % 3)], [(2, (i + 1) % 3), (P - 1, 0)], [(i + 3, 2)]) for i in range(n_constraints)]
    inf = R1cs.build(3, 1, 1, 1, cons).csr_info()
    assert inf == dict(n=n, n_wires=3, n_constraints=n_constraints, n_terms=[n_constraints, 2 * n_constraints, n_constraints],
                       n_long_rows=[0, 0, 0], n_pool=3 + n_constraints)


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    good_r1cs = synth.mimc7_demo_r1cs(3)
    info = N.R1csCsrInfo()
    # section 1: the host calls
    assert lib.gkr_r1cs_csr_info(None, ctypes.byref(info)) == INVALID and lib.gkr_r1cs_csr_info(good_r1cs._h, None) == INVALID
    empty = R1cs.build(4, 1, 1, 1, [])
    no_wires = R1cs.build(0, 0, 0, 0, [([], [], [])])
    for bad in (empty, no_wires):
        assert lib.gkr_r1cs_csr_info(bad._h, ctypes.byref(info)) == INVALID
        assert lib.gkr_r1cs_csr_export(bad._h, 0, None, None, None, None) == INVALID
        with pytest.raises(GkrError) as e:
            bad.csr_info()
        assert e.value.status == INVALID
    for matrix in (-1, 3, 255):
        assert lib.gkr_r1cs_csr_export(good_r1cs._h, matrix, None, None, None, None) == INVALID
    assert lib.gkr_r1cs_csr_export(None, 0, None, None, None, None) == INVALID
    assert lib.gkr_r1cs_csr_export(good_r1cs._h, 2, None, None, None, None) == 0          # every output may be NULL
    with pytest.raises(GkrError):
        good_r1cs.csr(3)
    # section 3: NULL context or pointer (the optional outputs excepted) -- plain returns
    out = ctypes.c_void_p()
    prep = lib.gkr_r1cs_rows_prepare
    assert prep(None, good_r1cs._h, ctypes.byref(out)) == INVALID and prep(fake, None, ctypes.byref(out)) == INVALID
    assert prep(fake, good_r1cs._h, None) == INVALID
    assert prep(fake, empty._h, ctypes.byref(out)) == INVALID and not out.value           # refused by the info call, before the context
    assert lib.gkr_r1cs_rows_info(None, ctypes.byref(info)) == INVALID
    lib.gkr_r1cs_rows_free(None)                                                          # a no-op
    # ctx, rows, d_witness, stride, batch, d_out, out_first_bad: without a device there is no handle, so only the NULLs are reached here
    # (stride, batch, the 2^30 cap and a foreign handle: tests/test_gpu_r1cs_zerocheck.py)
    assert lib.gkr_r1cs_rows_device(None, fake, fake, 16, 1, fake, None) == INVALID
    assert lib.gkr_r1cs_rows_device(fake, None, fake, 16, 1, fake, None) == INVALID
    # ctx, rows, d_witness, stride, batch, z, out_coeffs, out_len, out_r, out_evals, out_eq, out_first_bad
    assert lib.gkr_r1cs_zerocheck_batch_device(None, fake, fake, 16, 1, fake, fake, fake, fake, None, None, None) == INVALID
    assert lib.gkr_r1cs_zerocheck_batch_device(fake, None, fake, 16, 1, fake, fake, fake, fake, None, None, None) == INVALID
    # ctx, r1cs, witness, n_witness, z, out_coeffs, out_len, out_r, out_evals, out_eq, out_first_bad
    host = lib.gkr_r1cs_zerocheck
    good = [fake, good_r1cs._h, fake, 15, fake, fake, fake, fake, None, None, None]
    for at in (0, 1, 2, 4, 5, 6, 7):
        args = list(good)
        args[at] = None
        assert host(*args) == INVALID, at
    args = list(good)
    args[3] = 14                                                                          # n_witness < n_wires = 15
    assert host(*args) == INVALID
    args[1], args[3] = empty._h, 15
    assert host(*args) == INVALID
    assert not any(word)                                                                  # nothing was written


def test_the_models_rows_of_a_satisfying_witness_pass_the_zero_check_on_integers():
    """mimc7_demo_r1cs(4): 16 constraints, n = 4.  a o b = c at every row, the zero-check's claim is 0 and the host verifier accepts
    its transcript with the R1CS terms; a broken witness has a first bad row, a non-zero claim and is refused with claim 0."""
    import random
    n_wires, cons = synth.mimc7_demo_constraints(4)
    assert len(cons) == 16
    w = synth.mimc7_demo_witness(2, 3, nrounds=4)
    assert len(w) == n_wires
    a, b, c = rows(cons, w, 4)
    assert all(x * y % P == v for x, y, v in zip(a, b, c)) and first_bad(cons, w, 4) is None
    rng = random.Random(1801)
    z = [rng.randrange(P) for _ in range(4)]
    proof, r, evals, eq_r = zerocheck_sumcheck([a, b, c], R1CS_ZEROCHECK_TERMS, z, 4)
    assert (sum(proof[0]) + proof[0][-1]) % P == 0 == zerocheck_claim([a, b, c], R1CS_ZEROCHECK_TERMS, z)
    assert verify_sumcheck_zerocheck(proof, r, evals, R1CS_ZEROCHECK_TERMS, z, 0)
    w2 = list(w)
    w2[9] = (w2[9] + 1) % P
    bad = first_bad(cons, w2, 4)
    assert bad is not None
    t2 = rows(cons, w2, 4)
    claim = zerocheck_claim(t2, R1CS_ZEROCHECK_TERMS, z)
    proof, r, evals, eq_r = zerocheck_sumcheck(t2, R1CS_ZEROCHECK_TERMS, z, 4)
    assert claim != 0 and verify_sumcheck_zerocheck(proof, r, evals, R1CS_ZEROCHECK_TERMS, z, claim)
    assert not verify_sumcheck_zerocheck(proof, r, evals, R1CS_ZEROCHECK_TERMS, z, 0)


def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """tests/r1cs_csr_selfcheck.cpp with csrc/r1cs.cpp: two systems through gkr_r1cs_build, the three matrices against a loop over
    gkr_r1cs_export, every array at its exact size; no sanitizer report.  A child process: nothing is loaded into this one."""
    exe = str(tmp_path / "r1cs_csr_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-pthread",
                            os.path.join(REPO, "tests", "r1cs_csr_selfcheck.cpp"), os.path.join(REPO, "gkr_amd", "csrc", "r1cs.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "r1cs_csr_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

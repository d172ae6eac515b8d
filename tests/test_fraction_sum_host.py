"""The fractional sum (LogUp) argument (include/gkr_amd.h, gkr_fraction_sum*) as far as no device is needed: the symbols, the
argument checks that return before a device is touched, the tree's launch geometry (host logic), the integer model
(tests/fraction_sum_model.py, written from the protocol on zerocheck_model and oracle.mimc7) held to the plain sum of fractions, to
every layer's claim summed entry by entry and to N~(z^(n)), D~(z^(n)); gkr_amd.verifier.verify_fraction_sum on the model's proofs
and on every single-element change of them, against the closed-form verdicts of tests/fraction_sum_sweeps.py; and the chain of
claims (csrc/fraction_sum_rounds.h) in a stand-alone program under AddressSanitizer and UBSan, on the cases this test writes out
from the model (a child process: no sanitizer goes near code loaded into python)."""

import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import gkr_amd
from gkr_amd import _native as N
from gkr_amd.prover import Context
from gkr_amd.verifier import verify_fraction_sum
from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, FRACTION_SUM, KINDS, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR,
                                fraction_sum, fraction_tree, fraction_tree_np, head_root, layer_row, layer_terms, make_tables, mle, mle_np,
                                model_verdict, proof_arrays, rounds)
from fraction_sum_sweeps import ACCEPTED, apply, check_inputs, layers_of, tamperings
from oracle.field import P
from zerocheck_model import zerocheck_claim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_fraction_sum_batch_device", "gkr_fraction_sum", "gkr_fraction_sum_verify_batch_device", "gkr_fraction_sum_verify",
         "gkr_selftest_fraction_sum_geometry", "gkr_devtest_fraction_sum_tree", "gkr_devtest_fraction_sum_chunk"]
SIZES = (3, 4, 5, 6)
CONFIGS = ((True, True), (False, True), (True, False))             # (claimed sums given, tables given)


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("fraction_sum_rounds", "fraction_sum_batch_device", "prove_fraction_sum", "verify_fraction_sum_batch_device", "verify_fraction_sum"):
        assert callable(getattr(Context, name)), name
    assert callable(gkr_amd.prove_fraction_sum) and callable(gkr_amd.verify_fraction_sum)
    assert "prove_fraction_sum" in gkr_amd.__all__ and "verify_fraction_sum" in gkr_amd.__all__
    assert re.search(r"GKR_VERIFY_ZERO_DENOMINATOR = 14\b", header) and N.GKR_VERIFY_ZERO_DENOMINATOR == 14 == ZERO_DENOMINATOR
    assert re.search(r"GKR_VERIFY_FRACTION_SUM = 15\b", header) and N.GKR_VERIFY_FRACTION_SUM == 15 == FRACTION_SUM
    assert (N.GKR_VERIFY_SHAPE, N.GKR_VERIFY_NON_CANONICAL, N.GKR_VERIFY_ROUND_SUM, N.GKR_VERIFY_CHALLENGE, N.GKR_VERIFY_FINAL_CLAIM,
            N.GKR_VERIFY_EVALUATION) == (SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION)
    assert Context.fraction_sum_rounds(3) == 2 == rounds(3) and Context.fraction_sum_rounds(17) == 135 == rounds(17)


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    # (n, batch): outside the shapes, with batch * 2^(n+1) = 2^31 at (30, 1), (29, 2) and (20, 1024)
    shapes = ((2, 1), (0, 1), (-1, 1), (31, 1), (3, 0), (3, -1), (3, 65536), (30, 1), (29, 2), (20, 1024))
    # ctx, tables, n, batch, out_sums, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims
    good = [fake, fake, 3, 1] + [fake] * 8
    for at in (0, 1, 4, 5, 6, 7, 8):                               # (9 .. 11, the optional outputs, may be NULL)
        args = list(good)
        args[at] = None
        assert lib.gkr_fraction_sum_batch_device(*args) == INVALID, at
    for n, batch in shapes:
        assert lib.gkr_fraction_sum_batch_device(fake, fake, n, batch, *([fake] * 8)) == INVALID, (n, batch)
    # ctx, numerators, denominators, n, out_sum, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims
    good = [fake, fake, fake, 3] + [fake] * 8
    for at in (0, 1, 2, 4, 5, 6, 7, 8):
        args = list(good)
        args[at] = None
        assert lib.gkr_fraction_sum(*args) == INVALID, at
    for bad in (2, 0, -1, 30, 31):                                 # (n = 30: 2^31 values in the pair)
        assert lib.gkr_fraction_sum(fake, fake, fake, bad, *([fake] * 8)) == INVALID, bad
    # ctx, tables, n, batch, sums, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check, out_sums
    good = [fake, fake, 3, 1] + [fake] * 11
    for at in (0, 1, 5, 6, 7, 8, 9, 10):                           # (4 and 11 .. 14 may be NULL)
        args = list(good)
        args[at] = None
        assert lib.gkr_fraction_sum_verify_batch_device(*args) == INVALID, at
    for n, batch in shapes:
        assert lib.gkr_fraction_sum_verify_batch_device(fake, fake, n, batch, *([fake] * 11)) == INVALID, (n, batch)
    # ctx, numerators, denominators, n, sum, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check
    good = [fake, fake, fake, 3] + [fake] * 10
    for at in (0, 1, 2, 5, 6, 7, 8, 9, 10):
        args = list(good)
        args[at] = None
        assert lib.gkr_fraction_sum_verify(*args) == INVALID, at
    for bad in (2, 0, -1, 30, 31):
        assert lib.gkr_fraction_sum_verify(fake, fake, fake, bad, *([fake] * 10)) == INVALID, bad
    # ctx, tables, n, batch, d_layers
    for args in ([None, fake, 3, 1, fake], [fake, None, 3, 1, fake], [fake, fake, 3, 1, None]) + tuple([fake, fake, n, batch, fake] for n, batch in shapes):
        assert lib.gkr_devtest_fraction_sum_tree(*args) == INVALID, args[2:4]
    # ctx, n, batch, out
    for args in ([None, 3, 1, fake], [fake, 3, 1, None]) + tuple([fake, n, batch, fake] for n, batch in shapes):
        assert lib.gkr_devtest_fraction_sum_chunk(*args) == INVALID, args[1:3]
    # n, blocks
    for args in ((2, fake), (31, fake), (0, fake), (-1, fake), (3, None)):
        assert lib.gkr_selftest_fraction_sum_geometry(*args) == INVALID, args[0]
    assert not any(word)                                           # nothing was written


def tree_geometry(n):
    """gkr_selftest_fraction_sum_geometry -> the blocks per pair of the launch of level k, k = 0 .. n - 1."""
    out = np.full(n + 1, 0xDEAD, dtype=np.uint32)
    assert N.lib().gkr_selftest_fraction_sum_geometry(n, out.ctypes.data) == N.GKR_OK
    assert out[n] == 0xDEAD                                       # n words, no more
    return [int(x) for x in out[:n]]


def test_the_trees_launch_geometry():
    """One launch per level with a thread per node in blocks of 256: level 8 is the last with one block per pair, so n = 10 is the
    first size whose top launch has two."""
    for n in range(3, 31):
        assert tree_geometry(n) == [max(1, (1 << k) // 256) for k in range(n)], n
    assert tree_geometry(9) == [1] * 9 and tree_geometry(10) == [1] * 9 + [2] and tree_geometry(17)[-1] == 256


@pytest.fixture(scope="module")
def proofs():
    """{(n, kind): (N, D, proof)} of the model, made once."""
    rng = random.Random(20261029)
    out = {}
    for n in SIZES:
        for kind in KINDS:
            num, den = make_tables(kind, n, rng)
            out[(n, kind)] = (num, den, fraction_sum(num, den, n))
    return out


def test_the_model_closes_the_chain(proofs):
    """(P, Q) is the plain sum of fractions over the common denominator, on integers; every layer's claim cp_k + lambda_k cq_k is
    its zero-check's sum, added up entry by entry on the level below at z^(k); the end claims are N~(z^(n)) and D~(z^(n)); the
    numpy form of the model gives the same proof."""
    for (n, kind), (num, den, g) in proofs.items():
        all_d, plain = 1, 0
        for d in den:
            all_d *= d
        for i, x in enumerate(num):
            others = 1
            for j, d in enumerate(den):
                if j != i:
                    others = others * d % P
            plain += x * others                                    # sum_i N[i] prod_{j != i} D[j]
        Pm, Qm = g["sums"]
        assert Pm == plain % P and Qm == all_d % P, (n, kind)
        assert (Pm * all_d - Qm * plain) % P == 0
        assert g["head"] == fraction_tree(num, den, n)[2][0] + fraction_tree(num, den, n)[2][1] and len(g["layers"]) == n - 2
        assert head_root(g["head"]) == g["sums"]
        for k in range(2, n):
            (p, q), h = g["levels"][k + 1], 1 << k
            cp, cq = g["claims"][k - 2]
            lam = g["lambdas"][k - 2]
            assert (cp + lam * cq) % P == zerocheck_claim([p[:h], p[h:], q[:h], q[h:]], layer_terms(lam), g["points"][k - 2]), (n, kind, k)
            assert cp == mle(g["levels"][k][0], g["points"][k - 2]) and cq == mle(g["levels"][k][1], g["points"][k - 2])
            proof, r, _ = g["layers"][k - 2]
            assert len(proof) == k == len(r) and len(g["points"][k - 2]) == k
            assert g["points"][k - 1][1:] == r
        assert len(g["point"]) == n and g["claim"] == (mle(num, g["point"]), mle(den, g["point"])), (n, kind)
        assert sum(len(lay[0]) for lay in g["layers"]) == rounds(n) and layer_row(n) == rounds(n)
        if n <= 4:
            an, ad = np.array(num, dtype=object), np.array(den, dtype=object)
            gn = fraction_sum(an, ad, n, use_np=True)
            assert [int(x) for x in fraction_tree_np(an, ad, n)[0][0]] == [Pm] and mle_np(an, g["point"]) == g["claim"][0]
            assert (gn["sums"], gn["head"], gn["layers"], gn["point"], gn["claim"]) == (g["sums"], g["head"], g["layers"], g["point"], g["claim"])


def test_the_kinds_of_the_model(proofs):
    """A real lookup sums to zero over non-zero denominators; zero numerators give P = 0 at every level; one zero denominator
    gives Q = 0 (the prover's proof is still exact: the relations hold); equal entries make every level constant, so the round
    vectors are short."""
    for n in SIZES:
        num, den, g = proofs[(n, "lookup")]
        assert g["sums"][0] == 0 and g["sums"][1] != 0 and all(den) and num[:1 << (n - 1)] == [1] * (1 << (n - 1))
        assert sum((-x) % P for x in num[1 << (n - 1):]) == 1 << (n - 1)               # the multiplicities add up to the witness count
        num, den, g = proofs[(n, "zero_numerators")]
        assert g["sums"][0] == 0 and g["sums"][1] != 0 and all(not any(p) for p, _ in g["levels"])
        num, den, g = proofs[(n, "one_zero_denominator")]
        assert g["sums"][1] == 0 and den.count(0) == 1
        num, den, g = proofs[(n, "all_max")]
        assert set(num) == {P - 1} == set(den) and all(len(vec) < 4 for proof, _, _ in g["layers"] for vec in proof)


def test_the_verifiers_accept_the_models_proofs(proofs):
    for (n, kind), (num, den, g) in proofs.items():
        want = (ZERO_DENOMINATOR, 0, 0) if kind == "one_zero_denominator" else ACCEPTED
        for tables in ((num, den), (None, None)):
            for sums in (g["sums"], None):
                assert verify_fraction_sum(g["head"], g["layers"], tables[0], tables[1], sums) == want, (n, kind)
                assert model_verdict(g["head"], g["layers"], tables[0], tables[1], sums) == want, (n, kind)
        assert layers_of(proof_arrays(g, n), n) == g["layers"]


@pytest.mark.parametrize("n", (3, 4, 5))
def test_every_single_element_change_gets_its_closed_form_verdict(proofs, n):
    """Head entries, each claimed sum, every used slot, every length (to 0 and to 5), every challenge, each of the four values of
    every layer, one entry of N and one of D, each also with a value >= r, one at a time, with and without claimed sums and
    tables: the verdict is the one tests/fraction_sum_sweeps.py works out in closed form, from gkr_amd.verifier.verify_fraction_sum
    and from the model's verifier.  The inputs are asserted to have no zero cofactor first."""
    num, den, g = proofs[(n, "random")]
    check_inputs(g, n, num, den)
    arrays = proof_arrays(g, n)
    seen = set()
    for with_sums, with_tables in CONFIGS:
        for name, what, want in tamperings(g, n, with_sums, with_tables):
            arr, tn, td, sums = apply(what, arrays, num if with_tables else None, den if with_tables else None, g["sums"] if with_sums else None)
            layers = layers_of(arr, n)
            assert verify_fraction_sum(arr[0], layers, tn, td, sums) == want, (n, name, with_sums, with_tables)
            assert model_verdict(arr[0], layers, tn, td, sums) == want, (n, name, with_sums, with_tables)
            seen.add(want[0])
    assert seen >= {0, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, FRACTION_SUM}


def test_unused_slots_are_never_read_and_the_order_of_the_form_checks(proofs):
    """all_max has rows shorter than four slots: whatever an unused slot holds, the proof is accepted (the sweep's rule, on the
    kind that has such slots).  SHAPE comes before NON_CANONICAL, the head before the layers, a lower layer before a higher one,
    NON_CANONICAL before ZERO_DENOMINATOR before FRACTION_SUM before the layers' relations."""
    n = 5
    num, den, g = proofs[(n, "all_max")]
    arrays = proof_arrays(g, n)
    unused = [(name, what, want) for name, what, want in tamperings(g, n, True, True) if "unused" in name]
    assert len(unused) == 2 * rounds(n) and all(want == ACCEPTED for _, _, want in unused)
    for name, what, want in unused:
        arr, tn, td, sums = apply(what, arrays, num, den, g["sums"])
        assert arr[1] != arrays[1] and verify_fraction_sum(arr[0], layers_of(arr, n), tn, td, sums) == want == model_verdict(arr[0], layers_of(arr, n), tn, td, sums)

    num, den, g = proofs[(n, "random")]
    head, C, L, R, E = proof_arrays(g, n)

    def verdict(arr, sums=g["sums"]):
        layers = layers_of(arr, n)
        got = verify_fraction_sum(arr[0], layers, num, den, sums)
        assert got == model_verdict(arr[0], layers, num, den, sums)
        return got

    bad = [list(e) for e in E]
    bad[0][0] = P
    assert verdict((head, C, L[:-1] + [5], R, bad)) == (SHAPE, n - 1, n - 2)
    assert verdict((head, C, L, R[:-1] + [P], bad)) == (NON_CANONICAL, 2, 2)
    assert verdict(([P] + head[1:], C, L, R, bad)) == (NON_CANONICAL, 0, 0)
    wrong = ((g["sums"][0] + 1) % P, g["sums"][1])
    assert verdict((head, C, L, R[:-1] + [P], E), sums=wrong) == (NON_CANONICAL, n - 1, n - 2)
    assert verdict((head, C, L, [(R[0] + 1) % P] + R[1:], E), sums=wrong) == (FRACTION_SUM, 0, 0)
    zero_q = head[:4] + [0] + head[5:]                              # Q = 0: before the claimed sums and before the layers
    assert verdict((zero_q, C, L, R, E), sums=wrong) == (ZERO_DENOMINATOR, 0, 0) == verdict((zero_q, C, L, R, E), sums=None)
    assert verdict((zero_q, C, L, R[:-1] + [P], E)) == (NON_CANONICAL, n - 1, n - 2)


def test_a_proof_of_another_pair_fails_the_evaluation(proofs):
    for n in SIZES:
        num, den, g = proofs[(n, "random")]
        other_n, other_d, _ = proofs[(n, "lookup")]
        assert verify_fraction_sum(g["head"], g["layers"], other_n, den, g["sums"]) == (EVALUATION, n, n)
        assert verify_fraction_sum(g["head"], g["layers"], num, other_d, g["sums"]) == (EVALUATION, n, n)


def _hex(values):
    return " ".join("%064x" % v for v in values)


def _write_case(f, n, arrays, num, den, sums, given, want, honest=None):
    head, C, L, R, E = arrays
    rows = [[P if (1 <= ln <= 4 and t < 4 - ln and v == 0) else v for t, v in enumerate(row)] for row, ln in zip(C, L)]   # unused slots: r, never read
    f.write("case %d %d %d %d %d %d\n" % ((n, 1 if given else 0, 1 if honest else 0) + tuple(want)))
    f.write("\n".join([_hex(sums), _hex(head), _hex(x for row in rows for x in row), " ".join(str(v) for v in L), _hex(R),
                       _hex(x for e in E for x in e), _hex(num), _hex(den)]) + "\n")
    if honest:
        f.write(_hex(list(honest["sums"]) + honest["point"] + list(honest["claim"])) + "\n")


def test_the_chain_of_claims_stands_alone_under_address_and_ub_sanitizers(proofs, tmp_path):
    """tests/fraction_sum_rounds_selfcheck.cpp with csrc/fraction_sum_rounds.h (and csrc/keccak.cpp for the hash constants) on the
    model's proofs of every kind at n = 3 .. 6 and on the whole sweep at n = 3, 4, 5, written out here: the relations the device
    verifier runs on its host threads, driven without a device; every verdict the model's rule, no sanitizer report.  A child
    process: nothing is loaded into this one.  (make -C gkr_amd/csrc asan_fs builds the same program.)"""
    cases = str(tmp_path / "cases.txt")
    with open(cases, "w") as f:
        for (n, kind), (num, den, g) in proofs.items():
            want = (ZERO_DENOMINATOR, 0, 0) if kind == "one_zero_denominator" else ACCEPTED
            for given in (True, False):
                _write_case(f, n, proof_arrays(g, n), num, den, g["sums"], given, want, honest=g)
        for n in (3, 4, 5):
            num, den, g = proofs[(n, "random")]
            arrays = proof_arrays(g, n)
            for with_sums in (True, False):
                for name, what, want in tamperings(g, n, with_sums, True):
                    arr, tn, td, sums = apply(what, arrays, num, den, g["sums"])
                    _write_case(f, n, arr, tn, td, sums, with_sums, want)
    exe = str(tmp_path / "fraction_sum_rounds_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                            os.path.join(REPO, "tests", "fraction_sum_rounds_selfcheck.cpp"), os.path.join(REPO, "gkr_amd", "csrc", "keccak.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr[-3000:]
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "fraction_sum_rounds_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

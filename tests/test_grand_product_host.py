"""The grand product argument (include/gkr_amd.h, gkr_grand_product*) as far as no device is needed: the symbols, the argument
checks that return before a device is touched, the tree's launch geometry (host logic), the integer model
(tests/grand_product_model.py, written from the protocol on zerocheck_model and oracle.mimc7) held to the plain product, to every
layer's claim summed entry by entry and to V~(z^(n)); gkr_amd.verifier.verify_grand_product on the model's proofs and on every
single-element change of them, against the closed-form verdicts of tests/grand_product_sweeps.py; and the chain of claims
(csrc/grand_product_rounds.h) in a stand-alone program under AddressSanitizer and UBSan (a child process: no sanitizer goes near
code loaded into python)."""

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
from gkr_amd.verifier import verify_grand_product
from grand_product_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, KINDS, NON_CANONICAL, PRODUCT, ROUND_SUM, SHAPE, TERMS, grand_product, layer_row,
                                 make_table, mle, model_verdict, product_tree, product_tree_np, proof_arrays, rounds)
from grand_product_sweeps import apply, layers_of, tamperings
from oracle.field import P
from zerocheck_model import zerocheck_claim

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_grand_product_batch_device", "gkr_grand_product", "gkr_grand_product_verify_batch_device", "gkr_grand_product_verify",
         "gkr_selftest_grand_product_geometry", "gkr_devtest_grand_product_tree", "gkr_devtest_grand_product_chunk"]
SIZES = (3, 4, 5, 6)


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("grand_product_batch_device", "prove_grand_product", "verify_grand_product_batch_device", "verify_grand_product"):
        assert callable(getattr(Context, name)), name
    assert callable(gkr_amd.prove_grand_product) and callable(gkr_amd.verify_grand_product)
    assert "prove_grand_product" in gkr_amd.__all__ and "verify_grand_product" in gkr_amd.__all__
    assert re.search(r"GKR_VERIFY_PRODUCT = 13\b", header) and N.GKR_VERIFY_PRODUCT == 13 == PRODUCT
    assert (N.GKR_VERIFY_SHAPE, N.GKR_VERIFY_NON_CANONICAL, N.GKR_VERIFY_ROUND_SUM, N.GKR_VERIFY_CHALLENGE, N.GKR_VERIFY_FINAL_CLAIM,
            N.GKR_VERIFY_EVALUATION) == (SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION)


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    shapes = ((2, 2), (2, 0), (2, -1), (2, 31), (3, 0), (3, -1), (3, 65536))
    # ctx, tables, n, batch, out_products, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claim
    good = [fake, fake, 3, 1] + [fake] * 8
    for at in (0, 1, 4, 5, 6, 7, 8):                               # (9 .. 11, the optional outputs, may be NULL)
        args = list(good)
        args[at] = None
        assert lib.gkr_grand_product_batch_device(*args) == INVALID, at
    for at, bad in shapes + ((2, 30), (3, 2048)):                  # (n = 30 with batch 1 is the limit: refused with batch 2 below)
        args = list(good)
        args[at] = bad
        if (at, bad) == (2, 30):
            args[3] = 2                                            # batch * 2^n = 2^31
        if (at, bad) == (3, 2048):
            args[2] = 20                                           # 2048 * 2^20 = 2^31
        assert lib.gkr_grand_product_batch_device(*args) == INVALID, (at, bad)
    # ctx, table, n, out_product, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claim
    good = [fake, fake, 3] + [fake] * 8
    for at in (0, 1, 3, 4, 5, 6, 7):
        args = list(good)
        args[at] = None
        assert lib.gkr_grand_product(*args) == INVALID, at
    for bad in (2, 0, -1, 31):
        assert lib.gkr_grand_product(fake, fake, bad, *([fake] * 8)) == INVALID, bad
    # ctx, tables, n, batch, products, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check, out_products
    good = [fake, fake, 3, 1] + [fake] * 11
    for at in (0, 1, 5, 6, 7, 8, 9, 10):                           # (4 and 11 .. 14 may be NULL)
        args = list(good)
        args[at] = None
        assert lib.gkr_grand_product_verify_batch_device(*args) == INVALID, at
    for at, bad in shapes:
        args = list(good)
        args[at] = bad
        assert lib.gkr_grand_product_verify_batch_device(*args) == INVALID, (at, bad)
    # ctx, table, n, product, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check
    good = [fake, fake, 3] + [fake] * 10
    for at in (0, 1, 4, 5, 6, 7, 8, 9):
        args = list(good)
        args[at] = None
        assert lib.gkr_grand_product_verify(*args) == INVALID, at
    for bad in (2, 0, -1, 31):
        assert lib.gkr_grand_product_verify(fake, fake, bad, *([fake] * 10)) == INVALID, bad
    # ctx, tables, n, batch, d_layers
    for args in ([None, fake, 3, 1, fake], [fake, None, 3, 1, fake], [fake, fake, 3, 1, None], [fake, fake, 2, 1, fake], [fake, fake, 3, 0, fake],
                 [fake, fake, 31, 1, fake], [fake, fake, 3, 65536, fake]):
        assert lib.gkr_devtest_grand_product_tree(*args) == INVALID, args[2:4]
    # ctx, n, batch, out: the verifier's shapes
    for args in ([None, 3, 1, fake], [fake, 3, 1, None]) + tuple([fake, n, batch, fake] for n, batch in
                                                              ((2, 1), (0, 1), (-1, 1), (31, 1), (3, 0), (3, -1), (3, 65536), (30, 2), (20, 2048))):
        assert lib.gkr_devtest_grand_product_chunk(*args) == INVALID, args[1:3]
    assert word[0] == 0                                            # nothing was written


def tree_geometry(n):
    """gkr_selftest_grand_product_geometry -> the blocks per table of the launch of level k, k = 0 .. n - 1."""
    out = np.full(n + 1, 0xDEAD, dtype=np.uint32)
    assert N.lib().gkr_selftest_grand_product_geometry(n, out.ctypes.data) == N.GKR_OK
    assert out[n] == 0xDEAD                                       # n words, no more
    return [int(x) for x in out[:n]]


def test_the_trees_launch_geometry():
    """One launch per level with a thread per product in blocks of 256; the thresholds the GPU tests run at are where this says
    they are: level 8 is the last with one block per table, so n = 10 is the first table whose top launch has two."""
    lib = N.lib()
    out = np.zeros(40, dtype=np.uint32)
    for n in range(3, 31):
        assert tree_geometry(n) == [max(1, (1 << k) // 256) for k in range(n)], n
    assert tree_geometry(9) == [1] * 9 and tree_geometry(10) == [1] * 9 + [2] and tree_geometry(20)[-1] == 2048
    for args in ((2, out.ctypes.data), (31, out.ctypes.data), (0, out.ctypes.data), (-1, out.ctypes.data), (3, None)):
        assert lib.gkr_selftest_grand_product_geometry(*args) == N.GKR_ERR_INVALID, args[0]


@pytest.fixture(scope="module")
def proofs():
    """{(n, kind): (table, proof)} of the model, made once."""
    rng = random.Random(20261021)
    out = {}
    for n in SIZES:
        for kind in KINDS:
            table = make_table(kind, n, rng)
            out[(n, kind)] = (table, grand_product(table, n))
    return out


def test_the_model_closes_the_chain(proofs):
    """P is the plain product; every layer's claim c_k is its zero-check's sum, added up entry by entry on the level below at
    z^(k); the last claim is V~(z^(n)); the numpy form of the model gives the same proof."""
    for (n, kind), (table, g) in proofs.items():
        plain = 1
        for v in table:
            plain = plain * v % P
        assert g["product"] == plain, (n, kind)
        assert g["head"] == product_tree(table, n)[2] and len(g["layers"]) == n - 2
        assert (g["head"][0] * g["head"][1] * g["head"][2] * g["head"][3] - plain) % P == 0
        for k in range(2, n):
            up, h = g["levels"][k + 1], 1 << k
            assert g["claims"][k - 2] == zerocheck_claim([up[:h], up[h:]], TERMS, g["points"][k - 2]), (n, kind, k)
            proof, r, _ = g["layers"][k - 2]
            assert len(proof) == k == len(r) and len(g["points"][k - 2]) == k
            assert g["points"][k - 1][1:] == r
        assert len(g["point"]) == n and g["claim"] == mle(table, g["point"]), (n, kind)
        assert sum(len(lay[0]) for lay in g["layers"]) == rounds(n) and layer_row(n) == rounds(n)
        if n <= 4:
            gn = grand_product(np.array(table, dtype=object), n, use_np=True)
            assert [int(x) for x in product_tree_np(np.array(table, dtype=object), n)[0]] == [plain]
            assert (gn["product"], gn["head"], gn["layers"], gn["point"], gn["claim"]) == (g["product"], g["head"], g["layers"], g["point"], g["claim"])


def test_the_zero_tables_of_the_model(proofs):
    """One zero entry: P = 0, a zero in every level on its path, the layers' vectors not all [0].  The whole upper half zero: every
    level below the table is zero, g vanishes identically in EVERY layer, the last included -- every vector [0] with length 1 (the
    zero-check's own rule), a_k = b_k = 0 below the last layer and b_{n-1} = 0."""
    for n in SIZES:
        table, g = proofs[(n, "one_zero")]
        assert g["product"] == 0 and g["head"].count(0) == 1 and all(lvl.count(0) == 1 for lvl in g["levels"])
        assert any(vec != [0] for proof, _, _ in g["layers"] for vec in proof)
        table, g = proofs[(n, "upper_zero")]
        assert g["product"] == 0 and g["head"] == [0] * 4 and all(set(lvl) == {0} for lvl in g["levels"][:n])
        assert all(vec == [0] for proof, _, _ in g["layers"] for vec in proof)
        assert all(ab == (0, 0) for _, _, ab in g["layers"][:-1]) and g["layers"][-1][2][1] == 0 and g["layers"][-1][2][0] != 0
        assert g["claims"][:-1] == [0] * (n - 2)
        table, g = proofs[(n, "all_max")]
        assert g["product"] == 1 and g["head"] == [1, 1, 1, 1] and set(table) == {P - 1}          # (-1)^(2^n) with n >= 3


def test_the_verifiers_accept_the_models_proofs(proofs):
    for (n, kind), (table, g) in proofs.items():
        for tb in (table, None):
            for product in (g["product"], None):
                assert verify_grand_product(g["head"], g["layers"], tb, product) == (0, 0, 0), (n, kind)
                assert model_verdict(g["head"], g["layers"], tb, product) == (0, 0, 0), (n, kind)
        assert layers_of(proof_arrays(g, n), n) == g["layers"]


@pytest.mark.parametrize("n", (3, 4, 5))
def test_every_single_element_change_gets_its_closed_form_verdict(proofs, n):
    """Head entries, every used slot, every length (+ 1 and - 1), every challenge, every value, the claimed product and every table
    entry, one at a time, on every kind of table, with and without a claimed product and a table: the verdict is the one
    tests/grand_product_sweeps.py works out in closed form, from gkr_amd.verifier.verify_grand_product and from the model's verifier."""
    seen = set()
    for kind in KINDS:
        table, g = proofs[(n, kind)]
        arrays = proof_arrays(g, n)
        for with_product, with_table in ((True, True), (False, True), (True, False)):
            for name, what, want in tamperings(g, n, with_product, with_table):
                arr, tb, product = apply(what, arrays, table if with_table else None, g["product"] if with_product else None)
                layers = layers_of(arr, n)
                assert verify_grand_product(arr[0], layers, tb, product) == want, (n, kind, name, with_product, with_table)
                assert model_verdict(arr[0], layers, tb, product) == want, (n, kind, name, with_product, with_table)
                seen.add(want[0])
    assert seen >= {0, SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, PRODUCT}


def test_elements_outside_the_field_are_non_canonical_in_the_order_of_the_header(proofs):
    n = 5
    table, g = proofs[(n, "random")]
    arrays = proof_arrays(g, n)

    def verdict(arr, product=g["product"]):
        layers = layers_of(arr, n)
        got = verify_grand_product(arr[0], layers, table, product)
        assert got == model_verdict(arr[0], layers, table, product)
        return got

    head, C, L, R, E = arrays
    assert verdict((head[:2] + [P] + head[3:], C, L, R, E)) == (NON_CANONICAL, 0, 0)
    assert verdict(arrays, product=P) == (NON_CANONICAL, 0, 0)
    for k in range(2, n):
        for j in range(k):
            row = layer_row(k) + j
            bad = [list(c) for c in C]
            bad[row][3] = P + 1
            assert verdict((head, bad, L, R, E)) == (NON_CANONICAL, k, j)
            assert verdict((head, C, L, R[:row] + [P] + R[row + 1:], E)) == (NON_CANONICAL, k, j)
            if L[row] < 4:                                         # an unused slot is never read
                bad = [list(c) for c in C]
                bad[row][0] = P
                assert verdict((head, bad, L, R, E)) == (0, 0, 0)
        for w in range(2):
            bad = [list(e) for e in E]
            bad[k - 2][w] = P
            assert verdict((head, C, L, R, bad)) == (NON_CANONICAL, k, k)
    # SHAPE comes before NON_CANONICAL, a lower layer's element before a higher layer's, the head before both
    bad = [list(e) for e in E]
    bad[0][0] = P
    assert verdict((head, C, L[:-1] + [5], R, bad)) == (SHAPE, n - 1, n - 2)
    assert verdict((head, C, L, R[:-1] + [P], bad)) == (NON_CANONICAL, 2, 2)
    assert verdict(([P] + head[1:], C, L, R, bad)) == (NON_CANONICAL, 0, 0)
    # ... and PRODUCT behind NON_CANONICAL, before the layers
    assert verdict((head, C, L, R[:-1] + [P], E), product=(g["product"] + 1) % P) == (NON_CANONICAL, n - 1, n - 2)
    assert verdict((head, C, L, [(R[0] + 1) % P] + R[1:], E), product=(g["product"] + 1) % P) == (PRODUCT, 0, 0)


def test_a_proof_of_another_table_fails_the_evaluation(proofs):
    for n in SIZES:
        table, g = proofs[(n, "random")]
        other, _ = proofs[(n, "one_zero")]
        assert verify_grand_product(g["head"], g["layers"], other, g["product"]) == (EVALUATION, n, n)


def test_the_chain_of_claims_stands_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/grand_product_rounds_selfcheck.cpp with csrc/grand_product_rounds.h (and csrc/keccak.cpp for the hash constants): the
    relations the device verifier runs on its host threads, driven without a device; no sanitizer report.  A child process: nothing is
    loaded into this one.  (make -C gkr_amd/csrc asan_gp builds the same program.)"""
    exe = str(tmp_path / "grand_product_rounds_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                            os.path.join(REPO, "tests", "grand_product_rounds_selfcheck.cpp"), os.path.join(REPO, "gkr_amd", "csrc", "keccak.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "grand_product_rounds_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

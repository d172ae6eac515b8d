"""ogkr_grand_product (oracle/c/ogkr.c; cdense.grand_product_raw), the C twin of tests/grand_product_model.py that
tests/test_gpu_grand_product_sizes.py compares gkr_grand_product_batch_device with at sizes the Python model cannot reach.  It is
written from the protocol on the oracle's own pieces -- a loop of ogkr_fr_mul per level, ogkr_multi_hash, and the EXPLICIT
zero-check ogkr_sumcheck_zerocheck per layer -- and shares nothing with gkr_amd/csrc.  What holds it:

  a. grand_product_model.grand_product for n = 3 .. 8 over all KINDS of table: every array, and every level of the tree;
  b. at n = 16, where only the C side is fast: grand_product_model.model_verdict and gkr_amd.verifier.verify_grand_product accept a
     proof the oracle made alone (with the table and a claimed product), and give the closed-form verdict of
     tests/grand_product_sweeps.py for one change of every kind of element; the product is the plain product;
  c. the same bytes under 1, 3 and all usable threads;
  d. bad shapes are -1;
  e. a stand-alone program (oracle/c/grand_product_selfcheck.c) built with the C file under ASan + UBSan, run as a child process."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from gkr_amd.verifier import verify_grand_product
from grand_product_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, KINDS, PRODUCT, ROUND_SUM, SHAPE, grand_product, make_table, model_verdict,
                                 proof_arrays, rounds)
from grand_product_oracle import as_model, limb_table, pick, zero_index
from grand_product_sweeps import apply, layers_of, tamperings
from oracle import cdense
from oracle.field import P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. the model, every array ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(3, 9))
def test_every_array_equals_the_model(n):
    short = full = 0
    for ki, kind in enumerate(KINDS):
        table = make_table(kind, n, random.Random(15000 + 10 * n + ki))
        g = grand_product(table, n)
        head, C, L, R, E = proof_arrays(g, n)
        Pl, H, Cl, Ll, Rl, El, Zl, Kl, levels = cdense.grand_product_raw(cdense.to_limbs(table), n, levels=True)
        what = (n, kind)
        assert Cl.shape == (rounds(n), 4, 4) and Ll.dtype == np.uint32 and levels.shape == ((1 << n) - 1, 4), what
        assert cdense.from_limbs(Pl) == [g["product"]] and cdense.from_limbs(H) == head, what
        assert [cdense.from_limbs(row) for row in Cl] == C and [int(x) for x in Ll] == L and cdense.from_limbs(Rl) == R, what
        assert cdense.from_limbs(El) == [x for e in E for x in e], what
        assert cdense.from_limbs(Zl) == g["point"] and cdense.from_limbs(Kl) == [g["claim"]], what
        for k in range(n):
            assert cdense.from_limbs(levels[(1 << k) - 1:(2 << k) - 1]) == g["levels"][k], (what, k)
        got = as_model((Pl, H, Cl, Ll, Rl, El, Zl, Kl), n)
        assert all(got[key] == g[key] for key in ("product", "head", "layers", "points", "claims", "eqs", "point", "claim")), what
        without = cdense.grand_product_raw(cdense.to_limbs(table), n)
        assert len(without) == 8 and all(np.array_equal(a, b) for a, b in zip(without, (Pl, H, Cl, Ll, Rl, El, Zl, Kl))), what
        short += any(v < 4 for v in L)
        full += all(v == 4 for v in L)
    assert short and full                                          # the length rule was in play, and not everywhere


# ---- b. a size only the C side reaches ------------------------------------------------------------------------------------------------------
N_LARGE = 16


@pytest.fixture(scope="module")
def large():
    """{kind: (table as integers, limbs, raw oracle arrays, the proof as the model's dict)} at n = 16."""
    out = {}
    for kind, seed in (("random", 1616), ("one_zero", 1617)):
        T = limb_table(kind, N_LARGE, seed)
        raw = cdense.grand_product_raw(T, N_LARGE)
        out[kind] = (cdense.from_limbs(T), T, raw, as_model(raw, N_LARGE))
    return out


def test_the_verifiers_accept_a_proof_the_oracle_made_alone(large):
    n = N_LARGE
    for kind, (table, T, raw, g) in large.items():
        plain = 1
        for v in table:
            plain = plain * v % P
        assert g["product"] == plain and (kind == "random") == (plain != 0), kind
        assert table.count(0) == (kind == "one_zero") and (kind == "random" or table[zero_index(n)] == 0)
        assert len(g["layers"]) == n - 2 and sum(len(lay[0]) for lay in g["layers"]) == rounds(n) == 119
        assert model_verdict(g["head"], g["layers"], table, g["product"]) == (0, 0, 0), kind
        assert verify_grand_product(g["head"], g["layers"], table, g["product"]) == (0, 0, 0), kind
        assert model_verdict(g["head"], g["layers"]) == (0, 0, 0) == verify_grand_product(g["head"], g["layers"]), kind


def test_one_change_of_every_kind_of_element_gets_its_closed_form_verdict(large):
    n = N_LARGE
    seen = set()
    for kind, (table, T, raw, g) in large.items():
        arrays = proof_arrays(g, n)
        sweep = tamperings(g, n, True, True)
        k, j = 9, 4
        last = len(g["layers"][k - 2][0][j]) - 1                  # the sweep counts a round's used slots: 0 the leading one, `last` the constant
        cases = pick(sweep, "head 1", "layer %d round %d slot 0" % (k, j), "layer %d round %d slot %d" % (k, j, last),
                     "layer %d challenge %d" % (k, j), "layer %d length %d + 1" % (k, j), "layer %d length %d - 1" % (k, j),
                     "layer %d value 0" % k, "layer %d value 1" % (n - 1), "claimed product", "table entry 0", "table entry %d" % zero_index(n))
        for name, what, want in cases:
            arr, tb, product = apply(what, arrays, table, g["product"])
            layers = layers_of(arr, n)
            assert model_verdict(arr[0], layers, tb, product) == want, (kind, name)
            assert verify_grand_product(arr[0], layers, tb, product) == want, (kind, name)
            seen.add(want[0])
        # a head entry without a claimed product moves z^(2) instead
        name, what, want = pick(tamperings(g, n, False, False), "head 2")[0]
        arr, _, _ = apply(what, arrays, None, None)
        assert want == (ROUND_SUM, 2, 0) == model_verdict(arr[0], layers_of(arr, n)) == verify_grand_product(arr[0], layers_of(arr, n)), kind
    assert seen == {SHAPE, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, PRODUCT}, seen


# ---- c. threads -----------------------------------------------------------------------------------------------------------------------------
def test_the_results_do_not_depend_on_the_thread_count(large):
    for kind, (_, T, raw, _) in large.items():
        want = cdense.grand_product_raw(T, N_LARGE, levels=True)
        assert all(np.array_equal(a, b) for a, b in zip(want, raw)), kind
        for threads in (1, 3, cdense.usable_threads()):
            got = cdense.grand_product_raw(T, N_LARGE, threads=threads, levels=True)
            assert len(got) == 9 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (kind, threads)


# ---- d. bad shapes --------------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_are_minus_one():
    T = cdense.fill_table(1 << 6, 3)
    cdense.grand_product_raw(T[:8], 3)                             # (the good shapes next to them)
    cdense.grand_product_raw(T[:32], 5)
    for n in (2, 1, 0, -1, 31, 40):
        with pytest.raises(ValueError, match="rc=-1"):
            cdense.grand_product_raw(T[:4], n)
    for n, rows in ((5, 31), (5, 33), (4, 32), (3, 0)):
        with pytest.raises(ValueError, match="rc=-1"):
            cdense.grand_product_raw(T[:rows], n)
    fn = cdense.lib().ogkr_grand_product
    fn.restype = ctypes.c_int
    n = 3
    bufs = [np.zeros((16, 4), dtype=np.uint64) for _ in range(9)]
    good = [b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    table = T.ctypes.data_as(ctypes.c_void_p)
    assert fn(table, ctypes.c_int(n), *good[:8], None, ctypes.c_int(1)) == 0
    assert fn(table, ctypes.c_int(n), *good, ctypes.c_int(1)) == 0
    assert fn(None, ctypes.c_int(n), *good, ctypes.c_int(1)) == -1
    for at in range(8):                                            # (the ninth, the levels, may be NULL)
        args = list(good)
        args[at] = None
        assert fn(table, ctypes.c_int(n), *args, ctypes.c_int(1)) == -1, at
    for bad in (2, 31, 0, -1):
        assert fn(table, ctypes.c_int(bad), *good, ctypes.c_int(1)) == -1, bad


# ---- e. under the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """`make -C oracle/c grand_product_selfcheck`: n = 3 .. 10, three kinds of table, 1 and 4 threads and with and without the
    levels give equal bytes, the tree and the chain equal the ones the program builds itself, exact-size output buffers; no
    sanitizer report.  A child process: nothing is loaded into this one."""
    exe = str(tmp_path / "grand_product_selfcheck")
    build = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "c"), "grand_product_selfcheck", "OUT=" + exe], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "grand_product_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

"""ogkr_fraction_sum (oracle/c/ogkr.c; cdense.fraction_sum_raw), the C twin of tests/fraction_sum_model.py that
tests/test_gpu_fraction_sum_sizes.py and tests/test_gpu_lookup_sizes.py compare the device with at sizes the Python model cannot
reach.  It is written from the protocol on the oracle's own pieces -- a loop of ogkr_fr_mul / ogkr_fr_add per level,
ogkr_multi_hash, and the EXPLICIT zero-check ogkr_sumcheck_zerocheck per layer -- and shares nothing with gkr_amd/csrc.  What
holds it:

  a. fraction_sum_model.fraction_sum for n = 3 .. 8 over all KINDS of pair: every array, and every level of the tree;
  b. at n = 16, where only the C side is fast: fraction_sum_model.model_verdict and gkr_amd.verifier.verify_fraction_sum accept a
     proof the oracle made alone (with the pair and claimed sums, and without), and give the closed-form verdict of
     tests/fraction_sum_sweeps.py for one change of every kind of element; a lookup-shaped pair has P = 0 and Q the plain product;
  c. the same bytes under 1, 3 and all usable threads;
  d. bad shapes and NULLs are -1;
  e. a stand-alone program (oracle/c/fraction_sum_selfcheck.c, which covers the lookup functions too) built with the C file under
     ASan + UBSan, run as a child process."""

import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from gkr_amd.verifier import verify_fraction_sum
from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, FRACTION_SUM, KINDS, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR,
                                fraction_sum, make_tables, model_verdict, proof_arrays, rounds)
from fraction_sum_oracle import PAIR_KINDS, as_model, limb_pair, pick, zero_index
from fraction_sum_sweeps import ACCEPTED, apply, check_cofactors, check_inputs, layers_of, table_entries, tamperings
from oracle import cdense
from oracle.field import P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. the model, every array ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(3, 9))
def test_every_array_equals_the_model(n):
    short = full = 0
    for ki, kind in enumerate(KINDS):
        num, den = make_tables(kind, n, random.Random(16000 + 10 * n + ki))
        g = fraction_sum(num, den, n)
        head, C, L, R, E = proof_arrays(g, n)
        pair = cdense.to_limbs(num + den)
        S, H, Cl, Ll, Rl, El, Zl, Kl, levels = cdense.fraction_sum_raw(pair, n, levels=True)
        what = (n, kind)
        assert Cl.shape == (rounds(n), 4, 4) and Ll.dtype == np.uint32 and levels.shape == (2 * ((1 << n) - 1), 4), what
        assert tuple(cdense.from_limbs(S)) == g["sums"] and cdense.from_limbs(H) == head, what
        assert [cdense.from_limbs(row) for row in Cl] == C and [int(x) for x in Ll] == L and cdense.from_limbs(Rl) == R, what
        assert cdense.from_limbs(El) == [x for e in E for x in e], what
        assert cdense.from_limbs(Zl) == g["point"] and tuple(cdense.from_limbs(Kl)) == g["claim"], what
        for k in range(n):
            at = 2 * ((1 << k) - 1)
            assert cdense.from_limbs(levels[at:at + (2 << k)]) == [int(x) for x in g["levels"][k][0]] + [int(x) for x in g["levels"][k][1]], (what, k)
        got = as_model((S, H, Cl, Ll, Rl, El, Zl, Kl), n)
        assert all(got[key] == g[key] for key in ("sums", "head", "layers", "points", "lambdas", "claims", "eqs", "point", "claim")), what
        without = cdense.fraction_sum_raw(pair.reshape(2, 1 << n, 4), n)
        assert len(without) == 8 and all(np.array_equal(a, b) for a, b in zip(without, (S, H, Cl, Ll, Rl, El, Zl, Kl))), what
        short += any(v < 4 for v in L)
        full += all(v == 4 for v in L)
    assert short and full                                          # the length rule was in play, and not everywhere


# ---- b. a size only the C side reaches ------------------------------------------------------------------------------------------------------
N_LARGE = 16


@pytest.fixture(scope="module")
def large():
    """{kind: (N, D as integers, limbs, raw oracle arrays, the proof as the model's dict)} at n = 16."""
    out = {}
    for kind, seed in (("random", 1626), ("lookup", 1627), ("padded", 1628), ("one_zero_denominator", 1629), ("upper_zero", 1630)):
        T = limb_pair(kind, N_LARGE, seed)
        raw = cdense.fraction_sum_raw(T, N_LARGE)
        out[kind] = (cdense.from_limbs(T[0]), cdense.from_limbs(T[1]), T, raw, as_model(raw, N_LARGE))
    return out


def test_the_pair_kinds_are_what_their_names_say(large):
    n = N_LARGE
    assert PAIR_KINDS == KINDS + ["padded", "upper_zero"] and zero_index(n) >> 8 == (1 << (n - 8)) - 1 and 0 < zero_index(n) & 255 < 255
    num, den, _, _, g = large["one_zero_denominator"]
    assert den.count(0) == 1 and den[zero_index(n)] == 0 and g["sums"][1] == 0 and all(num)
    num, den, _, raw, g = large["upper_zero"]
    assert not any(num[1 << (n - 1):]) and not any(den[1 << (n - 1):]) and all(num[:1 << (n - 1)]) and all(den[:1 << (n - 1)])
    assert g["sums"] == (0, 0) and (raw[3] == 1).all() and not raw[2].any()      # every round vector is [0]
    for kind, n_w in (("lookup", n - 1), ("padded", n - 5)):
        num, den, _, _, g = large[kind]
        half = 1 << (n - 1)
        assert num[:1 << n_w] == [1] * (1 << n_w) and num[1 << n_w:half] == [0] * (half - (1 << n_w)) and den[1 << n_w:half] == [1] * (half - (1 << n_w))
        assert sum((P - x) % P for x in num[half:]) == 1 << n_w and all(den)
        plain = 1
        for v in den:
            plain = plain * v % P
        assert g["sums"] == (0, plain) and plain != 0, kind            # the lookup holds: P = 0, and Q is the plain product
    assert 16 * (1 << (n - 5)) == 1 << (n - 1)                         # padded: fifteen sixteenths of the witness half is (0, 1)


def test_the_verifiers_accept_a_proof_the_oracle_made_alone(large):
    n = N_LARGE
    for kind, (num, den, T, raw, g) in large.items():
        want = (ZERO_DENOMINATOR, 0, 0) if kind in ("one_zero_denominator", "upper_zero") else ACCEPTED
        assert len(g["layers"]) == n - 2 and sum(len(lay[0]) for lay in g["layers"]) == rounds(n) == 119
        assert model_verdict(g["head"], g["layers"], num, den, g["sums"]) == want, kind
        assert verify_fraction_sum(g["head"], g["layers"], num, den, g["sums"]) == want, kind
        assert model_verdict(g["head"], g["layers"]) == want == verify_fraction_sum(g["head"], g["layers"]), kind


def test_one_change_of_every_kind_of_element_gets_its_closed_form_verdict(large):
    n = N_LARGE
    num, den, _, _, g = large["one_zero_denominator"]              # the one verdict no single change of a good proof gives
    seen = {model_verdict(g["head"], g["layers"], num, den, g["sums"])[0]}
    for kind in ("random", "lookup", "padded"):
        num, den, T, raw, g = large[kind]
        if kind == "random":
            check_inputs(g, n, num, den)
        else:
            check_cofactors(g, n)
        arrays = proof_arrays(g, n)
        sweep = tamperings(g, n, True, True, length_steps=True)
        k, j = 9, 4
        first = 4 - len(g["layers"][k - 2][0][j])
        i_num, i_den = table_entries(n)
        cases = pick(sweep, "head 1 + 1", "head 6 + 1", "head 2 >= r", "layer %d round %d slot %d + 1" % (k, j, first), "layer %d round %d slot 3 + 1" % (k, j),
                     "layer %d round %d slot 3 >= r" % (k, j), "layer %d challenge %d + 1" % (k, j), "layer %d length %d + 1" % (k, j),
                     "layer %d length %d - 1" % (k, j), "layer %d length %d -> 5" % (n - 1, 0), "layer %d value 0 + 1" % k, "layer %d value 1 + 1" % 2,
                     "layer %d value 2 + 1" % (n - 1), "layer %d value 3 + 1" % k, "claimed sum 0 + 1", "claimed sum 1 + 1",
                     "num entry %d + 1" % i_num, "den entry %d + 1" % i_den)
        for name, what, want in cases:
            arr, tn, td, sums = apply(what, arrays, num, den, g["sums"])
            layers = layers_of(arr, n)
            assert model_verdict(arr[0], layers, tn, td, sums) == want, (kind, name)
            assert verify_fraction_sum(arr[0], layers, tn, td, sums) == want, (kind, name)
            seen.add(want[0])
        # a head entry without claimed sums moves z^(2) instead
        name, what, want = pick(tamperings(g, n, False, False), "head 2 + 1")[0]
        arr, _, _, _ = apply(what, arrays, None, None, None)
        assert want == (ROUND_SUM, 2, 0) == model_verdict(arr[0], layers_of(arr, n)) == verify_fraction_sum(arr[0], layers_of(arr, n)), kind
    assert seen == {SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, ZERO_DENOMINATOR, FRACTION_SUM}, seen


# ---- c. threads -----------------------------------------------------------------------------------------------------------------------------
def test_the_results_do_not_depend_on_the_thread_count(large):
    for kind, (_, _, T, raw, _) in large.items():
        want = cdense.fraction_sum_raw(T, N_LARGE, levels=True)
        assert all(np.array_equal(a, b) for a, b in zip(want, raw)), kind
        for threads in (1, 3, cdense.usable_threads()):
            got = cdense.fraction_sum_raw(T, N_LARGE, threads=threads, levels=True)
            assert len(got) == 9 and all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), (kind, threads)


# ---- d. bad shapes --------------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_and_nulls_are_minus_one():
    T = cdense.fill_table(1 << 7, 3)
    cdense.fraction_sum_raw(T[:16], 3)                             # (the good shapes next to them)
    cdense.fraction_sum_raw(T[:64], 5)
    for n in (2, 1, 0, -1, 30, 40):
        with pytest.raises(ValueError, match="rc=-1"):
            cdense.fraction_sum_raw(T[:8], n)
    for n, rows in ((5, 63), (5, 65), (4, 64), (3, 0), (3, 8)):
        with pytest.raises(ValueError, match="rc=-1"):
            cdense.fraction_sum_raw(T[:rows], n)
    fn = cdense.lib().ogkr_fraction_sum
    fn.restype = ctypes.c_int
    n = 3
    bufs = [np.zeros((16, 4), dtype=np.uint64) for _ in range(9)]
    good = [b.ctypes.data_as(ctypes.c_void_p) for b in bufs]
    num, den = T.ctypes.data_as(ctypes.c_void_p), T[8:].ctypes.data_as(ctypes.c_void_p)
    assert fn(num, den, ctypes.c_int(n), *good[:8], None, ctypes.c_int(1)) == 0
    assert fn(num, den, ctypes.c_int(n), *good, ctypes.c_int(1)) == 0
    assert fn(None, den, ctypes.c_int(n), *good, ctypes.c_int(1)) == -1 == fn(num, None, ctypes.c_int(n), *good, ctypes.c_int(1))
    for at in range(8):                                            # (the ninth, the levels, may be NULL)
        args = list(good)
        args[at] = None
        assert fn(num, den, ctypes.c_int(n), *args, ctypes.c_int(1)) == -1, at
    for bad in (2, 30, 0, -1):
        assert fn(num, den, ctypes.c_int(bad), *good, ctypes.c_int(1)) == -1, bad


# ---- e. under the sanitizers ----------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_under_address_and_ub_sanitizers(tmp_path):
    """`make -C oracle/c fraction_sum_selfcheck`: n = 3 .. 10, four kinds of pair, 1 and 4 threads and with and without the levels
    give equal bytes, the tree and the chain equal the ones the program builds itself, exact-size output buffers; the lookup's
    multiplicities against a quadratic count and its pair entry by entry; no sanitizer report.  A child process: nothing is loaded
    into this one."""
    exe = str(tmp_path / "fraction_sum_selfcheck")
    build = subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "c"), "fraction_sum_selfcheck", "OUT=" + exe], capture_output=True, text=True)
    if build.returncode != 0:
        if "sanitize" in build.stderr or "asan" in build.stderr or "ubsan" in build.stderr:
            pytest.skip("no AddressSanitizer runtime for this compiler: " + build.stderr[-200:])
        pytest.fail(build.stdout + build.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "fraction_sum_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

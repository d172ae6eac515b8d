"""The lookup argument (include/gkr_amd.h, gkr_lookup*) as far as no device is needed: the symbols; the slot function h
(gkr_selftest_lookup_slot, the function the kernels call) against its restatement in tests/lookup_model.py; the identity the
argument rests on -- sum N / D = 0 on integers for honest instances, != 0 for every dishonest instance the GPU tests expect LOOKUP
for, so that expectation does not rest on chance; gkr_amd.verifier.verify_lookup against the model's verdict over every
single-element change of a proof (tests/fraction_sum_sweeps.py) and over the lookup's own changes; the closed forms of N~(z) and
D~(z) in W~, T~, M~ and the padding's prefix factor; the argument checks that return before a device is touched; and
csrc/lookup_rules.h in a stand-alone program under AddressSanitizer and UBSan (a child process: no sanitizer goes near code loaded
into python)."""

import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import gkr_amd
from gkr_amd import _native as N
from gkr_amd.field import to_limbs
from gkr_amd.prover import Context
from gkr_amd.verifier import verify_lookup
from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR, head_root, mle, proof_arrays)
from fraction_sum_sweeps import ACCEPTED, apply, layers_of, tamperings
from lookup_model import (EMPTY, LOOKUP, SEED, dishonest_instances, fresh_alpha, honest_instance, lookup, model_verdict, multiplicities, pair,
                          pair_log2, plain_sum, slot, split_instance)
from oracle.field import P

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_lookup_multiplicities_device", "gkr_lookup_batch_device", "gkr_lookup_verify_batch_device", "gkr_lookup", "gkr_lookup_verify",
         "gkr_selftest_lookup_slot", "gkr_devtest_lookup_pair"]


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("lookup_multiplicities_device", "lookup_batch_device", "verify_lookup_batch_device", "prove_lookup", "verify_lookup"):
        assert callable(getattr(Context, name)), name
    assert callable(gkr_amd.prove_lookup) and callable(gkr_amd.verify_lookup)
    assert "prove_lookup" in gkr_amd.__all__ and "verify_lookup" in gkr_amd.__all__
    assert re.search(r"GKR_VERIFY_LOOKUP = 16\b", header) and N.GKR_VERIFY_LOOKUP == 16 == LOOKUP


# ---- the slot function ----------------------------------------------------------------------------------------------------------------------
def native_slot(v, log_slots):
    out = np.full(2, 0xDEAD, dtype=np.uint32)
    assert N.lib().gkr_selftest_lookup_slot(to_limbs([v]).ctypes.data, log_slots, out.ctypes.data) == N.GKR_OK
    assert out[1] == 0xDEAD
    return int(out[0])


def slot_values():
    rng = random.Random(SEED)
    base = rng.randrange(P >> 2)                                   # (room for a bit in every limb)
    return ([rng.randrange(P) for _ in range(64)] + [0, 1, 2, 3, P - 1, P - 2, (1 << 64) - 1, 1 << 64, 1 << 128, 1 << 192]
            + [base] + [base ^ (1 << (32 * limb + 7)) for limb in range(8)])


def test_the_slot_function_is_the_models():
    values = slot_values()
    for v in values:
        for s in (1, 3, 4, 10, 21, 31, 32):
            got = native_slot(v, s)
            assert got == slot(v, s) and got < 1 << s, (hex(v), s)
    # values that differ in ONE of the eight 32-bit limbs, each in turn: every limb reaches the slot
    base, flipped = values[-9], values[-8:]
    full = [slot(v, 32) for v in [base] + flipped]
    assert len(set(full)) == 9, full
    assert len({slot(v, 10) for v in range(1024)}) > 600           # small integers spread (a uniform draw fills ~647 of 1024)


def test_the_slot_function_refuses_bad_arguments():
    word = (ctypes.c_uint64 * 8)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    for args in ((None, 4, fake), (fake, 4, None), (fake, 0, fake), (fake, -1, fake), (fake, 33, fake)):
        assert N.lib().gkr_selftest_lookup_slot(*args) == N.GKR_ERR_INVALID, args[1]
    assert not any(word)


# ---- the identity the argument rests on -----------------------------------------------------------------------------------------------------
SHAPES = ((2, 4), (3, 3), (5, 2), (4, 3))                          # n_w <, =, > n_t


def test_honest_instances_sum_to_zero_on_integers():
    rng = random.Random(SEED + 1)
    for n_w, n_t in SHAPES:
        for duplicates in (False, True):
            W, T = honest_instance(n_w, n_t, rng, duplicates)
            M, missing, first = multiplicities(W, T)
            assert (missing, first) == (0, EMPTY) and sum(M) == len(W)
            if duplicates:
                assert M[1] == 0 == M[-1] and M[3] == 0 and M[0] >= 2 and M[2] >= 1    # the lowest index takes the whole count
            alpha = fresh_alpha(W, T, rng)
            num, den = pair(W, T, M, alpha, n_w, n_t)
            assert len(num) == 2 << max(n_w, n_t) == len(den) and all(den)
            assert plain_sum(num, den) == 0, (n_w, n_t, duplicates)
            g = lookup(W, T, M, alpha, n_w, n_t)
            assert g["sums"][0] == 0 and g["sums"][1] != 0
            assert model_verdict(g["head"], g["layers"], W, T, M, alpha, n_w, n_t) == ACCEPTED
            assert verify_lookup(W, T, M, alpha, g["head"], g["layers"]) == ACCEPTED


def test_dishonest_instances_do_not_sum_to_zero_and_a_lossless_split_does():
    """What the GPU test expects LOOKUP for is asserted here on the model's own P.  A count split over a value's copies with
    nothing lost is no such instance -- the copies' denominators are equal -- and is held to P = 0 and an accepted proof."""
    for n_w, n_t in SHAPES:
        rng = random.Random(SEED + 2)
        for name, (W, T, M) in dishonest_instances(n_w, n_t, rng).items():
            alpha = fresh_alpha(W, T, rng)
            num, den = pair(W, T, M, alpha, n_w, n_t)
            assert plain_sum(num, den) != 0, (n_w, n_t, name)
            g = lookup(W, T, M, alpha, n_w, n_t)
            assert g["sums"][0] != 0 and g["sums"][1] != 0 and g["sums"][0] == plain_sum(num, den) * g["sums"][1] % P
            assert model_verdict(g["head"], g["layers"], W, T, M, alpha, n_w, n_t) == (LOOKUP, 0, 0), (n_w, n_t, name)
            assert verify_lookup(W, T, M, alpha, g["head"], g["layers"]) == (LOOKUP, 0, 0), (n_w, n_t, name)
            if name == "miss":
                assert multiplicities(W, T)[1:] == (1, len(W) // 2)
        W, T, M = split_instance(n_w, n_t, rng)
        alpha = fresh_alpha(W, T, rng)
        assert M != multiplicities(W, T)[0] and plain_sum(*pair(W, T, M, alpha, n_w, n_t)) == 0
        g = lookup(W, T, M, alpha, n_w, n_t)
        assert g["sums"][0] == 0 and verify_lookup(W, T, M, alpha, g["head"], g["layers"]) == ACCEPTED


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def proof():
    """One honest proof at n_w = n_t = 3, L = 4."""
    rng = random.Random(SEED + 3)
    W, T = honest_instance(3, 3, rng)
    M = multiplicities(W, T)[0]
    alpha = fresh_alpha(W, T, rng)
    return W, T, M, alpha, lookup(W, T, M, alpha, 3, 3)


def test_every_single_element_change_gets_the_models_verdict(proof):
    """The sweep of tests/fraction_sum_sweeps.py on the proof's elements: gkr_amd.verifier.verify_lookup against lookup_model's
    verdict.  A head entry + 1 that moves P off zero is LOOKUP at (0, 0), where the fractional sum without claimed sums reports
    ROUND_SUM at (2, 0) -- which stands where the entry's cofactor is zero and P stays; every other change leaves the head alone
    and gets the sweep's closed-form verdict."""
    W, T, M, alpha, g = proof
    L = 4
    arrays = proof_arrays(g, L)
    seen, moved = set(), 0
    for name, what, want in tamperings(g, L, False, False):
        arr, _, _, _ = apply(what, arrays, None, None, None)
        layers = layers_of(arr, L)
        if what[0] == "head" and what[-1] == "+1":
            assert want == (ROUND_SUM, 2, 0), name
            if head_root(arr[0])[0] != 0:                          # (P moves by the entry's cofactor, which a quarter without hits makes zero)
                want = (LOOKUP, 0, 0)
                moved += 1
        assert model_verdict(arr[0], layers, W, T, M, alpha, 3, 3) == want, name
        assert verify_lookup(W, T, M, alpha, arr[0], layers) == want, name
        seen.add(want[0])
    assert seen >= {SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, LOOKUP} and moved >= 4


def test_the_lookups_own_changes(proof):
    W, T, M, alpha, g = proof
    L, head, layers = 4, g["head"], g["layers"]

    def verdict(W=W, T=T, M=M, alpha=alpha, head=head, layers=layers):
        got = verify_lookup(W, T, M, alpha, head, layers)
        assert got == model_verdict(head, layers, W, T, M, alpha, 3, 3)
        return got

    assert verdict() == ACCEPTED
    j = next(j for j, m in enumerate(M) if m)
    assert verdict(M=M[:j] + [M[j] + 1] + M[j + 1:]) == (EVALUATION, L, L)           # M other than the prover's
    assert verdict(M=M[:j] + [M[j] - 1] + M[j + 1:]) == (EVALUATION, L, L)
    assert verdict(alpha=(alpha + 1) % P) == (EVALUATION, L, L)                      # alpha other than the prover's
    # alpha equal to a table value, or to a witness value: a zero in D, Q = 0, proved all the same
    for bad in (T[5], W[1]):
        gz = lookup(W, T, M, bad, 3, 3)
        assert gz["sums"][1] == 0 and verdict(alpha=bad, head=gz["head"], layers=gz["layers"]) == (ZERO_DENOMINATOR, 0, 0)
    # the order: NON_CANONICAL and ZERO_DENOMINATOR before LOOKUP, LOOKUP before the layers and the evaluation
    rng = random.Random(SEED + 2)
    Wm, Tm, Mm = dishonest_instances(3, 3, rng)["miss"]
    am = fresh_alpha(Wm, Tm, rng)
    gm = lookup(Wm, Tm, Mm, am, 3, 3)
    assert verdict(Wm, Tm, Mm, am, gm["head"], gm["layers"]) == (LOOKUP, 0, 0)
    assert verdict(Wm, Tm, Mm, (am + 1) % P, gm["head"], gm["layers"]) == (LOOKUP, 0, 0)            # (not EVALUATION)
    proof0, r0, vals0 = gm["layers"][0]
    assert verdict(Wm, Tm, Mm, am, gm["head"], [(proof0, [(r0[0] + 1) % P] + r0[1:], vals0)] + gm["layers"][1:]) == (LOOKUP, 0, 0)
    assert verdict(Wm, Tm, Mm, am, gm["head"], [(proof0, [P] + r0[1:], vals0)] + gm["layers"][1:]) == (NON_CANONICAL, 2, 0)
    assert verdict(Wm, Tm, Mm, am, [P] + gm["head"][1:], gm["layers"]) == (NON_CANONICAL, 0, 0)
    assert verdict(Wm, Tm, Mm, am, gm["head"][:4] + [0] + gm["head"][5:], gm["layers"]) == (ZERO_DENOMINATOR, 0, 0)


# ---- the closed forms of N~ and D~ ---------------------------------------------------------------------------------------------------------
def test_the_closed_forms_of_the_pairs_extensions():
    """With z = (z_1, z'), z' of L - 1 coordinates, and for a side of 2^m entries padded to 2^(L-1): pre = prod over the first
    L - 1 - m coordinates of z' of (1 - z'_i), tail = the last m coordinates:
        N~(z) = (1 - z_1) pre_w  -  z_1 pre_t M~(tail_t)
        D~(z) = (1 - z_1) (pre_w (alpha - W~(tail_w)) + 1 - pre_w)  +  z_1 (pre_t (alpha - T~(tail_t)) + 1 - pre_t)
    -- what a verifier with W~, T~, M~ at the sub-points needs instead of the rebuilt pair."""
    rng = random.Random(SEED + 4)
    for n_w, n_t in SHAPES:
        W, T = honest_instance(n_w, n_t, rng, duplicates=True)
        M = multiplicities(W, T)[0]
        alpha = fresh_alpha(W, T, rng)
        num, den = pair(W, T, M, alpha, n_w, n_t)
        L = pair_log2(n_w, n_t)
        for _ in range(3):
            z = [rng.randrange(P) for _ in range(L)]
            rest = z[1:]

            def side(m):
                pre = 1
                for x in rest[:L - 1 - m]:
                    pre = pre * (1 - x) % P
                return pre, rest[L - 1 - m:]

            (pre_w, tail_w), (pre_t, tail_t) = side(n_w), side(n_t)
            want_n = ((1 - z[0]) * pre_w - z[0] * pre_t * mle(M, tail_t)) % P
            want_d = ((1 - z[0]) * (pre_w * (alpha - mle(W, tail_w)) + 1 - pre_w) + z[0] * (pre_t * (alpha - mle(T, tail_t)) + 1 - pre_t)) % P
            assert (mle(num, z), mle(den, z)) == (want_n, want_d), (n_w, n_t)


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------
# (n_w, n_t, batch) outside the shapes: batch * 2^(L+1) = 2^31 at (29, 2, 1), (2, 29, 1), (28, 3, 2) and (19, 19, 1024)
BAD_SHAPES = ((1, 3, 1), (3, 1, 1), (0, 3, 1), (3, -1, 1), (30, 3, 1), (3, 30, 1), (31, 3, 1), (3, 3, 0), (3, 3, -1), (3, 3, 65536),
              (29, 2, 1), (2, 29, 1), (28, 3, 2), (19, 19, 1024))
GOOD_SHAPES = ((2, 2, 1, 3), (3, 3, 65535, 4), (28, 2, 1, 29), (2, 28, 1, 29), (19, 19, 512, 20), (5, 2, 3, 6))


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device / host pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID

    def sweep(fn, good, required, shape_at):
        for at in required:
            args = list(good)
            args[at] = None
            assert fn(*args) == INVALID, (fn.__name__, at)
        for n_w, n_t, batch in BAD_SHAPES:
            args = list(good)
            args[shape_at[0]], args[shape_at[1]] = n_w, n_t
            if shape_at[2] is None:
                if batch != 1:
                    continue
            else:
                args[shape_at[2]] = batch
            assert fn(*args) == INVALID, (fn.__name__, n_w, n_t, batch)

    # ctx, d_witness, n_w, d_table, n_t, shared_table, batch, d_mult, out_missing, out_first_missing
    sweep(lib.gkr_lookup_multiplicities_device, [fake, fake, 3, fake, 3, 0, 1, fake, fake, fake], (0, 1, 3, 7, 8, 9), (2, 4, 6))
    # ctx, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, the eight outputs (the last three may be NULL)
    sweep(lib.gkr_lookup_batch_device, [fake, fake, 3, fake, 3, 0, fake, fake, 1] + [fake] * 8, (0, 1, 3, 6, 7, 9, 10, 11, 12, 13), (2, 4, 8))
    # .., batch, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check, out_sums (the last four may be NULL)
    sweep(lib.gkr_lookup_verify_batch_device, [fake, fake, 3, fake, 3, 0, fake, fake, 1] + [fake] * 10, (0, 1, 3, 6, 7, 9, 10, 11, 12, 13, 14), (2, 4, 8))
    # ctx, witness, n_w, table, n_t, alpha, out_mult, out_missing, out_first_missing, the eight outputs
    sweep(lib.gkr_lookup, [fake, fake, 3, fake, 3] + [fake] * 12, (0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13), (2, 4, None))
    # ctx, witness, n_w, table, n_t, mult, alpha, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check
    sweep(lib.gkr_lookup_verify, [fake, fake, 3, fake, 3] + [fake] * 11, (0, 1, 3, 5, 6, 7, 8, 9, 10, 11, 12), (2, 4, None))
    # ctx, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, d_pair
    sweep(lib.gkr_devtest_lookup_pair, [fake, fake, 3, fake, 3, 0, fake, fake, 1, fake], (0, 1, 3, 6, 7, 9), (2, 4, 8))
    assert not any(word)                                           # nothing was written


# ---- csrc/lookup_rules.h alone under sanitizers -------------------------------------------------------------------------------------------------
def test_the_rules_stand_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/lookup_rules_selfcheck.cpp with csrc/lookup_rules.h: the slot function on this file's values at every log_slots, the
    shapes above, and the verdict rule on every inner verdict x (P zero, P not zero), each against lookup_model's statement; no
    sanitizer report.  (make -C gkr_amd/csrc asan_lk builds the same program.)"""
    cases = str(tmp_path / "cases.txt")
    inner = [ACCEPTED, (SHAPE, 3, 1), (NON_CANONICAL, 0, 0), (NON_CANONICAL, 2, 2), (ZERO_DENOMINATOR, 0, 0), (ROUND_SUM, 2, 0), (CHALLENGE, 3, 2),
             (FINAL_CLAIM, 3, 3), (EVALUATION, 4, 4)]
    with open(cases, "w") as f:
        for v in slot_values():
            for s in range(1, 33):
                f.write("slot %064x %d %d\n" % (v, s, slot(v, s)))
        for n_w, n_t, batch in BAD_SHAPES:
            f.write("shape %d %d %d 0\n" % (n_w, n_t, batch))
        for n_w, n_t, batch, L in GOOD_SHAPES:
            assert L == pair_log2(n_w, n_t)
            f.write("shape %d %d %d %d\n" % (n_w, n_t, batch, L))
        for v in inner:
            for p in (0, 1, 1 << 64, 1 << 128, 1 << 192, P - 1):
                want = v if p == 0 or v[0] in (SHAPE, NON_CANONICAL, ZERO_DENOMINATOR) else (LOOKUP, 0, 0)
                f.write("verdict %064x %d %d %d %d %d %d\n" % ((p, v[0], v[1], v[2]) + want))
    exe = str(tmp_path / "lookup_rules_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                            os.path.join(REPO, "tests", "lookup_rules_selfcheck.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr[-3000:]
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "lookup_rules_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]

"""The plain sumcheck's verifier and the multilinear evaluation (include/gkr_amd.h, "the plain sumcheck's verifier") as far as no
device is needed: the three symbols, the argument checks that run before a device is touched, the option, a model of the
streaming kernel's index mapping (csrc/kernels_mle_eval.hip), and the closed-form verdict model of tests/mle_verify_sweeps.py
against the relations evaluated one after the other on Python integers."""

import ctypes
import os
import random
import re

import numpy as np
import pytest

import gkr_amd
from gkr_amd import _native as N
from gkr_amd import multi_hash
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.prover import Context, options
from gkr_amd.verifier import mle_eval, verify_sumcheck, verify_sumcheck_table
from mle_verify_sweeps import (ACCEPTED, LENGTH_RULE_TABLES, arrays_of, assert_sweep_reaches_short_rows, build_batch, cases, eq_weight,
                               reference_verdict, rounds_of)
from verify_sweeps import value

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_mle_eval_batch_device", "gkr_sumcheck_mle_verify_batch_device", "gkr_sumcheck_mle_verify"]


def test_the_three_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    assert re.search(r"GKR_VERIFY_EVALUATION\s*=\s*10\b", header) and N.GKR_VERIFY_EVALUATION == 10
    assert callable(Context.mle_eval_batch_device) and callable(Context.verify_sumcheck_batch_device) and callable(Context.verify_sumcheck)
    assert "mle_eval" in gkr_amd.__all__ and "verify_sumcheck_table" in gkr_amd.__all__


def test_bad_arguments_are_invalid_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context / device pointer that is never dereferenced."""
    lib = N.lib()
    word = (ctypes.c_uint64 * 64)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    accept, rnd, check = ctypes.c_int(7), ctypes.c_uint32(9), ctypes.c_uint32(9)
    INVALID = N.GKR_ERR_INVALID
    ev = lib.gkr_mle_eval_batch_device
    assert ev(None, fake, 3, 1, fake, fake) == INVALID
    assert ev(fake, None, 3, 1, fake, fake) == INVALID
    assert ev(fake, fake, 3, 1, None, fake) == INVALID
    assert ev(fake, fake, 3, 1, fake, None) == INVALID
    for batch in (0, -2):
        assert ev(fake, fake, 3, batch, fake, fake) == INVALID
    for n in (0, -1, 31):
        assert ev(fake, fake, n, 1, fake, fake) == INVALID
    vb = lib.gkr_sumcheck_mle_verify_batch_device
    good = [fake, fake, 3, 1, fake, fake, fake, fake, ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check), fake]
    for at in (0, 1, 5, 6, 7, 8):                      # ctx, tables, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert vb(*args) == INVALID, at
    for at, bad in ((3, 0), (3, -1), (2, 1), (2, 0), (2, 31)):      # batch < 1; n outside 2 .. 30
        args = list(good)
        args[at] = bad
        assert vb(*args) == INVALID, (at, bad)
    v1 = lib.gkr_sumcheck_mle_verify
    good = [fake, fake, 3, fake, fake, fake, fake, ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check)]
    for at in (0, 1, 4, 5, 6, 7):                      # ctx, table, coeffs, len, r, accept
        args = list(good)
        args[at] = None
        assert v1(*args) == INVALID, at
    for n in (1, 0, 31):
        args = list(good)
        args[2] = n
        assert v1(*args) == INVALID, n
    assert (accept.value, rnd.value, check.value) == (7, 9, 9)          # nothing was written


def test_the_option_is_in_the_table():
    table = {name: (env, doc) for name, env, doc in options()}
    assert "mle_eval_mfma_min_n" in table
    env, doc = table["mle_eval_mfma_min_n"]
    assert env == "GKR_MLE_EVAL_MFMA_MIN_N" and "gkr_mle_eval_batch_device" in doc


# ---- the streaming kernel's index mapping, on integers -------------------------------------------------------------------------
# k_mle_eval_mfma: the five leading variables are bound by the fold (weights w_b = eq((r_1..r_5), b) over 32 streams of stride
# S = 2^(n-5)); output i of the fold is weighted by eq((r_6..r_n), i) = E_up[i >> 6] * E_63[i & 63].  A block owns `chunk`
# consecutive outputs; its four waves turn 64 outputs each per iteration (tile start e0 = begin + cur * 256 + wave * 64), the
# iterations start at rot % iters and wrap around; a lane sums y * E_up[e0 >> 6] over its iterations and multiplies by E_63[lane]
# once; the block's lanes are added up, then the blocks.
# (The four constants below restate kEvalChunk .. kEvalMaxBlocks of kernels_mle_eval.hip by hand: nothing ties them to the
# library, so these tests hold the SCHEME -- any power-of-two block count in that range leaves whole wave tiles -- and not the
# library's numbers; the kernel's results at its own block counts are what test_gpu_mle_eval.py checks.)
EVAL_CHUNK, EVAL_MIN_CHUNK, EVAL_FILL_BLOCKS, EVAL_MAX_BLOCKS = 2048, 256, 2048, 4096


def model_blocks(n, batch):
    S = 1 << (n - 5)
    b = max(1, S // EVAL_CHUNK)
    while b * batch < EVAL_FILL_BLOCKS and S // (2 * b) >= EVAL_MIN_CHUNK:
        b *= 2
    return min(b, EVAL_MAX_BLOCKS)


def model_fold5(table, point):
    """The fold's outputs: y[i] = sum_b eq((r_1..r_5), b) T[b S + i]."""
    S = len(table) >> 5
    w = [eq_weight(point[:5], b) for b in range(32)]
    return [sum(w[b] * table[b * S + i] for b in range(32)) % P for i in range(S)]


def model_streaming_eval(y, point, nblk, table_index=0):
    n = len(point)
    m = n - 5
    S = 1 << m
    e_up = [eq_weight(point[5:n - 6], u) for u in range(1 << (m - 6))]
    e_63 = [eq_weight(point[n - 6:], l) for l in range(64)]
    chunk = S // nblk
    assert chunk * nblk == S and chunk % 64 == 0
    seen = [0] * S
    total = 0
    for bx in range(nblk):
        begin, span = bx * chunk, chunk
        iters = (span + 255) // 256
        rot = bx * 5 + table_index * 3
        lane_sums = [[0] * 64 for _ in range(4)]
        for wave in range(4):
            if wave * 64 >= span:
                continue
            cur = rot % iters
            for _ in range(iters):
                e0 = begin + cur * 256 + wave * 64
                assert e0 % 64 == 0 and begin <= e0 and e0 + 64 <= begin + span
                for lane in range(64):
                    i = e0 + lane
                    assert i >> 6 == e0 >> 6 and i & 63 == lane      # the wave-uniform factor and the lane's constant factor
                    seen[i] += 1
                    lane_sums[wave][lane] += y[i] * e_up[e0 >> 6]
                cur = 0 if cur + 1 == iters else cur + 1
        total += sum(lane_sums[wv][lane] % P * e_63[lane] for wv in range(4) for lane in range(64))
    assert seen == [1] * S                                             # every output exactly once, whatever the start
    return total % P


@pytest.mark.parametrize("m", range(6, 13))
def test_model_of_the_streaming_form_reproduces_the_sum(m):
    """Every n - 5 in 6 .. 12 (the middle table has 0 .. 6 variables: odd and even counts, and none at all at n = 11), chunks of
    one wave tile, of part of an iteration (idle waves), of one and of several iterations with every wrap-around start."""
    n = m + 5
    rng = random.Random(700 + m)
    small = [0, 1, P - 1, 2, P - 2]
    table = [rng.choice(small) if rng.random() < 0.25 else rng.randrange(P) for _ in range(1 << n)]
    point = [rng.choice([0, 1, P - 1]) if rng.random() < 0.2 else rng.randrange(P) for _ in range(n)]
    want = mle_eval(table, point)
    if m <= 8:
        assert want == sum(eq_weight(point, i) * table[i] for i in range(1 << n)) % P
    y = model_fold5(table, point)
    S = 1 << m
    counts = {model_blocks(n, 1), model_blocks(n, 9), model_blocks(n, 4096), 1, S // 64}
    for nblk in sorted(counts):
        for table_index in (0, 1, 5):
            assert model_streaming_eval(y, point, nblk, table_index) == want, (nblk, table_index)


def test_model_block_counts_divide_the_outputs_into_wave_tiles():
    for n in range(11, 31):
        for batch in (1, 2, 3, 9, 64, 1024, 4096, 32768):
            b = model_blocks(n, batch)
            S = 1 << (n - 5)
            assert 1 <= b <= EVAL_MAX_BLOCKS and S % b == 0 and (S // b) % 64 == 0, (n, batch, b)


# ---- the closed-form verdict model -------------------------------------------------------------------------------------------------
def test_verdict_model_against_the_relations_on_the_golden_cases(mle_cases):
    """Every tampering of the sweep, with and without a claim: the model's triple equals the relations run in order on Python
    integers; where the tampered transcript is still well-formed, its accept bit equals gkr_amd.verifier's verify_sumcheck plus a
    Python fold of the table (verify_sumcheck_table)."""
    for case in mle_cases:
        n, table = case["n"], [int(x) for x in case["table"]]
        proof, r = [[int(x) for x in g] for g in case["proof"]], [int(x) for x in case["r"]]
        assert all(eq_weight(r, i) != 0 for i in range(1 << n))        # a table entry + 1 always moves T(r)
        claim = sum(table) % P
        assert verify_sumcheck(claim, proof, r) == (True, mle_eval(table, r))
        C, L, R = arrays_of(proof, r)
        T = to_limbs(table)
        for with_claim in (True, False):
            sweep = cases(C, L, R, with_claim)
            kinds = {c.what for c in sweep}
            assert kinds == {"honest", "slot", "r", "len", "table"} | ({"claim"} if with_claim else set())
            Tb, Cb, Lb, Rb, cl = build_batch(T, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
            for e, c in enumerate(sweep):
                cl_e = value(cl[e]) if with_claim else None
                tab_e = from_limbs(Tb[e])
                assert reference_verdict(tab_e, Cb[e], Lb[e], Rb[e], cl_e, multi_hash) == c.verdict, (n, with_claim, c)
                well_formed = c.verdict[2] not in (1, 2) and all(1 <= int(x) <= 2 for x in Lb[e]) and \
                    all(value(x) < P for x in Rb[e]) and all(value(Cb[e, j, t]) < P for j in range(n) for t in range(2 - int(Lb[e, j]), 2))
                if well_formed:
                    assert verify_sumcheck_table(tab_e, rounds_of(Cb[e], Lb[e]), from_limbs(Rb[e]), cl_e) == c.verdict[0], (n, c)
            assert sweep[0].verdict == ACCEPTED and sweep[-1].verdict == ACCEPTED


def test_verdict_model_against_the_relations_on_rows_of_length_one():
    """The golden transcripts have two coefficients in every row.  Tables that do not depend on some variable (the oracle's prover
    gives their transcripts) have rows of length 1: the sweep then holds every unused slot changed (accepted: never read) and
    every length 1 -> 2 (the same polynomial under another hash: CHALLENGE at that row)."""
    from oracle import cdense
    for table in LENGTH_RULE_TABLES:
        n = len(table).bit_length() - 1
        T = to_limbs(table)
        C, L, R = cdense.sumcheck_mle_raw(T, n)
        r = from_limbs(R)
        assert all(eq_weight(r, i) != 0 for i in range(1 << n))
        claim = sum(table) % P
        assert verify_sumcheck_table(table, rounds_of(C, L), r, claim)
        for with_claim in (True, False):
            sweep = cases(C, L, R, with_claim)
            assert_sweep_reaches_short_rows(sweep, L)
            Tb, Cb, Lb, Rb, cl = build_batch(T, C, L, R, to_limbs([claim])[0] if with_claim else None, sweep)
            for e, c in enumerate(sweep):
                cl_e = value(cl[e]) if with_claim else None
                assert reference_verdict(from_limbs(Tb[e]), Cb[e], Lb[e], Rb[e], cl_e, multi_hash) == c.verdict, (n, with_claim, c)

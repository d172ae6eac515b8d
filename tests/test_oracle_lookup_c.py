"""ogkr_lookup_multiplicities and ogkr_lookup_pair (oracle/c/ogkr.c; cdense.lookup_multiplicities_raw, lookup_pair_raw, lookup_raw),
the C twins of tests/lookup_model.py that tests/test_gpu_lookup_sizes.py compares gkr_lookup* with at sizes the Python model
cannot reach.  The count sorts the table's indices by (value, index) and searches per witness entry: no hash table, no slot
function, nothing of csrc/kernels_lookup.hip.  What holds them:

  a. lookup_model.multiplicities and .pair on every instance of tests/lookup_cases.py (the ones the device runs in
     tests/test_gpu_lookup.py), and the whole proof against lookup_model.lookup where the model is fast (L <= 8);
  b. the same at (n_w, n_t) = (2, 4), (3, 3), (5, 2), (7, 7) on honest instances with and without repeated table values, on every
     dishonest instance (P != 0, LOOKUP from the model's verifier on the oracle's proof) and on the lossless split (P = 0, accepted);
  c. at (12, 12), beyond the model's proof: the count against numpy's own sort, the pair by its rule in limbs, P = 0;
  d. bad shapes are -1.
The stand-alone sanitizer program of tests/test_oracle_fraction_sum_c.py covers both functions too."""

import random

import numpy as np
import pytest

from fraction_sum_model import proof_arrays
from fraction_sum_oracle import as_model, lookup_instance
from fraction_sum_sweeps import ACCEPTED
from lookup_cases import CASES
from lookup_model import (EMPTY, LOOKUP, SEED, dishonest_instances, fresh_alpha, honest_instance, lookup, model_verdict, multiplicities, pair,
                          pair_log2, split_instance)
from oracle import cdense
from oracle.field import P

SHAPES = ((2, 4), (3, 3), (5, 2), (7, 7))
MODEL_PROOF_MAX_L = 8


def _log2(values):
    return len(values).bit_length() - 1


def _assert_instance(W, T, M, alpha, what, counted=True):
    """The oracle's count (if M is the honest count), pair and proof of (W, T, M, alpha) against the model's -> the proof's dict
    (the model's where it is fast, else the oracle's own)."""
    n_w, n_t = _log2(W), _log2(T)
    L = pair_log2(n_w, n_t)
    Wl, Tl, Ml, al = cdense.to_limbs(W), cdense.to_limbs(T), cdense.to_limbs(M), cdense.to_limbs([alpha])[0]
    Mo, missing, first = cdense.lookup_multiplicities_raw(Wl, Tl)
    want = multiplicities(W, T)
    assert (cdense.from_limbs(Mo), missing, first) == want, what
    if counted:
        assert want[0] == M, what
    num, den = pair(W, T, M, alpha, n_w, n_t)
    Po = cdense.lookup_pair_raw(Wl, Tl, Ml, al)
    assert Po.shape == (2, 1 << L, 4) and cdense.from_limbs(Po[0]) == num and cdense.from_limbs(Po[1]) == den, what
    raw = cdense.lookup_raw(Wl, Tl, Ml, al)
    assert all(np.array_equal(a, b) for a, b in zip(raw, cdense.fraction_sum_raw(Po, L))), what
    got = as_model(raw, L)
    if L <= MODEL_PROOF_MAX_L:
        g = lookup(W, T, M, alpha, n_w, n_t, use_np=L > 5)
        assert all(got[key] == g[key] for key in ("sums", "head", "layers", "points", "lambdas", "claims", "eqs", "point", "claim")), what
        assert proof_arrays(got, L) == proof_arrays(g, L), what
    return got


# ---- a. the instances the device runs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_shared_cases_match_the_model(name):
    W, T = CASES[name]
    M, missing, _ = multiplicities(W, T)
    g = _assert_instance(W, T, M, fresh_alpha(W, T, random.Random(SEED + 20)), name)
    assert (g["sums"][0] == 0) == (missing == 0) and g["sums"][1] != 0, name


# ---- b. the host test's shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_w,n_t", SHAPES)
def test_honest_dishonest_and_split_instances_match_the_model(n_w, n_t):
    rng = random.Random(SEED + 21 + 100 * n_w + n_t)
    L = pair_log2(n_w, n_t)
    for duplicates in (False, True):
        W, T = honest_instance(n_w, n_t, rng, duplicates=duplicates)
        M, alpha = multiplicities(W, T)[0], fresh_alpha(W, T, rng)
        g = _assert_instance(W, T, M, alpha, (n_w, n_t, duplicates))
        assert g["sums"][0] == 0 and g["sums"][1] != 0 and sum(M) == 1 << n_w
        assert model_verdict(g["head"], g["layers"], W, T, M, alpha, n_w, n_t) == ACCEPTED
    for name, (W, T, M) in dishonest_instances(n_w, n_t, rng).items():
        alpha = fresh_alpha(W, T, rng)
        g = _assert_instance(W, T, M, alpha, (n_w, n_t, name), counted=name == "miss")
        assert g["sums"][0] != 0, name
        assert model_verdict(g["head"], g["layers"], W, T, M, alpha, n_w, n_t) == (LOOKUP, 0, 0), name
    W, T, M = split_instance(n_w, n_t, rng)
    alpha = fresh_alpha(W, T, rng)
    g = _assert_instance(W, T, M, alpha, (n_w, n_t, "split"), counted=False)
    assert g["sums"][0] == 0 and M != multiplicities(W, T)[0] and model_verdict(g["head"], g["layers"], W, T, M, alpha, n_w, n_t) == ACCEPTED
    assert len(g["layers"]) == L - 2


# ---- c. beyond the model's proof --------------------------------------------------------------------------------------------------------
def test_a_large_instance_against_numpy():
    """n_w = n_t = 12, the table with 2^11 distinct values each twice (at j and j + 2^11), sixteen witness entries outside it."""
    n = 12
    _, T, _, alpha = lookup_instance(n, n, 1212)
    T[1 << (n - 1):] = T[:1 << (n - 1)]
    W = np.ascontiguousarray(T[np.random.default_rng(1214).integers(0, 1 << n, size=1 << n)])
    outside = cdense.fill_table(16, 1213)
    W[100:4096:256] = outside
    keys = lambda a: [bytes(row) for row in np.ascontiguousarray(a[:, ::-1]).astype(">u8")]
    first = {}
    for j, key in enumerate(keys(T)):
        first.setdefault(key, j)
    assert len(first) == 1 << (n - 1) and not set(keys(outside)) & set(first)
    want, misses = np.zeros(1 << n, dtype=np.uint64), []
    for i, key in enumerate(keys(W)):
        if key in first:
            want[first[key]] += 1
        else:
            misses.append(i)
    M, missing, first_missing = cdense.lookup_multiplicities_raw(W, T)
    assert np.array_equal(M[:, 0], want) and not M[:, 1:].any() and not M[1 << (n - 1):].any()
    assert (missing, first_missing) == (16, 100) == (len(misses), misses[0])
    W[100:4096:256] = T[5]                                         # now the lookup holds
    M, missing, first_missing = cdense.lookup_multiplicities_raw(W, T)
    assert (missing, first_missing) == (0, EMPTY) and int(M[:, 0].sum()) == 1 << n and int(M[5, 0]) >= 16
    pr = cdense.lookup_pair_raw(W, T, M, alpha)
    a = cdense.from_limbs(alpha.reshape(1, 4))[0]
    assert cdense.from_limbs(pr[0]) == [1] * (1 << n) + [(P - int(m)) % P for m in M[:, 0]]
    assert cdense.from_limbs(pr[1]) == [(a - w) % P for w in cdense.from_limbs(W)] + [(a - t) % P for t in cdense.from_limbs(T)]
    raw = cdense.lookup_raw(W, T, M, alpha)
    assert not raw[0][0].any() and raw[0][1].any()                 # P = 0, Q != 0
    as_model(raw, n + 1)                                           # the chain, formed a second time


# ---- d. bad shapes --------------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_are_minus_one():
    T = cdense.fill_table(16, 5)
    cdense.lookup_multiplicities_raw(T[:4], T[:8])
    cdense.lookup_multiplicities_raw(T[:1], T[:1])                 # n_w = n_t = 0
    for w, t in ((3, 4), (4, 6), (0, 4), (4, 0)):
        with pytest.raises(ValueError, match="rc=-1"):
            cdense.lookup_multiplicities_raw(T[:w], T[:t])
    assert cdense.lookup_pair_raw(T[:1], T[:1], T[:1], T[0]).shape == (2, 2, 4)
    for w, t, m in ((3, 4, 4), (4, 4, 8), (4, 6, 6)):
        with pytest.raises(ValueError):
            cdense.lookup_pair_raw(T[:w], T[:t], T[:m], T[0])
    with pytest.raises(ValueError, match="rc=-1"):
        cdense.lookup_raw(T[:2], T[:2], T[:2], T[0])               # L = 2: below the fractional sum's n >= 3

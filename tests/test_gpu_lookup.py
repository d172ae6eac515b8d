"""gkr_lookup* (csrc/kernels_lookup.hip, csrc/capi_lookup.hip) on the device, against the integer model (tests/lookup_model.py):

  a. the multiplicities, bit for bit, with canaries around d_mult: keys chosen through the slot function so that all land in one
     slot (the longest chain), in the last slot (the wrap) or in distinct slots; a value two and four times in the table (the
     extra copies get 0); entries equal in seven limbs; 0 and r - 1; the first two-block launches on either side (blocks of 256
     threads: n_t = 9, n_w = 9 and 10); one value 2^12 times (every lane on one counter); 0, 1 and several misses, one of them a
     value whose probe chain runs through occupied slots before the empty one (tests/lookup_cases.py); a shared table against
     per-column copies;
  b. the pair (gkr_devtest_lookup_pair) against the model at (n_w, n_t) = (2, 4), (3, 3), (5, 2), with canaries;
  c. the proof: byte-equal to fraction_sum_batch_device on the model's pair uploaded as is, equal to the model at L = 4 .. 6, and
     a batch of 3 with a shared table equal to per-column copies and to each column proved alone;
  d. the verifier: honest proofs under both hash sides; one batch of honest proofs, every dishonest instance of the host test and
     every lookup-specific change, the verdicts lookup_model.model_verdict's;
  e. a fractional-sum call and a lookup call interleaved on one context;  f. the host one-shot forms.

The library's own output is never the reference of a verdict or a value."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from fraction_sum_model import EVALUATION, NON_CANONICAL, ROUND_SUM, ZERO_DENOMINATOR, head_root, proof_arrays, rounds
from fraction_sum_sweeps import ACCEPTED, layers_of
from lookup_cases import CASES, draw as _draw
from lookup_model import (EMPTY, LOOKUP, SEED, dishonest_instances, fresh_alpha, honest_instance, lookup, model_verdict, multiplicities, pair,
                          pair_log2, slot, split_instance)
from resident_tables import Resident
from verify_sweeps import R_LIMBS

pytestmark = pytest.mark.gpu

CANARY = np.array([0xC0DEC0DEC0DEC0DE, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
PAD = 16


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ptr_at(d, elements):
    return ctypes.c_void_p(d.value + 32 * elements)


def _device_multiplicities(ctx, Ws, Ts, shared):
    """Columns Ws against tables Ts (one table with shared) -> ([M], missing, first_missing), canaries around d_mult checked."""
    batch, n_w, n_t = len(Ws), len(Ws[0]).bit_length() - 1, len(Ts[0]).bit_length() - 1
    assert len(Ts) == (1 if shared else batch)
    total = batch << n_t
    with Resident(ctx, to_limbs([x for W in Ws for x in W])) as dw, Resident(ctx, to_limbs([x for T in Ts for x in T])) as dt, \
            Resident(ctx, np.tile(CANARY, (total + 2 * PAD, 1))) as dm:
        missing, first = ctx.lookup_multiplicities_device(dw.d, n_w, dt.d, n_t, shared, batch, _ptr_at(dm.d, PAD))
        dw.assert_unchanged("witness")
        dt.assert_unchanged("table")
        got = ctx.download(dm.d, (total + 2 * PAD, 4))
    assert (got[:PAD] == CANARY).all() and (got[PAD + total:] == CANARY).all(), "canaries around d_mult"
    flat = from_limbs(got[PAD:PAD + total])
    return [flat[b << n_t:(b + 1) << n_t] for b in range(batch)], [int(x) for x in missing], [int(x) for x in first]


# ---- a. the multiplicities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_multiplicities_match_the_model(ctx, name):
    W, T = CASES[name]
    want = multiplicities(W, T)
    if "miss" not in name:
        assert want[1:] == (0, EMPTY) and sum(want[0]) == len(W)
    (M,), missing, first = _device_multiplicities(ctx, [W], [T], True)
    assert (M, missing[0], first[0]) == want, name


def test_the_cases_are_what_their_names_say():
    one = CASES["one slot, n_t = 3"][1]
    assert {slot(v, 4) for v in one} == {5} and {slot(v, 4) for v in CASES["last slot, n_t = 3"][1]} == {15}
    assert {slot(v, 3) for v in CASES["last slot, n_t = 2"][1]} == {7} and len({slot(v, 4) for v in CASES["distinct slots, n_t = 3"][1]}) == 8
    W, T = CASES["repeated table values"]
    assert multiplicities(W, T)[0] == [7, 5, 0, 4, 0, 0, 0, 0]
    W, T = CASES["a miss behind a full chain"]
    assert multiplicities(W, T) == ([1, 0, 0, 0, 0, 0, 0, 1], 2, 1)
    assert multiplicities(*CASES["several misses"])[1:] == (4, 0) and multiplicities(*CASES["every entry a miss"]) == ([0] * 4, 4, 0)
    assert multiplicities(*CASES["one value 2^12 times"])[0] == [0] * 6 + [1 << 12, 0]


def test_a_shared_table_against_per_column_copies_and_per_column_tables(ctx):
    rng = random.Random(SEED + 11)
    Ts = [honest_instance(4, 3, rng)[1] for _ in range(3)]
    Ws = [_draw(Ts[0], 4, rng) for _ in range(3)]
    Ws[1][5] = Ts[1][0]                                            # a miss against table 0
    want = [multiplicities(W, Ts[0]) for W in Ws]
    shared = _device_multiplicities(ctx, Ws, Ts[:1], True)
    assert shared == _device_multiplicities(ctx, Ws, [Ts[0]] * 3, False)
    assert shared == ([w[0] for w in want], [w[1] for w in want], [w[2] for w in want]) and shared[1] == [0, 1, 0] and shared[2][1] == 5
    Ws = [_draw(T, 4, rng) for T in Ts]                            # every column against its own table
    want = [multiplicities(W, T) for W, T in zip(Ws, Ts)]
    assert _device_multiplicities(ctx, Ws, Ts, False) == ([w[0] for w in want], [0] * 3, [EMPTY] * 3)


# ---- b. the pair ------------------------------------------------------------------------------------------------------------------------------
SHAPES = ((2, 4), (3, 3), (5, 2))
_instances = {}


def _instance(n_w, n_t, b=0):
    """(W, T, M, alpha, model proof) of column b at this shape, the same in every test."""
    if (n_w, n_t, b) not in _instances:
        rng = random.Random(SEED + 100 * n_w + 10 * n_t + b)
        W, T = honest_instance(n_w, n_t, rng, duplicates=b == 1)
        M, alpha = multiplicities(W, T)[0], fresh_alpha(W, T, rng)
        _instances[(n_w, n_t, b)] = (W, T, M, alpha, lookup(W, T, M, alpha, n_w, n_t, use_np=True))
    return _instances[(n_w, n_t, b)]


class _Columns:
    """Columns (W, T, M, alpha, ..) of one shape resident on the device: d_w, d_t (per-column tables), d_m."""

    def __init__(self, ctx, cols):
        self.ctx, self.cols = ctx, cols
        self.parts = [Resident(ctx, to_limbs([x for c in cols for x in c[i]])) for i in range(3)]
        self.alpha = [c[3] for c in cols]

    def __enter__(self):
        self.d_w, self.d_t, self.d_m = (p.__enter__().d for p in self.parts)
        return self

    def __exit__(self, *a):
        for p in self.parts:
            p.assert_unchanged("the lookup's inputs")
            p.__exit__(*a)


@pytest.mark.parametrize("n_w,n_t", SHAPES)
def test_the_pair_matches_the_model(ctx, n_w, n_t):
    cols = [_instance(n_w, n_t, b) for b in range(2)]
    L = pair_log2(n_w, n_t)
    total = 2 * (2 << L)
    want = [x for W, T, M, alpha, _ in cols for half in pair(W, T, M, alpha, n_w, n_t) for x in half]
    with _Columns(ctx, cols) as c, Resident(ctx, np.tile(CANARY, (total + 2 * PAD, 1))) as dp:
        alpha = to_limbs(c.alpha)
        rc = N.lib().gkr_devtest_lookup_pair(ctx._h, c.d_w, n_w, c.d_t, n_t, 0, c.d_m, alpha.ctypes.data, 2, _ptr_at(dp.d, PAD))
        assert rc == N.GKR_OK, rc
        got = ctx.download(dp.d, (total + 2 * PAD, 4))
    assert (got[:PAD] == CANARY).all() and (got[PAD + total:] == CANARY).all(), "canaries around the pair"
    assert from_limbs(got[PAD:PAD + total]) == want
    half = 1 << (L - 1)
    assert want[(1 << n_w):half] == [0] * (half - (1 << n_w)) and want[(1 << L) + (1 << n_w):(1 << L) + half] == [1] * (half - (1 << n_w))   # the padding


# ---- c. the proof -----------------------------------------------------------------------------------------------------------------------------
NAMES = ("sums", "head", "coefficients", "lengths", "challenges", "values", "point", "claims")


def _model_arrays(gs, L):
    """The model's proofs as the eight arrays of Context.lookup_batch_device."""
    arrs = [proof_arrays(g, L) for g in gs]
    B, R = len(gs), rounds(L)
    return (to_limbs([x for g in gs for x in g["sums"]]).reshape(B, 2, 4), to_limbs([x for a in arrs for x in a[0]]).reshape(B, 8, 4),
            to_limbs([x for a in arrs for row in a[1] for x in row]).reshape(B, R, 4, 4), np.array([a[2] for a in arrs], dtype=np.uint32).reshape(B, R),
            to_limbs([x for a in arrs for x in a[3]]).reshape(B, R, 4), to_limbs([x for a in arrs for e in a[4] for x in e]).reshape(B, L - 2, 4, 4),
            to_limbs([x for g in gs for x in g["point"]]).reshape(B, L, 4), to_limbs([x for g in gs for x in g["claim"]]).reshape(B, 2, 4))


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("n_w,n_t", SHAPES)
def test_the_proof_is_the_fraction_sums_of_the_pair_and_the_models(ctx, n_w, n_t):
    """L = 5, 4, 6.  Batch 2 with per-column tables: every output byte the model's, and byte-equal to fraction_sum_batch_device
    on the model's pair uploaded as is; P = 0 and Q != 0: the lookups hold; the verifier accepts under both hash sides."""
    cols = [_instance(n_w, n_t, b) for b in range(2)]
    L = pair_log2(n_w, n_t)
    want = _model_arrays([c[4] for c in cols], L)
    with _Columns(ctx, cols) as c:
        got = ctx.lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, c.alpha, 2)
        _assert_same(got, want, (n_w, n_t))
        with Resident(ctx, to_limbs([x for col in cols for half in col[4]["pair"] for x in half])) as dp:
            plain = ctx.fraction_sum_batch_device(dp.d, L, 2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, plain))
        assert not got[0][:, 0].any() and got[0][:, 1].any(axis=-1).all()
        try:
            for hash_min in (1, 2 * rounds(L) + 1):
                ctx.set_option("verify_device_hash_min", hash_min)
                accept, layer, rnd, check, sums = ctx.verify_lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, c.alpha, 2, *got[1:6])
                assert accept.all() and not check.any() and not layer.any() and not rnd.any() and np.array_equal(sums, want[0]), hash_min
        finally:
            ctx.set_option("verify_device_hash_min", 0)


def test_a_shared_table_equals_per_column_copies_and_each_column_alone(ctx):
    n_w, n_t, rng = 4, 3, random.Random(SEED + 12)
    T = honest_instance(n_w, n_t, rng, duplicates=True)[1]
    Ws = [_draw(T, n_w, rng) for _ in range(3)]
    alphas = [fresh_alpha(W, T, rng) for W in Ws]
    Ms = [multiplicities(W, T)[0] for W in Ws]
    with Resident(ctx, to_limbs([x for W in Ws for x in W])) as dw, Resident(ctx, to_limbs(T * 3)) as dt, \
            Resident(ctx, np.zeros((3 << n_t, 4), dtype=np.uint64)) as dm:
        missing, first = ctx.lookup_multiplicities_device(dw.d, n_w, dt.d, n_t, True, 3, dm.d)
        assert not missing.any() and (first == EMPTY).all()
        assert from_limbs(ctx.download(dm.d, (3 << n_t, 4))) == [x for M in Ms for x in M]
        shared = ctx.lookup_batch_device(dw.d, n_w, dt.d, n_t, True, dm.d, alphas, 3)
        copies = ctx.lookup_batch_device(dw.d, n_w, dt.d, n_t, False, dm.d, alphas, 3)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(shared, copies))
        for b in range(3):
            alone = ctx.lookup_batch_device(_ptr_at(dw.d, b << n_w), n_w, dt.d, n_t, True, _ptr_at(dm.d, b << n_t), alphas[b:b + 1], 1)
            assert all(a[b].tobytes() == x[0].tobytes() for a, x in zip(shared, alone)), b
        _assert_same(shared, _model_arrays([lookup(W, T, M, a, n_w, n_t, use_np=True) for W, M, a in zip(Ws, Ms, alphas)], 5), "shared")
        accept, _, _, check, _ = ctx.verify_lookup_batch_device(dw.d, n_w, dt.d, n_t, True, dm.d, alphas, 3, *shared[1:6])
        assert accept.all() and not check.any()


# ---- d. the verifier --------------------------------------------------------------------------------------------------------------------------
def _verdicts(check, layer, rnd):
    return [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]


def _changed(arrays, which, at):
    """One element of (head, C, L, R, E) + 1 modulo r."""
    head, C, Ln, R, E = list(arrays[0]), [list(c) for c in arrays[1]], list(arrays[2]), list(arrays[3]), [list(e) for e in arrays[4]]
    if which == "head":
        head[at] = (head[at] + 1) % P
    elif which == "coeffs":
        C[at][3] = (C[at][3] + 1) % P
    elif which == "r":
        R[at] = (R[at] + 1) % P
    else:
        E[at][2] = (E[at][2] + 1) % P
    return head, C, Ln, R, E


def test_one_batch_of_honest_dishonest_and_changed_proofs_gets_the_models_verdicts(ctx):
    """n_w = n_t = 3, L = 4, per-column tables.  Every case is (what the verifier is given: W, T, M, alpha; the proof's arrays);
    the expectation is lookup_model.model_verdict on exactly that, and the verdicts the header names are also written out."""
    n_w = n_t = 3
    L = 4
    W, T, M, alpha, g = _instance(3, 3)
    arrays = proof_arrays(g, L)
    cases = [("honest", W, T, M, alpha, arrays, ACCEPTED)]
    gz = lookup(W, T, M, T[5], 3, 3)
    cases.append(("alpha = a table value", W, T, M, T[5], proof_arrays(gz, L), (ZERO_DENOMINATOR, 0, 0)))
    j = next(j for j, m in enumerate(M) if m)
    cases.append(("d_mult changed after proving", W, T, M[:j] + [M[j] + 1] + M[j + 1:], alpha, arrays, (EVALUATION, L, L)))
    cases.append(("alpha changed after proving", W, T, M, (alpha + 1) % P, arrays, (EVALUATION, L, L)))
    rng = random.Random(SEED + 2)                                  # the host test's instances at this shape
    for name, (Wd, Td, Md) in dishonest_instances(3, 3, rng).items():
        ad = fresh_alpha(Wd, Td, rng)
        cases.append((name, Wd, Td, Md, ad, proof_arrays(lookup(Wd, Td, Md, ad, 3, 3), L), (LOOKUP, 0, 0)))
    Ws, Ts, Ms = split_instance(3, 3, rng)
    a_s = fresh_alpha(Ws, Ts, rng)
    cases.append(("a lossless split", Ws, Ts, Ms, a_s, proof_arrays(lookup(Ws, Ts, Ms, a_s, 3, 3), L), ACCEPTED))
    cases.append(("head changed", W, T, M, alpha, _changed(arrays, "head", 0), (LOOKUP, 0, 0)))
    cases.append(("coefficient changed", W, T, M, alpha, _changed(arrays, "coeffs", 3), (ROUND_SUM, 3, 1)))
    cases.append(("challenge changed", W, T, M, alpha, _changed(arrays, "r", 0), (5, 2, 0)))
    cases.append(("value changed", W, T, M, alpha, _changed(arrays, "evals", 1), (6, 3, 3)))
    cases.append(("head >= r", W, T, M, alpha, ([P] + list(arrays[0][1:]),) + tuple(arrays[1:]), (NON_CANONICAL, 0, 0)))
    cases.append(("honest", W, T, M, alpha, arrays, ACCEPTED))
    want = []
    for name, Wc, Tc, Mc, ac, arr, expect in cases:
        v = model_verdict(arr[0], layers_of(arr, L), Wc, Tc, Mc, ac, 3, 3)
        assert v == expect, (name, v, expect)
        want.append(v)
    B, R = len(cases), rounds(L)
    raw = lambda values: np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in values], dtype=np.uint64)
    H = raw([x for c in cases for x in c[5][0]]).reshape(B, 8, 4)
    C = raw([x for c in cases for row in c[5][1] for x in row]).reshape(B, R, 4, 4)
    Ln = np.array([c[5][2] for c in cases], dtype=np.uint32).reshape(B, R)
    Rr = raw([x for c in cases for x in c[5][3]]).reshape(B, R, 4)
    E = raw([x for c in cases for e in c[5][4] for x in e]).reshape(B, L - 2, 4, 4)
    cols = [(c[1], c[2], c[3], c[4]) for c in cases]
    roots = [head_root(c[5][0]) if w[0] != NON_CANONICAL else (0, 0) for c, w in zip(cases, want)]
    with _Columns(ctx, cols) as c:
        try:
            for hash_min in (1, B * R + 1):
                ctx.set_option("verify_device_hash_min", hash_min)
                accept, layer, rnd, check, sums = ctx.verify_lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, c.alpha, B, H, C, Ln, Rr, E)
                got = _verdicts(check, layer, rnd)
                diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
                assert diff is None, (hash_min, cases[diff][0], got[diff], want[diff])
                assert list(accept) == [w == ACCEPTED for w in want]
                assert from_limbs(sums.reshape(-1, 4)) == [x for root in roots for x in root]
        finally:
            ctx.set_option("verify_device_hash_min", 0)
        # the device's own proofs of the same columns are the model's, so what was verified is what the device proves
        honest = [i for i, case in enumerate(cases) if case[0] in ("honest", "miss", "plus_one", "split_lossy", "a lossless split")]
        got = ctx.lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, c.alpha, B)
        for i in honest:
            assert got[1][i].tobytes() == H[i].tobytes() and got[2][i].tobytes() == C[i].tobytes() and got[4][i].tobytes() == Rr[i].tobytes(), cases[i][0]
    with _Columns(ctx, cols[:1]) as c, pytest.raises(GkrError) as e:
        ctx.verify_lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, R_LIMBS.reshape(1, 4), 1, H[:1], C[:1], Ln[:1], Rr[:1], E[:1])
    assert e.value.status == N.GKR_ERR_NON_CANONICAL
    with _Columns(ctx, cols[:1]) as c, pytest.raises(GkrError) as e:
        ctx.lookup_batch_device(c.d_w, n_w, c.d_t, n_t, False, c.d_m, R_LIMBS.reshape(1, 4), 1)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL


# ---- e. one context ---------------------------------------------------------------------------------------------------------------------------
def test_a_fraction_sum_and_a_lookup_share_one_context():
    """Interleaved on one context, each call is byte-equal to its run on a fresh context."""
    n = 9
    cols = [_instance(5, 2, b) for b in range(2)]

    def run(c, which):
        out = {}
        d = c.alloc(32 * (2 << n))
        try:
            with _Columns(c, cols) as col:
                for w in which:
                    if w == "f":
                        c.fill_table(d, 2 << n, 77)
                        out[w] = c.fraction_sum_batch_device(d, n, 1)
                    else:
                        out[w] = c.lookup_batch_device(col.d_w, 5, col.d_t, 2, False, col.d_m, col.alpha, 2)
            return out
        finally:
            c.free(d)

    fresh = {}
    for w in "fl":
        with Context(0) as c:
            fresh.update(run(c, w))
    with Context(0) as c:
        for order in ("flfl", "lf"):
            got = run(c, order)
            for w in set(order):
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got[w], fresh[w])), (order, w)


# ---- f. the host one-shot forms ---------------------------------------------------------------------------------------------------------------
def test_the_one_shot_forms(ctx):
    W, T, M, alpha, g = _instance(3, 3)
    mult, miss, sums, head, layers, point, claims = ctx.prove_lookup(W, T, alpha)
    assert (mult, miss) == (M, (0, EMPTY))
    assert (sums, head, layers, point, claims) == (g["sums"], g["head"], g["layers"], g["point"], g["claim"]) and sums[0] == 0
    assert ctx.verify_lookup(W, T, mult, alpha, head, layers) == ACCEPTED
    assert ctx.verify_lookup(W, T, mult, (alpha + 1) % P, head, layers) == (EVALUATION, 4, 4)
    rng = random.Random(SEED + 2)
    Wd, Td, Md = dishonest_instances(3, 3, rng)["miss"]
    ad = fresh_alpha(Wd, Td, rng)
    mult, miss, sums, head, layers, _, _ = ctx.prove_lookup(Wd, Td, ad)
    assert (mult, miss) == (Md, (1, 4)) and sums[0] != 0
    assert ctx.verify_lookup(Wd, Td, mult, ad, head, layers) == (LOOKUP, 0, 0) == model_verdict(head, layers, Wd, Td, Md, ad, 3, 3)
    raw = np.ascontiguousarray(to_limbs(W))
    raw[3] = R_LIMBS
    with pytest.raises(GkrError) as e:
        ctx.prove_lookup(raw, T, alpha)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL

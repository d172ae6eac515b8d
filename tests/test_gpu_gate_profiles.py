"""The layer sumcheck's gate passes AT the thresholds of their control flow.  Which path a gate pass takes is decided by how
many gates share an operand; the other GPU suites draw gates uniformly (bucket lengths Poisson around 2^(k_i - k)) or in one
compiler-like shape, so a threshold is met only if a draw lands on it.  Here the gate lists are built to sit on every one
(tests/gate_profiles.py), each case first asserts what the production list build made of them (gkr_devtest_gate_plan: the
form and the plan's counts) against an integer model -- a case that stops hitting its threshold fails, it does not pass
vacuously -- and then compares (coefficients, lengths, challenges) byte for byte with the C oracle's linear-time layer
prover, which tests/test_oracle_gate_profiles.py holds to the dense provers on scaled-down versions of the same profiles.

Item plan (k = 13):
  I1 (13 | 11, 13)  every bucket one gate / three quarters empty: nothing to combine, no group of two steps
  I2 (14, 13)       buckets of 0 .. 49 gates, items = 1 | 63 (mod 64), groups of at most one step = 1 | 3 (mod 4)
  I3 (16, 13)       1008 .. 1041 gates (63 .. 66 items: 64 | 65) and twenty buckets of 17 .. 1000: both sides of the combine grid
  I4 (18, 13)       16368 .. 32769 gates: 1023, 1024 | 1025, 2048 | 2049 items (one chunk | two | three)
  I5 (22, 13)       2^20 - 16, 2^20 + 1, 3 * 2^19 gates: 64, 65 and 96 chunks (the completing wave's second trip)
  I6 (24, 13)       700 buckets of 16385 .. 16400 gates: 1400 chunks of two-chunk buckets, the capped chunk grid
  I7 (16 | 21, 13)  one bucket holds the layer on both halves
Every case runs through Context.sumcheck_layer_raw (fresh lists, grids from capacities) and ResidentGates.sumcheck_raw twice
(cached lists, exact grids, I1's skipped combine launch), all on ONE context: a plan's arrival counters are met by the next."""

import ctypes
import functools

import numpy as np
import pytest

import gate_profiles as gp
from gkr_amd import Context, GKRCircuit, GkrError, Layer, parallel
from gkr_amd import _native as N
from oracle import cdense

pytestmark = pytest.mark.gpu
K = 13
HALVES = ("left", "right", "both")
LADDER = (0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def _run(ctx, prof, form, w_names, seed=0, mean_log2=4):
    """the devtest's form and counts against the model, then the two call paths against the oracle; -> the counts"""
    counts = gp.assert_plan(ctx, prof, form, mean_log2)
    k_i, k = prof.k_i, prof.k
    lay, z = Layer(k_i, *prof.arrays()), gp.z_point(k_i, seed)
    gates = parallel.ResidentGates(ctx, k_i, 0, *prof.arrays())
    try:
        for i, name in enumerate(w_names):
            W = gp.w_pattern(name, k, seed=seed + i)
            want = cdense.sumcheck_layer_lin_raw(k_i, k, *prof.arrays(), z, W)
            assert _same(ctx.sumcheck_layer_raw(lay, k, z, W), want), ("fresh lists", name)
            for again in range(2 if i == 0 else 1):
                assert _same(gates.sumcheck_raw(k, z, W), want), ("cached lists", name, again)
    finally:
        gates.close()
    return counts


def _spread(k, n, seed, avoid=()):
    """n distinct buckets"""
    rng = np.random.default_rng(seed)
    pool = np.setdiff1d(np.arange(1 << k), np.array(list(avoid), dtype=np.int64))
    return [int(b) for b in rng.choice(pool, n, replace=False)]


def _spec(k, lengths, seed, avoid=()):
    return list(zip(_spread(k, len(lengths), seed, avoid), lengths))


def _halves(half, lengths, seed, k=K):
    """the profile on the left half, the right half, or both (other buckets, another permutation)"""
    out = {}
    if half in ("left", "both"):
        out["left"] = _spec(k, lengths, seed)
    if half in ("right", "both"):
        out["right"] = _spec(k, lengths, seed + 1)
    return out


# ------------------------------------------------------------------------------------------------ I1
@pytest.mark.parametrize("k_i", [13, 11])
@pytest.mark.parametrize("types", ["random", "by_bucket"])
def test_i1_every_bucket_at_most_one_gate(ctx, k_i, types):
    g = 1 << k_i
    prof = gp.build(k_i, K, left=_spec(K, [1] * g, 1), right=_spec(K, [1] * g, 2), types=types, seed=k_i)
    assert prof.hist_left.max() == prof.hist_right.max() == 1 and int((prof.hist_left == 0).sum()) == (1 << K) - g
    counts = _run(ctx, prof, gp.FORM_ITEMS, gp.W_PATTERNS, seed=k_i)
    for half in range(2):     # items, groups, multi, long, groups of two and more steps, chunks
        assert counts[half, :6].tolist() == [8192, 128, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ I2
I2_LENGTHS = [n for n in LADDER for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _i2_filler(items_mod, singles_mod):
    """filler buckets of 17, 2 and 1 gates (the rest empty) that put the half's items at items_mod (mod 64) and its groups of at
    most one step at singles_mod (mod SINGLE_PER_LANE)"""
    free, rest = (1 << K) - len(I2_LENGTHS), (1 << 14) - sum(I2_LENGTHS)
    base = gp.plan_header(I2_LENGTHS + [1] * free)[0]          # every filler bucket of <= 16 gates is one item
    d = (items_mod - base) % 64                                # a bucket of 17 gates is two
    for a in range(max(0, rest - 16 * d - free), (rest - 17 * d) // 2 + 1):
        filler = [17] * d + [2] * a + [1] * (rest - 17 * d - 2 * a)
        hdr = gp.plan_header(I2_LENGTHS + filler + [0] * (free - len(filler)))
        if hdr[0] % 64 == items_mod and (hdr[1] - hdr[4]) % gp.SINGLE_PER_LANE == singles_mod:
            return tuple(filler)
    raise AssertionError("no filler with these residues")


@pytest.mark.parametrize("order", gp.ORDER_PATTERNS)
@pytest.mark.parametrize("types", gp.TYPE_PATTERNS)
@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("items_mod,singles_mod", [(1, 1), (63, 3)])
def test_i2_item_lengths_and_ragged_last_groups(ctx, items_mod, singles_mod, half, types, order):
    prof = gp.build(14, K, types=types, order=order, seed=items_mod, filler=list(_i2_filler(items_mod, singles_mod)),
                    **_halves(half, I2_LENGTHS, 20 + items_mod))
    counts = _run(ctx, prof, gp.FORM_ITEMS, gp.W_PATTERNS, seed=items_mod)
    for h in ([0] if half == "left" else [1] if half == "right" else [0, 1]):
        assert counts[h, 0] % 64 == items_mod and (int(counts[h, 1]) - int(counts[h, 4])) % gp.SINGLE_PER_LANE == singles_mod
        # buckets of two and more items: the named ones of 17 .. 49 gates and the filler's of 17
        assert counts[h, 2] == 3 * 6 + _i2_filler(items_mod, singles_mod).count(17) and counts[h, 3] == 0


# ------------------------------------------------------------------------------------------------ I3
I3_LENGTHS = [1008, 1009, 1024, 1025, 1040, 1041] + [int(n) for n in np.linspace(17, 1000, 20)]


def _i3(half, types="random", order="shuffled", seed=3):
    return gp.build(16, K, types=types, order=order, seed=seed, **_halves(half, I3_LENGTHS, 30))


def _assert_i3_counts(counts, h):
    # 1008, 1009, 1024 gates: 63, 64, 64 items; 1025, 1040, 1041: 65, 65, 66 items, a chunk each
    assert counts[h, 2] == 3 + 20 and counts[h, 3] == 3 and counts[h, 5] == 3


@pytest.mark.parametrize("order", gp.ORDER_PATTERNS)
@pytest.mark.parametrize("types", gp.TYPE_PATTERNS)
@pytest.mark.parametrize("half", HALVES)
def test_i3_lane_buckets_and_wave_buckets_in_one_half(ctx, half, types, order):
    prof = _i3(half, types, order)
    assert gp.items_per_bucket([1008, 1009, 1024, 1025, 1040, 1041]).tolist() == [63, 64, 64, 65, 65, 66]
    counts = _run(ctx, prof, gp.FORM_ITEMS, gp.W_PATTERNS, seed=3)
    for h in ([0] if half == "left" else [1] if half == "right" else [0, 1]):
        _assert_i3_counts(counts, h)


# ------------------------------------------------------------------------------------------------ I4 .. I7
I4_LENGTHS = [16368, 16384, 16385, 32768, 32769] + [int(n) for n in np.linspace(17, 1000, 10)]


def _i4(half, types="random", seed=4):
    return gp.build(18, K, types=types, seed=seed, **_halves(half, I4_LENGTHS, 40))


@pytest.mark.parametrize("half,types,w_names", [("right", "by_bucket", ("r_minus_1", "random")), ("both", "random", ("one_hot", "mont_r_minus_1"))])
def test_i4_one_chunk_two_chunks_three_chunks(ctx, half, types, w_names):
    prof = _i4(half, types)
    assert gp.items_per_bucket(I4_LENGTHS[:5]).tolist() == [1023, 1024, 1025, 2048, 2049]
    counts = _run(ctx, prof, gp.FORM_ITEMS, w_names, seed=4)
    for h in ([1] if half == "right" else [0, 1]):
        hist = prof.hist_left if h == 0 else prof.hist_right
        per = gp.items_per_bucket(hist)
        assert (per == 1024).sum() == 1 and (per == 1025).sum() == 1          # one chunk | two chunks
        assert counts[h, 3] == 5 and counts[h, 5] == 1 + 1 + 2 + 2 + 3 and counts[h, 2] >= 10


I5_LENGTHS = [(1 << 20) - 16, (1 << 20) + 1, 3 << 19] + [int(n) for n in np.linspace(17, 1000, 10)]


@pytest.mark.parametrize("half,types,w_name", [("left", "by_bucket", "r_minus_1"), ("right", "random", "random")])
def test_i5_more_than_64_chunks_in_one_bucket(ctx, half, types, w_name):
    prof = gp.build(22, K, types=types, seed=5, **_halves(half, I5_LENGTHS, 50))
    counts = _run(ctx, prof, gp.FORM_ITEMS, (w_name,), seed=5)
    h = 0 if half == "left" else 1
    per = gp.items_per_bucket(prof.hist_left if h == 0 else prof.hist_right)
    chunks = sorted((-(-per[per > gp.LONG_ITEMS] // gp.CHUNK_ITEMS)).tolist())
    assert chunks == [64, 65, 96] and counts[h, 3] == 3 and counts[h, 5] == 64 + 65 + 96 and counts[h, 2] > 0


def test_i6_a_thousand_chunks_of_two_chunk_buckets(ctx):
    lengths = [16385 + (i % 16) for i in range(700)]
    prof = gp.build(24, K, types="by_bucket", seed=6, left=_spec(K, lengths, 60))
    counts = _run(ctx, prof, gp.FORM_ITEMS, ("r_minus_1",), seed=6)
    assert counts[0, 3] == 700 and counts[0, 5] == 1400 and counts[0, 5] >= 1024       # the chunk grid is capped from 1024 chunks on
    assert counts[1, 3] == counts[1, 5] == 1 << K      # (the right half: 2^11 gates in every bucket, a chunk each)


@pytest.mark.parametrize("k_i", [16, 21])
@pytest.mark.parametrize("types,w_name", [("by_bucket", "r_minus_1"), ("random", "random")])
def test_i7_one_bucket_holds_the_layer_on_both_halves(ctx, k_i, types, w_name):
    g = 1 << k_i
    prof = gp.build(k_i, K, left=[(5, g)], right=[(8191, g)], types=types, seed=7)
    assert (prof.left == 5).all() and (prof.right == 8191).all()
    counts = _run(ctx, prof, gp.FORM_ITEMS, (w_name,), seed=k_i)
    for h in range(2):
        assert counts[h, 2] == 0 and counts[h, 3] == 1 and counts[h, 5] == g // (gp.ITEM_MAX * gp.CHUNK_ITEMS)


# ------------------------------------------------------------------------------------------------ whole proofs
def _random_layer(k_i, k, seed):
    rng = np.random.default_rng(seed)
    g = 1 << k_i
    return rng.integers(0, 2, g, dtype=np.uint8), rng.integers(0, 1 << k, g, dtype=np.uint32), rng.integers(0, 1 << k, g, dtype=np.uint32)


def _witnesses(n, k, seed):
    return np.ascontiguousarray(np.stack([gp.w_pattern("random", k, seed=seed + b) for b in range(n)]))


def _check_proofs(arrs, layers, ks, witnesses):
    sc, sl, sr, q, ql, z, rr, dco, ico = arrs
    for b in range(witnesses.shape[0]):
        ref = cdense.prove_raw(layers, witnesses[b])
        ro = qo = 0
        zo = ks[0]
        for i in range(len(layers)):
            k = ks[i + 1]
            assert np.array_equal(sc[b, ro:ro + 2 * k], ref["C"][i]), (b, i)
            assert np.array_equal(sl[b, ro:ro + 2 * k], ref["L"][i]), (b, i)
            assert np.array_equal(sr[b, ro:ro + 2 * k], ref["R"][i]), (b, i)
            assert int(ql[b, i]) == ref["q_len"][i] and np.array_equal(q[b, qo:qo + k + 1], ref["q"][i]), (b, i)
            assert np.array_equal(z[b, zo:zo + k], ref["z"][i + 1]), (b, i)
            ro += 2 * k
            qo += k + 1
            zo += k
        assert np.array_equal(rr[b], ref["r"])
        assert np.array_equal(dco[b], cdense.mobius_raw(ref["values"][0], ks[0]))
        assert np.array_equal(ico[b], cdense.mobius_raw(ref["values"][-1], ks[-1]))


@pytest.mark.parametrize("case", ["I3", "I4"])
def test_batch_of_three_witnesses_through_a_profile_layer(ctx, case):
    prof = _i3("both", "by_bucket") if case == "I3" else _i4("both", "by_bucket")
    counts = gp.assert_plan(ctx, prof, gp.FORM_ITEMS)
    assert counts[0, 2] > 0 and counts[0, 3] > 0 and counts[1, 2] > 0 and counts[1, 3] > 0
    ks = [prof.k_i, K, 8]
    layers = [prof.arrays(), _random_layer(K, 8, 77)]
    circuit = GKRCircuit([Layer(ks[i], *layers[i]) for i in range(2)], ks[-1])
    wit = _witnesses(3, 8, 700)
    _check_proofs(ctx.prove_batch_raw(circuit, wit, all_arrays=True), layers, ks, wit)


def test_lockstep_group_whose_members_differ_in_having_long_buckets(ctx):
    """ks = [12, 13] for every member: I1 (every bucket at most one gate: nothing to combine), I3's lengths scaled to 2^12 gates
    (one bucket of 2049 gates: 129 items, a long bucket; buckets of 17 .. 100: a lane each) and a uniform draw."""
    ks = [12, K]
    g = 1 << 12
    scaled = [2049] + [int(n) for n in np.linspace(17, 100, 12)]
    profs = [gp.build(12, K, left=_spec(K, [1] * g, 11), right=_spec(K, [1] * g, 12), seed=1),
             gp.build(12, K, left=_spec(K, scaled, 13), right=_spec(K, scaled, 14), types="by_bucket", seed=2),
             gp.build(12, K, left=_spec(K, scaled, 15), seed=3),
             gp.build(12, K, filler="random", seed=4)]
    want_counts = [gp.assert_plan(ctx, p, gp.FORM_ITEMS) for p in profs]
    assert want_counts[0][:, 2:6].tolist() == [[0, 0, 0, 0]] * 2
    assert want_counts[1][:, 2:6].tolist() == [[12, 1, want_counts[1][0, 4], 1]] * 2 and want_counts[2][1, 3] == 0
    assert want_counts[3][0, 3] == 0 and want_counts[3][1, 3] == 0
    work, raw = [], []
    for j, p in enumerate(profs):
        raw.append([p.arrays()])
        work.append((GKRCircuit([Layer(12, *p.arrays())], K), _witnesses(2 if j == 1 else 1, K, 800 + 10 * j)))
    alone = [[a.copy() for a in ctx.prove_batch_raw(c, x, all_arrays=True)] for c, x in work]
    for j, (c, x) in enumerate(work):
        _check_proofs(alone[j], raw[j], ks, x)
    for threads in (0, 2):
        got = ctx.prove_many_raw(ctx.prepare_many(work), threads)
        for j, (gj, wj) in enumerate(zip(got, alone)):
            for n, (a, b) in enumerate(zip(gj, wj)):
                assert np.array_equal(a, b), (threads, "item", j, "array", n)


def test_i3_split_by_gates_over_three_ranks(ctx):
    """unaligned spans (2^16 gates over three ranks) and gate_base != 0: every rank's own item plan over its share"""
    prof = _i3("both", "by_bucket")
    counts = gp.assert_plan(ctx, prof, gp.FORM_ITEMS)
    _assert_i3_counts(counts, 0)
    _assert_i3_counts(counts, 1)
    z, W = gp.z_point(16, 9), gp.w_pattern("random", K, seed=9)
    want = cdense.sumcheck_layer_lin_raw(16, K, *prof.arrays(), z, W)
    got = parallel.prove_sumcheck_opt_logical_gates_dev(0, Layer(16, *prof.arrays()), K, z, W, 3)
    assert len(got) == 3 and all(_same(g, want) for g in got)


# ------------------------------------------------------------------------------------------------ bucket kernels
BUCKET_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513]


@pytest.mark.parametrize("order", gp.ORDER_PATTERNS)
@pytest.mark.parametrize("types", gp.TYPE_PATTERNS)
def test_bucket_kernels_block_size_edges(ctx, types, order):
    prof = gp.build(12, 8, types=types, order=order, seed=8, left=_spec(8, BUCKET_LENGTHS, 80), right=_spec(8, BUCKET_LENGTHS, 81))
    counts = _run(ctx, prof, gp.FORM_BUCKETS, gp.W_PATTERNS, seed=8)
    assert not counts.any()


@pytest.mark.parametrize("sort_global", [0, 1])
@pytest.mark.parametrize("order", gp.ORDER_PATTERNS + ("one_bucket",))
def test_bucket_kernels_sorts_and_gate_orders(ctx, order, sort_global):
    """2^16 gates over 2^12 values: the LDS-privatised sort (default) and the global-atomic sort (gate_sort_global), whose wave
    leaders meet runs of 64 equal operands, two alternating buckets and three interleaved ones"""
    g = 1 << 16
    if order == "one_bucket":
        prof = gp.build(16, 12, left=[(77, g)], right=[(4095, g)], types="random", seed=9)
    else:
        lengths = BUCKET_LENGTHS + [(1 << 14) + 1, 4096, 64 * 3, 64 * 2]
        prof = gp.build(16, 12, order=order, types="by_bucket", seed=9, left=_spec(12, lengths, 90), right=_spec(12, lengths, 91))
    ctx.set_option("gate_sort_global", sort_global)
    try:
        _run(ctx, prof, gp.FORM_BUCKETS, ("random", "r_minus_1"), seed=9)
    finally:
        ctx.set_option("gate_sort_global", 0)


@pytest.mark.parametrize("types", ["random", "all_add", "all_mult"])
def test_bucket_kernels_two_buckets(ctx, types):
    g = 1 << 16
    prof = gp.build(16, 1, left=[(0, g - 1), (1, 1)], right=[(1, g // 2 + 1), (0, g // 2 - 1)], types=types, order="interleave2", seed=10)
    _run(ctx, prof, gp.FORM_BUCKETS, ("random", "mont_r_minus_1"), seed=10)


# ------------------------------------------------------------------------------------------------ segment form
SEG_LENGTHS = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97)


def _segment_profile(k_i, k, mean_log2, whole_layer, types, seed):
    shift, runs, _ = gp.segment_geometry(k_i, k, mean_log2)
    nb, run_len = 1 << k, 1 << shift
    if whole_layer:
        return gp.build(k_i, k, left=[(3, run, run_len) for run in range(runs)], right=[(nb - 1, run, run_len) for run in range(runs)],
                        shift=shift, types=types, seed=seed)
    spec = {}
    for name, first in (("left", 1), ("right", nb // 2)):
        per_bucket = -(-len(SEG_LENGTHS) // runs) + 1
        ladder = [(first + j, run, SEG_LENGTHS[(run + j * runs) % len(SEG_LENGTHS)]) for j in range(per_bucket) for run in range(runs)]
        one_run = first + per_bucket                       # a bucket whose gates lie in one run
        every_run = one_run + 1                            # a bucket with one gate in every run
        pure = [(every_run + 1 + j, j % runs, gp.SEG_CAP) for j in range(4)]   # four items of 32 gates: their types are set below
        spec[name] = (ladder + [(one_run, run, 500 if run == runs - 1 else 0) for run in range(runs)] + [(every_run, run, 1) for run in range(runs)] +
                      [(b, run, n if run == at else 0) for b, at, n in pure for run in range(runs)])
    prof = gp.build(k_i, k, shift=shift, types=types, seed=seed, **spec)
    # items that are all-add, all-mult, 31 add + 1 mult, 1 add + 31 mult (the add gates are packed first: one accumulator
    # exchange at the first mult gate, at entry 0, 31, 1 or never)
    for arr, first in ((prof.left, 1), (prof.right, nb // 2)):
        base = first + (-(-len(SEG_LENGTHS) // runs) + 1) + 2
        for j, n_mult in enumerate((0, gp.SEG_CAP, 1, gp.SEG_CAP - 1)):
            at = np.flatnonzero(arr == base + j)
            assert len(at) == gp.SEG_CAP and len(set((at >> shift).tolist())) == 1
            prof.gate_type[at] = 0
            prof.gate_type[at[len(at) - n_mult:]] = 1
    return prof


@pytest.mark.parametrize("k_i,k,option,whole_layer,types", [
    (16, 8, None, False, "random"), (16, 8, None, True, "random"), (16, 8, None, False, "all_add"),
    (17, 9, None, False, "by_bucket"), (17, 9, ("gate_segments_no_lds", 1), False, "random"), (17, 9, None, False, "all_mult"),
    (18, 12, None, False, "random"), (18, 12, ("gate_segment_log2", 2), False, "by_bucket"), (18, 12, None, True, "by_bucket")])
def test_segment_form_item_edges(ctx, k_i, k, option, whole_layer, types):
    mean_log2 = option[1] if option and option[0] == "gate_segment_log2" else 4
    prof = _segment_profile(k_i, k, mean_log2, whole_layer, types, seed=k_i)
    ctx.set_option("gate_segments_min_log2", 16)
    if option:
        ctx.set_option(*option)
    try:
        counts = _run(ctx, prof, gp.FORM_SEGMENTS, ("random", "r_minus_1"), seed=k_i, mean_log2=mean_log2)
        assert counts[0, :3].tolist() == list(gp.segment_geometry(k_i, k, mean_log2))
        if whole_layer:
            assert counts[0, 3] == counts[1, 3] == (1 << k_i) // gp.SEG_CAP
    finally:
        ctx.set_option("gate_segments_min_log2", 22)
        if option:
            ctx.set_option(option[0], 0)


# ------------------------------------------------------------------------------------------------ the devtest itself
def test_gate_plan_devtest_checks_its_arguments(ctx):
    lib = N.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    gt, l, r = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    form, counts = np.zeros(1, dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    args = [p(gt), p(l), p(r), p(form), p(counts)]
    for i in range(5):
        bad = list(args)
        bad[i] = None
        assert lib.gkr_devtest_gate_plan(ctx._h, 2, 1, *bad) == N.GKR_ERR_INVALID, i
    for k_i, k in ((-1, 1), (2, 0), (2, -1), (2, 25), (29, 1)):
        assert lib.gkr_devtest_gate_plan(ctx._h, k_i, k, *args) == N.GKR_ERR_INVALID, (k_i, k)
    assert lib.gkr_devtest_gate_plan(ctx._h, 2, 1, *args) == 0 and form[0] == gp.FORM_BUCKETS and not counts.any()
    l[3] = 2                                                  # an operand out of range
    with pytest.raises(GkrError):
        ctx._check(lib.gkr_devtest_gate_plan(ctx._h, 2, 1, *args))
    l[3] = 0
    # and the context keeps working
    prof = gp.build(13, K, filler="random", seed=1)
    assert gp.device_plan(ctx, prof)[0] == gp.FORM_ITEMS

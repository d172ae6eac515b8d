"""The judge of tests/test_gpu_gate_profiles.py on the lists it judges there.  cdense.sumcheck_layer_lin_raw (the C oracle's
linear-time layer prover) has so far met uniform gate lists; here it is held to the dense C prover (k <= 6) and to the
pure-Python dense prover (k <= 3) on scaled-down versions of every profile family the GPU file runs: one bucket holding the
layer, every bucket one gate, all buckets empty but two, ladders of bucket lengths, runs and interleaved gate orders, all-add
and all-mult layers, and the four W patterns.  The same file holds the builder (tests/gate_profiles.py) to exactness and its
integer model of the item plan and the segment form to hand-worked histograms.  CPU only."""

import numpy as np
import pytest

import gate_profiles as gp
from oracle import cdense, dense
from oracle.field import P


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _families(k_i, k):
    """scaled-down profiles at (k_i, k), k_i >= k + 2: name -> build() arguments"""
    g, nb = 1 << k_i, 1 << k
    ladder = [n for n in (0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 49) if n <= g // 8][:nb - 1]
    lad = [((5 * i + 1) % nb, n) for i, n in enumerate(ladder)]      # (nb is a power of two: distinct buckets)
    fam = {
        "ladder_left": dict(left=lad),
        "ladder_right": dict(right=lad),
        "ladder_both": dict(left=lad, right=[(nb - 1 - b, n) for b, n in lad]),
        "one_bucket_holds_the_layer": dict(left=[(5 % nb, g)], right=[(nb - 1, g)]),
        "all_empty_but_two": dict(left=[(0, g - 3), (nb - 1, 3)], right=[(1, g // 2), (nb - 2, g // 2)]),
        "heavy_and_medium": dict(left=[(1, g // 2 + 1), (2, g // 8), (3, 17 % g)], right=[(0, 5 * g // 8)]),
        "segments": dict(left=[(1, run, n) for run, n in enumerate((0, 1, (g >> 2) - 1, 3))],
                         right=[(2, run, 1) for run in range(4)], shift=k_i - 2),
    }
    return fam


@pytest.mark.parametrize("types", gp.TYPE_PATTERNS + ("by_bucket_edges",))
@pytest.mark.parametrize("order", gp.ORDER_PATTERNS)
def test_linear_oracle_equals_dense_c_on_scaled_down_profiles(types, order):
    for k_i, k in ((10, 6), (9, 4), (7, 5)):
        for j, (name, args) in enumerate(_families(k_i, k).items()):
            prof = gp.build(k_i, k, types=types, order=order, seed=31 * k_i + j, **args)
            z = gp.z_point(k_i, j)
            for wp in gp.W_PATTERNS:
                W = gp.w_pattern(wp, k, seed=j)
                want = cdense.sumcheck_layer_raw(k_i, k, *prof.arrays(), z, W)
                assert _same(cdense.sumcheck_layer_lin_raw(k_i, k, *prof.arrays(), z, W), want), (k_i, k, name, wp)


@pytest.mark.parametrize("k_i,k", [(6, 6), (4, 6), (5, 5), (3, 5)])
def test_linear_oracle_on_permutations_every_bucket_at_most_one_gate(k_i, k):
    """every bucket one gate on both halves (k_i = k), or most buckets empty (k_i < k)"""
    rng = np.random.default_rng(k_i * 8 + k)
    g = 1 << k_i
    for types in ("random", "all_add", "all_mult"):
        l = rng.permutation(1 << k)[:g].astype(np.uint32)
        r = rng.permutation(1 << k)[:g].astype(np.uint32)
        gt = {"random": rng.integers(0, 2, g, dtype=np.uint8), "all_add": np.zeros(g, np.uint8), "all_mult": np.ones(g, np.uint8)}[types]
        z = gp.z_point(k_i, k)
        for wp in gp.W_PATTERNS:
            W = gp.w_pattern(wp, k, seed=k_i)
            assert _same(cdense.sumcheck_layer_lin_raw(k_i, k, gt, l, r, z, W), cdense.sumcheck_layer_raw(k_i, k, gt, l, r, z, W)), (types, wp)


@pytest.mark.parametrize("types", ["random", "all_add", "all_mult", "by_bucket"])
def test_linear_oracle_equals_python_dense_on_scaled_down_profiles(types):
    for k_i, k in ((5, 3), (4, 2), (3, 3)):
        g, nb = 1 << k_i, 1 << k
        specs = [dict(left=[(1, g)], right=[(nb - 1, g)]),
                 dict(left=[(0, g - 1), (nb - 1, 1)], right=[(1, g // 2), (2, g // 2)]),
                 dict(left=[(0, 0), (1, 1), (2, 2)], right=[(3, 0), (2, 1)])]
        if k_i == k:
            specs.append(dict(left=[(b, 1) for b in range(nb)], right=[(nb - 1 - b, 1) for b in range(nb)]))
        for j, args in enumerate(specs):
            for order in ("shuffled", "interleave2"):
                prof = gp.build(k_i, k, types=types, order=order, seed=j, **args)
                z = cdense.from_limbs(gp.z_point(k_i, j))
                for wp in gp.W_PATTERNS:
                    W = cdense.from_limbs(gp.w_pattern(wp, k, seed=j))
                    gt, l, r = (a.tolist() for a in prof.arrays())
                    assert cdense.sumcheck_layer_lin(k_i, k, gt, l, r, z, W) == dense.sumcheck_layer(k_i, k, gt, l, r, z, W), (k_i, k, j, order, wp)


# ------------------------------------------------------------------------------------------------ the builder
def test_builder_gives_the_named_buckets_their_exact_lengths():
    k_i, k = 12, 7
    left = [(3, 0), (9, 1), (17, 63), (18, 64), (19, 65), (100, 1000)]
    right = [(0, 2049), (127, 16)]
    for order in gp.ORDER_PATTERNS:
        for filler in ("even", "random"):
            prof = gp.build(k_i, k, left=left, right=right, order=order, filler=filler, seed=3)
            assert len(prof.gate_type) == len(prof.left) == len(prof.right) == 1 << k_i
            assert prof.left.dtype == prof.right.dtype == np.uint32 and prof.gate_type.dtype == np.uint8
            assert prof.left.max() < 1 << k and prof.right.max() < 1 << k and set(prof.gate_type.tolist()) <= {0, 1}
            for spec, arr, hist in ((left, prof.left, prof.hist_left), (right, prof.right, prof.hist_right)):
                assert np.array_equal(hist, np.bincount(arr, minlength=1 << k)) and hist.sum() == 1 << k_i
                for b, n in spec:
                    assert hist[b] == n, (order, filler, b, n)
    # even filler: the remaining gates over the remaining buckets, lengths differing by at most one
    prof = gp.build(k_i, k, left=left, seed=1)
    rest = np.delete(prof.hist_left, [b for b, _ in left])
    assert rest.max() - rest.min() <= 1 and rest.sum() == (1 << k_i) - sum(n for _, n in left)
    # explicit filler lengths go to the first buckets that are not named
    prof = gp.build(6, 3, left=[(0, 10), (2, 4)], filler=[20, 0, 30], seed=1)
    assert prof.hist_left.tolist() == [10, 20, 4, 0, 30, 0, 0, 0]
    with pytest.raises(AssertionError):
        gp.build(6, 3, left=[(0, 10)], filler=[20, 30])                # does not add up
    with pytest.raises(AssertionError):
        gp.build(6, 3, left=[(0, 65)])                                 # more than the layer holds
    with pytest.raises(AssertionError):
        gp.build(6, 3, left=[(b, 1) for b in range(8)])                # gates left over and every bucket named


def test_builder_runs_gate_orders_and_types():
    k_i, k, shift = 10, 4, 8
    trip = [(1, 0, 0), (1, 1, 1), (1, 2, 33), (1, 3, 256), (2, 0, 31), (2, 2, 97)]
    prof = gp.build(k_i, k, left=trip, right=[(7, run, 1) for run in range(4)], shift=shift, seed=2)
    for b, run, n in trip:
        assert int((prof.left[run << shift:(run + 1) << shift] == b).sum()) == n
    for run in range(4):
        assert int((prof.right[run << shift:(run + 1) << shift] == 7).sum()) == 1
    assert gp.segment_items(prof.left, k, shift) == sum(-(-n // 32) for _, _, n in trip) + int(
        sum(-(-int(c) // 32) for run in range(4) for b, c in enumerate(np.bincount(prof.left[run << shift:(run + 1) << shift], minlength=16)) if b not in (1, 2)))
    # gate orders: runs of equal left operands; two and three buckets taking turns
    prof = gp.build(12, 3, left=[(b, 512) for b in range(8)], order="sorted_by_left")
    assert (np.diff(prof.left.astype(np.int64)) >= 0).all() and np.array_equal(prof.left[:512], np.zeros(512, np.uint32))
    for n, order in ((2, "interleave2"), (3, "interleave3")):
        prof = gp.build(12, 3, left=[(b, 512) for b in range(8)], right=[(b, 512) for b in range(8)], order=order)
        for arr in (prof.left, prof.right):
            assert (arr[:-n] == arr[n:]).mean() > 0.99 and (arr[:-1] != arr[1:]).all()
            assert len(set(arr[:n].tolist())) == n
    # types
    spec = [(3, 40), (5, 41), (6, 42), (9, 43)]
    assert not gp.build(10, 4, left=spec, types="all_add").gate_type.any()
    assert gp.build(10, 4, left=spec, types="all_mult").gate_type.all()
    prof = gp.build(10, 4, left=spec, types="by_bucket", seed=5)
    for i, (b, _) in enumerate(spec):
        assert set(prof.gate_type[prof.left == b].tolist()) == {i % 2}
    prof = gp.build(10, 4, left=spec, types="by_bucket_edges", seed=5)
    for i, (b, n) in enumerate(spec):
        t = prof.gate_type[prof.left == b]
        assert t[:-1].tolist() == [i & 1] * (n - 1) and int(t[-1]) == (i & 1) ^ (i >> 1)


def test_w_patterns():
    for name in gp.W_PATTERNS:
        vals = cdense.from_limbs(gp.w_pattern(name, 5, seed=2))
        assert len(vals) == 32 and all(0 <= v < P for v in vals)
    assert set(cdense.from_limbs(gp.w_pattern("r_minus_1", 3))) == {P - 1}
    x = cdense.from_limbs(gp.w_pattern("mont_r_minus_1", 3))[0]
    assert x * pow(2, 256, P) % P == P - 1 and x not in (0, 1, P - 1)
    assert sum(1 for v in cdense.from_limbs(gp.w_pattern("one_hot", 5, seed=2)) if v) == 1
    assert len(set(cdense.from_limbs(gp.w_pattern("random", 5, seed=2)))) == 32


# ------------------------------------------------------------------------------------------------ the model
def test_item_plan_model_on_hand_worked_histograms():
    # bucket of     0  1  16  17  1024  1025  16384  16385 gates
    # items         1  1   1   2    64    65   1024   1025      = 2183 -> 35 groups
    # kind          -  -   -   m     m     L      L      L      2 of 2 .. 64 items, 3 long
    # chunks                                1      1      2      = 4
    # items >= 2 g  0  0   1   1    64    64   1024   1024      = 2178 -> 35 groups of two and more steps
    assert gp.plan_header([0, 1, 16, 17, 1024, 1025, 16384, 16385]) == [2183, 35, 2, 3, 35, 4]
    assert gp.items_per_bucket([0, 1, 16, 17, 1024, 1025, 16384, 16385]).tolist() == [1, 1, 1, 2, 64, 65, 1024, 1025]
    # every bucket one gate: 8192 items in 128 groups, nothing to combine, no group of two steps
    assert gp.plan_header([1] * 8192) == [8192, 128, 0, 0, 0, 0]
    # three quarters of the buckets empty: the same (an empty bucket is an item of no gates)
    assert gp.plan_header(([1] + [0] * 3) * 2048) == [8192, 128, 0, 0, 0, 0]
    # 65 items of 2 gates among single gates: two groups of two steps (64 + 1), 3 groups in all (130 items)
    assert gp.plan_header([2] * 65 + [1] * 65) == [130, 3, 0, 0, 2, 0]
    # one bucket of 2^20 + 1 gates: 65537 items, 65 chunks (64 full and one of one item)
    assert gp.plan_header([(1 << 20) + 1, 0]) == [65538, 1025, 0, 1, 1024, 65]
    assert gp.plan_header([(1 << 20) - 16]) == [65535, 1024, 0, 1, 1024, 64]


def test_segment_model_on_hand_worked_lists():
    # (16, 8): 4 sort blocks of 2^14 gates, shift max(8 + 4, 14) = 14: a run per block
    assert gp.segment_geometry(16, 8) == (14, 4, 1)
    assert gp.segment_geometry(17, 9) == (14, 8, 1)
    # (18, 12): 16 blocks; shift 12 + 4 = 16: four blocks per run, four runs; mean length 2^2: shift 14, a run per block
    assert gp.segment_geometry(18, 12) == (16, 4, 4)
    assert gp.segment_geometry(18, 12, mean_log2=2) == (14, 16, 1)
    assert gp.segment_geometry(22, 11) == (15, 128, 2)
    # two runs of 2^3 gates over four buckets: bucket 0 has 8 + 0, bucket 1 has 0 + 3, bucket 3 has 0 + 5 gates
    operand = np.array([0] * 8 + [1, 3, 1, 3, 3, 1, 3, 3])
    assert gp.segment_items(operand, 2, 3) == 3
    # one bucket with 33, 64, 65 and 0 gates in four runs of 2^7: 2 + 2 + 3 + 0 items; the other bucket 3 + 2 + 2 + 4
    operand = np.concatenate([np.r_[np.zeros(n, int), np.ones(128 - n, int)] for n in (33, 64, 65, 0)])
    assert gp.segment_items(operand, 1, 7) == 7 + 11

"""Gate lists built to sit ON the thresholds of the layer sumcheck's gate passes, and an integer model of what the list build
makes of them (gkr_devtest_gate_plan reports the build's own counts; every GPU case asserts them against the model first, so a
case that stops hitting its threshold fails instead of passing vacuously).

The three forms and their constants, as the kernels have them:
  * item plan (csrc/kernels_wide.hip, k_next >= 13): buckets cut into items of ITEM_MAX gates, 64 items per wave; groups of at
    most one step SINGLE_PER_LANE per lane; buckets of 2 .. LONG_ITEMS items a lane per bucket, longer ones a wave per chunk of
    CHUNK_ITEMS items;
  * bucket kernels (csrc/kernels.hip, k_next <= 12): a block per bucket;
  * segments (csrc/gate_seg.h): a bucket's gates inside one aligned run of 2^shift gate indices, cut into items of SEG_CAP gates.
tests/test_oracle_gate_profiles.py holds the builder and the model to hand-worked histograms."""

import ctypes
from dataclasses import dataclass

import numpy as np

from oracle.field import P

ITEM_MAX = 16
LONG_ITEMS = 64
CHUNK_ITEMS = 1024
SINGLE_PER_LANE = 4
SEG_CAP = 32
SORT_BLOCK_LOG2 = 14          # gates per block of the LDS-privatised sort (from 2^16 gates on, k_next <= 12)

TYPE_PATTERNS = ("random", "all_add", "all_mult", "by_bucket")
ORDER_PATTERNS = ("shuffled", "sorted_by_left", "interleave2", "interleave3")
W_PATTERNS = ("random", "r_minus_1", "mont_r_minus_1", "one_hot")
FORM_BUCKETS, FORM_ITEMS, FORM_SEGMENTS = 0, 1, 2


@dataclass
class Profile:
    k_i: int
    k: int
    gate_type: np.ndarray
    left: np.ndarray
    right: np.ndarray
    hist_left: np.ndarray     # gates per left-operand bucket, exact
    hist_right: np.ndarray

    def arrays(self):
        return self.gate_type, self.left, self.right


def _entries(spec, shift, k_i):
    """(bucket, length) pairs -> one run that is the whole layer; (bucket, run, length) triples -> runs of 2^shift gates"""
    spec = list(spec or ())
    if spec and len(spec[0]) == 3:
        assert shift is not None and all(len(e) == 3 for e in spec)
        return [(int(b), int(run), int(n)) for b, run, n in spec], shift
    assert all(len(e) == 2 for e in spec)
    return [(int(b), 0, int(n)) for b, n in spec], k_i


def _arrange(values, order, is_left, rng):
    if order == "shuffled" or (order == "sorted_by_left" and not is_left):
        return rng.permutation(values)
    s = np.sort(values) if is_left else np.sort(values)[::-1]
    if order == "sorted_by_left":
        return s
    n = {"interleave2": 2, "interleave3": 3}[order]
    out = np.empty_like(s)
    for j, part in enumerate(np.array_split(s, n)):      # consecutive gates take turns between n places of the sorted list
        out[j::n] = part
    return out


def _half(k_i, k, spec, shift, order, filler, is_left, rng):
    entries, shift = _entries(spec, shift, k_i)
    if not spec and not isinstance(filler, str):
        filler = "even"                                   # (explicit filler lengths belong to the halves that name buckets)
    nb, run_len, runs = 1 << k, 1 << shift, 1 << (k_i - shift)
    named = sorted({b for b, _, _ in entries})
    assert all(0 <= b < nb for b in named) and len({(b, run) for b, run, _ in entries}) == len(entries), "a bucket named twice"
    free = np.setdiff1d(np.arange(nb, dtype=np.uint32), np.array(named, dtype=np.uint32))
    out = np.empty(1 << k_i, dtype=np.uint32)
    for run in range(runs):
        mine = [(b, n) for b, rr, n in entries if rr == run]
        vals = [np.full(n, b, dtype=np.uint32) for b, n in mine]
        rest = run_len - sum(n for _, n in mine)
        assert rest >= 0, "the named buckets hold more gates than the run has"
        if rest:
            assert len(free), "gates left over and no filler bucket"
            if isinstance(filler, str) and filler == "even":
                lens = np.full(len(free), rest // len(free), dtype=np.int64)
                lens[:rest % len(free)] += 1
                vals.append(np.repeat(free, lens))
            elif isinstance(filler, str) and filler == "random":
                vals.append(free[rng.integers(0, len(free), rest)])
            else:                                         # explicit lengths of the first filler buckets
                lens = np.asarray(filler, dtype=np.int64)
                assert runs == 1 and len(lens) <= len(free) and int(lens.sum()) == rest, (len(lens), len(free), int(lens.sum()), rest)
                vals.append(np.repeat(free[:len(lens)], lens))
        out[run * run_len:(run + 1) * run_len] = _arrange(np.concatenate(vals), order, is_left, rng)
    return out, named


def build(k_i, k, left=None, right=None, types="random", order="shuffled", seed=0, filler="even", shift=None):
    """gate_type, left, right of exactly 2^k_i gates over 2^k values.  left / right: the named buckets of the half as (bucket,
    length) pairs, or (bucket, run, length) triples (the bucket's gates inside run `run` of 2^shift gate indices); the remaining
    gates go to the buckets the half does not name -- filler = "even" (spread evenly, the first ones one more), "random", or the
    lengths of the first filler buckets.  A half without a spec is filler only.
    types: TYPE_PATTERNS, or "by_bucket_edges" (named bucket i: all-add, all-mult, add with its last gate mult, mult with its last
    gate add, by i % 4).  order: ORDER_PATTERNS, applied inside every run."""
    rng = np.random.default_rng(seed)
    l, named_l = _half(k_i, k, left, shift, order, filler, True, rng)
    r, named_r = _half(k_i, k, right, shift, order, filler, False, rng)
    g = 1 << k_i
    if types == "all_add":
        gt = np.zeros(g, dtype=np.uint8)
    elif types == "all_mult":
        gt = np.ones(g, dtype=np.uint8)
    else:
        gt = rng.integers(0, 2, g, dtype=np.uint8)
        if types in ("by_bucket", "by_bucket_edges"):
            mod = 2 if types == "by_bucket" else 4
            for arr, named in ((r, named_r), (l, named_l)):      # (the left half's named buckets decide last)
                tab = np.full(1 << k, 255, dtype=np.uint8)
                for i, b in enumerate(named):
                    tab[b] = i % mod
                t = tab[arr]
                gt = np.where(t != 255, t & 1, gt).astype(np.uint8)
                for i, b in enumerate(named):
                    if i % mod >= 2:
                        at = np.flatnonzero(arr == b)
                        if len(at):
                            gt[at[-1]] ^= 1
        else:
            assert types == "random", types
    nb = 1 << k
    return Profile(k_i, k, gt, l, r, np.bincount(l, minlength=nb).astype(np.int64), np.bincount(r, minlength=nb).astype(np.int64))


# ------------------------------------------------------------------------------------------------ the model
def plan_header(hist):
    """Words 0 .. 5 of a half's item-plan header, from the half's histogram (k_plan_count / k_plan_items / k_plan_groups):
    items, groups of 64 items, buckets of 2 .. 64 items, buckets of more, groups of two and more steps, chunks."""
    h = np.asarray(hist, dtype=np.int64)
    per = np.maximum(1, -(-h // ITEM_MAX))                      # an empty bucket is one item of no gates
    items = int(per.sum())
    long_ = per > LONG_ITEMS
    steps2 = int((h // ITEM_MAX).sum() + ((h % ITEM_MAX) >= 2).sum())   # items of two and more gates: sorted by length, they come first
    return [items, -(-items // 64), int(((per >= 2) & ~long_).sum()), int(long_.sum()), -(-steps2 // 64),
            int((-(-per[long_] // CHUNK_ITEMS)).sum())]


def items_per_bucket(hist):
    h = np.asarray(hist, dtype=np.int64)
    return np.maximum(1, -(-h // ITEM_MAX))


def segment_geometry(k_i, k, mean_log2=4):
    """(shift, runs, m) of the segment form for a whole layer that takes it (seg_plan, csrc/kernels.hip)."""
    blocks = min(1024, 1 << max(0, k_i - SORT_BLOCK_LOG2))
    pb = k_i - (blocks.bit_length() - 1)
    shift = min(max(k + mean_log2, pb), k_i)
    m = 1 << (shift - pb)
    return shift, -(-blocks // m), m


def segment_items(operand, k, shift):
    """Items of one half of the segment form: the sum over (bucket, run) of ceil(len / SEG_CAP)."""
    operand = np.asarray(operand, dtype=np.int64)
    runs = len(operand) >> shift
    key = operand * runs + (np.arange(len(operand), dtype=np.int64) >> shift)
    seg = np.bincount(key, minlength=runs << k)
    return int((-(-seg // SEG_CAP)).sum())


def expected_counts(prof, form, shift=None, mean_log2=4):
    """The 2 x 8 words gkr_devtest_gate_plan reports for the profile in the given form."""
    out = np.zeros((2, 8), dtype=np.uint32)
    if form == FORM_ITEMS:
        out[0, :6] = plan_header(prof.hist_left)
        out[1, :6] = plan_header(prof.hist_right)
    elif form == FORM_SEGMENTS:
        sh, runs, m = segment_geometry(prof.k_i, prof.k, mean_log2)
        assert shift is None or shift == sh
        out[0, :4] = [sh, runs, m, segment_items(prof.left, prof.k, sh)]
        out[1, :4] = [sh, runs, m, segment_items(prof.right, prof.k, sh)]
    return out


def device_plan(ctx, prof):
    """gkr_devtest_gate_plan -> (form, counts[2][8]): what the production list build makes of the profile under ctx's options."""
    from gkr_amd import _native as N
    gt = np.ascontiguousarray(prof.gate_type, dtype=np.uint8)
    l = np.ascontiguousarray(prof.left, dtype=np.uint32)
    r = np.ascontiguousarray(prof.right, dtype=np.uint32)
    form = ctypes.c_uint32(99)
    counts = np.zeros((2, 8), dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ctx._check(N.lib().gkr_devtest_gate_plan(ctx._h, prof.k_i, prof.k, p(gt), p(l), p(r), ctypes.byref(form), p(counts)))
    return int(form.value), counts


def assert_plan(ctx, prof, form, mean_log2=4):
    """the devtest's form and counts against the model; returns the model's counts"""
    got_form, got = device_plan(ctx, prof)
    want = expected_counts(prof, form, mean_log2=mean_log2)
    assert got_form == form, (got_form, form)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return want


# ------------------------------------------------------------------------------------------------ W
R_MINUS_1 = P - 1
MONT_R_MINUS_1 = (-pow(2, -256, P)) % P       # x with x * 2^256 = r - 1 (mod r): the Montgomery image the kernels hold is r - 1


def _limbs(x):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def w_pattern(name, k, seed=0):
    """2^k canonical values as (2^k, 4) uint64 limbs."""
    n = 1 << k
    if name == "random":
        a = np.random.default_rng(seed).integers(0, 1 << 63, (n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64((1 << 61) - 1)
        return a
    if name in ("r_minus_1", "mont_r_minus_1"):
        return np.ascontiguousarray(np.tile(np.array(_limbs(R_MINUS_1 if name == "r_minus_1" else MONT_R_MINUS_1), dtype=np.uint64), (n, 1)))
    assert name == "one_hot", name
    a = np.zeros((n, 4), dtype=np.uint64)
    a[(5 + 3 * seed) % n] = np.array(_limbs(1 + (seed % 7)), dtype=np.uint64)
    return a


def z_point(k_i, seed=0):
    a = np.random.default_rng(1000 + seed).integers(0, 1 << 63, (k_i, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)
    return a

"""Pass 0 of the plain sumcheck as a pipelined read (csrc/kernels.hip k_mle_sub_sums_stream, option pass0_stream = 2): a wave per
one or two partials, 16-byte pieces per lane, half-entry sums joined once per partial, the x_n test across a quad of lanes.
Streaming launches take it (nothing published from the last block, chunks of whole 256 entries, whole blocks of waves) -- eight
loads per lane and a partial per wave, or sixteen and two where the launch has at least 24 576 partials of whole 512 entries;
every other launch keeps k_mle_sub_sums.  The partials are the same integers, so every case is checked byte for byte against the C oracle
(cdense.sumcheck_mle_raw), or against pass0_stream = 1 where the oracle would take too long.  A case that names the launch it means to
reach first asserts it on the context's plan (tests/mle_plan.py pin: the library's own launch plan against tests/mle_shapes.py)."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import mle_plan as mp
import mle_shapes as ms
from gkr_amd import Context
from oracle import cdense
from oracle.field import P

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LOW = (1 << 128) - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    c.set_option("pass0_stream", 2)
    yield c
    c.close()


def _limbs(values):
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@functools.lru_cache(maxsize=None)
def _oracle_of_seed(n, seed):
    """The oracle's transcript of fill_table(2^n, seed): computed once, shared by the cases that use the table."""
    return cdense.sumcheck_mle_raw(cdense.fill_table(1 << n, seed), n)


def _batch_of_seeds(ctx, n, seeds):
    count = 1 << n
    d = ctx.alloc(len(seeds) * count * 32)
    try:
        for b, seed in enumerate(seeds):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, seed)
        return ctx.sumcheck_mle_batch_device(d, n, len(seeds))
    finally:
        ctx.free(d)


@pytest.mark.parametrize("levels", [2, 1])
@pytest.mark.parametrize("n,batch", [(18, 1), (18, 3), (19, 3), (20, 1), (20, 3)])
def test_sizes_match_oracle(ctx, n, batch, levels):
    """Chunks of 256, 512 and 1024 entries ahead of the two-level first fold (one, two and four rounds of eight loads per
    partial; n = 18 is the smallest case of the kernel; a lone 2^20 fills the chip with 2048 blocks of 512).  first_fold_levels = 1
    gives the passes BEHIND pass 0 another form; pass 0 itself has the same blocks at these sizes, as the plan shows (few tables: the
    chip's 2048 blocks decide, not the sub-blocks) -- eight tables of 2^18, where one level takes 256 blocks and two take 1024, are
    tests/test_gpu_mle_plan.py's cases one-level-256-blocks-n18-b8 and two-level-1024-blocks-n18-b8."""
    seeds = [22000 + 97 * n + b for b in range(batch)]
    chunk = {(18, 1): 256, (18, 3): 256, (19, 3): 512, (20, 1): 512, (20, 3): 1024}[(n, batch)]
    ctx.set_option("first_fold_levels", levels)
    try:
        rows = mp.pin(ctx, n, batch, kind=ms.STREAM_8_1, nblk=(1 << n) // chunk, chunk=chunk, publisher=ms.PUB_REDUCE)
        assert rows[1]["kind"] == (ms.FINE_SUMS if levels == 2 else ms.FOLD_MFMA)
        C, L, R = _batch_of_seeds(ctx, n, seeds)
    finally:
        ctx.set_option("first_fold_levels", 0)
    for b, seed in enumerate(seeds):
        assert _same((C[b], L[b], R[b]), _oracle_of_seed(n, seed)), (n, b, levels)


@pytest.mark.parametrize("n", [19, 20])
def test_launches_of_many_partials_match_oracle(ctx, n):
    """The kernel's deeper instance (sixteen loads per lane, TWO partials per wave) takes launches of at least 24 576 partials
    (kernels.h kMlePass0DeepMinPartials).  A batch of 24 is cut into two groups of 12 by the default schedule, so the groups are
    set to 24 here: ONE pass-0 launch of 24 tables x 1024 partials.  n = 19: one round of loads per partial, a partial ends in
    every round of the loop; n = 20: two.  Wave 137 of a table sums partials 274 and 275.  Beside p - 1 throughout (every half
    sum carries) and a table that does not depend on x_n, that table with ONE odd entry changed: in the first and in the last
    pair of the even partial, in the first and in the last pair of the odd one (both sides of the boundary inside the wave, and
    the wave's last quad), and in the table's last pair.  A table that is zero outside partial 274: a half sum carried over the
    boundary would show in partial 275's fine sum (rounds 6 - 10)."""
    count, batch = 1 << n, 24
    chunk = count // 1024
    seeds = [22100 + 97 * n + b for b in range(batch)]
    base = cdense.fill_table(count, seeds[1])
    flat = np.ascontiguousarray(base[np.arange(count) >> 1])
    special = {0: np.repeat(_limbs([P - 1]), count, axis=0), 1: flat}
    odd_entries = [274 * chunk + 1, 275 * chunk - 1, 275 * chunk + 1, 276 * chunk - 1, count - 1]
    for k, e in enumerate(odd_entries):
        t = flat.copy()
        t[e, (k % 4)] ^= np.uint64(1 << (3 + 32 * (k % 2)))
        special[2 + k] = t
    lone = np.zeros((count, 4), dtype=np.uint64)
    lone[274 * chunk:275 * chunk] = base[274 * chunk:275 * chunk]
    special[7] = lone
    assert mp.context_plan(ctx, n, batch)[0][3] == 2   # (the default schedule: two groups)
    ctx.set_option("group_size", batch)
    d = ctx.alloc(batch * count * 32)
    try:
        mp.pin(ctx, n, batch, kind=ms.STREAM_16_2, nblk=1024, chunk=chunk, nb=batch, publisher=ms.PUB_REDUCE)
        for b, seed in enumerate(seeds):
            at = ctypes.c_void_p(d.value + b * count * 32)
            if b in special:
                ctx.upload(at, special[b])
            else:
                ctx.fill_table(at, count, seed)
        C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
    finally:
        ctx.free(d)
        ctx.set_option("group_size", 0)
    for b, seed in enumerate(seeds):
        want = cdense.sumcheck_mle_raw(special[b], n) if b in special else _oracle_of_seed(n, seed)
        assert _same((C[b], L[b], R[b]), want), (n, b)
    assert int(L[1][-1]) == 1 and [int(L[2 + k][-1]) for k in range(len(odd_entries))] == [2] * len(odd_entries)


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [13, 14, 15, 16, 17])
def test_small_tables_same_bytes_with_either_kernel(ctx, n, batch):
    """Around the launcher's conditions (launches that publish from their last block, chunks of 256 entries in few blocks): the
    same bytes with options 1 and 2, whichever kernel each launch takes, and the oracle's."""
    seeds = [22500 + 31 * n + b for b in range(batch)]
    fused = n == 13 or (batch == 1 and n <= 15)   # (32 blocks per table at n = 13; 64 and 128 blocks of a lone table)
    mp.pin(ctx, n, batch, kind=ms.SUB_SUMS if fused else ms.STREAM_8_1, chunk=256, publisher=ms.PUB_FUSED if fused else ms.PUB_REDUCE)
    got = _batch_of_seeds(ctx, n, seeds)
    ctx.set_option("pass0_stream", 1)
    try:
        mp.pin(ctx, n, batch, kind=ms.SUB_SUMS, chunk=256)
        want = _batch_of_seeds(ctx, n, seeds)
    finally:
        ctx.set_option("pass0_stream", 2)
    assert _same(got, want)
    for b, seed in enumerate(seeds):
        assert _same((got[0][b], got[1][b], got[2][b]), _oracle_of_seed(n, seed)), (n, b)


@pytest.mark.parametrize("n", [24, 25])
def test_large_tables_same_bytes_with_either_kernel(ctx, n):
    """n = 24: 2048 partials of 8192 entries (32 rounds of loads each); n = 25: the one-level schedule's pass 0."""
    count = 1 << n
    rows = mp.pin(ctx, n, 1, kind=ms.STREAM_8_1, nblk=2048, chunk=count // 2048)
    assert (rows[1]["kind"] == ms.FINE_SUMS) == (n == 24)
    d = ctx.alloc(count * 32)
    try:
        ctx.fill_table(d, count, 22000 + n)
        got = ctx.sumcheck_mle_batch_device(d, n, 1)
        ctx.set_option("pass0_stream", 1)
        try:
            mp.pin(ctx, n, 1, kind=ms.SUB_SUMS, nblk=2048)
            want = ctx.sumcheck_mle_batch_device(d, n, 1)
        finally:
            ctx.set_option("pass0_stream", 2)
    finally:
        ctx.free(d)
    assert _same(got, want)
    assert all(int(x) in (1, 2) for x in got[1][0])


def test_carries_between_the_half_sums(ctx):
    """A lane sums one 128-bit half of its entries: tables that carry out of the low half at every addend, that never do, whose
    halves are all ones / all zero, and the byte-pattern specials of test_gpu_mle_two_level_fold."""
    n = 18
    count = 1 << n
    specials = _limbs([0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
                       int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
                       int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128, LOW, (P - 1) & ~LOW])
    rng = np.random.default_rng(5000 + n)
    tables = {"all_p_minus_1": np.repeat(_limbs([P - 1]), count, axis=0), "low_half_ones": np.repeat(_limbs([LOW]), count, axis=0),
              "high_half_only": np.repeat(_limbs([(P - 1) & ~LOW]), count, axis=0), "specials": specials[rng.integers(0, len(specials), count)]}
    for name, t in tables.items():
        t = np.ascontiguousarray(t)
        assert _same(ctx.sumcheck_mle_raw(t, n), cdense.sumcheck_mle_raw(t, n)), name


@pytest.mark.parametrize("where", ["first_pair", "last_pair", "lanes_60_63"])
def test_dependence_on_the_last_variable(ctx, where):
    """base[idx >> 1] does not depend on x_n (last round: one coefficient); with ONE odd entry changed in ONE 32-bit limb it does
    (two), wherever the pair sits -- the first and the last quad of the table, the last quad of a wave's load step -- and
    whichever limb of either half differs."""
    n = 18
    count = 1 << n
    base = cdense.fill_table(count, 22818)
    flat = np.ascontiguousarray(base[np.arange(count) >> 1])
    want = cdense.sumcheck_mle_raw(flat, n)
    assert int(want[1][-1]) == 1 and _same(ctx.sumcheck_mle_raw(flat, n), want)
    odd = {"first_pair": 1, "last_pair": count - 1, "lanes_60_63": 32 * 4321 + 31}[where]
    for limb in (0, 3, 4, 7):
        t = flat.copy()
        t[odd, limb // 2] ^= np.uint64(1 << (32 * (limb % 2) + 3))
        want = cdense.sumcheck_mle_raw(t, n)
        assert int(want[1][-1]) == 2, (where, limb)
        assert _same(ctx.sumcheck_mle_raw(t, n), want), (where, limb)


def test_constant_and_zero_tables(ctx):
    n = 18
    count = 1 << n
    for name, t in (("constant", np.repeat(cdense.fill_table(8, 22819)[3:4], count, axis=0)), ("zero", np.zeros((count, 4), dtype=np.uint64))):
        t = np.ascontiguousarray(t)
        assert _same(ctx.sumcheck_mle_raw(t, n), cdense.sumcheck_mle_raw(t, n)), name


@pytest.mark.parametrize("depth", ["1", "16"])
def test_ragged_batch_in_small_groups(depth):
    """(18, 7) in groups of three (3 + 3 + 1), pass 0 queued one group at a time or all up front, two tables on the byte-pattern
    extremes."""
    env = dict(os.environ, GKR_PASS0_STREAM="2", GKR_GROUP_SIZE="3", GKR_PASS_QUEUE_DEPTH=depth)
    out = subprocess.run([sys.executable, os.path.join(HERE, "fold_variants_worker.py"), "18", "7"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_twenty_calls_same_bytes_and_inputs_untouched(ctx):
    """The partial slots are shared call after call; the kernel only reads the tables."""
    n, seeds = 18, [22950, 22951]
    count = 1 << n
    mp.pin(ctx, n, len(seeds), kind=ms.STREAM_8_1, nblk=1024, chunk=256)
    d = ctx.alloc(len(seeds) * count * 32)
    try:
        for b, seed in enumerate(seeds):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, seed)
        for rep in range(20):
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, len(seeds))
            for b, seed in enumerate(seeds):
                assert _same((C[b], L[b], R[b]), _oracle_of_seed(n, seed)), (rep, b)
        after = ctx.download(d, (len(seeds) * count, 4))
    finally:
        ctx.free(d)
    assert np.array_equal(after, np.concatenate([cdense.fill_table(count, seed) for seed in seeds]))

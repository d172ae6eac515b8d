"""Pass 0 of the plain sumcheck read through ONE rolling load buffer (csrc/kernels.hip k_mle_sub_sums_roll, option pass0_stream = 3):
the contract of the two-set form k_mle_sub_sums_stream -- a wave owns whole partials, 16-byte non-temporal pieces, a 128-bit
half-entry sum with a carry limb per lane, the x_n test across a quad -- with every piece loaded again, sixteen steps ahead, as soon
as it has been added, and with the blocks that share an XCD on one contiguous eighth of the launch.  The launcher's instance is a
partial per wave in blocks of four waves; it takes the launches the two-set <16, 2> takes with option 2: at least 24 576 partials
of whole 512 entries (kernels.h kMlePass0DeepMinPartials); every other launch keeps what option 2 gives it.  The partials are the
same integers, so every case is checked byte for byte against the C oracle (cdense.sumcheck_mle_raw), or against pass0_stream = 1
where the oracle would take too long.  A case that names the launch it means to reach first asserts it on the context's plan
(tests/mle_plan.py pin: the library's own launch plan against tests/mle_shapes.py)."""

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
PPW = 1        # partials a wave of the launcher's instance owns
WAVE = 274     # the wave whose partials carry the marked entries: partials PPW * WAVE .. PPW * WAVE + PPW - 1 of a table


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    c.set_option("pass0_stream", 3)
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


def _specials(count):
    return _limbs([0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
                   int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
                   int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128, LOW, (P - 1) & ~LOW])


@pytest.mark.parametrize("n", [19, 20])
def test_deep_launch_matches_oracle(ctx, n):
    """ONE pass-0 launch of 24 tables x 1024 partials (group_size = 24: the default schedule would cut the batch into two groups of
    12, below the kernel's threshold): 6144 blocks, every XCD's 768 on three of the tables.  n = 19: one round of sixteen loads per partial, the loop does not run at all; n = 20: two
    rounds.  Wave 274 of a table (the third wave of block 68) sums partial 274.  Members of the batch:
      0      p - 1 throughout: every half sum carries at every addend;
      1      a table that does not depend on x_n (L[..][-1] = 1);
      2 - 4  that table with ONE odd entry changed in one 32-bit limb (L[..][-1] = 2): in the first and in the last pair of the
             wave's partial (the last pair is the wave's last quad), and in the table's last pair;
      5      zero outside partial 274: a sum or a flag that reached a neighbour wave's partial shows in that partial's fine sum
             (rounds 6 - 10) or in the last round's length;
      6 - 8  carries between the two half sums and into the carry limb: the low half all ones, the high half only, and the
             byte-pattern specials of test_gpu_mle_pass0_stream;
      the rest: seeded tables."""
    count, batch = 1 << n, 24
    chunk = count // 1024
    first = PPW * WAVE
    seeds = [25100 + 97 * n + b for b in range(batch)]
    base = cdense.fill_table(count, seeds[1])
    flat = np.ascontiguousarray(base[np.arange(count) >> 1])
    special = {0: np.repeat(_limbs([P - 1]), count, axis=0), 1: flat}
    odd_entries = []
    for p in range(first, first + PPW):
        odd_entries += [p * chunk + 1, (p + 1) * chunk - 1]
    odd_entries.append(count - 1)
    for k, e in enumerate(odd_entries):
        t = flat.copy()
        t[e, (k % 4)] ^= np.uint64(1 << (3 + 32 * (k % 2)))
        special[2 + k] = t
    at = 2 + len(odd_entries)
    for p in sorted({first, first + PPW - 1}):
        lone = np.zeros((count, 4), dtype=np.uint64)
        lone[p * chunk:(p + 1) * chunk] = base[p * chunk:(p + 1) * chunk]
        special[at] = lone
        at += 1
    rng = np.random.default_rng(5000 + n)
    sp = _specials(count)
    for t in (np.repeat(_limbs([LOW]), count, axis=0), np.repeat(_limbs([(P - 1) & ~LOW]), count, axis=0), sp[rng.integers(0, len(sp), count)]):
        special[at] = np.ascontiguousarray(t)
        at += 1
    assert at <= batch
    assert mp.context_plan(ctx, n, batch)[0][3] == 2   # (the default schedule: two groups)
    ctx.set_option("group_size", batch)
    d = ctx.alloc(batch * count * 32)
    try:
        mp.pin(ctx, n, batch, kind=ms.ROLL, nblk=1024, chunk=chunk, nb=batch, publisher=ms.PUB_REDUCE)
        for b, seed in enumerate(seeds):
            where = ctypes.c_void_p(d.value + b * count * 32)
            if b in special:
                ctx.upload(where, special[b])
            else:
                ctx.fill_table(where, count, seed)
        C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
    finally:
        ctx.free(d)
        ctx.set_option("group_size", 0)
    for b, seed in enumerate(seeds):
        want = cdense.sumcheck_mle_raw(special[b], n) if b in special else _oracle_of_seed(n, seed)
        assert _same((C[b], L[b], R[b]), want), (n, b)
    assert int(L[1][-1]) == 1 and [int(L[2 + k][-1]) for k in range(len(odd_entries))] == [2] * len(odd_entries)


@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("n", [13, 14, 15, 16, 17, 18])
def test_launcher_conditions_same_bytes_with_every_option(ctx, n, batch):
    """Launches that publish from their last block, chunks of 256 entries in few blocks, launches below the rolling kernel's
    threshold: the same bytes with options 1, 2 and 3, whichever kernel each launch takes, and the oracle's."""
    seeds = [25500 + 31 * n + b for b in range(batch)]
    fused = n == 13 or (batch == 1 and n <= 15)   # (32 blocks per table at n = 13; 64 and 128 blocks of a lone table)
    form = {"kind": ms.SUB_SUMS if fused else ms.STREAM_8_1, "chunk": 256, "publisher": ms.PUB_FUSED if fused else ms.PUB_REDUCE}
    mp.pin(ctx, n, batch, **form)   # (below the rolling kernel's threshold: what option 2 gives the launch)
    got = _batch_of_seeds(ctx, n, seeds)
    try:
        for other in (1, 2):
            ctx.set_option("pass0_stream", other)
            mp.pin(ctx, n, batch, **(form if other == 2 else dict(form, kind=ms.SUB_SUMS)))
            assert _same(got, _batch_of_seeds(ctx, n, seeds)), other
    finally:
        ctx.set_option("pass0_stream", 3)
    for b, seed in enumerate(seeds):
        assert _same((got[0][b], got[1][b], got[2][b]), _oracle_of_seed(n, seed)), (n, b)


def test_one_large_table_same_bytes_with_either_kernel(ctx):
    """n = 24: 2048 partials of 8192 entries -- below the rolling kernel's 24 576 partials: the shallow pipelined form against
    k_mle_sub_sums, as the plan says."""
    n = 24
    count = 1 << n
    mp.pin(ctx, n, 1, kind=ms.STREAM_8_1, nblk=2048, chunk=8192)
    d = ctx.alloc(count * 32)
    try:
        ctx.fill_table(d, count, 25000 + n)
        got = ctx.sumcheck_mle_batch_device(d, n, 1)
        ctx.set_option("pass0_stream", 1)
        try:
            want = ctx.sumcheck_mle_batch_device(d, n, 1)
        finally:
            ctx.set_option("pass0_stream", 3)
    finally:
        ctx.free(d)
    assert _same(got, want)
    assert all(int(x) in (1, 2) for x in got[1][0])


@pytest.mark.parametrize("depth", ["1", "16"])
@pytest.mark.parametrize("n", ["18", "20"])
def test_ragged_batch_in_small_groups(n, depth):
    """(n, 7) in groups of three (3 + 3 + 1), pass 0 queued one group at a time or all up front, two tables on the byte-pattern
    extremes."""
    env = dict(os.environ, GKR_PASS0_STREAM="3", GKR_GROUP_SIZE="3", GKR_PASS_QUEUE_DEPTH=depth)
    out = subprocess.run([sys.executable, os.path.join(HERE, "fold_variants_worker.py"), n, "7"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("batch", [2, 24])
def test_twenty_calls_same_bytes_and_inputs_untouched(ctx, batch):
    """The partial slots are shared call after call; the kernel only reads the tables.  Two tables, as the schedule takes them; and the
    same two within ONE launch of 24 tables, which the rolling kernel takes."""
    n = 19
    count = 1 << n
    seeds = [25950 + b for b in range(batch)]
    ctx.set_option("group_size", batch)
    d = ctx.alloc(batch * count * 32)
    try:
        mp.pin(ctx, n, batch, kind=ms.ROLL if batch == 24 else ms.STREAM_8_1, nblk=1024, chunk=512, nb=batch)
        for b, seed in enumerate(seeds):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, seed)
        before = ctx.download(d, (batch * count, 4))
        first = ctx.sumcheck_mle_batch_device(d, n, batch)
        for rep in range(19):
            assert _same(ctx.sumcheck_mle_batch_device(d, n, batch), first), rep
        after = ctx.download(d, (batch * count, 4))
    finally:
        ctx.free(d)
        ctx.set_option("group_size", 0)
    for b, seed in enumerate(seeds):
        assert _same((first[0][b], first[1][b], first[2][b]), _oracle_of_seed(n, seed)), b
    assert np.array_equal(after, before)
    assert np.array_equal(after[:2 * count], np.concatenate([cdense.fill_table(count, seed) for seed in seeds[:2]]))


def test_block_count_no_multiple_of_eight(ctx):
    """The runs of blocks an XCD takes are of two lengths when the grid is no multiple of eight blocks.  1537 tables of 2^14 entries,
    three rounds per pass: pass 0 has 16 partials of 1024 entries per table, 4 blocks per table, 6148 blocks = 8 * 768 + 4 in one
    launch of 24 592 partials.  The same bytes as with k_mle_sub_sums, and the oracle's for the first tables, one in the middle
    and the last one."""
    n, batch = 14, 1537
    count = 1 << n
    seeds = [26000 + b for b in range(batch)]
    d = ctx.alloc(batch * count * 32)
    try:
        for b, seed in enumerate(seeds):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, seed)
        got = {}
        for option in (3, 1):
            ctx.set_option("pass0_stream", option)
            ctx.set_option("rounds_per_pass", 3)
            ctx.set_option("group_size", batch)
            mp.pin(ctx, n, batch, kind=ms.ROLL if option == 3 else ms.SUB_SUMS, nblk=16, chunk=1024, nb=batch, jout=3)
            got[option] = ctx.sumcheck_mle_batch_device(d, n, batch)
    finally:
        ctx.free(d)
        ctx.set_option("pass0_stream", 3)
        ctx.set_option("rounds_per_pass", 0)
        ctx.set_option("group_size", 0)
    assert _same(got[3], got[1])
    for b in (0, 1, 2, 768, batch - 1):
        assert _same((got[3][0][b], got[3][1][b], got[3][2][b]), _oracle_of_seed(n, seeds[b])), b

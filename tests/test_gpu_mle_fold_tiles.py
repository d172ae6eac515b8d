"""The two-level first fold as a loop over tiles with a rolling load buffer (csrc/kernels.hip k_mle_multifold2_mfma,
csrc/mfma_fold.h), one tile per block by default, more with option fold2_tiles.  No value of it changes a byte: (C, L, R) is
compared with the C oracle (cdense.sumcheck_mle_raw) and with the run at one tile per block.  Every run first asserts the tiles per block
it means to reach on the context's plan (tests/mle_plan.py pin: the library's own launch plan against tests/mle_shapes.py)."""

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


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    c.set_option("first_fold_levels", 2)
    yield c
    c.close()


def _seed(n, b):
    return 24000 + 89 * n + b


@functools.lru_cache(maxsize=None)
def _oracle(n, b):
    """(C, L, R) of table b at size n: computed once, shared by every case that uses the table."""
    return cdense.sumcheck_mle_raw(cdense.fill_table(1 << n, _seed(n, b)), n)


def _limbs(values):
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def _filled_batch(ctx, n, batch, tiles):
    count = 1 << n
    d = ctx.alloc(batch * count * 32)
    ctx.set_option("fold2_tiles", tiles)
    try:
        # the fold's row: the largest power of two of tiles that is at most what was asked and at most 2^(n-16), one for 0
        T = 1 << (max(min(tiles, 1 << (n - 16)), 1).bit_length() - 1)
        mp.pin(ctx, n, batch, row=2, kind=ms.FOLD2, chunk=256 * T, nblk=(1 << (n - 13)) // T, jin=10)
        for b in range(batch):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, _seed(n, b))
        return ctx.sumcheck_mle_batch_device(d, n, batch)
    finally:
        ctx.set_option("fold2_tiles", 0)
        ctx.free(d)


_one_tile = {}


def _one_tile_run(ctx, n, batch):
    if (n, batch) not in _one_tile:
        _one_tile[(n, batch)] = _filled_batch(ctx, n, batch, 1)
    return _one_tile[(n, batch)]


CASES = ([(18, b, t) for b in (1, 3) for t in (1, 2, 4, 64)] +      # I = 256: four tiles, g = 8, eight partials per tile; 64 clamps to 4
         [(19, b, t) for b in (1, 3) for t in (1, 2, 8)] +
         [(20, b, t) for b in (1, 3) for t in (1, 4, 16)] +         # 16: all tiles of a (table, cq) in one block
         [(21, 1, t) for t in (0, 8)])                              # sub = 64: g = 64, one partial per tile; 0: the rule


@pytest.mark.parametrize("n,batch,tiles", CASES)
def test_tiles_per_block_match_oracle_and_one_tile(ctx, n, batch, tiles):
    C, L, R = _filled_batch(ctx, n, batch, tiles)
    assert _same((C, L, R), _one_tile_run(ctx, n, batch)), "differs from one tile per block"
    for b in range(batch):
        assert _same((C[b], L[b], R[b]), _oracle(n, b)), (n, b, tiles)


def test_extreme_bytes_and_length_rule_at_four_tiles(ctx):
    """n = 18, four tiles per block: all 0 (the folded table is zero: every round vector has one coefficient), all r - 1, every
    byte 0xFF below the modulus (the digits' and the bias's extremes), a table that does not depend on x_n (the last round's
    length), and one that is zero but for a single entry."""
    n = 18
    count = 1 << n
    base = cdense.fill_table(count, _seed(n, 40))
    idx = np.arange(count)
    one_entry = np.zeros((count, 4), dtype=np.uint64)
    one_entry[(9 << 13) + (21 << 8) + 201] = base[5]
    ff = _limbs([int.from_bytes(b"\xff" * 31 + b"\x2f", "little")])
    assert int.from_bytes(b"\xff" * 31 + b"\x2f", "little") < P
    tables = {"zero": np.zeros((count, 4), dtype=np.uint64), "all_max": np.repeat(_limbs([P - 1]), count, axis=0),
              "all_ff": np.repeat(ff, count, axis=0), "no_x_n": base[idx >> 1], "one_entry": one_entry}
    ctx.set_option("fold2_tiles", 4)
    try:
        mp.pin(ctx, n, 1, row=2, kind=ms.FOLD2, chunk=1024, nblk=8)
        for name, t in tables.items():
            t = np.ascontiguousarray(t)
            assert _same(ctx.sumcheck_mle_raw(t, n), cdense.sumcheck_mle_raw(t, n)), name
    finally:
        ctx.set_option("fold2_tiles", 0)
    assert int(cdense.sumcheck_mle_raw(np.ascontiguousarray(tables["no_x_n"]), n)[1][n - 1]) == 1


@pytest.mark.parametrize("batch", ["7", "1"])
@pytest.mark.parametrize("depth", ["1", "16"])
@pytest.mark.parametrize("tiles", ["0", "4"])
def test_small_groups_in_a_child_interpreter(batch, depth, tiles):
    """(18, 7) in groups of two (2 + 2 + 2 + 1), pass 0 queued one group at a time or all up front, one tile per block or four:
    several groups' folds in flight beside the side stream's launches, two tables on the byte-pattern extremes; every run
    matches the oracle, so all have the same bytes.  Batch 1 is one group."""
    env = dict(os.environ, GKR_FIRST_FOLD_LEVELS="2", GKR_GROUP_SIZE="2", GKR_PASS_QUEUE_DEPTH=depth, GKR_FOLD2_TILES=tiles)
    out = subprocess.run([sys.executable, os.path.join(HERE, "fold_variants_worker.py"), "18", batch], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_twenty_calls_give_the_same_bytes(ctx):
    """(18, 7) in groups of two on one context: the partial slots that pass 0, the fine sums and the fold share, call after call;
    the input tables are what they were."""
    n, batch = 18, 7
    count = 1 << n
    d = ctx.alloc(batch * count * 32)
    ctx.set_option("group_size", 2)
    try:
        assert mp.context_plan(ctx, n, batch)[0][10:15] == [0, 1, 3, 5, 7]   # (four groups: 1 + 2 + 2 + 2 by the bounds' rounding)
        mp.pin(ctx, n, batch, group=1, row=2, kind=ms.FOLD2, chunk=256, nblk=32, nb=2)
        for b in range(batch):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, _seed(n, b))
        before = ctx.download(d, (batch * count, 4))
        for rep in range(20):
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
            for b in range(batch):
                assert _same((C[b], L[b], R[b]), _oracle(n, b)), (rep, b)
        assert np.array_equal(ctx.download(d, (batch * count, 4)), before)
        assert np.array_equal(before[:count], cdense.fill_table(count, _seed(n, 0)))
    finally:
        ctx.set_option("group_size", 0)
        ctx.free(d)

"""The plain sumcheck's first fold at two levels (csrc/kernels.hip k_mle_multifold2_mfma, option first_fold_levels = 2): ten
variables bound in the table's second read, rounds 6-10 hashed from sums the device forms out of pass 0's partials, the
folded table left in eight partial planes for the one-block pass behind it.  Host-hashed sumchecks of 2^18 .. 2^24 points take
it; everything is checked byte for byte against the C oracle (cdense.sumcheck_mle_raw), or against the one-level schedule
where the oracle would take too long.  A case that names the launches it means to reach first asserts them on the context's plan
(tests/mle_plan.py pin: the library's own launch plan against tests/mle_shapes.py)."""

import ctypes
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
TWO_LEVEL = [ms.STREAM_8_1, ms.FINE_SUMS, ms.FOLD2, ms.FOLD_SMALL]   # (pass 0, the fine sums, the fold of ten variables, the pass that reads its planes)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    c.set_option("first_fold_levels", 2)
    yield c
    c.close()


def _limbs(values):
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def _run_batch(ctx, tables, n):
    """The batch entry point on uploaded tables; also returns the tables as they are on the device after the call."""
    count, batch = 1 << n, len(tables)
    d = ctx.alloc(batch * count * 32)
    try:
        for b, t in enumerate(tables):
            ctx.upload(ctypes.c_void_p(d.value + b * count * 32), t)
        out = ctx.sumcheck_mle_batch_device(d, n, batch)
        after = ctx.download(d, (batch * count, 4))
    finally:
        ctx.free(d)
    return out, after


def test_schedule_reports_the_two_level_fold():
    """10 | 5 | ... for 18 <= n <= 24 (mfma = 2), the one-level schedule on either side and for mfma = 1."""
    from gkr_amd import _native as N
    L = N.lib()

    def schedule(n, mfma):
        rounds = np.zeros(64, dtype=np.uint32)
        count = ctypes.c_size_t()
        assert L.gkr_selftest_pass_schedule(ctypes.c_int(n), ctypes.c_int(mfma), rounds.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(64),
                                            ctypes.byref(count)) == 0
        return [int(x) for x in rounds[:count.value]]
    assert schedule(20, 2) == [10, 5, 5] and schedule(18, 2) == [10, 5, 3] and schedule(24, 2) == [10, 5, 5, 4]
    assert schedule(20, 1) == [5, 3, 5, 5, 2]
    for n in (17, 25):
        assert schedule(n, 2) == schedule(n, 1)
    for n in range(18, 25):
        assert sum(schedule(n, 2)) == n


@pytest.mark.parametrize("n,batch", [(18, 1), (18, 3), (19, 1), (19, 3), (20, 1), (20, 3)])
def test_random_tables_match_oracle(ctx, n, batch):
    """n = 18 is the smallest size on the new path (pass 0 with 1024 one-iteration blocks, sub-blocks of 8 entries behind the fold),
    19 has sub-blocks of 16, 20 is the headline's (half-wave sub-blocks)."""
    count = 1 << n
    rows = mp.pin(ctx, n, batch, row=3, kinds=TWO_LEVEL, src_planes=8, chunk=1 << (n - 15), m_src=n - 10)
    assert rows[0]["nblk"] % 1024 == 0 and (n != 18 or (rows[0]["nblk"], rows[0]["chunk"]) == (1024, 256))
    d = ctx.alloc(batch * count * 32)
    try:
        for b in range(batch):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, 21000 + 97 * n + b)
        C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
    finally:
        ctx.free(d)
    for b in range(batch):
        want = cdense.sumcheck_mle_raw(cdense.fill_table(count, 21000 + 97 * n + b), n)
        assert _same((C[b], L[b], R[b]), want), (n, b)


def test_below_the_new_path_matches_oracle(ctx):
    """n = 17: the one-level schedule, whatever the option says."""
    n = 17
    assert ms.FOLD2 not in [r["kind"] for r in mp.pin(ctx, n, 1, row=1, kind=ms.FOLD_MFMA, m_src=17, jin=5)]
    table = cdense.fill_table(1 << n, 21717)
    assert _same(ctx.sumcheck_mle_raw(table, n), cdense.sumcheck_mle_raw(table, n))


@pytest.mark.parametrize("n", [24, 25])
def test_boundary_sizes_match_the_one_level_schedule(ctx, n):
    """n = 24 is the last size on the new path (2^14-entry planes, 2048 partials per table, a one-block pass of 512 outputs behind
    the fold), n = 25 the first above it: identical (C, L, R) bytes with first_fold_levels = 1."""
    count = 1 << n
    if n == 24:
        mp.pin(ctx, n, 1, row=3, kinds=TWO_LEVEL + [ms.FOLD_SMALL], src_planes=8, chunk=512, m_src=14)
    else:
        mp.pin(ctx, n, 1, row=1, kind=ms.FOLD_MFMA, m_src=25, jin=5)
    d = ctx.alloc(count * 32)
    try:
        ctx.fill_table(d, count, 21000 + n)
        got = ctx.sumcheck_mle_batch_device(d, n, 1)
        ctx.set_option("first_fold_levels", 1)
        try:
            mp.pin(ctx, n, 1, row=1, kind=ms.FOLD_MFMA, m_src=n, jin=5)
            want = ctx.sumcheck_mle_batch_device(d, n, 1)
        finally:
            ctx.set_option("first_fold_levels", 2)
    finally:
        ctx.free(d)
    assert _same(got, want)
    assert all(int(x) in (1, 2) for x in got[1][0])


def test_extreme_byte_patterns_match_oracle(ctx):
    """The tables of test_gpu_parity.test_mle_extreme_byte_patterns_match_oracle at n = 18: the byte patterns on the sign and carry
    boundaries of the matrix-core fold's digits, p - 1 throughout for the bounds of the lazy sums behind it."""
    n = 18
    count = 1 << n
    specials = _limbs([0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
                       int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
                       int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128])
    rng = np.random.default_rng(4000 + n)
    picked = specials[rng.integers(0, len(specials), count)]
    tables = {"all_max": np.repeat(specials[2:3], count, axis=0), "specials": picked,
              "mixed": np.where(rng.random(count)[:, None] < 0.5, picked, cdense.fill_table(count, 4000 + n))}
    for mode, t in tables.items():
        t = np.ascontiguousarray(t)
        assert _same(ctx.sumcheck_mle_raw(t, n), cdense.sumcheck_mle_raw(t, n)), mode


def test_length_rule_in_the_rounds_from_device_formed_sums(ctx):
    """Rounds 6-10 come from sums the device forms: tables that do not depend on variables 6-10 (their round vectors have one
    coefficient), not on x_n, constant ones, and one that is zero but for a single entry."""
    n = 18
    count = 1 << n
    base = cdense.fill_table(count, 21818)
    idx = np.arange(count)
    one_entry = np.zeros((count, 4), dtype=np.uint64)
    one_entry[(5 << 13) + (19 << 8) + 77] = base[7]
    tables = {"no_vars_6_10": base[((idx >> 13) << 8) | (idx & 255)], "no_x_n": base[idx >> 1],
              "constant": np.repeat(base[3:4], count, axis=0), "zero": np.zeros((count, 4), dtype=np.uint64), "one_entry": one_entry}
    for name, t in tables.items():
        t = np.ascontiguousarray(t)
        got, want = ctx.sumcheck_mle_raw(t, n), cdense.sumcheck_mle_raw(t, n)
        assert _same(got, want), name
    lengths = cdense.sumcheck_mle_raw(np.ascontiguousarray(tables["no_vars_6_10"]), n)[1]
    assert [int(x) for x in lengths[5:10]] == [1] * 5 and int(lengths[4]) == 2


@pytest.mark.parametrize("depth", ["1", "16"])
def test_ragged_batch_in_small_groups(depth):
    """(18, 7) in groups of three (3 + 3 + 1), pass 0 queued one group at a time or all up front: the side stream's launches of
    several groups in flight, two tables on the byte-pattern extremes."""
    env = dict(os.environ, GKR_FIRST_FOLD_LEVELS="2", GKR_GROUP_SIZE="3", GKR_PASS_QUEUE_DEPTH=depth)
    out = subprocess.run([sys.executable, os.path.join(HERE, "fold_variants_worker.py"), "18", "7"], env=env, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr


def test_input_tables_are_untouched(ctx):
    n = 18
    tables = [cdense.fill_table(1 << n, 21900 + b) for b in range(2)]
    (C, L, R), after = _run_batch(ctx, tables, n)
    assert np.array_equal(after, np.concatenate(tables))
    for b in range(2):
        assert _same((C[b], L[b], R[b]), cdense.sumcheck_mle_raw(tables[b], n)), b


def test_fifty_calls_give_the_same_bytes(ctx):
    """Tickets, and the partial slots that pass 0, the fine sums and the fold share, call after call."""
    n, batch = 18, 2
    count = 1 << n
    mp.pin(ctx, n, batch, kinds=TWO_LEVEL, nblk=1024, chunk=256)
    d = ctx.alloc(batch * count * 32)
    try:
        for b in range(batch):
            ctx.fill_table(ctypes.c_void_p(d.value + b * count * 32), count, 21950 + b)
        want = [cdense.sumcheck_mle_raw(cdense.fill_table(count, 21950 + b), n) for b in range(batch)]
        for rep in range(50):
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
            for b in range(batch):
                assert _same((C[b], L[b], R[b]), want[b]), (rep, b)
    finally:
        ctx.free(d)

"""Streaming passes of the plain sumcheck that publish flag-in-word records (option stream_publish; csrc/flagged_rec.h, kernels.hip
k_mle_sub_sums_roll_pub and k_mle_multifold2_mfma<true>, capi_mle_passes.hip try_total): the blocks store {limb, ticket} words to pinned
memory, the hashing threads total them, no reduce launch follows.  No value of the option changes a byte: (C, L, R) of
stream_publish = 2 is compared with stream_publish = 1 (every pass through k_mle_sub_reduce) and with the C oracle.

Shapes, the smallest that reach the two kernels: n = 19, batch 48 in groups of 24 (24 x 1024 partials: the rolling pass 0); n = 20,
batch 50 with group_size 24 (three groups of 16 / 17 / 17: pass 0 below the rolling form's threshold keeps its reduce while the folds
publish -- both forms in one call); n = 18, batch 48 (pass 0 takes the <8, 1> form and keeps its reduce, and so does the fold, whose
partials are shorter than a record).  Which kernels ran is read from the context's profile rows (launches of k_mle_sub_reduce).
Tables 0 - 3 of every batch: all zero (valid records that carry zero data), r - 1 everywhere (the carry limbs), constant in x_n, and
constant in x_n but for the last pair (dep from exactly one block).  Every call first asserts the context's launch plan against the model
(tests/mle_plan.py, tests/mle_shapes.py); the reduce launches the profile counts are held against the plan's as well."""

import ctypes
import functools

import numpy as np
import pytest

import mle_plan as mp
import mle_shapes as ms
from gkr_amd import Context
from oracle import cdense
from oracle.field import P

pytestmark = pytest.mark.gpu

POOL = {18: 48, 19: 72, 20: 50}   # tables kept on the device per size; a case takes the first `batch` of them


def _seed(n, b):
    return 26000 + 97 * n + b


def _limbs(values):
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _special(n, b):
    count = 1 << n
    if b == 0:
        return np.zeros((count, 4), dtype=np.uint64)
    if b == 1:
        return np.ascontiguousarray(np.repeat(_limbs([P - 1]), count, axis=0))
    flat = cdense.fill_table(count, _seed(n, b))[np.arange(count) >> 1]
    if b == 3:
        flat[count - 1] = flat[0]
        assert not np.array_equal(flat[count - 1], flat[count - 2])
    return np.ascontiguousarray(flat)


@functools.lru_cache(maxsize=None)
def _oracle(n, b):
    """(C, L, R) of table b at size n: computed once, shared by every case that uses the table."""
    return cdense.sumcheck_mle_raw(_special(n, b) if b < 4 else cdense.fill_table(1 << n, _seed(n, b)), n)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pools(ctx):
    """n -> device buffer of POOL[n] tables, filled once."""
    bufs = {}
    for n, batch in POOL.items():
        count = 1 << n
        d = ctx.alloc(batch * count * 32)
        for b in range(batch):
            at = ctypes.c_void_p(d.value + b * count * 32)
            if b < 4:
                ctx.upload(at, _special(n, b))
            else:
                ctx.fill_table(at, count, _seed(n, b))
        bufs[n] = d
    yield bufs
    for d in bufs.values():
        ctx.free(d)


def _planned_reduces(ctx, n, batch):
    """k_mle_sub_reduce launches the context's plan (asserted against the model) holds for the call: a row per pass that publishes
    through one, and the one two-level fold that keeps its reduce where the others publish records."""
    header, rows = mp.context_plan(ctx, n, batch)
    mp.assert_plan(ctx, n, batch)
    return sum(r[8] == ms.PUB_REDUCE for r in rows) + (1 if header[7] else 0)


def _run_planned(ctx, d, n, batch, **options):
    """(outputs, the k_mle_sub_reduce launches the plan holds for the call, group 1's rows -- or group 0's of a one-group call)."""
    for k, v in options.items():
        ctx.set_option(k, v)
    try:
        planned = _planned_reduces(ctx, n, batch)
        rows = mp.assert_plan(ctx, n, batch, group=1) or mp.assert_plan(ctx, n, batch, group=0)
        return ctx.sumcheck_mle_batch_device(d, n, batch), planned, rows
    finally:
        for k in options:
            ctx.set_option(k, 0)


def _run(ctx, d, n, batch, **options):
    return _run_planned(ctx, d, n, batch, **options)[0]


def _check(got, n, batch, what):
    C, L, R = got
    for b in range(batch):
        assert _same((C[b], L[b], R[b]), _oracle(n, b)), (what, n, b)


def test_length_rule_of_the_special_tables():
    for n in POOL:
        assert int(_oracle(n, 2)[1][n - 1]) == 1 and int(_oracle(n, 3)[1][n - 1]) == 2 and int(_oracle(n, 0)[1][0]) == 1


def _reduce_launches(ctx, d, n, batch, **options):
    """(outputs, launches of k_mle_sub_reduce in the call) -- from the context's profile rows, every kernel timed; held to the plan's
    count and, if `kinds` = (pass 0's kind, the two-level fold's publisher) is given, to those of the context's plan rows."""
    kinds = options.pop("kinds", None)
    ctx.profile(1)
    try:
        ctx.profile_reset()
        out, planned, rows = _run_planned(ctx, d, n, batch, **options)
        launches = ctx.profile_get("mle_sub_reduce")["launches"]
        assert launches == planned, (launches, planned)
        if kinds:
            assert (rows[0]["kind"], rows[2]["kind"], rows[2]["publisher"]) == (kinds[0], ms.FOLD2, kinds[1]), (n, batch, options)
        return out, launches
    finally:
        ctx.profile(0)
        ctx.profile_reset()


# k_mle_sub_reduce launches of a call with stream_publish = 2: with 1 every pass 0 and every first fold has one (2 per group; later
# passes are one-block kernels that publish themselves).  n = 19, two groups of 24: both pass 0s (the rolling form) and the first
# group's fold publish records, the call's last fold keeps its reduce: 1.  n = 20, groups of 16 / 17 / 17: the pass 0s are below the
# rolling form's threshold and keep theirs, two of three folds publish: 3 + 1.  n = 18: pass 0 takes <8, 1> and the fold's partials
# have eight entries, fewer than a record's ten words: nothing publishes, 4.
REDUCES = {19: (1, 4), 20: (4, 6), 18: (4, 4)}


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("n,batch", [(19, 48), (20, 50), (18, 48)])
def test_published_records_match_reduce_kernel_and_oracle(ctx, pools, n, batch, depth):
    # (what the docstring names, on the context's plan rows: pass 0's kind and the fold's publisher of the second group)
    new_kinds = {19: (ms.ROLL_PUB, ms.PUB_FLAGGED), 20: (ms.STREAM_8_1, ms.PUB_FLAGGED), 18: (ms.STREAM_8_1, ms.PUB_REDUCE)}[n]
    old_kinds = {19: (ms.ROLL, ms.PUB_REDUCE), 20: (ms.STREAM_8_1, ms.PUB_REDUCE), 18: (ms.STREAM_8_1, ms.PUB_REDUCE)}[n]
    new, new_reduces = _reduce_launches(ctx, pools[n], n, batch, stream_publish=2, group_size=24, pass_queue_depth=depth, kinds=new_kinds)
    old, old_reduces = _reduce_launches(ctx, pools[n], n, batch, stream_publish=1, group_size=24, pass_queue_depth=depth, kinds=old_kinds)
    assert (new_reduces, old_reduces) == REDUCES[n], "the publishing kernels were not the ones that ran"
    assert _same(new, old), "stream_publish 2 differs from 1"
    _check(new, n, batch, "stream_publish 2")


def test_default_matches(ctx, pools):
    _check(_run(ctx, pools[19], 19, 48, group_size=24), 19, 48, "defaults")


def test_calls_in_a_row_leave_stale_tickets(ctx, pools):
    """72 tables, then 48, then 72 on one context: every slot holds the records of an earlier call, under older tickets."""
    for batch in (72, 48, 72):
        _check(_run(ctx, pools[19], 19, batch, stream_publish=2, group_size=24), 19, batch, "batch %d in a row" % batch)


def test_one_group_and_device_hashed_calls_keep_the_reduce(ctx, pools):
    """One group (nothing waits behind its reduce) and a call with a device-hashed share, whose chain never publishes records."""
    out, reduces = _reduce_launches(ctx, pools[19], 19, 24, stream_publish=2, group_size=24)
    assert reduces == 2, "a one-group call published records"
    _check(out, 19, 24, "one group")
    _check(_run(ctx, pools[19], 19, 72, stream_publish=2, group_size=24, device_hash_percent=25), 19, 72, "device-hashed share")

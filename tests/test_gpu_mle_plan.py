"""The plain sumcheck on either side of every cut of its launch plan (tests/mle_shapes.py: the schedule of a batch, the pass-0 form, who
publishes, the fold form and its blocks, the stream, the host tail).  Each case names the cuts it sits on and the outcome it means to
meet; it first asserts that the context's own plan (gkr_selftest_mle_plan_ctx: the functions the driver and its launches call) equals
the model's rows and that those rows went through the named comparisons with the named outcomes -- a case that has drifted off its
threshold, or a retuned constant, fails there -- and only then compares coefficients, lengths and challenges of every sumcheck byte for
byte with the C oracle (cdense.sumcheck_mle_raw), and the downloaded inputs with what was uploaded.

Tables: seeded ones (a cycle of 61 seeds where the batch is larger, so neighbours always differ) and, at the head of the batch, the
members that bite at a launch edge: every entry r - 1; a table that does not depend on x_n; that table with one bit changed in the
first pair of the first partial, in the last pair of the last partial and in the last pair of a middle block (the last round's length
is asserted on the oracle's output: 1, then 2, 2, 2); a table that is zero outside one partial; the byte-pattern specials of
test_gpu_mle_pass0_rolling.  A batch smaller than the list takes it in several calls (and one more of seeded tables alone where the
list fills every call).  Tables of 2^22 and 2^23 entries take the members that reach furthest -- the last-pair bit and the lone
partial -- and the seeded table; the two cases at 2^24 and 2^25 entries (either side of the two-level cut) the seeded table alone,
filled on the device: one upload of 512 MiB or 1 GiB with its oracle transcript is what took them past twice the longest case of
test_gpu_layer_dense.py.  The launch-edge members at those two sizes reach kernels that the cases at 2^22 (2048 partials of pass 0,
the two-level fold without records) and at 2^21 on one level already run with them.

tests/test_mle_shapes_host.py asserts on the host that every case here meets the cuts it names (CASES is data)."""

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
LOW = (1 << 128) - 1
SEED_CYCLE = 61
THREADS = 4   # every case fixes the context's hashing threads: the schedule depends on them

# (id, n, batch, options, threads, [(cut, outcome) the model's decisions must go through], kinds of group 0's rows or None)
K = ms
CASES = [
    # ---- pass 0: the small kernel | k_mle_sub_sums
    ("pass0-small-n9", 9, 1, (), THREADS, [("pass0.small: len <= 512", True)], [K.SMALL0, K.FOLD_SMALL]),
    ("pass0-blocks-n10", 10, 1, (), THREADS, [("pass0.small: len <= 512", False), ("fused: nblk <= 128", True)], [K.SUB_SUMS, K.FOLD_SMALL]),
    # ---- the fused last block | a reduce launch
    ("fused-256-blocks-n10-b8", 10, 8, (), THREADS, [("fused: nblk * nb <= 256", True)], None),
    ("reduce-288-blocks-n10-b9", 10, 9, (), THREADS, [("fused: nblk * nb <= 256", False)], None),
    ("fused-n12-b2", 12, 2, (), THREADS, [("fused: nblk * nb <= 256", True)], None),
    ("reduce-n12-b9", 12, 9, (), THREADS, [("fused: nblk * nb <= 256", False)], None),
    ("fused-n13-b4", 13, 4, (), THREADS, [("fused: nblk * nb <= 256", True)], None),
    ("fused-n11-b8", 11, 8, (), THREADS, [("fused: nblk * nb <= 256", True)], None),
    ("reduce-n11-b9", 11, 9, (), THREADS, [("fused: nblk * nb <= 256", False)], None),
    ("fused-n13-b8", 13, 8, (), THREADS, [("fused: nblk * nb <= 256", True)], None),
    ("reduce-n13-b9", 13, 9, (), THREADS, [("fused: nblk * nb <= 256", False)], None),
    ("fused-128-blocks-n15", 15, 1, (), THREADS, [("fused: nblk <= 128", True)], None),
    ("reduce-256-blocks-n16", 16, 1, (), THREADS, [("fused: nblk <= 128", False)], None),
    ("fused-64MiB-n20-b2", 20, 2, (("fold_min_chunk", 4096), ("first_fold_levels", 1)), THREADS, [("fused: bytes read <= 64 MiB", True)], None),
    ("reduce-128MiB-n21-b2", 21, 2, (("fold_min_chunk", 4096), ("first_fold_levels", 1)), THREADS, [("fused: bytes read <= 64 MiB", False)], None),
    ("arrival-counters-end-at-4096", 10, 4097, (("device_hash_percent", 90), ("rounds_per_pass", 3)), 14, [("fused: b0 + nb <= 4096", False),
                                                                                                         ("fused: b0 + nb <= 4096", True)], None),
    ("no-arrival-counters-n22", 22, 1, (), THREADS, [("arrivals: table <= 64 MiB", False)], None),
    # ---- pass 0: k_mle_sub_sums | stream<8, 1>
    ("form0-chunk-64-n10", 10, 1, (("no_fused_reduce", 1),), THREADS, [("pass0.stream: chunk % 256 == 0", False)], [K.SUB_SUMS, K.FOLD_SMALL]),
    ("form1-chunk-256-n13", 13, 1, (("no_fused_reduce", 1),), THREADS, [("pass0.stream: chunk % 256 == 0", True), ("pass0.stream: nblk % 4 == 0", True)],
     [K.STREAM_8_1, K.FOLD_SMALL, K.FOLD_SMALL]),
    ("form0-two-blocks-n10", 10, 1024, (("rounds_per_pass", 1), ("group_size", 1024)), THREADS, [("pass0.stream: nblk % 4 == 0", False)], None),
    # ---- pass 0: stream<8, 1> | the deep forms
    ("shallow-chunk-256-n18", 18, 24, (("group_size", 24),), THREADS, [("pass0.deep: chunk % 512 == 0", False)], [K.STREAM_8_1, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("deep-24-tables-n19", 19, 24, (("group_size", 24),), THREADS, [("pass0.deep: batch * nblk >= 24576", True)], [K.ROLL, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("shallow-23-tables-n19", 19, 23, (("group_size", 24),), THREADS, [("pass0.deep: batch * nblk >= 24576", False)], [K.STREAM_8_1, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("deep-two-per-wave-n19", 19, 24, (("group_size", 24), ("pass0_stream", 2)), THREADS, [("pass0.deep: batch * nblk >= 24576", True)],
     [K.STREAM_16_2, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("deep-off-n19", 19, 24, (("group_size", 24), ("pass0_stream", 1)), THREADS, [], [K.SUB_SUMS, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("shallow-four-blocks", 12, 512, (("rounds_per_pass", 2), ("group_size", 512)), THREADS, [("pass0.deep: chunk % 512 == 0", True), ("pass0.deep: nblk % 8 == 0", False)], None),
    ("roll-2048-partials-reduce", 20, 23, (("items_per_block", 256),), THREADS, [("pass0.flagged: nblk == 1024", False)], None),
    # ---- the publishing rolling form | the rolling form
    ("roll-pub-two-groups-n19", 19, 48, (("group_size", 24),), THREADS, [("pass0.flagged: nblk == 1024", True), ("fold2.flagged: partials of >= 16 entries", True)],
     [K.ROLL_PUB, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("roll-reduce-two-groups-n19", 19, 48, (("group_size", 24), ("stream_publish", 1)), THREADS, [], [K.ROLL, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("roll-pub-explicit-n19", 19, 48, (("group_size", 24), ("stream_publish", 2)), THREADS, [("pass0.flagged: nblk == 1024", True)], [K.ROLL_PUB, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("fold2-reduce-small-partials-n18", 18, 2, (("group_size", 1),), THREADS, [("fold2.flagged: partials of >= 16 entries", False)], None),
    ("fold2-reduce-512-partials-n22", 22, 2, (("group_size", 1),), THREADS, [("fold2.flagged: 256 partials per table", False)], None),
    # ---- folds: one block | the grid; the block rule; the forms
    ("fold-one-block-S512", 10, 1, (("rounds_per_pass", 1),), THREADS, [("fold.small: S <= 512", True)], None),
    ("fold-grid-S1024", 11, 1, (("rounds_per_pass", 1),), THREADS, [("fold.small: S <= 512", False), ("fold.mfma: (S / nblk) % 64 == 0", True),
                                                                    ("fold_blocks.min_chunk: half the chunk >= the minimum", False)], None),
    ("fold-valu-by-option", 14, 3, (("no_mfma_fold", 1),), THREADS, [], [K.SUB_SUMS, K.FOLD_VALU, K.FOLD_SMALL, K.FOLD_SMALL, K.HOST_FOLD]),
    ("fold-blocks-target", 15, 127, (("fold_blocks", 2048),), THREADS, [("fold_blocks.target: blocks over the batch < target", False)], None),
    ("fold-blocks-cap-2048", 21, 1, (("rounds_per_pass", 1),), THREADS, [("fold_blocks.cap: twice the blocks <= 2048", False)], None),
    ("fold-min-chunk-64", 17, 5, (("fold_min_chunk", 64),), THREADS, [("fold_blocks.min_chunk: half the chunk >= the minimum", True)], None),
    # ---- late | main stream, the plan's stream
    ("late-m16-two-groups", 21, 2, (("group_size", 1), ("first_fold_levels", 1)), THREADS, [("fold.late: m_src <= 16", True)], None),
    ("main-m17-two-groups", 22, 2, (("group_size", 1), ("first_fold_levels", 1)), THREADS, [("fold.late: m_src <= 16", False)], None),
    ("main-m16-one-group", 21, 1, (("first_fold_levels", 1),), THREADS, [("fold.late: m_src <= 16", True)], None),
    ("plan-main-two-groups", 17, 2, (("group_size", 1), ("plan_main", 1)), THREADS, [], None),
    ("plan-side-two-groups", 17, 2, (("group_size", 1),), THREADS, [], None),
    ("no-late-stream-two-groups", 17, 2, (("group_size", 1), ("no_late_stream", 1)), THREADS, [], None),
    # ---- the two-level first fold: its range, its planes
    ("one-level-n17", 17, 1, (), THREADS, [("two_level: n >= 18", False)], [K.STREAM_8_1, K.FOLD_MFMA, K.FOLD_SMALL, K.HOST_FOLD]),
    ("two-level-n18", 18, 1, (), THREADS, [("two_level: n >= 18", True), ("two_level: n <= 24", True)], [K.STREAM_8_1, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("two-level-n24", 24, 1, (), THREADS, [("two_level: n <= 24", True)], [K.STREAM_8_1, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL, K.FOLD_SMALL]),
    ("one-level-n25", 25, 1, (), THREADS, [("two_level: n <= 24", False)], None),
    # (one level | two: pass 0 of eight tables of 2^18 in 256 blocks of 1024 entries | in the 1024 of 256 the fine sums need)
    ("one-level-256-blocks-n18-b8", 18, 8, (("first_fold_levels", 1),), THREADS, [], [K.STREAM_8_1, K.FOLD_MFMA, K.FOLD_SMALL, K.FOLD_SMALL]),
    ("two-level-1024-blocks-n18-b8", 18, 8, (), THREADS, [("pass0.two_level: chunk < 256", False)], [K.STREAM_8_1, K.FINE_SUMS, K.FOLD2, K.FOLD_SMALL]),
    ("leave-2-12-not-2-10-n15", 15, 1, (), THREADS, [("rounds.leave_2^10_or_2^11", True)], None),
    ("leave-2-12-not-2-11-n16", 16, 3, (), THREADS, [("rounds.leave_2^10_or_2^11", True)], None),
    # ---- the host tail
    ("tail-batch-8", 17, 8, (), THREADS, [("host_tail: batch <= 8 (host_tail_max_batch)", True), ("host_tail: m <= 7", True), ("host_tail: m - j > 0", True)], None),
    ("no-tail-batch-9", 17, 9, (), THREADS, [("host_tail: batch <= 8 (host_tail_max_batch)", False)], None),
    ("tail-m8-stays-on-device", 13, 2, (), THREADS, [("host_tail: m <= 7", False)], None),
    ("tail-nothing-to-save", 10, 2, (), THREADS, [("host_tail: m - j > 0", False)], None),
    ("tail-off", 17, 3, (("host_tail_log2", -1),), THREADS, [], [K.STREAM_8_1, K.FOLD_MFMA, K.FOLD_SMALL, K.FOLD_SMALL]),
    ("tail-three-host-folds", 9, 2, (("rounds_per_pass", 1),), THREADS, [("host_tail: m <= 7", True)], None),
    # ---- the schedule
    ("one-group-batch-15-n17", 17, 15, (), THREADS, [("groups.size: host batch >= 16", False)], None),
    ("two-groups-batch-16-n17", 17, 16, (), THREADS, [("groups.size: host batch >= 16", True)], None),
    ("two-groups-batch-127-n17", 17, 127, (), THREADS, [("groups.size: host batch >= 128", False)], None),
    ("four-groups-batch-128-n17", 17, 128, (), THREADS, [("groups.size: host batch >= 128", True)], None),
    ("four-groups-batch-255-n17", 17, 255, (), THREADS, [("groups.small_tables: host batch >= 256", False)], None),
    ("sixteen-groups-batch-256-n17", 17, 256, (), THREADS, [("groups.small_tables: host batch >= 256", True)], None),
    ("one-group-batch-15-n18", 18, 15, (), THREADS, [("groups.size: host batch >= 16", False)], None),
    ("two-groups-batch-16-n18", 18, 16, (), THREADS, [("groups.size: host batch >= 16", True)], None),
    ("two-groups-batch-127-n18", 18, 127, (), THREADS, [("groups.size: host batch >= 128", False)], None),
    ("four-groups-batch-128-n18", 18, 128, (), THREADS, [("groups.size: host batch >= 128", True)], None),
    ("four-groups-batch-255-n18", 18, 255, (), THREADS, [("groups.small_tables: n <= 17", False)], None),
    ("four-groups-batch-256-n18", 18, 256, (), THREADS, [("groups.small_tables: n <= 17", False), ("groups.few_threads: threads <= 3", False)], None),
    ("sixteen-groups-three-threads", 18, 256, (), 3, [("groups.few_threads: threads <= 3", True), ("groups.few_threads: host batch >= 256", True)], None),
    ("thirty-two-groups-of-33", 10, 33, (("group_size", 1),), THREADS, [("groups.cap: more than 32", True)], None),
    ("hash-chunk-16-full-calls", 10, 64, (("group_size", 64),), 2, [("hash_chunk: nb >= 32 threads", True)], None),
    ("hash-chunk-8", 10, 9, (), 2, [("hash_chunk: per thread <= 8", True)], None),
    ("hash-chunk-one-per-thread", 10, 9, (), 1, [("hash_chunk: per thread <= 8", False), ("hash_chunk: per thread <= 16", True)], None),
    ("hash-chunk-16-capped", 10, 17, (("group_size", 24),), 1, [("hash_chunk: per thread <= 16", False)], None),
    # ---- the device-hashed share
    ("device-hash-batch-63-none", 12, 63, (("device_hash_percent", 50),), THREADS, [("device_hash: batch >= 64", False)], None),
    ("device-hash-batch-64-half", 12, 64, (("device_hash_percent", 50),), THREADS, [("device_hash: batch >= 64", True), ("device_hash: batch - n_dev < 16", False)], None),
    ("device-hash-keeps-16-for-the-host", 12, 64, (("device_hash_percent", 90),), THREADS, [("device_hash: batch - n_dev < 16", True)], None),
    ("device-hash-fewer-than-8-none", 12, 64, (("device_hash_percent", 10),), THREADS, [("device_hash: n_dev < 8", True)], None),
]
CASE_IDS = [c[0] for c in CASES]

# What a case's id claims, on the rows: id -> [(group, row, {field: value})], and on the header: id -> {word: value} (3 the groups, 2 the
# device-hashed sumchecks, 43 the first group's hash chunk).  Asserted on the context's plan by every case and on the model by the host test.
_F, _R = {"publisher": K.PUB_FUSED}, {"publisher": K.PUB_REDUCE}
ROW_PINS = {
    "fused-256-blocks-n10-b8": [(0, 0, dict(_F, nblk=32))], "reduce-288-blocks-n10-b9": [(0, 0, dict(_R, nblk=32))],
    "fused-n12-b2": [(0, 0, _F)], "reduce-n12-b9": [(0, 0, dict(_R, nblk=32))], "fused-n13-b4": [(0, 0, _F)],
    "fused-n11-b8": [(0, 0, dict(_F, nblk=32))], "reduce-n11-b9": [(0, 0, dict(_R, nblk=32))],
    "fused-n13-b8": [(0, 0, dict(_F, nblk=32))], "reduce-n13-b9": [(0, 0, dict(_R, nblk=32))],
    "fused-128-blocks-n15": [(0, 0, dict(_F, nblk=128))], "reduce-256-blocks-n16": [(0, 0, dict(_R, nblk=256))],
    "fused-64MiB-n20-b2": [(0, 1, dict(_F, kind=K.FOLD_MFMA, nblk=8, m_src=20))], "reduce-128MiB-n21-b2": [(0, 1, dict(_R, kind=K.FOLD_MFMA, nblk=16, m_src=21))],
    "arrival-counters-end-at-4096": [(14, 0, dict(_F, nblk=8)), (15, 0, dict(_R, nblk=8, b0=4070, nb=27))],
    "fold-one-block-S512": [(0, 1, dict(kind=K.FOLD_SMALL, chunk=512))], "fold-grid-S1024": [(0, 1, dict(kind=K.FOLD_MFMA, nblk=4, chunk=256))],
    "fold-blocks-target": [(1, 1, dict(kind=K.FOLD_MFMA, nblk=32, nb=64))],   # (the second group: 64 tables x 32 blocks, the target of 2048)
    "fold-blocks-cap-2048": [(0, 1, dict(kind=K.FOLD_MFMA, nblk=2048, chunk=512))],
    "fold-min-chunk-64": [(0, 1, dict(kind=K.FOLD_MFMA, nblk=64, chunk=64))],   # (32 blocks of 128 without the option)
    "late-m16-two-groups": [(0, 2, dict(stream=K.ST_LATE, m_src=16, kind=K.FOLD_MFMA, plan=K.PLAN_OWN))],
    "main-m17-two-groups": [(0, 2, dict(stream=K.ST_MAIN, m_src=17, kind=K.FOLD_MFMA, plan=K.PLAN_SIDE))],
    "main-m16-one-group": [(0, 2, dict(stream=K.ST_MAIN, m_src=16, kind=K.FOLD_MFMA, plan=K.PLAN_OWN))],
    "plan-main-two-groups": [(0, 1, dict(plan=K.PLAN_OWN, stream=K.ST_MAIN)), (0, 2, dict(stream=K.ST_LATE))],
    "plan-side-two-groups": [(0, 1, dict(plan=K.PLAN_SIDE, stream=K.ST_MAIN)), (0, 2, dict(stream=K.ST_LATE))],
    "no-late-stream-two-groups": [(0, 1, dict(plan=K.PLAN_SIDE, stream=K.ST_MAIN)), (0, 2, dict(stream=K.ST_MAIN))],
    "one-level-256-blocks-n18-b8": [(0, 0, dict(nblk=256, chunk=1024))], "two-level-1024-blocks-n18-b8": [(0, 0, dict(nblk=1024, chunk=256))],
    "tail-batch-8": [(0, 2, dict(export_tail=1, chunk=128)), (0, 3, dict(kind=K.HOST_FOLD))], "no-tail-batch-9": [(0, 2, dict(export_tail=0, kind=K.FOLD_SMALL))],
    "tail-m8-stays-on-device": [(0, 1, dict(export_tail=0, chunk=256))], "tail-nothing-to-save": [(0, 1, dict(export_tail=0, chunk=32, jout=5))],
    "tail-three-host-folds": [(0, 2, dict(export_tail=1, chunk=128)), (0, 3, dict(kind=K.HOST_FOLD)), (0, 8, dict(kind=K.HOST_FOLD))],
    "roll-reduce-two-groups-n19": [(0, 0, _R), (0, 2, _R)], "roll-pub-two-groups-n19": [(0, 0, {"publisher": K.PUB_FLAGGED}), (0, 2, {"publisher": K.PUB_FLAGGED})],
    "fold2-reduce-small-partials-n18": [(0, 2, dict(_R, kind=K.FOLD2))], "fold2-reduce-512-partials-n22": [(0, 2, dict(_R, kind=K.FOLD2))],
    "device-hash-batch-64-half": [(2, 0, dict(stream=K.ST_CHAIN, nb=32, b0=0))],
}
HEADER_PINS = {
    "one-group-batch-15-n17": {3: 1}, "two-groups-batch-16-n17": {3: 2}, "two-groups-batch-127-n17": {3: 2}, "four-groups-batch-128-n17": {3: 4},
    "four-groups-batch-255-n17": {3: 4, 4: 2}, "sixteen-groups-batch-256-n17": {3: 16, 4: 4}, "one-group-batch-15-n18": {3: 1}, "two-groups-batch-16-n18": {3: 2},
    "two-groups-batch-127-n18": {3: 2}, "four-groups-batch-128-n18": {3: 4}, "four-groups-batch-255-n18": {3: 4}, "four-groups-batch-256-n18": {3: 4, 4: 2},
    "sixteen-groups-three-threads": {3: 16, 4: 2}, "thirty-two-groups-of-33": {3: 32, 10: 0, 11: 1, 42: 33},
    "hash-chunk-16-full-calls": {43: 16}, "hash-chunk-8": {43: 8}, "hash-chunk-one-per-thread": {43: 9}, "hash-chunk-16-capped": {43: 16},
    "device-hash-batch-63-none": {2: 0}, "device-hash-batch-64-half": {2: 32}, "device-hash-keeps-16-for-the-host": {2: 48}, "device-hash-fewer-than-8-none": {2: 0},
    "arrival-counters-end-at-4096": {2: 3680, 3: 16}, "tail-batch-8": {5: 1}, "no-tail-batch-9": {5: 0}, "tail-off": {5: 0},
}


def check_pins(name, header, rows):
    """The header words and row fields the case's id claims, on a plan (the context's, or the model's)."""
    for word, value in HEADER_PINS.get(name, {}).items():
        assert header[word] == value, (name, word, header[word], value)
    for group, row, fields in ROW_PINS.get(name, []):
        mine = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == group]
        got = {k: mine[row][k] for k in fields}
        assert got == fields, (name, group, row, got, fields)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _limbs(values):
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in values], dtype=np.uint64)


def _same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


@functools.lru_cache(maxsize=None)
def _seeded(n, seed):
    """fill_table(2^n, seed)'s oracle transcript: computed once, shared by every case that uses the table."""
    return cdense.sumcheck_mle_raw(cdense.fill_table(1 << n, seed), n)


def _seed(n, b):
    return 41000 + 131 * n + b % SEED_CYCLE


_SPECIALS = _limbs([0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
                    int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
                    int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128, LOW, (P - 1) & ~LOW])


@functools.lru_cache(maxsize=None)
def _members(n, chunk):
    """The launch-edge members for tables of 2^n entries whose pass 0 takes `chunk` entries per block: [(table, oracle transcript,
    last round's length or None)], the furthest-reaching first."""
    count = 1 << n
    if n >= 24:   # (no member: the seeded table alone, filled on the device)
        return []
    base = cdense.fill_table(count, 40000 + n)
    flat = np.ascontiguousarray(base[np.arange(count) >> 1])
    nblk = count // chunk
    mid = nblk // 2
    out = []

    def flipped(entry, k):
        t = flat.copy()
        t[entry, k % 4] ^= np.uint64(1 << (3 + 32 * (k % 2)))
        return t

    lone = np.zeros((count, 4), dtype=np.uint64)
    lone[mid * chunk:(mid + 1) * chunk] = base[mid * chunk:(mid + 1) * chunk]
    tables = [(flipped(count - 1, 1), 2), (lone, None)]
    if n < 22:
        rng = np.random.default_rng(7000 + n)
        tables += [(flat, 1), (flipped(1, 0), 2), (flipped((mid + 1) * chunk - 1, 2), 2), (np.repeat(_limbs([P - 1]), count, axis=0), None),
                   (np.ascontiguousarray(_SPECIALS[rng.integers(0, len(_SPECIALS), count)]), None)]
    for t, last in tables:
        want = cdense.sumcheck_mle_raw(t, n)
        if last is not None:
            assert int(want[1][-1]) == last, (n, last)   # (on the oracle's output: the member is what it is meant to be)
        out.append((t, want, last))
    return out


class _Options:
    def __init__(self, ctx, options, threads):
        self.ctx, self.options, self.threads = ctx, options, threads

    def __enter__(self):
        self.ctx.set_host_threads(self.threads)
        for k, v in self.options:
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, _ in self.options:
            self.ctx.set_option(k, 0)
        self.ctx.set_host_threads(0)


def _assert_plan(ctx, n, batch, options, threads, pins, kinds, name=None):
    rows = mp.assert_plan(ctx, n, batch, options, kinds)
    if name:
        check_pins(name, *mp.context_plan(ctx, n, batch))
    header, _, hits = ms.plan(n, batch, threads, options)
    assert mp.context_plan(ctx, n, batch)[0][9] == threads
    for pin in pins:
        assert pin in hits, (pin, n, batch, options, threads)
    return rows


def _run(ctx, n, batch, options, threads, pins, kinds, name=None):
    """One case: the plan, then every sumcheck against the oracle, then the inputs.  Returns the bytes of every call it made."""
    count = 1 << n
    outputs = []
    with _Options(ctx, options, threads):
        rows = _assert_plan(ctx, n, batch, options, threads, pins, kinds, name)
        members = _members(n, rows[0]["chunk"] if rows[0]["kind"] != ms.SMALL0 else max(count // 8, 2))
        d = ctx.alloc(batch * count * 32)
        try:
            starts = list(range(0, len(members), batch)) + ([len(members)] if len(members) % batch == 0 else [])
            for first in starts:
                mine = members[first:first + batch]
                for b in range(batch):
                    where = ctypes.c_void_p(d.value + b * count * 32)
                    if b < len(mine):
                        ctx.upload(where, mine[b][0])
                    elif first == 0 or b < len(members[first - batch:first]):
                        ctx.fill_table(where, count, _seed(n, b))   # (a seeded table, also where the call before had a member)
                C, L, R = ctx.sumcheck_mle_batch_device(d, n, batch)
                outputs.append((C, L, R))
                for b in range(batch):
                    want = mine[b][1] if b < len(mine) else _seeded(n, _seed(n, b))
                    assert _same((C[b], L[b], R[b]), want), (n, batch, first, b)
                # the inputs are what was uploaded: the members, and a seeded table at either end of the rest
                for b in sorted(set(list(range(min(len(mine), batch))) + [min(len(mine), batch - 1), batch - 1])):
                    got = ctx.download(ctypes.c_void_p(d.value + b * count * 32), (count, 4))
                    assert np.array_equal(got, mine[b][0] if b < len(mine) else cdense.fill_table(count, _seed(n, b))), (n, batch, first, b)
                if batch * count < 1 << 24 and len(mine) < batch:
                    got = ctx.download(d, (batch * count, 4))
                    for b in range(len(mine), batch):
                        assert np.array_equal(got[b * count:(b + 1) * count], cdense.fill_table(count, _seed(n, b))), (n, batch, first, b)
        finally:
            ctx.free(d)
    return outputs


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_either_side_of_a_cut(ctx, case):
    name, n, batch, options, threads, pins, kinds = case
    _run(ctx, n, batch, options, threads, pins, kinds, name)


def test_three_pass0_options_three_rows_same_bytes(ctx):
    """24 x 2^19 in one group: pass0_stream 1, 2 and 3 give k_mle_sub_sums, stream<16, 2> and the rolling form -- three different plan
    rows (asserted), the same bytes."""
    n, batch = 19, 24
    seen, rows = [], []
    for option in (1, 2, 3):
        options = (("group_size", 24), ("pass0_stream", option))
        rows.append(ms.rows_of(n, batch, THREADS, options, 0)[0]["kind"])
        seen.append(_run(ctx, n, batch, options, THREADS, [], None))
    assert rows == [ms.SUB_SUMS, ms.STREAM_16_2, ms.ROLL]
    for other in seen[1:]:
        assert all(_same(a, b) for a, b in zip(seen[0], other))


# fused, then reduce, then fused again; large, then small; flagged, then not flagged: each call meets what the one before left in the
# partials, the records, the tickets and the arrival counters
STALE_SEQUENCE = ["fused-256-blocks-n10-b8", "reduce-288-blocks-n10-b9", "fused-256-blocks-n10-b8", "roll-pub-two-groups-n19", "fused-n13-b4",
                  "roll-reduce-two-groups-n19", "roll-pub-two-groups-n19", "reduce-256-blocks-n16", "fused-128-blocks-n15", "tail-batch-8",
                  "fused-n12-b2", "two-level-n18", "pass0-small-n9"]


def test_stale_state_of_earlier_calls(ctx):
    """The sequence on the module's context (which every case above has used) and on a fresh one: every call against the oracle (in
    _run), and the two runs' bytes equal."""
    by_id = {c[0]: c for c in CASES}
    used = [_run(ctx, *by_id[name][1:]) for name in STALE_SEQUENCE]
    with Context(0) as fresh:
        clean = [_run(fresh, *by_id[name][1:]) for name in STALE_SEQUENCE]
    for name, a, b in zip(STALE_SEQUENCE, used, clean):
        assert len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b)), name

"""tests/mle_shapes.py -- the plain sumcheck's launch plan on plain integers -- against hand-worked rows, against the library's own
report (gkr_selftest_mle_plan: the functions the driver and its launches call, no device) over the whole grid, its invariants over the
same grid, and the cut table it keeps as data against a fresh derivation.  Host only: arithmetic, no GPU."""

import ctypes

import numpy as np
import pytest

import mle_plan as mp
import mle_shapes as ms
from gkr_amd import _native as N


def _pick(row, *fields):
    return tuple(row[f] for f in fields)


# ---- hand-worked rows
def test_headline_1024_tables_of_2_20_on_14_threads():
    """32 GiB of tables: eight groups of 128 (4 GiB each), pass 0 of two queued up front, ten tables per hashing thread at a time.  Pass 0
    has 1024 partials per table for the two-level fold (128 x 1024 = 131 072 partials, chunks of 1024 entries: the deep launch, on the
    rolling form, whose blocks publish flag-in-word records), the fine sums read those 1024 partials on the side stream, the fold of
    ten variables takes 2^15 / 256 = 128 blocks of one tile and leaves 2^10 entries in eight planes, which one late one-block pass
    (S = 32, the sums of rounds 16 - 20) finishes.  Seven folds publish records, the one launched last a reduce."""
    header, rows, _ = ms.plan(20, 1024, 14)
    assert header[:10] == [5, 5, 0, 8, 2, 0, 1, 7, 1, 14]
    assert header[10:19] == [128 * g for g in range(9)] and header[43:51] == [10] * 8 and not any(header[51:])
    assert len(rows) == 8 * 4
    g3 = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == 3]
    assert [r["kind"] for r in g3] == [ms.ROLL_PUB, ms.FINE_SUMS, ms.FOLD2, ms.FOLD_SMALL]
    assert _pick(g3[0], "m_src", "jin", "jout", "nblk", "chunk", "publisher", "stream", "b0", "nb") == (20, 0, 5, 1024, 1024, ms.PUB_FLAGGED, ms.ST_MAIN, 384, 128)
    assert _pick(g3[1], "jin", "jout", "nblk", "publisher", "stream", "plan") == (5, 5, 1024, ms.PUB_SELF, ms.ST_SIDE, ms.PLAN_SIDE)
    assert _pick(g3[2], "jin", "jout", "nblk", "chunk", "publisher", "stream") == (10, 5, 128, 256, ms.PUB_FLAGGED, ms.ST_MAIN)
    assert _pick(g3[3], "m_src", "jin", "jout", "chunk", "stream", "src_planes", "export_tail") == (10, 5, 5, 32, ms.ST_LATE, 8, 0)


def test_4096_tables_of_2_16_sixteen_groups_depth_4():
    """Small tables, a batch of 256 and more: sixteen groups of 256 with pass 0 of four queued ahead, sixteen tables per hash call.  Four
    rounds first (16 - 5 would leave 2^11), 64 blocks of 1024 entries per table: whole 512-entry chunks in a multiple of eight blocks, but
    256 x 64 = 16 384 partials is below 24 576: the shallow pipelined form; then the matrix-core fold to 2^12 in 32 blocks of 128 entries (256 x 32 =
    8192 < 65 536 blocks, but half of 128 is below the 256-entry minimum), plan on the side stream, and two late one-block passes."""
    header, rows, _ = ms.plan(16, 4096, 14)
    assert header[:10] == [5, 4, 0, 16, 4, 0, 0, 0, 0, 14]
    assert header[10:27] == [256 * g for g in range(17)] and header[43:59] == [16] * 16
    g = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == 15]
    assert [r["kind"] for r in g] == [ms.STREAM_8_1, ms.FOLD_MFMA, ms.FOLD_SMALL, ms.FOLD_SMALL]
    assert _pick(g[0], "jout", "nblk", "chunk", "publisher", "b0", "nb") == (4, 64, 1024, ms.PUB_REDUCE, 3840, 256)
    assert _pick(g[1], "m_src", "jin", "jout", "nblk", "chunk", "publisher", "stream", "plan") == (16, 4, 5, 32, 128, ms.PUB_REDUCE, ms.ST_MAIN, ms.PLAN_SIDE)
    assert _pick(g[2], "m_src", "jin", "jout", "chunk", "stream") == (12, 5, 5, 128, ms.ST_LATE)
    assert _pick(g[3], "m_src", "jin", "jout", "chunk", "stream") == (7, 5, 2, 4, ms.ST_LATE)


def test_a_lone_2_20():
    """One group, so no late and no side stream and no flag records; host tail on (batch <= 8) but the two-level schedule 10 | 5 | 5 ends
    on tables of 2^5 entries whose sums cover the last five rounds: no pass left for the host to save.  Pass 0: 2048 blocks of 512 entries (the chip is filled by one table;
    2048 x 1 partials is below the deep threshold: the shallow pipelined form), 32 MiB read but 2048 blocks: a reduce launch."""
    header, rows, _ = ms.plan(20, 1, 14)
    assert header[:10] == [5, 5, 0, 1, 2, 1, 1, 0, 1, 14] and header[10:12] == [0, 1] and header[43] == 8
    g = [dict(zip(ms.ROW_FIELDS, r)) for r in rows]
    assert [r["kind"] for r in g] == [ms.STREAM_8_1, ms.FINE_SUMS, ms.FOLD2, ms.FOLD_SMALL]
    assert _pick(g[0], "nblk", "chunk", "publisher") == (2048, 512, ms.PUB_REDUCE)
    assert _pick(g[1], "nblk", "stream", "plan") == (2048, ms.ST_MAIN, ms.PLAN_OWN)
    assert _pick(g[2], "nblk", "chunk", "publisher") == (128, 256, ms.PUB_REDUCE)
    assert _pick(g[3], "stream", "src_planes", "export_tail") == (ms.ST_MAIN, 8, 0)


def test_a_lone_2_14():
    """64 blocks of 256 entries, 512 KiB read, 64 blocks: the last block publishes, so the launch is k_mle_sub_sums whatever
    pass0_stream says; the fold leaves 2^9 entries: the one-block fold, then 2^4 on the device too (4 rounds cover it: no pass to save)."""
    g = ms.rows_of(14, 1, 14)
    assert [r["kind"] for r in g] == [ms.SUB_SUMS, ms.FOLD_SMALL, ms.FOLD_SMALL]
    assert _pick(g[0], "jout", "nblk", "chunk", "publisher") == (5, 64, 256, ms.PUB_FUSED)
    assert _pick(g[1], "m_src", "jin", "jout", "chunk", "export_tail") == (14, 5, 5, 512, 0)
    assert _pick(g[2], "m_src", "jin", "jout", "chunk", "export_tail") == (9, 5, 4, 16, 0)


def test_5_tables_of_2_17_with_the_host_tail():
    """17 = 5 | 5 | 5 | 2: the fold to 2^7 leaves its tables to the host, which binds the last five variables itself.  Pass 0: 512 blocks of
    256 entries (5 x 512 = 2560 > 256 blocks: a reduce launch; chunk % 512 != 0: the shallow form); the first fold: 32 blocks of 128,
    160 blocks, 20 MiB: its last block publishes."""
    header, rows, _ = ms.plan(17, 5, 14)
    assert header[:10] == [5, 5, 0, 1, 2, 1, 0, 0, 0, 14]
    g = [dict(zip(ms.ROW_FIELDS, r)) for r in rows]
    assert [r["kind"] for r in g] == [ms.STREAM_8_1, ms.FOLD_MFMA, ms.FOLD_SMALL, ms.HOST_FOLD]
    assert _pick(g[0], "nblk", "chunk", "publisher") == (512, 256, ms.PUB_REDUCE)
    assert _pick(g[1], "nblk", "chunk", "publisher", "plan") == (32, 128, ms.PUB_FUSED, ms.PLAN_OWN)
    assert _pick(g[2], "m_src", "jin", "jout", "chunk", "export_tail") == (12, 5, 5, 128, 1)
    assert _pick(g[3], "m_src", "jin", "jout", "chunk", "publisher", "stream") == (7, 5, 2, 4, ms.PUB_HOST, ms.ST_HOST)


def test_a_device_hashed_share():
    """256 x 2^17 on two threads with half the batch hashed on the device: sumchecks 0 .. 127 run as one chain (reported as group 4, on
    the chain's stream, its digit matrices there too), the other 128 in four groups of 32 (host batch 128: ceil(128 / 4))."""
    header, rows, _ = ms.plan(17, 256, 2, (("device_hash_percent", 50),))
    assert header[:10] == [5, 5, 128, 4, 2, 0, 0, 0, 0, 2] and header[10:15] == [128, 160, 192, 224, 256] and header[43:47] == [16] * 4
    chain = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == 4]
    assert [r["kind"] for r in chain] == [ms.STREAM_8_1, ms.FOLD_MFMA, ms.FOLD_SMALL, ms.FOLD_SMALL]
    assert all(_pick(r, "stream", "b0", "nb") == (ms.ST_CHAIN, 0, 128) for r in chain) and chain[1]["plan"] == ms.PLAN_OWN
    first = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == 0]
    assert _pick(first[0], "b0", "nb", "stream") == (128, 32, ms.ST_MAIN) and first[1]["plan"] == ms.PLAN_SIDE and first[2]["stream"] == ms.ST_LATE


# ---- the grid: one walk, shared
class _Sweep:
    def __init__(self):
        lib = N.lib()
        header = np.zeros(ms.HEADER_WORDS, dtype=np.uint32)
        rows = np.zeros((mp.ROW_CAPACITY, ms.ROW_WORDS), dtype=np.uint32)
        n_rows = ctypes.c_size_t()
        hp, rp, np_ = header.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_rows)
        self.shapes, self.differ, self.broken = 0, [], []
        arrays, marshalled = {}, {}

        def visit(shape, want_header, want_rows):
            n, batch, threads, options = shape
            if options not in marshalled:
                names = (ctypes.c_char_p * max(len(options), 1))(*[k.encode() for k, _ in options])
                values = (ctypes.c_longlong * max(len(options), 1))(*[v for _, v in options])
                marshalled[options] = (names, values, ctypes.cast(names, ctypes.c_void_p), ctypes.cast(values, ctypes.c_void_p))
            _, _, names, values = marshalled[options]
            rc = lib.gkr_selftest_mle_plan(n, batch, threads, names, values, len(options), hp, rp, mp.ROW_CAPACITY, np_)
            if id(want_rows) not in arrays:
                arrays[id(want_rows)] = (want_rows, np.array(want_rows, dtype=np.uint32).reshape(-1, ms.ROW_WORDS))
            want = arrays[id(want_rows)][1]
            self.shapes += 1
            if rc != 0 or n_rows.value != len(want) or header.tolist() != want_header or not np.array_equal(rows[:len(want)], want):
                self.differ.append(shape)
            groups, n_dev = want_header[3], want_header[2]
            bound = want_header[10:11 + groups]
            if bound[0] != n_dev or bound[-1] != batch or any(a >= b for a, b in zip(bound, bound[1:])) or groups > ms.MAX_GROUPS:
                self.broken.append((shape, "the bounds partition [n_dev, batch)"))

        self.best = ms.derive_cut_table(visit)
        for key, (group_rows, _) in ms.GROUP_PLANS.items():
            self.broken += [(key, why) for why in _invariants(key[0], group_rows)]


def _invariants(n, rows):
    """What must hold of every group's passes, from the model's rows: the names of what does not."""
    R = [dict(zip(ms.ROW_FIELDS, r)) for r in rows]
    if sum(r["jout"] for r in R) != n:
        yield "rounds sum to n in every group"
    for i, r in enumerate(R):
        kind, nblk, chunk, nb = r["kind"], r["nblk"], r["chunk"], r["nb"]
        out = r["m_src"] - r["jin"] if kind >= ms.FOLD_SMALL else r["m_src"]
        if not 1 <= nblk <= ms.MAX_BLOCKS_PER_TABLE:
            yield "nblk <= 2048"
        if kind in (ms.SUB_SUMS, ms.STREAM_8_1, ms.STREAM_16_2, ms.ROLL, ms.ROLL_PUB, ms.FOLD_MFMA, ms.FOLD_VALU):
            if nblk * chunk != 1 << out:
                yield "blocks x entries per block = the entries of the pass"
            if nblk < 1 << r["jout"] or nblk & (nblk - 1):
                yield "a block lies in one sub-block: nblk a power of two >= 2^jout"
        if kind == ms.STREAM_8_1 and (chunk % 256 or nblk % 4 or r["publisher"] != ms.PUB_REDUCE):
            yield "the shallow pipelined form's divisibility"
        if kind in (ms.STREAM_16_2, ms.ROLL, ms.ROLL_PUB) and (chunk % 512 or nblk % 8 or nblk * nb < ms.PASS0_DEEP_MIN_PARTIALS or r["publisher"] == ms.PUB_FUSED):
            yield "the deep forms' divisibility and partial count"
        if kind == ms.ROLL_PUB and (nblk != 4 * ms.FLAG_RECS_PER_TABLE or r["publisher"] != ms.PUB_FLAGGED or R[i + 1]["kind"] != ms.FINE_SUMS):
            yield "the publishing rolling form: 1024 partials ahead of the fine sums"
        if (r["publisher"] == ms.PUB_FLAGGED) != (kind == ms.ROLL_PUB or (kind == ms.FOLD2 and r["publisher"] == ms.PUB_FLAGGED)):
            yield "flag-in-word records come from the two publishing kernels"
        if kind == ms.FOLD_MFMA and chunk % 64:
            yield "the matrix-core fold: whole 64-entry tiles"
        if r["publisher"] == ms.PUB_FUSED and (r["b0"] + nb > ms.ARRIVAL_COUNTERS or nblk > 128 or nblk * nb > ms.FUSED_PUBLISH_BLOCKS):
            yield "b0 + nb <= 4096 (and the block limits) wherever the last block publishes"
        if kind == ms.FINE_SUMS and (nblk % 1024 or chunk % 256 or nblk * chunk != 1 << n or R[i - 1]["nblk"] != nblk or R[i + 1]["kind"] != ms.FOLD2):
            yield "the fine sums see a multiple of 1024 partials of whole 256-entry chunks, pass 0's, ahead of the two-level fold"
        if kind == ms.FOLD2 and (nblk * chunk != 1 << (n - 5) or not 18 <= n <= 24 or R[i + 1]["src_planes"] != ms.FOLD2_PLANES):
            yield "the two-level fold: 18 <= n <= 24, its planes read by the next pass"
        if r["src_planes"] != 1 and (kind != ms.FOLD_SMALL or r["m_src"] != n - 10 or R[i - 1]["kind"] != ms.FOLD2):
            yield "planes are read by the one-block fold behind the two-level fold"
        if r["export_tail"] and (kind != ms.FOLD_SMALL or out > ms.TAIL_LOG2 or R[i + 1]["kind"] != ms.HOST_FOLD):
            yield "the host tail takes tables of 2^7 entries and fewer from a one-block fold"
        if kind == ms.HOST_FOLD and not (R[i - 1]["export_tail"] or R[i - 1]["kind"] == ms.HOST_FOLD):
            yield "the host folds what was exported"
        if kind in (ms.SMALL0, ms.FOLD_SMALL) and chunk > ms.SMALL_PASS_ENTRIES:
            yield "the one-block kernels: at most 512 entries"


@pytest.fixture(scope="module")
def sweep():
    return _Sweep()


def test_model_equals_library_over_the_grid(sweep):
    """n = 2 .. 30, every batch of GRID_BATCHES the ABI admits, 1 / 2 / 3 / 4 / 14 threads, every option set of GRID_OPTIONS: header and rows."""
    assert sweep.shapes > 150_000
    assert not sweep.differ, (len(sweep.differ), sweep.differ[:5])


def test_invariants_over_the_grid(sweep):
    assert not sweep.broken, (len(sweep.broken), sweep.broken[:5])


def test_cut_table_is_complete_and_minimal(sweep):
    """CUT_TABLE has an entry for every comparison the model records (mle_shapes.CUTS) and for nothing else; each side holds the
    smallest shape of the grid that meets it, as a fresh derivation finds it, or a reason where the grid has none."""
    assert len(set(ms.CUTS)) == len(ms.CUTS) and set(ms.CUTS) == set(ms.CUT_TABLE), (set(ms.CUTS) ^ set(ms.CUT_TABLE))
    # (every name is a comparison the model makes: _Trace.cut refuses a name that is not in CUTS, and each is met or carries a reason)
    for name, sides in ms.CUT_TABLE.items():
        assert set(sides) == {False, True}, name
        for outcome, entry in sides.items():
            found = sweep.best.get(name, {}).get(outcome)
            if isinstance(entry, str):
                assert found is None and len(entry) > 20, (name, outcome, found)
            else:
                assert entry == found, (name, outcome, entry, found)


def test_cut_table_entries_meet_their_cut():
    for name, sides in ms.CUT_TABLE.items():
        for outcome, entry in sides.items():
            if not isinstance(entry, str):
                assert (name, outcome) in ms.plan(*entry)[2], (name, outcome)


def test_what_the_search_found_against_what_was_expected():
    """Expected unreachable, found reachable: a launch kept from publishing from its last block by its arrival counters ALONE.  A fused
    launch has nblk x nb <= 256, so a small group -- and with a device-hashed share the host-hashed groups are small AND start high in the
    batch: 4097 x 2^10, 90 % on the device, leaves sixteen groups of 26 or 27 from sumcheck 3680 on, the last one [4070, 4097).
    Expected reachable by geometry, found unreachable: the v_mad_u64_u32 fold without option no_mfma_fold."""
    n, batch, threads, options = ms.CUT_TABLE["fused: b0 + nb <= 4096"][False]
    assert (n, batch, dict(options)) == (10, 4097, {"device_hash_percent": 90, "rounds_per_pass": 3})
    last = ms.rows_of(n, batch, threads, options, group=15)[0]
    assert _pick(last, "kind", "nblk", "b0", "nb", "publisher") == (ms.SUB_SUMS, 8, 4070, 27, ms.PUB_REDUCE)
    assert ms.rows_of(n, batch, threads, options, group=14)[0]["publisher"] == ms.PUB_FUSED
    assert isinstance(ms.CUT_TABLE["fold.mfma: (S / nblk) % 64 == 0"][False], str)


# ---- the entry points' argument checks
def test_plan_entry_points_check_their_arguments():
    assert "gkr_selftest_mle_plan" in N.SYMBOLS and "gkr_selftest_mle_plan_ctx" in N.SYMBOLS
    lib = N.lib()
    header = np.zeros(ms.HEADER_WORDS, dtype=np.uint32)
    n_rows = ctypes.c_size_t()
    hp, cnt = header.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_rows)
    assert lib.gkr_selftest_mle_plan(20, 1024, 14, None, None, 0, hp, None, 0, cnt) == 0 and n_rows.value == 32   # (the count alone)
    for n, batch, threads in ((1, 1, 1), (31, 1, 1), (20, 1025, 1), (2, 0, 1), (2, 65536, 1), (2, 1, 0), (2, 1, 257)):
        assert lib.gkr_selftest_mle_plan(n, batch, threads, None, None, 0, hp, None, 0, cnt) == N.GKR_ERR_INVALID, (n, batch, threads)
    assert lib.gkr_selftest_mle_plan(2, 1, 1, None, None, 0, None, None, 0, cnt) == N.GKR_ERR_INVALID
    assert lib.gkr_selftest_mle_plan(2, 1, 1, None, None, 0, hp, None, 0, None) == N.GKR_ERR_INVALID
    assert lib.gkr_selftest_mle_plan(2, 1, 1, None, None, 0, hp, None, 4, cnt) == N.GKR_ERR_INVALID
    assert lib.gkr_selftest_mle_plan(2, 1, 1, None, None, 1, hp, None, 0, cnt) == N.GKR_ERR_INVALID
    with pytest.raises(AssertionError):
        mp.library_plan(2, 1, 1, (("no_such_option", 1),))
    assert lib.gkr_selftest_mle_plan_ctx(None, 2, 1, hp, None, 0, cnt) == N.GKR_ERR_INVALID
    # the environment's name of an option is accepted as gkr_ctx_set_option accepts it
    assert mp.library_plan(20, 4, 14, (("GKR_GROUP_SIZE", 1),)) == mp.library_plan(20, 4, 14, (("group_size", 1),))


# ---- the GPU cases (tests/test_gpu_mle_plan.py CASES is data): on their cuts, and between them on every reachable side
def test_gpu_cases_meet_the_cuts_they_name_and_cover_the_table():
    import test_gpu_mle_plan as gpu
    covered = set()
    for name, n, batch, options, threads, pins, kinds in gpu.CASES:
        assert ms.admissible(n, batch), name
        header, rows, hits = ms.plan(n, batch, threads, options)
        gpu.check_pins(name, header, rows)
        assert pins or kinds is not None or name in gpu.ROW_PINS or name in gpu.HEADER_PINS, name   # (no case asserts model == library alone)
        for pin in pins:
            assert pin in hits, (name, pin)
        if kinds is not None:
            assert ms.kinds(n, batch, threads, options) == kinds, (name, ms.kinds(n, batch, threads, options))
        covered |= hits
    assert set(gpu.ROW_PINS) | set(gpu.HEADER_PINS) <= set(gpu.CASE_IDS)
    assert len(set(gpu.CASE_IDS)) == len(gpu.CASES) and set(gpu.STALE_SEQUENCE) <= set(gpu.CASE_IDS)
    missing = [(name, outcome) for name, sides in ms.CUT_TABLE.items() for outcome, entry in sides.items()
               if not isinstance(entry, str) and (name, outcome) not in covered]
    # 16 GiB of tables (4096 x 2^17, the smallest call with four whole 4 GiB groups): asserted on the host alone, as the headline's plan is
    assert missing == [("groups: fewer than four 4 GiB groups", False), ("groups: more than eight 4 GiB groups", False)], missing

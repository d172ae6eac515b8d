"""The launch plan of the plain sumcheck's multi-round driver (csrc/capi_mle_passes.hip, the k_mle_* launches of csrc/kernels.hip)
restated on plain integers, from the comments and constants of that code: the schedule of a batch, and per (group, pass) the kernel
form, its blocks, who publishes its sums, the stream.  Nothing here calls the library; tests/test_mle_shapes_host.py holds this model
against the library's own report (gkr_selftest_mle_plan, tests/mle_plan.py) over a grid, and the GPU cases pin their shapes with it.

Every comparison of the decision code is a CUT: the model records each one it evaluates, with its outcome, under the cut's name
(`_Trace.cut`).  CUT_TABLE holds, per cut, the smallest shape of the grid on either side -- derived by derive_cut_table(), kept as data,
re-derived by the host test -- or why a side cannot be reached.  CUTS lists the names; a comparison recorded under another name is an error.

Comparisons that are deliberately NOT cuts, and why: the arithmetic of the block counts (blocks_per_table: items_per_block, the 2048 / batch
fill, the 256-entry floor, the 2048 cap; pass_blocks' doubling loop) -- they have no two outcomes that select a kernel, only a value, nblk,
which every row reports and the grid holds against the library at 212 850 shapes, and whose consequences ARE cuts (nblk % 4, nblk % 8,
nblk * nb <= 256, nblk <= 128, nblk == 1024); `want < 16` in the few-threads rule (true whenever the rule's other two comparisons are, unless
small_tables already made it 16: the same sixteen groups either way); the group size of 64 with a device-hashed share on few threads (a value,
reported as the bounds; the option tables of the grid reach it at 256 x 2^n on 2 threads with device_hash_percent); the option tests
(an option is 0 or not: the grid's option sets are their either side)."""

import functools

# ---- constants (kernels.h, capi_internal.h, capi_mle_passes.hip, flagged_rec.h)
SMALL_PASS_ENTRIES = 512
MAX_BLOCKS_PER_TABLE = 2048
MAX_GROUPS = 32
PASS_MAX_ROUNDS = 5
TWO_LEVEL_ROUNDS = 10
TAIL_LOG2 = 7
FUSED_PUBLISH_BYTES = 64 << 20
FUSED_PUBLISH_BLOCKS = 256
ARRIVAL_COUNTERS = 4096
FLAG_RECS_PER_TABLE = 256
PASS0_DEEP_MIN_PARTIALS = 2 * 12 * 256 * 4
FOLD2_PLANES = 8
MAX_N, MAX_BATCH, MAX_VALUES = 30, 65535, 1 << 30

# kinds, publishers, streams, plan placements (include/gkr_amd.h GKR_MLE_*)
SMALL0, SUB_SUMS, STREAM_8_1, STREAM_16_2, ROLL, ROLL_PUB, FINE_SUMS, FOLD2, FOLD_SMALL, FOLD_MFMA, FOLD_VALU, HOST_FOLD = range(12)
PUB_SELF, PUB_FUSED, PUB_REDUCE, PUB_FLAGGED, PUB_HOST = range(5)
ST_MAIN, ST_LATE, ST_SIDE, ST_CHAIN, ST_HOST = range(5)
PLAN_NONE, PLAN_OWN, PLAN_SIDE = range(3)
ROW_FIELDS = ("group", "pass", "kind", "m_src", "jin", "jout", "nblk", "chunk", "publisher", "stream", "plan", "export_tail", "src_planes",
              "b0", "nb", "zero")
HEADER_WORDS, ROW_WORDS = 80, 16

# the options the plan reads, all 0 by default (options.h)
OPTIONS = ("rounds_per_pass", "no_mfma_fold", "first_fold_levels", "pass0_stream", "fold2_tiles", "stream_publish", "no_fused_reduce",
           "hash_chunk", "device_hash_percent", "group_size", "pass_queue_depth", "no_late_stream", "plan_main", "fold_blocks",
           "fold_min_chunk", "items_per_block", "host_tail_log2", "host_tail_max_batch")


def admissible(n, batch):
    return 2 <= n <= MAX_N and 1 <= batch <= MAX_BATCH and (batch << n) <= MAX_VALUES


CUTS = (
    "arrivals: table <= 64 MiB",
    "device_hash: batch >= 64", "device_hash: batch - n_dev < 16", "device_hash: n_dev < 8",
    "groups: fewer than four 4 GiB groups", "groups: more than eight 4 GiB groups", "groups: more than 96 GiB",
    "groups.small_tables: n <= 17", "groups.small_tables: host batch >= 256", "groups.few_threads: threads <= 3",
    "groups.few_threads: host batch >= 256", "groups.size: host batch >= 128", "groups.size: host batch >= 16", "groups.cap: more than 32",
    "hash_chunk: nb >= 32 threads", "hash_chunk: per thread <= 8", "hash_chunk: per thread <= 16",
    "host_tail: batch <= 8 (host_tail_max_batch)", "host_tail: m <= 7", "host_tail: m - j > 0",
    "rounds.whole_tiles: j > m - 6", "rounds.leave_2^10_or_2^11", "two_level: n >= 18", "two_level: n <= 24",
    "pass0.small: len <= 512", "pass0.two_level: chunk < 256", "pass0.stream: chunk % 256 == 0", "pass0.stream: nblk % 4 == 0",
    "pass0.deep: chunk % 512 == 0", "pass0.deep: nblk % 8 == 0", "pass0.deep: batch * nblk >= 24576",
    "pass0.flagged: j == 5", "pass0.flagged: nblk == 1024",
    "fused: b0 + nb <= 4096", "fused: bytes read <= 64 MiB", "fused: nblk * nb <= 256", "fused: nblk <= 128",
    "streams: more than one group", "fold.late: m_src != n", "fold.late: m_src <= 16", "fold.small: S <= 512", "fold.mfma: (S / nblk) % 64 == 0",
    "fold_blocks.target: blocks over the batch < target", "fold_blocks.min_chunk: half the chunk >= the minimum",
    "fold_blocks.cap: twice the blocks <= 2048",
    "fold2.flagged: 256 partials per table", "fold2.flagged: partials of >= 16 entries",
)
_CUT_SET = frozenset(CUTS)


class _Trace:
    """The comparisons one evaluation of the model went through: (cut name, outcome) pairs."""

    def __init__(self):
        self.hits = set()

    def cut(self, name, outcome):
        assert name in _CUT_SET, name
        self.hits.add((name, bool(outcome)))
        return bool(outcome)


class _Opts:
    def __init__(self, pairs):
        self.d = dict.fromkeys(OPTIONS, 0)
        for k, v in pairs:
            if k not in self.d:
                raise KeyError(k)
            self.d[k] = v

    def __getitem__(self, k):
        return self.d[k]


# ---- rounds per pass (capi_internal.h mle_pass_rounds, mle_two_level_first_fold)
def pass_rounds(m, n, jmax, t):
    j = min(m, jmax)
    if (1 << m) > SMALL_PASS_ENTRIES and m != n and t.cut("rounds.whole_tiles: j > m - 6", j > m - 6):
        j = m - 6
    if jmax > 3 and t.cut("rounds.leave_2^10_or_2^11", m - j in (10, 11)) and m - 12 >= 1:
        j = m - 12
    return max(j, 1)


def two_level(n, o, t):
    levels = o["first_fold_levels"] if o["first_fold_levels"] in (1, 2) else 2
    if levels != 2 or o["no_mfma_fold"] or o["rounds_per_pass"] > 0:
        return False
    return t.cut("two_level: n >= 18", n >= 18) and t.cut("two_level: n <= 24", n <= 24)


# ---- blocks (kernels.hip mle_blocks_per_table, mle_pass_blocks, mle_multifold_blocks, mle_multifold_uses_mfma)
def blocks_per_table(items, batch, o):
    per_block = o["items_per_block"] if o["items_per_block"] >= 256 else 1024
    b = (items + per_block - 1) // per_block
    b = max(b, (2048 + batch - 1) // batch)
    b = min(b, (items + 255) // 256, MAX_BLOCKS_PER_TABLE)
    return max(b, 1)


def pass_blocks(items, jout, batch, o):
    want = blocks_per_table(items, batch, o)
    b = 1 << jout
    while b < want and b * 2 <= items and b * 2 <= MAX_BLOCKS_PER_TABLE:
        b <<= 1
    return min(b, items)


def multifold_blocks(S, jout, batch, o, t):
    if o["no_mfma_fold"]:
        return pass_blocks(S, jout, batch, o)
    target = o["fold_blocks"] if o["fold_blocks"] > 0 else 65536
    mc = o["fold_min_chunk"]
    min_chunk = mc if mc >= 64 and mc & (mc - 1) == 0 else 256
    b = 1 << jout
    while True:
        # (the loop stops at the first of its three conditions to fail, tested in this order)
        if not t.cut("fold_blocks.target: blocks over the batch < target", b * batch < target):
            break
        if not t.cut("fold_blocks.min_chunk: half the chunk >= the minimum", S // (2 * b) >= min_chunk):
            break
        if not t.cut("fold_blocks.cap: twice the blocks <= 2048", 2 * b <= MAX_BLOCKS_PER_TABLE):
            break
        b <<= 1
    return min(b, S)


def uses_mfma(S, nblk, o, t):
    if o["no_mfma_fold"]:
        return False
    return t.cut("fold.mfma: (S / nblk) % 64 == 0", nblk > 0 and S % nblk == 0 and (S // nblk) % 64 == 0)


def stream_form(length, batch, nblk, publishes, o, t):
    want = o["pass0_stream"] if 1 <= o["pass0_stream"] <= 3 else 3
    if want < 2 or publishes or nblk == 0 or length % nblk:
        return 0
    chunk = length // nblk
    if (t.cut("pass0.deep: chunk % 512 == 0", chunk % 512 == 0) and t.cut("pass0.deep: nblk % 8 == 0", nblk % 8 == 0)
            and t.cut("pass0.deep: batch * nblk >= 24576", batch * nblk >= PASS0_DEEP_MIN_PARTIALS)):
        return 3 if want == 3 else 2
    return 1 if t.cut("pass0.stream: chunk % 256 == 0", chunk % 256 == 0) and t.cut("pass0.stream: nblk % 4 == 0", nblk % 4 == 0) else 0


def fold2_partials(S):
    I = S >> 5
    sub = I >> 5
    return 8 * (I // min(sub, 64))


def fold2_tiles(S, o):
    tiles, T = S >> 11, 1
    while 2 * T <= tiles and 2 * T <= o["fold2_tiles"]:
        T <<= 1
    return T


def fold2_publishes_flagged(S, t):
    return t.cut("fold2.flagged: 256 partials per table", fold2_partials(S) == FLAG_RECS_PER_TABLE) and \
        t.cut("fold2.flagged: partials of >= 16 entries", (S >> 10) >= 16)


def fused_applies(arrivals, b0, nb, nblk, bytes_read, t):
    """The last block publishes: four conditions, all of which must hold.  A condition is recorded as met with outcome False only where
    it ALONE keeps the launch from publishing (the others hold), with outcome True where the launch publishes."""
    if not arrivals:
        return False
    tests = (("fused: b0 + nb <= 4096", b0 + nb <= ARRIVAL_COUNTERS), ("fused: bytes read <= 64 MiB", bytes_read <= FUSED_PUBLISH_BYTES),
             ("fused: nblk * nb <= 256", nblk * nb <= FUSED_PUBLISH_BLOCKS), ("fused: nblk <= 128", nblk <= 128))
    failed = [name for name, ok in tests if not ok]
    if not failed:
        for name, _ in tests:
            t.cut(name, True)
    elif len(failed) == 1:
        t.cut(failed[0], False)
    return not failed


# ---- the schedule of a batch (capi_mle_passes.hip mle_schedule)
def schedule(n, batch, threads, o, t):
    sc = {}
    jcap = 3 if o["no_mfma_fold"] else PASS_MAX_ROUNDS
    jwant = o["rounds_per_pass"] if o["rounds_per_pass"] > 0 else jcap
    sc["jmax"] = min(jwant, jcap)
    sc["j_first"] = pass_rounds(n, n, sc["jmax"], t)
    sc["two_level"] = two_level(n, o, t)
    dev_percent = min(max(o["device_hash_percent"], 0), 90)
    n_dev = 0
    if dev_percent > 0 and t.cut("device_hash: batch >= 64", batch >= 64):
        n_dev = (batch * dev_percent // 100) & ~7
        if t.cut("device_hash: batch - n_dev < 16", batch - n_dev < 16):
            n_dev = (batch - 16) & ~7
        if t.cut("device_hash: n_dev < 8", n_dev < 8):
            n_dev = 0
    sc["n_dev"] = n_dev
    hb = batch - n_dev
    gib4 = ((hb << n) * 32) >> 32
    if t.cut("groups: fewer than four 4 GiB groups", gib4 < 4):
        want = 4
    elif t.cut("groups: more than eight 4 GiB groups", gib4 > 8):
        want = 16 if t.cut("groups: more than 96 GiB", (hb << n) * 32 > 96 << 30) else 8
    else:
        want = gib4
    small_tables = t.cut("groups.small_tables: n <= 17", n <= 17) and t.cut("groups.small_tables: host batch >= 256", hb >= 256)
    if small_tables:
        want = 16
    if t.cut("groups.few_threads: threads <= 3", threads <= 3) and t.cut("groups.few_threads: host batch >= 256", hb >= 256) and want < 16:
        want = 16
    if t.cut("groups.size: host batch >= 128", hb >= 128):
        gs = (hb + want - 1) // want
    elif t.cut("groups.size: host batch >= 16", hb >= 16):
        gs = (hb + 1) // 2
    else:
        gs = hb
    if n_dev and threads <= 3 and hb >= 256:
        gs = 64
    if o["group_size"] > 0:
        gs = o["group_size"]
    groups = (hb + gs - 1) // gs
    if t.cut("groups.cap: more than 32", groups > MAX_GROUPS):
        groups = MAX_GROUPS
    sc["groups"] = groups
    sc["bound"] = [n_dev + hb * g // groups for g in range(groups + 1)]
    forced = o["hash_chunk"]
    sc["chunk"] = []
    for g in range(groups):
        nb = sc["bound"][g + 1] - sc["bound"][g]
        per = (nb + threads - 1) // threads
        if forced in (8, 16):
            c = forced
        elif t.cut("hash_chunk: nb >= 32 threads", nb >= 32 * threads):
            c = 16
        elif t.cut("hash_chunk: per thread <= 8", per <= 8):
            c = 8
        else:
            c = per if t.cut("hash_chunk: per thread <= 16", per <= 16) else 16
        sc["chunk"].append(c)
    sc["depth"] = o["pass_queue_depth"] if o["pass_queue_depth"] > 0 else (4 if small_tables else 2)
    max_tail = o["host_tail_max_batch"] if o["host_tail_max_batch"] > 0 else 8
    sc["tail_on"] = o["host_tail_log2"] >= 0 and n_dev == 0 and t.cut("host_tail: batch <= 8 (host_tail_max_batch)", batch <= max_tail)
    return sc


# ---- the passes of one group (MlePassRun::step and what it launches; queue_device_chain for the device-hashed share)
def _group_rows(n, b0, nb, chain, okey, jmax, j_first, two, groups, tail_on):
    """Rows without their group index, and the cuts met: a function of these arguments alone (cached)."""
    o, t = _Opts(okey), _Trace()
    length = 1 << n
    arrivals = o["no_fused_reduce"] == 0 and t.cut("arrivals: table <= 64 MiB", length * 32 <= FUSED_PUBLISH_BYTES)
    two = two and not chain
    several = t.cut("streams: more than one group", groups > 1)   # (the late stream, the side stream and the flag records all ask this)
    late_stream = not o["no_late_stream"] and several
    side = not o["plan_main"] and several
    flag_records = o["stream_publish"] != 1 and two and several
    own = ST_CHAIN if chain else ST_MAIN
    rows = []

    def row(kind, m_src, jin, jout, nblk, chunk, publisher, stream, plan=PLAN_NONE, export=0, planes=1):
        rows.append([0, len(rows), kind, m_src, jin, jout, nblk, chunk, publisher, stream, plan, int(export), planes, b0, nb, 0])

    def pass0_nblk(jout, blocks_jout):
        nblk = pass_blocks(length, blocks_jout if blocks_jout else jout, nb, o)
        if blocks_jout and t.cut("pass0.two_level: chunk < 256", length // nblk < 256):
            nblk = length // 256
        return nblk

    m, j = n, j_first
    if t.cut("pass0.small: len <= 512", length <= SMALL_PASS_ENTRIES):
        row(SMALL0, n, 0, j, 1, length, PUB_SELF, own)
    else:
        nblk = pass0_nblk(j, TWO_LEVEL_ROUNDS if two else 0)
        fused = fused_applies(arrivals, b0, nb, nblk, nb * length * 32, t)
        form = stream_form(length, nb, nblk, fused, o, t)
        flagged = flag_records and t.cut("pass0.flagged: j == 5", j == PASS_MAX_ROUNDS) and not fused and form == 3 and \
            t.cut("pass0.flagged: nblk == 1024", nblk == 4 * FLAG_RECS_PER_TABLE)
        row(ROLL_PUB if flagged else SUB_SUMS + form, n, 0, j, nblk, length // nblk, PUB_FUSED if fused else (PUB_FLAGGED if flagged else PUB_REDUCE), own)
    planes = on_host = False
    while m - j > 0:
        if m == n and two:
            nblk0 = pass0_nblk(j, TWO_LEVEL_ROUNDS)
            row(FINE_SUMS, n, j, PASS_MAX_ROUNDS, nblk0, length // nblk0, PUB_SELF, ST_SIDE if side else ST_MAIN, PLAN_SIDE if side else PLAN_OWN)
            S = 1 << (n - PASS_MAX_ROUNDS)
            T = fold2_tiles(S, o)
            pub = PUB_FLAGGED if flag_records and fold2_publishes_flagged(S, t) else PUB_REDUCE
            row(FOLD2, n, TWO_LEVEL_ROUNDS, PASS_MAX_ROUNDS, (S >> 8) // T, 256 * T, pub, ST_MAIN)
            m, j, planes, on_host = n - TWO_LEVEL_ROUNDS, PASS_MAX_ROUNDS, True, False
            continue
        m_src, jin = m, j
        m -= jin
        j = pass_rounds(m, n, jmax, t)
        if on_host:
            row(HOST_FOLD, m_src, jin, j, 1, 1 << m, PUB_HOST, ST_HOST)
            continue
        if chain:
            stream = ST_CHAIN
        else:
            late = t.cut("fold.late: m_src != n", m_src != n) and t.cut("fold.late: m_src <= 16", m_src <= 16)
            stream = ST_LATE if late and late_stream else ST_MAIN
        on_host = tail_on and not chain and t.cut("host_tail: m <= 7", m <= TAIL_LOG2) and t.cut("host_tail: m - j > 0", m - j > 0)
        S = 1 << m
        if t.cut("fold.small: S <= 512", S <= SMALL_PASS_ENTRIES):
            row(FOLD_SMALL, m_src, jin, j, 1, S, PUB_SELF, stream, PLAN_NONE, on_host, FOLD2_PLANES if planes else 1)
        else:
            nblk = multifold_blocks(S, j, nb, o, t)
            mfma = uses_mfma(S, nblk, o, t)
            fused = fused_applies(arrivals, b0, nb, nblk, nb * (1 << m_src) * 32, t)
            plan = PLAN_NONE if not mfma else (PLAN_SIDE if stream == ST_MAIN and side else PLAN_OWN)
            row(FOLD_MFMA if mfma else FOLD_VALU, m_src, jin, j, nblk, S // nblk, PUB_FUSED if fused else PUB_REDUCE, stream, plan, 0,
                FOLD2_PLANES if planes else 1)
        planes = False
    return tuple(tuple(r) for r in rows), frozenset(t.hits)


GROUP_PLANS = {}   # every group the model has planned so far: _group_rows' arguments -> (rows, hits)
_assembled = {}


def _group_rows_cached(*key):
    if key not in GROUP_PLANS:
        GROUP_PLANS[key] = _group_rows(*key)
    return GROUP_PLANS[key]


@functools.lru_cache(maxsize=None)
def _options(options):
    okey = tuple(sorted(dict(options).items()))
    return okey, _Opts(okey)


def plan(n, batch, threads, options=()):
    """(header, rows, hits): the 80 header words and the 16-word rows (a tuple, shared between calls) gkr_selftest_mle_plan reports for (n, batch, threads) with the
    (name, value) pairs of `options` laid over the defaults, and the (cut, outcome) pairs the decisions went through."""
    assert admissible(n, batch) and threads >= 1
    (okey, o), t = _options(tuple(options)), _Trace()
    sc = schedule(n, batch, threads, o, t)
    key = (n, okey, tuple(sc["bound"]), sc["jmax"], sc["j_first"], sc["two_level"], sc["tail_on"])
    if key not in _assembled:
        rows, hits = [], set()
        groups = [(g, sc["bound"][g], sc["bound"][g + 1] - sc["bound"][g], False) for g in range(sc["groups"])]
        if sc["n_dev"]:
            groups.append((sc["groups"], 0, sc["n_dev"], True))
        for g, b0, nb, chain in groups:
            # (b0 enters through one comparison only, b0 + nb <= 4096, and as a reported word)
            r, h = _group_rows_cached(n, 0 if b0 + nb <= ARRIVAL_COUNTERS else b0, nb, chain, okey, sc["jmax"], sc["j_first"], sc["two_level"],
                                      sc["groups"], sc["tail_on"])
            rows += [(g,) + x[1:13] + (b0,) + x[14:] for x in r]
            hits |= h
        _assembled[key] = (tuple(rows), frozenset(hits))
    rows, hits = _assembled[key]
    hits = hits | t.hits
    S = 1 << max(n - PASS_MAX_ROUNDS, 0)
    flags = sc["two_level"] and o["stream_publish"] != 1 and sc["groups"] > 1 and fold2_partials(S) == FLAG_RECS_PER_TABLE and (S >> 10) >= 16
    header = [sc["jmax"], sc["j_first"], sc["n_dev"], sc["groups"], sc["depth"], int(sc["tail_on"]), int(sc["two_level"]),
              sc["groups"] - 1 if flags else 0, (1 if flags else sc["groups"]) if sc["two_level"] else 0, threads]
    header += sc["bound"] + [0] * (MAX_GROUPS + 1 - len(sc["bound"])) + sc["chunk"] + [0] * (MAX_GROUPS - len(sc["chunk"]))
    header += [0] * (HEADER_WORDS - len(header))
    return header, rows, hits


def rows_of(n, batch, threads, options=(), group=None):
    """The plan's rows as dicts over ROW_FIELDS (of one group, if given)."""
    return [dict(zip(ROW_FIELDS, r)) for r in plan(n, batch, threads, options)[1] if group is None or r[0] == group]


def kinds(n, batch, threads, options=(), group=0):
    return [r["kind"] for r in rows_of(n, batch, threads, options, group)]


# ---- the grid the model is held against the library on, and the cuts are searched on
GRID_BATCHES = sorted(set(list(range(1, 10)) + [15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513,
                                                 4095, 4096, 4097, 65535]))
GRID_THREADS = (1, 2, 3, 4, 14)
# each option alone at the values tests/test_gpu_parity.py uses, and that module's combinations
GRID_OPTIONS = (
    (), (("no_mfma_fold", 1),), (("rounds_per_pass", 1),), (("rounds_per_pass", 2),), (("rounds_per_pass", 3),), (("rounds_per_pass", 4),),
    (("first_fold_levels", 1),),
    (("first_fold_levels", 2),), (("pass0_stream", 1),), (("pass0_stream", 2),), (("pass0_stream", 3),), (("stream_publish", 1),),
    (("stream_publish", 2),), (("no_fused_reduce", 1),), (("group_size", 1),), (("group_size", 2),), (("group_size", 3),), (("group_size", 24),), (("group_size", 64),),
    (("pass_queue_depth", 1),), (("pass_queue_depth", 16),), (("device_hash_percent", 10),), (("device_hash_percent", 25),), (("device_hash_percent", 50),),
    (("device_hash_percent", 90),), (("fold_blocks", 8192),), (("fold_blocks", 2048),), (("fold_min_chunk", 64),), (("fold_min_chunk", 4096),),
    (("items_per_block", 256),), (("items_per_block", 768),), (("host_tail_log2", -1),), (("host_tail_max_batch", 2),),
    (("host_tail_max_batch", 64),), (("no_late_stream", 1),), (("plan_main", 1),), (("hash_chunk", 8),), (("hash_chunk", 16),),
    (("fold2_tiles", 4),),
    (("no_mfma_fold", 1), ("rounds_per_pass", 2)), (("no_mfma_fold", 1), ("pass0_stream", 2)), (("group_size", 3), ("pass_queue_depth", 1)),
    (("group_size", 3), ("pass_queue_depth", 16)), (("group_size", 24), ("pass0_stream", 2)), (("group_size", 24), ("stream_publish", 1)),
    (("device_hash_percent", 50), ("group_size", 8)), (("no_late_stream", 1), ("plan_main", 1)), (("first_fold_levels", 1), ("group_size", 24)),
    (("rounds_per_pass", 3), ("group_size", 1537)), (("no_fused_reduce", 1), ("host_tail_log2", -1)), (("plan_main", 1), ("fold_blocks", 8192)),
    (("group_size", 2), ("pass_queue_depth", 16)), (("no_fused_reduce", 1), ("no_mfma_fold", 1)), (("device_hash_percent", 90), ("rounds_per_pass", 3)),
    (("fold_min_chunk", 4096), ("first_fold_levels", 1)),
)


def grid():
    for options in GRID_OPTIONS:
        for n in range(2, MAX_N + 1):
            for batch in GRID_BATCHES:
                if admissible(n, batch):
                    for threads in GRID_THREADS:
                        yield n, batch, threads, options


def _cost(shape):
    n, batch, threads, options = shape
    return (batch << n, len(options), n, threads != 14, threads, options)


def grid_by_cost():
    """The grid, smallest shape first: fewest table entries in the call, then fewest options, then the smaller n, then fourteen threads
    before others."""
    return sorted(grid(), key=_cost)


def derive_cut_table(visit=None):
    """{cut: {True: smallest grid shape that meets the comparison with that outcome, or None, False: ...}}.  visit(shape, header, rows):
    called for every shape of the grid on the way."""
    seen, table = set(), {}
    for shape in grid_by_cost():
        header, rows, hits = plan(*shape)
        for name, outcome in hits - seen:
            table.setdefault(name, {True: None, False: None})[outcome] = shape
        seen |= hits
        if visit:
            visit(shape, header, rows)
    return table


# ---- the cuts: per comparison of the decision code and outcome, the smallest (n, batch, threads, options) of the grid that meets it
# (derive_cut_table(); tests/test_mle_shapes_host.py derives it afresh), or why no shape can
CUT_TABLE = {
    'arrivals: table <= 64 MiB': {
        False: (22, 1, 14, ()),
        True: (2, 1, 14, ()),
    },
    'device_hash: batch - n_dev < 16': {
        False: (2, 64, 14, (('device_hash_percent', 10),)),
        True: (2, 64, 14, (('device_hash_percent', 90),)),
    },
    'device_hash: batch >= 64': {
        False: (2, 1, 14, (('device_hash_percent', 10),)),
        True: (2, 64, 14, (('device_hash_percent', 10),)),
    },
    'device_hash: n_dev < 8': {
        False: (2, 64, 14, (('device_hash_percent', 25),)),
        True: (2, 64, 14, (('device_hash_percent', 10),)),
    },
    'fold.late: m_src != n': {
        False: (2, 1, 14, (('rounds_per_pass', 1),)),
        True: (3, 9, 14, (('rounds_per_pass', 1),)),
    },
    'fold.late: m_src <= 16': {
        False: (18, 1, 14, (('rounds_per_pass', 1),)),
        True: (3, 9, 14, (('rounds_per_pass', 1),)),
    },
    'fold.mfma: (S / nblk) % 64 == 0': {
        False: 'mle_pass_rounds gives a fold of more than 512 outputs sub-blocks of whole 64-entry tiles (j <= m - 6) and mle_multifold_blocks a power of two of blocks from 2^j up to S / 64 at the most: this driver reaches the v_mad_u64_u32 fold through option no_mfma_fold alone',
        True: (11, 1, 14, (('rounds_per_pass', 1),)),
    },
    'fold.small: S <= 512': {
        False: (11, 1, 14, (('rounds_per_pass', 1),)),
        True: (2, 1, 14, (('rounds_per_pass', 1),)),
    },
    'fold2.flagged: 256 partials per table': {
        False: (22, 2, 14, (('group_size', 1),)),
        True: (18, 2, 14, (('group_size', 1),)),
    },
    'fold2.flagged: partials of >= 16 entries': {
        False: (18, 2, 14, (('group_size', 1),)),
        True: (19, 2, 14, (('group_size', 1),)),
    },
    'fold_blocks.cap: twice the blocks <= 2048': {
        False: (21, 1, 14, (('rounds_per_pass', 1),)),
        True: (11, 1, 14, (('rounds_per_pass', 1),)),
    },
    'fold_blocks.min_chunk: half the chunk >= the minimum': {
        False: (11, 1, 14, (('rounds_per_pass', 1),)),
        True: (11, 1, 14, (('rounds_per_pass', 1),)),
    },
    'fold_blocks.target: blocks over the batch < target': {
        False: (15, 127, 14, (('fold_blocks', 2048),)),
        True: (11, 1, 14, (('rounds_per_pass', 1),)),
    },
    'fused: b0 + nb <= 4096': {
        False: (10, 4097, 14, (('device_hash_percent', 90), ('rounds_per_pass', 3))),
        True: (10, 1, 14, ()),
    },
    'fused: bytes read <= 64 MiB': {
        False: (19, 5, 14, (('fold_min_chunk', 4096), ('first_fold_levels', 1))),
        True: (10, 1, 14, ()),
    },
    'fused: nblk * nb <= 256': {
        False: (10, 9, 14, ()),
        True: (10, 1, 14, ()),
    },
    'fused: nblk <= 128': {
        False: (16, 1, 14, ()),
        True: (10, 1, 14, ()),
    },
    'groups.cap: more than 32': {
        False: (2, 1, 14, ()),
        True: (2, 33, 14, (('group_size', 1),)),
    },
    'groups.few_threads: host batch >= 256': {
        False: (2, 1, 1, ()),
        True: (2, 256, 1, ()),
    },
    'groups.few_threads: threads <= 3': {
        False: (2, 1, 14, ()),
        True: (2, 1, 1, ()),
    },
    'groups.size: host batch >= 128': {
        False: (2, 1, 14, ()),
        True: (2, 128, 14, ()),
    },
    'groups.size: host batch >= 16': {
        False: (2, 1, 14, ()),
        True: (2, 16, 14, ()),
    },
    'groups.small_tables: host batch >= 256': {
        False: (2, 1, 14, ()),
        True: (2, 256, 14, ()),
    },
    'groups.small_tables: n <= 17': {
        False: (18, 1, 14, ()),
        True: (2, 1, 14, ()),
    },
    'groups: fewer than four 4 GiB groups': {
        False: (17, 4096, 14, ()),
        True: (2, 1, 14, ()),
    },
    'groups: more than 96 GiB': {
        False: 'only asked of batches of more than 32 GiB, which the ABI refuses',
        True: 'only asked of batches of more than 32 GiB, which the ABI refuses',
    },
    'groups: more than eight 4 GiB groups': {
        False: (17, 4096, 14, ()),
        True: 'a call holds 2^30 values = 32 GiB of tables at the most: eight groups of 4 GiB, not more',
    },
    'hash_chunk: nb >= 32 threads': {
        False: (2, 1, 14, ()),
        True: (2, 32, 1, (('group_size', 64),)),
    },
    'hash_chunk: per thread <= 16': {
        False: (2, 17, 1, (('group_size', 24),)),
        True: (2, 9, 1, ()),
    },
    'hash_chunk: per thread <= 8': {
        False: (2, 9, 1, ()),
        True: (2, 1, 14, ()),
    },
    'host_tail: batch <= 8 (host_tail_max_batch)': {
        False: (2, 3, 14, (('host_tail_max_batch', 2),)),
        True: (2, 1, 14, ()),
    },
    'host_tail: m - j > 0': {
        False: (2, 1, 14, (('rounds_per_pass', 1),)),
        True: (3, 1, 14, (('rounds_per_pass', 1),)),
    },
    'host_tail: m <= 7': {
        False: (9, 1, 14, (('rounds_per_pass', 1),)),
        True: (2, 1, 14, (('rounds_per_pass', 1),)),
    },
    'pass0.deep: batch * nblk >= 24576': {
        False: (17, 8, 14, ()),
        True: (19, 24, 14, (('group_size', 24),)),
    },
    'pass0.deep: chunk % 512 == 0': {
        False: (10, 1, 14, (('no_fused_reduce', 1),)),
        True: (17, 8, 14, ()),
    },
    'pass0.deep: nblk % 8 == 0': {
        False: (10, 65535, 14, (('rounds_per_pass', 1),)),
        True: (17, 8, 14, ()),
    },
    'pass0.flagged: j == 5': {
        False: 'the records are offered on the two-level schedule alone, which option rounds_per_pass switches off: five rounds per pass, and n - 5 = 13 .. 19 is never the 2^10 or 2^11 that would shorten pass 0',
        True: (18, 2, 14, (('group_size', 1),)),
    },
    'pass0.flagged: nblk == 1024': {
        False: (20, 23, 14, (('items_per_block', 256),)),
        True: (19, 63, 14, ()),
    },
    'pass0.small: len <= 512': {
        False: (10, 1, 14, ()),
        True: (2, 1, 14, ()),
    },
    'pass0.stream: chunk % 256 == 0': {
        False: (10, 1, 14, (('no_fused_reduce', 1),)),
        True: (11, 1, 14, (('no_fused_reduce', 1), ('no_mfma_fold', 1))),
    },
    'pass0.stream: nblk % 4 == 0': {
        False: (10, 65535, 14, (('rounds_per_pass', 1),)),
        True: (11, 1, 14, (('no_fused_reduce', 1), ('no_mfma_fold', 1))),
    },
    'pass0.two_level: chunk < 256': {
        False: (18, 1, 14, ()),
        True: 'mle_pass_blocks stops below twice mle_blocks_per_table, which gives no more than one block per 256 entries: chunks of more than 128 entries, powers of two; and the 1024 blocks it starts from are 256 entries each at n = 18',
    },
    'rounds.leave_2^10_or_2^11': {
        False: (2, 1, 14, ()),
        True: (14, 1, 14, (('rounds_per_pass', 4),)),
    },
    'rounds.whole_tiles: j > m - 6': {
        False: (11, 1, 14, (('rounds_per_pass', 1),)),
        True: 'only a fold to 2^10 entries with five rounds could meet it (5 > 10 - 6), and no pass of this driver leaves 2^10 entries when it runs more than three rounds per pass (the rule behind it); the driver of a table split over ranks has its own tests',
    },
    'streams: more than one group': {
        False: (2, 1, 14, ()),
        True: (2, 2, 14, (('group_size', 1),)),
    },
    'two_level: n <= 24': {
        False: (25, 1, 14, ()),
        True: (18, 1, 14, ()),
    },
    'two_level: n >= 18': {
        False: (2, 1, 14, ()),
        True: (18, 1, 14, ()),
    },
}

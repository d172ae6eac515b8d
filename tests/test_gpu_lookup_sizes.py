"""gkr_lookup* (csrc/kernels_lookup.hip, csrc/capi_lookup.hip) bit for bit against the C oracle's ogkr_lookup_multiplicities,
ogkr_lookup_pair and ogkr_fraction_sum (cdense.lookup_multiplicities_raw, lookup_pair_raw, lookup_raw;
tests/test_oracle_lookup_c.py and tests/test_oracle_fraction_sum_c.py hold them to the integer models) at the sizes
tests/test_gpu_lookup.py does not reach.  The oracle counts by sorting: it has no index, no slot function and no probe chain, so
what crosses a wave or a block in the index build and in the count is held to something that shares no algorithm with it.  A
block is 256 threads: n = 10 is four blocks and sixteen waves.

  a. the index build across waves and blocks (n_t = 10, 12; n_w = 12): one value everywhere, sixteen values interleaved through
     every wave, a value's lowest index outside block 0, a value at {700, 3, 1023}, all keys in one slot (a chain of 1024), all
     keys in the last slot (every chain wraps), 2^11 values twice each;
  b. the count's wave combine (n_t = 10, n_w = 10 .. 12): 64 distinct indices per wave, two groups per wave in three patterns, a
     miss in lane 0, misses everywhere but lane 63, a leader outside the largest group, one value 2^14 times, misses in the last
     block only and in every block;
  c. batches whose columns span blocks: per-column tables of disjoint values, a column's misses its own, a shared table against
     copies, and the batch limit 65535;
  d. the pair against ogkr_lookup_pair at (9, 12), (12, 9), (10, 10) with canaries and the padding runs, and one call whose pair
     and witness lie 4 GiB into their allocations;
  e. the proof at L = 13 and 16 against cdense.lookup_raw;  f. the verifier at L = 13, verdicts from lookup_model.model_verdict.

The adversarial keys come from a numpy restatement of the slot function, held to lookup_model.slot first.  The library's own
output is never the reference of a value or a verdict.  Each case prints the seconds the oracle and the device calls took."""

import ctypes
import functools
import time

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from fraction_sum_model import EVALUATION, NON_CANONICAL, ROUND_SUM, SHAPE, ZERO_DENOMINATOR, head_root, layer_row
from fraction_sum_oracle import as_model
from fraction_sum_sweeps import ACCEPTED
from lookup_model import EMPTY, LOOKUP, model_verdict, slot
from oracle import cdense
from oracle.field import P
from resident_tables import Resident, free_bytes

pytestmark = pytest.mark.gpu

CANARY = np.array([0xC0DEC0DEC0DEC0DE, 0x0123456789ABCDEF, 0xFEDCBA9876543210, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
PAD = 16
NAMES = ("sums", "head", "coefficients", "lengths", "challenges", "values", "point", "claims")


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _ptr_at(d, elements):
    return ctypes.c_void_p(d.value + 32 * elements)


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
def slot_np(v, log_slots):
    """lookup_model.slot on (k, 4) limbs at once."""
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, 4)
    x = np.full(len(v), 0x9E3779B97F4A7C15, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(4):
            x = (x ^ v[:, i]) * np.uint64(0xFF51AFD7ED558CCD)
            x ^= x >> np.uint64(32)
        x = x * np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(29)
    return (x >> np.uint64(64 - log_slots)).astype(np.int64)


def _values(count, seed):
    """`count` canonical values (below 2^253), distinct in practice -- asserted where a case needs it."""
    return cdense.fill_table(count, seed)


def _keys_in_slot(target, log_slots, count, seed):
    """`count` distinct values whose slot among 2^log_slots is `target`."""
    cand = _values(2 * count << log_slots, seed)
    keys = cand[slot_np(cand, log_slots) == target][:count]
    assert len(keys) == count and len(np.unique(keys, axis=0)) == count
    return np.ascontiguousarray(keys)


def _draw(T, n_w, seed):
    return np.ascontiguousarray(T[np.random.default_rng(seed).integers(0, len(T), size=1 << n_w)])


def _distinct(a):
    return len(np.unique(a.reshape(-1, 4), axis=0)) == a.size // 4


def test_the_numpy_slot_function_is_the_models():
    v = _values(1000, 31000)
    v[:4] = cdense.to_limbs([0, 1, P - 1, 1 << 200])
    ints = cdense.from_limbs(v)
    for s in (1, 3, 11, 13, 32):
        assert [int(x) for x in slot_np(v, s)] == [slot(x, s) for x in ints], s
    t0 = time.perf_counter()
    keys = _keys_in_slot(5, 11, 1 << 10, 31001)
    assert time.perf_counter() - t0 < 5.0 and {slot(x, 11) for x in cdense.from_limbs(keys)} == {5}


# ---- the device against the oracle ------------------------------------------------------------------------------------------------------------
_seconds = {"oracle": 0.0, "device": 0.0}


def _oracle_multiplicities(W, T):
    t0 = time.perf_counter()
    cols = [cdense.lookup_multiplicities_raw(W[b], T[b if len(T) > 1 else 0]) for b in range(len(W))]
    _seconds["oracle"] += time.perf_counter() - t0
    return np.stack([c[0] for c in cols]), [c[1] for c in cols], [c[2] for c in cols]


def _device_multiplicities(ctx, W, T, shared):
    """W (batch, 2^n_w, 4), T (1 or batch, 2^n_t, 4) -> (M (batch, 2^n_t, 4), missing, first_missing); canaries around d_mult, W and T
    unchanged."""
    batch, n_w, n_t = W.shape[0], W.shape[1].bit_length() - 1, T.shape[1].bit_length() - 1
    assert T.shape[0] == (1 if shared else batch)
    total = batch << n_t
    with Resident(ctx, W) as dw, Resident(ctx, T) as dt, Resident(ctx, np.tile(CANARY, (total + 2 * PAD, 1))) as dm:
        t0 = time.perf_counter()
        missing, first = ctx.lookup_multiplicities_device(dw.d, n_w, dt.d, n_t, shared, batch, _ptr_at(dm.d, PAD))
        _seconds["device"] += time.perf_counter() - t0
        dw.assert_unchanged("witness")
        dt.assert_unchanged("table")
        got = ctx.download(dm.d, (total + 2 * PAD, 4))
    assert (got[:PAD] == CANARY).all() and (got[PAD + total:] == CANARY).all(), "canaries around d_mult"
    return got[PAD:PAD + total].reshape(batch, 1 << n_t, 4), [int(x) for x in missing], [int(x) for x in first]


def _assert_multiplicities(ctx, W, T, shared, what):
    """The device's M, missing and first_missing are the oracle's, bit for bit -> the oracle's."""
    W, T = (np.ascontiguousarray(a).reshape((-1,) + a.shape[-2:]) for a in (W, T))
    _seconds["oracle"] = _seconds["device"] = 0.0
    want = _oracle_multiplicities(W, T)
    got = _device_multiplicities(ctx, W, T, shared)
    if not np.array_equal(got[0], want[0]):
        b, j = (int(x) for x in np.argwhere((got[0] != want[0]).any(axis=-1))[0])
        pytest.fail("%s: M differs first at column %d, entry %d: got %s, want %s (%d entries in all)"
                    % (what, b, j, got[0][b, j], want[0][b, j], int((got[0] != want[0]).any(axis=-1).sum())))
    assert got[1:] == want[1:], (what, got[1:], want[1:])
    print("\ntiming %s: oracle %.2f ms, device %.2f ms" % (what, 1e3 * _seconds["oracle"], 1e3 * _seconds["device"]))
    return want


# ---- a. the index build across waves and blocks ---------------------------------------------------------------------------------------------
BUILD_NAMES = ["one value", "sixteen values through every wave", "a lowest index outside block 0", "a value at 700, 3 and 1023", "one slot",
               "the last slot", "2^11 values twice"]


@functools.lru_cache(maxsize=None)
def _build_tables():
    """name -> T (2^n_t, 4)."""
    n_t, size = 10, 1 << 10
    out = {}
    v = _values(size + 16, 31100)
    out["one value"] = np.tile(v[0], (size, 1))
    sixteen = v[size:size + 16]
    out["sixteen values through every wave"] = sixteen[(np.arange(size) * 5 + np.arange(size) // 16) % 16]
    order = (np.arange(size) * 5 + np.arange(size) // 16) % 16     # value 15 leaves block 0 for value 14's places in block 3
    at15, at14 = np.flatnonzero((order == 15) & (np.arange(size) < 256)), np.flatnonzero((order == 14) & (np.arange(size) >= 768))
    assert len(at15) == len(at14) == 16
    order[at15], order[at14] = 14, 15
    out["a lowest index outside block 0"] = sixteen[order]
    t = v[:size].copy()
    t[700] = t[1023] = t[3]
    out["a value at 700, 3 and 1023"] = t
    out["one slot"] = _keys_in_slot(1234, n_t + 1, size, 31101)
    out["the last slot"] = _keys_in_slot((2 << n_t) - 1, n_t + 1, size, 31102)
    half = _values(1 << 11, 31103)
    out["2^11 values twice"] = np.concatenate([half, half])
    assert sorted(out) == sorted(BUILD_NAMES)
    return out


def test_the_build_tables_are_what_their_names_say():
    T = _build_tables()
    assert len(np.unique(T["one value"], axis=0)) == 1
    for name in ("sixteen values through every wave", "a lowest index outside block 0"):
        values, first, counts = np.unique(T[name], axis=0, return_index=True, return_counts=True)
        assert len(values) == 16 and (counts == 64).all(), name
        per_wave = [len(np.unique(T[name][w * 64:(w + 1) * 64], axis=0)) for w in range(16)]
        assert (per_wave == [16] * 16 and first.max() < 64) if "every wave" in name else (first.max() >= 256 and min(per_wave) >= 15), name
    t = T["a value at 700, 3 and 1023"]
    assert len(np.unique(t, axis=0)) == 1022 and [int(j) for j in np.flatnonzero((t == t[3]).all(axis=1))] == [3, 700, 1023]
    assert set(slot_np(T["one slot"], 11)) == {1234} and set(slot_np(T["the last slot"], 11)) == {2047}
    assert _distinct(T["one slot"]) and _distinct(T["the last slot"])
    t = T["2^11 values twice"]
    assert t.shape == (1 << 12, 4) and _distinct(t[:1 << 11]) and np.array_equal(t[:1 << 11], t[1 << 11:])


@pytest.mark.parametrize("name", BUILD_NAMES)
def test_the_index_build_across_waves_and_blocks(ctx, name):
    T = _build_tables()[name]
    W = _draw(T, 12, 31110)
    M, missing, first = _assert_multiplicities(ctx, W[None], T[None], True, name)
    assert missing == [0] and first == [EMPTY] and int(M[0, :, 0].sum()) == 1 << 12
    if name == "one value":
        assert int(M[0, 0, 0]) == 1 << 12
    if name == "2^11 values twice":
        assert not M[0, 1 << 11:].any()                            # the lower copy takes the count


# ---- b. the count's wave combine ------------------------------------------------------------------------------------------------------------
COUNT_NAMES = ["64 distinct indices per wave", "two groups, alternating", "two groups, halves", "two groups, 63 + 1", "lane 0 misses",
               "all lanes miss but lane 63", "a leader outside the largest group", "one value 2^14 times, a table of four",
               "misses in the last block only", "misses in every block"]


@functools.lru_cache(maxsize=None)
def _count_cases():
    """name -> (W, T): n_t = 10 with distinct values unless the name says otherwise; every miss is a value outside T."""
    size = 1 << 10
    v = _values(size + 4096, 31200)
    T, outside = np.ascontiguousarray(v[:size]), v[size:]
    assert _distinct(v)
    rng = np.random.default_rng(31201)
    lane = np.arange(64)
    out = {}
    out["64 distinct indices per wave"] = (T[rng.permutation(size)], T)

    def waves(n_w, fill):
        """A witness of 2^n_w entries, wave w filled by fill(w, a, b, c) -> 64 rows (a, b, c: three distinct table indices)."""
        rows = []
        for w in range((1 << n_w) // 64):
            a, b, c = (int(x) for x in rng.choice(size, size=3, replace=False))
            rows.append(fill(w, a, b, c))
        return np.ascontiguousarray(np.concatenate(rows))

    pick2 = lambda mask, a, b: np.where(mask[:, None], T[a][None], T[b][None])
    out["two groups, alternating"] = (waves(10, lambda w, a, b, c: pick2(lane % 2 == 0, a, b)), T)
    out["two groups, halves"] = (waves(11, lambda w, a, b, c: pick2(lane < 32, a, b)), T)
    out["two groups, 63 + 1"] = (waves(12, lambda w, a, b, c: pick2(lane < 63, a, b)), T)

    def with_misses(mask_miss, base, w):
        rows = base.copy()
        rows[mask_miss] = outside[w * 64 + np.flatnonzero(mask_miss)]
        return rows

    out["lane 0 misses"] = (waves(10, lambda w, a, b, c: with_misses(lane == 0, np.tile(T[a], (64, 1)), w)), T)
    out["all lanes miss but lane 63"] = (waves(11, lambda w, a, b, c: with_misses(lane < 63, np.tile(T[a], (64, 1)), w)), T)
    out["a leader outside the largest group"] = (waves(12, lambda w, a, b, c: with_misses(lane == 0, pick2(lane == 1, c, a), w)), T)
    four = np.ascontiguousarray(T[:4])
    out["one value 2^14 times, a table of four"] = (np.tile(four[2], (1 << 14, 1)), four)
    W = T[rng.integers(0, size, size=1 << 11)]
    W[(1 << 11) - 256 + np.array([5, 64, 130, 255])] = outside[:4]
    out["misses in the last block only"] = (np.ascontiguousarray(W), T)
    W = T[rng.integers(0, size, size=1 << 12)]
    at = np.arange(16) * 256 + rng.integers(0, 256, size=16)
    W[at] = outside[4:20]
    out["misses in every block"] = (np.ascontiguousarray(W), T)
    assert sorted(out) == sorted(COUNT_NAMES)
    return out


COUNT_MISSES = {"lane 0 misses": (16, 0), "all lanes miss but lane 63": (32 * 63, 0), "a leader outside the largest group": (64, 0),
                "misses in the last block only": (4, 2048 - 256 + 5), "misses in every block": (16, None)}


@pytest.mark.parametrize("name", COUNT_NAMES)
def test_the_counts_wave_combine(ctx, name):
    W, T = _count_cases()[name]
    if name.startswith("two groups") or name == "64 distinct indices per wave":
        groups = [len(np.unique(W[w * 64:(w + 1) * 64], axis=0)) for w in range(len(W) // 64)]
        assert groups == [64 if "distinct" in name else 2] * (len(W) // 64)
    M, missing, first = _assert_multiplicities(ctx, W[None], T[None], True, name)
    want_missing, want_first = COUNT_MISSES.get(name, (0, EMPTY))
    assert missing == [want_missing] and int(M[0, :, 0].sum()) == len(W) - want_missing, name
    if want_first is not None:
        assert first == [want_first], name
    if name == "misses in the last block only":
        assert first[0] >= len(W) - 256
    if name == "misses in every block":
        assert first[0] < 256


# ---- c. batches at multi-block sizes --------------------------------------------------------------------------------------------------------
def test_batches_whose_columns_span_blocks(ctx):
    """Batch 3, n_w = 11 (eight blocks a column), n_t = 9 (two): per-column tables with pairwise disjoint values, each column's
    witness drawn from its own table; the same with five entries of column 1 taken from column 0's table -- column 1's misses, and
    only column 1's; a shared table against per-column copies."""
    n_w, n_t, batch = 11, 9, 3
    T = _values(batch << n_t, 31300).reshape(batch, 1 << n_t, 4)
    assert _distinct(T)
    W = np.stack([_draw(T[b], n_w, 31301 + b) for b in range(batch)])
    M, missing, first = _assert_multiplicities(ctx, W, T, False, "per-column tables")
    assert missing == [0] * 3 and first == [EMPTY] * 3 and [int(M[b, :, 0].sum()) for b in range(3)] == [1 << n_w] * 3
    at = [300, 301, 1000, 1999, 2047]
    W2 = W.copy()
    W2[1, at] = T[0, [7, 7, 300, 511, 0]]
    M2, missing, first = _assert_multiplicities(ctx, W2, T, False, "column 1 takes values of column 0's table")
    assert missing == [0, 5, 0] and first == [EMPTY, 300, EMPTY] and np.array_equal(M2[0], M[0]) and np.array_equal(M2[2], M[2])
    Ws = np.stack([_draw(T[0], n_w, 31310 + b) for b in range(batch)])
    Ws[2, 1234] = T[1, 0]                                          # one miss against the shared table
    shared = _assert_multiplicities(ctx, Ws, T[:1], True, "a shared table")
    copies = _assert_multiplicities(ctx, Ws, np.stack([T[0]] * 3), False, "per-column copies")
    assert np.array_equal(shared[0], copies[0]) and shared[1:] == copies[1:] == ([0, 0, 1], [EMPTY, EMPTY, 1234])


def test_the_batch_limit_of_65535_columns(ctx):
    """n_w = n_t = 2, seven instances in turn (per-column tables), instance 3 with a miss at entry 2."""
    batch = 65535
    T7 = _values(7 * 4, 31400).reshape(7, 4, 4)
    T7[5, 3] = T7[5, 0]                                            # a repeated table value
    rng = np.random.default_rng(31401)
    W7 = np.stack([T7[i][rng.integers(0, 4, size=4)] for i in range(7)])
    W7[5, 1] = T7[5, 0]
    W7[3, 2] = T7[4, 0]
    want7 = _oracle_multiplicities(W7, T7)
    assert want7[1] == [0, 0, 0, 1, 0, 0, 0] and want7[2][3] == 2 and not want7[0][5, 3].any()
    idx = np.arange(batch) % 7
    t0 = time.perf_counter()
    M, missing, first = _device_multiplicities(ctx, np.ascontiguousarray(W7[idx]), np.ascontiguousarray(T7[idx]), False)
    assert np.array_equal(M, want7[0][idx]) and missing == [want7[1][i] for i in idx] and first == [want7[2][i] for i in idx]
    print("\ntiming batch 65535: device and transfers %.3f s" % (time.perf_counter() - t0))


# ---- d. the pair ------------------------------------------------------------------------------------------------------------------------------
def _columns(n_w, n_t, batch, seed, shared, duplicates=False):
    """-> (W (batch, ..), T (1 or batch, ..), M (batch, ..) the oracle's, alpha (batch, 4)) of lookups that hold."""
    tables = 1 if shared else batch
    T = _values(tables << n_t, seed).reshape(tables, 1 << n_t, 4)
    if duplicates:
        T[:, 1] = T[:, -1] = T[:, 0]
        T[:, 1 << (n_t - 1)] = T[:, 2]
    W = np.stack([_draw(T[b if not shared else 0], n_w, seed + 1 + b) for b in range(batch)])
    M, missing, _ = _oracle_multiplicities(W, T)
    assert missing == [0] * batch
    return W, T, M, _values(batch, seed + 100)


def _device_pair(ctx, W, T, M, alpha, shared):
    batch, n_w, n_t = W.shape[0], W.shape[1].bit_length() - 1, T.shape[1].bit_length() - 1
    L = max(n_w, n_t) + 1
    total = batch * (2 << L)
    with Resident(ctx, W) as dw, Resident(ctx, T) as dt, Resident(ctx, M) as dm, Resident(ctx, np.tile(CANARY, (total + 2 * PAD, 1))) as dp:
        alpha = np.ascontiguousarray(alpha)
        rc = N.lib().gkr_devtest_lookup_pair(ctx._h, dw.d, n_w, dt.d, n_t, int(shared), dm.d, alpha.ctypes.data, batch, _ptr_at(dp.d, PAD))
        assert rc == N.GKR_OK, rc
        for part in (dw, dt, dm):
            part.assert_unchanged("the pair's inputs")
        got = ctx.download(dp.d, (total + 2 * PAD, 4))
    assert (got[:PAD] == CANARY).all() and (got[PAD + total:] == CANARY).all(), "canaries around the pair"
    return got[PAD:PAD + total].reshape(batch, 2, 1 << L, 4)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n_w,n_t", [(9, 12), (12, 9), (10, 10)])
def test_the_pair_matches_the_c_oracle(ctx, n_w, n_t, shared):
    W, T, M, alpha = _columns(n_w, n_t, 2, 31500 + 10 * n_w + shared, shared)
    got = _device_pair(ctx, W, T, M, alpha, shared)
    half = 1 << max(n_w, n_t)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    for b in range(2):
        want = cdense.lookup_pair_raw(W[b], T[0 if shared else b], M[b], alpha[b])
        assert np.array_equal(got[b], want), (n_w, n_t, shared, b)
        for lo, hi in (((1 << n_w), half), (half + (1 << n_t), 2 * half)):      # the padding of either side is (0, 1)
            assert not got[b, 0, lo:hi].any() and (got[b, 1, lo:hi] == one).all(), (b, lo, hi)
        assert (got[b, 0, :1 << n_w] == one).all() and got[b, 1].any(axis=1).all()


def test_the_pair_and_the_witness_four_gib_into_their_allocations(ctx):
    """n_w = n_t = 10 (L = 11: 128 KiB a pair), batch 32769: the pair of column 32768 starts at byte 2^32 of d_pair, and the witness
    pointer itself lies 2^32 bytes into its allocation.  Columns 0 and 32768 are the oracle's on the downloaded inputs."""
    n, batch = 10, 32769
    L, col = n + 1, 32 << n
    assert (batch - 1) * (64 << L) == 1 << 32
    need = (1 << 32) + 3 * batch * col + batch * (64 << L)
    if free_bytes() < int(1.1 * need):
        pytest.skip("not enough free device memory for %d MiB of columns and pairs" % (need >> 20))
    alpha = _values(batch, 31600)
    d_w, d_t, d_m, d_p = ctx.alloc((1 << 32) + batch * col), ctx.alloc(batch * col), ctx.alloc(batch * col), ctx.alloc(batch * (64 << L))
    try:
        w = ctypes.c_void_p(d_w.value + (1 << 32))
        ctx.fill_table(w, batch << n, 31601)
        ctx.fill_table(d_t, batch << n, 31602)
        ctx.fill_table(d_m, batch << n, 31603)                     # (any canonical values: the pair is a rule of W, T, M and alpha)
        t0 = time.perf_counter()
        assert N.lib().gkr_devtest_lookup_pair(ctx._h, w, n, d_t, n, 0, d_m, alpha.ctypes.data, batch, d_p) == N.GKR_OK
        device_s = time.perf_counter() - t0
        for b in (0, batch - 1):
            Wb, Tb, Mb = (ctx.download(_ptr_at(d, b << n), (1 << n, 4)) for d in (w, d_t, d_m))
            got = ctx.download(_ptr_at(d_p, b << (L + 1)), (2, 1 << L, 4))
            assert np.array_equal(got, cdense.lookup_pair_raw(Wb, Tb, Mb, alpha[b])), b
    finally:
        for d in (d_w, d_t, d_m, d_p):
            ctx.free(d)
    print("\ntiming the 4 GiB pair: device %.2f ms" % (1e3 * device_s))


# ---- e. the proof -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_w,n_t,batch", [(12, 9, 1), (9, 12, 1), (12, 12, 3), (15, 15, 1)])
def test_the_proof_matches_the_c_oracle(ctx, n_w, n_t, batch):
    """The device's multiplicities are the oracle's; all eight arrays of the proof are cdense.lookup_raw's on them; P = 0 and
    Q != 0; the verifier accepts under both hash sides.  (12, 12, 3) shares one table that has repeated values; L = 16 at (15, 15)
    reaches the layer whose round kernel makes exactly one trip over the partials."""
    shared = batch > 1
    W, T, M, alpha = _columns(n_w, n_t, batch, 31700 + 10 * n_w + n_t, shared, duplicates=shared)
    L = max(n_w, n_t) + 1
    t0 = time.perf_counter()
    raws = [cdense.lookup_raw(W[b], T[0 if shared else b], M[b], alpha[b]) for b in range(batch)]
    oracle_s = time.perf_counter() - t0
    want = tuple(np.stack([r[i] for r in raws]) for i in range(8))
    with Resident(ctx, W) as dw, Resident(ctx, T) as dt, Resident(ctx, np.zeros_like(M)) as dm:
        t0 = time.perf_counter()
        missing, first = ctx.lookup_multiplicities_device(dw.d, n_w, dt.d, n_t, shared, batch, dm.d)
        assert not missing.any() and (first == EMPTY).all() and np.array_equal(ctx.download(dm.d, M.shape), M)
        got = ctx.lookup_batch_device(dw.d, n_w, dt.d, n_t, shared, dm.d, alpha, batch)
        prove_s = time.perf_counter() - t0
        for name, g, w in zip(NAMES, got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), ((n_w, n_t, batch), name)
        assert not want[0][:, 0].any() and want[0][:, 1].any(axis=-1).all()
        t0 = time.perf_counter()
        try:
            for hash_min in (-1, 1):
                ctx.set_option("verify_device_hash_min", hash_min)
                accept, layer, rnd, check, sums = ctx.verify_lookup_batch_device(dw.d, n_w, dt.d, n_t, shared, dm.d, alpha, batch, *want[1:6])
                assert accept.all() and not check.any() and not layer.any() and not rnd.any() and np.array_equal(sums, want[0]), hash_min
        finally:
            ctx.set_option("verify_device_hash_min", 0)
        verify_s = time.perf_counter() - t0
        for part in (dw, dt):
            part.assert_unchanged("the lookup's inputs")
    print("\ntiming proof (%d, %d, %d): oracle %.2f s, device count and prover %.3f s, device verifier (twice) %.3f s"
          % (n_w, n_t, batch, oracle_s, prove_s, verify_s))


# ---- f. the verifier at L = 13 --------------------------------------------------------------------------------------------------------------
def _plus_one(limbs):
    return cdense.to_limbs([cdense.from_limbs(np.asarray(limbs).reshape(1, 4))[0] + 1])[0]


def test_the_verifier_at_thirteen_variables(ctx):
    """n_w = n_t = 12, L = 13, per-column tables, ONE batch.  Every case is (what the verifier is given: W, T, M, alpha; the proof:
    the oracle's of what was proved); the expectation is lookup_model.model_verdict on exactly that, and the verdicts the header
    names are also written out.  Both hash sides, one chunk and several."""
    n, L = 12, 13
    size, last = 1 << n, (1 << n) - 256
    W, T, M, alpha = (a[0] for a in _columns(n, n, 1, 31800, False, duplicates=True))
    W[:3] = T[0]                                                   # the duplicated value occurs: its count can be split
    M = cdense.lookup_multiplicities_raw(W, T)[0]
    outside = _values(1, 31801)[0]
    oracle_s = []

    def proved(key, W, T, M, alpha):
        t0 = time.perf_counter()
        raw = cdense.lookup_raw(W, T, M, alpha)
        oracle_s.append(time.perf_counter() - t0)
        return raw

    honest = proved("honest", W, T, M, alpha)
    cases = [("honest", W, T, M, alpha, honest, ACCEPTED)]
    Wm = W.copy()
    Wm[last + 100] = outside
    Mm, missing, first = cdense.lookup_multiplicities_raw(Wm, T)
    assert (missing, first) == (1, last + 100)
    cases.append(("a witness value outside the table, proved as it stands", Wm, T, Mm, alpha, proved("miss", Wm, T, Mm, alpha), (LOOKUP, 0, 0)))
    Mp = M.copy()
    Mp[last + 7] = _plus_one(M[last + 7])
    cases.append(("M + 1 in the last block, proved as it stands", W, T, Mp, alpha, proved("plus", W, T, Mp, alpha), (LOOKUP, 0, 0)))
    for j in (0, size - 1):
        Mc = M.copy()
        Mc[j] = _plus_one(M[j])
        cases.append(("d_mult[%d] changed after proving" % j, W, T, Mc, alpha, honest, (EVALUATION, L, L)))
    Wc = W.copy()
    Wc[last + 200] = _plus_one(W[last + 200])
    cases.append(("a witness entry changed after proving", Wc, T, M, alpha, honest, (EVALUATION, L, L)))
    Tc = T.copy()
    Tc[last + 50] = _plus_one(T[last + 50])
    cases.append(("a table entry changed after proving", W, Tc, M, alpha, honest, (EVALUATION, L, L)))
    cases.append(("alpha + 1 after proving", W, T, M, _plus_one(alpha), honest, (EVALUATION, L, L)))
    cases.append(("alpha = a table value", W, T, M, T[last + 9], proved("zero", W, T, M, T[last + 9]), (ZERO_DENOMINATOR, 0, 0)))
    Ms = M.copy()
    assert int(M[0, 0]) >= 3 and not M[1].any() and np.array_equal(T[1], T[0])
    Ms[0, 0], Ms[1, 0] = M[0, 0] - 1, 1
    cases.append(("a lossless split", W, T, Ms, alpha, proved("split", W, T, Ms, alpha), ACCEPTED))
    row = layer_row(12) + 5
    changed = tuple(a.copy() for a in honest)
    changed[2][row, 3] = _plus_one(honest[2][row, 3])
    cases.append(("a coefficient of layer 12 changed", W, T, M, alpha, changed, (ROUND_SUM, 12, 5)))
    cases.append(("honest", W, T, M, alpha, honest, ACCEPTED))
    want, roots = [], []
    t0 = time.perf_counter()
    for name, Wc, Tc, Mc, ac, raw, expect in cases:
        g = as_model(raw, L)
        v = model_verdict(g["head"], g["layers"], cdense.from_limbs(Wc), cdense.from_limbs(Tc), cdense.from_limbs(Mc),
                          cdense.from_limbs(np.asarray(ac).reshape(1, 4))[0], n, n)
        assert v == expect, (name, v, expect)
        want.append(v)
        roots.append((0, 0) if v[0] in (SHAPE, NON_CANONICAL) else head_root(g["head"]))
    model_s = time.perf_counter() - t0
    B = len(cases)
    Wb, Tb, Mb, ab = (np.stack([np.asarray(c[i]) for c in cases]) for i in (1, 2, 3, 4))
    H, C, Ln, R, E = (np.stack([c[5][i] for c in cases]) for i in (1, 2, 3, 4, 5))
    expect_sums = cdense.to_limbs([x for root in roots for x in root]).reshape(B, 2, 4)
    chunk = np.zeros(1, dtype=np.uint32)
    verify_s = []
    with Resident(ctx, Wb) as dw, Resident(ctx, Tb) as dt, Resident(ctx, Mb) as dm:
        try:
            for mb in (0, 1):
                for hash_min in (-1, 1):
                    ctx.set_option("verify_workspace_mb", mb)
                    ctx.set_option("verify_device_hash_min", hash_min)
                    assert N.lib().gkr_devtest_fraction_sum_chunk(ctx._h, L, B, chunk.ctypes.data) == N.GKR_OK
                    assert (chunk[0] == B) if mb == 0 else (1 <= chunk[0] <= B), (mb, chunk[0])     # (1 MiB holds these twelve: the pair is not the chunk's)
                    t0 = time.perf_counter()
                    accept, layer, rnd, check, sums = ctx.verify_lookup_batch_device(dw.d, n, dt.d, n, False, dm.d, ab, B, H, C, Ln, R, E)
                    verify_s.append(time.perf_counter() - t0)
                    got = [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]
                    diff = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
                    assert diff is None, ((mb, hash_min), cases[diff][0], got[diff], want[diff])
                    assert list(accept) == [w == ACCEPTED for w in want] and np.array_equal(sums, expect_sums), (mb, hash_min)
        finally:
            ctx.set_option("verify_workspace_mb", 0)
            ctx.set_option("verify_device_hash_min", 0)
        for part in (dw, dt, dm):
            part.assert_unchanged("the verifier's inputs")
    print("\ntiming verifier (12, 12, %d): oracle %.2f s (five proofs), model verdicts %.2f s, device verifier %.3f s (four settings)"
          % (B, sum(oracle_s), model_s, sum(verify_s)))

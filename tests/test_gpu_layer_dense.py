"""The dense-table forms of the layer sumcheck and the step-wise sessions at the edges of their launch geometry, bit for bit against
the C oracle (oracle/c/ogkr.c through oracle/cdense.py) or Python integers -- never against the library itself:

  predicate tables   gkr_predicate_tables and, per shard, gkr_devtest_predicates under both builders (counting sort, and the
                     widened-atomic scatter of option predicate_atomics) against cdense.predicate_tables;
  device transcript  one layer and a whole batch of proofs under GKR_TRANSCRIPT_DEVICE, with the fused b-phase round and with
                     layer_no_fused, against cdense.sumcheck_layer_lin_raw / cdense.prove_raw;
  layer sessions     parallel.prove_sumcheck_opt_logical against the oracle's transcript, one shard at a time against an integer
                     model, and gkr_layer_session_open_tables on its own;
  plain sessions     parallel.prove_sumcheck_logical against cdense.sumcheck_mle_raw.

Every case first asserts its row of tests/dense_shapes.py against the library's own launch arithmetic
(gkr_selftest_layer_dense_geometry), so a case that no longer sits on its threshold fails its pin."""

import ctypes
import functools

import numpy as np
import pytest

import dense_shapes as ds
import gate_profiles as gp
from gkr_amd import Context, GKRCircuit, GkrError, Layer, parallel, synth
from gkr_amd import _native as N
from gkr_amd.field import from_limbs, to_limbs
from oracle import cdense
from oracle.field import P
from product_shapes import product_geometry

pytestmark = pytest.mark.gpu

R_MINUS_1 = np.array(gp._limbs(P - 1), dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


@pytest.fixture(scope="module")
def ctx_atomics():
    with Context(0) as c:
        c.set_option("predicate_atomics", 1)
        yield c


@pytest.fixture(scope="module")
def ctx_device():
    with Context(0) as c:
        c.set_transcript(N.GKR_TRANSCRIPT_DEVICE)
        yield c


@pytest.fixture(scope="module")
def ctx_device_unfused():
    with Context(0) as c:
        c.set_transcript(N.GKR_TRANSCRIPT_DEVICE)
        c.set_option("layer_no_fused", 1)
        yield c


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def _gates(k_i, k, seed, pattern="uniform"):
    rng = np.random.default_rng(seed)
    g = 1 << k_i
    gt = rng.integers(0, 2, g, dtype=np.uint8)
    l = rng.integers(0, 1 << k, g, dtype=np.uint32)
    r = rng.integers(0, 1 << k, g, dtype=np.uint32)
    if pattern == "all_add":
        gt[:] = 0
    elif pattern == "all_mult":
        gt[:] = 1
    elif pattern == "sorted_left":     # runs of one left operand: neighbouring threads of the fill kernel meet on a few cursors
        l = np.sort(l)
        r = (r >> max(k - 2, 0)).astype(np.uint32)
    else:
        assert pattern == "uniform", pattern
    return gt, l, r


# =========================================================================== predicate tables

PREDICATE_SHAPES = [(0, 1), (1, 5), (9, 6), (13, 10), (12, 11), (21, 6)]
GATE_PATTERNS = ("uniform", "all_add", "all_mult", "sorted_left")


def _device_predicates(c, k_i, k, gates, z, log_p=0, shard=0):
    n = 1 << (2 * k - log_p)
    A, M = np.zeros((n, 4), dtype=np.uint64), np.zeros((n, 4), dtype=np.uint64)
    c._check(N.lib().gkr_devtest_predicates(c._h, k_i, k, _p(gates[0]), _p(gates[1]), _p(gates[2]), _p(z), log_p, shard, _p(A), _p(M)))
    return A, M


def _oracle_predicates(k_i, k, gates, z):
    return cdense.predicate_tables(k_i, k, *gates, from_limbs(z))


@pytest.mark.parametrize("k_i,k", PREDICATE_SHAPES)
def test_predicate_tables_at_scan_and_grid_thresholds(ctx, ctx_atomics, k_i, k):
    """All 2 * 2^(2k) entries under both builders: one full scan block and several, k_scan_sums over one full trip of 1024 block sums
    and over four with the carry between them, the grid-stride trips of the cell kernels (k_pred_sum, k_predicate_normalise) and of
    the gate kernels (2^21 gates, ~512 per cell)."""
    assert ds.predicate_row(k, 0) == ds.PREDICATE[(k, 0)]
    assert ctx.get_option("predicate_atomics") == 0 and ctx_atomics.get_option("predicate_atomics") == 1
    z = synth.rand_fr(np.random.default_rng(100 + k_i), k_i)
    for pattern in GATE_PATTERNS:
        gates = _gates(k_i, k, 1000 * k_i + k, pattern)
        lay = Layer(k_i, *gates)
        want = _oracle_predicates(k_i, k, gates, z)
        if pattern == "all_add":
            assert want[0].any() and not want[1].any()
        if pattern == "all_mult":
            assert want[1].any() and not want[0].any()
        for c in (ctx, ctx_atomics):
            assert _same(c.predicate_tables(lay, k, z), want), (pattern, c is ctx_atomics)


def test_predicate_tables_one_cell(ctx, ctx_atomics):
    """2^16 gates on the last cell of both tables, add and mult alternating, then on the first: one list of 2^15 gates per table, every
    other entry zero."""
    k_i, k = 16, 5
    assert ds.predicate_row(k, 0) == ds.PREDICATE[(k, 0)]
    g = 1 << k_i
    z = synth.rand_fr(np.random.default_rng(7), k_i)
    gt = (np.arange(g) & 1).astype(np.uint8)
    for operand in ((1 << k) - 1, 0):
        gates = (gt, np.full(g, operand, dtype=np.uint32), np.full(g, operand, dtype=np.uint32))
        want = _oracle_predicates(k_i, k, gates, z)
        cell = (operand << k) | operand
        for t in want:
            assert t[cell].any() and not np.delete(t, cell, axis=0).any()
        for c in (ctx, ctx_atomics):
            assert _same(c.predicate_tables(Layer(k_i, *gates), k, z), want), (operand, c is ctx_atomics)


@pytest.mark.parametrize("k_i,k,log_p", [(12, 8, 1), (12, 8, 3), (12, 8, 8), (13, 10, 2)])
def test_predicate_tables_of_every_shard(ctx, ctx_atomics, k_i, k, log_p):
    """gkr_devtest_predicates (build_predicates as gkr_layer_session_open calls it): shard p of 2^log_p holds the cells
    A_p[b * 2^kc + c'] = A[b * 2^k + c' * P + p]."""
    assert ds.predicate_row(k, log_p) == ds.PREDICATE[(k, log_p)]
    shards, kc = 1 << log_p, k - log_p
    gates = _gates(k_i, k, 77 + log_p)
    z = synth.rand_fr(np.random.default_rng(78), k_i)
    want = [t.reshape(1 << k, 1 << kc, shards, 4) for t in _oracle_predicates(k_i, k, gates, z)]
    for c in (ctx, ctx_atomics):
        for p in range(shards):
            got = _device_predicates(c, k_i, k, gates, z, log_p, p)
            assert _same(got, [np.ascontiguousarray(t[:, :, p]).reshape(-1, 4) for t in want]), (p, c is ctx_atomics)
    # the entry's own refusals
    for bad_log_p, bad_shard in ((k + 1, 0), (log_p, shards)):
        with pytest.raises(GkrError) as e:
            _device_predicates(ctx, k_i, k, gates, z, bad_log_p, bad_shard)
        assert e.value.status == N.GKR_ERR_INVALID


def test_predicate_build_refuses_a_bad_gate_in_the_last_block(ctx, ctx_atomics):
    """2^21 gates are validated on the device only: an operand = 2^k or a type 2 at the very end (the last block's second grid-stride
    trip) is GKR_ERR_INVALID under both builders, and the context builds a good layer correctly afterwards."""
    k_i, k = 21, 6
    good = _gates(k_i, k, 4321)
    z = synth.rand_fr(np.random.default_rng(4322), k_i)
    want = _oracle_predicates(k_i, k, good, z)
    last = (1 << k_i) - 1
    for c in (ctx, ctx_atomics):
        for which, value in ((1, 1 << k), (2, 1 << k), (0, 2)):
            bad = [a.copy() for a in good]
            bad[which][last - (3 * which)] = value
            with pytest.raises(GkrError) as e:
                c.predicate_tables(Layer(k_i, *bad), k, z)
            assert e.value.status == N.GKR_ERR_INVALID, (which, c is ctx_atomics)
        assert _same(c.predicate_tables(Layer(k_i, *good), k, z), want), c is ctx_atomics


# =========================================================================== device transcript, one layer

DEVICE_SHAPES = [(10, 8), (12, 9), (12, 10), (13, 11)]
W_KINDS = ("random", "r_minus_1", "one_hot", "independent")


def _w(kind, k, seed):
    if kind != "independent":
        return gp.w_pattern(kind, k, seed)
    # no dependence on variable 1 (the top index bit), variable k (the lowest) and one in the middle
    idx = np.arange(1 << k)
    drop = (1 << (k - 1)) | 1 | (1 << (k // 2))
    return np.ascontiguousarray(synth.rand_fr(np.random.default_rng(seed), 1 << k)[idx & ~drop])


@functools.lru_cache(maxsize=None)
def _device_case(k_i, k, kind):
    gates = _gates(k_i, k, 31 * k_i + k)
    z = synth.rand_fr(np.random.default_rng(500 + k), k_i)
    W = _w(kind, k, 600 + k)
    want = cdense.sumcheck_layer_lin_raw(k_i, k, *gates, z, W)
    for a in gates + (z, W) + tuple(want):
        a.setflags(write=False)
    return Layer(k_i, *gates), z, W, want


@pytest.mark.parametrize("k_i,k", DEVICE_SHAPES)
def test_device_transcript_layer_at_grid_thresholds(ctx_device, ctx_device_unfused, k_i, k):
    """Coefficients, lengths and challenges of one layer with the fused b-phase round (256 columns exactly, two column blocks, 2 and 8
    rows per chunk, 2048 partials) and with k_layer_round in its place (layer_no_fused: at k = 11 the 2048-block cap with four
    grid-stride trips); every W kind."""
    assert ds.device_row(k) == (ds.DEVICE_ROUND0[k], ds.DEVICE_TRIPS[k])
    assert ctx_device.get_option("layer_no_fused") == 0 and ctx_device_unfused.get_option("layer_no_fused") == 1
    for kind in W_KINDS:
        lay, z, W, want = _device_case(k_i, k, kind)
        lens = want[1]
        if kind == "independent":     # short round vectors in both phases
            assert lens[0] == 2 and lens[k] == 2 and lens[k - 1] == 2 and lens[2 * k - 1] == 2 and (lens == 3).sum() == 2 * (k - 3)
        elif kind == "r_minus_1":
            assert (lens == 2).all()
        else:
            assert (lens == 3).all()
        for c in (ctx_device, ctx_device_unfused):
            assert _same(c.sumcheck_layer_raw(lay, k, z, W), want), (kind, c is ctx_device_unfused)


@pytest.mark.parametrize("unfused", [0, 1])
def test_device_transcript_partials_of_a_larger_layer_do_not_leak(unfused):
    """(13, 11) leaves 2048 partials behind, (10, 8) on the same context writes 256 (128 unfused): its transcript is the one a fresh
    context gives, and the oracle's."""
    assert ds.DEVICE_ROUND0[11][0][3] == 2048 and ds.DEVICE_ROUND0[8] == ((1, 128, 1, 256), 128)
    assert ds.device_row(11)[0] == ds.DEVICE_ROUND0[11] and ds.device_row(8)[0] == ds.DEVICE_ROUND0[8]
    big, small = _device_case(13, 11, "random"), _device_case(10, 8, "random")
    outs = []
    for first in (big, None):
        with Context(0) as c:
            c.set_transcript(N.GKR_TRANSCRIPT_DEVICE)
            c.set_option("layer_no_fused", unfused)
            if first is not None:
                assert _same(c.sumcheck_layer_raw(first[0], 11, first[1], first[2]), first[3])
            outs.append(c.sumcheck_layer_raw(small[0], 8, small[1], small[2]))
    assert _same(outs[0], outs[1]) and _same(outs[0], small[3])


def test_device_transcript_whole_proofs_in_a_batch(ctx_device):
    """ks = [12, 9, 10], three witnesses: run_layer_dense's per-proof offsets of z and W; every array of every proof."""
    ks = [12, 9, 10]
    assert ds.device_row(9)[0] == ds.DEVICE_ROUND0[9] and ds.device_row(10)[0] == ds.DEVICE_ROUND0[10]
    layers = [_gates(ks[i], ks[i + 1], 900 + i) for i in range(2)]
    circuit = GKRCircuit([Layer(ks[i], *layers[i]) for i in range(2)], ks[-1])
    wit = np.stack([synth.rand_fr(np.random.default_rng(910 + b), 1 << ks[-1]) for b in range(3)])
    sc, sl, sr, q, ql, z, rr, dco, ico = ctx_device.prove_batch_raw(circuit, wit, all_arrays=True)
    for b in range(3):
        ref = cdense.prove_raw(layers, wit[b])
        ro = qo = 0
        zo = ks[0]
        assert not z[b, :ks[0]].any()
        for i in range(2):
            k = ks[i + 1]
            assert np.array_equal(sc[b, ro:ro + 2 * k], ref["C"][i]), (b, i)
            assert np.array_equal(sl[b, ro:ro + 2 * k], ref["L"][i]), (b, i)
            assert np.array_equal(sr[b, ro:ro + 2 * k], ref["R"][i]), (b, i)
            assert int(ql[b, i]) == ref["q_len"][i] and np.array_equal(q[b, qo:qo + k + 1], ref["q"][i]), (b, i)
            assert np.array_equal(z[b, zo:zo + k], ref["z"][i + 1]), (b, i)
            ro += 2 * k
            qo += k + 1
            zo += k
        assert np.array_equal(rr[b], ref["r"])
        assert np.array_equal(dco[b], cdense.mobius_raw(ref["values"][0], ks[0]))
        assert np.array_equal(ico[b], cdense.mobius_raw(ref["values"][-1], ks[-1]))
    assert not np.array_equal(sr[0], sr[1]) and not np.array_equal(sr[1], sr[2])


# =========================================================================== layer sessions

SESSION_SHAPES = [(10, 5, 1), (12, 8, 1), (12, 8, 4), (12, 8, 256), (13, 10, 2), (13, 11, 2), (13, 11, 1)]


def _decode(C, L, R, k):
    return [from_limbs(C[j])[3 - int(L[j]):] for j in range(2 * k)], from_limbs(R)


@pytest.mark.parametrize("k_i,k,shards", SESSION_SHAPES)
def test_layer_sessions_at_grid_thresholds(ctx, k_i, k, shards):
    """The trailing-variable split over logical ranks: k_layer_round over several blocks and on its cap, the reduce beyond 64
    partials, k_layer_fold beyond its cap, k_fold_small over two stripes and more, kc != k and kc = 0; W random, and W without its
    last variable (a rank bit whenever there is more than one shard)."""
    assert ds.session_row(k, shards) == ds.SESSION_ROUND0[(k, shards)]
    gates = _gates(k_i, k, 41 * k_i + k + shards)
    lay = Layer(k_i, *gates)
    z = synth.rand_fr(np.random.default_rng(700 + k), k_i)
    rng = np.random.default_rng(701 + k)
    for kind, W in (("random", synth.rand_fr(rng, 1 << k)), ("no last variable", np.repeat(synth.rand_fr(rng, 1 << (k - 1)), 2, axis=0))):
        W = np.ascontiguousarray(W)
        C, L, R = cdense.sumcheck_layer_lin_raw(k_i, k, *gates, z, W)
        assert L[k - 1] == L[2 * k - 1] == (3 if kind == "random" else 2)
        assert parallel.prove_sumcheck_opt_logical(ctx, lay, k, z, W, shards) == _decode(C, L, R, k), kind


def test_layer_sessions_without_column_bits_over_two_blocks(ctx):
    """kc = 0 (as many shards as W has entries, every shard one column) where a shard's b-phase still takes two blocks: k_next = 10
    over 1024 shards is the smallest such split -- (12, 8, 256) above has one block per shard."""
    k_i, k, shards = 8, 10, 1024
    assert ds.session_row(k, shards) == ds.SESSION_ROUND0[(k, shards)] and ds.SESSION_ROUND0[(k, shards)][0] == 2
    gates = _gates(k_i, k, 6060)
    z = synth.rand_fr(np.random.default_rng(6061), k_i)
    W = synth.rand_fr(np.random.default_rng(6062), 1 << k)
    want = _decode(*cdense.sumcheck_layer_lin_raw(k_i, k, *gates, z, W), k)
    assert parallel.prove_sumcheck_opt_logical(ctx, Layer(k_i, *gates), k, z, W, shards) == want


def _fold(t, r):
    h = len(t) // 2
    return [(t[i] + r * (t[i + h] - t[i])) % P for i in range(h)]


def _model_sums(A, M, Wb, Wc):
    """(c0, g(1), c2) of one round over the current tables, from f(b, c) = A (W_b + W_c) + M W_b W_c: the sums of f over the low
    and the high half, and of the leading coefficient of f along the bound variable.  len(Wb) > 1: a b variable is bound, cell
    i = row * len(Wc) + col; else a c variable, cell i = col."""
    h = len(A) // 2
    c0 = g1 = c2 = 0
    ncol = len(Wc)
    for i in range(h):
        if len(Wb) > 1:
            row, col = divmod(i, ncol)
            p0, p1, q0, q1 = Wb[row], Wb[row + len(Wb) // 2], Wc[col], Wc[col]
        else:
            p0, p1, q0, q1 = Wb[0], Wb[0], Wc[i], Wc[i + h]
        a0, a1, m0, m1 = A[i], A[i + h], M[i], M[i + h]
        c0 += a0 * (p0 + q0) + m0 * p0 * q0
        g1 += a1 * (p1 + q1) + m1 * p1 * q1
        c2 += (a1 - a0) * ((p1 + q1) - (p0 + q0)) + (m1 - m0) * (p1 * q1 - p0 * q0)
    return [c0 % P, g1 % P, c2 % P]


def test_layer_session_of_every_shard_against_the_integer_model(ctx):
    """(12, 8) over 4 shards, one shard at a time: sums() of every local round and tail() against Python integers on the oracle's
    sliced predicate tables, folded with the oracle transcript's challenges -- two shards cannot hide an error between them."""
    k_i, k, shards = 12, 8, 4
    log_p, kc = 2, 6
    assert ds.session_row(k, shards) == ds.SESSION_ROUND0[(k, shards)]
    gates = _gates(k_i, k, 5150)
    lay = Layer(k_i, *gates)
    z = synth.rand_fr(np.random.default_rng(5151), k_i)
    W = synth.rand_fr(np.random.default_rng(5152), 1 << k)
    rs = from_limbs(cdense.sumcheck_layer_lin_raw(k_i, k, *gates, z, W)[2])
    tables = [t.reshape(1 << k, 1 << kc, shards, 4) for t in _oracle_predicates(k_i, k, gates, z)]
    w = from_limbs(W)
    total = [[0, 0, 0] for _ in range(2 * k - log_p)]
    for p in range(shards):
        A, M = (from_limbs(np.ascontiguousarray(t[:, :, p])) for t in tables)
        Wb, Wc = list(w), w[p::shards]
        s = parallel.LayerSession.open(ctx, lay, k, z, W, shards, p)
        try:
            for j in range(2 * k - log_p):
                want = _model_sums(A, M, Wb, Wc)
                assert s.sums() == want, (p, j)
                total[j] = [(x + y) % P for x, y in zip(total[j], want)]
                s.bind(rs[j])
                A, M = _fold(A, rs[j]), _fold(M, rs[j])
                if j < k:
                    Wb = _fold(Wb, rs[j])
                else:
                    Wc = _fold(Wc, rs[j])
            assert s.tail() == [A[0], M[0], Wc[0], Wb[0]], p
        finally:
            s.close()
    # and the shards' sums add up to the oracle's round polynomials: the model and the oracle agree
    proof = _decode(*cdense.sumcheck_layer_lin_raw(k_i, k, *gates, z, W), k)[0]
    for j, t in enumerate(total):
        assert parallel.layer_round_vector(t, True) == proof[j], j


@pytest.mark.parametrize("kc", [1, 8, 9, 10, 14])
def test_layer_session_on_explicit_tables(ctx, kc):
    """gkr_layer_session_open_tables (the redundant tail after the all-gather) on its own: all kc rounds against the integer model in
    its c-phase form, an external transcript of fixed challenges with 0, 1 and r - 1 among them."""
    n = 1 << kc
    rng = np.random.default_rng(8000 + kc)
    A, M, Wc = (from_limbs(synth.rand_fr(rng, n)) for _ in range(3))
    A[0], M[n - 1], Wc[n // 2] = P - 1, P - 1, P - 1
    Wb = from_limbs(synth.rand_fr(rng, 1))
    fixed = from_limbs(synth.rand_fr(rng, 4))
    challenges = [fixed[0], 0, fixed[1], 1, fixed[2], P - 1, fixed[3]]
    s = parallel.LayerSession.open_tables(ctx, kc, A, M, Wb[0], Wc)
    try:
        with pytest.raises(GkrError):
            s.tail()
        for j in range(kc):
            assert s.sums() == _model_sums(A, M, Wb, Wc), j
            r = challenges[j % len(challenges)]
            s.bind(r)
            A, M, Wc = _fold(A, r), _fold(M, r), _fold(Wc, r)
        assert s.tail() == [A[0], M[0], Wc[0], Wb[0]]
        for call in (s.sums, lambda: s.bind(5)):
            with pytest.raises(GkrError) as e:
                call()
            assert e.value.status == N.GKR_ERR_INVALID
    finally:
        s.close()


def test_layer_session_on_explicit_tables_refusals(ctx):
    ok = to_limbs([1, 2, 3, 4])
    for kc in (0, 15):
        with pytest.raises(GkrError) as e:
            parallel.LayerSession.open_tables(ctx, kc, [1] * (1 << kc), [1] * (1 << kc), 1, [1] * (1 << kc))
        assert e.value.status == N.GKR_ERR_INVALID
    modulus = np.array([gp._limbs(P)], dtype=np.uint64)
    for which in range(4):       # A, M, wb, Wc with an entry = r
        args = [ok.copy(), ok.copy(), ok[:1].copy(), ok.copy()]
        args[which][-1] = modulus[0]
        h = ctypes.c_void_p()
        rc = N.lib().gkr_layer_session_open_tables(ctx._h, ctypes.c_int(2), *[_p(a) for a in args], ctypes.byref(h))
        assert rc == N.GKR_ERR_NON_CANONICAL and not h.value, which
    s = parallel.LayerSession.open_tables(ctx, 2, [1, 2, 3, 4], [5, 6, 7, 8], 9, [10, 11, 12, 13])
    assert s.sums() == _model_sums([1, 2, 3, 4], [5, 6, 7, 8], [9], [10, 11, 12, 13])
    s.close()


# =========================================================================== plain sessions

def _mle_tables(n, log_p, seed):
    """random; constant across a shard's last local variable but for ONE pair in the last block of the shard's upper half (every
    shard alike: no dependence on a rank bit); constant across it everywhere while the shards differ."""
    rng = np.random.default_rng(seed)
    shards, half = 1 << log_p, 1 << (n - log_p - 1)
    t1 = synth.rand_fr(rng, 1 << n)
    t2 = np.broadcast_to(synth.rand_fr(rng, half)[:, None, None, :], (half, 2, shards, 4)).copy()
    t2[half - 1, 1] = synth.rand_fr(rng, 1)[0]
    t3 = np.broadcast_to(synth.rand_fr(rng, half * shards).reshape(half, 1, shards, 4), (half, 2, shards, 4)).copy()
    return [np.ascontiguousarray(t.reshape(-1, 4)) for t in (t1, t2, t3)]


@pytest.mark.parametrize("n,shards", [(17, 1), (17, 4), (21, 2)])
def test_plain_sessions_at_grid_thresholds(ctx, n, shards):
    """gkr_mle_session_* over logical ranks: shards of 2^17, 2^15 and 2^20 entries (256, 64 and 2048 blocks in the first round); the
    length of the last round vector, which hangs on one pair in the last block or on the rank bit alone."""
    log_p = shards.bit_length() - 1
    assert product_geometry(n - log_p, 1)[0][0] == ds.MLE_SESSION_ROUND0[n - log_p]
    last_lens = []
    for t in _mle_tables(n, log_p, 50 + n + shards):
        C, L, R = cdense.sumcheck_mle_raw(t, n)
        want = [from_limbs(C[j])[2 - int(L[j]):] for j in range(n)], from_limbs(R)
        last_lens.append(int(L[n - 1]))
        ptrs = []
        try:
            for p in range(shards):
                part = np.ascontiguousarray(t[p::shards])
                ptrs.append(ctx.alloc(part.nbytes))
                ctx.upload(ptrs[-1], part)
            assert parallel.prove_sumcheck_logical(ctx, ptrs, n) == want
        finally:
            for d in ptrs:
                ctx.free(d)
    assert last_lens[0] == 2 and sorted(last_lens[1:]) == [1, 2] and last_lens[1] == (2 if shards == 1 else 1)

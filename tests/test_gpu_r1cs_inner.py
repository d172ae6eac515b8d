"""gkr_r1cs_cols_* / gkr_r1cs_inner* (csrc/kernels_r1cs.hip, csrc/capi_r1cs.hip) through the C ABI: the table T bit-exact against
the integer model of tests/r1cs_cols_model.py, and the inner sumcheck byte for byte against gkr_sumcheck_product_batch_device on
the model's tables.

  a. the table against the model: sizes around the 256-thread block, padding, several blocks, coefficient and rho mixes, random
     and boolean points, batches with a stride, canaries in the gaps and behind the batch;
  b. column lengths: the three kernels writing one table, the lengths around the long-column cut, the wave's loop and the
     segment length; wire 0 in every constraint of all three matrices; other segment lengths give the same table;
  c. the call: byte equality, the link to the zero-check's claims, the evaluations, the host verifier, the product verifier on
     the device, the host entry point;
  d. a witness past 4 GiB;
  e. one context: workspaces, a rows and a cols handle, two cols handles, a foreign handle, the argument checks that need a handle."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError, synth
from gkr_amd import _native as N
from gkr_amd.convert import R1cs
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import r1cs_matrix_evals, verify_r1cs_inner
from r1cs_cols_model import LONG_COL, cols_table, n_y_of
from r1cs_rows_model import table_log2

pytestmark = pytest.mark.gpu

SEG = N.GKR_R1CS_COL_SEGMENT
CANARY = 0xC3C3C3C3C3C3C3C3
COEFF_MIX = ["ones", "minus_ones", "random", "minus_one_and_two"]
R_LIMBS = np.array([P & (2**64 - 1), (P >> 64) & (2**64 - 1), (P >> 128) & (2**64 - 1), P >> 192], dtype=np.uint64)   # the entry r


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _coeff(kind, rng):
    if kind == "ones":
        return 1
    if kind == "minus_ones":
        return P - 1
    if kind == "random":
        return rng.randrange(1, P)
    return (P - 1, 2)[rng.randrange(2)]


def _random_constraints(rng, n_constraints, n_wires, kind):
    """Rows of 0 .. 4 terms (a wire may repeat)."""
    return [tuple([(_coeff(kind, rng), rng.randrange(n_wires)) for _ in range(rng.randrange(5))] for _ in range(3))
            for _ in range(n_constraints)]


def _rho(kind, rng):
    return {"zero": 0, "one": 1, "minus_one": P - 1}.get(kind, rng.randrange(P))


def _point(rng, n, boolean):
    return [rng.randrange(2) if boolean else rng.randrange(P) for _ in range(n)]


def _model(cons, n_wires, xs, rhos):
    """The model's tables of a batch as (batch, 2^n_y, 4) limbs."""
    n_y = n_y_of(n_wires)
    return np.stack([to_limbs(cols_table(cons, n_wires, x, rho, n_y)) for x, rho in zip(xs, rhos)])


def _run_cols(ctx, r1cs, xs, rhos, stride=None, segment=None):
    """-> (batch, 2^n_y, 4) limbs.  The tables lie `stride` elements apart in a buffer filled with a canary that the gaps and the
    slot behind the batch keep."""
    inf = r1cs.csc_info()
    n_y, batch = inf["n_y"], len(xs)
    stride = (1 << n_y) if stride is None else stride
    out = np.full(((batch + 1) * stride, 4), CANARY, dtype=np.uint64)
    d_out = ctx.alloc(out.nbytes)
    try:
        ctx.upload(d_out, out)
        with ctx.r1cs_cols(r1cs, segment=segment) as handle:
            assert handle.info() == inf
            ctx.r1cs_cols_device(handle, xs, rhos, batch, d_out, stride=stride)
        got = ctx.download(d_out, out.shape).reshape(batch + 1, stride, 4)
    finally:
        ctx.free(d_out)
    assert (got[batch] == np.uint64(CANARY)).all(), "nothing is written past the batch"
    assert (got[:batch, 1 << n_y:] == np.uint64(CANARY)).all(), "nothing is written between the tables"
    return np.ascontiguousarray(got[:batch, :1 << n_y])


# ---- a. the table against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n_wires", [1, 3, 4, 5, 255, 256, 257, 1000, 16384 + 1])
def test_table_matches_the_model(ctx, n_wires, batch):
    """Sumcheck 1 of a batch of three has rho = (0, 0, 0): the zero table.  The other weights cycle through 0, 1, r - 1 and random
    values; boolean and random points alternate."""
    rng = random.Random(19100 + 7 * n_wires + batch)
    n_constraints = 41 + n_wires % 13 if n_wires < 1000 else 3000
    kind = COEFF_MIX[(n_wires + batch) % 4]
    cons = _random_constraints(rng, n_constraints, n_wires, kind)
    n_x, n_y = table_log2(n_constraints), n_y_of(n_wires)
    kinds = ["zero", "one", "minus_one", "random"]
    rhos = [[_rho(kinds[(n_wires + b + m) % 4], rng) for m in range(3)] for b in range(batch)]
    if batch == 3:
        rhos[1] = [0, 0, 0]
    xs = [_point(rng, n_x, (n_wires + b) % 2 == 1) for b in range(batch)]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    assert r1cs.csc_info()["n_y"] == n_y and r1cs.csc_info()["n_x"] == n_x
    got = _run_cols(ctx, r1cs, xs, rhos, stride=None if batch == 1 else (1 << n_y) + 3)
    assert np.array_equal(got, _model(cons, n_wires, xs, rhos))
    assert not got[:, n_wires:].any(), "padding y >= n_wires is zero"
    if batch == 3:
        assert not got[1].any()


@pytest.mark.parametrize("coeffs", COEFF_MIX)
@pytest.mark.parametrize("rho", ["zero", "one", "minus_one", "random"])
def test_every_rho_under_every_coefficient_mix(ctx, rho, coeffs):
    rng = random.Random(19200 + 5 * len(rho) + len(coeffs))
    n_constraints, n_wires = 300, 53
    cons = _random_constraints(rng, n_constraints, n_wires, coeffs)
    rhos = [[_rho(rho, rng) for _ in range(3)], [_rho(rho, rng), rng.randrange(P), 0]]
    xs = [_point(rng, 9, False), _point(rng, 9, True)]
    got = _run_cols(ctx, R1cs.build(n_wires, 1, 1, 1, cons), xs, rhos, stride=64 + 1)
    assert np.array_equal(got, _model(cons, n_wires, xs, rhos))


# ---- b. column lengths ------------------------------------------------------------------------------------------------------------------
def _system_of_column_lengths(lens, kinds):
    """Column y of matrix m has lens[m][y] records: wire y stands in the constraints 0 .. lens[m][y] - 1 of matrix m, with a
    coefficient of the column's kind (products for the long ones of kind r - 2, the addition path for 1 and r - 1)."""
    n_wires = len(lens[0])
    n_constraints = max(max(l) for l in lens)
    cons = []
    for i in range(n_constraints):
        con = []
        for m in range(3):
            con.append([(kinds[(y + m) % 3] if lens[m][y] > 8 else (kinds[(y + m) % 3], 1, P - 1, 12345)[(i + y) % 4], y)
                        for y in range(n_wires) if i < lens[m][y]])
        cons.append(tuple(con))
    return n_wires, cons


def test_column_lengths_around_the_cut_the_wave_loop_and_the_segment(ctx):
    """One R1CS whose table all three kernels write.  A: 0, 1, LONG_COL - 1 .. LONG_COL + 1, 63 .. 65, 127 .. 129, 4097, SEG - 1 ..
    SEG + 1 and, as the LAST column of a table without padding (n_wires = 16 = 2^n_y), 2 SEG + 1 records.  B: the same lengths
    the other way round, so most columns are long in one matrix and short in another; column 4 (33 records in A) has 1 in B and 2
    in C: long in one matrix, short in the other two.  C: short columns only, column 0 empty in all three.  Other segment lengths
    (none, 512, 64) give the same table."""
    lens_a = [0, 1, LONG_COL - 1, LONG_COL, LONG_COL + 1, 63, 64, 65, 127, 128, 129, 4097, SEG - 1, SEG, SEG + 1, 2 * SEG + 1]
    lens_b = [0] + lens_a[:0:-1]
    lens_b[4] = 1
    lens_c = [0, LONG_COL, 1, 1, 2, 1, 1, 1, 1, 1, LONG_COL - 1, 1, 1, 1, 1, 3]
    kinds = [P - 2, P - 1, 1]
    n_wires, cons = _system_of_column_lengths([lens_a, lens_b, lens_c], kinds)
    assert n_wires == 16 and len(cons) == max(4097, 2 * SEG + 1)
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    inf = r1cs.csc_info()
    assert inf["n_y"] == 4 and inf["n_long_cols"] == [12, 11, 0]
    for m, lens in enumerate((lens_a, lens_b, lens_c)):
        col_ptr, _, long_cols, _ = r1cs.csc(m)
        assert np.diff(col_ptr.astype(np.int64)).tolist() == lens
        assert long_cols.tolist() == [y for y, l in enumerate(lens) if l > LONG_COL]
    rng = random.Random(19300)
    n_x = inf["n_x"]
    xs = [_point(rng, n_x, False), _point(rng, n_x, False), [0] * n_x]                 # the last one picks row 0: the plain sum of its records
    rhos = [[rng.randrange(P) for _ in range(3)], [1, P - 1, rng.randrange(P)], [P - 1, P - 1, P - 1]]
    want = _model(cons, n_wires, xs, rhos)
    got = _run_cols(ctx, r1cs, xs, rhos, stride=16 + 5)
    assert np.array_equal(got, want)
    assert not got[:, 0].any() and got[0, 15].any()
    for segment in (0, 512, 64):
        assert np.array_equal(_run_cols(ctx, r1cs, xs, rhos, segment=segment), want), segment


def test_wire_zero_in_every_constraint_of_all_three_matrices(ctx):
    """16 385 constraints (n_x = 15), wire 0 with a record in each of them in A, B and C at once -- 9 segments per matrix at the
    default length -- beside short columns; all-max eq entries cannot be arranged, all-max coefficients can (r - 1 and r - 2)."""
    rng = random.Random(19400)
    n_constraints, n_wires = 16384 + 1, 50
    cons = [([(P - 2, 0), (1, 1 + i % 49)], [(P - 1, 0)], [(1 + i % 3, 0), (P - 1, 1 + (5 * i) % 49), (5, 0)]) for i in range(n_constraints)]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    inf = r1cs.csc_info()
    assert inf["n_x"] == 15 and inf["n_y"] == 6 and inf["n_long_cols"] == [50, 1, 50]
    assert int(r1cs.csc(2)[0][1]) == 2 * n_constraints                      # wire 0 twice in every row of C
    xs = [_point(rng, 15, False), _point(rng, 15, False)]
    rhos = [[rng.randrange(P) for _ in range(3)], [0, 1, 0]]
    got = _run_cols(ctx, r1cs, xs, rhos, stride=64 + 1)
    assert np.array_equal(got, _model(cons, n_wires, xs, rhos))
    assert not got[1, 1:].any() and got[1, 0].any()                        # B has wire 0 alone


# ---- c. the call ------------------------------------------------------------------------------------------------------------------------
def _systems():
    four = [([(1, 1)], [(1, 2)], [(1, 3)]), ([(1, 3)], [(1, 0)], [(1, 3)]), ([(2, 0), (P - 1, 1)], [(1, 0)], [(2, 0), (P - 1, 1)])]
    five = [([(1, 1)], [(1, 2)], [(1, 3)]), ([(1, 3), (5, 0)], [(P - 1, 1)], [(1, 4)]), ([(2, 4)], [(1, 4), (1, 1)], [(1, 5)]),
            ([(1, 5)], [(1, 0)], [(1, 5)]), ([(1, 0)], [(7, 0)], [(7, 0)])]

    def four_witness(x, y):
        return [1, x, y, x * y % P]

    def five_witness(x, y):
        w3 = x * y % P
        w4 = (w3 + 5) * (P - x) % P
        return [1, x, y, w3, w4, 2 * w4 * (w4 + x) % P]
    return {"four": (4, four, four_witness), "five": (6, five, five_witness),
            "mimc91": synth.mimc7_demo_constraints(91) + (lambda x, y: synth.mimc7_demo_witness(x, y, nrounds=91),),
            "mimc4000": synth.mimc7_demo_constraints(4000) + (lambda x, y: synth.mimc7_demo_witness(x, y, nrounds=4000),)}


@pytest.fixture(scope="module")
def systems():
    return _systems()


def _claim(C, b):
    g = from_limbs(C[b, 0])
    return (sum(g) + g[-1]) % P                                   # g_1(0) + g_1(1); the unused leading slots are zero


def _upload_witnesses(ctx, wits, n_wires, stride):
    W = np.full((len(wits) * stride, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    for b, w in enumerate(wits):
        W[b * stride:b * stride + n_wires] = to_limbs(w)
    d_w = ctx.alloc(W.nbytes)
    ctx.upload(d_w, W)
    return d_w, W


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["four", "five", "mimc91", "mimc4000"])
def test_inner_is_the_product_sumcheck_on_the_models_tables(ctx, systems, name, batch):
    """The two-call sequence: the zero-check, then the inner sumcheck at its challenges.  Sumcheck 1 of a batch of three has a
    broken witness: the identity holds for it all the same."""
    n_wires, cons, witness = systems[name]
    n_x, n_y = table_log2(len(cons)), n_y_of(n_wires)
    assert n_y == {"four": 2, "five": 3, "mimc91": 9, "mimc4000": 14}[name]
    rng = random.Random(19500 + n_y + batch)
    wits = [witness(2 + b, 3 + b) for b in range(batch)]
    if batch == 3:
        wits[1][n_wires - 1] = (wits[1][n_wires - 1] + 1) % P
    zs = [_point(rng, n_x, False) for _ in range(batch)]
    rhos = [[rng.randrange(1, P) for _ in range(3)] for _ in range(batch)]
    stride = n_wires + 2
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    d_w, W = _upload_witnesses(ctx, wits, n_wires, stride)
    d_t = ctx.alloc((batch * 2 << n_y) * 32)
    try:
        with ctx.r1cs_rows(r1cs) as rows_handle:
            _, _, RX, EX, _, bad = ctx.r1cs_zerocheck_batch_device(rows_handle, d_w, batch, zs, stride=stride)
        assert [int(v) != 0xFFFFFFFF for v in bad] == [batch == 3 and b == 1 for b in range(batch)]
        xs = [from_limbs(RX[b]) for b in range(batch)]
        with ctx.r1cs_cols(r1cs) as handle:
            got = ctx.r1cs_inner_batch_device(handle, d_w, batch, RX, rhos, stride=stride)
        assert np.array_equal(ctx.download(d_w, W.shape), W), "the witnesses are not modified"
        # the model's tables {T_b, w_b padded} and the product path on them
        T = np.zeros((batch, 2, 1 << n_y, 4), dtype=np.uint64)
        T[:, 0] = _model(cons, n_wires, xs, rhos)
        for b, w in enumerate(wits):
            T[b, 1, :n_wires] = to_limbs(w)
        ctx.upload(d_t, T)
        want = ctx.sumcheck_product_batch_device(d_t, n_y, 2, batch)
        for what, g, w in zip(("coeffs", "len", "r", "evals"), got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), what
        C, L, R, E = got
        claims = []
        for b in range(batch):
            abc = from_limbs(EX[b])
            claims.append(sum(r * v for r, v in zip(rhos[b], abc)) % P)
            assert _claim(C, b) == claims[b]                      # g_1(0) + g_1(1) = sum_m rho_m (the zero-check's out_evals)
            ry, ev = from_limbs(R[b]), from_limbs(E[b])
            assert ev[0] == sum(r * v for r, v in zip(rhos[b], r1cs_matrix_evals(cons, xs[b], ry))) % P
            proof = [from_limbs(C[b, j])[3 - int(L[b, j]):] for j in range(n_y)]
            assert verify_r1cs_inner(cons, xs[b], rhos[b], abc, proof, ry, ev) == (ry, ev[1])
            assert verify_r1cs_inner(cons, xs[b], rhos[b], [abc[0], abc[1], (abc[2] + 1) % P], proof, ry, ev) is None
        # w~(r_y): one evaluation of the padded witness
        Wp = np.ascontiguousarray(T[:, 1])
        ctx.upload(d_t, Wp)
        assert np.array_equal(ctx.mle_eval_batch_device(d_t, n_y, batch, R), E[:, 1])
        # the transcripts through the product verifier on the tables
        ctx.upload(d_t, T)
        accept, rnd, check, out_claims, out_evals = ctx.verify_sumcheck_product_batch_device(d_t, n_y, 2, batch, C, L, R, to_limbs(claims))
        assert accept.all() and (check == N.GKR_VERIFY_OK).all() and np.array_equal(out_evals, E)
    finally:
        ctx.free(d_w)
        ctx.free(d_t)
    if batch == 1:                                                # the host entry point
        proof, r, evals = ctx.prove_r1cs_inner(r1cs, wits[0], xs[0], rhos[0])
        assert proof == [from_limbs(C[0, j])[3 - int(L[0, j]):] for j in range(n_y)] and r == from_limbs(R[0]) and evals == from_limbs(E[0])


def test_a_zero_rho_gives_the_all_zero_transcript_and_bad_inputs_are_refused(ctx, systems):
    n_wires, cons, witness = systems["mimc91"]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    rng = random.Random(19600)
    x = _point(rng, 9, False)
    w = witness(5, 6) + [P - 1, 17]                               # n_witness > n_wires: the tail is not read
    proof, r, evals = ctx.prove_r1cs_inner(r1cs, w, x, [0, 0, 0])
    assert proof == [[0]] * 9 and evals[0] == 0
    proof2, _, _ = ctx.prove_r1cs_inner(r1cs, w, x, [1, 2, 3])
    assert proof2 != proof and len(proof2[0]) == 3
    limbs = to_limbs(w)
    limbs[100] = R_LIMBS
    xl = to_limbs(x).reshape(1, 9, 4)
    xl[0, 4] = R_LIMBS
    rl = to_limbs([1, 2, 3]).reshape(1, 3, 4)
    rl[0, 2] = R_LIMBS
    for call in (lambda: ctx.prove_r1cs_inner(r1cs, limbs, x, [1, 2, 3]), lambda: ctx.prove_r1cs_inner(r1cs, w, xl, [1, 2, 3]),
                 lambda: ctx.prove_r1cs_inner(r1cs, w, x, rl)):
        with pytest.raises(GkrError) as e:
            call()
        assert e.value.status == N.GKR_ERR_NON_CANONICAL
    with pytest.raises(GkrError) as e:
        ctx.prove_r1cs_inner(r1cs, w[:n_wires - 1], x, [1, 2, 3])
    assert e.value.status == N.GKR_ERR_INVALID


# ---- d. offsets -------------------------------------------------------------------------------------------------------------------------
def test_a_witness_past_four_gib(ctx, systems):
    """Batch 2 with a stride of 2^27 + 5 elements: witness 1 starts 160 bytes past 4 GiB.  Only the two witnesses' own entries are
    uploaded; sumcheck 1's transcript equals the same witness run alone."""
    n_wires, cons, witness = systems["mimc91"]
    stride = (1 << 27) + 5
    assert stride * 32 > 1 << 32
    wits = [witness(2, 3), witness(11, 3)]
    wits[1][77] = (wits[1][77] + 1) % P
    rng = random.Random(19700)
    xs = [_point(rng, 9, False) for _ in range(2)]
    rhos = [[rng.randrange(P) for _ in range(3)] for _ in range(2)]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    d_w = ctx.alloc((stride + n_wires) * 32)
    try:
        second = ctypes.c_void_p(d_w.value + stride * 32)
        ctx.upload(d_w, to_limbs(wits[0]))
        ctx.upload(second, to_limbs(wits[1]))
        with ctx.r1cs_cols(r1cs) as handle:
            both = ctx.r1cs_inner_batch_device(handle, d_w, 2, xs, rhos, stride=stride)
            alone = ctx.r1cs_inner_batch_device(handle, second, 1, xs[1:], rhos[1:])
            first = ctx.r1cs_inner_batch_device(handle, d_w, 1, xs[:1], rhos[:1])
    finally:
        ctx.free(d_w)
    for g, a, f in zip(both, alone, first):
        assert np.array_equal(g[1:], a) and np.array_equal(g[:1], f)
    assert not np.array_equal(both[0][:1], alone[0])
    assert from_limbs(both[3][1])[1] != from_limbs(both[3][0])[1]


# ---- e. one context ---------------------------------------------------------------------------------------------------------------------
def test_one_context_two_handles_and_a_foreign_handle(ctx, systems):
    """A rows handle and a cols handle in use alternately, two cols handles of different R1CS alive at once, a zero-check, a product
    call and an inner call interleaved: equal results.  A handle on another context, and the other argument checks that need a
    handle: GKR_ERR_INVALID; an x or rho entry >= r: GKR_ERR_NON_CANONICAL through the context."""
    nw_a, cons_a, wit_a = systems["mimc91"]
    nw_b, cons_b, wit_b = systems["five"]
    rng = random.Random(19800)
    Wa, Wb = to_limbs(wit_a(4, 1)), to_limbs(wit_b(9, 8))
    za, xa, xb = [_point(rng, 9, False)], [_point(rng, 9, False)], [_point(rng, 3, False)]
    ra, rb = [[rng.randrange(P) for _ in range(3)]], [[rng.randrange(P) for _ in range(3)]]
    other = np.random.default_rng(19801).integers(0, 1 << 60, size=(2 * 2 << 11, 4), dtype=np.uint64)
    r1cs_a, r1cs_b = R1cs.build(nw_a, 1, 1, 1, cons_a), R1cs.build(nw_b, 1, 1, 1, cons_b)
    d_a, d_b, d_o = ctx.alloc(Wa.nbytes), ctx.alloc(Wb.nbytes), ctx.alloc(other.nbytes)
    try:
        ctx.upload(d_a, Wa)
        ctx.upload(d_b, Wb)
        ctx.upload(d_o, other)
        with ctx.r1cs_rows(r1cs_a) as rows_a, ctx.r1cs_cols(r1cs_a) as ha, ctx.r1cs_cols(r1cs_b) as hb:
            zc1 = ctx.r1cs_zerocheck_batch_device(rows_a, d_a, 1, za)
            first = ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, ra)
            small = ctx.r1cs_inner_batch_device(hb, d_b, 1, xb, rb)
            between = ctx.sumcheck_product_batch_device(d_o, 11, 2, 2)
            zc2 = ctx.r1cs_zerocheck_batch_device(rows_a, d_a, 1, za)
            third = ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, ra)
            small2 = ctx.r1cs_inner_batch_device(hb, d_b, 1, xb, rb)
            again = ctx.sumcheck_product_batch_device(d_o, 11, 2, 2)
            for one, two in ((zc1, zc2), (first, third), (small, small2), (between, again)):
                assert all(np.array_equal(x, y) for x, y in zip(one, two))
            with Context(0) as c2:
                d2 = c2.alloc(Wa.nbytes)
                try:
                    c2.upload(d2, Wa)
                    with c2.r1cs_cols(r1cs_a) as h2:
                        assert all(np.array_equal(x, y) for x, y in zip(between, c2.sumcheck_product_batch_device(d_o, 11, 2, 2)))
                        assert all(np.array_equal(x, y) for x, y in zip(first, c2.r1cs_inner_batch_device(h2, d2, 1, xa, ra)))
                        for call in (lambda: ctx.r1cs_inner_batch_device(h2, d_a, 1, xa, ra), lambda: ctx.r1cs_cols_device(h2, xa, ra, 1, d_o),
                                     lambda: c2.r1cs_cols_device(ha, xa, ra, 1, d_o), lambda: c2.r1cs_inner_batch_device(ha, d2, 1, xa, ra)):
                            with pytest.raises(GkrError) as e:
                                call()
                            assert e.value.status == N.GKR_ERR_INVALID
                finally:
                    c2.free(d2)
            # batch outside 1 .. 65535, a witness stride below n_wires, an output stride below 2^n_y
            for batch in (0, -1, 65536):
                for call in (lambda: ctx.r1cs_cols_device(ha, np.zeros((max(batch, 0), 9, 4), dtype=np.uint64), np.zeros((max(batch, 0), 3, 4), dtype=np.uint64), batch, d_o),
                             lambda: ctx.r1cs_inner_batch_device(ha, d_a, batch, np.zeros((max(batch, 0), 9, 4), dtype=np.uint64), np.zeros((max(batch, 0), 3, 4), dtype=np.uint64))):
                    with pytest.raises(GkrError) as e:
                        call()
                    assert e.value.status == N.GKR_ERR_INVALID, batch
            for call in (lambda: ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, ra, stride=nw_a - 1), lambda: ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, ra, stride=0),
                         lambda: ctx.r1cs_cols_device(ha, xa, ra, 1, d_o, stride=511), lambda: ctx.r1cs_cols_device(ha, xa, ra, 1, d_o, stride=0)):
                with pytest.raises(GkrError) as e:
                    call()
                assert e.value.status == N.GKR_ERR_INVALID
            # NULL pointers behind a good handle (out_evals alone may be NULL)
            lib, word = N.lib(), (ctypes.c_uint64 * 512)()
            fake = ctypes.c_void_p(ctypes.addressof(word))
            good = [ctx._h, ha._h, d_a, nw_a, 1, fake, fake, fake, fake, fake, None]
            for at in (0, 1, 2, 5, 6, 7, 8, 9):
                args = list(good)
                args[at] = None
                assert lib.gkr_r1cs_inner_batch_device(*args) == N.GKR_ERR_INVALID, at
            good = [ctx._h, ha._h, fake, fake, 1, d_o, 512]
            for at in (0, 1, 2, 3, 5):
                args = list(good)
                args[at] = None
                assert lib.gkr_r1cs_cols_device(*args) == N.GKR_ERR_INVALID, at
            # an x or rho entry >= r
            xl, rl = to_limbs(xa[0]).reshape(1, 9, 4), to_limbs(ra[0]).reshape(1, 3, 4)
            xl[0, 8] = R_LIMBS
            rl[0, 0] = R_LIMBS
            for call in (lambda: ctx.r1cs_inner_batch_device(ha, d_a, 1, xl, ra), lambda: ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, rl),
                         lambda: ctx.r1cs_cols_device(ha, xl, ra, 1, d_o), lambda: ctx.r1cs_cols_device(ha, xa, rl, 1, d_o)):
                with pytest.raises(GkrError) as e:
                    call()
                assert e.value.status == N.GKR_ERR_NON_CANONICAL
            assert all(np.array_equal(x, y) for x, y in zip(first, ctx.r1cs_inner_batch_device(ha, d_a, 1, xa, ra)))
        # batch * 2 * 2^n_y above 2^30 (n_y = 14: 32769 sumchecks), batch * 2^n_x above 2^30 (n_x = 15, n_y = 6: 32769 sumchecks)
        nw_c, cons_c, _ = systems["mimc4000"]
        with ctx.r1cs_cols(R1cs.build(nw_c, 1, 1, 1, cons_c)) as hc:
            assert 32769 * 2 << 14 > 1 << 30 >= 32768 * 2 << 14 and 32769 << 14 <= 1 << 30
            for call in (lambda: ctx.r1cs_cols_device(hc, np.zeros((32769, 14, 4), dtype=np.uint64), np.zeros((32769, 3, 4), dtype=np.uint64), 32769, d_o),
                         lambda: ctx.r1cs_inner_batch_device(hc, d_a, 32769, np.zeros((32769, 14, 4), dtype=np.uint64), np.zeros((32769, 3, 4), dtype=np.uint64),
                                                             stride=nw_c)):
                with pytest.raises(GkrError) as e:
                    call()
                assert e.value.status == N.GKR_ERR_INVALID
        tall = [([(1, i % 50)], [(1, 0)], [(1, (i + 1) % 50)]) for i in range(16384 + 1)]
        with ctx.r1cs_cols(R1cs.build(50, 1, 1, 1, tall)) as ht:
            assert ht.info()["n_x"] == 15 and ht.info()["n_y"] == 6 and 32769 << 15 > 1 << 30 >= 32768 << 15 and 32769 * 2 << 6 <= 1 << 30
            for call in (lambda: ctx.r1cs_cols_device(ht, np.zeros((32769, 15, 4), dtype=np.uint64), np.zeros((32769, 3, 4), dtype=np.uint64), 32769, d_o),
                         lambda: ctx.r1cs_inner_batch_device(ht, d_a, 32769, np.zeros((32769, 15, 4), dtype=np.uint64), np.zeros((32769, 3, 4), dtype=np.uint64),
                                                             stride=50)):
                with pytest.raises(GkrError) as e:
                    call()
                assert e.value.status == N.GKR_ERR_INVALID
    finally:
        ctx.free(d_a)
        ctx.free(d_b)
        ctx.free(d_o)

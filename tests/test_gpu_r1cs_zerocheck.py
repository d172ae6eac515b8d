"""gkr_r1cs_rows_* / gkr_r1cs_zerocheck* (csrc/kernels_r1cs.hip, csrc/capi_r1cs.hip) through the C ABI: the tables Az, Bz, Cz bit-exact
against the integer model of tests/r1cs_rows_model.py, and the zero-check on them byte for byte against
gkr_sumcheck_zerocheck_batch_device on the model's tables.

  a. rows against the model: table sizes around the 256-thread block, padding, several blocks, witness and coefficient mixes,
     batches with a stride, inputs unmodified, nothing written past the batch;
  b. row lengths: both kernels writing one table, the lengths around the long-row cut and the wave's loop, all-max operands;
  c. first_bad;
  d. the zero-check: byte equality, claims, the host verifier, the SOP verifier on the device, the host entry point;
  e. a witness past 4 GiB;
  f. one context: workspaces, two handles, a foreign handle, the argument checks that need a handle."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError, synth
from gkr_amd import _native as N
from gkr_amd.convert import R1cs
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import R1CS_ZEROCHECK_TERMS, verify_sumcheck_zerocheck
from r1cs_rows_model import LONG_ROW, first_bad, rows, table_log2
from sop_model import limbs_to_object
from zerocheck_model import lift_terms, zerocheck_claim_np

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TERMS = R1CS_ZEROCHECK_TERMS
WITNESS_MIX = ["random", "all_max", "zero", "bits"]
COEFF_MIX = ["ones", "minus_ones", "random", "minus_one_and_two"]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _witness(kind, n_wires, rng):
    if kind == "random":
        return [rng.randrange(P) for _ in range(n_wires)]
    if kind == "all_max":
        return [P - 1] * n_wires
    if kind == "zero":
        return [0] * n_wires
    return [rng.randrange(2) for _ in range(n_wires)]


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


def _tables(cons, wits, n):
    """The model's tables of a batch as (batch, 3, 2^n, 4) limbs."""
    return np.stack([np.stack([to_limbs(t) for t in rows(cons, w, n)]) for w in wits])


def _run_rows(ctx, r1cs, wits, stride, check=True):
    """-> ((batch, 3, 2^n, 4) limbs, first_bad).  The witnesses lie `stride` elements apart in a buffer filled with a pattern; the
    buffer is downloaded afterwards and must be what was uploaded; the table slot behind the batch keeps its canary."""
    inf = r1cs.csr_info()
    n, nw, batch = inf["n"], inf["n_wires"], len(wits)
    W = np.full((batch * stride, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    for b, w in enumerate(wits):
        W[b * stride:b * stride + nw] = to_limbs(w)
    out = np.full(((batch + 1) * 3 << n, 4), 0xC3C3C3C3C3C3C3C3, dtype=np.uint64)
    d_w, d_out = ctx.alloc(W.nbytes), ctx.alloc(out.nbytes)
    try:
        ctx.upload(d_w, W)
        ctx.upload(d_out, out)
        with ctx.r1cs_rows(r1cs) as handle:
            assert handle.info() == inf
            bad = ctx.r1cs_rows_device(handle, d_w, batch, d_out, stride=stride, check=check)
        got = ctx.download(d_out, out.shape)
        assert np.array_equal(ctx.download(d_w, W.shape), W), "the witnesses are not modified"
    finally:
        ctx.free(d_w)
        ctx.free(d_out)
    assert (got[batch * 3 << n:] == np.uint64(0xC3C3C3C3C3C3C3C3)).all(), "nothing is written past the batch"
    return got[:batch * 3 << n].reshape(batch, 3, 1 << n, 4), bad


def _want_bad(cons, wits, n):
    return [NONE if (i := first_bad(cons, w, n)) is None else i for w in wits]


# ---- a. rows against the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n_constraints", [1, 3, 4, 5, 255, 256, 257, 1000, 16384 + 1])
def test_rows_match_the_model(ctx, n_constraints, batch):
    rng = random.Random(18100 + 7 * n_constraints + batch)
    n_wires = 37 + n_constraints % 11
    assert n_wires & (n_wires - 1)
    kind = COEFF_MIX[(n_constraints + batch) % 4]
    cons = _random_constraints(rng, n_constraints, n_wires, kind)
    wits = [_witness(WITNESS_MIX[(n_constraints + b) % 4], n_wires, rng) for b in range(batch)]
    n = table_log2(n_constraints)
    got, bad = _run_rows(ctx, R1cs.build(n_wires, 1, 1, 1, cons), wits, n_wires if batch == 1 else n_wires + 5)
    assert got.shape[2] == 1 << n and np.array_equal(got, _tables(cons, wits, n))
    assert not got[:, :, n_constraints:].any(), "rows past n_constraints are zero"
    assert bad.tolist() == _want_bad(cons, wits, n)


@pytest.mark.parametrize("coeffs", COEFF_MIX)
@pytest.mark.parametrize("witness", WITNESS_MIX)
def test_every_witness_mix_under_every_coefficient_mix(ctx, witness, coeffs):
    rng = random.Random(18200 + 5 * len(witness) + len(coeffs))
    n_constraints, n_wires = 300, 53
    cons = _random_constraints(rng, n_constraints, n_wires, coeffs)
    wits = [_witness(witness, n_wires, rng)]
    got, bad = _run_rows(ctx, R1cs.build(n_wires, 1, 1, 1, cons), wits, n_wires + 1, check=False)
    assert bad is None and np.array_equal(got, _tables(cons, wits, 9))


# ---- b. row lengths ---------------------------------------------------------------------------------------------------------------------
def test_row_lengths_around_the_long_row_cut_and_the_wave_loop(ctx):
    """One R1CS whose tables both kernels write.  A: a 4097-term row of products first, then 0, 1, LONG_ROW - 1 .. LONG_ROW + 1, 63,
    64, 65 terms.  B: long rows in the middle and as the LAST real row (row n_constraints - 1 = 20, padding behind it), under the
    three coefficient kinds: r - 2 (products of all-max operands: the carries into the accumulator's top limbs), r - 1 and 1 (the
    addition path).  C: no long row at all.  Row 10 is empty in A, B and C."""
    n_wires = 4099
    lens_a = [4097, 0, 1, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 63, 64, 65, 2, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    lens_b = [1, 1, 65, 1, 4097, 1, LONG_ROW + 1, 1, 1, 64, 0, 1, 1, 4097, 1, 1, 1, 1, 1, 1, 4097]
    lens_c = [LONG_ROW, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, LONG_ROW - 1, 1, 1, 1, 1, 1, 1, 1, 2]
    kinds = [P - 2, P - 1, 1]

    def lc(length, row):
        c = kinds[row % 3]
        return [(c if length > 8 else (c, 1, P - 1, 12345)[t % 4], (row * 13 + 7 * t) % n_wires) for t in range(length)]
    cons = [(lc(a, i), lc(b, i + 1), lc(c, i + 2)) for i, (a, b, c) in enumerate(zip(lens_a, lens_b, lens_c))]
    assert len(cons) == 21 and not any(cons[10])
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    inf = r1cs.csr_info()
    assert inf["n"] == 5 and inf["n_long_rows"] == [5, 6, 0]
    assert r1cs.csr(0)[2].tolist() == [0, 5, 6, 7, 8] and r1cs.csr(1)[2].tolist() == [2, 4, 6, 9, 13, 20]
    rng = random.Random(18300)
    wits = [[P - 1] * n_wires, _witness("random", n_wires, rng)]
    got, bad = _run_rows(ctx, r1cs, wits, n_wires + 3)
    want = _tables(cons, wits, 5)
    assert np.array_equal(got, want)
    assert from_limbs(got[0, 0, 0:1])[0] == 4097 * (P - 2) * (P - 1) % P      # all-max operands, 4097 products
    assert bad.tolist() == _want_bad(cons, wits, 5)


@pytest.mark.parametrize("n_constraints", [4, 32, 256])
def test_a_long_row_as_the_last_row_of_a_full_table(ctx, n_constraints):
    """n_constraints = 2^n: no padding behind row 2^n - 1, which is long in A (products) and in C (the addition path) and short in B;
    A's row 0 is long too, so the list has a first and a last entry (256: the last thread of the only block of the short kernel)."""
    n_wires, last = 211, n_constraints - 1
    n = table_log2(n_constraints)
    assert 1 << n == n_constraints
    rng = random.Random(18350 + n_constraints)
    cons = _random_constraints(rng, n_constraints, n_wires, "random")
    cons[0] = ([(rng.randrange(2, P), rng.randrange(n_wires)) for _ in range(LONG_ROW + 1)], cons[0][1], cons[0][2])
    cons[last] = ([(P - 2, (5 * t) % n_wires) for t in range(130)], [(3, 1)], [((1, P - 1)[t % 2], (7 * t + 1) % n_wires) for t in range(65)])
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    assert r1cs.csr_info()["n"] == n
    assert r1cs.csr(0)[2].tolist() == [0, last] and r1cs.csr(1)[2].tolist() == [] and r1cs.csr(2)[2].tolist() == [last]
    wits = [[P - 1] * n_wires, _witness("random", n_wires, rng), _witness("bits", n_wires, rng)]
    got, bad = _run_rows(ctx, r1cs, wits, n_wires + 2)
    assert got.shape[2] == n_constraints and np.array_equal(got, _tables(cons, wits, n))
    assert from_limbs(got[0, 0, last:])[0] == 130 * (P - 2) * (P - 1) % P
    assert bad.tolist() == _want_bad(cons, wits, n)


# ---- c. first_bad -----------------------------------------------------------------------------------------------------------------------
def test_first_bad(ctx):
    """mimc7_demo_r1cs(91): 364 constraints in two blocks of 256 rows, 148 padding rows behind them."""
    nr = 91
    n_wires, cons = synth.mimc7_demo_constraints(nr)
    r1cs = synth.mimc7_demo_r1cs(nr)
    assert len(cons) == 364 and table_log2(364) == 9
    good = [synth.mimc7_demo_witness(2 + b, 3, nrounds=nr) for b in range(3)]

    def broken(w, *wires):
        w = list(w)
        for k in wires:
            w[k] = (w[k] + 1) % P
        return w
    one = broken(good[0], 150)
    two_blocks = broken(good[1], 300, 40)              # wire 40: a row of block 0; wire 300: a row of block 1 (wires 4 + 4 * round ..)
    last = broken(good[2], 1)                          # the output: the last real row alone
    wants = _want_bad(cons, [one, two_blocks, last], 9)
    assert all(x != NONE for x in wants) and wants[1] < 256 and wants[2] == 363
    assert first_bad(cons, broken(good[1], 300), 9) >= 256
    for wits, want in (([good[0]], [NONE]), ([one], wants[:1]), ([two_blocks], wants[1:2]), ([last], wants[2:]),
                       ([good[0], one, good[2]], [NONE, wants[0], NONE]), ([one, two_blocks, last], wants)):
        got, bad = _run_rows(ctx, r1cs, wits, n_wires + 7)
        assert bad.tolist() == want
        assert np.array_equal(got, _tables(cons, wits, 9))


# ---- d. the zero-check ------------------------------------------------------------------------------------------------------------------
def _systems():
    five = [([(1, 1)], [(1, 2)], [(1, 3)]), ([(1, 3), (5, 0)], [(P - 1, 1)], [(1, 4)]), ([(2, 4)], [(1, 4), (1, 1)], [(1, 5)]),
            ([(1, 5)], [(1, 0)], [(1, 5)]), ([(1, 0)], [(7, 0)], [(7, 0)])]

    def five_witness(x, y):
        w3 = x * y % P
        w4 = (w3 + 5) * (P - x) % P
        return [1, x, y, w3, w4, 2 * w4 * (w4 + x) % P]
    return {"five": (6, five, five_witness), "mimc91": synth.mimc7_demo_constraints(91) + (lambda x, y: synth.mimc7_demo_witness(x, y, nrounds=91),),
            "mimc4096": synth.mimc7_demo_constraints(4096) + (lambda x, y: synth.mimc7_demo_witness(x, y, nrounds=4096),)}


@pytest.fixture(scope="module")
def systems():
    return _systems()


def _claim(C, b):
    g = from_limbs(C[b, 0])
    return (sum(g) + g[-1]) % P                                   # g_1(0) + g_1(1); the unused leading slots are zero


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["five", "mimc91", "mimc4096"])
def test_zerocheck_is_the_zerocheck_on_the_models_tables(ctx, systems, name, batch):
    """Sumcheck 1 of a batch of three has a broken witness: its claim is the model's non-zero sum, the others' are zero."""
    n_wires, cons, witness = systems[name]
    n = table_log2(len(cons))
    assert n == {"five": 3, "mimc91": 9, "mimc4096": 14}[name]
    rng = random.Random(18400 + n + batch)
    wits = [witness(2 + b, 3 + b) for b in range(batch)]
    if batch == 3:
        wits[1][n_wires - 1] = (wits[1][n_wires - 1] + 1) % P
    zs = [[rng.randrange(P) for _ in range(n)] for _ in range(batch)]
    Z = to_limbs([x for z in zs for x in z]).reshape(batch, n, 4)
    T = _tables(cons, wits, n)
    stride = n_wires + 2
    W = np.zeros((batch * stride, 4), dtype=np.uint64)
    for b, w in enumerate(wits):
        W[b * stride:b * stride + n_wires] = to_limbs(w)
    S = np.zeros((batch, 4, 1 << n, 4), dtype=np.uint64)
    S[:, 1:] = T
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    d_w, d_t, d_s = ctx.alloc(W.nbytes), ctx.alloc(T.nbytes), ctx.alloc(S.nbytes)
    try:
        ctx.upload(d_w, W)
        ctx.upload(d_t, T)
        ctx.upload(d_s, S)
        with ctx.r1cs_rows(r1cs) as handle:
            got = ctx.r1cs_zerocheck_batch_device(handle, d_w, batch, Z, stride=stride)
        want = ctx.sumcheck_zerocheck_batch_device(d_t, n, 3, TERMS, batch, Z)
        for what, g, w in zip(("coeffs", "len", "r", "evals", "eq"), got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), what
        C, L, R, E, Q, bad = got
        assert bad.tolist() == _want_bad(cons, wits, n)
        claims = [zerocheck_claim_np(limbs_to_object(T[b]), TERMS, zs[b]) for b in range(batch)]
        for b in range(batch):
            broken = batch == 3 and b == 1
            assert (bad[b] != NONE) == broken and (claims[b] != 0) == broken
            assert _claim(C, b) == claims[b]
            proof = [from_limbs(C[b, j])[4 - int(L[b, j]):] for j in range(n)]
            assert verify_sumcheck_zerocheck(proof, from_limbs(R[b]), from_limbs(E[b]), TERMS, zs[b], claims[b])
            assert verify_sumcheck_zerocheck(proof, from_limbs(R[b]), from_limbs(E[b]), TERMS, zs[b], 0) == (not broken)
        # the transcripts through the SOP verifier on the tables plus the device-built eq table
        ctx.eq_table_device(Z, n, batch, d_s, stride=4 << n)
        accept, rnd, check, out_claims, out_evals = ctx.verify_sumcheck_sop_batch_device(d_s, n, 4, lift_terms(TERMS), batch, C, L, R, to_limbs(claims))
        assert accept.all() and (check == N.GKR_VERIFY_OK).all()
        assert np.array_equal(out_evals[:, 1:], E) and np.array_equal(out_evals[:, 0], Q)
    finally:
        ctx.free(d_w)
        ctx.free(d_t)
        ctx.free(d_s)
    if batch == 1:                                                # the host entry point
        proof, r, evals, eq_r, first = ctx.prove_r1cs_zerocheck(r1cs, wits[0], zs[0])
        assert proof == [from_limbs(C[0, j])[4 - int(L[0, j]):] for j in range(n)] and r == from_limbs(R[0])
        assert evals == from_limbs(E[0]) and eq_r == from_limbs(Q)[0] and first is None
        assert verify_sumcheck_zerocheck(proof, r, evals, TERMS, zs[0], 0)


def test_host_entry_point_reports_a_broken_witness_and_refuses_what_is_not_canonical(ctx, systems):
    n_wires, cons, witness = systems["mimc91"]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    rng = random.Random(18500)
    z = [rng.randrange(P) for _ in range(9)]
    w = witness(5, 6) + [P - 1, 17]                               # n_witness > n_wires: the tail is not read
    w[200] = (w[200] + 1) % P
    proof, r, evals, eq_r, first = ctx.prove_r1cs_zerocheck(r1cs, w, z)
    assert first == first_bad(cons, w, 9) and first is not None
    claim = zerocheck_claim_np(np.array(rows(cons, w, 9), dtype=object), TERMS, z)
    assert claim != 0 and (sum(proof[0]) + proof[0][-1]) % P == claim
    assert verify_sumcheck_zerocheck(proof, r, evals, TERMS, z, claim) and not verify_sumcheck_zerocheck(proof, r, evals, TERMS, z, 0)
    limbs = to_limbs(w)
    limbs[100] = np.array([P & (2**64 - 1), (P >> 64) & (2**64 - 1), (P >> 128) & (2**64 - 1), P >> 192], dtype=np.uint64)   # the entry r
    with pytest.raises(GkrError) as e:
        ctx.prove_r1cs_zerocheck(r1cs, limbs, z)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL
    zl = to_limbs(z).reshape(1, 9, 4)
    zl[0, 4] = limbs[100]
    with pytest.raises(GkrError) as e:
        ctx.prove_r1cs_zerocheck(r1cs, w, zl)
    assert e.value.status == N.GKR_ERR_NON_CANONICAL
    with pytest.raises(GkrError) as e:
        ctx.prove_r1cs_zerocheck(r1cs, w[:n_wires - 1], z)
    assert e.value.status == N.GKR_ERR_INVALID


# ---- e. offsets -------------------------------------------------------------------------------------------------------------------------
def test_a_witness_past_four_gib(ctx, systems):
    """Batch 2 with a stride of 2^27 + 5 elements: witness 1 starts 160 bytes past 4 GiB.  Only the two witnesses' own entries are
    uploaded; sumcheck 1's tables equal the same witness run alone."""
    n_wires, cons, witness = systems["mimc91"]
    stride = (1 << 27) + 5
    assert stride * 32 > 1 << 32
    wits = [witness(2, 3), witness(11, 3)]
    wits[1][77] = (wits[1][77] + 1) % P
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    try:
        d_w = ctx.alloc((stride + n_wires) * 32)
    except GkrError as e:
        pytest.skip("no 4 GiB device allocation here: %s" % e)
    d_out = ctx.alloc(2 * 3 * 512 * 32)
    try:
        second = ctypes.c_void_p(d_w.value + stride * 32)
        ctx.upload(d_w, to_limbs(wits[0]))
        ctx.upload(second, to_limbs(wits[1]))
        with ctx.r1cs_rows(r1cs) as handle:
            bad = ctx.r1cs_rows_device(handle, d_w, 2, d_out, stride=stride)
            both = ctx.download(d_out, (2, 3, 512, 4))
            bad1 = ctx.r1cs_rows_device(handle, second, 1, d_out)
            alone = ctx.download(d_out, (3, 512, 4))
    finally:
        ctx.free(d_w)
        ctx.free(d_out)
    assert np.array_equal(both[1], alone) and not np.array_equal(both[0], alone)
    assert np.array_equal(both, _tables(cons, wits, 9))
    assert bad.tolist() == _want_bad(cons, wits, 9) and bad1.tolist() == bad.tolist()[1:] and bad[0] == NONE != bad[1]


# ---- f. one context ---------------------------------------------------------------------------------------------------------------------
def test_one_context_two_handles_and_a_foreign_handle(ctx, systems):
    """An R1CS call, a zero-check on other tables, the R1CS call again: equal.  Two handles of different R1CS alive at once.  A
    handle on another context, and the other argument checks that need a handle: GKR_ERR_INVALID."""
    nw_a, cons_a, wit_a = systems["mimc91"]
    nw_b, cons_b, wit_b = systems["five"]
    rng = random.Random(18600)
    Wa, Wb = to_limbs(wit_a(4, 1)), to_limbs(wit_b(9, 8))
    za, zb = [[rng.randrange(P) for _ in range(9)]], [[rng.randrange(P) for _ in range(3)]]
    other = np.random.default_rng(18601).integers(0, 1 << 60, size=(2 * 3 << 11, 4), dtype=np.uint64)
    z_other = [[rng.randrange(P) for _ in range(11)] for _ in range(2)]
    d_a, d_b, d_o = ctx.alloc(Wa.nbytes), ctx.alloc(Wb.nbytes), ctx.alloc(other.nbytes)
    try:
        ctx.upload(d_a, Wa)
        ctx.upload(d_b, Wb)
        ctx.upload(d_o, other)
        with ctx.r1cs_rows(R1cs.build(nw_a, 1, 1, 1, cons_a)) as ha, ctx.r1cs_rows(R1cs.build(nw_b, 1, 1, 1, cons_b)) as hb:
            first = ctx.r1cs_zerocheck_batch_device(ha, d_a, 1, za)
            small = ctx.r1cs_zerocheck_batch_device(hb, d_b, 1, zb)
            between = ctx.sumcheck_zerocheck_batch_device(d_o, 11, 3, TERMS, 2, z_other)
            third = ctx.r1cs_zerocheck_batch_device(ha, d_a, 1, za)
            small2 = ctx.r1cs_zerocheck_batch_device(hb, d_b, 1, zb)
            assert all(np.array_equal(x, y) for x, y in zip(first, third)) and all(np.array_equal(x, y) for x, y in zip(small, small2))
            assert _claim(first[0], 0) == 0 == _claim(small[0], 0) and first[5][0] == NONE == small[5][0]
            with Context(0) as c2:
                d2 = c2.alloc(Wa.nbytes)
                try:
                    c2.upload(d2, Wa)
                    with c2.r1cs_rows(R1cs.build(nw_a, 1, 1, 1, cons_a)) as h2:
                        alone = c2.sumcheck_zerocheck_batch_device(d_o, 11, 3, TERMS, 2, z_other)
                        assert all(np.array_equal(x, y) for x, y in zip(between, alone))
                        assert all(np.array_equal(x, y) for x, y in zip(first, c2.r1cs_zerocheck_batch_device(h2, d2, 1, za)))
                        for call in (lambda: ctx.r1cs_zerocheck_batch_device(h2, d_a, 1, za), lambda: ctx.r1cs_rows_device(h2, d_a, 1, d_o),
                                     lambda: c2.r1cs_rows_device(ha, d2, 1, d_o)):
                            with pytest.raises(GkrError) as e:
                                call()
                            assert e.value.status == N.GKR_ERR_INVALID
                finally:
                    c2.free(d2)
            # batch outside 1 .. 65535, a stride below n_wires, batch * 3 * 2^n above 2^30 (2^9: 699051 > 65535, so the 2^14 system)
            for batch, stride in ((0, None), (-1, None), (65536, None), (1, nw_a - 1), (1, 0)):
                for call in (lambda: ctx.r1cs_rows_device(ha, d_a, batch, d_o, stride=stride),
                             lambda: ctx.r1cs_zerocheck_batch_device(ha, d_a, batch, np.zeros((max(batch, 0), 9, 4), dtype=np.uint64), stride=stride)):
                    with pytest.raises(GkrError) as e:
                        call()
                    assert e.value.status == N.GKR_ERR_INVALID, (batch, stride)
            nw_c, cons_c, _ = systems["mimc4096"]
            with ctx.r1cs_rows(R1cs.build(nw_c, 1, 1, 1, cons_c)) as hc:
                assert 21846 * 3 << 14 > 1 << 30 >= 21845 * 3 << 14
                with pytest.raises(GkrError) as e:
                    ctx.r1cs_rows_device(hc, d_a, 21846, d_o)
                assert e.value.status == N.GKR_ERR_INVALID
    finally:
        ctx.free(d_a)
        ctx.free(d_b)
        ctx.free(d_o)

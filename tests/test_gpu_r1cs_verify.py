"""gkr_r1cs_matrix_evals_device / gkr_r1cs_verify* (csrc/kernels_r1cs.hip, csrc/capi_r1cs_verify.hip) through the C ABI.

  a. the matrices' extensions at a point, exactly verifier.r1cs_matrix_evals: sizes around the 256-thread block, padding rows
     and wires, several blocks, the sum kernel's second trip, coefficient mixes, random and boolean points, an empty matrix;
  b. row lengths around the long-row cut and the wave's loop with all-max operands, another number of long rows in every matrix;
  c. on every system of a and b the call equals, byte for byte, gkr_eq_table_device -> gkr_r1cs_rows_device ->
     gkr_mle_eval_batch_device on the same context;
  d. the verifier: proofs of the two device provers accepted with and without the witness; the tamper sweep of
     tests/test_r1cs_verify_host.py as one batch per proof against verifier.verify_r1cs; a changed matrix, a changed witness, a
     broken witness, non-canonical elements beside honest neighbours; both hash paths and several chunks; the host entry point;
     the refusals that need a handle; rows, cols and verify on one context."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError, synth
from gkr_amd import _native as N
from gkr_amd.convert import R1cs
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import r1cs_matrix_evals, verify_r1cs
from r1cs_cols_model import n_y_of
from r1cs_rows_model import LONG_ROW, table_log2

pytestmark = pytest.mark.gpu

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


def _system(rng, n_constraints, n_wires):
    """A random system and THE witness that satisfies it (tests/test_r1cs_verify_host.py's): A and B random combinations of 1 .. 3
    terms, C = c w_k + (a b - c w_k) w_0 with w_0 = 1."""
    w = [1] + [rng.randrange(1, P) for _ in range(n_wires - 1)]
    cons = []
    for _ in range(n_constraints):
        A = [(rng.randrange(1, P), rng.randrange(n_wires)) for _ in range(rng.randrange(1, 4))]
        B = [((1, P - 1, rng.randrange(1, P))[rng.randrange(3)], rng.randrange(n_wires)) for _ in range(rng.randrange(1, 4))]
        a, b = (sum(c * w[k] for c, k in lc) % P for lc in (A, B))
        k, c = rng.randrange(n_wires), rng.randrange(1, P)
        cons.append((A, B, [(c, k), ((a * b - c * w[k]) % P, 0)]))
    return cons, w


def _bits(index, n):
    return [(index >> (n - 1 - j)) & 1 for j in range(n)]


def _composition(ctx, rows, inf, n_y, xs, ys):
    """The three public calls the fused pass replaces: eq(y_b, .) as the "witness" of the rows call, its three tables at x_b."""
    n, batch = inf["n"], len(xs)
    d_ey, d_t = ctx.alloc((batch << n_y) * 32), ctx.alloc((batch * 3 << n) * 32)
    try:
        ctx.eq_table_device(ys, n_y, batch, d_ey)
        ctx.r1cs_rows_device(rows, d_ey, batch, d_t, stride=1 << n_y, check=False)
        pts = np.repeat(to_limbs([v for x in xs for v in x]).reshape(batch, 1, n, 4), 3, axis=1).reshape(batch * 3, n, 4)
        return ctx.mle_eval_batch_device(d_t, n, batch * 3, pts).reshape(batch, 3, 4)
    finally:
        ctx.free(d_ey)
        ctx.free(d_t)


def _check_system(ctx, cons, n_wires, xs, ys):
    """The call on one system and a batch of points: the integer model, and the composition byte for byte.  -> the values."""
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    n_y = n_y_of(n_wires)
    with ctx.r1cs_rows(r1cs) as rows:
        inf = rows.info()
        assert inf["n"] == table_log2(len(cons)) == len(xs[0]) and n_y == len(ys[0])
        got = ctx.r1cs_matrix_evals_device(rows, xs, ys)
        want = np.stack([to_limbs(r1cs_matrix_evals(cons, x, y)) for x, y in zip(xs, ys)])
        assert np.array_equal(got, want)
        comp = _composition(ctx, rows, inf, n_y, xs, ys)
        assert got.shape == comp.shape and got.dtype == comp.dtype and got.tobytes() == comp.tobytes()
        again = ctx.r1cs_matrix_evals_device(rows, xs, ys)                  # no slot is left over from the run before
        assert np.array_equal(again, got)
    return [from_limbs(g) for g in got]


def _entry(cons, m, row, wire):
    """The matrix entry the extension takes at a boolean point: the sum of the coefficients at (row, wire); zero outside."""
    return sum(c for c, w in cons[row][m] if w == wire) % P if row < len(cons) else 0


# ---- a. the matrices' extensions against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n_constraints", [1, 2, 255, 256, 257, 1000, 16384 + 1])
def test_matrix_evals_match_the_model_and_the_composition(ctx, n_constraints, batch):
    """Point 0 of three is random; 1 a boolean one inside the matrix; 2 the boolean one at the last row and the last wire of the
    tables: padding (the value must be zero) unless both tables are full.  A lone point is boolean for 5 wires, random otherwise."""
    n = table_log2(n_constraints)
    for n_wires in (1, 5, 257):
        rng = random.Random(20200 + 7 * n_constraints + 3 * n_wires + batch)
        n_y = n_y_of(n_wires)
        cons = _random_constraints(rng, n_constraints, n_wires, COEFF_MIX[(n_constraints + n_wires + batch) % 4])
        row_in, wire_in, row_last, wire_last = rng.randrange(n_constraints), rng.randrange(n_wires), (1 << n) - 1, (1 << n_y) - 1
        random_point = ([rng.randrange(P) for _ in range(n)], [rng.randrange(P) for _ in range(n_y)])
        inside, last = (_bits(row_in, n), _bits(wire_in, n_y)), (_bits(row_last, n), _bits(wire_last, n_y))
        points = [random_point, inside, last] if batch == 3 else [inside if n_wires == 5 else random_point]
        got = _check_system(ctx, cons, n_wires, [p[0] for p in points], [p[1] for p in points])
        if batch == 3:
            assert got[1] == [_entry(cons, m, row_in, wire_in) for m in range(3)]
            assert got[2] == [_entry(cons, m, row_last, wire_last) for m in range(3)]
            if row_last >= n_constraints or wire_last >= n_wires:
                assert got[2] == [0, 0, 0], "a padding row or a padding wire"
        elif n_wires == 5:
            assert got[0] == [_entry(cons, m, row_in, wire_in) for m in range(3)]


def test_a_matrix_without_terms_and_the_sum_kernels_second_trip(ctx):
    """65 537 constraints: 257 blocks of rows, one more slot than the sum kernel's 256 threads take in one trip; C has no term at
    all and evaluates to exactly zero; the last row (the only one of block 256) is not lost: a boolean point picks it."""
    rng = random.Random(20300)
    n_constraints, n_wires = 65536 + 1, 5
    cons = [([(_coeff("minus_one_and_two", rng), rng.randrange(n_wires)) for _ in range(rng.randrange(5))],
             [(_coeff("random", rng), rng.randrange(n_wires))] if i % 3 else [], []) for i in range(n_constraints - 1)]
    cons.append(([(7, 4), (P - 1, 4)], [(P - 2, 0)], []))
    xs = [[rng.randrange(P) for _ in range(17)], _bits(65536, 17)]
    ys = [[rng.randrange(P) for _ in range(3)], _bits(4, 3)]
    got = _check_system(ctx, cons, n_wires, xs, ys)
    assert got[0][2] == 0 and got[1] == [6, 0, 0] and got[0][0] != 0 and got[0][1] != 0


# ---- b. row lengths ------------------------------------------------------------------------------------------------------------------------
def test_row_lengths_around_the_cut_and_the_wave_loop_with_all_max_operands(ctx):
    """One system: A has rows of 0, 1, LONG_ROW, LONG_ROW + 1, 64, 65 and 4097 terms and a long row as its LAST constraint (five
    long rows), B two long rows among short ones, C none: the long kernel's grid is five blocks wide, B's three and C's five
    surplus blocks store zero.  Coefficients r - 1 (the addition path) and r - 2 (the product path); points whose eq entries are
    3^a (-2)^b -- r minus something small among them -- beside a random one and a boolean one at the last row."""
    lens = [[0, 1, LONG_ROW, LONG_ROW + 1, 64, 65, 4097, 2, 4097], [LONG_ROW + 1, 0, 1, LONG_ROW, 1, 2, 65, 3, 1], [1, 2, 0, 3, LONG_ROW, 1, 2, 4, 0]]
    n_wires = 6
    cons = [tuple([((P - 1, P - 2, P - 1)[(m + i) % 3], (t + i) % n_wires) for t in range(lens[m][i])] for m in range(3)) for i in range(9)]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    assert r1cs.csr_info()["n_long_rows"] == [5, 2, 0] and r1cs.csr_info()["n"] == 4
    rng = random.Random(20400)
    xs = [[P - 2] * 4, [rng.randrange(P) for _ in range(4)], _bits(8, 4)]
    ys = [[P - 2] * 3, [rng.randrange(P) for _ in range(3)], _bits(2, 3)]
    got = _check_system(ctx, cons, n_wires, xs, ys)
    assert got[2] == [_entry(cons, m, 8, 2) for m in range(3)] and got[2][0] != 0 and got[2][2] == 0
    assert all(v != 0 for v in got[0])


# ---- d. the verifier -----------------------------------------------------------------------------------------------------------------------
def _upload(ctx, wits, n_wires, stride):
    W = np.full((len(wits) * stride, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    for b, w in enumerate(wits):
        W[b * stride:b * stride + n_wires] = to_limbs(w[:n_wires])
    d_w = ctx.alloc(W.nbytes)
    ctx.upload(d_w, W)
    return d_w


def _prove(ctx, r1cs, rows, d_w, batch, zs, rhos, stride):
    """The two device provers, the inner one at the zero-check's challenges: -> (zerocheck (C, L, R, E), inner (C, L, R, E))."""
    CX, LX, RX, EX, _, _ = ctx.r1cs_zerocheck_batch_device(rows, d_w, batch, zs, stride=stride)
    with ctx.r1cs_cols(r1cs) as cols:
        inner = ctx.r1cs_inner_batch_device(cols, d_w, batch, RX, rhos, stride=stride)
    return (CX, LX, RX, EX), inner


def _rounds(C, L, width):
    """A transcript's rows as the integer model takes them: the used slots; a length beyond the width takes zeros in front."""
    out = []
    for j in range(C.shape[0]):
        ln, slots = int(L[j]), from_limbs(C[j])
        out.append(slots[width - ln:] if ln <= width else [0] * (ln - width) + slots)
    return out


def _model_verdict(cons, z, rho, zc, inner, b, witness=None):
    (CX, LX, RX, EX), (CY, LY, RY, EY) = zc, inner
    return verify_r1cs(cons, z, rho, _rounds(CX[b], LX[b], 4), from_limbs(RX[b]), from_limbs(EX[b]), _rounds(CY[b], LY[b], 3), from_limbs(RY[b]),
                       from_limbs(EY[b]), witness)


def _plus_one(limbs):
    return to_limbs([(from_limbs(limbs)[0] + 1) % P])[0]


def _sweep(zc, inner):
    """The sweep of tests/test_r1cs_verify_host.py on the arrays of ONE proof: -> (zerocheck, inner) of a batch whose entry 0 is
    the honest proof and every other entry differs from it in one slot, one challenge, one evaluation (x + 1 mod r) or one
    length (+- 1), honest copies in between."""
    entries = []
    arrays = [a[0] for a in zc] + [a[0] for a in inner]                     # CX LX RX EX CY LY RY EY of the one proof

    def changed(at, index, value):
        e = [a.copy() for a in arrays]
        e[at][index] = value
        entries.append(e)
    entries.append([a.copy() for a in arrays])
    for base, width in ((0, 4), (4, 3)):
        C, L, R, E = arrays[base:base + 4]
        for j in range(C.shape[0]):
            for k in range(width - int(L[j]), width):
                changed(base, (j, k), _plus_one(C[j, k]))
            changed(base + 2, j, _plus_one(R[j]))
            changed(base + 1, j, int(L[j]) + 1)
            changed(base + 1, j, int(L[j]) - 1)
            if j % 3 == 1:
                entries.append([a.copy() for a in arrays])
        for m in range(E.shape[0]):
            changed(base + 3, m, _plus_one(E[m]))
    stacked = [np.ascontiguousarray(np.stack([e[i] for e in entries])) for i in range(8)]
    return tuple(stacked[:4]), tuple(stacked[4:])


def _verdicts(got):
    accept, stage, rnd, check = got
    assert all((int(a) == 1) == (int(c) == 0) for a, c in zip(accept, check))
    return [(int(s), int(r), int(c)) for s, r, c in zip(stage, rnd, check)]


def _verifier_systems():
    rng = random.Random(20500)
    cons, w = _system(rng, 7, 4)
    small = synth.mimc7_demo_constraints(2)
    chain = synth.mimc7_demo_constraints(91)
    return {"random-n3-ny2": (4, cons, lambda b: list(w)),
            "mimc2-n3-ny4": small + (lambda b: synth.mimc7_demo_witness(2 + b, 3 + b, nrounds=2)[:small[0]],),
            "mimc91-n9-ny9": chain + (lambda b: synth.mimc7_demo_witness(2 + b, 3 + b, nrounds=91)[:chain[0]],)}


@pytest.fixture(scope="module")
def vsystems():
    return _verifier_systems()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["random-n3-ny2", "mimc2-n3-ny4", "mimc91-n9-ny9"])
def test_honest_proofs_are_accepted_and_single_changes_rejected_as_the_model_says(ctx, vsystems, name, batch):
    """The device provers' proofs of `batch` satisfied witnesses: accepted with and without the witness.  Then the sweep on proof
    batch - 1 (a boolean z at batch 1, a random one at batch 3), one batch of its own; the verdicts with the witness, under both
    hash paths and in several chunks, equal the model's entry by entry.  (The random system has ONE witness; its batch repeats it.)"""
    n_wires, cons, witness = vsystems[name]
    n, n_y = table_log2(len(cons)), n_y_of(n_wires)
    assert (n, n_y) == {"random-n3-ny2": (3, 2), "mimc2-n3-ny4": (3, 4), "mimc91-n9-ny9": (9, 9)}[name]
    rng = random.Random(20600 + n_y + batch)
    wits = [witness(b) for b in range(batch)]
    zs = [[rng.randrange(2) if (b % 2 == 1 or batch == 1) else rng.randrange(P) for _ in range(n)] for b in range(batch)]
    rhos = [[rng.randrange(1, P) for _ in range(3)] for _ in range(batch)]
    stride = n_wires + 3
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    d_w = _upload(ctx, wits, n_wires, stride)
    try:
        with ctx.r1cs_rows(r1cs) as rows:
            zc, inner = _prove(ctx, r1cs, rows, d_w, batch, zs, rhos, stride)
            for d in (d_w, None):
                assert _verdicts(ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner, d_witness=d, stride=stride)) == [(0, 0, 0)] * batch
            for b in range(batch):
                assert _model_verdict(cons, zs[b], rhos[b], zc, inner, b, wits[b][:n_wires]) == (0, 0, 0)
            # the sweep on the last proof: its witness once per entry of the sweep's batch
            b = batch - 1
            one = lambda arrs: tuple(a[b:b + 1] for a in arrs)
            szc, sinner = _sweep(one(zc), one(inner))
            count = szc[0].shape[0]
            d_rep = _upload(ctx, [wits[b]] * count, n_wires, n_wires)
            try:
                want = [_model_verdict(cons, zs[b], rhos[b], szc, sinner, e, wits[b][:n_wires]) for e in range(count)]
                assert want[0] == (0, 0, 0) and sum(v == (0, 0, 0) for v in want) == 1 + sum(1 for j in range(n) if j % 3 == 1) + sum(
                    1 for j in range(n_y) if j % 3 == 1), "only the honest copies are accepted"
                args = (rows, count, [zs[b]] * count, szc, [rhos[b]] * count, sinner)
                try:
                    for hash_min, mb in ((-1, 0), (1, 0), (1, 1), (-1, 1)):
                        ctx.set_option("verify_device_hash_min", hash_min)
                        ctx.set_option("verify_workspace_mb", mb)
                        assert _verdicts(ctx.verify_r1cs_batch_device(*args, d_witness=d_rep)) == want, (hash_min, mb)
                finally:
                    ctx.set_option("verify_device_hash_min", 0)
                    ctx.set_option("verify_workspace_mb", 0)
                assert _verdicts(ctx.verify_r1cs_batch_device(*args)) == want, "stages 1 and 2 do not look at the witness"
            finally:
                ctx.free(d_rep)
    finally:
        ctx.free(d_w)


def test_several_chunks_are_forced(ctx, vsystems):
    """verify_workspace_mb = 1 on the chain: a proof's share is above 32 KiB (two eq tables of 2^9 entries), so a batch of 40
    takes two chunks at least; the verdicts of a batch with rejected proofs spread over it do not move."""
    n_wires, cons, witness = vsystems["mimc91-n9-ny9"]
    rng = random.Random(20700)
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    w = witness(0)
    d_w = _upload(ctx, [w], n_wires, n_wires)
    try:
        with ctx.r1cs_rows(r1cs) as rows:
            z, rho = [[rng.randrange(P) for _ in range(9)]], [[rng.randrange(1, P) for _ in range(3)]]
            zc, inner = _prove(ctx, r1cs, rows, d_w, 1, z, rho, n_wires)
            count = 40
            assert count * 2 * (32 << 9) > 1 << 20
            rep = lambda arrs: tuple(np.ascontiguousarray(np.repeat(a, count, axis=0)) for a in arrs)
            zc, inner = rep(zc), rep(inner)
            for e in (0, 17, 31, 32, 39):
                inner[3][e, 0] = _plus_one(inner[3][e, 0])                  # e_T: stage 2, EVALUATION
            want = [(2, 9, N.GKR_VERIFY_EVALUATION) if e in (0, 17, 31, 32, 39) else (0, 0, 0) for e in range(count)]
            try:
                for mb in (0, 1):
                    ctx.set_option("verify_workspace_mb", mb)
                    assert _verdicts(ctx.verify_r1cs_batch_device(rows, count, z * count, zc, rho * count, inner)) == want, mb
            finally:
                ctx.set_option("verify_workspace_mb", 0)
    finally:
        ctx.free(d_w)


def test_further_rejections_and_the_host_entry(ctx, vsystems):
    """A changed matrix coefficient in the verifier's R1CS: stage 3.  A changed witness entry: stage 4, accepted without a witness.
    A broken witness's own proof: stage 1, round 0, ROUND_SUM.  A slot, a challenge and an evaluation >= r: NON_CANONICAL at the
    right round, the honest neighbours in the same batch accepted.  gkr_r1cs_verify on one proof."""
    n_wires, cons, witness = vsystems["mimc2-n3-ny4"]
    n, n_y = 3, 4
    rng = random.Random(20800)
    batch = 3
    wits = [witness(b) for b in range(batch)]
    wits[1][5] = (wits[1][5] + 1) % P                                      # breaks a constraint
    zs = [[rng.randrange(P) for _ in range(n)] for _ in range(batch)]
    rhos = [[rng.randrange(1, P) for _ in range(3)] for _ in range(batch)]
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    A, B, C = cons[2]
    other = list(cons)
    other[2] = (A, [((B[0][0] + 1) % P, B[0][1])] + list(B[1:]), C)
    d_w = _upload(ctx, wits, n_wires, n_wires)
    changed = [list(w) for w in wits]
    changed[2][n_wires - 1] = (changed[2][n_wires - 1] + 1) % P
    d_c = _upload(ctx, changed, n_wires, n_wires)
    try:
        with ctx.r1cs_rows(r1cs) as rows, ctx.r1cs_rows(R1cs.build(n_wires, 1, 1, 1, other)) as rows_other:
            zc, inner = _prove(ctx, r1cs, rows, d_w, batch, zs, rhos, n_wires)
            honest = [(0, 0, 0), (1, 0, N.GKR_VERIFY_ROUND_SUM), (0, 0, 0)]
            assert _verdicts(ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner, d_witness=d_w)) == honest
            assert [_model_verdict(cons, zs[b], rhos[b], zc, inner, b, wits[b]) for b in range(batch)] == honest
            got = _verdicts(ctx.verify_r1cs_batch_device(rows_other, batch, zs, zc, rhos, inner, d_witness=d_w))
            assert got == [(3, n_y, N.GKR_VERIFY_MATRIX), honest[1], (3, n_y, N.GKR_VERIFY_MATRIX)]
            assert got == [_model_verdict(other, zs[b], rhos[b], zc, inner, b, wits[b]) for b in range(batch)]
            got = _verdicts(ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner, d_witness=d_c))
            assert got == [honest[0], honest[1], (4, n_y, N.GKR_VERIFY_WITNESS)]
            assert got == [_model_verdict(cons, zs[b], rhos[b], zc, inner, b, changed[b]) for b in range(batch)]
            assert _verdicts(ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner)) == honest
            # elements >= r in proof 0 (and once in proof 2), proof 2 (proof 0) honest beside it
            for at, index, want in ((0, (1, 3), (1, 1, 2)), (2, (2,), (1, 2, 2)), (3, (1,), (1, n, 2)), (4, (0, 2), (2, 0, 2)), (6, (3,), (2, 3, 2)),
                                    (7, (0,), (2, n_y, 2)), (7, (1,), (2, n_y, 2))):
                for b in (0, 2):
                    arrays = [a.copy() for a in zc + inner]
                    arrays[at][(b,) + index] = R_LIMBS
                    got = _verdicts(ctx.verify_r1cs_batch_device(rows, batch, zs, tuple(arrays[:4]), rhos, tuple(arrays[4:]), d_witness=d_w))
                    assert got == [want if e == b else honest[e] for e in range(batch)], (at, index, b)
                    assert got[b] == _model_verdict(cons, zs[b], rhos[b], tuple(arrays[:4]), tuple(arrays[4:]), b, wits[b])
            # z and rho are the verifier's own: an entry >= r is an error of the call
            zl, rl = to_limbs([v for z in zs for v in z]).reshape(batch, n, 4), to_limbs([v for r in rhos for v in r]).reshape(batch, 3, 4)
            zl[2, 1] = R_LIMBS
            rl[1, 2] = R_LIMBS
            for call in (lambda: ctx.verify_r1cs_batch_device(rows, batch, zl, zc, rhos, inner), lambda: ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rl, inner)):
                with pytest.raises(GkrError) as e:
                    call()
                assert e.value.status == N.GKR_ERR_NON_CANONICAL
            xl = to_limbs([0] * n).reshape(1, n, 4)
            xl[0, 0] = R_LIMBS
            with pytest.raises(GkrError) as e:
                ctx.r1cs_matrix_evals_device(rows, xl, [[0] * n_y])
            assert e.value.status == N.GKR_ERR_NON_CANONICAL
            # a witness stride below n_wires; a handle of another context
            with pytest.raises(GkrError) as e:
                ctx.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner, d_witness=d_w, stride=n_wires - 1)
            assert e.value.status == N.GKR_ERR_INVALID
            with Context(0) as c2:
                for call in (lambda: c2.verify_r1cs_batch_device(rows, batch, zs, zc, rhos, inner), lambda: c2.r1cs_matrix_evals_device(rows, zs, [[0] * n_y] * batch)):
                    with pytest.raises(GkrError) as e:
                        call()
                    assert e.value.status == N.GKR_ERR_INVALID
        # the host entry point: prove_r1cs_zerocheck / prove_r1cs_inner's results as they are
        px = ctx.prove_r1cs_zerocheck(r1cs, wits[0], zs[0])
        py = ctx.prove_r1cs_inner(r1cs, wits[0], px[1], rhos[0])
        assert ctx.verify_r1cs(r1cs, zs[0], rhos[0], px[:3], py, witness=wits[0]) == (0, 0, 0)
        assert ctx.verify_r1cs(r1cs, zs[0], rhos[0], px[:3], py) == (0, 0, 0)
        assert ctx.verify_r1cs(r1cs, zs[0], rhos[0], px[:3], py, witness=changed[2]) == (4, n_y, N.GKR_VERIFY_WITNESS)
        assert ctx.verify_r1cs(r1cs, zs[0], rhos[0], px[:3], (py[0], py[1], [py[2][0], py[2][1] + 1])) == (2, n_y, N.GKR_VERIFY_EVALUATION)
        assert ctx.verify_r1cs(R1cs.build(n_wires, 1, 1, 1, other), zs[0], rhos[0], px[:3], py) == (3, n_y, N.GKR_VERIFY_MATRIX)
    finally:
        ctx.free(d_w)
        ctx.free(d_c)


def test_the_cap_and_one_context_for_rows_cols_and_verify(ctx, vsystems):
    """batch * (2^n + 2^n_y) above 2^30 values (n = 15, n_y = 6: 32 704 proofs fit, 32 705 do not) is refused before anything is
    read.  A rows call, a cols call, the matrix pass and the verifier interleaved on one context: equal results the second time."""
    tall = [([(1, i % 50)], [(1, 0)], [(1, (i + 1) % 50)]) for i in range(16384 + 1)]
    with ctx.r1cs_rows(R1cs.build(50, 1, 1, 1, tall)) as ht:
        assert ht.info()["n"] == 15 and n_y_of(50) == 6
        fits = (1 << 30) // ((1 << 15) + (1 << 6))
        assert fits == 32704 and (fits + 1) * ((1 << 15) + (1 << 6)) > 1 << 30
        batch = fits + 1
        with pytest.raises(GkrError) as e:
            ctx.r1cs_matrix_evals_device(ht, np.zeros((batch, 15, 4), dtype=np.uint64), np.zeros((batch, 6, 4), dtype=np.uint64))
        assert e.value.status == N.GKR_ERR_INVALID
        lib, word = N.lib(), (ctypes.c_uint64 * 8)()
        fake = ctypes.c_void_p(ctypes.addressof(word))                       # (never read: the cap is decided from the handle and the batch)
        assert lib.gkr_r1cs_verify_batch_device(ctx._h, ht._h, batch, *([fake] * 10), None, 0, fake, None, None, None) == N.GKR_ERR_INVALID
    n_wires, cons, witness = vsystems["mimc91-n9-ny9"]
    rng = random.Random(20900)
    r1cs = R1cs.build(n_wires, 1, 1, 1, cons)
    w = witness(1)
    d_w = _upload(ctx, [w], n_wires, n_wires)
    d_t = ctx.alloc((3 << 9) * 32)
    try:
        z, rho = [[rng.randrange(P) for _ in range(9)]], [[rng.randrange(1, P) for _ in range(3)]]
        with ctx.r1cs_rows(r1cs) as rows, ctx.r1cs_cols(r1cs) as cols:
            def once():
                zc = ctx.r1cs_zerocheck_batch_device(rows, d_w, 1, z)
                inner = ctx.r1cs_inner_batch_device(cols, d_w, 1, zc[2], rho)
                mats = ctx.r1cs_matrix_evals_device(rows, zc[2], inner[2])
                verdict = _verdicts(ctx.verify_r1cs_batch_device(rows, 1, z, zc[:4], rho, inner, d_witness=d_w))
                ctx.r1cs_rows_device(rows, d_w, 1, d_t)
                ctx.r1cs_cols_device(cols, zc[2], rho, 1, d_t)
                return list(zc) + list(inner) + [mats], verdict
            first, v1 = once()
            second, v2 = once()
            assert v1 == v2 == [(0, 0, 0)] and all(np.array_equal(a, b) for a, b in zip(first, second))
            e_t = from_limbs(first[9][0])[0]
            assert e_t == sum(r * v for r, v in zip(rho[0], from_limbs(first[10][0]))) % P
    finally:
        ctx.free(d_w)
        ctx.free(d_t)

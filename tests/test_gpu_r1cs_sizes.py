"""The R1CS argument's device calls -- gkr_r1cs_rows_device, gkr_r1cs_zerocheck_batch_device, gkr_r1cs_cols_device,
gkr_r1cs_inner_batch_device, gkr_r1cs_matrix_evals_device, gkr_r1cs_verify_batch_device (csrc/kernels_r1cs.hip, csrc/capi_r1cs.hip,
csrc/capi_r1cs_verify.hip) -- bit for bit against the C oracle at sizes where both sumchecks are multi-block: ogkr_r1cs_rows,
ogkr_r1cs_cols and ogkr_r1cs_matrix_evals for the tables (loops over the flat records; tests/test_oracle_r1cs_c.py holds them to the
Python models), ogkr_sumcheck_zerocheck on the oracle's rows with A B - C and ogkr_sumcheck_product at degree 2 on {oracle T, w
zero-padded} for the two sumchecks.  The systems are tests/r1cs_systems.py's, built from arrays; every expectation, first_bad and
the verifier's verdicts included, comes from the oracle and is asserted on the oracle before the device is asked.

The cases (n_x, n_y, batch), constraints x wires, and what each reaches:

  (16, 16, 1)   2^16 x 2^16        both sumchecks at the pinned (16, 1): 128 blocks of 256; no padding row and no padding wire, the
                                   last row long (4097 terms) and read by the last wire; 32 wire-0 segments per matrix, 96
                                   partials in the wire-0 combine column at the default segment length; the cols table also with
                                   segment = 0 and 64 (1024 segments a matrix); the Python verifier on the same proofs
  (16, 16, 20)  the same system    both at the pinned (16, 20): 103 blocks, chunk 512; witness kinds random / all r - 1 / bits /
                                   small in turn, points random / boolean / one z_j = 1/2 in turn; member 6 breaks the last row
                                   alone (only the last of 256 row blocks has something to report), member 12 breaks rows in
                                   blocks 10 and 200 (the lower one must win the atomicMin), member 18 rows in 200 blocks and more
  (18, 16, 5)   2^17+257 x 2^15+257   the zero-check at the pinned (18, 5): 410 blocks, chunk 512; n_x > n_y; nearly 511 blocks of
                                   padding rows and 127 blocks' worth of padding wires; an output wire is read by four rows; 65
                                   segments per matrix, the last of 257 records; member 2 breaks the last real row, in block 513
  (16, 20, 1)   2^15+257 x 2^19+257   n_y > n_x: the inner sumcheck at the pinned (20, 1), 2048 blocks, over a table whose columns
                                   are mostly single records and, past n_constraints output wires, empty; nearly 127 blocks of
                                   padding rows; the zero-check at (16, 1) with z_j = 1/2 at index 8
  (20, 18, 1)   2^20 x 2^18        the zero-check at the pinned (20, 1): 2048 blocks; 512 wire-0 segments per matrix, 1536
                                   partials in the combine column; the matrices' extensions and first_bad over 4096 blocks of
                                   rows; several hundred long rows in A, fewer in B, none in C; a boolean z

Batches (20, 4) and (23, 1) are left out on purpose: tests/test_gpu_zerocheck_sizes.py and tests/test_gpu_product_sizes.py hold the
sumcheck kernels there, and the R1CS drivers add only the construction of the tables, which takes the batch as a grid dimension and
nothing else.

Per case: a. rows and first_bad; b. the zero-check; c. the cols table; d. the inner sumcheck; e. the matrices' extensions; f. the
verifier."""

import random

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from gkr_amd.verifier import R1CS_ZEROCHECK_TERMS, verify_r1cs
from oracle import cdense
from oracle.field import P
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from r1cs_systems import LONG, NO_BAD, SEG, bad_rows, build_r1cs, constraints_of, generate, limbs, witness
from resident_tables import Resident, assert_same

pytestmark = pytest.mark.gpu

CASES = [(16, 16, 1), (16, 16, 20), (18, 16, 5), (16, 20, 1), (20, 18, 1)]
SIZES = {(16, 16): (1 << 16, 1 << 16), (18, 16): ((1 << 17) + 257, (1 << 15) + 257), (16, 20): ((1 << 15) + 257, (1 << 19) + 257),
         (20, 18): (1 << 20, 1 << 18)}
PINNED = {(16, 16, 1): ((16, 1), (16, 1)), (16, 16, 20): ((16, 20), (16, 20)), (18, 16, 5): ((18, 5), None), (16, 20, 1): ((16, 1), (20, 1)),
          (20, 18, 1): ((20, 1), None)}                              # the PRODUCT_GEOMETRY rows of (zero-check, inner sumcheck)
WITNESS_KINDS = ["random", "all_max", "bits", "small"]
POINTS = ["random", "boolean", "half"]
FIRST_POINT = {(16, 16, 1): 0, (16, 16, 20): 0, (18, 16, 5): 1, (16, 20, 1): 2, (20, 18, 1): 1}
BROKEN = {(16, 16, 20): {6: "last", 12: "two", 18: "inputs"}, (18, 16, 5): {2: "last"}}                # member -> how its witness is broken (at a point that is not boolean)
TWO = (200 * 256 + 5, 10 * 256 + 7)                                 # the output wires "two" changes = the first rows that fail
HALF = (P + 1) // 2
CANARY = 0xC3C3C3C3C3C3C3C3
GAP = 0x5A5A5A5A5A5A5A5A
PAD = 3                                                             # witness b starts n_wires + PAD elements after witness b - 1


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


_systems, _oracle_cache = {}, {}


def _system(n_x, n_y):
    """(System, R1cs) of a size, made once."""
    if (n_x, n_y) not in _systems:
        n_constraints, n_wires = SIZES[(n_x, n_y)]
        system = generate(n_constraints, n_wires, 40000 + 100 * n_x + n_y)
        r1cs = build_r1cs(*system.flat(), n_wires)
        csr, csc = r1cs.csr_info(), r1cs.csc_info()
        assert (csr["n"], csc["n_x"], csc["n_y"]) == (n_x, n_x, n_y) and csr["n_constraints"] == n_constraints and csr["n_wires"] == n_wires
        # what the case claims: wire 0 in every constraint of A, B and C; long rows up to the last real one, another count in every
        # matrix and none in C; the long columns the library sees are the arrays'
        assert system.column_lengths(0) == [n_constraints] * 3
        long_rows = system.long_rows()
        assert csr["n_long_rows"] == [len(l) for l in long_rows] and len(long_rows[0]) > len(long_rows[1]) > 20 and len(long_rows[2]) == 0
        assert int(long_rows[0][-1]) == n_constraints - 1 and int(system.counts[-3]) > 4096 and int(long_rows[0][0]) < 256
        assert csc["n_long_cols"] == system.long_columns() and csr["n_terms"] == system.nonzero_terms().sum(axis=0).tolist()
        _systems[(n_x, n_y)] = (system, r1cs)
    return _systems[(n_x, n_y)]


def _break(system, w, how):
    """how = "last": the last wire, which the last real row alone reads; "two": the output wires of the rows TWO; "inputs": three
    input wires, which rows all over the table read."""
    for wire in {"last": [system.n_wires - 1], "two": [system.n_in + k for k in TWO], "inputs": [5, 6, 7]}[how]:
        w[wire, 0] ^= np.uint64(1)
    return w


def _point(kind, n, rng):
    if kind == "boolean":
        return [rng.randrange(2) for _ in range(n)]
    z = [rng.randrange(P) for _ in range(n)]
    if kind == "half":
        z[n // 2] = HALF
    return z


class Case:
    """Everything the oracle says about one case: the witnesses W (batch, stride, 4) with GAP between them, the points Z, the
    weights RHO, per member the rows tables, first_bad, the two transcripts and the matrices' values at (r_x, r_y)."""

    def __init__(self, n_x, n_y, batch):
        self.key, self.n_x, self.n_y, self.batch = (n_x, n_y, batch), n_x, n_y, batch
        self.system, self.r1cs = _system(n_x, n_y)
        s = self.system
        self.flat, self.n_wires, self.n_constraints, self.stride = s.flat(), s.n_wires, s.n_constraints, s.n_wires + PAD
        self.broken = BROKEN.get(self.key, {})
        rng = random.Random(41000 + 1000 * n_x + 10 * n_y + batch)
        self.W = np.full((batch, self.stride, 4), GAP, dtype=np.uint64)
        for b in range(batch):
            w = witness(s, WITNESS_KINDS[b % 4], 42000 + 100 * n_x + b)
            self.W[b, :self.n_wires] = _break(s, w, self.broken[b]) if b in self.broken else w
        kinds = [POINTS[(FIRST_POINT[self.key] + b) % 3] for b in range(batch)]
        self.z = [_point(k, n_x, rng) for k in kinds]
        self.rho = [[rng.randrange(1, P) for _ in range(3)] for _ in range(batch)]
        if batch > 1:
            self.rho[1] = [1, P - 1, rng.randrange(1, P)]
        self.Z = cdense.to_limbs([v for z in self.z for v in z]).reshape(batch, n_x, 4)
        self.RHO = cdense.to_limbs([v for r in self.rho for v in r]).reshape(batch, 3, 4)
        self.rows = np.stack([cdense.r1cs_rows_raw(*self.flat, self.n_wires, self.W[b, :self.n_wires], n_x) for b in range(batch)])
        self.bad = [bad_rows(self.rows[b], self.n_constraints) for b in range(batch)]
        self.first_bad = np.array([int(x[0]) if len(x) else NO_BAD for x in self.bad], dtype=np.uint32)
        outs = [cdense.sumcheck_zerocheck_raw(self.rows[b], n_x, 3, R1CS_ZEROCHECK_TERMS, self.Z[b]) for b in range(batch)]
        self.zerocheck = tuple(np.stack([o[k] for o in outs]) for k in range(5))
        RX = self.zerocheck[2]
        self.T = np.stack([cdense.r1cs_cols_raw(*self.flat, self.n_wires, RX[b], self.RHO[b], n_y) for b in range(batch)])
        pairs = np.zeros((batch, 2, 1 << n_y, 4), dtype=np.uint64)
        pairs[:, 0] = self.T
        pairs[:, 1, :self.n_wires] = self.W[:, :self.n_wires]
        outs = [cdense.sumcheck_product_raw(pairs[b], n_y, 2) for b in range(batch)]
        self.inner = tuple(np.stack([o[k] for o in outs]) for k in range(4))
        self.matrices = np.stack([cdense.r1cs_matrix_evals_raw(*self.flat, self.n_wires, RX[b], self.inner[2][b]) for b in range(batch)])
        self._check()

    def honest(self, b):
        return b not in self.broken

    def claim(self, C, b):
        g = cdense.from_limbs(C[b, 0])
        return (sum(g) + g[-1]) % P                                 # g_1(0) + g_1(1); the unused leading slots are zero

    def _check(self):
        """The oracle-only preconditions."""
        n_c = self.n_constraints
        for b in range(self.batch):
            how = self.broken.get(b)
            if how is None:
                assert len(self.bad[b]) == 0 and self.claim(self.zerocheck[0], b) == 0, ("an honest witness", self.key, b)
            else:
                if how == "inputs":                                 # hundreds of blocks report a row; the lowest must win
                    assert len(np.unique(self.bad[b] // 256)) >= 200 and self.first_bad[b] == self.bad[b].min(), (self.key, b, len(self.bad[b]))
                else:
                    want = [n_c - 1] if how == "last" else sorted(TWO)
                    assert self.bad[b].tolist() == want and self.first_bad[b] == want[0], ("a broken witness", self.key, b, self.bad[b][:5])
                assert self.claim(self.zerocheck[0], b) != 0, ("a broken witness's claim", self.key, b)
            ex, et = cdense.from_limbs(self.zerocheck[3][b]), cdense.from_limbs(self.inner[3][b])[0]
            assert self.claim(self.inner[0], b) == sum(r * v for r, v in zip(self.rho[b], ex)) % P, ("sum_m rho_m v_m", self.key, b)
            assert et == sum(r * v for r, v in zip(self.rho[b], cdense.from_limbs(self.matrices[b]))) % P, ("e_T", self.key, b)
        assert TWO[0] // 256 != TWO[1] // 256


def _case(key):
    if key not in _oracle_cache:
        _oracle_cache[key] = Case(*key)
    return _oracle_cache[key]


def _assert_geometry(case):
    """Both sumchecks are multi-block, and run the pinned launch geometry where tests/product_shapes.py pins one."""
    for (n, pinned) in zip((case.n_x, case.n_y), PINNED[case.key]):
        geometry = product_geometry(n, case.batch)
        assert geometry[0][0] > 1 and geometry[1][0] > 1, (n, case.batch, geometry[:2])
        if pinned is not None:
            assert pinned == (n, case.batch)
            assert tuple(geometry[:2]) == PRODUCT_GEOMETRY[pinned], (n, case.batch)
        else:
            assert (n, case.batch) not in PRODUCT_GEOMETRY


def _canaried(ctx, count, slots):
    """Device memory for `slots` blocks of `count` elements, every one the canary."""
    return Resident(ctx, np.full((slots, count, 4), CANARY, dtype=np.uint64))


# ---- a. rows ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES)
def test_rows_and_first_bad_match_the_oracle(ctx, key):
    case = _case(key)
    _assert_geometry(case)
    n, batch = case.n_x, case.batch
    with ctx.r1cs_rows(case.r1cs) as handle, Resident(ctx, case.W) as dw, _canaried(ctx, 3 << n, batch + 1) as out:
        bad = ctx.r1cs_rows_device(handle, dw.d, batch, out.d, stride=case.stride)
        got = ctx.download(out.d, out.T.shape).reshape(batch + 1, 3, 1 << n, 4)
        dw.assert_unchanged(key)
        assert np.array_equal(bad, case.first_bad), (bad, case.first_bad)
        assert (got[batch] == np.uint64(CANARY)).all(), "nothing is written behind the batch"
        assert np.array_equal(got[:batch], case.rows), np.argwhere((got[:batch] != case.rows).any(axis=-1))[:4]
        assert not got[:batch, :, case.n_constraints:].any()
        if batch == 1:                                              # no spare member: the witness that breaks the last row alone, by itself
            w = _break(case.system, case.W[0, :case.n_wires].copy(), "last")
            want = cdense.r1cs_rows_raw(*case.flat, case.n_wires, w, n)
            assert bad_rows(want, case.n_constraints).tolist() == [case.n_constraints - 1], "oracle"
            ctx.upload(dw.d, w)
            bad = ctx.r1cs_rows_device(handle, dw.d, 1, out.d)
            assert bad.tolist() == [case.n_constraints - 1]
            assert np.array_equal(ctx.download(out.d, (3, 1 << n, 4)), want)


# ---- b. the zero-check ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES)
def test_zerocheck_matches_the_oracle_on_the_oracles_tables(ctx, key):
    case = _case(key)
    _assert_geometry(case)
    with ctx.r1cs_rows(case.r1cs) as handle, Resident(ctx, case.W) as dw:
        got = ctx.r1cs_zerocheck_batch_device(handle, dw.d, case.batch, case.Z, stride=case.stride)
        dw.assert_unchanged(key)
    assert np.array_equal(got[5], case.first_bad), (got[5], case.first_bad)
    assert_same(got[:5], case.zerocheck, ("the R1CS zero-check", key))
    assert [case.claim(got[0], b) == 0 for b in range(case.batch)] == [case.honest(b) for b in range(case.batch)]


# ---- c. the cols table ------------------------------------------------------------------------------------------------------------------
def _segments(length, segment):
    return (length + segment - 1) // segment if segment else 1


@pytest.mark.parametrize("key", CASES)
def test_cols_table_at_the_zerochecks_challenges_matches_the_oracle(ctx, key):
    case = _case(key)
    n_y, batch, n_c = case.n_y, case.batch, case.n_constraints
    assert _segments(n_c, SEG) == {(16, 16): 32, (18, 16): 65, (16, 20): 17, (20, 18): 512}[key[:2]]                 # per matrix, wire 0's column
    assert (3 * _segments(n_c, SEG) > 64) == (key[:2] != (16, 20)) and 3 * _segments(n_c, 64) > 64
    RX, stride = case.zerocheck[2], (1 << n_y) + 5
    for segment in (None, 0, 64) if key == (16, 16, 1) else (None,):
        with ctx.r1cs_cols(case.r1cs, segment=segment) as handle, _canaried(ctx, stride, batch + 1) as out:
            assert handle.info() == case.r1cs.csc_info()
            ctx.r1cs_cols_device(handle, RX, case.RHO, batch, out.d, stride=stride)
            got = ctx.download(out.d, out.T.shape)
        assert (got[batch] == np.uint64(CANARY)).all(), "nothing is written behind the batch"
        assert (got[:batch, 1 << n_y:] == np.uint64(CANARY)).all(), "nothing is written between the tables"
        got = got[:batch, :1 << n_y]
        assert np.array_equal(got, case.T), (segment, np.argwhere((got != case.T).any(axis=-1))[:4])
        assert not got[:, case.n_wires:].any()


# ---- d. the inner sumcheck --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES)
def test_inner_sumcheck_matches_the_product_oracle_on_the_oracles_tables(ctx, key):
    case = _case(key)
    _assert_geometry(case)
    with ctx.r1cs_cols(case.r1cs) as handle, Resident(ctx, case.W) as dw:
        got = ctx.r1cs_inner_batch_device(handle, dw.d, case.batch, case.zerocheck[2], case.RHO, stride=case.stride)
        dw.assert_unchanged(key)
    assert_same(got, case.inner, ("the R1CS inner sumcheck", key))
    for b in range(case.batch):                                     # (asserted on the oracle's transcript in Case._check)
        assert case.claim(got[0], b) == sum(r * v for r, v in zip(case.rho[b], cdense.from_limbs(case.zerocheck[3][b]))) % P


# ---- e. the matrices' extensions --------------------------------------------------------------------------------------------------------
def _bits(index, n):
    return [(index >> (n - 1 - j)) & 1 for j in range(n)]


@pytest.mark.parametrize("key", CASES)
def test_matrix_evals_match_the_oracle(ctx, key):
    case = _case(key)
    n_x, n_y, n_c, s = case.n_x, case.n_y, case.n_constraints, case.system
    rng = random.Random(43000 + n_x + n_y)
    last_row, its_c_wire = n_c - 1, int(s.wires[s.record(n_c - 1, 2, 1)])
    assert its_c_wire == case.n_wires - 1
    xs = [cdense.from_limbs(case.zerocheck[2][0]), _point("random", n_x, rng), _bits(last_row, n_x), _bits((1 << n_x) - 1, n_x)]
    ys = [cdense.from_limbs(case.inner[2][0]), _point("random", n_y, rng), _bits(its_c_wire, n_y), _bits((1 << n_y) - 1, n_y)]
    X, Y = (cdense.to_limbs([v for p in pts for v in p]).reshape(4, -1, 4) for pts in (xs, ys))
    want = np.stack([cdense.r1cs_matrix_evals_raw(*case.flat, case.n_wires, X[k], Y[k]) for k in range(4)])
    assert np.array_equal(want[0], case.matrices[0])
    assert not want[2, :2].any() and np.array_equal(want[2, 2], s.coeffs[s.record(n_c - 1, 2, 1)]), "the entry C[last row][its wire] = s"
    padded = n_c < 1 << n_x or case.n_wires < 1 << n_y
    assert padded == (key[:2] not in ((16, 16), (20, 18))) and (not want[3].any() if padded else np.array_equal(want[3], want[2]))
    with ctx.r1cs_rows(case.r1cs) as handle:
        got = ctx.r1cs_matrix_evals_device(handle, X, Y)
        again = ctx.r1cs_matrix_evals_device(handle, X, Y)
    assert np.array_equal(got, want), (got, want)
    assert got.tobytes() == again.tobytes()


# ---- f. the verifier --------------------------------------------------------------------------------------------------------------------
def _changed(case, record):
    """The R1CS with one coefficient changed (to 12345), and what that does to sum_m rho_m M_m~(r_x, r_y) per member."""
    coeffs = case.system.coeffs
    keep = coeffs[record].copy()
    assert not np.array_equal(keep, limbs(12345))
    coeffs[record] = limbs(12345)
    try:
        r1cs = build_r1cs(*case.flat, case.n_wires)
        mats = [cdense.from_limbs(cdense.r1cs_matrix_evals_raw(*case.flat, case.n_wires, case.zerocheck[2][b], case.inner[2][b])) for b in range(case.batch)]
    finally:
        coeffs[record] = keep
    return r1cs, [sum(r * v for r, v in zip(case.rho[b], mats[b])) % P for b in range(case.batch)]


def _eq_at(point, index):
    v = 1
    for j, x in enumerate(point):
        v = v * (x if (index >> (len(point) - 1 - j)) & 1 else 1 - x) % P
    return v


def _verdicts(result):
    accept, stage, rnd, check = result
    assert [bool(a) for a in accept] == [s == 0 for s in stage]
    return [(int(s), int(r), int(c)) for s, r, c in zip(stage, rnd, check)]


@pytest.mark.parametrize("key", CASES)
def test_verifier_verdicts_follow_from_the_oracle(ctx, key):
    """The stage order is verifier.verify_r1cs's: 1 the zero-check's transcript, 2 the inner sumcheck's, 3 MATRIX, 4 WITNESS."""
    case = _case(key)
    _assert_geometry(case)
    batch, n_y, n_c, s = case.batch, case.n_y, case.n_constraints, case.system
    ok, round_sum = (0, 0, 0), (1, 0, N.GKR_VERIFY_ROUND_SUM)
    base = [ok if case.honest(b) else round_sum for b in range(batch)]
    with ctx.r1cs_rows(case.r1cs) as rows, ctx.r1cs_cols(case.r1cs) as cols, Resident(ctx, case.W) as dw:
        zc = ctx.r1cs_zerocheck_batch_device(rows, dw.d, batch, case.Z, stride=case.stride)[:4]
        inner = ctx.r1cs_inner_batch_device(cols, dw.d, batch, zc[2], case.RHO, stride=case.stride)
        assert_same(zc, case.zerocheck[:4], ("the zero-check", key))
        assert_same(inner, case.inner, ("the inner sumcheck", key))

        def verify(handle, witness=True, zc=zc, inner=inner):
            return _verdicts(ctx.verify_r1cs_batch_device(handle, batch, case.Z, zc, case.RHO, inner, dw.d if witness else None,
                                                          case.stride if witness else None))
        assert verify(rows) == base and verify(rows, witness=False) == base
        # one coefficient changed: in the last real row (its 4097-term A), in a long row of a far block, in the last segment of
        # the wire-0 column of B
        far = int(case.system.long_rows()[0][-2])
        assert s.counts[3 * far] > LONG and far // 256 > (n_c // 256) // 2 and (n_c - 3) // SEG == (n_c - 1) // SEG
        records = [s.record(n_c - 1, 0, 2000), s.record(far, 0, 5), s.record(n_c - 3, 1, 0)]
        assert int(s.wires[records[2]]) == 0
        e_t = [cdense.from_limbs(case.inner[3][b])[0] for b in range(batch)]
        for record in records:
            r1cs, moved = _changed(case, record)
            assert all(moved[b] != e_t[b] for b in range(batch)), "the change moves sum_m rho_m M_m~"
            with ctx.r1cs_rows(r1cs) as other:
                assert verify(other) == [(3, n_y, N.GKR_VERIFY_MATRIX) if case.honest(b) else round_sum for b in range(batch)], record
        # the last wire of every resident witness changed (an honest proof of another witness)
        for b in range(batch):
            assert _eq_at(cdense.from_limbs(case.inner[2][b]), case.n_wires - 1) != 0, "the change moves w~(r_y)"
        W2 = case.W.copy()
        W2[:, case.n_wires - 1, 0] ^= np.uint64(2)
        ctx.upload(dw.d, W2)
        assert verify(rows) == [(4, n_y, N.GKR_VERIFY_WITNESS) if case.honest(b) else round_sum for b in range(batch)]
        assert verify(rows, witness=False) == base
        ctx.upload(dw.d, case.W)
        if key == (16, 16, 1):
            _python_verifier_agrees(case, verify, rows, zc, inner, records[0], ctx)


def _python_verifier_agrees(case, verify, rows, zc, inner, record, ctx):
    """The honest proof and one tamper per stage through verifier.verify_r1cs as well: the two verifiers give one verdict."""
    cons = constraints_of(*case.flat, case.n_constraints)
    w = cdense.from_limbs(case.W[0, :case.n_wires])

    def rounds(C, L):
        return [cdense.from_limbs(C[0, j])[C.shape[2] - int(L[0, j]):] for j in range(C.shape[1])]

    def python(cons, zc, inner, witness):
        return verify_r1cs(cons, case.z[0], case.rho[0], rounds(zc[0], zc[1]), cdense.from_limbs(zc[2][0]), cdense.from_limbs(zc[3][0]),
                           rounds(inner[0], inner[1]), cdense.from_limbs(inner[2][0]), cdense.from_limbs(inner[3][0]), witness)
    assert python(cons, zc, inner, w) == (0, 0, 0)
    one = tuple(a.copy() for a in zc)
    one[0][0, 7, 3, 0] ^= np.uint64(1)                              # round 7's constant coefficient
    assert verify(rows, zc=one) == [python(cons, one, inner, w)] == [(1, 7, N.GKR_VERIFY_ROUND_SUM)]
    two = tuple(a.copy() for a in inner)
    two[3][0, 1, 0] ^= np.uint64(1)                                 # e_w
    assert verify(rows, inner=two) == [python(cons, zc, two, w)] == [(2, case.n_y, N.GKR_VERIFY_EVALUATION)]
    i = int(np.searchsorted(case.system.offset, record, side="right")) - 1
    t = record - case.system.record(i, 0, 0)
    changed = list(cons)
    changed[i] = ([(12345, k) if at == t else (c, k) for at, (c, k) in enumerate(cons[i][0])],) + tuple(cons[i][1:])
    assert python(changed, zc, inner, w) == (3, case.n_y, N.GKR_VERIFY_MATRIX)
    w2 = w[:]
    w2[-1] ^= 2
    assert python(cons, zc, inner, w2) == (4, case.n_y, N.GKR_VERIFY_WITNESS)

"""gkr_sumcheck_product_batch_device (csrc/kernels_product.hip, csrc/capi_product.hip) bit for bit against the C oracle's
ogkr_sumcheck_product (cdense.sumcheck_product_raw; tests/test_oracle_product_c.py holds it to the model, the reference's prover and
the plain C sumcheck) at the smallest shapes that reach each launch geometry tests/product_shapes.py pins: several trips of the
round kernel's wave loop over partials that differ per block, block counts that are no power of two (trailing blocks with an
empty range), chunks of 512, 1024 and 2048 entries (2 .. 8 table pairs per thread into one lazy sum), the cap of 2048 blocks, and
the per-factor flags when only a far block sets them.

  a. the shape matrix at degree 2 and 3, factor kinds mixed per (sumcheck, factor);
  b. "depends on x_n" / "has a non-zero entry" set by a single entry in a far block, in the lower and in the upper half;
  c. two factors that ignore x_1: round 0's leading coefficients cancel over every block;
  d. the device verifier and its evaluation kernel on the same shapes against the oracle's values, and one tampered entry;
  e. degree 1 against the plain C sumcheck and the plain device path.

Tables are built with numpy on limb arrays; the oracle is called once per sumcheck and its results are kept."""

import numpy as np
import pytest

from gkr_amd import Context
from gkr_amd import _native as N
from oracle import cdense
from oracle.field import P
from product_model import SPECIALS
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from resident_tables import Resident, assert_same as _assert_same

pytestmark = pytest.mark.gpu

MIX = ["random", "specials", "indep_last", "bits", "indep_first"]
# (n, batch, degree): every row of PRODUCT_GEOMETRY at degree 2 and 3; n = 23 (512 MiB of tables at degree 2) at degree 2 only
MATRIX = [(n, batch, degree) for (n, batch) in PRODUCT_GEOMETRY for degree in (2, 3) if (n, degree) != (23, 3)]
ACCEPTED = (True, 0, 0)


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _value(limbs):
    return sum(int(x) << (64 * k) for k, x in enumerate(limbs))


def _assert_geometry(n, batch):
    assert tuple(product_geometry(n, batch)[:2]) == PRODUCT_GEOMETRY[(n, batch)], (n, batch)


def _kinds(n, batch, degree):
    return [[MIX[(n + 2 * b + 3 * f + degree) % len(MIX)] for f in range(degree)] for b in range(batch)]


def _tables(n, batch, degree):
    """(batch, degree, 2^n, 4) limbs: cdense.fill_table's values, the structured kinds sliced in."""
    size, h = 1 << n, 1 << (n - 1)
    T = cdense.fill_table((batch * degree) << n, 7700 + 97 * n + 7 * degree + batch).reshape(batch, degree, size, 4)
    rng = np.random.default_rng(8800 + 97 * n + 7 * degree + batch)
    specials = cdense.to_limbs(SPECIALS)
    for b, row in enumerate(_kinds(n, batch, degree)):
        for f, kind in enumerate(row):
            t = T[b, f]
            if kind == "specials":
                t[:] = specials[rng.integers(0, len(SPECIALS), size=size)]
            elif kind == "bits":
                t[:] = 0
                t[:, 0] = rng.integers(0, 2, size=size, dtype=np.uint64)
            elif kind == "indep_last":
                t[1::2] = t[0::2]
            elif kind == "indep_first":
                t[h:] = t[:h]
    return T


_oracle_cache = {}


def _oracle(key, T):
    """cdense.sumcheck_product_raw per sumcheck of T (batch, degree, 2^n, 4), stacked as the device returns them; computed once per key."""
    if key not in _oracle_cache:
        batch, degree, size = T.shape[:3]
        n = size.bit_length() - 1
        outs = [cdense.sumcheck_product_raw(T[b], n, degree) for b in range(batch)]
        _oracle_cache[key] = tuple(np.stack([o[k] for o in outs]) for k in range(4))
    return _oracle_cache[key]


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,degree", MATRIX)
def test_shape_matrix_matches_the_c_oracle(ctx, n, batch, degree):
    _assert_geometry(n, batch)
    T = _tables(n, batch, degree)
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_product_batch_device(dev.d, n, degree, batch)
    _assert_same(got, _oracle((n, batch, degree), T), (n, batch, degree))


def test_the_shape_matrix_reaches_short_vectors_in_the_first_and_the_last_round():
    """(oracle only) a round-0 vector and a last-round vector shorter than degree + 1 both occur in the matrix, at every degree."""
    for degree in (2, 3):
        where = set()
        for n, batch, d in MATRIX:
            if d == degree:
                L = _oracle((n, batch, d), None if (n, batch, d) in _oracle_cache else _tables(n, batch, d))[1]
                where |= {"first"} if (L[:, 0] < degree + 1).any() else set()
                where |= {"last"} if (L[:, -1] < degree + 1).any() else set()
        assert where == {"first", "last"}, (degree, where)


# ---- b. flags that only a far block sees ------------------------------------------------------------------------------------------------
def _far_flag_base(n, seed):
    """(3, 2^n, 4): factor 0 ignores x_n, factor 1 is the zero table, factor 2 is random."""
    T = cdense.fill_table(3 << n, seed).reshape(3, 1 << n, 4)
    T[0, 1::2] = T[0, 0::2]
    T[1] = 0
    return T


def _differs(T0, even):
    """Entry even + 1 of a factor made to differ from entry `even`."""
    out = T0[even].copy()
    out[0] ^= np.uint64(1)                      # (fill_table's values are below 2^253: still canonical)
    return out


# variant -> (factor 0 has ONE pair that differs: where; factor 1 has ONE non-zero entry)
VARIANTS = [("lower", True), ("upper", True), (None, True), ("lower", False)]


def _assert_far_flags(variant, C, L, E, what):
    pair, nonzero = variant
    if not nonzero:                              # a zero factor: every vector [0], whatever else is in the tables
        assert (L == 1).all() and not C.any() and not E[1].any(), what
    else:                                        # the zero-factor rule does not apply; the last length counts factors 1, 2 and, with a pair, 0
        assert C[:, :-1].any() and L.max() > 1, what
        assert L[-1] == (4 if pair else 3), (what, int(L[-1]))


def test_flags_set_by_one_entry_in_a_far_block_of_2048(ctx):
    """n = 20, batch 1, degree 3: 2048 blocks of 256.  The pair that makes factor 0 depend on x_n sits in block 1999 (lower half)
    or in block 70's upper-half entries; factor 1's only non-zero entry in block 1500's upper-half entries."""
    n, degree = 20, 3
    _assert_geometry(n, 1)
    h = 1 << (n - 1)
    where = {"lower": 256 * 1999 + 130, "upper": h + 256 * 70 + 130}
    entry = h + 256 * 1500 + 77
    value = cdense.fill_table(1, 20077)[0]
    size = 1 << n
    with Resident(ctx, _far_flag_base(n, 2020)) as dev:
        T = dev.T
        for vi, (pair, nonzero) in enumerate(VARIANTS):
            if pair:
                dev.set_entry(where[pair] + 1, _differs(T[0], where[pair]))
            if nonzero:
                dev.set_entry(size + entry, value)
            got = ctx.sumcheck_product_batch_device(dev.d, n, degree, 1)
            want = _oracle(("far", n, vi), T[None])
            _assert_far_flags((pair, nonzero), want[0][0], want[1][0], want[3][0], ("oracle", vi))
            _assert_same(got, want, ("far flags", n, pair, nonzero))
            if pair:                                                     # back to the base tables
                dev.set_entry(where[pair] + 1, T[0, where[pair]].copy())
            dev.set_entry(size + entry, np.zeros(4, dtype=np.uint64))


def test_flags_set_by_one_entry_in_the_last_working_blocks_of_103(ctx):
    """n = 16, batch 20, degree 3: 103 blocks of chunk 512, of which the first 64 have entries -- the round kernel's first trip
    ends with the blocks that hold the flags (blocks 62 and 63, counted from 0), its second trip reads 39 empty ones.  Sumcheck b
    runs variant b % 4."""
    n, degree, batch = 16, 3, 20
    _assert_geometry(n, batch)
    h, size = 1 << (n - 1), 1 << n
    where = {"lower": 512 * 62 + 130, "upper": h + 512 * 63 + 130}
    entry = h + 512 * 63 + 77
    T = np.stack([_far_flag_base(n, 1600 + b) for b in range(batch)])
    for b in range(batch):
        pair, nonzero = VARIANTS[b % 4]
        if pair:
            T[b, 0, where[pair] + 1] = _differs(T[b, 0], where[pair])
        if nonzero:
            T[b, 1, entry] = cdense.fill_table(1, 16077 + b)[0]
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_product_batch_device(dev.d, n, degree, batch)
    want = _oracle(("far", n), T)
    for b in range(batch):
        _assert_far_flags(VARIANTS[b % 4], want[0][b], want[1][b], want[3][b], ("oracle", b))
    _assert_same(got, want, ("far flags", n, batch))


# ---- c. two factors that ignore x_1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,which", [(16, (0, 1)), (20, (0, 2))])
def test_leading_coefficients_cancel_over_every_block(ctx, n, which):
    """batch 1, degree 3, two factors with T[h:] = T[:h]: round 0's polynomial is linear, its c_3 and c_2 are sums over 128 or
    2048 blocks' partials that cancel exactly."""
    degree = 3
    _assert_geometry(n, 1)
    h = 1 << (n - 1)
    T = cdense.fill_table(degree << n, 3300 + n).reshape(1, degree, 1 << n, 4)
    for f in which:
        T[0, f, h:] = T[0, f, :h]
    want = _oracle(("indep_first", n), T)
    assert want[1][0, 0] == 2 and (want[1][0, 1:] == degree + 1).all()
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_product_batch_device(dev.d, n, degree, 1)
    _assert_same(got, want, ("two factors ignore x_1", n))


# ---- d. the verifier and the evaluation kernel at the same sizes ----------------------------------------------------------------------------
def _eq(point, index):
    """prod_i (bit_i(index) ? point_i : 1 - point_i), variable 1 = most significant bit, on Python integers."""
    k, v = len(point), 1
    for i, x in enumerate(point):
        v = v * (x if (index >> (k - 1 - i)) & 1 else 1 - x) % P
    return v


def _triples(res):
    return [(bool(a), int(r), int(c)) for a, r, c in zip(res[0], res[1], res[2])]


@pytest.mark.parametrize("n,batch,degree", MATRIX)
def test_verifier_accepts_and_its_evaluations_are_the_oracles(ctx, n, batch, degree):
    _assert_geometry(n, batch)
    T = _tables(n, batch, degree)
    want = _oracle((n, batch, degree), T)
    # the sums the transcripts prove, from the oracle's round 0: P(0) + P(1) = 2 c_0 + c_1 + .. + c_d (unused slots are zero)
    claims = cdense.to_limbs([(sum(cdense.from_limbs(want[0][b, 0])) + _value(want[0][b, 0, degree])) % P for b in range(batch)])
    h, (nblk, chunk) = 1 << (n - 1), PRODUCT_GEOMETRY[(n, batch)][0]
    index = h + ((h + chunk - 1) // chunk - 1) * chunk + 77              # the upper half's entries of round 0's last working block
    assert h < index < 2 * h and (h + chunk - 1) // chunk <= nblk
    with Resident(ctx, T) as dev:
        C, L, R, E = ctx.sumcheck_product_batch_device(dev.d, n, degree, batch)
        res = ctx.verify_sumcheck_product_batch_device(dev.d, n, degree, batch, C, L, R, claims=claims)
        assert _triples(res) == [ACCEPTED] * batch, (n, batch, degree)
        assert np.array_equal(res[3], claims)
        _assert_same((C, L, R, res[4]), want, ("verifier's evaluations", n, batch, degree))
        # one entry of the last sumcheck's last factor set to x + 1
        flat = ((batch * degree - 1) << n) + index
        x = _value(T[batch - 1, degree - 1, index])
        dev.set_entry(flat, cdense.to_limbs([(x + 1) % P])[0])
        res = ctx.verify_sumcheck_product_batch_device(dev.d, n, degree, batch, C, L, R, claims=claims)
    assert _triples(res) == [ACCEPTED] * (batch - 1) + [(False, n, N.GKR_VERIFY_EVALUATION)], (n, batch, degree)
    keep = np.ones((batch, degree), dtype=bool)
    keep[batch - 1, degree - 1] = False
    assert np.array_equal(res[4][keep], want[3][keep])
    moved = (_value(want[3][batch - 1, degree - 1]) + _eq(cdense.from_limbs(want[2][batch - 1]), index)) % P
    assert _value(res[4][batch - 1, degree - 1]) == moved


# ---- e. degree 1 through the product entry point ----------------------------------------------------------------------------------------
def test_degree_one_equals_the_plain_c_sumcheck_and_the_plain_device_path(ctx):
    n, batch = 20, 4
    _assert_geometry(n, batch)
    h = 1 << (n - 1)
    T = cdense.fill_table(batch << n, 2004).reshape(batch, 1, 1 << n, 4)
    T[1, 0, 1::2] = T[1, 0, 0::2]                                       # one table that ignores x_n, one that ignores x_1
    T[2, 0, h:] = T[2, 0, :h]
    plain_c = [cdense.sumcheck_mle_raw(T[b, 0], n) for b in range(batch)]
    with Resident(ctx, T) as dev:
        C, L, R, E = ctx.sumcheck_product_batch_device(dev.d, n, 1, batch)
        plain = ctx.sumcheck_mle_batch_device(dev.d, n, batch)
    want = tuple(np.stack([o[k] for o in plain_c]) for k in range(3))
    assert L[1, -1] == 1 and L[2, 0] == 1
    _assert_same((C, L, R, E), want + (E,), ("degree 1 against ogkr_sumcheck_mle", n, batch))
    _assert_same(plain + (E,), want + (E,), ("the plain device path against ogkr_sumcheck_mle", n, batch))
    _assert_same((C, L, R, E), _oracle(("degree 1", n, batch), T), ("degree 1 against ogkr_sumcheck_product", n, batch))

"""gkr_sumcheck_zerocheck_batch_device (csrc/kernels_zerocheck.hip, csrc/capi_zerocheck.hip) bit for bit against the C oracle's
ogkr_sumcheck_zerocheck (cdense.sumcheck_zerocheck_raw; tests/test_oracle_sop_c.py holds it to the implicit model and the
reference's prover) at the launch geometries tests/product_shapes.py pins.  The oracle writes eq(z, .) out as a table of 2^n
entries and shares no code with the library, so what is the zero-check's own -- E_hi[i >> 8] with several entries per block at
chunks of 512 and more, the E_lo product after the lazy reduction, the (fa + fb X) h_j step -- and what it shares with the
sum-of-products path are both held to something independent.  EVERY sumcheck of every case is compared: coefficients, lengths,
challenges, evaluations and eq(z, r), and the inputs are downloaded afterwards and must be unchanged.

  a. the shape matrix: every row of PRODUCT_GEOMETRY, all five structures, factor kinds mixed per (sumcheck, table), a point per
     sumcheck: random, boolean, 0 / 1 / random mixed, and z_j = 1/2 (where 2 z_j - 1 = 0 and the round's leading coefficient
     vanishes because of the linear factor, not because of h_j) at index 0, at index n - 9 (the round where E_hi becomes [1]) and at
     the last index; eq(z, r) against the closed form;
  b. cancellation between terms over every block; c. tables that ignore x_1 and x_n;
  d. lazy-sum headroom per term with a boolean and with a random point;
  e. byte equality with the SOP path on the device-built eq table at the four geometries tests/test_gpu_zerocheck.py leaves out."""

import random

import numpy as np
import pytest

from gkr_amd import Context
from oracle import cdense
from oracle.field import P
from oracle.mimc7 import multi_hash
from product_model import SPECIALS
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from resident_tables import Resident, assert_same, free_bytes, structured_tables
from sop_model import STRUCTURES
from test_gpu_zerocheck import _assert_bytes_equal, _both_paths
from zerocheck_model import zc_degree

pytestmark = pytest.mark.gpu

MIX = ["random", "specials", "indep_last", "bits", "indep_first", "indep_middle"]
POINTS = ["random", "boolean", "mixed", "half at index 0", "half at index n - 9", "half at the last index"]
HALF = (P + 1) // 2
SPECIAL_LIMBS = cdense.to_limbs(SPECIALS + [P - 1])
ZC_STRUCTURES = [s for s in STRUCTURES if s[0] in ("AB-C", "5AB+7BC+11A", "AA+3B", "AB-AB", "AB-AC")]
# (n, batch, structure, the point kind of sumcheck 0 -- sumcheck b takes the b-th after it): every row of PRODUCT_GEOMETRY with a
# structure of its own, and all five at the smallest row; n = 23 (256 MiB a table) runs on the two-table structure only
MATRIX = [(16, 1, "AB-AB", 0), (16, 20, "5AB+7BC+11A", 0), (18, 5, "AB-C", 1), (19, 3, "AB-AC", 3), (20, 1, "AB-C", 4), (20, 4, "5AB+7BC+11A", 2),
          (23, 1, "AA+3B", 5), (16, 1, "AB-C", 3), (16, 1, "5AB+7BC+11A", 4), (16, 1, "AA+3B", 5), (16, 1, "AB-AC", 1)]
LEFT_OUT = [(18, 5), (19, 3), (20, 4), (23, 1)]                    # what test_bytes_equal_the_sop_path_at_multi_block_shapes does not run


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _structure(name):
    return next(s for s in STRUCTURES if s[0] == name)


def _assert_geometry(n, batch):
    assert tuple(product_geometry(n, batch)[:2]) == PRODUCT_GEOMETRY[(n, batch)], (n, batch)


def _point(kind, n, rng):
    z = [rng.randrange(P) for _ in range(n)]
    if kind == "boolean":
        z = [rng.randrange(2) for _ in range(n)]
    elif kind == "mixed":
        z = [(0, 1, x)[(j + n) % 3] for j, x in enumerate(z)]
    elif kind != "random":
        z[{"half at index 0": 0, "half at index n - 9": n - 9, "half at the last index": n - 1}[kind]] = HALF
    return z


def _point_kinds(batch, first):
    return [POINTS[(first + b) % len(POINTS)] for b in range(batch)]


def _points(n, kinds, seed):
    """-> (batch, n, 4) limbs."""
    rng = random.Random(seed)
    return cdense.to_limbs([x for kind in kinds for x in _point(kind, n, rng)]).reshape(len(kinds), n, 4)


def _kinds(n, batch, M):
    return [[MIX[(n + 2 * b + 5 * m + M) % len(MIX)] for m in range(M)] for b in range(batch)]


def _matrix_case(n, batch, name, first):
    M = _structure(name)[1]
    seed = 9500 + 97 * n + 7 * len(name) + batch
    return structured_tables(_kinds(n, batch, M), n, seed, SPECIAL_LIMBS), _points(n, _point_kinds(batch, first), seed + 2)


_oracle_cache = {}


def _oracle(key, case, terms):
    """cdense.sumcheck_zerocheck_raw per sumcheck of (T (batch, M, 2^n, 4), Z (batch, n, 4)), stacked as the device returns them
    (C, L, R, E, Q); computed once per key.  case may be a function that builds the pair (not called when the key is known)."""
    if key not in _oracle_cache:
        T, Z = case() if callable(case) else case
        batch, M, size = T.shape[:3]
        n = size.bit_length() - 1
        outs = [cdense.sumcheck_zerocheck_raw(T[b], n, M, terms, Z[b]) for b in range(batch)]
        _oracle_cache[key] = tuple(np.stack([o[k] for o in outs]) for k in range(5))
    return _oracle_cache[key]


def _closed_form_eq(Z, R):
    """prod_j (z_j r_j + (1 - z_j)(1 - r_j)) per sumcheck, as (batch, 4) limbs."""
    out = []
    for zb, rb in zip(Z, R):
        v = 1
        for zj, rj in zip(cdense.from_limbs(zb), cdense.from_limbs(rb)):
            v = v * (zj * rj + (1 - zj) * (1 - rj)) % P
        out.append(v)
    return cdense.to_limbs(out)


def _run(ctx, T, Z, terms, want, what):
    batch, M, size = T.shape[:3]
    assert np.array_equal(want[4], _closed_form_eq(Z, want[2])), ("eq(z, r) in closed form", what)
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_zerocheck_batch_device(dev.d, size.bit_length() - 1, M, terms, batch, Z)
        dev.assert_unchanged(what)
    assert_same(got, want, what)


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,name,first", MATRIX)
def test_shape_matrix_matches_the_c_oracle(ctx, n, batch, name, first):
    _assert_geometry(n, batch)
    terms = _structure(name)[2]
    T, Z = _matrix_case(n, batch, name, first)
    _run(ctx, T, Z, terms, _oracle((n, batch, name), (T, Z), terms), (n, batch, name))


def test_the_shape_matrix_covers_every_structure_and_point_and_reaches_short_vectors():
    """(oracle only) every row of the geometry table, every structure and every kind of point is in the matrix.  Outside
    A B - A B (all [0]) a vector shorter than D + 1 occurs in round 0, in a round strictly between the first and the last, and in
    the last round; and in each of the three places at least once BECAUSE OF z_j = 1/2 ALONE: the vector of the round whose z_j is
    1/2 has exactly D entries with a non-zero first one, so h_j has its full degree D - 1 there."""
    assert {(n, b) for n, b, _, _ in MATRIX} == set(PRODUCT_GEOMETRY) and {s for _, _, s, _ in MATRIX} == {s[0] for s in ZC_STRUCTURES}
    short, by_half, points = set(), set(), set()
    for n, batch, name, first in MATRIX:
        terms = _structure(name)[2]
        C, L, R, E, Q = _oracle((n, batch, name), lambda: _matrix_case(n, batch, name, first), terms)
        D = zc_degree(terms)
        kinds = _point_kinds(batch, first)
        points |= set(kinds)
        if name == "AB-AB":
            assert (L == 1).all() and not C.any()
            continue
        for where, part in (("first", L[:, 0]), ("middle", L[:, 1:-1]), ("last", L[:, -1])):
            short |= {where} if (part < D + 1).any() else set()
        for b, kind in enumerate(kinds):
            for where, j in (("half at index 0", 0), ("half at index n - 9", n - 9), ("half at the last index", n - 1)):
                if kind == where:
                    assert L[b, j] <= D, (n, batch, name, b, kind)                        # 2 z_j - 1 = 0: never the full length
                    if L[b, j] == D and C[b, j, 1].any():
                        by_half.add(where)
    assert points == set(POINTS)
    assert short == {"first", "middle", "last"}, short
    assert by_half == set(POINTS[3:]), by_half


# ---- b. cancellation between terms over every block -----------------------------------------------------------------------------------------
def _bump(entry):
    out = entry.copy()
    out[0] ^= np.uint64(1)                                          # (cdense.fill_table's values are below 2^253: still canonical)
    return out


def test_terms_cancel_on_all_but_one_index_of_a_far_block_of_2048(ctx):
    """n = 20, batch 1, A B - A C at a random point.  C = B: all [0].  Then ONE entry of C in block 1500's upper-half entries
    differs: g lives on one index of the upper half, so round 0's constant coefficient is zero."""
    n = 20
    _assert_geometry(n, 1)
    _, M, terms = _structure("AB-AC")
    index = (1 << (n - 1)) + 256 * 1500 + 77
    T = cdense.fill_table(M << n, 2022).reshape(1, M, 1 << n, 4)
    T[0, 2] = T[0, 1]
    Z = _points(n, ["random"], 2023)
    zero_r = cdense.to_limbs([multi_hash([0], 0)])[0]
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_zerocheck_batch_device(dev.d, n, M, terms, 1, Z)
        want = _oracle(("cancel", n, "all"), (dev.T, Z), terms)
        assert (want[1] == 1).all() and not want[0].any() and (want[2] == zero_r).all(), "oracle"
        assert_same(got, want, ("A B - A C with C = B", n))
        dev.set_entry((2 << n) + index, _bump(dev.T[0, 2, index]))
        got = ctx.sumcheck_zerocheck_batch_device(dev.d, n, M, terms, 1, Z)
        dev.assert_unchanged("one index")
        want = _oracle(("cancel", n, "one"), (dev.T, Z), terms)
        assert want[0][0, 0, :3].any() and not want[0][0, 0, 3].any(), "oracle"                          # g_1(0) == 0
        assert_same(got, want, ("A B - A C with C = B but for one entry", n))


def test_terms_cancel_in_the_middle_sumchecks_of_103_blocks(ctx):
    """n = 16, batch 20, A B - A C, the six kinds of point in turn.  Odd sumchecks: C = B, all [0] with r = multi_hash([0], 0);
    sumchecks 0, 4, ..: C random; sumchecks 2, 6, ..: C = B but for one entry in the upper-half entries of block 62 or 63."""
    n, batch = 16, 20
    _assert_geometry(n, batch)
    _, M, terms = _structure("AB-AC")
    h = 1 << (n - 1)
    T = cdense.fill_table((batch * M) << n, 1622).reshape(batch, M, 1 << n, 4)
    for b in range(batch):
        if b % 4:
            T[b, 2] = T[b, 1]
        if b % 4 == 2:
            index = h + 512 * (62 + (b // 4) % 2) + 77 + b
            T[b, 2, index] = _bump(T[b, 2, index])
    kinds = _point_kinds(batch, 0)
    Z = _points(n, kinds, 1623)
    want = _oracle(("cancel", n, batch), (T, Z), terms)
    zero_r = cdense.to_limbs([multi_hash([0], 0)])[0]
    for b in range(batch):
        if b % 2:
            assert (want[1][b] == 1).all() and not want[0][b].any() and (want[2][b] == zero_r).all(), ("oracle", b)
        elif b % 4 == 0 and kinds[b] in ("random", "mixed"):
            assert (want[1][b] == 4).all(), ("oracle", b, want[1][b])
        elif b % 4 == 2 and kinds[b] not in ("boolean", "mixed"):                                      # (a 0 / 1 entry of z can zero the index's weight)
            assert want[0][b, 0, :3].any() and not want[0][b, 0, 3].any(), ("oracle", b)                # g_1(0) == 0
    _run(ctx, T, Z, terms, want, ("A B - A C, zero in the middle", n, batch))


# ---- c. tables that ignore x_1, and x_n -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 20])
def test_tables_that_ignore_the_first_and_the_last_variable(ctx, n):
    """batch 1, A B - C at a random point.  A and B ignore x_1: h_1 is linear, the A B term's c_2 and c_1 being sums over 128 or 2048
    blocks' weighted partials that cancel exactly.  B ignores x_n as well: h_n is linear."""
    _assert_geometry(n, 1)
    _, M, terms = _structure("AB-C")
    h = 1 << (n - 1)
    T = cdense.fill_table(M << n, 3500 + n).reshape(1, M, 1 << n, 4)
    T[0, 1, 1::2] = T[0, 1, 0::2]
    for m in (0, 1):
        T[0, m, h:] = T[0, m, :h]
    Z = _points(n, ["random"], 3600 + n)
    want = _oracle(("indep", n), (T, Z), terms)
    assert want[1][0, 0] == 3 and want[1][0, -1] == 3 and (want[1][0, 1:-1] == 4).all(), ("oracle", want[1])
    _run(ctx, T, Z, terms, want, ("A and B ignore x_1, B ignores x_n", n))


# ---- d. lazy-sum headroom per term ----------------------------------------------------------------------------------------------------------
def test_largest_entries_at_four_pairs_per_thread(ctx):
    """(20, 4), 5 A B + 7 B C + 11 A, chunk 1024: a thread adds 4 unreduced products into one lazy sum per term and value -- for a
    degree-1 term T[i] E_hi[c] with four different E_hi entries, for a degree-2 term (T[i] E_hi[c]) T'[i] -- against the 2^36 a Lazy17
    takes (csrc/fr32.h); the E_lo product follows the reduction.  Sumchecks 0, 1: every entry r - 1, at a boolean and at a random
    point; sumchecks 2, 3: the special byte patterns, at a boolean and at a random point."""
    n, batch = 20, 4
    _assert_geometry(n, batch)
    _, M, terms = _structure("5AB+7BC+11A")
    T = structured_tables([[k] * M for k in ("all_max", "all_max", "specials", "specials")], n, 4700, SPECIAL_LIMBS)
    Z = _points(n, ["boolean", "random", "boolean", "random"], 4701)
    _run(ctx, T, Z, terms, _oracle(("headroom", n, batch), (T, Z), terms), ("largest entries", n, batch))


@pytest.mark.parametrize("kind", ["all_max", "specials"])
def test_largest_entries_at_eight_pairs_per_thread(ctx, kind):
    """(23, 1), A A + 3 B, chunk 2048: 8 unreduced products per lane, term and value, with eight different E_hi entries, against
    2^36.  Both tables r - 1 everywhere, or the special byte patterns; each at a boolean and at a random point, on the same
    resident tables."""
    n = 23
    _assert_geometry(n, 1)
    _, M, terms = _structure("AA+3B")
    T = structured_tables([[kind] * M], n, 4800, SPECIAL_LIMBS)
    with Resident(ctx, T) as dev:
        for point in ("boolean", "random"):
            Z = _points(n, [point], 4801)
            want = _oracle(("headroom", n, kind, point), (T, Z), terms)
            assert np.array_equal(want[4], _closed_form_eq(Z, want[2]))
            got = ctx.sumcheck_zerocheck_batch_device(dev.d, n, M, terms, 1, Z)
            assert_same(got, want, ("largest entries", n, kind, point))
        dev.assert_unchanged((n, kind))


def test_eight_terms_over_eight_tables_at_chunk_512(ctx):
    """n = 16, batch 20, eight terms of degree 1 and 2 over eight tables (a zero coefficient, r - 1, r - 2 and a 241-bit one): eight
    weighted partials per block, 2 products per lane and term with two E_hi entries per block.  Sumcheck b: every table r - 1
    (b = 0 mod 3), the special patterns (1 mod 3), kinds mixed per table (2 mod 3); the six kinds of point in turn."""
    n, batch, M = 16, 20, 8
    _assert_geometry(n, batch)
    terms = [((0, 1, P - 1, 0x1234567890ABCDEF << 180, 2, P - 2, 1, 5)[k], (k, (k + 3) % 8)[:1 + k % 2]) for k in range(8)]
    assert {i for _, idx in terms for i in idx} == set(range(M))
    rows = [[("all_max", "specials", MIX[(b + 5 * m) % len(MIX)])[b % 3] for m in range(M)] for b in range(batch)]
    T = structured_tables(rows, n, 4900, SPECIAL_LIMBS)
    Z = _points(n, _point_kinds(batch, 1), 4901)
    _run(ctx, T, Z, terms, _oracle(("eight terms", n, batch), (T, Z), terms), ("eight terms over eight tables", n, batch))


# ---- e. the SOP path on the device-built eq table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", LEFT_OUT)
def test_bytes_equal_the_sop_path_at_the_other_multi_block_shapes(ctx, n, batch):
    """The matrix's tables and points of this row (1/2 entries and boolean points included, so not every vector has full
    length): gkr_sumcheck_sop_batch_device on {gkr_eq_table_device's table, T_0 ..} with the lifted terms gives the zero-check's
    bytes, and both are the oracle's."""
    _assert_geometry(n, batch)
    name, first = next((s, f) for (nn, bb, s, f) in MATRIX if (nn, bb) == (n, batch))
    M, terms = _structure(name)[1:]
    T, Z = _matrix_case(n, batch, name, first)
    if free_bytes() < int(1.75 * (T.nbytes + T.nbytes // M * (M + 1))):
        pytest.skip("not enough free device memory for %d MiB of tables" % ((2 * T.nbytes + T.nbytes // M) >> 20))
    sop, zc = _both_paths(ctx, T, n, terms, Z)
    _assert_bytes_equal(sop, zc, (n, batch))
    assert_same(zc, _oracle((n, batch, name), (T, Z), terms), ("against the oracle", n, batch, name))

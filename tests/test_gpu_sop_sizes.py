"""gkr_sumcheck_sop_batch_device (csrc/kernels_sop.hip, csrc/capi_sop.hip) bit for bit against the C oracle's ogkr_sumcheck_sop
(cdense.sumcheck_sop_raw; tests/test_oracle_sop_c.py holds it to the model, the reference's prover and the product oracle) at the
launch geometries tests/product_shapes.py pins.  EVERY sumcheck of every case is compared: coefficients, lengths, challenges and
evaluations, and the inputs are downloaded afterwards and must be unchanged.

  a. the shape matrix: every row of PRODUCT_GEOMETRY, all six structures, factor kinds mixed per (sumcheck, table);
  b. cancellation BETWEEN terms over every block (across terms_total's reduced sums): g on one index of a far block, a leading
     coefficient that cancels in every round, g == 0 in the middle of a batch;
  c. tables that ignore x_1 (round 0's leading coefficients cancel within a term over all blocks) and x_n;
  d. lazy-sum headroom per term: all entries r - 1 and the special byte patterns at chunks of 1024 and 2048, eight terms.

Tables are built with numpy on limb arrays; the oracle is called once per sumcheck and its results are kept."""

import numpy as np
import pytest

from gkr_amd import Context
from oracle import cdense
from oracle.field import P
from oracle.mimc7 import multi_hash
from product_model import SPECIALS
from product_shapes import PRODUCT_GEOMETRY, product_geometry
from resident_tables import Resident, assert_same, structured_tables
from sop_model import STRUCTURES, sop_degree
from sop_terms import BOOKKEEPING

pytestmark = pytest.mark.gpu

MIX = ["random", "specials", "indep_last", "bits", "indep_first", "indep_middle"]
SPECIAL_LIMBS = cdense.to_limbs(SPECIALS + [P - 1])
# every row of PRODUCT_GEOMETRY with a structure of its own, and all six at the smallest row.  (20, 1) is the four-table case;
# n = 23 (256 MiB a table) runs on the two-table structure only
ROW_STRUCTURE = {(16, 1): "AB-AB", (16, 20): "5AB+7BC+11A", (18, 5): "AB-C", (19, 3): "AB-AC", (20, 1): "ABC-AD", (20, 4): "5AB+7BC+11A",
                 (23, 1): "AA+3B"}
MATRIX = [(n, batch, ROW_STRUCTURE[(n, batch)]) for (n, batch) in PRODUCT_GEOMETRY] + \
         [(16, 1, s[0]) for s in STRUCTURES if s[0] != ROW_STRUCTURE[(16, 1)]]


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _structure(name):
    return next(s for s in STRUCTURES if s[0] == name)


def _assert_geometry(n, batch):
    assert tuple(product_geometry(n, batch)[:2]) == PRODUCT_GEOMETRY[(n, batch)], (n, batch)


def _kinds(n, batch, M):
    return [[MIX[(n + 2 * b + 5 * m + M) % len(MIX)] for m in range(M)] for b in range(batch)]


def _matrix_tables(n, batch, name):
    M = _structure(name)[1]
    return structured_tables(_kinds(n, batch, M), n, 9100 + 97 * n + 7 * len(name) + batch, SPECIAL_LIMBS)


_oracle_cache = {}


def _oracle(key, T, terms):
    """cdense.sumcheck_sop_raw per sumcheck of T (batch, M, 2^n, 4), stacked as the device returns them; computed once per key.
    T may be a function that builds the tables (not called when the key is known)."""
    if key not in _oracle_cache:
        T = T() if callable(T) else T
        batch, M, size = T.shape[:3]
        n = size.bit_length() - 1
        outs = [cdense.sumcheck_sop_raw(T[b], n, M, terms) for b in range(batch)]
        _oracle_cache[key] = tuple(np.stack([o[k] for o in outs]) for k in range(4))
    return _oracle_cache[key]


def _run(ctx, T, terms, want, what):
    batch, M, size = T.shape[:3]
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_sop_batch_device(dev.d, size.bit_length() - 1, M, terms, batch)
        dev.assert_unchanged(what)
    assert_same(got, want, what)


# ---- a. the shape matrix ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,name", MATRIX)
def test_shape_matrix_matches_the_c_oracle(ctx, n, batch, name):
    _assert_geometry(n, batch)
    terms = _structure(name)[2]
    T = _matrix_tables(n, batch, name)
    _run(ctx, T, terms, _oracle((n, batch, name), T, terms), (n, batch, name))


def test_the_shape_matrix_covers_every_structure_and_reaches_short_vectors():
    """(oracle only) every row of the geometry table and every structure is in the matrix; outside A B - A B (all [0]) a vector
    shorter than D + 1 occurs in round 0, in a round strictly between the first and the last, and in the last round; and
    full-length vectors occur in all three places too."""
    assert {(n, b) for n, b, _ in MATRIX} == set(PRODUCT_GEOMETRY) and {s for _, _, s in MATRIX} == {s[0] for s in STRUCTURES}
    short, full = set(), set()
    for n, batch, name in MATRIX:
        terms = _structure(name)[2]
        C, L, R, E = _oracle((n, batch, name), lambda: _matrix_tables(n, batch, name), terms)
        D = sop_degree(terms)
        if name == "AB-AB":
            assert (L == 1).all() and not C.any()
            continue
        for where, part in (("first", L[:, 0]), ("middle", L[:, 1:-1]), ("last", L[:, -1])):
            short |= {where} if (part < D + 1).any() else set()
            full |= {where} if (part == D + 1).any() else set()
    assert short == full == {"first", "middle", "last"}, (short, full)


# ---- b. cancellation between terms over every block -----------------------------------------------------------------------------------------
ZERO_R = None


def _assert_all_zero(C, L, R, what):
    global ZERO_R
    if ZERO_R is None:
        ZERO_R = cdense.to_limbs([multi_hash([0], 0)])[0]
    assert (L == 1).all() and not C.any() and (R == ZERO_R).all(), what


def _bump(entry):
    """A canonical value that differs from `entry` (cdense.fill_table's values are below 2^253)."""
    out = entry.copy()
    out[0] ^= np.uint64(1)
    return out


def test_terms_cancel_on_all_but_one_index_of_a_far_block_of_2048(ctx):
    """n = 20, batch 1, A B - A C (2048 blocks of 256).  First C = B: every block's partials of the two terms cancel after the
    terms' reductions, every vector is [0] and r = multi_hash([0], 0).  Then ONE entry of C, in block 1500's upper-half entries,
    differs: g = A (B - C) lives on one index of the upper half, so round 0's constant coefficient is zero and nothing else is."""
    n = 20
    _assert_geometry(n, 1)
    _, M, terms = _structure("AB-AC")
    h = 1 << (n - 1)
    index = h + 256 * 1500 + 77
    T = cdense.fill_table(M << n, 2021).reshape(1, M, 1 << n, 4)
    T[0, 2] = T[0, 1]
    with Resident(ctx, T) as dev:
        got = ctx.sumcheck_sop_batch_device(dev.d, n, M, terms, 1)
        want = _oracle(("cancel", n, "all"), dev.T, terms)
        _assert_all_zero(want[0], want[1], want[2], "oracle")
        assert_same(got, want, ("A B - A C with C = B", n))
        dev.set_entry((2 << n) + index, _bump(dev.T[0, 2, index]))
        got = ctx.sumcheck_sop_batch_device(dev.d, n, M, terms, 1)
        dev.assert_unchanged("one index")
        want = _oracle(("cancel", n, "one"), dev.T, terms)
        assert want[0][0, 0, :2].any() and not want[0][0, 0, 2].any() and want[0][0, 1:, 2].any(), "oracle"   # g(0, .) == 0
        assert_same(got, want, ("A B - A C with C = B but for one entry", n))


def test_terms_cancel_in_the_middle_sumchecks_of_103_blocks(ctx):
    """n = 16, batch 20, A B - A C (103 blocks of chunk 512, 64 of them with entries).  Odd sumchecks: C = B, all [0] with
    r = multi_hash([0], 0); sumchecks 0, 4, ..: C random, every vector has full length; sumchecks 2, 6, ..: C = B but for one entry
    in the upper-half entries of block 62 or 63, the last two that work."""
    n, batch = 16, 20
    _assert_geometry(n, batch)
    _, M, terms = _structure("AB-AC")
    h = 1 << (n - 1)
    T = cdense.fill_table((batch * M) << n, 1621).reshape(batch, M, 1 << n, 4)
    for b in range(batch):
        if b % 4:
            T[b, 2] = T[b, 1]
        if b % 4 == 2:
            index = h + 512 * (62 + (b // 4) % 2) + 77 + b
            T[b, 2, index] = _bump(T[b, 2, index])
    want = _oracle(("cancel", n, batch), T, terms)
    for b in range(batch):
        if b % 2:
            _assert_all_zero(want[0][b], want[1][b], want[2][b], ("oracle", b))
        elif b % 4 == 0:
            assert (want[1][b] == 3).all(), ("oracle", b)
        else:
            assert want[0][b, 0, :2].any() and not want[0][b, 0, 2].any(), ("oracle", b)                # g(0, .) == 0
    _run(ctx, T, terms, want, ("A B - A C, zero in the middle", n, batch))


@pytest.mark.parametrize("n,batch", [(16, 20), (20, 1)])
def test_the_leading_coefficient_cancels_between_terms_in_every_round(ctx, n, batch):
    """A B C - A B D with D = C + k (a k per sumcheck): the two terms' degree-3 coefficients cancel in every round, over 103 or 2048
    blocks' partials, the degree-2 ones do not (g = -k A B)."""
    _assert_geometry(n, batch)
    terms = [(1, (0, 1, 2)), (P - 1, (0, 1, 3))]
    T = cdense.fill_table((batch * 4) << n, 2300 + n).reshape(batch, 4, 1 << n, 4)
    for b in range(batch):
        k = 0x1234567 + b                                             # (entries below 2^253 plus k: canonical, no carry out of limb 0 ...
        T[b, 3] = T[b, 2]
        T[b, 3, :, 0] = (T[b, 2, :, 0] & np.uint64((1 << 63) - 1)) + np.uint64(k)   # ... with limb 0's top bit cleared in both)
        T[b, 2, :, 0] &= np.uint64((1 << 63) - 1)
    want = _oracle(("ABC-ABD", n, batch), T, terms)
    assert (want[1] == 3).all() and not want[0][:, :, 0].any(), "oracle"
    _run(ctx, T, terms, want, ("A B C - A B D", n, batch))


# ---- c. tables that ignore x_1, and x_n -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,name", [(16, "ABC-AD"), (20, "AB-C")])
def test_tables_that_ignore_the_first_and_the_last_variable(ctx, n, name):
    """batch 1.  A and B ignore x_1 (T[h:] = T[:h]): in round 0 the term A B .. loses two degrees, its leading coefficients being
    sums over 128 or 2048 blocks' partials that cancel exactly, and the vector has two entries (A B C - A D and A B - C are both
    linear in x_1 then).  B ignores x_n as well, which shortens the last round's vector by one."""
    _assert_geometry(n, 1)
    _, M, terms = _structure(name)
    D, h = sop_degree(terms), 1 << (n - 1)
    T = cdense.fill_table(M << n, 3400 + n).reshape(1, M, 1 << n, 4)
    T[0, 1, 1::2] = T[0, 1, 0::2]
    for m in (0, 1):
        T[0, m, h:] = T[0, m, :h]
    want = _oracle(("indep", n, name), T, terms)
    assert want[1][0, 0] == 2 and want[1][0, -1] == D and (want[1][0, 1:-1] == D + 1).all(), ("oracle", want[1])
    _run(ctx, T, terms, want, ("A and B ignore x_1, B ignores x_n", n, name))


# ---- d. lazy-sum headroom per term ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch,name,kinds", [(20, 4, "ABC-AD", ("all_max", "specials", "all_max", "specials")),
                                                (23, 1, "AA+3B", ("all_max",)), (23, 1, "AA+3B", ("specials",))])
def test_largest_entries_at_four_and_eight_pairs_per_thread(ctx, n, batch, name, kinds):
    """Every entry r - 1 (the largest products a lane can add: differences are 0, values (r - 1)^2) and the special byte patterns,
    where a thread adds the most products into one lazy sum per term and value: chunk 1024 at (20, 4) -- 4 unreduced products per
    lane -- and chunk 2048 at (23, 1) -- 8 per lane -- against the 2^36 a Lazy17 takes (csrc/fr32.h; the blocks' Acc<9> partials take
    2^32 elements and get 256, the round kernel's Acc<10> gets 512 or 2048 of those).  Sumcheck b's tables are all of kinds[b]; at
    (20, 4) sumchecks 2 and 3 have the first table random, so that not every difference is zero."""
    _assert_geometry(n, batch)
    _, M, terms = _structure(name)
    rows = [[("random" if (b >= 2 and m == 0) else kinds[b]) for m in range(M)] for b in range(batch)]
    T = structured_tables(rows, n, 4500 + n, SPECIAL_LIMBS)
    want = _oracle(("headroom", n, batch, kinds), T, terms)
    _run(ctx, T, terms, want, ("largest entries", n, batch, kinds))


def test_eight_terms_over_eight_tables_at_chunk_512(ctx):
    """n = 16, batch 20, the eight-term list (degrees 1 .. 3, a zero coefficient, r - 1, r - 2 and a 241-bit one): eight partials
    per block, 2 products per lane and term.  Sumcheck b: every table r - 1 (b = 0 mod 3), the special patterns (1 mod 3), kinds
    mixed per table (2 mod 3)."""
    n, batch = 16, 20
    _assert_geometry(n, batch)
    M, terms = BOOKKEEPING["eight terms over eight tables"]
    rows = [[("all_max", "specials", MIX[(b + 5 * m) % len(MIX)])[b % 3] for m in range(M)] for b in range(batch)]
    T = structured_tables(rows, n, 4600, SPECIAL_LIMBS)
    want = _oracle(("eight terms", n, batch), T, terms)
    _run(ctx, T, terms, want, ("eight terms over eight tables", n, batch))

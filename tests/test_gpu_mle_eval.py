"""gkr_mle_eval_batch_device (csrc/kernels_mle_eval.hip) against a fold on Python integers (gkr_amd.verifier.mle_eval): both
kernels -- one block per table below n = 11 and by default below kMleEvalMfmaMinN, the streaming matrix-core form from there --
forced with the option mle_eval_mfma_min_n wherever both apply, over tables of random values, of p - 1 throughout and of the byte
patterns that sit on the matrix-core fold's sign and carry boundaries, at points with coordinates 0, 1, p - 1 and random."""

import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from gkr_amd.verifier import mle_eval
from verify_sweeps import R_LIMBS

pytestmark = pytest.mark.gpu
MFMA_VALID_N = 11          # kernels.h kMleEvalMfmaValidN
SPECIALS = [0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
            int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
            int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128]   # test_mle_extreme_byte_patterns_match_oracle's


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _table(kind, n, rng):
    if kind == "all_max":
        return [P - 1] * (1 << n)
    if kind == "specials":
        return [SPECIALS[rng.randrange(len(SPECIALS))] for _ in range(1 << n)]
    if kind == "mixed":
        return [SPECIALS[rng.randrange(len(SPECIALS))] if rng.random() < 0.5 else rng.randrange(P) for _ in range(1 << n)]
    return [rng.randrange(P) for _ in range(1 << n)]


def _point(n, b, rng):
    """Coordinates 0, 1 and p - 1 at places that move with the table's index, random ones between them."""
    fixed = [0, 1, P - 1]
    return [fixed[(b + j) % 7] if (b + j) % 7 < 3 else rng.randrange(P) for j in range(n)]


KINDS = ["random", "all_max", "specials", "mixed"]
_cache = {}


def _inputs(n, batch):
    """Tables, points and the reference values of a shape, computed once (distinct point per table; every kind of table)."""
    if (n, batch) not in _cache:
        rng = random.Random(9000 + 31 * n + batch)
        kinds = [KINDS[(b + batch) % 4] for b in range(batch)]
        tables = [_table(k, n, rng) for k in kinds]
        points = [_point(n, b + batch, rng) for b in range(batch)]
        if batch > 1:
            points[1] = [rng.randrange(P) for _ in range(n)]                   # one point without a special coordinate
        for b in range(batch):                                                 # at n = 1 the special coordinates come round again:
            while points[b] in points[:b]:                                     # a repeated point gives way to a random one
                points[b] = [rng.randrange(P) for _ in range(n)]
        assert len({tuple(p) for p in points}) == batch
        want = [mle_eval(t, p) for t, p in zip(tables, points)]
        T = np.concatenate([to_limbs(t) for t in tables])
        Pt = np.stack([to_limbs(p) for p in points])
        _cache[(n, batch)] = (T, Pt, want)
    return _cache[(n, batch)]


def _forms(n):
    """The option values to run a shape under: the default, and from n = 11 on both kernels by force."""
    return [0] if n < MFMA_VALID_N else [0, MFMA_VALID_N, 31]


@pytest.mark.parametrize("batch", [1, 3, 9])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 10, 11, 12, 13, 14])
def test_evaluation_matches_the_integer_fold(ctx, n, batch):
    T, Pt, want = _inputs(n, batch)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        got = {}
        for form in _forms(n):
            ctx.set_option("mle_eval_mfma_min_n", form)
            got[form] = from_limbs(ctx.mle_eval_batch_device(d, n, batch, Pt))
            assert got[form] == want, (n, batch, form)
        assert np.array_equal(ctx.download(d, T.shape), T)                     # the tables are not modified
    finally:
        ctx.set_option("mle_eval_mfma_min_n", 0)
        ctx.free(d)


@pytest.mark.parametrize("n", [3, 11, 13])
def test_every_kind_of_table_alone(ctx, n):
    """batch = 1 with each kind of table (the batch matrix above gives a lone table one kind only), in both forms where both apply."""
    rng = random.Random(9500 + n)
    for kind in KINDS:
        t, p = _table(kind, n, rng), _point(n, rng.randrange(7), rng)
        T, want = to_limbs(t), mle_eval(t, p)
        d = ctx.alloc(T.nbytes)
        try:
            ctx.upload(d, T)
            for form in _forms(n):
                ctx.set_option("mle_eval_mfma_min_n", form)
                assert from_limbs(ctx.mle_eval_batch_device(d, n, 1, to_limbs(p)[None])) == [want], (kind, form)
        finally:
            ctx.set_option("mle_eval_mfma_min_n", 0)
            ctx.free(d)


def test_corner_points_select_single_entries(ctx):
    """A point of zeros and ones is an index: the value is that entry -- first and last of the table and of a leading stream."""
    n = 12
    rng = random.Random(77)
    t = [rng.randrange(P) for _ in range(1 << n)]
    T = to_limbs(t)
    idx = [0, (1 << n) - 1, 1 << (n - 5), (1 << (n - 5)) - 1, 0b101010101010, 63, 64]
    Pt = np.stack([to_limbs([(i >> (n - 1 - j)) & 1 for j in range(n)]) for i in idx])
    d = ctx.alloc(T.nbytes * len(idx))
    try:
        ctx.upload(d, np.concatenate([T] * len(idx)))
        for form in _forms(n):
            ctx.set_option("mle_eval_mfma_min_n", form)
            assert from_limbs(ctx.mle_eval_batch_device(d, n, len(idx), Pt)) == [t[i] for i in idx], form
    finally:
        ctx.set_option("mle_eval_mfma_min_n", 0)
        ctx.free(d)


def test_a_non_canonical_point_is_refused(ctx):
    n, batch = 5, 3
    T, Pt, _ = _inputs(n, batch)
    d = ctx.alloc(T.nbytes)
    try:
        ctx.upload(d, T)
        for at in ((0, 0), (1, 2), (2, n - 1)):
            bad = Pt.copy()
            bad[at] = R_LIMBS
            with pytest.raises(GkrError) as e:
                ctx.mle_eval_batch_device(d, n, batch, bad)
            assert e.value.status == N.GKR_ERR_NON_CANONICAL
    finally:
        ctx.free(d)

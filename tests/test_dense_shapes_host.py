"""tests/dense_shapes.py against hand-worked values and against the library's own arithmetic (gkr_selftest_layer_dense_geometry: host
logic only, no device): every row the GPU cases of tests/test_gpu_layer_dense.py pin, and the self-test over every round of every
shape against a restatement of the launch rules in Python integers."""

import ctypes

import numpy as np
import pytest

import dense_shapes as ds
from gkr_amd import _native as N
from product_shapes import product_geometry


def _ceil(a, b):
    return -(-a // b)


def _model(k, log_p, rnd):
    """The launch rules of kernels_layer_dense.hip and launch_predicate_sorted, restated."""
    cells = 1 << (2 * k - log_p)
    h = cells >> (rnd + 1)
    g = dict.fromkeys(ds.FIELDS, 0)
    if log_p == 0 and rnd < k:
        hb = h >> k
        col_blocks = _ceil(1 << k, 256)
        chunks = max(1, min(1024 // col_blocks, hb))
        rows = _ceil(hb, chunks)
        chunks = _ceil(hb, rows)
        g.update(col_blocks=col_blocks, chunks=chunks, rows_per_chunk=rows, partials=2 * col_blocks * chunks)
    g.update(phase=0 if rnd < k else 1, round_blocks=min(max(_ceil(h, 256), 1), 2048), fold_blocks=min(max(_ceil(h, 256), 1), 4097),
             scan_blocks=_ceil(2 * cells, 2048), sum_blocks=min(max(_ceil(2 * cells, 256), 1), 8192))
    return g


def test_device_transcript_rows():
    # k = 8: 256 columns = 1 column block; hb = 128 row pairs <= 1024 chunks -> 128 chunks of 1 row; 2 tables -> 256 partials = 4 x 64;
    #        unfused: 2^15 pairs / 256 = 128 blocks
    assert ds.device_row(8) == (((1, 128, 1, 256), 128), (4, 1))
    # k = 9: 512 columns = 2 blocks; 1024 / 2 = 512 chunks, cut to hb = 256; 2 * 2 * 256 = 1024 partials; 2^17 / 256 = 512 blocks
    assert ds.device_row(9) == (((2, 256, 1, 1024), 512), (16, 1))
    # k = 10: 4 column blocks; 1024 / 4 = 256 chunks < hb = 512 -> 2 rows per chunk; 2 * 4 * 256 = 2048; 2^19 / 256 = 2048 blocks
    assert ds.device_row(10) == (((4, 256, 2, 2048), 2048), (32, 1))
    # k = 11: 8 column blocks; 128 chunks, hb = 1024 -> 8 rows per chunk; 2 * 8 * 128 = 2048; 2^21 / 256 = 8192 -> cap 2048, 4 trips
    assert ds.device_row(11) == (((8, 128, 8, 2048), 2048), (32, 4))
    for k in ds.DEVICE_ROUND0:
        assert ds.device_row(k) == (ds.DEVICE_ROUND0[k], ds.DEVICE_TRIPS[k]), k
    # the fused round writes at most kMaxLayerBlocks partials at any width and round, and every chunk has a row
    for k in range(1, 15):
        for rnd in range(k):
            g = ds.dense_geometry(k, 0, rnd)
            assert 2 <= g["partials"] <= 2048 and g["chunks"] * g["rows_per_chunk"] >= 1 << (k - 1 - rnd) > (g["chunks"] - 1) * g["rows_per_chunk"], (k, rnd)
    # the c-phase of k = 11 starts with a fold of 2^12 entries (2^11 pairs, 8 blocks) into the row of 2^11
    assert ds.pick(ds.dense_geometry(11, 0, 10), "phase", "fold_blocks") == (0, 8) and ds.dense_geometry(11, 0, 11)["phase"] == 1


def test_session_rows():
    hand = {
        (5, 1): (2, 1, 1, 2, 1, 1),            # 2^9 pairs / 256
        (8, 1): (128, 1, 2, 128, 1, 1),        # 2^15 / 256 = 128 = 2 x 64
        (8, 4): (32, 1, 1, 32, 1, 1),          # 2^13 / 256
        (8, 256): (1, 1, 1, 1, 1, 1),          # 2^7 pairs
        (10, 1024): (2, 1, 1, 2, 1, 2),        # 2^9 pairs / 256; Wb: 512 pairs
        (10, 2): (1024, 1, 16, 1024, 1, 2),    # 2^18 / 256; Wb: 512 pairs = 2 stripes of 256
        (11, 2): (2048, 2, 32, 4096, 1, 4),    # 2^20 / 256 = 4096 -> 2048 x 2 trips; fold 4096 <= 4097
        (11, 1): (2048, 4, 32, 4097, 2, 4),    # 2^21 / 256 = 8192 -> 2048 x 4; fold 4097 x 2
    }
    assert hand == ds.SESSION_ROUND0
    for (k, shards), want in hand.items():
        assert ds.session_row(k, shards) == want, (k, shards)
    # a shard's phase changes after k_next rounds whatever the split
    assert [ds.dense_geometry(8, 2, r)["phase"] for r in (0, 7, 8, 13)] == [0, 0, 1, 1]


def test_predicate_rows():
    hand = {
        (1, 0): (1, 1, 1, 1), (5, 0): (1, 1, 8, 1), (6, 0): (4, 1, 32, 1), (10, 0): (1024, 1, 8192, 1), (11, 0): (4096, 4, 8192, 4),
        (8, 1): (32, 1, 256, 1), (8, 3): (8, 1, 64, 1), (8, 8): (1, 1, 2, 1), (10, 2): (256, 1, 2048, 1),
    }
    assert hand == ds.PREDICATE
    for (k, log_p), want in hand.items():
        assert ds.predicate_row(k, log_p) == want, (k, log_p)


def test_plain_session_rows():
    # mle_blocks_per_table(2^(n-1), 1): at least 2048 blocks wanted, never more than one per 256 items, at most 2048
    assert ds.MLE_SESSION_ROUND0 == {15: 64, 17: 256, 20: 2048}
    for n, want in ds.MLE_SESSION_ROUND0.items():
        assert product_geometry(n, 1)[0] == (want, 256), n


def test_selftest_agrees_with_the_launch_rules_at_every_round():
    for k in range(1, 15):
        for log_p in range(k + 1):
            for rnd in range(2 * k - log_p):
                assert ds.dense_geometry(k, log_p, rnd) == _model(k, log_p, rnd), (k, log_p, rnd)


def test_selftest_refusals():
    lib = N.lib()
    out = np.full(8, 7, dtype=np.uint32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for k, log_p, rnd in ((0, 0, 0), (15, 0, 0), (8, -1, 0), (8, 9, 0), (8, 0, -1), (8, 0, 16), (8, 2, 14), (1, 1, 1)):
        assert lib.gkr_selftest_layer_dense_geometry(k, log_p, rnd, p) == N.GKR_ERR_INVALID, (k, log_p, rnd)
    assert lib.gkr_selftest_layer_dense_geometry(8, 0, 0, None) == N.GKR_ERR_INVALID
    assert (out == 7).all()
    assert lib.gkr_selftest_layer_dense_geometry(14, 0, 27, p) == 0 and lib.gkr_selftest_layer_dense_geometry(1, 1, 0, p) == 0


def test_predicates_devtest_refuses_a_missing_context():
    """gkr_devtest_predicates builds on the device: without a context it returns GKR_ERR_INVALID before it reads an argument (its other
    refusals need a device: tests/test_gpu_layer_dense.py)."""
    assert "gkr_devtest_predicates" in N.SYMBOLS and "gkr_selftest_layer_dense_geometry" in N.SYMBOLS
    A = np.full((4, 4), 7, dtype=np.uint64)
    gt, l, r = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    z = np.zeros((2, 4), dtype=np.uint64)
    args = [a.ctypes.data_as(ctypes.c_void_p) for a in (gt, l, r, z)]
    assert N.lib().gkr_devtest_predicates(None, 2, 1, *args, 0, 0, A.ctypes.data_as(ctypes.c_void_p), A.ctypes.data_as(ctypes.c_void_p)) == N.GKR_ERR_INVALID
    assert (A == 7).all()

"""The launch geometry of the dense layer forms (gkr_selftest_layer_dense_geometry) and the shapes the tests pin:
tests/test_dense_shapes_host.py holds the tables below to hand-worked values and to the library, tests/test_gpu_layer_dense.py
asserts a case's row before it runs the case.  A retuned constant has to fail a pin, not leave the GPU cases of these shapes
running something other than what their names say.

The arithmetic behind the numbers (N = 2^(2k - log_p) cells per table, h = N / 2 pairs in round 0, blocks of 256 threads):
  fused b-phase round   col_blocks = ceil(2^k / 256); chunks = min(1024 / col_blocks, hb) with hb = 2^(k-1) row pairs;
                        rows_per_chunk = ceil(hb / chunks); partials = 2 * col_blocks * chunks
  k_layer_round         min(ceil(h / 256), 2048) blocks (kMaxLayerBlocks, the size of the partials buffer)
  k_layer_fold          min(ceil(h / 256), 4097) blocks
  scan                  ceil(2 N / 2048) blocks; k_scan_sums walks them 1024 at a time
  k_pred_sum            min(ceil(2 N / 256), 8192) blocks
"""

import ctypes

import numpy as np

from gkr_amd import _native as N

FIELDS = ("col_blocks", "chunks", "rows_per_chunk", "partials", "phase", "round_blocks", "fold_blocks", "scan_blocks", "sum_blocks")


def dense_geometry(k, log_p=0, rnd=0):
    """gkr_selftest_layer_dense_geometry as a dict over FIELDS (phase: 0 while a b variable is bound, 1 after)."""
    out = np.zeros(8, dtype=np.uint32)
    rc = N.lib().gkr_selftest_layer_dense_geometry(k, log_p, rnd, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (k, log_p, rnd, rc)
    o = [int(x) for x in out]
    return dict(zip(FIELDS, o[:4] + [o[4] >> 31, o[4] & 0x7FFFFFFF] + o[5:]))


def pick(geometry, *names):
    return tuple(geometry[n] for n in names)


# ---- the device transcript, one layer: k_next -> round 0 as (col_blocks, chunks, rows_per_chunk, partials) of the fused round and
# the blocks of the unfused one (layer_no_fused), with the pairs of that round for the trips of its grid-stride loop
DEVICE_ROUND0 = {
    8: ((1, 128, 1, 256), 128),       # 256 columns: one full column block; 128 row pairs, one per chunk
    9: ((2, 256, 1, 1024), 512),      # two column blocks; 1024 / 2 = 512 chunks cut to hb = 256
    10: ((4, 256, 2, 2048), 2048),    # 512 row pairs over 256 chunks: 2 rows per chunk; 2048 partials = kMaxLayerBlocks already here
    11: ((8, 128, 8, 2048), 2048),    # 1024 row pairs over 128 chunks: 8 rows per chunk; unfused: 2^21 pairs over the 2048-block cap, 4 trips
}
# k_next -> trips of k_layer_round_hash's 64-lane loop over round 0's partials, and of the unfused k_layer_round over its pairs
DEVICE_TRIPS = {8: (4, 1), 9: (16, 1), 10: (32, 1), 11: (32, 4)}

# ---- layer sessions: (k_next, shards) -> round 0 as (blocks of k_layer_round, trips of its grid-stride loop, trips of the reduce's
# 64-lane loop, blocks of k_layer_fold, trips of its loop, stripes of k_fold_small over Wb's 2^(k-1) pairs)
SESSION_ROUND0 = {
    (5, 1): (2, 1, 1, 2, 1, 1),                 # 2^9 pairs: 2 blocks
    (8, 1): (128, 1, 2, 128, 1, 1),             # 2^15 pairs: 128 partials, the reduce's second trip
    (8, 4): (32, 1, 1, 32, 1, 1),               # kc = 6: 2^13 pairs per shard
    (8, 256): (1, 1, 1, 1, 1, 1),               # kc = 0: 2^7 pairs per shard, ONE block
    (10, 1024): (2, 1, 1, 2, 1, 2),             # kc = 0 with two blocks: the smallest such split
    (10, 2): (1024, 1, 16, 1024, 1, 2),         # Wb folds 512 pairs: k_fold_small's second stripe
    (11, 2): (2048, 2, 32, 4096, 1, 4),         # 2^20 pairs: the 2048-block cap, two trips
    (11, 1): (2048, 4, 32, 4097, 2, 4),         # 2^21 pairs: k_layer_fold's 4097-block cap, two trips
}

# ---- predicate tables: (k_next, log_p) -> (scan blocks, trips of k_scan_sums, blocks of k_pred_sum, trips of its loop)
PREDICATE = {
    (1, 0): (1, 1, 1, 1),               # 8 counters
    (5, 0): (1, 1, 8, 1),               # 2 N = 2048: one full scan block
    (6, 0): (4, 1, 32, 1),
    (10, 0): (1024, 1, 8192, 1),        # one full trip of k_scan_sums; k_pred_sum at its cap, one trip
    (11, 0): (4096, 4, 8192, 4),        # four trips with carry; k_pred_sum's (and k_predicate_normalise's) grid-stride trips
    (8, 1): (32, 1, 256, 1),
    (8, 3): (8, 1, 64, 1),
    (8, 8): (1, 1, 2, 1),               # 2 N = 512
    (10, 2): (256, 1, 2048, 1),
}

# ---- plain sessions: local variables of a shard -> blocks of the first round's sum kernel (gkr_selftest_product_geometry(n, 1), round 0)
MLE_SESSION_ROUND0 = {15: 64, 17: 256, 20: 2048}


def device_row(k):
    g = dense_geometry(k, 0, 0)
    pairs = 1 << (2 * k - 1)
    blocks = g["round_blocks"]
    return (pick(g, "col_blocks", "chunks", "rows_per_chunk", "partials"), blocks), ((g["partials"] + 63) // 64, -(-pairs // (256 * blocks)))


def session_row(k, shards):
    log_p = shards.bit_length() - 1
    g = dense_geometry(k, log_p, 0)
    pairs = 1 << (2 * k - log_p - 1)
    rb, fb = g["round_blocks"], g["fold_blocks"]
    return rb, -(-pairs // (256 * rb)), (rb + 63) // 64, fb, -(-pairs // (256 * fb)), -(-(1 << (k - 1)) // 256)


def predicate_row(k, log_p):
    g = dense_geometry(k, log_p, 0)
    cells = 2 << (2 * k - log_p)
    return g["scan_blocks"], (g["scan_blocks"] + 1023) // 1024, g["sum_blocks"], -(-cells // (256 * g["sum_blocks"]))

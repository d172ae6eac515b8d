"""The launch geometry of the product sumcheck's passes (gkr_selftest_product_geometry) and the shapes the tests pin:
tests/test_host_library.py holds the values, tests/test_gpu_product_sizes.py runs the shapes for what they reach."""

import ctypes

import numpy as np

from gkr_amd import _native as N


def product_geometry(n, batch):
    """[(nblk, chunk)] per round of gkr_sumcheck_product_batch_device's passes."""
    nblk, chunk = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    rc = N.lib().gkr_selftest_product_geometry(n, batch, nblk.ctypes.data_as(ctypes.c_void_p), chunk.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, (n, batch, rc)
    return [(int(a), int(b)) for a, b in zip(nblk, chunk)]


# (n, batch) -> the value pass of round 0 and the fold pass of round 1, as (blocks per sumcheck, chunk): what
# mle_blocks_per_table gives with the default items_per_block.  A retuned geometry has to fail the pin, not leave the GPU
# tests of these shapes running something else.
PRODUCT_GEOMETRY = {
    (16, 1): ((128, 256), (64, 256)),        # two full trips of the round kernel's wave loop
    (16, 20): ((103, 512), (64, 256)),       # a block count that is no power of two, 39 empty blocks, chunk 512
    (18, 5): ((410, 512), (256, 256)),       # 154 empty blocks, 7 trips
    (19, 3): ((683, 512), (512, 256)),       # 171 empty blocks; round 1's count differs from round 0's
    (20, 1): ((2048, 256), (1024, 256)),     # the cap, 32 trips
    (20, 4): ((512, 1024), (512, 512)),      # the benchmark's per-sumcheck geometry; the fold pass with 2 pairs per thread
    (23, 1): ((2048, 2048), (2048, 1024)),   # 8 pairs per thread
}

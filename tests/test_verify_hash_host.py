"""The device hashing of the verifier's round vectors, the part of its surface that needs no device (include/gkr_amd.h,
gkr_mimc7_multi_hash_device; csrc/options.h, verify_device_hash_min): the symbol, the argument checks that run before a device is
touched, and the option's row in the one table."""

import ctypes
import os
import re

import numpy as np

from gkr_amd import _native as N
from gkr_amd.prover import Context, options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gkr_mimc7_multi_hash_device"


def test_the_symbol_is_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    assert NAME in N.SYMBOLS
    assert re.search(r"\bint\s+%s\(gkr_ctx \*ctx, const gkr_fr \*rows, const uint32_t \*len, size_t n, gkr_fr \*out, uint32_t \*valid\);" % NAME,
                     header)
    assert hasattr(lib, NAME)
    assert callable(Context.multi_hash_batch)
    assert '"verify_hash"' in header                          # the profile row is named where gkr_ctx_profile is described


def test_null_arguments_and_no_rows_are_invalid():
    """No context exists here (no device): every one of these is decided before a device is touched."""
    fn = getattr(N.lib(), NAME)
    rows = np.zeros((2, 3, 4), dtype=np.uint64)
    lens = np.ones(2, dtype=np.uint32)
    out = np.full((2, 4), 7, dtype=np.uint64)
    valid = np.full(2, 7, dtype=np.uint32)
    word = ctypes.c_uint64(0)
    fake = ctypes.c_void_p(ctypes.addressof(word))            # stands for a context that is never dereferenced
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_size_t(2)
    assert fn(None, p(rows), p(lens), n, p(out), p(valid)) == N.GKR_ERR_INVALID                    # NULL ctx
    assert fn(fake, None, p(lens), n, p(out), p(valid)) == N.GKR_ERR_INVALID
    assert fn(fake, p(rows), None, n, p(out), p(valid)) == N.GKR_ERR_INVALID
    assert fn(fake, p(rows), p(lens), n, None, p(valid)) == N.GKR_ERR_INVALID
    assert fn(fake, p(rows), p(lens), n, p(out), None) == N.GKR_ERR_INVALID
    assert fn(fake, p(rows), p(lens), ctypes.c_size_t(0), p(out), p(valid)) == N.GKR_ERR_INVALID   # n = 0
    assert (out == 7).all() and (valid == 7).all()            # nothing was written


def test_the_threshold_option_is_in_the_table():
    table = {name: (env, doc) for name, env, doc in options()}
    assert "verify_device_hash_min" in table
    env, doc = table["verify_device_hash_min"]
    assert env == "GKR_VERIFY_DEVICE_HASH_MIN" and "gkr_verify_prepared" in doc
    assert "-1" in doc and "never" in doc                     # the parent commit's path stays reachable, and the text says how

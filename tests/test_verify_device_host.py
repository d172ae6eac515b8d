"""The device verifier's surface that needs no device (include/gkr_amd.h, "verifier on the device"): the four symbols, the
argument checks that run before a device is touched, and the workspace option."""

import ctypes
import mmap
import os
import re

import numpy as np
import pytest

from gkr_amd import GKRCircuit, Layer, _native as N
from gkr_amd.prover import Context, options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_verify_prepare", "gkr_verify_prepared", "gkr_verify_circuit_free", "gkr_verify_device"]


def _circuit(ks, seed=0):
    rng = np.random.default_rng(seed)
    return GKRCircuit([Layer(ks[i], rng.integers(0, 2, 1 << ks[i]).tolist(), rng.integers(0, 1 << ks[i + 1], 1 << ks[i]).tolist(),
                             rng.integers(0, 1 << ks[i + 1], 1 << ks[i]).tolist()) for i in range(len(ks) - 1)], ks[-1])


def test_the_four_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
    assert "typedef struct gkr_verify_circuit gkr_verify_circuit;" in header
    assert lib.gkr_verify_circuit_free.restype is None
    import gkr_amd
    from gkr_amd import dropin
    assert "VerifyHandle" in gkr_amd.__all__ and callable(dropin.verify_device)
    assert callable(Context.prepare_verify) and callable(Context.verify_batch)


def test_null_arguments_and_an_empty_batch_are_invalid():
    """No context exists here (no device): every one of these is decided before a device is touched."""
    lib = N.lib()
    desc, alive = Context._circuit_desc(None, _circuit([2, 3, 2]))
    sizes = N.ProofSizes()
    assert lib.gkr_proof_sizes(ctypes.byref(desc), ctypes.byref(sizes)) == 0
    word = ctypes.c_uint64(0)
    buf = N.ProofBuf(*([ctypes.addressof(word)] * 9))
    accept, layer, check = ctypes.c_int(7), ctypes.c_uint32(0), ctypes.c_uint32(0)
    handle = ctypes.c_void_p()
    fake = ctypes.c_void_p(ctypes.addressof(word))            # stands for a context / handle that is never dereferenced
    assert lib.gkr_verify_prepare(None, ctypes.byref(desc), ctypes.byref(handle)) == N.GKR_ERR_INVALID      # NULL ctx
    assert lib.gkr_verify_prepare(fake, None, ctypes.byref(handle)) == N.GKR_ERR_INVALID                    # NULL circuit
    assert lib.gkr_verify_prepare(fake, ctypes.byref(desc), None) == N.GKR_ERR_INVALID                      # NULL out
    assert not handle.value
    args = (ctypes.byref(accept), ctypes.byref(layer), ctypes.byref(check))
    assert lib.gkr_verify_prepared(None, fake, ctypes.byref(buf), ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_prepared(fake, None, ctypes.byref(buf), ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_prepared(fake, fake, None, ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_prepared(fake, fake, ctypes.byref(buf), ctypes.c_int(1), None, args[1], args[2]) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_prepared(fake, fake, ctypes.byref(buf), ctypes.c_int(0), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_prepared(fake, fake, ctypes.byref(buf), ctypes.c_int(-3), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_device(None, ctypes.byref(desc), ctypes.byref(buf), ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_device(fake, None, ctypes.byref(buf), ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_device(fake, ctypes.byref(desc), None, ctypes.c_int(1), *args) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_device(fake, ctypes.byref(desc), ctypes.byref(buf), ctypes.c_int(1), None, args[1], args[2]) == N.GKR_ERR_INVALID
    assert lib.gkr_verify_device(fake, ctypes.byref(desc), ctypes.byref(buf), ctypes.c_int(0), *args) == N.GKR_ERR_INVALID
    assert accept.value == 7                                  # nothing was written


@pytest.mark.parametrize("ks", [[2, 0], [3, 2, 0], [2, 0, 3]])
def test_a_degenerate_k_list_is_refused_without_context_or_proof(ks):
    """k[i] == 0 for some i >= 1: GKR_ERR_DEGENERATE from the circuit alone -- with a NULL context, and with a proof whose every
    array is one page that may not be read (a read ends the process), as gkr_verify is tested in test_dropin_host.py."""
    libc = ctypes.CDLL(None)
    libc.mmap.restype = ctypes.c_void_p
    libc.mmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long]
    libc.munmap.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    page = libc.mmap(None, mmap.PAGESIZE, 0, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)       # PROT_NONE
    assert page and page != ctypes.c_void_p(-1).value
    try:
        lib = N.lib()
        desc, alive = Context._circuit_desc(None, _circuit(ks, seed=len(ks)))
        buf = N.ProofBuf(*([page] * 9))
        accept, layer, check = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        handle = ctypes.c_void_p()
        assert lib.gkr_verify_prepare(None, ctypes.byref(desc), ctypes.byref(handle)) == N.GKR_ERR_DEGENERATE
        assert not handle.value
        rc = lib.gkr_verify_device(None, ctypes.byref(desc), ctypes.byref(buf), ctypes.c_int(1), ctypes.byref(accept), ctypes.byref(layer),
                                   ctypes.byref(check))
        assert rc == N.GKR_ERR_DEGENERATE and accept.value == 0
    finally:
        libc.munmap(page, mmap.PAGESIZE)


def test_k_limits_are_those_of_the_host_verifier():
    lib = N.lib()
    handle = ctypes.c_void_p()
    for ks in ([29, 3], [3, 25]):
        karr = np.asarray(ks, dtype=np.uint32)
        one = (ctypes.c_void_p * 1)(ctypes.addressof(handle))           # never dereferenced: the k list is refused first
        desc = N.CircuitDesc(1, karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), one, one, one)
        assert lib.gkr_verify_prepare(None, ctypes.byref(desc), ctypes.byref(handle)) == N.GKR_ERR_INVALID
    karr = np.asarray([2, 2], dtype=np.uint32)
    for depth in (0, 4097):
        desc = N.CircuitDesc(depth, karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), one, one, one)
        assert lib.gkr_verify_prepare(None, ctypes.byref(desc), ctypes.byref(handle)) == N.GKR_ERR_INVALID


def test_freeing_nothing_is_harmless():
    lib = N.lib()
    lib.gkr_verify_circuit_free(None, None)
    lib.gkr_verify_circuit_free(None, None)


def test_the_workspace_option_is_in_the_table():
    table = {name: (env, doc) for name, env, doc in options()}
    assert "verify_workspace_mb" in table
    env, doc = table["verify_workspace_mb"]
    assert env == "GKR_VERIFY_WORKSPACE_MB" and "gkr_verify_prepared" in doc

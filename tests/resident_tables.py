"""What the exact multi-block GPU tests share (tests/test_gpu_product_sizes.py, test_gpu_sop_sizes.py, test_gpu_zerocheck_sizes.py):
limb arrays held in device memory for the length of a `with`, and the report of the first place where the device's arrays and
the C oracle's differ."""

import ctypes

import numpy as np
import pytest

NAMES = ("coefficients", "lengths", "challenges", "evals", "eq")


def free_bytes():
    import torch
    return torch.cuda.mem_get_info()[0]


class Resident:
    """A limb array in device memory for the length of a `with` (skips when the device has no room for it and the workspace)."""

    def __init__(self, ctx, T):
        self.ctx, self.T = ctx, np.ascontiguousarray(T)

    def __enter__(self):
        if free_bytes() < int(1.75 * self.T.nbytes):
            pytest.skip("not enough free device memory for %d MiB of tables" % (self.T.nbytes >> 20))
        self.d = self.ctx.alloc(self.T.nbytes)
        try:
            self.ctx.upload(self.d, self.T)
        except Exception:
            self.ctx.free(self.d)
            raise
        return self

    def __exit__(self, *a):
        self.ctx.free(self.d)

    def set_entry(self, flat_index, limbs):
        """One entry, in the host copy and on the device."""
        self.T.reshape(-1, 4)[flat_index] = limbs
        self.ctx.upload(ctypes.c_void_p(self.d.value + 32 * flat_index), np.ascontiguousarray(limbs, dtype=np.uint64).reshape(1, 4))

    def assert_unchanged(self, what):
        """The device's copy is still the host's: the call under test did not write its inputs."""
        assert np.array_equal(self.ctx.download(self.d, self.T.shape), self.T), ("the inputs are not modified", what)


def structured_tables(kinds, n, seed, specials):
    """(batch, M, 2^n, 4) limbs for kinds[b][m] in {"random", "specials", "bits", "all_max", "indep_last", "indep_first",
    "indep_middle"}: cdense.fill_table's values with the structured kinds written over them by numpy (no Python integer per entry).
    specials: (k, 4) limbs to draw the "specials" entries from, the last of them the "all_max" value."""
    from oracle import cdense
    batch, M, size, h = len(kinds), len(kinds[0]), 1 << n, 1 << (n - 1)
    T = cdense.fill_table((batch * M) << n, seed).reshape(batch, M, size, 4)
    rng = np.random.default_rng(seed + 1)
    for b, row in enumerate(kinds):
        for m, kind in enumerate(row):
            t = T[b, m]
            if kind == "specials":
                t[:] = specials[rng.integers(0, len(specials), size=size)]
            elif kind == "all_max":
                t[:] = specials[-1]
            elif kind == "bits":
                t[:] = 0
                t[:, 0] = rng.integers(0, 2, size=size, dtype=np.uint64)
            elif kind == "indep_last":
                t[1::2] = t[0::2]
            elif kind == "indep_first":
                t[h:] = t[:h]
            elif kind == "indep_middle":                          # the 0-based variable n // 2, as product_model.factor has it
                v = t.reshape(1 << (n // 2), 2, -1, 4)
                v[:, 1] = v[:, 0]
            else:
                assert kind == "random", kind
    return T


def assert_same(got, want, what):
    """(C, L, R, E[, Q]) of the device against the oracle's; the first differing (sumcheck, round, slot) on a mismatch."""
    assert len(got) == len(want), (what, len(got), len(want))
    for name, g, w in sorted(zip(NAMES, got, want), key=lambda x: x[0] != "lengths"):         # lengths first: the plainest report
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            differ = (g != w) if name == "lengths" else (g != w).any(axis=-1)
            at = tuple(int(x) for x in np.argwhere(differ)[0])               # (sumcheck, round[, slot]), (sumcheck, table) or (sumcheck,)
            pytest.fail("%s: %s differ first at %s: got %s, want %s (%d places in all)" % (what, name, at, g[at], w[at], int(differ.sum())))

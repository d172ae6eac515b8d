"""The library's own report of the plain sumcheck's launch plan (gkr_selftest_mle_plan: host logic from the functions the driver and
its launches call, no device) in the shape tests/mle_shapes.py models it, and the assertion the GPU cases open with."""

import ctypes

import numpy as np

import mle_shapes as ms
from gkr_amd import _native as N

ROW_CAPACITY = (ms.MAX_GROUPS + 1) * 32


def _unpack(rc, header, rows, n_rows):
    assert rc == 0 and n_rows.value <= ROW_CAPACITY, (rc, n_rows.value)
    return [int(x) for x in header], [tuple(int(x) for x in r) for r in rows[:n_rows.value]]


def library_plan(n, batch, threads, options=()):
    """(header, rows) for the option table's defaults with `options` ((name, value) pairs) laid over them: no context, no environment."""
    header = np.zeros(ms.HEADER_WORDS, dtype=np.uint32)
    rows = np.zeros((ROW_CAPACITY, ms.ROW_WORDS), dtype=np.uint32)
    n_rows = ctypes.c_size_t()
    names = (ctypes.c_char_p * max(len(options), 1))(*[k.encode() for k, _ in options])
    values = (ctypes.c_longlong * max(len(options), 1))(*[v for _, v in options])
    rc = N.lib().gkr_selftest_mle_plan(n, batch, threads, ctypes.cast(names, ctypes.c_void_p), ctypes.cast(values, ctypes.c_void_p), len(options),
                                       header.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p), ROW_CAPACITY, ctypes.byref(n_rows))
    return _unpack(rc, header, rows, n_rows)


def context_plan(ctx, n, batch):
    """(header, rows) for the context's options and thread count."""
    header = np.zeros(ms.HEADER_WORDS, dtype=np.uint32)
    rows = np.zeros((ROW_CAPACITY, ms.ROW_WORDS), dtype=np.uint32)
    n_rows = ctypes.c_size_t()
    ctx._check(N.lib().gkr_selftest_mle_plan_ctx(ctx._h, n, batch, header.ctypes.data_as(ctypes.c_void_p), rows.ctypes.data_as(ctypes.c_void_p),
                                                 ROW_CAPACITY, ctypes.byref(n_rows)))
    return _unpack(0, header, rows, n_rows)


def context_options(ctx):
    """The options of the context that the plan reads and that are not 0, as (name, value) pairs."""
    return tuple((k, ctx.get_option(k)) for k in ms.OPTIONS if ctx.get_option(k) != 0)


def assert_plan(ctx, n, batch, options=None, kinds=None, group=0):
    """The context's plan for (n, batch) IS the model's for the context's thread count and options (`options`, if given, is what the
    caller believes it has set: asserted too); then the kinds of group `group`'s rows are `kinds`.  Returns that group's rows as dicts
    over ROW_FIELDS."""
    if options is None:
        options = context_options(ctx)
    assert dict(options) == dict(context_options(ctx)), (options, context_options(ctx))
    header, rows = context_plan(ctx, n, batch)
    want_header, want_rows, _ = ms.plan(n, batch, header[9], options)
    assert header == want_header, (n, batch, options, header, want_header)
    assert rows == list(want_rows), (n, batch, options, [r for r in zip(rows, want_rows) if r[0] != r[1]][:3])
    mine = [dict(zip(ms.ROW_FIELDS, r)) for r in rows if r[0] == group]
    if kinds is not None:
        assert [r["kind"] for r in mine] == list(kinds), (n, batch, options, [r["kind"] for r in mine])
    return mine


def pin(ctx, n, batch, row=0, group=0, kinds=None, **want):
    """assert_plan under the context's options as they stand, then row `row` of group `group` has the values `want` (ROW_FIELDS)."""
    rows = assert_plan(ctx, n, batch, None, kinds, group)
    got = {k: rows[row][k] for k in want}
    assert got == want, (n, batch, context_options(ctx), got, want)
    return rows

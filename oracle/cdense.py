"""ctypes front-end of the plain-C dense oracle (oracle/c/libogkr.so).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Field elements travel as
numpy uint64 arrays of shape (..., 4): little-endian limbs of the canonical
value.
"""

import ctypes
import os
import subprocess

import numpy as np

from .field import P

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "c", "libogkr.so")
_lib = None


def build(force=False):
    if force or not os.path.exists(_SO):
        subprocess.check_call(["make", "-C", os.path.join(_HERE, "c")], stdout=subprocess.DEVNULL)
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_SO)
        _lib.ogkr_max_threads.restype = ctypes.c_int
        # OpenMP's default is one thread per visible CPU; a container whose cgroup quota is smaller (the GPU box
        # shows 256 CPUs under a 16-CPU quota) then spends its time throttled
        if hasattr(_lib, "ogkr_set_threads"):
            _lib.ogkr_set_threads(ctypes.c_int(_quota_cpus()))
    return _lib


def _quota_cpus():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return max(1, n)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def to_limbs(values):
    """list of Python ints -> uint64 array (n, 4)."""
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        v %= P
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_limbs(arr):
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(arr[i, j]) << (64 * j) for j in range(4)) for i in range(arr.shape[0])]


def max_threads():
    return lib().ogkr_max_threads()


def usable_threads():
    """Threads the process can really run (affinity and cgroup quota), what the library's loops default to."""
    return max(1, min(_quota_cpus(), max_threads()))


def fr_mul(a, b):
    A, B = to_limbs([a]), to_limbs([b])
    O = np.zeros((1, 4), dtype=np.uint64)
    lib().ogkr_fr_mul(_p(A), _p(B), _p(O))
    return from_limbs(O)[0]


def multi_hash(values, key=0):
    A = to_limbs(list(values)) if len(values) else np.zeros((0, 4), dtype=np.uint64)
    K = to_limbs([key])
    O = np.zeros((1, 4), dtype=np.uint64)
    lib().ogkr_multi_hash(_p(A), ctypes.c_size_t(len(values)), _p(K), _p(O))
    return from_limbs(O)[0]


def mimc7_constant(i):
    O = np.zeros((1, 4), dtype=np.uint64)
    lib().ogkr_mimc7_constant(ctypes.c_int(i), _p(O))
    return from_limbs(O)[0]


def fill_table(count, seed):
    T = np.empty((count, 4), dtype=np.uint64)
    lib().ogkr_fill_table(_p(T), ctypes.c_size_t(count), ctypes.c_uint64(seed))
    return T


def sumcheck_mle_raw(table_limbs, n, threads=0):
    """-> (coeffs (n,2,4) uint64 right-aligned, lens (n,) uint32, r (n,4) uint64)."""
    table_limbs = np.ascontiguousarray(table_limbs, dtype=np.uint64)
    assert table_limbs.shape == (1 << n, 4)
    C = np.zeros((n, 2, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    R = np.zeros((n, 4), dtype=np.uint64)
    rc = lib().ogkr_sumcheck_mle(_p(table_limbs), ctypes.c_int(n), _p(C), _p(L), _p(R), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_mle rc=%d" % rc)
    return C, L, R


def sumcheck_mle_inplace_raw(table_limbs, n, threads=0):
    """sumcheck_mle_raw on the caller's array, which is overwritten (no copy: 2^30 entries are 32 GiB)."""
    assert table_limbs.flags["C_CONTIGUOUS"] and table_limbs.dtype == np.uint64 and table_limbs.shape == (1 << n, 4)
    C = np.zeros((n, 2, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    R = np.zeros((n, 4), dtype=np.uint64)
    rc = lib().ogkr_sumcheck_mle_inplace(_p(table_limbs), ctypes.c_int(n), _p(C), _p(L), _p(R), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_mle_inplace rc=%d" % rc)
    return C, L, R


def sumcheck_product_raw(tables_limbs, n, degree, threads=0):
    """ogkr_sumcheck_product on `degree` tables of 2^n entries, one after the other ((degree * 2^n, 4) or (degree, 2^n, 4))
    -> (coeffs (n, degree + 1, 4) uint64 right-aligned, lens (n,) uint32, r (n, 4) uint64, evals (degree, 4) uint64):
    one sumcheck's slice of what the product's gkr_sumcheck_product_batch_device returns."""
    tables_limbs = np.ascontiguousarray(tables_limbs, dtype=np.uint64)
    if degree < 1 or tables_limbs.size != (degree << n) * 4:
        raise ValueError("degree tables of 2^n entries expected")
    C = np.zeros((n, degree + 1, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    R = np.zeros((n, 4), dtype=np.uint64)
    E = np.zeros((degree, 4), dtype=np.uint64)
    fn = lib().ogkr_sumcheck_product
    fn.restype = ctypes.c_int
    rc = fn(_p(tables_limbs), ctypes.c_int(n), ctypes.c_int(degree), _p(C), _p(L), _p(R), _p(E),
            ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_product rc=%d" % rc)
    return C, L, R, E


class _SopTerm(ctypes.Structure):
    _fields_ = [("degree", ctypes.c_uint8), ("table", ctypes.c_uint8 * 3)]


def _sop_terms(terms, max_degree):
    """[(coeff, (table indices ..)), ..] -> (ogkr_sop_term array, coefficients (n_terms, 4), the largest term degree)."""
    terms = list(terms)
    if not terms or any(not 1 <= len(idx) <= max_degree or any(not 0 <= i < 256 for i in idx) for _, idx in terms):
        raise ValueError("1 or more terms of 1 .. %d table indices expected" % max_degree)
    arr = (_SopTerm * len(terms))()
    for k, (_, idx) in enumerate(terms):
        arr[k].degree = len(idx)
        for f, i in enumerate(idx):
            arr[k].table[f] = i
    return arr, to_limbs([c for c, _ in terms]), max(len(idx) for _, idx in terms)


def sumcheck_sop_raw(tables_limbs, n, n_tables, terms, threads=0):
    """ogkr_sumcheck_sop on n_tables tables of 2^n entries, one after the other, terms [(coeff, (table indices ..)), ..]
    -> (coeffs (n, D + 1, 4) uint64 right-aligned, lens (n,) uint32, r (n, 4) uint64, evals (n_tables, 4) uint64), D the largest
    term degree: one sumcheck's slice of what gkr_sumcheck_sop_batch_device returns."""
    tables_limbs = np.ascontiguousarray(tables_limbs, dtype=np.uint64)
    if n_tables < 1 or tables_limbs.size != (n_tables << n) * 4:
        raise ValueError("n_tables tables of 2^n entries expected")
    arr, coeffs, D = _sop_terms(terms, 3)
    C = np.zeros((n, D + 1, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    R = np.zeros((n, 4), dtype=np.uint64)
    E = np.zeros((n_tables, 4), dtype=np.uint64)
    fn = lib().ogkr_sumcheck_sop
    fn.restype = ctypes.c_int
    rc = fn(_p(tables_limbs), ctypes.c_int(n), ctypes.c_int(n_tables), ctypes.cast(arr, ctypes.c_void_p), _p(coeffs), ctypes.c_int(len(arr)),
            _p(C), _p(L), _p(R), _p(E), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_sop rc=%d" % rc)
    return C, L, R, E


def sumcheck_zerocheck_raw(tables_limbs, n, n_tables, terms, z_limbs, threads=0):
    """ogkr_sumcheck_zerocheck (the eq table materialised) on n_tables tables of 2^n entries, terms of 1 or 2 indices, z (n, 4)
    -> (coeffs (n, D + 2, 4), lens (n,), r (n, 4), evals (n_tables, 4), eq_r (4,)), D the largest term degree: one sumcheck's slice
    of what gkr_sumcheck_zerocheck_batch_device returns."""
    tables_limbs = np.ascontiguousarray(tables_limbs, dtype=np.uint64)
    z_limbs = np.ascontiguousarray(z_limbs, dtype=np.uint64)
    if n_tables < 1 or tables_limbs.size != (n_tables << n) * 4 or z_limbs.size != 4 * n:
        raise ValueError("n_tables tables of 2^n entries and a point of n entries expected")
    arr, coeffs, d = _sop_terms(terms, 2)
    C = np.zeros((n, d + 2, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    R = np.zeros((n, 4), dtype=np.uint64)
    E = np.zeros((n_tables, 4), dtype=np.uint64)
    Q = np.zeros(4, dtype=np.uint64)
    fn = lib().ogkr_sumcheck_zerocheck
    fn.restype = ctypes.c_int
    rc = fn(_p(tables_limbs), ctypes.c_int(n), ctypes.c_int(n_tables), ctypes.cast(arr, ctypes.c_void_p), _p(coeffs), ctypes.c_int(len(arr)),
            _p(z_limbs), _p(C), _p(L), _p(R), _p(E), _p(Q), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_zerocheck rc=%d" % rc)
    return C, L, R, E, Q


def grand_product_raw(table_limbs, n, threads=0, levels=False):
    """ogkr_grand_product on one table of 2^n entries ((2^n, 4) limbs) -> (P (4,), H (4, 4), C (R, 4, 4) right-aligned, L (R,) uint32,
    R (R, 4), E (n - 2, 2, 4), Z (n, 4), K (4,)) with R = n (n - 1) / 2 - 1: one proof's slice of the eight arrays
    gkr_grand_product_batch_device returns.  levels=True: a ninth array (2^n - 1, 4), level k of the tree at 2^k - 1."""
    table_limbs = np.ascontiguousarray(table_limbs, dtype=np.uint64)
    rounds = n * (n - 1) // 2 - 1 if n >= 3 else 0
    good = 3 <= n <= 30 and table_limbs.size == 4 << n
    out = [np.zeros(s, dtype=np.uint64) for s in ((4,), (4, 4), (rounds, 4, 4))] + [np.zeros(rounds, dtype=np.uint32)]
    out += [np.zeros(s, dtype=np.uint64) for s in ((rounds, 4), (max(n - 2, 0), 2, 4), (max(n, 0), 4), (4,))]
    lv = np.zeros(((1 << n) - 1, 4), dtype=np.uint64) if levels and good else None
    fn = lib().ogkr_grand_product
    fn.restype = ctypes.c_int
    rc = fn(_p(table_limbs) if good else None, ctypes.c_int(n), *[_p(a) for a in out], _p(lv) if lv is not None else None, _threads(threads))
    if rc:
        raise ValueError("ogkr_grand_product rc=%d" % rc)
    return tuple(out) + ((lv,) if levels else ())


def fraction_sum_raw(pair_limbs, n, threads=0, levels=False):
    """ogkr_fraction_sum on one pair, N then D ((2, 2^n, 4) or (2^(n+1), 4) limbs) -> (S (2, 4), H (8, 4), C (R, 4, 4) right-aligned,
    L (R,) uint32, R (R, 4), E (n - 2, 4, 4), Z (n, 4), K (2, 4)) with R = n (n - 1) / 2 - 1: one proof's slice of the eight arrays
    gkr_fraction_sum_batch_device returns.  levels=True: a ninth array (2 (2^n - 1), 4), level k of the tree at 2 (2^k - 1), p_k
    then q_k."""
    pair_limbs = np.ascontiguousarray(pair_limbs, dtype=np.uint64)
    rounds = n * (n - 1) // 2 - 1 if n >= 3 else 0
    good = 3 <= n <= 29 and pair_limbs.size == 8 << n
    out = [np.zeros(s, dtype=np.uint64) for s in ((2, 4), (8, 4), (rounds, 4, 4))] + [np.zeros(rounds, dtype=np.uint32)]
    out += [np.zeros(s, dtype=np.uint64) for s in ((rounds, 4), (max(n - 2, 0), 4, 4), (max(n, 0), 4), (2, 4))]
    lv = np.zeros((2 * ((1 << n) - 1), 4), dtype=np.uint64) if levels and good else None
    flat = pair_limbs.reshape(-1, 4)
    fn = lib().ogkr_fraction_sum
    fn.restype = ctypes.c_int
    rc = fn(_p(flat) if good else None, _p(flat[1 << n:]) if good else None, ctypes.c_int(n), *[_p(a) for a in out],
            _p(lv) if lv is not None else None, _threads(threads))
    if rc:
        raise ValueError("ogkr_fraction_sum rc=%d" % rc)
    return tuple(out) + ((lv,) if levels else ())


def _log2_exact(rows):
    return rows.bit_length() - 1 if rows > 0 and rows & (rows - 1) == 0 else -1


def lookup_multiplicities_raw(witness_limbs, table_limbs):
    """ogkr_lookup_multiplicities on (2^n_w, 4) and (2^n_t, 4) limbs -> (M (2^n_t, 4), missing, first_missing)."""
    witness_limbs = np.ascontiguousarray(witness_limbs, dtype=np.uint64).reshape(-1, 4)
    table_limbs = np.ascontiguousarray(table_limbs, dtype=np.uint64).reshape(-1, 4)
    M = np.zeros_like(table_limbs)
    missing, first = ctypes.c_uint32(0), ctypes.c_uint32(0)
    fn = lib().ogkr_lookup_multiplicities
    fn.restype = ctypes.c_int
    rc = fn(_p(witness_limbs), ctypes.c_int(_log2_exact(witness_limbs.shape[0])), _p(table_limbs), ctypes.c_int(_log2_exact(table_limbs.shape[0])),
            _p(M), ctypes.byref(missing), ctypes.byref(first))
    if rc:
        raise ValueError("ogkr_lookup_multiplicities rc=%d" % rc)
    return M, int(missing.value), int(first.value)


def lookup_pair_raw(witness_limbs, table_limbs, mult_limbs, alpha_limbs):
    """ogkr_lookup_pair -> (2, 2^L, 4) limbs: N then D, L = max(n_w, n_t) + 1."""
    witness_limbs = np.ascontiguousarray(witness_limbs, dtype=np.uint64).reshape(-1, 4)
    table_limbs = np.ascontiguousarray(table_limbs, dtype=np.uint64).reshape(-1, 4)
    mult_limbs = np.ascontiguousarray(mult_limbs, dtype=np.uint64).reshape(-1, 4)
    alpha_limbs = np.ascontiguousarray(alpha_limbs, dtype=np.uint64).reshape(-1)
    n_w, n_t = _log2_exact(witness_limbs.shape[0]), _log2_exact(table_limbs.shape[0])
    if n_w < 0 or n_t < 0 or mult_limbs.shape != table_limbs.shape or alpha_limbs.shape != (4,):
        raise ValueError("a witness and a table of a power of two entries, a multiplicity per table entry and one alpha expected")
    out = np.zeros((2, 2 << max(n_w, n_t), 4), dtype=np.uint64)
    fn = lib().ogkr_lookup_pair
    fn.restype = ctypes.c_int
    rc = fn(_p(witness_limbs), ctypes.c_int(n_w), _p(table_limbs), ctypes.c_int(n_t), _p(mult_limbs), _p(alpha_limbs), _p(out))
    if rc:
        raise ValueError("ogkr_lookup_pair rc=%d" % rc)
    return out


def lookup_raw(witness_limbs, table_limbs, mult_limbs, alpha_limbs, threads=0, levels=False):
    """The lookup's proof: fraction_sum_raw of lookup_pair_raw, n = L."""
    pair = lookup_pair_raw(witness_limbs, table_limbs, mult_limbs, alpha_limbs)
    return fraction_sum_raw(pair, pair.shape[1].bit_length() - 1, threads, levels)


def _r1cs_flat(counts, wires, coeffs):
    """The flat form of an R1CS (what gkr_r1cs_export writes): counts (3 * n_constraints,) uint32, wires (records,) uint32, coeffs
    (records, 4) uint64, checked against each other -> (n_constraints, counts, wires, coeffs)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    wires = np.ascontiguousarray(wires, dtype=np.uint32).reshape(-1)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
    if counts.size % 3 or int(counts.sum(dtype=np.uint64)) != wires.size or coeffs.shape[0] != wires.size:
        raise ValueError("counts of A, B, C per constraint and one wire and one coefficient per record expected")
    return counts.size // 3, counts, wires, coeffs


def _threads(threads):
    return ctypes.c_int(threads if threads > 0 else usable_threads())


def r1cs_rows_raw(counts, wires, coeffs, n_wires, witness_limbs, n, threads=0):
    """ogkr_r1cs_rows -> (3, 2^n, 4) uint64: Az, Bz, Cz of the witness ((n_wires, 4) limbs), rows past the constraints zero."""
    n_constraints, counts, wires, coeffs = _r1cs_flat(counts, wires, coeffs)
    witness_limbs = np.ascontiguousarray(witness_limbs, dtype=np.uint64)
    if witness_limbs.shape != (n_wires, 4) or not 0 <= n <= 40:
        raise ValueError("a witness of n_wires entries and 0 <= n <= 40 expected")
    out = np.zeros((3, 1 << n, 4), dtype=np.uint64)
    fn = lib().ogkr_r1cs_rows
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_size_t(n_constraints), ctypes.c_uint32(n_wires), _p(counts), _p(wires), _p(coeffs), _p(witness_limbs), ctypes.c_int(n),
            _p(out), _threads(threads))
    if rc:
        raise ValueError("ogkr_r1cs_rows rc=%d" % rc)
    return out


def r1cs_cols_raw(counts, wires, coeffs, n_wires, x_limbs, rho_limbs, n_y, threads=0):
    """ogkr_r1cs_cols -> (2^n_y, 4) uint64: T[y] = sum_m rho_m sum_i M_m[i][y] eq(x, i); x (n_x, 4) limbs, rho (3, 4) limbs."""
    n_constraints, counts, wires, coeffs = _r1cs_flat(counts, wires, coeffs)
    x_limbs = np.ascontiguousarray(x_limbs, dtype=np.uint64).reshape(-1, 4)
    rho_limbs = np.ascontiguousarray(rho_limbs, dtype=np.uint64)
    n_x = x_limbs.shape[0]
    if rho_limbs.shape != (3, 4) or not 0 <= n_y <= 40 or n_x > 40:
        raise ValueError("three weights, at most 40 coordinates and 0 <= n_y <= 40 expected")
    out = np.zeros((1 << n_y, 4), dtype=np.uint64)
    fn = lib().ogkr_r1cs_cols
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_size_t(n_constraints), ctypes.c_uint32(n_wires), _p(counts), _p(wires), _p(coeffs), _p(x_limbs), ctypes.c_int(n_x),
            _p(rho_limbs), ctypes.c_int(n_y), _p(out), _threads(threads))
    if rc:
        raise ValueError("ogkr_r1cs_cols rc=%d" % rc)
    return out


def r1cs_matrix_evals_raw(counts, wires, coeffs, n_wires, x_limbs, y_limbs, threads=0):
    """ogkr_r1cs_matrix_evals -> (3, 4) uint64: [A~, B~, C~](x, y); x (n_x, 4) and y (n_y, 4) limbs."""
    n_constraints, counts, wires, coeffs = _r1cs_flat(counts, wires, coeffs)
    x_limbs = np.ascontiguousarray(x_limbs, dtype=np.uint64).reshape(-1, 4)
    y_limbs = np.ascontiguousarray(y_limbs, dtype=np.uint64).reshape(-1, 4)
    if x_limbs.shape[0] > 40 or y_limbs.shape[0] > 40:
        raise ValueError("at most 40 coordinates expected")
    out = np.zeros((3, 4), dtype=np.uint64)
    fn = lib().ogkr_r1cs_matrix_evals
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_size_t(n_constraints), ctypes.c_uint32(n_wires), _p(counts), _p(wires), _p(coeffs), _p(x_limbs),
            ctypes.c_int(x_limbs.shape[0]), _p(y_limbs), ctypes.c_int(y_limbs.shape[0]), _p(out), _threads(threads))
    if rc:
        raise ValueError("ogkr_r1cs_matrix_evals rc=%d" % rc)
    return out


def _many(name, a_limbs, b_limbs):
    a_limbs = np.ascontiguousarray(a_limbs, dtype=np.uint64)
    b_limbs = np.ascontiguousarray(b_limbs, dtype=np.uint64)
    if a_limbs.shape != b_limbs.shape or a_limbs.shape[-1:] != (4,):
        raise ValueError("two limb arrays of one shape expected")
    out = np.zeros_like(a_limbs)
    fn = getattr(lib(), name)
    fn.restype = None
    fn(_p(a_limbs), _p(b_limbs), _p(out), ctypes.c_size_t(a_limbs.size // 4))
    return out


def fr_mul_many(a_limbs, b_limbs):
    """ogkr_fr_mul_many: the entrywise product of two limb arrays of one shape (canonical in, canonical out)."""
    return _many("ogkr_fr_mul_many", a_limbs, b_limbs)


def fr_add_many(a_limbs, b_limbs):
    """ogkr_fr_add_many: the entrywise sum."""
    return _many("ogkr_fr_add_many", a_limbs, b_limbs)


def sumcheck_mle(table, n, threads=0):
    C, L, R = sumcheck_mle_raw(to_limbs(table), n, threads)
    proof = [from_limbs(C[j])[2 - int(L[j]):] for j in range(n)]
    return proof, from_limbs(R)


def _gates(gate_type, left, right):
    return (np.ascontiguousarray(gate_type, dtype=np.uint8), np.ascontiguousarray(left, dtype=np.uint32),
            np.ascontiguousarray(right, dtype=np.uint32))


def sumcheck_layer_raw(k_i, k_next, gate_type, left, right, z_limbs, w_limbs, threads=0):
    gt, l, r = _gates(gate_type, left, right)
    v = 2 * k_next
    C = np.zeros((v, 3, 4), dtype=np.uint64)
    L = np.zeros(v, dtype=np.uint32)
    R = np.zeros((v, 4), dtype=np.uint64)
    z_limbs = np.ascontiguousarray(z_limbs, dtype=np.uint64).reshape(-1, 4)
    w_limbs = np.ascontiguousarray(w_limbs, dtype=np.uint64)
    rc = lib().ogkr_sumcheck_layer(ctypes.c_int(k_i), ctypes.c_int(k_next), _p(gt), _p(l), _p(r), _p(z_limbs),
                                   _p(w_limbs), _p(C), _p(L), _p(R), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_layer rc=%d" % rc)
    return C, L, R


def sumcheck_layer_lin_raw(k_i, k_next, gate_type, left, right, z_limbs, w_limbs, threads=0):
    """The linear-time twin (ogkr_sumcheck_layer_lin): same outputs as sumcheck_layer_raw, any k_next <= 28."""
    gt, l, r = _gates(gate_type, left, right)
    v = 2 * k_next
    C = np.zeros((v, 3, 4), dtype=np.uint64)
    L = np.zeros(v, dtype=np.uint32)
    R = np.zeros((v, 4), dtype=np.uint64)
    z_limbs = np.ascontiguousarray(z_limbs, dtype=np.uint64).reshape(-1, 4)
    w_limbs = np.ascontiguousarray(w_limbs, dtype=np.uint64)
    assert w_limbs.shape == (1 << k_next, 4) and len(gt) == 1 << k_i
    rc = lib().ogkr_sumcheck_layer_lin(ctypes.c_int(k_i), ctypes.c_int(k_next), _p(gt), _p(l), _p(r), _p(z_limbs),
                                       _p(w_limbs), _p(C), _p(L), _p(R), ctypes.c_int(threads if threads > 0 else usable_threads()))
    if rc:
        raise ValueError("ogkr_sumcheck_layer_lin rc=%d" % rc)
    return C, L, R


def sumcheck_layer_lin(k_i, k_next, gate_type, left, right, z, w, threads=0):
    zl = to_limbs(z) if len(z) else np.zeros((0, 4), dtype=np.uint64)
    C, L, R = sumcheck_layer_lin_raw(k_i, k_next, gate_type, left, right, zl, to_limbs(w), threads)
    proof = [from_limbs(C[j])[3 - int(L[j]):] for j in range(2 * k_next)]
    return proof, from_limbs(R)


def sumcheck_layer(k_i, k_next, gate_type, left, right, z, w, threads=0):
    zl = to_limbs(z) if len(z) else np.zeros((0, 4), dtype=np.uint64)
    C, L, R = sumcheck_layer_raw(k_i, k_next, gate_type, left, right, zl, to_limbs(w), threads)
    proof = [from_limbs(C[j])[3 - int(L[j]):] for j in range(2 * k_next)]
    return proof, from_limbs(R)


def predicate_tables(k_i, k_next, gate_type, left, right, z):
    gt, l, r = _gates(gate_type, left, right)
    n = 1 << (2 * k_next)
    A = np.zeros((n, 4), dtype=np.uint64)
    M = np.zeros((n, 4), dtype=np.uint64)
    zl = to_limbs(z) if len(z) else np.zeros((0, 4), dtype=np.uint64)
    rc = lib().ogkr_predicate_tables(ctypes.c_int(k_i), ctypes.c_int(k_next), _p(gt), _p(l), _p(r), _p(zl), _p(A), _p(M))
    if rc:
        raise ValueError("ogkr_predicate_tables rc=%d" % rc)
    return A, M


def layer_eval_raw(gate_type, left, right, prev_limbs):
    gt, l, r = _gates(gate_type, left, right)
    prev_limbs = np.ascontiguousarray(prev_limbs, dtype=np.uint64)
    out = np.zeros((len(gt), 4), dtype=np.uint64)
    lib().ogkr_layer_eval(ctypes.c_size_t(len(gt)), _p(gt), _p(l), _p(r), _p(prev_limbs), _p(out))
    return out


def line_restriction_raw(b_limbs, c_limbs, w_limbs, k):
    """-> (q (k+1,4) right-aligned highest first, length)."""
    O = np.zeros((k + 1, 4), dtype=np.uint64)
    ln = ctypes.c_uint32(0)
    B = np.ascontiguousarray(b_limbs, dtype=np.uint64).reshape(-1, 4)
    Cc = np.ascontiguousarray(c_limbs, dtype=np.uint64).reshape(-1, 4)
    Wl = np.ascontiguousarray(w_limbs, dtype=np.uint64)
    rc = lib().ogkr_line_restriction(ctypes.c_int(k), _p(B), _p(Cc), _p(Wl), _p(O), ctypes.byref(ln))
    if rc:
        raise ValueError("ogkr_line_restriction rc=%d" % rc)
    return O, int(ln.value)


def mobius_raw(w_limbs, k):
    """evaluation table -> monomial coefficients (get_multi_ext, poly.rs:502-536), limbs in, limbs out."""
    out = np.array(w_limbs, dtype=np.uint64, copy=True).reshape(1 << k, 4)
    lib().ogkr_mobius(_p(out), ctypes.c_int(k))
    return out


def prove_raw(layers, input_limbs, threads=0):
    """prover.rs:6-96 on limb arrays only (no Python integers per table entry): for circuits with wide layers, where
    the dense layer form cannot follow.  Uses the linear-time layer prover.  z[0] = 0 (prover.rs:16-21).
    -> dict of numpy arrays: per layer C (2k,3,4), L (2k,), R (2k,4), q (k+1,4), q_len; z list of (k_i,4); r (depth,4);
    values list of (2^k_i,4)."""
    vals = [np.ascontiguousarray(input_limbs, dtype=np.uint64).reshape(-1, 4)]
    for gt, l, r in reversed(layers):
        vals.append(layer_eval_raw(gt, l, r, vals[-1]))
    vals.reverse()
    ks = [max(0, (v.shape[0] - 1).bit_length()) for v in vals]
    z = [np.zeros((ks[0], 4), dtype=np.uint64)]
    Cs, Ls, Rs, qs, qlens, rstars = [], [], [], [], [], []
    for i, (gt, l, r) in enumerate(layers):
        kn = ks[i + 1]
        C, L, R = sumcheck_layer_lin_raw(ks[i], kn, gt, l, r, z[i], vals[i + 1], threads)
        Cs.append(C)
        Ls.append(L)
        Rs.append(R)
        q, qlen = line_restriction_raw(R[:kn], R[kn:], vals[i + 1], kn)
        qs.append(q)
        qlens.append(qlen)
        r_star = from_limbs(R[2 * kn - 1:2 * kn])[0]   # multi_hash(last round vector) = the last challenge (prover.rs:74-78)
        bs, cs = from_limbs(R[:kn]), from_limbs(R[kn:])
        z.append(to_limbs([(bi + (ci - bi) * r_star) % P for bi, ci in zip(bs, cs)]))
        rstars.append(r_star)
    return dict(C=Cs, L=Ls, R=Rs, q=qs, q_len=qlens, z=z, r=to_limbs(rstars), k=ks, values=vals)


def line_restriction(b, c, w, k):
    O = np.zeros((k + 1, 4), dtype=np.uint64)
    ln = ctypes.c_uint32(0)
    B = to_limbs(b) if k else np.zeros((0, 4), dtype=np.uint64)
    Cc = to_limbs(c) if k else np.zeros((0, 4), dtype=np.uint64)
    rc = lib().ogkr_line_restriction(ctypes.c_int(k), _p(B), _p(Cc), _p(to_limbs(w)), _p(O), ctypes.byref(ln))
    if rc:
        raise ValueError("ogkr_line_restriction rc=%d" % rc)
    return from_limbs(O)[k + 1 - ln.value:]


def prove(layers, input_values, z0=None, threads=0):
    """prover.rs:6-96 composed from the C pieces (same dict as dense.prove)."""
    from .mimc7 import multi_hash as py_hash  # tiny; the C hash is checked against it separately
    vals = [to_limbs(list(input_values))]
    for gt, l, r in reversed(layers):
        vals.append(layer_eval_raw(gt, l, r, vals[-1]))
    vals.reverse()
    ks = [max(0, (v.shape[0] - 1).bit_length()) for v in vals]
    z = [[0] * ks[0]] if z0 is None else [[x % P for x in z0]]
    sps, srs, qs, rstars = [], [], [], []
    for i, (gt, l, r) in enumerate(layers):
        kn = ks[i + 1]
        zl = to_limbs(z[i]) if ks[i] else np.zeros((0, 4), dtype=np.uint64)
        C, L, R = sumcheck_layer_raw(ks[i], kn, gt, l, r, zl, vals[i + 1], threads)
        sp = [from_limbs(C[j])[3 - int(L[j]):] for j in range(2 * kn)]
        sr = from_limbs(R)
        sps.append(sp)
        srs.append(sr)
        b_star, c_star = sr[:kn], sr[kn:]
        qs.append(line_restriction(b_star, c_star, from_limbs(vals[i + 1]), kn))
        r_star = multi_hash(sp[-1], 0)
        assert r_star == py_hash(sp[-1], 0)
        z.append([(bi + (ci - bi) * r_star) % P for bi, ci in zip(b_star, c_star)])
        rstars.append(r_star)
    return dict(sumcheck_proofs=sps, sumcheck_r=srs, q=qs, z=z, r=rstars, depth=len(layers) + 1, k=ks,
                values=[from_limbs(v) for v in vals])

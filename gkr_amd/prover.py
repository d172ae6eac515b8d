"""Host-side mirror of the reference's prover interface over the C ABI.

Names follow the reference (rust/src/gkr.rs, rust/src/gkr/prover.rs,
rust/src/gkr/sumcheck.rs) so parity tests read like tests of the reference:

    reference (Rust)                                   here
    ------------------------------------------------   ---------------------------------
    GKRCircuit { layer: Vec<Layer>, input_k }          GKRCircuit(layers, input_k)
    Layer { k, add, mult, wire }                       Layer(k, gate_type, left, right)
    prover::prove(&circuit, &input) -> Proof           prove(circuit, input_values) -> Proof
    sumcheck::prove_sumcheck_opt(..., v)               prove_sumcheck_opt(layer, k_next, z, W)
    sumcheck::prove_sumcheck(g, v)                     prove_sumcheck(table, v)
    Mimc7::multi_hash(v, &Fr::from(0))                 multi_hash(values, key=0)

The reference stores a layer's wiring as term-list polynomials add_i / mult_i
plus 0/1 wire strings (convert.rs:715-774); both are functions of the gate
list (type, left operand, right operand), which is what this interface takes.
Everything numeric happens in libgkr_amd.so on the GPU; this module only
marshals.  Errors: the reference panics, here a GkrError carries the status.
"""

import ctypes
from dataclasses import dataclass, field as dc_field
from typing import List, Sequence

import numpy as np

from . import _native as N
from .field import MODULUS, as_limbs, from_limbs, to_limbs


class GkrError(RuntimeError):
    def __init__(self, status, message=""):
        self.status = status
        text = N.lib().gkr_strerror(status).decode()
        super().__init__("%s (status %d)%s" % (text, status, ": " + message if message else ""))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@dataclass
class Layer:
    """One gate layer: gate g is add (0) or mult (1) of entries left[g], right[g]
    of the next layer (gkr.rs:35-51; wiring convert.rs:715-767)."""
    k: int
    gate_type: Sequence[int]
    left: Sequence[int]
    right: Sequence[int]

    def arrays(self):
        gt = np.ascontiguousarray(self.gate_type, dtype=np.uint8)
        l = np.ascontiguousarray(self.left, dtype=np.uint32)
        r = np.ascontiguousarray(self.right, dtype=np.uint32)
        if not (len(gt) == len(l) == len(r) == 1 << self.k):
            raise GkrError(N.GKR_ERR_INVALID, "layer with k=%d needs %d gates" % (self.k, 1 << self.k))
        return gt, l, r


@dataclass
class GKRCircuit:
    """gkr.rs:53-114."""
    layer: List[Layer]
    input_k: int

    def depth(self):
        return len(self.layer)

    def k(self, i):
        return self.input_k if i == len(self.layer) else self.layer[i].k

    def get_k_list(self):
        return [self.k(i) for i in range(self.depth() + 1)]


@dataclass
class Proof:
    """gkr.rs:7-19.  d / input_func are term lists [coeff, e_1..e_k] (order not
    significant: the reference emits them in HashMap order)."""
    sumcheck_proofs: List[List[List[int]]]
    sumcheck_r: List[List[int]]
    d: List[List[int]]
    q: List[List[int]]
    z: List[List[int]]
    r: List[int]
    depth: int
    input_func: List[List[int]]
    k: List[int]
    values: List[List[int]] = dc_field(default_factory=list, repr=False)


def multi_hash(values, key=0):
    """MiMC7-91 multi_hash on the host side of the library (no GPU needed)."""
    arr = to_limbs(values) if len(values) else np.zeros((0, 4), dtype=np.uint64)
    k = to_limbs([key])
    out = np.zeros((1, 4), dtype=np.uint64)
    rc = N.lib().gkr_mimc7_multi_hash(_ptr(arr), ctypes.c_size_t(len(values)), _ptr(k), _ptr(out))
    if rc:
        raise GkrError(rc)
    return from_limbs(out)[0]


def options():
    """The library's option table: [(name, environment variable, what it does)] (no GPU needed)."""
    lib = N.lib()
    for f in (lib.gkr_option_name, lib.gkr_option_doc, lib.gkr_option_env):
        f.restype = ctypes.c_char_p
        f.argtypes = [ctypes.c_int]
    lib.gkr_option_count.restype = ctypes.c_int
    return [(lib.gkr_option_name(i).decode(), lib.gkr_option_env(i).decode(), lib.gkr_option_doc(i).decode())
            for i in range(lib.gkr_option_count())]


def host_hash_us(length):
    """(us per hash in sixteen IFMA lanes, us per scalar hash) of a `length`-element round vector on one host thread."""
    a, b = ctypes.c_double(), ctypes.c_double()
    rc = N.lib().gkr_ubench_host_hash(ctypes.c_int(length), ctypes.byref(a), ctypes.byref(b))
    if rc:
        raise GkrError(rc)
    return a.value, b.value


def _proof_bufs(arrays, B):
    """The B gkr_proof_buf structures (nine pointers each) over arrays whose first axis is the proof: one address
    matrix, base + b * stride per array, built in numpy -- not B x 9 ctypes objects (0.5 - 1 ms of interpreter time per
    call, which the proving threads of ProvingStep.prove_raw_concurrent pay one after the other under the GIL)."""
    addr = np.empty((B, len(arrays)), dtype=np.uint64)
    for j, a in enumerate(arrays):
        addr[:, j] = a.ctypes.data + np.arange(B, dtype=np.uint64) * np.uint64(a.strides[0])
    return (N.ProofBuf * B).from_buffer(addr)


def _decode_proofs(arrays, ks):
    """The nine output arrays of gkr_prove_batch / one gkr_prove_many item (first axis = proof) -> Proof objects."""
    sc, sl, sr, q, ql, z, rr, dco, ico = arrays
    L = len(ks) - 1
    out = []
    for b in range(sc.shape[0]):
        proofs, rs, qs, zs = [], [], [], []
        ro = qo = 0
        for i in range(L):
            k = ks[i + 1]
            proofs.append([from_limbs(sc[b, ro + j])[3 - int(sl[b, ro + j]):] for j in range(2 * k)])
            rs.append(from_limbs(sr[b, ro:ro + 2 * k]))
            qs.append(from_limbs(q[b, qo:qo + k + 1])[k + 1 - int(ql[b, i]):])
            ro += 2 * k
            qo += k + 1
        zo = 0
        for i in range(L + 1):
            zs.append(from_limbs(z[b, zo:zo + ks[i]]) if ks[i] else [])
            zo += ks[i]
        out.append(Proof(sumcheck_proofs=proofs, sumcheck_r=rs, d=_terms_from_coeffs(dco[b], ks[0]), q=qs, z=zs,
                         r=from_limbs(rr[b]), depth=L + 1, input_func=_terms_from_coeffs(ico[b], ks[-1]), k=ks))
    return out


def _terms_from_coeffs(coeffs, k):
    """monomial-coefficient table -> reference term list (non-zero terms only)."""
    vals = from_limbs(coeffs)
    return [[c] + [(m >> (k - 1 - j)) & 1 for j in range(k)] for m, c in enumerate(vals) if c]


def _tree_rounds(n):
    """R = n (n - 1) / 2 - 1: the rows of the layers k = 2 .. n - 1 of a tree argument (grand product, fractional sum) over 2^n leaves."""
    return n * (n - 1) // 2 - 1


def _tree_row(k):
    """the first row of layer k"""
    return k * (k - 1) // 2 - 1


class VerifyHandle:
    """A circuit prepared for the device verifier (gkr_verify_prepare): its gate arrays live on the context's device until
    close().  Context.prepare_verify makes one; Context.verify_batch takes it any number of times."""

    def __init__(self, ctx, handle, k_list):
        self._ctx = ctx
        self._h = handle
        self.k = list(k_list)

    def close(self):
        if self._h:
            N.lib().gkr_verify_circuit_free(self._ctx._h if self._ctx else None, self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            if self._ctx is not None and self._ctx._h:
                self.close()
        except Exception:
            pass


class R1csRows:
    """An R1CS's matrices in CSR form on a context's device (gkr_r1cs_rows_prepare): made once per R1CS by Context.r1cs_rows, taken
    by Context.r1cs_rows_device / r1cs_zerocheck_batch_device for witness after witness.  Close it before its context."""

    def __init__(self, ctx, handle):
        self._ctx = ctx
        self._h = handle

    def info(self):
        """The CSR form's sizes: n (tables of 2^n entries), n_wires, n_constraints, n_terms / n_long_rows per matrix, n_pool."""
        out = N.R1csCsrInfo()
        rc = N.lib().gkr_r1cs_rows_info(self._h, ctypes.byref(out))
        if rc:
            raise GkrError(rc, "gkr_r1cs_rows_info")
        return out.as_dict()

    def close(self):
        if self._h:
            N.lib().gkr_r1cs_rows_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            if self._ctx is not None and self._ctx._h:
                self.close()
        except Exception:
            pass


class R1csCols:
    """An R1CS's matrices in column-major form on a context's device (gkr_r1cs_cols_prepare): made once per R1CS by
    Context.r1cs_cols, taken by Context.r1cs_cols_device / r1cs_inner_batch_device for call after call.  Close it before its
    context."""

    def __init__(self, ctx, handle):
        self._ctx = ctx
        self._h = handle

    def info(self):
        """The column-major form's sizes: n_x, n_y, n_wires, n_constraints, n_terms / n_long_cols per matrix, n_pool."""
        out = N.R1csCscInfo()
        rc = N.lib().gkr_r1cs_cols_info(self._h, ctypes.byref(out))
        if rc:
            raise GkrError(rc, "gkr_r1cs_cols_info")
        return out.as_dict()

    def close(self):
        if self._h:
            N.lib().gkr_r1cs_cols_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            if self._ctx is not None and self._ctx._h:
                self.close()
        except Exception:
            pass


class Context:
    """One GPU context (one HIP stream).  Not thread-safe; use one per thread."""

    def __init__(self, device=0, devices=None):
        """device: the GPU of this context.  devices=[ids]: gkr_ctx_create_multi -- the context lives on ids[0] and
        prove_many deals its items over child contexts on all of them (one host process, several GPUs)."""
        self._h = ctypes.c_void_p()
        if devices is not None:
            ids = (ctypes.c_int * len(devices))(*devices)
            rc = N.lib().gkr_ctx_create_multi(ids, ctypes.c_int(len(devices)), ctypes.byref(self._h))
        else:
            rc = N.lib().gkr_ctx_create(ctypes.c_int(device), ctypes.byref(self._h))
        if rc:
            self._h = None
            raise GkrError(rc, "gkr_ctx_create(device=%d)" % device)

    def close(self):
        if self._h:
            N.lib().gkr_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise GkrError(rc, (N.lib().gkr_last_error(self._h) or b"").decode())

    # -- context knobs
    def device_name(self):
        buf = ctypes.create_string_buffer(256)
        self._check(N.lib().gkr_ctx_device_name(self._h, buf, ctypes.c_size_t(256)))
        return buf.value.decode()

    def device_count(self):
        """Devices prove_many deals over (1 unless created with devices=[...])."""
        N.lib().gkr_ctx_device_count.restype = ctypes.c_int
        return int(N.lib().gkr_ctx_device_count(self._h))

    def set_transcript(self, mode):
        self._check(N.lib().gkr_ctx_set_transcript(self._h, ctypes.c_int(mode)))

    def set_option(self, name, value):
        """One of the library's switches (csrc/options.h; gkr_amd.options() lists them) for THIS context only."""
        N.lib().gkr_ctx_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_longlong]
        self._check(N.lib().gkr_ctx_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        N.lib().gkr_ctx_get_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
        v = ctypes.c_longlong()
        self._check(N.lib().gkr_ctx_get_option(self._h, name.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_host_threads(self, threads):
        """Host threads the context may use for the transcript, the caller included (0 = default)."""
        self._check(N.lib().gkr_ctx_set_host_threads(self._h, ctypes.c_int(threads)))

    def profile(self, enable=True):
        """0/False off, 1/True every kernel, 2 the bandwidth-bound kernels only (see gkr_amd.h)."""
        self._check(N.lib().gkr_ctx_profile(self._h, ctypes.c_int(int(enable))))

    def profile_reset(self):
        self._check(N.lib().gkr_ctx_profile_reset(self._h))

    def profile_get(self, kernel):
        n = ctypes.c_uint64()
        ms = ctypes.c_double()
        b = ctypes.c_double()
        self._check(N.lib().gkr_ctx_profile_get(self._h, kernel.encode(), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(b)))
        return dict(launches=n.value, total_ms=ms.value, bytes=b.value)

    def profile_samples(self, kernel, capacity=4096):
        """[(ms, algorithmic bytes)] of the single launches of `kernel` since the last reset."""
        ms = np.zeros(capacity, dtype=np.float64)
        by = np.zeros(capacity, dtype=np.float64)
        n = ctypes.c_size_t()
        self._check(N.lib().gkr_ctx_profile_samples(self._h, kernel.encode(), _ptr(ms), _ptr(by), ctypes.c_size_t(capacity),
                                                    ctypes.byref(n)))
        k = min(n.value, capacity)
        return list(zip(ms[:k].tolist(), by[:k].tolist()))

    # -- device memory
    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(N.lib().gkr_device_alloc(self._h, ctypes.c_size_t(nbytes), ctypes.byref(p)))
        return p

    def free(self, dptr):
        self._check(N.lib().gkr_device_free(self._h, dptr))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._check(N.lib().gkr_device_upload(self._h, dptr, _ptr(arr), ctypes.c_size_t(arr.nbytes)))

    def download(self, dptr, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        self._check(N.lib().gkr_device_download(self._h, _ptr(out), dptr, ctypes.c_size_t(out.nbytes)))
        return out

    def fill_table(self, dptr, count, seed):
        self._check(N.lib().gkr_device_fill_table(self._h, dptr, ctypes.c_size_t(count), ctypes.c_uint64(seed)))

    def fill_shard(self, dptr, n, log2_shards, shard, seed):
        """Rank `shard`'s entries (gkr_sumcheck_mle_sharded_dev's layout) of the table fill_table(dptr, 2^n, seed) writes."""
        self._check(N.lib().gkr_device_fill_shard(self._h, dptr, ctypes.c_int(n), ctypes.c_int(log2_shards), ctypes.c_int(shard),
                                                  ctypes.c_uint64(seed)))

    def synchronize(self):
        self._check(N.lib().gkr_device_synchronize(self._h))

    def ceilings(self, nbytes=2 << 30):
        """The box's own ceilings, measured now: {"copy_GBps", "read_GBps", "modmul_per_sec"} (gkr_ubench_ceilings)."""
        c, r, m = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._check(N.lib().gkr_ubench_ceilings(self._h, ctypes.c_size_t(nbytes), ctypes.byref(c), ctypes.byref(r), ctypes.byref(m)))
        return {"copy_GBps": c.value, "read_GBps": r.value, "modmul_per_sec": m.value}

    # -- plain multilinear sumcheck (prove_sumcheck, sumcheck.rs:158-214)
    def sumcheck_mle_raw(self, table_limbs, n):
        table_limbs = np.ascontiguousarray(table_limbs, dtype=np.uint64)
        if table_limbs.shape != (1 << n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "table must have 2^n rows")
        C = np.zeros((n, 2, 4), dtype=np.uint64)
        L = np.zeros(n, dtype=np.uint32)
        R = np.zeros((n, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_mle(self._h, _ptr(table_limbs), ctypes.c_int(n), _ptr(C), _ptr(L), _ptr(R)))
        return C, L, R

    def sumcheck_mle_batch_device(self, d_tables, n, batch, out=None):
        """out: (C, L, R) arrays of an earlier call to write into (a caller that proves batch after batch saves the
        page faults of fresh output arrays, which otherwise land inside the hash workers)."""
        if out is not None:
            C, L, R = out
            if C.shape != (batch, n, 2, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4):
                raise GkrError(N.GKR_ERR_INVALID, "output arrays do not match (batch, n)")
        else:
            C = np.zeros((batch, n, 2, 4), dtype=np.uint64)
            L = np.zeros((batch, n), dtype=np.uint32)
            R = np.zeros((batch, n, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_mle_batch_device(self._h, d_tables, ctypes.c_int(n), ctypes.c_int(batch),
                                                          _ptr(C), _ptr(L), _ptr(R)))
        return C, L, R

    def prove_sumcheck(self, table, v):
        """(proof, r) like the reference: proof[j] is the round vector, highest degree first."""
        C, L, R = self.sumcheck_mle_raw(as_limbs(table), v)
        return [from_limbs(C[j])[2 - int(L[j]):] for j in range(v)], from_limbs(R)

    # -- sumcheck over a product of tables (prove_sumcheck on mult_poly of the tables' extensions; sumcheck.rs:158-214, poly.rs:349-386)
    def sumcheck_product_batch_device(self, d_tables, n, degree, batch, out=None):
        """gkr_sumcheck_product_batch_device: `batch` sumchecks over the product of `degree` resident tables of 2^n entries each
        (factor f of sumcheck b at d_tables + (b * degree + f) * 2^n elements; not modified).  -> (C, L, R, E): C (batch, n,
        degree + 1, 4) right-aligned round vectors, highest degree first; L (batch, n) lengths; R (batch, n, 4) challenges; E
        (batch, degree, 4) the factors' values at the challenges.  out: the four arrays of an earlier call to write into."""
        if out is not None:
            C, L, R, E = out
            if C.shape != (batch, n, degree + 1, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4) or E.shape != (batch, degree, 4):
                raise GkrError(N.GKR_ERR_INVALID, "output arrays do not match (batch, n, degree)")
        else:
            C = np.zeros((batch, n, max(degree, 0) + 1, 4), dtype=np.uint64)
            L = np.zeros((batch, n), dtype=np.uint32)
            R = np.zeros((batch, n, 4), dtype=np.uint64)
            E = np.zeros((batch, max(degree, 1), 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_product_batch_device(self._h, d_tables, n, degree, batch, _ptr(C), _ptr(L), _ptr(R), _ptr(E)))
        return C, L, R, E

    def prove_sumcheck_product(self, tables, v):
        """Sumcheck of sum_x prod_f tables[f](x) over {0,1}^v: tables is a list of 1 .. 3 tables of 2^v values.
        -> (proof, r, evals): proof[j] the round vector (its used slots, highest degree first, 1 .. len(tables) + 1 of them), r
        the challenges, evals[f] = tables[f]~(r), the factor's multilinear extension at the challenges.
        Context.verify_sumcheck_product(tables, proof, r) checks the transcript AND that it belongs to these tables (it
        evaluates them at r on the device); verifier.verify_sumcheck_product is the transcript's part of it on plain integers."""
        degree = len(tables)
        limbs = np.concatenate([as_limbs(t) for t in tables], axis=0) if degree else np.zeros((0, 4), dtype=np.uint64)
        if limbs.shape[0] != degree << v:
            raise GkrError(N.GKR_ERR_INVALID, "every table must have 2^v values")
        C = np.zeros((v, degree + 1, 4), dtype=np.uint64)
        L = np.zeros(v, dtype=np.uint32)
        R = np.zeros((v, 4), dtype=np.uint64)
        E = np.zeros((max(degree, 1), 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_product(self._h, _ptr(limbs), v, degree, _ptr(C), _ptr(L), _ptr(R), _ptr(E)))
        return [from_limbs(C[j])[degree + 1 - int(L[j]):] for j in range(v)], from_limbs(R), from_limbs(E[:degree])

    # -- sumcheck over a sum of products of tables, g = sum_k c_k prod_j T_t(k,j) (prove_sumcheck on add_poly of scaled mult_poly's)
    @staticmethod
    def _sop_terms(terms, n_tables):
        """[(coeff, (table indices ..)), ..] -> (SopTerm array, (K, 4) coefficient limbs, the largest degree)."""
        K = len(terms)
        if not 1 <= K <= N.GKR_SOP_MAX_TERMS:
            raise GkrError(N.GKR_ERR_INVALID, "1 .. %d terms expected" % N.GKR_SOP_MAX_TERMS)
        arr = (N.SopTerm * K)()
        for k, (_, idx) in enumerate(terms):
            idx = tuple(int(i) for i in idx)
            if not 1 <= len(idx) <= 3 or any(not 0 <= i < n_tables for i in idx):
                raise GkrError(N.GKR_ERR_INVALID, "a term is a product of 1 .. 3 tables of the call")
            arr[k].degree = len(idx)
            for j, i in enumerate(idx):
                arr[k].table[j] = i
        return arr, to_limbs([int(c) % MODULUS for c, _ in terms]), max(t.degree for t in arr)

    def sumcheck_sop_batch_device(self, d_tables, n, n_tables, terms, batch, out=None):
        """gkr_sumcheck_sop_batch_device: `batch` sumchecks of sum_k c_k prod_j T_t(k,j) over n_tables resident tables of 2^n entries
        each (table m of sumcheck b at d_tables + (b * n_tables + m) * 2^n elements; not modified).  terms: [(coeff, (table
        indices ..)), ..], shared by the batch.  -> (C, L, R, E): C (batch, n, D + 1, 4) right-aligned round vectors, highest degree
        first, D the largest term degree; L (batch, n) lengths; R (batch, n, 4) challenges; E (batch, n_tables, 4) the tables'
        values at the challenges.  out: the four arrays of an earlier call to write into."""
        arr, coeffs, D = self._sop_terms(terms, n_tables)
        if out is not None:
            C, L, R, E = out
            if C.shape != (batch, n, D + 1, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4) or E.shape != (batch, n_tables, 4):
                raise GkrError(N.GKR_ERR_INVALID, "output arrays do not match (batch, n, degree, n_tables)")
        else:
            C = np.zeros((batch, n, D + 1, 4), dtype=np.uint64)
            L = np.zeros((batch, n), dtype=np.uint32)
            R = np.zeros((batch, n, 4), dtype=np.uint64)
            E = np.zeros((batch, n_tables, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_sop_batch_device(self._h, d_tables, n, n_tables, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs),
                                                          len(terms), batch, _ptr(C), _ptr(L), _ptr(R), _ptr(E)))
        return C, L, R, E

    def prove_sumcheck_sop(self, tables, terms, v):
        """Sumcheck of sum_x sum_k c_k prod_j tables[t(k,j)](x) over {0,1}^v: tables is a list of 1 .. 8 tables of 2^v values,
        terms [(coeff, (table indices ..)), ..] with 1 .. 3 indices each.  -> (proof, r, evals): proof[j] the round vector (its
        used slots, highest degree first), r the challenges, evals[m] = tables[m]~(r).  Context.verify_sumcheck_sop(tables, terms,
        proof, r) checks the transcript AND that it belongs to these tables (it evaluates them at r on the device);
        verifier.verify_sumcheck_sop checks the transcript against evals on plain integers."""
        M = len(tables)
        if not 1 <= M <= N.GKR_SOP_MAX_TABLES:
            raise GkrError(N.GKR_ERR_INVALID, "1 .. %d tables expected" % N.GKR_SOP_MAX_TABLES)
        arr, coeffs, D = self._sop_terms(terms, M)
        limbs = np.concatenate([as_limbs(t) for t in tables], axis=0)
        if limbs.shape[0] != M << v:
            raise GkrError(N.GKR_ERR_INVALID, "every table must have 2^v values")
        C = np.zeros((v, D + 1, 4), dtype=np.uint64)
        L = np.zeros(v, dtype=np.uint32)
        R = np.zeros((v, 4), dtype=np.uint64)
        E = np.zeros((M, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_sop(self._h, _ptr(limbs), v, M, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs), len(terms), _ptr(C),
                                             _ptr(L), _ptr(R), _ptr(E)))
        return [from_limbs(C[j])[D + 1 - int(L[j]):] for j in range(v)], from_limbs(R), from_limbs(E)

    # -- the zero-check: sum_x eq(z, x) sum_k c_k prod_j T_t(k,j)(x), term degrees 1 and 2, eq(z, .) never a table
    @staticmethod
    def _points(z, batch, n):
        """z as (batch, n, 4) limbs: such an array, or `batch` lists of n integers (reduced modulo r)."""
        if isinstance(z, np.ndarray) and z.dtype == np.uint64:
            pts = np.ascontiguousarray(z)
        else:
            pts = to_limbs([int(x) % MODULUS for row in z for x in row]).reshape(-1, n, 4) if len(z) else np.zeros((0, n, 4), dtype=np.uint64)
        if pts.shape != (batch, n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "points of shape (batch, n, 4) expected")
        return pts

    def sumcheck_zerocheck_batch_device(self, d_tables, n, n_tables, terms, batch, z, out=None):
        """gkr_sumcheck_zerocheck_batch_device: `batch` sumchecks of eq(z_b, .) * sum_k c_k prod_j T_t(k,j) over n_tables resident
        tables of 2^n entries each (the layout of sumcheck_sop_batch_device; not modified), terms of 1 or 2 tables, z (batch, n, 4)
        limbs or `batch` lists of n integers.  -> (C, L, R, E, Q): C (batch, n, D + 1, 4) right-aligned round vectors, D = the
        largest term degree + 1; L (batch, n); R (batch, n, 4); E (batch, n_tables, 4) the tables' values at the challenges;
        Q (batch, 4) eq(z_b, r_b).  The first four are byte for byte what sumcheck_sop_batch_device returns on the tables
        {eq(z, .), T_0 ..} with every term prefixed by table 0.  out: the five arrays of an earlier call to write into."""
        arr, coeffs, d = self._sop_terms(terms, n_tables)
        if d > 2:
            raise GkrError(N.GKR_ERR_INVALID, "a zero-check's terms are products of 1 or 2 tables")
        pts = self._points(z, batch, n)
        if out is not None:
            C, L, R, E, Q = out
            if (C.shape != (batch, n, d + 2, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4) or E.shape != (batch, n_tables, 4)
                    or Q.shape != (batch, 4)):
                raise GkrError(N.GKR_ERR_INVALID, "output arrays do not match (batch, n, degree, n_tables)")
        else:
            C = np.zeros((batch, n, d + 2, 4), dtype=np.uint64)
            L = np.zeros((batch, n), dtype=np.uint32)
            R = np.zeros((batch, n, 4), dtype=np.uint64)
            E = np.zeros((batch, n_tables, 4), dtype=np.uint64)
            Q = np.zeros((batch, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_zerocheck_batch_device(self._h, d_tables, n, n_tables, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs),
                                                                len(terms), batch, _ptr(pts), _ptr(C), _ptr(L), _ptr(R), _ptr(E), _ptr(Q)))
        return C, L, R, E, Q

    def prove_zerocheck(self, tables, terms, z, v):
        """Sumcheck of sum_x eq(z, x) sum_k c_k prod_j tables[t(k,j)](x) over {0,1}^v: tables is a list of 1 .. 8 tables of 2^v
        values, terms [(coeff, (table indices ..)), ..] with 1 or 2 indices each, z a point of v integers (0 and 1 allowed).
        -> (proof, r, evals, eq_r): proof[j] the round vector (its used slots, highest degree first), r the challenges,
        evals[m] = tables[m]~(r), eq_r = eq(z, r).  verifier.verify_sumcheck_zerocheck checks the transcript on plain integers."""
        M = len(tables)
        if not 1 <= M <= N.GKR_SOP_MAX_TABLES:
            raise GkrError(N.GKR_ERR_INVALID, "1 .. %d tables expected" % N.GKR_SOP_MAX_TABLES)
        arr, coeffs, d = self._sop_terms(terms, M)
        if d > 2:
            raise GkrError(N.GKR_ERR_INVALID, "a zero-check's terms are products of 1 or 2 tables")
        limbs = np.concatenate([as_limbs(t) for t in tables], axis=0)
        if limbs.shape[0] != M << v:
            raise GkrError(N.GKR_ERR_INVALID, "every table must have 2^v values")
        pts = self._points([z], 1, v)
        C = np.zeros((v, d + 2, 4), dtype=np.uint64)
        L = np.zeros(v, dtype=np.uint32)
        R = np.zeros((v, 4), dtype=np.uint64)
        E = np.zeros((M, 4), dtype=np.uint64)
        Q = np.zeros((1, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_zerocheck(self._h, _ptr(limbs), v, M, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs), len(terms),
                                                   _ptr(pts), _ptr(C), _ptr(L), _ptr(R), _ptr(E), _ptr(Q)))
        return [from_limbs(C[j])[d + 2 - int(L[j]):] for j in range(v)], from_limbs(R), from_limbs(E), from_limbs(Q)[0]

    def eq_table_device(self, z, n, batch, d_out, stride=None):
        """gkr_eq_table_device: the canonical tables eq(z_b, .) of `batch` points (z: (batch, n, 4) limbs or `batch` lists of n
        integers; variable 1 = the most significant index bit) written to device memory, table b at d_out + b * stride elements
        (stride >= 2^n; None: one table after the other).  With stride = n_tables * 2^n the call fills table 0 of every
        sumcheck of an SOP layout."""
        pts = self._points(z, batch, n)
        self._check(N.lib().gkr_eq_table_device(self._h, _ptr(pts), n, batch, d_out, (1 << n) if stride is None else int(stride)))

    # -- the two GKR tree arguments, the grand product (W = 1 table per proof) and the fractional sum (W = 2): one plumbing for both.
    # Every width follows from W: the head 4 W values, a layer's end values 2 W, the root and the end claims W (an axis of their
    # own only for W > 1); R = _tree_rounds(n) rows, layer k from row _tree_row(k).
    @staticmethod
    def _tree_shapes(W, n, lead):
        """The shapes of (root, H, C, L, R, E, Z, K) behind the leading axes `lead` -- (batch,), or () for one proof."""
        rounds, vals = _tree_rounds(n), lead + ((4,) if W == 1 else (W, 4))
        return [vals, lead + (4 * W, 4), lead + (rounds, 4, 4), lead + (rounds,), lead + (rounds, 4), lead + (n - 2, 2 * W, 4), lead + (n, 4), vals]

    def _tree_batch_device(self, fn, W, d_tables, n, batch, out):
        shapes = [(s, np.uint32 if i == 3 else np.uint64) for i, s in enumerate(self._tree_shapes(W, n, (batch,)))]
        if n < 3 or batch < 1:
            raise GkrError(N.GKR_ERR_INVALID, "n >= 3 and batch >= 1 expected")
        if out is not None:
            if len(out) != 8 or any(a.shape != s or a.dtype != d for a, (s, d) in zip(out, shapes)):
                raise GkrError(N.GKR_ERR_INVALID, "output arrays do not match (batch, n)")
        else:
            out = tuple(np.zeros(s, dtype=d) for s, d in shapes)
        self._check(fn(self._h, d_tables, n, batch, *(_ptr(a) for a in out)))
        return out

    def _tree_prove(self, fn, W, tables, v):
        """fn(ctx, *tables, v, the eight outputs) -> (root, head, layers, point, claims) as lists of integers."""
        shapes = self._tree_shapes(W, v, ())
        shapes[0] = shapes[7] = (W, 4)                                     # (W values also where W = 1)
        S, H, C, L, R, E, Z, K = (np.zeros(s, dtype=np.uint32 if i == 3 else np.uint64) for i, s in enumerate(shapes))
        self._check(fn(self._h, *(_ptr(t) for t in tables), v, *(_ptr(a) for a in (S, H, C, L, R, E, Z, K))))
        rs, layers = from_limbs(R), []
        for k in range(2, v):
            row = _tree_row(k)
            layers.append(([from_limbs(C[row + j])[4 - int(L[row + j]):] for j in range(k)], rs[row:row + k], tuple(from_limbs(E[k - 2]))))
        return from_limbs(S), from_limbs(H), layers, from_limbs(Z), from_limbs(K)

    def _tree_verify_batch_device(self, fn, W, name, d_tables, n, batch, H, C, L, R, E, claimed):
        shapes = self._tree_shapes(W, n, (batch,))
        H, C, R, E = (np.ascontiguousarray(a, dtype=np.uint64) for a in (H, C, R, E))
        L = np.ascontiguousarray(L, dtype=np.uint32)
        if [a.shape for a in (H, C, L, R, E)] != shapes[1:6]:
            raise GkrError(N.GKR_ERR_INVALID, "proof arrays do not match (batch, n)")
        if claimed is not None:
            claimed = np.ascontiguousarray(claimed, dtype=np.uint64)
            if claimed.shape != shapes[0]:
                raise GkrError(N.GKR_ERR_INVALID, "%s of shape (%s) expected" % (name, ", ".join(["batch"] + [str(x) for x in shapes[0][1:]])))
        accept = np.zeros(batch, dtype=np.int32)
        layer, rnd, check = (np.zeros(batch, dtype=np.uint32) for _ in range(3))
        out = np.zeros(shapes[0], dtype=np.uint64)
        self._check(fn(self._h, d_tables, n, batch, _ptr(claimed) if claimed is not None else None, _ptr(H), _ptr(C), _ptr(L), _ptr(R), _ptr(E),
                       _ptr(accept), _ptr(layer), _ptr(rnd), _ptr(check), _ptr(out)))
        return accept.astype(bool), layer, rnd, check, out

    def _tree_verify(self, fn, W, tables, head, layers, claimed):
        """fn(ctx, *tables, n, claimed or None, the proof, the verdict's four outputs) -> (check, layer, round)"""
        n = len(layers) + 2
        _, _, cs, ls, rs, es, _, _ = self._tree_shapes(W, n, ())
        C, L, R, E = np.zeros(cs, dtype=np.uint64), np.zeros(ls, dtype=np.uint32), np.zeros(rs, dtype=np.uint64), np.zeros(es, dtype=np.uint64)
        for k, (proof, r, vals) in enumerate(layers, start=2):
            row = _tree_row(k)
            if len(proof) != k or len(r) != k or len(vals) != 2 * W:
                raise GkrError(N.GKR_ERR_INVALID, "layer k has k round vectors, k challenges and %s values" % ("two", "four")[W - 1])
            for j, g in enumerate(proof):
                L[row + j] = len(g)
                if 1 <= len(g) <= 4:                                       # (another length: SHAPE, the slots are not read)
                    C[row + j, 4 - len(g):] = to_limbs([int(c) for c in g])
            R[row:row + k] = to_limbs([int(x) for x in r])
            E[k - 2] = to_limbs([int(x) for x in vals])
        H = to_limbs([int(x) for x in head])
        cl = to_limbs([int(x) for x in claimed]) if claimed is not None else None
        accept = ctypes.c_int(0)
        layer, rnd, check = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(fn(self._h, *(_ptr(t) for t in tables), n, _ptr(cl) if cl is not None else None, _ptr(H), _ptr(C), _ptr(L), _ptr(R), _ptr(E),
                       ctypes.byref(accept), ctypes.byref(layer), ctypes.byref(rnd), ctypes.byref(check)))
        return int(check.value), int(layer.value), int(rnd.value)

    # -- the grand product P = prod_i V[i]: the product tree on the device, a zero-check per layer, chained by Fiat-Shamir
    @staticmethod
    def grand_product_rounds(n):
        """R = n (n - 1) / 2 - 1: the rounds of the layers k = 2 .. n - 1 of a grand product over 2^n values; layer k's rows start
        at k (k - 1) / 2 - 1."""
        return _tree_rounds(n)

    def grand_product_batch_device(self, d_tables, n, batch, out=None):
        """gkr_grand_product_batch_device: `batch` grand products over resident tables of 2^n canonical values (table b at
        d_tables + b * 2^n elements; not modified), n >= 3.  -> (P, H, C, L, R, E, Z, K): P (batch, 4) the products; H (batch, 4, 4)
        the heads L_2; C (batch, R, 4, 4) the layers' right-aligned round vectors, layers k = 2 .. n - 1 in order,
        R = grand_product_rounds(n); L (batch, R); R (batch, R, 4) the challenges; E (batch, n - 2, 2, 4) the layers' values
        (a_k, b_k); Z (batch, n, 4) the final point z^(n); K (batch, 4) the final claim c_n = V~(z^(n)).  Each layer is byte for
        byte sumcheck_zerocheck_batch_device on the two halves of the level below.  out: the eight arrays of an earlier call."""
        return self._tree_batch_device(N.lib().gkr_grand_product_batch_device, 1, d_tables, n, batch, out)

    def prove_grand_product(self, table, v):
        """The grand product of a table of 2^v values (v >= 3) with its GKR proof.  -> (product, head, layers, point, claim):
        head = L_2 (four values, product = their product); layers[k - 2] = (proof, r, (a_k, b_k)) of the zero-check of layer
        k = 2 .. v - 1 (proof[j] the round vector's used slots, highest degree first); point = z^(v) and claim = c_v, the
        evaluation of the table the proof leaves.  verifier.verify_grand_product checks it on plain integers."""
        limbs = as_limbs(table)
        if v < 3 or limbs.shape[0] != 1 << v:
            raise GkrError(N.GKR_ERR_INVALID, "a table of 2^v values, v >= 3, expected")
        P, head, layers, point, K = self._tree_prove(N.lib().gkr_grand_product, 1, (limbs,), v)
        return P[0], head, layers, point, K[0]

    def verify_grand_product_batch_device(self, d_tables, n, batch, H, C, L, R, E, products=None):
        """gkr_grand_product_verify_batch_device on the resident tables and the arrays grand_product_batch_device returned (its H,
        C, L, R, E); products: (batch, 4) limbs of claimed products or None.  -> (accept (batch,) bool, failed_layer, failed_round,
        failed_check (batch,) uint32, products (batch, 4): the heads' own products).  verifier.verify_grand_product is the same
        verdict on plain integers."""
        return self._tree_verify_batch_device(N.lib().gkr_grand_product_verify_batch_device, 1, "products", d_tables, n, batch, H, C, L, R, E, products)

    def verify_grand_product(self, table, head, layers, product=None):
        """gkr_grand_product_verify on a host table and what prove_grand_product returned (its head and layers; product: the claimed
        product or None).  -> (check, layer, round), (0, 0, 0) for an accepted proof: verifier.verify_grand_product's verdict."""
        limbs = as_limbs(table)
        if limbs.shape[0] != 1 << (len(layers) + 2) or len(head) != 4:
            raise GkrError(N.GKR_ERR_INVALID, "a table of 2^n values, four head values and n - 2 layers expected")
        return self._tree_verify(N.lib().gkr_grand_product_verify, 1, (limbs,), head, layers, None if product is None else [product])

    # -- the fractional sum (LogUp) sum_i N[i] / D[i] = P / Q: the tree of fractions on the device, a zero-check per layer
    @staticmethod
    def fraction_sum_rounds(n):
        """R = n (n - 1) / 2 - 1: the rounds of the layers k = 2 .. n - 1 of a fractional sum over 2^n fractions; layer k's rows
        start at k (k - 1) / 2 - 1 (the grand product's bookkeeping)."""
        return _tree_rounds(n)

    def fraction_sum_batch_device(self, d_tables, n, batch, out=None):
        """gkr_fraction_sum_batch_device: `batch` fractional sums over resident pairs of tables of 2^n canonical values (pair b:
        N at d_tables + 2 b 2^n elements, D at + (2 b + 1) 2^n; not modified), n >= 3.  -> (S, H, C, L, R, E, Z, K): S (batch, 2, 4)
        the sums (P, Q); H (batch, 8, 4) the heads p_2, q_2; C (batch, R, 4, 4) the layers' right-aligned round vectors, layers
        k = 2 .. n - 1 in order, R = fraction_sum_rounds(n); L (batch, R); R (batch, R, 4) the challenges; E (batch, n - 2, 4, 4) the
        layers' values (a0, a1, b0, b1); Z (batch, n, 4) the final point z^(n); K (batch, 2, 4) the final claims cp_n = N~(z^(n)),
        cq_n = D~(z^(n)).  out: the eight arrays of an earlier call."""
        return self._tree_batch_device(N.lib().gkr_fraction_sum_batch_device, 2, d_tables, n, batch, out)

    def prove_fraction_sum(self, numerators, denominators, v):
        """The fractional sum of 2^v fractions N[i] / D[i] (v >= 3) with its GKR proof.  -> ((P, Q), head, layers, point, claims):
        head = p_2 then q_2 (eight values, (P, Q) their root); layers[k - 2] = (proof, r, (a0, a1, b0, b1)) of the zero-check of
        layer k = 2 .. v - 1 (proof[j] the round vector's used slots, highest degree first); point = z^(v) and claims = (cp_v, cq_v),
        the evaluations of N and D the proof leaves.  verifier.verify_fraction_sum checks it on plain integers."""
        num, den = as_limbs(numerators), as_limbs(denominators)
        if v < 3 or num.shape[0] != 1 << v or den.shape[0] != 1 << v:
            raise GkrError(N.GKR_ERR_INVALID, "two tables of 2^v values, v >= 3, expected")
        S, head, layers, point, K = self._tree_prove(N.lib().gkr_fraction_sum, 2, (num, den), v)
        return tuple(S), head, layers, point, tuple(K)

    def verify_fraction_sum_batch_device(self, d_tables, n, batch, H, C, L, R, E, sums=None):
        """gkr_fraction_sum_verify_batch_device on the resident pairs and the arrays fraction_sum_batch_device returned (its H, C,
        L, R, E); sums: (batch, 2, 4) limbs of claimed (P, Q) or None.  -> (accept (batch,) bool, failed_layer, failed_round,
        failed_check (batch,) uint32, sums (batch, 2, 4): the heads' own roots).  verifier.verify_fraction_sum is the same verdict
        on plain integers."""
        return self._tree_verify_batch_device(N.lib().gkr_fraction_sum_verify_batch_device, 2, "sums", d_tables, n, batch, H, C, L, R, E, sums)

    def verify_fraction_sum(self, numerators, denominators, head, layers, sums=None):
        """gkr_fraction_sum_verify on host tables and what prove_fraction_sum returned (its head and layers; sums: the claimed (P, Q)
        or None).  -> (check, layer, round), (0, 0, 0) for an accepted proof: verifier.verify_fraction_sum's verdict."""
        num, den = as_limbs(numerators), as_limbs(denominators)
        n = len(layers) + 2
        if num.shape[0] != 1 << n or den.shape[0] != 1 << n or len(head) != 8:
            raise GkrError(N.GKR_ERR_INVALID, "two tables of 2^n values, eight head values and n - 2 layers expected")
        return self._tree_verify(N.lib().gkr_fraction_sum_verify, 2, (num, den), head, layers, sums)

    # -- the lookup (LogUp with multiplicities): every witness value lies in the table iff the fractional sum of the pair
    # (1, alpha - W) | (-M, alpha - T) is zero; multiplicities and pair are built on the device, the proof is the fractional sum's
    @staticmethod
    def lookup_pair_log2(n_w, n_t):
        """L = max(n_w, n_t) + 1: the pair of a lookup has 2^L entries, its proof is a fractional sum's with n = L."""
        return max(n_w, n_t) + 1

    @staticmethod
    def _alphas(alpha, batch):
        a = np.ascontiguousarray(alpha if isinstance(alpha, np.ndarray) else to_limbs([int(x) for x in alpha]), dtype=np.uint64)
        if a.shape != (batch, 4):
            raise GkrError(N.GKR_ERR_INVALID, "one alpha per column expected")
        return a

    def lookup_multiplicities_device(self, d_witness, n_w, d_table, n_t, shared_table, batch, d_mult):
        """gkr_lookup_multiplicities_device: the multiplicities of `batch` resident witness columns of 2^n_w values in their tables of
        2^n_t values (one table for all with shared_table), written to d_mult (batch x 2^n_t elements on the device); the lowest
        index of a repeated table value takes the whole count.  -> (missing, first_missing), (batch,) uint32 each: the entries of a
        column that are not in its table and the lowest such index (0xFFFFFFFF: none)."""
        if batch < 1:
            raise GkrError(N.GKR_ERR_INVALID, "batch >= 1 expected")
        missing, first = np.zeros(batch, dtype=np.uint32), np.zeros(batch, dtype=np.uint32)
        self._check(N.lib().gkr_lookup_multiplicities_device(self._h, d_witness, n_w, d_table, n_t, int(bool(shared_table)), batch, d_mult,
                                                             _ptr(missing), _ptr(first)))
        return missing, first

    def lookup_batch_device(self, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, out=None):
        """gkr_lookup_batch_device: the pairs of `batch` lookups built on the device from W, T, d_mult and alpha (batch integers, or
        (batch, 4) limbs), then their fractional sums.  -> fraction_sum_batch_device's (S, H, C, L, R, E, Z, K) with
        n = lookup_pair_log2(n_w, n_t), byte for byte what that call returns on the same pairs; S[b] = (0, Q) where the lookup holds."""
        a = self._alphas(alpha, batch)
        fn = lambda h, d, n, b, *outs: N.lib().gkr_lookup_batch_device(h, d, n_w, d_table, n_t, int(bool(shared_table)), d_mult, _ptr(a), b, *outs)
        return self._tree_batch_device(fn, 2, d_witness, self.lookup_pair_log2(n_w, n_t), batch, out)

    def verify_lookup_batch_device(self, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, H, C, L, R, E):
        """gkr_lookup_verify_batch_device on the resident tables, d_mult, alpha and the arrays lookup_batch_device returned (its H, C,
        L, R, E).  -> (accept (batch,) bool, failed_layer, failed_round, failed_check (batch,) uint32, sums (batch, 2, 4): the heads'
        roots): the fractional sum's verdict on the rebuilt pair, and GKR_VERIFY_LOOKUP at (0, 0) for a head whose P is not 0.
        verifier.verify_lookup is the same verdict on plain integers."""
        a = self._alphas(alpha, batch)
        fn = lambda h, d, n, b, claimed, *rest: N.lib().gkr_lookup_verify_batch_device(h, d, n_w, d_table, n_t, int(bool(shared_table)), d_mult, _ptr(a),
                                                                                      b, *rest)
        return self._tree_verify_batch_device(fn, 2, "sums", d_witness, self.lookup_pair_log2(n_w, n_t), batch, H, C, L, R, E, None)

    @staticmethod
    def _lookup_tables(witness, table):
        w, t = as_limbs(witness), as_limbs(table)
        n_w, n_t = w.shape[0].bit_length() - 1, t.shape[0].bit_length() - 1
        if n_w < 2 or n_t < 2 or w.shape[0] != 1 << n_w or t.shape[0] != 1 << n_t:
            raise GkrError(N.GKR_ERR_INVALID, "a witness of 2^n_w and a table of 2^n_t values, n_w, n_t >= 2, expected")
        return w, n_w, t, n_t

    def prove_lookup(self, witness, table, alpha):
        """gkr_lookup: the multiplicities of the witness in the table and the proof that, with them, every witness value lies in the
        table.  -> (mult, (missing, first_missing), (P, Q), head, layers, point, claims): mult the 2^n_t multiplicities, the rest
        prove_fraction_sum's result on the lookup's pair; P = 0 where the lookup holds.  alpha is taken before the multiplicities
        exist: a convenience, not a sound composition (include/gkr_amd.h).  verifier.verify_lookup checks it on plain integers."""
        w, n_w, t, n_t = self._lookup_tables(witness, table)
        a = to_limbs([int(alpha)])
        M, miss, first = np.zeros((1 << n_t, 4), dtype=np.uint64), ctypes.c_uint32(0), ctypes.c_uint32(0)
        fn = lambda h, pw, v, *outs: N.lib().gkr_lookup(h, pw, n_w, _ptr(t), n_t, _ptr(a), _ptr(M), ctypes.byref(miss), ctypes.byref(first), *outs)
        S, head, layers, point, K = self._tree_prove(fn, 2, (w,), self.lookup_pair_log2(n_w, n_t))
        return from_limbs(M), (int(miss.value), int(first.value)), tuple(S), head, layers, point, tuple(K)

    def verify_lookup(self, witness, table, mult, alpha, head, layers):
        """gkr_lookup_verify on host tables and what prove_lookup returned (its mult, head and layers).  -> (check, layer, round),
        (0, 0, 0) for an accepted proof: verifier.verify_lookup's verdict."""
        w, n_w, t, n_t = self._lookup_tables(witness, table)
        m, a = as_limbs(mult), to_limbs([int(alpha)])
        if m.shape[0] != 1 << n_t or len(head) != 8 or len(layers) + 2 != self.lookup_pair_log2(n_w, n_t):
            raise GkrError(N.GKR_ERR_INVALID, "2^n_t multiplicities, eight head values and max(n_w, n_t) - 1 layers expected")
        fn = lambda h, pw, n, claimed, *rest: N.lib().gkr_lookup_verify(h, pw, n_w, _ptr(t), n_t, _ptr(m), _ptr(a), *rest)
        return self._tree_verify(fn, 2, (w,), head, layers, None)

    # -- the R1CS zero-check: Az, Bz, Cz of resident witnesses built on the device, then eq(z, .) (A B - C)
    def r1cs_rows(self, r1cs) -> R1csRows:
        """gkr_r1cs_rows_prepare: the CSR form of `r1cs` (convert.R1cs) resident on this context's device."""
        h = ctypes.c_void_p()
        self._check(N.lib().gkr_r1cs_rows_prepare(self._h, r1cs._h, ctypes.byref(h)))
        return R1csRows(self, h)

    def r1cs_rows_device(self, rows, d_witness, batch, d_out, stride=None, check=True):
        """gkr_r1cs_rows_device: the tables Az, Bz, Cz of `batch` resident witnesses (witness b: n_wires canonical elements at
        d_witness + b * stride elements; None: n_wires) into d_out, table m of witness b at (b * 3 + m) * 2^n elements, rows past
        n_constraints zero.  -> first_bad (batch,) uint32: the lowest constraint with a * b != c or 0xFFFFFFFF; None without check."""
        inf = rows.info()
        bad = np.zeros(max(int(batch), 0), dtype=np.uint32) if check else None
        self._check(N.lib().gkr_r1cs_rows_device(self._h, rows._h, d_witness, inf["n_wires"] if stride is None else int(stride), batch, d_out,
                                                 _ptr(bad) if check else None))
        return bad

    def r1cs_zerocheck_batch_device(self, rows, d_witness, batch, z, stride=None):
        """gkr_r1cs_zerocheck_batch_device: the tables of `batch` resident witnesses (as r1cs_rows_device lays them out, in context
        workspace), then the zero-check eq(z_b, .) (A B - C) with verifier.R1CS_ZEROCHECK_TERMS.  z: (batch, n, 4) limbs or `batch`
        lists of n integers.  -> (C, L, R, E, Q, first_bad): the first five are sumcheck_zerocheck_batch_device's on those tables
        (C (batch, n, 4, 4)), first_bad as r1cs_rows_device returns it.  An unsatisfied witness is not an error: its claim
        g_1(0) + g_1(1) is non-zero."""
        inf = rows.info()
        n = inf["n"]
        pts = self._points(z, batch, n)
        C = np.zeros((batch, n, 4, 4), dtype=np.uint64)
        L = np.zeros((batch, n), dtype=np.uint32)
        R = np.zeros((batch, n, 4), dtype=np.uint64)
        E = np.zeros((batch, 3, 4), dtype=np.uint64)
        Q = np.zeros((batch, 4), dtype=np.uint64)
        bad = np.zeros(batch, dtype=np.uint32)
        self._check(N.lib().gkr_r1cs_zerocheck_batch_device(self._h, rows._h, d_witness, inf["n_wires"] if stride is None else int(stride), batch,
                                                            _ptr(pts), _ptr(C), _ptr(L), _ptr(R), _ptr(E), _ptr(Q), _ptr(bad)))
        return C, L, R, E, Q, bad

    def prove_r1cs_zerocheck(self, r1cs, witness, z):
        """gkr_r1cs_zerocheck: the zero-check of one host witness (a list of at least n_wires integers) of `r1cs` at the point z of
        n = r1cs.csr_info()["n"] integers (or (1, n, 4) limbs; the witness may be (count, 4) limbs too).  -> (proof, r, evals, eq_r, first_bad): proof[j] the round vector (its used slots, highest
        degree first), r the challenges, evals = [Az~(r), Bz~(r), Cz~(r)], eq_r = eq(z, r), first_bad the lowest constraint the
        witness breaks or None.  verifier.verify_sumcheck_zerocheck(proof, r, evals, R1CS_ZEROCHECK_TERMS, z, 0) accepts a satisfied
        witness's transcript; the claims on evals are left to the caller."""
        n = r1cs.csr_info()["n"]
        wl = as_limbs(witness)
        pts = self._points(z if isinstance(z, np.ndarray) else [z], 1, n)      # (limbs: a (1, n, 4) array, passed as it is)
        C = np.zeros((n, 4, 4), dtype=np.uint64)
        L = np.zeros(n, dtype=np.uint32)
        R = np.zeros((n, 4), dtype=np.uint64)
        E = np.zeros((3, 4), dtype=np.uint64)
        Q = np.zeros((1, 4), dtype=np.uint64)
        bad = np.zeros(1, dtype=np.uint32)
        self._check(N.lib().gkr_r1cs_zerocheck(self._h, r1cs._h, _ptr(wl), wl.shape[0], _ptr(pts), _ptr(C), _ptr(L), _ptr(R), _ptr(E), _ptr(Q),
                                               _ptr(bad)))
        return ([from_limbs(C[j])[4 - int(L[j]):] for j in range(n)], from_limbs(R), from_limbs(E), from_limbs(Q)[0],
                None if int(bad[0]) == 0xFFFFFFFF else int(bad[0]))

    # -- the R1CS inner sumcheck: the zero-check's claims on Az, Bz, Cz at r_x reduced to one claim on the witness
    def r1cs_cols(self, r1cs, segment=None) -> R1csCols:
        """gkr_r1cs_cols_prepare: the column-major form of `r1cs` (convert.R1cs) resident on this context's device.  segment: long
        columns cut into segments of at most this many records instead of GKR_R1CS_COL_SEGMENT (0: no cut;
        gkr_r1cs_cols_prepare_segment, for measurements -- results do not depend on it)."""
        h = ctypes.c_void_p()
        if segment is None:
            self._check(N.lib().gkr_r1cs_cols_prepare(self._h, r1cs._h, ctypes.byref(h)))
        else:
            self._check(N.lib().gkr_r1cs_cols_prepare_segment(self._h, r1cs._h, int(segment), ctypes.byref(h)))
        return R1csCols(self, h)

    @staticmethod
    def _rho(rho, batch):
        """rho as (batch, 3, 4) limbs: such an array, or `batch` triples of integers (reduced modulo r)."""
        if isinstance(rho, np.ndarray) and rho.dtype == np.uint64:
            out = np.ascontiguousarray(rho)
        else:
            out = to_limbs([int(v) % MODULUS for row in rho for v in row]).reshape(-1, 3, 4) if len(rho) else np.zeros((0, 3, 4), dtype=np.uint64)
        if out.shape != (batch, 3, 4):
            raise GkrError(N.GKR_ERR_INVALID, "weights of shape (batch, 3, 4) expected")
        return out

    def r1cs_cols_device(self, cols, x, rho, batch, d_out, stride=None):
        """gkr_r1cs_cols_device: the tables T_b(y) = sum_m rho_{b,m} sum_i M_m[i][y] eq(x_b, i) of `batch` sumchecks into d_out,
        table b at d_out + b * stride elements (None: 2^n_y), zero for y >= n_wires.  x: (batch, n_x, 4) limbs or `batch` lists of
        n_x integers; rho: (batch, 3, 4) limbs or `batch` triples."""
        inf = cols.info()
        pts = self._points(x, batch, inf["n_x"])
        self._check(N.lib().gkr_r1cs_cols_device(self._h, cols._h, _ptr(pts), _ptr(self._rho(rho, batch)), batch, d_out,
                                                 (1 << inf["n_y"]) if stride is None else int(stride)))

    def r1cs_inner_batch_device(self, cols, d_witness, batch, x, rho, stride=None):
        """gkr_r1cs_inner_batch_device: the tables {T_b, w_b zero-padded to 2^n_y} of `batch` resident witnesses (witness b: n_wires
        canonical elements at d_witness + b * stride elements; None: n_wires) in context workspace, then the product sumcheck at
        degree 2 on them.  -> (C, L, R, E): sumcheck_product_batch_device's on those tables -- C (batch, n_y, 3, 4), L (batch, n_y),
        R (batch, n_y, 4), E (batch, 2, 4) = T_b~(r_y), w_b~(r_y)."""
        inf = cols.info()
        n_y = inf["n_y"]
        pts = self._points(x, batch, inf["n_x"])
        C = np.zeros((batch, n_y, 3, 4), dtype=np.uint64)
        L = np.zeros((batch, n_y), dtype=np.uint32)
        R = np.zeros((batch, n_y, 4), dtype=np.uint64)
        E = np.zeros((batch, 2, 4), dtype=np.uint64)
        self._check(N.lib().gkr_r1cs_inner_batch_device(self._h, cols._h, d_witness, inf["n_wires"] if stride is None else int(stride), batch,
                                                        _ptr(pts), _ptr(self._rho(rho, batch)), _ptr(C), _ptr(L), _ptr(R), _ptr(E)))
        return C, L, R, E

    def prove_r1cs_inner(self, r1cs, witness, x, rho):
        """gkr_r1cs_inner: the inner sumcheck of one host witness (at least n_wires integers, or (count, 4) limbs) of `r1cs` at the
        point x of n_x = r1cs.csc_info()["n_x"] integers -- the zero-check's challenges -- with the weights rho = (rho_A, rho_B,
        rho_C).  -> (proof, r, evals): proof[j] the round vector (its used slots, highest degree first), r the n_y challenges,
        evals = [T~(r), w~(r)].  verifier.verify_r1cs_inner(r1cs.constraints(), x, rho, claims_abc, proof, r, evals) checks it
        against the zero-check's claims and the public matrices and returns the claim left on the witness."""
        inf = r1cs.csc_info()
        n_y = inf["n_y"]
        wl = as_limbs(witness)
        pts = self._points(x if isinstance(x, np.ndarray) else [x], 1, inf["n_x"])
        rh = self._rho(rho if isinstance(rho, np.ndarray) else [rho], 1)
        C = np.zeros((n_y, 3, 4), dtype=np.uint64)
        L = np.zeros(n_y, dtype=np.uint32)
        R = np.zeros((n_y, 4), dtype=np.uint64)
        E = np.zeros((2, 4), dtype=np.uint64)
        self._check(N.lib().gkr_r1cs_inner(self._h, r1cs._h, _ptr(wl), wl.shape[0], _ptr(pts), _ptr(rh), _ptr(C), _ptr(L), _ptr(R), _ptr(E)))
        return [from_limbs(C[j])[3 - int(L[j]):] for j in range(n_y)], from_limbs(R), from_limbs(E)

    # -- the R1CS verifier: the two transcripts against z, rho, the public matrices and, where there is one, the witness
    @staticmethod
    def _n_y(rows_info):
        """n_y = max(2, ceil(log2 n_wires)) from a rows handle's info (the CSC info's rule)."""
        return max(2, (rows_info["n_wires"] - 1).bit_length())

    def r1cs_matrix_evals_device(self, rows, xs, ys):
        """gkr_r1cs_matrix_evals_device: [A~, B~, C~](x_b, y_b) of the R1CS behind `rows` for a batch of points, one pass over its
        non-zeros on the device.  xs: (batch, n, 4) limbs or `batch` lists of n integers; ys: the same with n_y coordinates.
        -> (batch, 3, 4) uint64 limbs, value for value verifier.r1cs_matrix_evals(constraints, x_b, y_b)."""
        inf = rows.info()
        batch = len(xs)
        px, py = self._points(xs, batch, inf["n"]), self._points(ys, batch, self._n_y(inf))
        out = np.zeros((batch, 3, 4), dtype=np.uint64)
        self._check(N.lib().gkr_r1cs_matrix_evals_device(self._h, rows._h, _ptr(px), _ptr(py), batch, _ptr(out)))
        return out

    def verify_r1cs_batch_device(self, rows, batch, z, zerocheck, rho, inner, d_witness=None, stride=None):
        """gkr_r1cs_verify_batch_device: `batch` proofs of the two R1CS sumchecks against the R1CS behind `rows`.  z: (batch, n, 4)
        limbs or `batch` lists of n integers; zerocheck = (C, L, R, E) as r1cs_zerocheck_batch_device returns them (its first four
        arrays); rho: (batch, 3, 4) limbs or `batch` triples; inner = (C, L, R, E) as r1cs_inner_batch_device returns them.
        d_witness: None, or the resident witnesses (witness b at d_witness + b * stride elements; None: n_wires) -- without one the
        claim (r_y, e_w) on the witness is left to the caller.  -> (accept, failed_stage, failed_round, failed_check), (batch,)
        arrays; verifier.verify_r1cs is the same verdict on plain integers."""
        inf = rows.info()
        n, n_y = inf["n"], self._n_y(inf)
        pts, rh = self._points(z, batch, n), self._rho(rho, batch)
        CX, LX, RX, EX = (np.ascontiguousarray(a) for a in zerocheck)
        CY, LY, RY, EY = (np.ascontiguousarray(a) for a in inner)
        want = [(CX, (batch, n, 4, 4), np.uint64), (LX, (batch, n), np.uint32), (RX, (batch, n, 4), np.uint64), (EX, (batch, 3, 4), np.uint64),
                (CY, (batch, n_y, 3, 4), np.uint64), (LY, (batch, n_y), np.uint32), (RY, (batch, n_y, 4), np.uint64), (EY, (batch, 2, 4), np.uint64)]
        if any(a.shape != shape or a.dtype != dtype for a, shape, dtype in want):
            raise GkrError(N.GKR_ERR_INVALID, "transcript arrays do not match (batch, n, n_y)")
        accept = np.zeros(batch, dtype=np.int32)
        stage, rnd, check = (np.zeros(batch, dtype=np.uint32) for _ in range(3))
        self._check(N.lib().gkr_r1cs_verify_batch_device(self._h, rows._h, batch, _ptr(pts), _ptr(CX), _ptr(LX), _ptr(RX), _ptr(EX), _ptr(rh), _ptr(CY),
                                                         _ptr(LY), _ptr(RY), _ptr(EY), d_witness,
                                                         (inf["n_wires"] if stride is None else int(stride)) if d_witness else 0, _ptr(accept),
                                                         _ptr(stage), _ptr(rnd), _ptr(check)))
        return accept, stage, rnd, check

    def verify_r1cs(self, r1cs, z, rho, proof_x, proof_y, witness=None):
        """gkr_r1cs_verify: one proof against `r1cs` (convert.R1cs) and, where given, a host witness (at least n_wires integers, or
        (count, 4) limbs).  z: n integers; rho: three; proof_x = (proof, r, evals) of prove_r1cs_zerocheck (its first three
        results); proof_y = (proof, r, evals) of prove_r1cs_inner.  -> (stage, round, check), (0, 0, 0) for an accepted proof:
        verifier.verify_r1cs's verdict."""
        inf = r1cs.csr_info()
        n, n_y = inf["n"], self._n_y(inf)

        def rows_of(proof, width, count):
            if len(proof) != count:
                raise GkrError(N.GKR_ERR_INVALID, "a transcript has one round vector per variable")
            C, L = np.zeros((count, width, 4), dtype=np.uint64), np.zeros(count, dtype=np.uint32)
            for j, g in enumerate(proof):
                L[j] = len(g)
                if 1 <= len(g) <= width:                                   # (another length: SHAPE, the slots are not read)
                    C[j, width - len(g):] = to_limbs([int(c) for c in g])
            return C, L
        (gx, rx, ex), (gy, ry, ey) = proof_x, proof_y
        CX, LX = rows_of(gx, 4, n)
        CY, LY = rows_of(gy, 3, n_y)
        RX, EX, RY, EY = to_limbs(list(rx)), to_limbs(list(ex)), to_limbs(list(ry)), to_limbs(list(ey))
        if RX.shape != (n, 4) or EX.shape != (3, 4) or RY.shape != (n_y, 4) or EY.shape != (2, 4):
            raise GkrError(N.GKR_ERR_INVALID, "n and n_y challenges, three and two evaluations expected")
        pts = self._points(z if isinstance(z, np.ndarray) else [z], 1, n)
        rh = self._rho(rho if isinstance(rho, np.ndarray) else [rho], 1)
        wl = None if witness is None else as_limbs(witness)
        accept = np.zeros(1, dtype=np.int32)
        stage, rnd, check = (np.zeros(1, dtype=np.uint32) for _ in range(3))
        self._check(N.lib().gkr_r1cs_verify(self._h, r1cs._h, _ptr(pts), _ptr(CX), _ptr(LX), _ptr(RX), _ptr(EX), _ptr(rh), _ptr(CY), _ptr(LY),
                                            _ptr(RY), _ptr(EY), None if wl is None else _ptr(wl), 0 if wl is None else wl.shape[0],
                                            _ptr(accept), _ptr(stage), _ptr(rnd), _ptr(check)))
        return int(stage[0]), int(rnd[0]), int(check[0])

    # -- the plain sumcheck's verifier (verify_sumcheck, python/sumcheck.py:55-70, plus g_n(r_n) = T(r)) and the evaluation behind it
    def mle_eval_batch_device(self, d_tables, n, batch, points):
        """gkr_mle_eval_batch_device: the multilinear extension of each of `batch` resident tables of 2^n entries at its own point.
        points: (batch, n, 4) uint64 limbs (canonical; GkrError GKR_ERR_NON_CANONICAL otherwise), variable 1 = most significant
        index bit.  -> (batch, 4) uint64 limbs."""
        points = np.ascontiguousarray(points, dtype=np.uint64)
        if points.shape != (batch, n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "points of shape (batch, n, 4) expected")
        out = np.zeros((batch, 4), dtype=np.uint64)
        self._check(N.lib().gkr_mle_eval_batch_device(self._h, d_tables, ctypes.c_int(n), ctypes.c_int(batch), _ptr(points), _ptr(out)))
        return out

    def verify_sumcheck_batch_device(self, d_tables, n, batch, C, L, R, claims=None):
        """gkr_sumcheck_mle_verify_batch_device on the arrays sumcheck_mle_batch_device returned (C (batch, n, 2, 4), L (batch, n),
        R (batch, n, 4)); claims: (batch, 4) uint64 limbs or None (round 0's sum check is skipped, the proven sums are returned).
        -> (accept (batch,) bool, failed_round (batch,) uint32, failed_check (batch,) uint32, claims (batch, 4) uint64)."""
        C = np.ascontiguousarray(C, dtype=np.uint64)
        L = np.ascontiguousarray(L, dtype=np.uint32)
        R = np.ascontiguousarray(R, dtype=np.uint64)
        if C.shape != (batch, n, 2, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "transcript arrays do not match (batch, n)")
        if claims is not None:
            claims = np.ascontiguousarray(claims, dtype=np.uint64)
            if claims.shape != (batch, 4):
                raise GkrError(N.GKR_ERR_INVALID, "claims of shape (batch, 4) expected")
        accept = np.zeros(batch, dtype=np.int32)
        rnd, check = np.zeros(batch, dtype=np.uint32), np.zeros(batch, dtype=np.uint32)
        out = np.zeros((batch, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_mle_verify_batch_device(
            self._h, d_tables, ctypes.c_int(n), ctypes.c_int(batch), _ptr(claims) if claims is not None else None, _ptr(C), _ptr(L), _ptr(R),
            _ptr(accept), _ptr(rnd), _ptr(check), _ptr(out)))
        return accept.astype(bool), rnd, check, out

    def verify_sumcheck(self, table, proof, r, claim=None):
        """gkr_sumcheck_mle_verify on what prove_sumcheck returned: proof[j] the round vector (one or two coefficients, highest
        degree first), r the challenges; claim: the sum the transcript is to prove, or None.  -> (accept, failed_round, failed_check)."""
        limbs = as_limbs(table)
        n = len(proof)
        if n < 1 or limbs.shape[0] != 1 << n or len(r) != n:
            raise GkrError(N.GKR_ERR_INVALID, "a table of 2^n entries, n round vectors and n challenges expected")
        C = np.zeros((n, 2, 4), dtype=np.uint64)
        L = np.zeros(n, dtype=np.uint32)
        for j, g in enumerate(proof):
            if not 1 <= len(g) <= 2:
                raise GkrError(N.GKR_ERR_INVALID, "a round vector has one or two coefficients")
            L[j] = len(g)
            C[j, 2 - len(g):] = to_limbs(g)
        R = to_limbs(r)
        cl = to_limbs([claim]) if claim is not None else None
        accept, rnd, check = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(N.lib().gkr_sumcheck_mle_verify(self._h, _ptr(limbs), ctypes.c_int(n), _ptr(cl) if cl is not None else None, _ptr(C), _ptr(L),
                                                    _ptr(R), ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check)))
        return bool(accept.value), int(rnd.value), int(check.value)

    # -- the product sumcheck's verifier: the same checks on rows of degree + 1 slots, g_n(r_n) = prod_f T_f~(r)
    def verify_sumcheck_product_batch_device(self, d_tables, n, degree, batch, C, L, R, claims=None):
        """gkr_sumcheck_product_verify_batch_device on the resident tables and the arrays sumcheck_product_batch_device returned (C
        (batch, n, degree + 1, 4), L (batch, n), R (batch, n, 4)); claims: (batch, 4) uint64 limbs or None (round 0's sum check
        is skipped, the proven sums are returned).  -> (accept (batch,) bool, failed_round (batch,) uint32, failed_check (batch,)
        uint32, claims (batch, 4) uint64, evals (batch, degree, 4) uint64: the tables' values at the challenges as computed here)."""
        C = np.ascontiguousarray(C, dtype=np.uint64)
        L = np.ascontiguousarray(L, dtype=np.uint32)
        R = np.ascontiguousarray(R, dtype=np.uint64)
        if degree < 1 or C.shape != (batch, n, degree + 1, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "transcript arrays do not match (batch, n, degree)")
        if claims is not None:
            claims = np.ascontiguousarray(claims, dtype=np.uint64)
            if claims.shape != (batch, 4):
                raise GkrError(N.GKR_ERR_INVALID, "claims of shape (batch, 4) expected")
        accept = np.zeros(batch, dtype=np.int32)
        rnd, check = np.zeros(batch, dtype=np.uint32), np.zeros(batch, dtype=np.uint32)
        out = np.zeros((batch, 4), dtype=np.uint64)
        evals = np.zeros((batch, degree, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_product_verify_batch_device(
            self._h, d_tables, n, degree, batch, _ptr(claims) if claims is not None else None, _ptr(C), _ptr(L), _ptr(R),
            _ptr(accept), _ptr(rnd), _ptr(check), _ptr(out), _ptr(evals)))
        return accept.astype(bool), rnd, check, out, evals

    def verify_sumcheck_product(self, tables, proof, r, claim=None):
        """gkr_sumcheck_product_verify on what prove_sumcheck_product returned: tables the 1 .. 3 factors, proof[j] the round
        vector (1 .. len(tables) + 1 coefficients, highest degree first), r the challenges; claim: the sum the transcript is to
        prove, or None.  -> (accept, failed_round, failed_check)."""
        degree, n = len(tables), len(proof)
        limbs = np.concatenate([as_limbs(t) for t in tables], axis=0) if degree else np.zeros((0, 4), dtype=np.uint64)
        if n < 1 or degree < 1 or limbs.shape[0] != degree << n or len(r) != n:
            raise GkrError(N.GKR_ERR_INVALID, "tables of 2^n entries each, n round vectors and n challenges expected")
        C = np.zeros((n, degree + 1, 4), dtype=np.uint64)
        L = np.zeros(n, dtype=np.uint32)
        for j, g in enumerate(proof):
            if not 1 <= len(g) <= degree + 1:
                raise GkrError(N.GKR_ERR_INVALID, "a round vector has 1 .. degree + 1 coefficients")
            L[j] = len(g)
            C[j, degree + 1 - len(g):] = to_limbs(g)
        R = to_limbs(r)
        cl = to_limbs([claim]) if claim is not None else None
        accept, rnd, check = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(N.lib().gkr_sumcheck_product_verify(self._h, _ptr(limbs), n, degree, _ptr(cl) if cl is not None else None, _ptr(C), _ptr(L),
                                                        _ptr(R), ctypes.byref(accept), ctypes.byref(rnd), ctypes.byref(check)))
        return bool(accept.value), int(rnd.value), int(check.value)

    # -- the sum-of-products sumcheck's verifier: the same checks on rows of D + 1 slots, g_n(r_n) = sum_k c_k prod_j T_t(k,j)~(r)
    def verify_sumcheck_sop_batch_device(self, d_tables, n, n_tables, terms, batch, C, L, R, claims=None):
        """gkr_sumcheck_sop_verify_batch_device on the resident tables, the terms ([(coeff, (table indices ..)), ..]) and the arrays
        sumcheck_sop_batch_device returned (C (batch, n, D + 1, 4), D the largest term degree; L (batch, n); R (batch, n, 4));
        claims: (batch, 4) uint64 limbs or None (round 0's sum check is skipped, the proven sums are returned; a zero-check passes
        zeros).  -> (accept (batch,) bool, failed_round (batch,) uint32, failed_check (batch,) uint32, claims (batch, 4) uint64,
        evals (batch, n_tables, 4) uint64: the tables' values at the challenges as computed here)."""
        arr, coeffs, D = self._sop_terms(terms, n_tables)
        C = np.ascontiguousarray(C, dtype=np.uint64)
        L = np.ascontiguousarray(L, dtype=np.uint32)
        R = np.ascontiguousarray(R, dtype=np.uint64)
        if n_tables < 1 or C.shape != (batch, n, D + 1, 4) or L.shape != (batch, n) or R.shape != (batch, n, 4):
            raise GkrError(N.GKR_ERR_INVALID, "transcript arrays do not match (batch, n, the largest term degree)")
        if claims is not None:
            claims = np.ascontiguousarray(claims, dtype=np.uint64)
            if claims.shape != (batch, 4):
                raise GkrError(N.GKR_ERR_INVALID, "claims of shape (batch, 4) expected")
        accept = np.zeros(batch, dtype=np.int32)
        rnd, check = np.zeros(batch, dtype=np.uint32), np.zeros(batch, dtype=np.uint32)
        out = np.zeros((batch, 4), dtype=np.uint64)
        evals = np.zeros((batch, n_tables, 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_sop_verify_batch_device(
            self._h, d_tables, n, n_tables, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs), len(terms), batch,
            _ptr(claims) if claims is not None else None, _ptr(C), _ptr(L), _ptr(R), _ptr(accept), _ptr(rnd), _ptr(check), _ptr(out), _ptr(evals)))
        return accept.astype(bool), rnd, check, out, evals

    def verify_sumcheck_sop(self, tables, terms, proof, r, claim=None):
        """gkr_sumcheck_sop_verify on what prove_sumcheck_sop returned: tables the 1 .. 8 tables, terms as the prover took them,
        proof[j] the round vector (1 .. D + 1 coefficients, highest degree first), r the challenges; claim: the sum the transcript
        is to prove, or None.  -> (accept, failed_round, failed_check)."""
        M, n = len(tables), len(proof)
        if not 1 <= M <= N.GKR_SOP_MAX_TABLES:
            raise GkrError(N.GKR_ERR_INVALID, "1 .. %d tables expected" % N.GKR_SOP_MAX_TABLES)
        arr, coeffs, D = self._sop_terms(terms, M)
        limbs = np.concatenate([as_limbs(t) for t in tables], axis=0)
        if n < 1 or limbs.shape[0] != M << n or len(r) != n:
            raise GkrError(N.GKR_ERR_INVALID, "tables of 2^n entries each, n round vectors and n challenges expected")
        C = np.zeros((n, D + 1, 4), dtype=np.uint64)
        L = np.zeros(n, dtype=np.uint32)
        for j, g in enumerate(proof):
            if not 1 <= len(g) <= D + 1:
                raise GkrError(N.GKR_ERR_INVALID, "a round vector has 1 .. D + 1 coefficients, D the largest term degree")
            L[j] = len(g)
            C[j, D + 1 - len(g):] = to_limbs(g)
        R = to_limbs(r)
        cl = to_limbs([claim]) if claim is not None else None
        accept, rnd, check = ctypes.c_int(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(N.lib().gkr_sumcheck_sop_verify(self._h, _ptr(limbs), n, M, ctypes.cast(arr, ctypes.c_void_p), _ptr(coeffs), len(terms),
                                                    _ptr(cl) if cl is not None else None, _ptr(C), _ptr(L), _ptr(R), ctypes.byref(accept),
                                                    ctypes.byref(rnd), ctypes.byref(check)))
        return bool(accept.value), int(rnd.value), int(check.value)

    # -- layer sumcheck (prove_sumcheck_opt, sumcheck.rs:36-156)
    def sumcheck_layer_raw(self, layer: Layer, k_next, z, W):
        gt, l, r = layer.arrays()
        zl = as_limbs(z) if layer.k else np.zeros((0, 4), dtype=np.uint64)
        wl = as_limbs(W)
        if zl.shape[0] != layer.k or wl.shape[0] != (1 << max(k_next, 0)):
            raise GkrError(N.GKR_ERR_INVALID, "z needs k_i entries and W 2^k_next entries")
        v = 2 * max(k_next, 0)
        C = np.zeros((max(v, 1), 3, 4), dtype=np.uint64)
        L = np.zeros(max(v, 1), dtype=np.uint32)
        R = np.zeros((max(v, 1), 4), dtype=np.uint64)
        self._check(N.lib().gkr_sumcheck_layer(self._h, ctypes.c_int(layer.k), ctypes.c_int(k_next), _ptr(gt), _ptr(l),
                                               _ptr(r), _ptr(zl), _ptr(wl), _ptr(C), _ptr(L), _ptr(R)))
        return C[:v], L[:v], R[:v]

    def prove_sumcheck_opt(self, layer: Layer, k_next, z, W):
        C, L, R = self.sumcheck_layer_raw(layer, k_next, z, W)
        return [from_limbs(C[j])[3 - int(L[j]):] for j in range(2 * k_next)], from_limbs(R)

    def predicate_tables(self, layer: Layer, k_next, z):
        gt, l, r = layer.arrays()
        zl = as_limbs(z) if layer.k else np.zeros((0, 4), dtype=np.uint64)
        n = 1 << (2 * max(k_next, 0))
        A = np.zeros((n, 4), dtype=np.uint64)
        M = np.zeros((n, 4), dtype=np.uint64)
        self._check(N.lib().gkr_predicate_tables(self._h, ctypes.c_int(layer.k), ctypes.c_int(k_next), _ptr(gt), _ptr(l),
                                                 _ptr(r), _ptr(zl), _ptr(A), _ptr(M)))
        return A, M

    def layer_eval(self, layer: Layer, prev):
        gt, l, r = layer.arrays()
        pl = as_limbs(prev)
        out = np.zeros((len(gt), 4), dtype=np.uint64)
        self._check(N.lib().gkr_layer_eval(self._h, ctypes.c_size_t(len(gt)), _ptr(gt), _ptr(l), _ptr(r), _ptr(pl),
                                           ctypes.c_size_t(pl.shape[0]), _ptr(out)))
        return out

    # -- full proof (prover::prove, prover.rs:6-96)
    def prove(self, circuit: GKRCircuit, input_values, require_zero_output=False) -> Proof:
        return self.prove_batch(circuit, [input_values], require_zero_output)[0]

    def prove_batch(self, circuit: GKRCircuit, inputs, require_zero_output=False) -> List[Proof]:
        """Proofs of one circuit for several witnesses, advanced together on the GPU (gkr_prove_batch)."""
        L = circuit.depth()
        B = len(inputs)
        ks = circuit.get_k_list()
        karr = np.asarray(ks, dtype=np.uint32)
        gates = [lay.arrays() for lay in circuit.layer]
        gt_p = (ctypes.c_void_p * L)(*[g[0].ctypes.data for g in gates])
        l_p = (ctypes.c_void_p * L)(*[g[1].ctypes.data for g in gates])
        r_p = (ctypes.c_void_p * L)(*[g[2].ctypes.data for g in gates])
        desc = N.CircuitDesc(L, karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), gt_p, l_p, r_p)
        sizes = N.ProofSizes()
        rc = N.lib().gkr_proof_sizes(ctypes.byref(desc), ctypes.byref(sizes))
        if rc:
            raise GkrError(rc, "gkr_proof_sizes")
        n_in = 1 << ks[-1]
        inp = np.empty((B, n_in, 4), dtype=np.uint64)
        for b, vals in enumerate(inputs):
            a = as_limbs(vals)
            if a.shape[0] != n_in:
                raise GkrError(N.GKR_ERR_INVALID, "input layer needs 2^input_k values")
            inp[b] = a
        sc = np.zeros((B, sizes.rounds, 3, 4), dtype=np.uint64)
        sl = np.zeros((B, sizes.rounds), dtype=np.uint32)
        sr = np.zeros((B, sizes.rounds, 4), dtype=np.uint64)
        q = np.zeros((B, sizes.q_slots, 4), dtype=np.uint64)
        ql = np.zeros((B, L), dtype=np.uint32)
        z = np.zeros((B, max(sizes.z_values, 1), 4), dtype=np.uint64)
        rr = np.zeros((B, L, 4), dtype=np.uint64)
        dco = np.zeros((B, sizes.d_coeffs, 4), dtype=np.uint64)
        ico = np.zeros((B, sizes.input_coeffs, 4), dtype=np.uint64)
        bufs = _proof_bufs((sc, sl, sr, q, ql, z, rr, dco, ico), B)
        self._check(N.lib().gkr_prove_batch(self._h, ctypes.byref(desc), _ptr(inp), ctypes.c_int(B),
                                            ctypes.c_int(1 if require_zero_output else 0), bufs))
        out = _decode_proofs((sc, sl, sr, q, ql, z, rr, dco, ico), ks)
        return out

    def _circuit_desc(self, circuit: GKRCircuit):
        """-> (gkr_circuit_desc, objects that must outlive its use)"""
        L = circuit.depth()
        karr = np.asarray(circuit.get_k_list(), dtype=np.uint32)
        gates = [lay.arrays() for lay in circuit.layer]
        gt_p = (ctypes.c_void_p * L)(*[g[0].ctypes.data for g in gates])
        l_p = (ctypes.c_void_p * L)(*[g[1].ctypes.data for g in gates])
        r_p = (ctypes.c_void_p * L)(*[g[2].ctypes.data for g in gates])
        desc = N.CircuitDesc(L, karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), gt_p, l_p, r_p)
        return desc, (karr, gates, gt_p, l_p, r_p)

    # -- the device verifier (gkr_verify_prepare / gkr_verify_prepared)
    def prepare_verify(self, circuit: GKRCircuit) -> VerifyHandle:
        """The circuit's gate arrays to the device, range-checked there (GkrError GKR_ERR_INVALID for a bad gate)."""
        desc, alive = self._circuit_desc(circuit)
        h = ctypes.c_void_p()
        self._check(N.lib().gkr_verify_prepare(self._h, ctypes.byref(desc), ctypes.byref(h)))
        return VerifyHandle(self, h, circuit.get_k_list())

    def verify_batch(self, handle_or_circuit, proof_or_arrays):
        """Verdicts of gkr_verify with the O(gates) sums on the GPU.  handle_or_circuit: a VerifyHandle (prepare_verify), or a
        GKRCircuit (gkr_verify_device: prepare + verify + free).  proof_or_arrays: a Proof, a list of Proofs, or the nine raw
        output arrays of prove_batch_raw(all_arrays=True) / a prove_many item (first axis = proof; every proof is verified).
        -> [(accept, failed_layer, failed_check)] in the proofs' order."""
        if isinstance(proof_or_arrays, Proof):
            proof_or_arrays = [proof_or_arrays]
        if len(proof_or_arrays) and all(isinstance(p, Proof) for p in proof_or_arrays):
            from .dropin import _arrays_of_proof
            per = [_arrays_of_proof(p) for p in proof_or_arrays]
            arrays = [np.ascontiguousarray(np.concatenate([a[j] for a in per], axis=0)) for j in range(9)]
        else:
            arrays = [np.ascontiguousarray(a) for a in proof_or_arrays]
        if len(arrays) != 9:
            raise GkrError(N.GKR_ERR_INVALID, "nine proof arrays expected")
        B = arrays[0].shape[0]
        bufs = _proof_bufs(arrays, B)
        accept = np.zeros(B, dtype=np.int32)
        layer, check = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
        if isinstance(handle_or_circuit, VerifyHandle):
            if not handle_or_circuit._h:
                raise GkrError(N.GKR_ERR_INVALID, "the verify handle is closed")
            rc = N.lib().gkr_verify_prepared(self._h, handle_or_circuit._h, bufs, ctypes.c_int(B), _ptr(accept), _ptr(layer), _ptr(check))
        else:
            desc, alive = self._circuit_desc(handle_or_circuit)
            rc = N.lib().gkr_verify_device(self._h, ctypes.byref(desc), bufs, ctypes.c_int(B), _ptr(accept), _ptr(layer), _ptr(check))
        self._check(rc)
        return [(bool(accept[b]), int(layer[b]), int(check[b])) for b in range(B)]

    def multi_hash_batch(self, rows, lens):
        """gkr_mimc7_multi_hash_device: many independent multi_hash calls (key 0) in one device call, the verifier's hash kernel.
        rows: (n, 3, 4) uint64 limbs, right-aligned as a proof's round vectors are; lens: n lengths.  -> (hashes (n, 4) uint64,
        valid (n,) uint32): a row whose length is outside 1..3 or whose used slots hold an element >= r has valid 0 and hash 0."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = lens.shape[0]
        if rows.shape != (n, 3, 4):
            raise GkrError(N.GKR_ERR_INVALID, "rows of shape (n, 3, 4) and n lengths expected")
        out = np.zeros((n, 4), dtype=np.uint64)
        valid = np.zeros(n, dtype=np.uint32)
        N.lib().gkr_mimc7_multi_hash_device.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2
        self._check(N.lib().gkr_mimc7_multi_hash_device(self._h, _ptr(rows), _ptr(lens), ctypes.c_size_t(n), _ptr(out), _ptr(valid)))
        return out, valid

    def prepare_many(self, work, require_zero_output=False):
        """work: [(GKRCircuit, inputs_limbs (B, 2^input_k, 4) uint64)] -> a prepared item list for prove_many_raw:
        circuit descriptions, output arrays and the gkr_prove_item array built once (an aggregation step proves the same
        circuits for every batch of inputs; only the input values change)."""
        keep, outs = [], []
        items = (N.ProveItem * len(work))()
        for i, (circuit, inputs_limbs) in enumerate(work):
            desc, alive = self._circuit_desc(circuit)
            sizes = N.ProofSizes()
            self._check(N.lib().gkr_proof_sizes(ctypes.byref(desc), ctypes.byref(sizes)))
            inp = np.ascontiguousarray(inputs_limbs, dtype=np.uint64)
            B, L = inp.shape[0], circuit.depth()
            arrs = [np.zeros((B, sizes.rounds, 3, 4), dtype=np.uint64), np.zeros((B, sizes.rounds), dtype=np.uint32),
                    np.zeros((B, sizes.rounds, 4), dtype=np.uint64), np.zeros((B, sizes.q_slots, 4), dtype=np.uint64),
                    np.zeros((B, L), dtype=np.uint32), np.zeros((B, max(sizes.z_values, 1), 4), dtype=np.uint64),
                    np.zeros((B, L, 4), dtype=np.uint64), np.zeros((B, sizes.d_coeffs, 4), dtype=np.uint64),
                    np.zeros((B, sizes.input_coeffs, 4), dtype=np.uint64)]
            bufs = _proof_bufs(arrs, B)
            items[i] = N.ProveItem(ctypes.cast(ctypes.pointer(desc), ctypes.c_void_p), inp.ctypes.data, B,
                                   1 if require_zero_output else 0, ctypes.cast(bufs, ctypes.c_void_p), 0)
            keep.append((desc, alive, inp, arrs, bufs))
            outs.append(arrs)
        return {"items": items, "keep": keep, "outs": outs}

    def prove_many_raw(self, prepared, max_concurrent=0):
        """gkr_prove_many on a prepare_many() list: every item proven by its own thread / child context of this context
        (the reference's par_iter over the (circuit, input) pairs).  -> per item the list of output arrays
        [coeffs, lens, challenges, q, q_len, z, r, d, input] (first axis = proof)."""
        items = prepared["items"]
        rc = N.lib().gkr_prove_many(self._h, items, ctypes.c_size_t(len(items)), ctypes.c_int(max_concurrent))
        self._check(rc)
        return prepared["outs"]

    def prove_many(self, work, require_zero_output=False, max_concurrent=0) -> List[List[Proof]]:
        """gkr_prove_many, decoded: work = [(GKRCircuit, inputs_limbs)] -> per item its proofs (one per witness)."""
        prepared = self.prepare_many(work, require_zero_output)
        outs = self.prove_many_raw(prepared, max_concurrent)
        return [_decode_proofs(arrs, circuit.get_k_list()) for arrs, (circuit, _) in zip(outs, work)]

    def prove_batch_raw(self, circuit: GKRCircuit, inputs_limbs, all_arrays=False, out=None):
        """gkr_prove_batch without decoding the outputs into Python ints (bench.py's proofs/sec leg; circuits with wide
        layers, whose d / input_func tables have 2^18 and more entries).
        inputs_limbs: (B, 2^input_k, 4) uint64.  Returns the challenge arrays (B, rounds, 4), or with all_arrays the nine
        output arrays [coeffs, lens, challenges, q, q_len, z, r, d, input] (first axis = proof)."""
        L = circuit.depth()
        B = inputs_limbs.shape[0]
        ks = circuit.get_k_list()
        karr = np.asarray(ks, dtype=np.uint32)
        gates = [lay.arrays() for lay in circuit.layer]
        gt_p = (ctypes.c_void_p * L)(*[g[0].ctypes.data for g in gates])
        l_p = (ctypes.c_void_p * L)(*[g[1].ctypes.data for g in gates])
        r_p = (ctypes.c_void_p * L)(*[g[2].ctypes.data for g in gates])
        desc = N.CircuitDesc(L, karr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), gt_p, l_p, r_p)
        sizes = N.ProofSizes()
        self._check(N.lib().gkr_proof_sizes(ctypes.byref(desc), ctypes.byref(sizes)))
        inp = np.ascontiguousarray(inputs_limbs, dtype=np.uint64)
        # (out: the nine arrays of an earlier call with the same shapes, reused -- a proof with a 2^20-value input layer
        # carries 40 MiB of coefficients, and fresh pages for them cost more than the proof)
        arrs = out if out is not None else [
            np.zeros((B, sizes.rounds, 3, 4), dtype=np.uint64), np.zeros((B, sizes.rounds), dtype=np.uint32),
            np.zeros((B, sizes.rounds, 4), dtype=np.uint64), np.zeros((B, sizes.q_slots, 4), dtype=np.uint64),
            np.zeros((B, L), dtype=np.uint32), np.zeros((B, max(sizes.z_values, 1), 4), dtype=np.uint64),
            np.zeros((B, L, 4), dtype=np.uint64), np.zeros((B, sizes.d_coeffs, 4), dtype=np.uint64),
            np.zeros((B, sizes.input_coeffs, 4), dtype=np.uint64)]
        bufs = _proof_bufs(arrs, B)
        self._check(N.lib().gkr_prove_batch(self._h, ctypes.byref(desc), _ptr(inp), ctypes.c_int(B), ctypes.c_int(0), bufs))
        return arrs if (all_arrays or out is not None) else arrs[2]


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def prove(circuit: GKRCircuit, input_values, require_zero_output=False) -> Proof:
    """prover::prove (prover.rs:6-9) on cuda:0 / HIP device 0."""
    return default_context().prove(circuit, input_values, require_zero_output)


def prove_sumcheck_opt(layer: Layer, k_next, z, W):
    return default_context().prove_sumcheck_opt(layer, k_next, z, W)


def prove_sumcheck(table, v):
    return default_context().prove_sumcheck(table, v)


def prove_sumcheck_product(tables, v):
    return default_context().prove_sumcheck_product(tables, v)


def prove_sumcheck_sop(tables, terms, v):
    return default_context().prove_sumcheck_sop(tables, terms, v)


def prove_zerocheck(tables, terms, z, v):
    return default_context().prove_zerocheck(tables, terms, z, v)


def prove_grand_product(table, v):
    return default_context().prove_grand_product(table, v)


def prove_fraction_sum(numerators, denominators, v):
    return default_context().prove_fraction_sum(numerators, denominators, v)


def prove_lookup(witness, table, alpha):
    return default_context().prove_lookup(witness, table, alpha)


def prove_r1cs_zerocheck(r1cs, witness, z):
    return default_context().prove_r1cs_zerocheck(r1cs, witness, z)


def prove_r1cs_inner(r1cs, witness, x, rho):
    return default_context().prove_r1cs_inner(r1cs, witness, x, rho)

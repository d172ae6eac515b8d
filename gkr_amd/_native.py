"""ctypes binding of libgkr_amd.so (include/gkr_amd.h).

The library is the product; there is no Python or CPU fallback.  Importing this
module without the built library raises, and every compute call needs a gfx950
device.
"""

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GKR_AMD_LIB: another build of the same library -- same-box A/B runs of two source states; never a fallback)
LIB_PATH = os.environ.get("GKR_AMD_LIB") or os.path.join(_HERE, "lib", "libgkr_amd.so")

GKR_OK = 0
GKR_ERR_INVALID = 1
GKR_ERR_NON_CANONICAL = 2
GKR_ERR_NO_DEVICE = 3
GKR_ERR_HIP = 4
GKR_ERR_NOMEM = 5
GKR_ERR_DEGENERATE = 6
GKR_ERR_UNSUPPORTED = 7

# verdicts of the verifiers (failed_check); 10 belongs to the plain, the product and the sum-of-products sumcheck's verifiers alone
GKR_VERIFY_OK, GKR_VERIFY_SHAPE, GKR_VERIFY_NON_CANONICAL = 0, 1, 2
GKR_VERIFY_ROUND_SUM, GKR_VERIFY_CHALLENGE, GKR_VERIFY_EVALUATION = 4, 5, 10
# the R1CS verifier's own (gkr_r1cs_verify*): e_T against the public matrices, e_w against the witness
GKR_VERIFY_MATRIX, GKR_VERIFY_WITNESS = 11, 12
# the grand product verifier's own (gkr_grand_product_verify*): a layer's last relation, a claimed product against the head's
GKR_VERIFY_FINAL_CLAIM, GKR_VERIFY_PRODUCT = 6, 13
# the fractional sum verifier's own (gkr_fraction_sum_verify*): the head's Q is zero, a claimed (P, Q) against the head's root
GKR_VERIFY_ZERO_DENOMINATOR, GKR_VERIFY_FRACTION_SUM = 14, 15
# the lookup verifier's own (gkr_lookup_verify*): the head's P is not zero
GKR_VERIFY_LOOKUP = 16

# rows of an R1CS matrix with more terms than this get a wave each on the device (GKR_R1CS_LONG_ROW)
GKR_R1CS_LONG_ROW = 32
# columns with more records than this are cut into segments of at most GKR_R1CS_COL_SEGMENT records, a wave each (GKR_R1CS_LONG_COL)
GKR_R1CS_LONG_COL = 32
GKR_R1CS_COL_SEGMENT = 2048

# limits of the sumcheck over a sum of products (gkr_sumcheck_sop*)
GKR_SOP_MAX_TABLES = 8
GKR_SOP_MAX_TERMS = 8

GKR_TRANSCRIPT_DEVICE = 0
GKR_TRANSCRIPT_HOST = 1

# every symbol include/gkr_amd.h declares (tests check the library exports them all)
SYMBOLS = [
    "gkr_strerror", "gkr_version", "gkr_ctx_create", "gkr_ctx_create_multi", "gkr_ctx_device_count", "gkr_ctx_destroy", "gkr_last_error",
    "gkr_ctx_set_transcript", "gkr_ctx_set_host_threads", "gkr_ctx_set_option", "gkr_ctx_get_option", "gkr_option_count", "gkr_option_name", "gkr_option_doc", "gkr_option_env", "gkr_host_help_while", "gkr_host_accounting", "gkr_host_accounting_read", "gkr_prove_many", "gkr_ctx_device_name", "gkr_ctx_profile", "gkr_ctx_profile_get", "gkr_ctx_profile_samples",
    "gkr_ctx_profile_reset", "gkr_mimc7_multi_hash", "gkr_mimc7_hash", "gkr_mimc7_constant",
    "gkr_selftest_mul", "gkr_selftest_wide_sum", "gkr_selftest_fold", "gkr_selftest_dot", "gkr_selftest_hash8", "gkr_selftest_host_pass", "gkr_selftest_host_prod_pass", "gkr_selftest_host_tail", "gkr_selftest_pass_schedule", "gkr_selftest_mle_plan", "gkr_selftest_mle_plan_ctx", "gkr_selftest_product_geometry", "gkr_selftest_layer_dense_geometry", "gkr_selftest_line_restriction", "gkr_selftest_seg_item", "gkr_devtest_field", "gkr_devtest_lazy", "gkr_devtest_reduce", "gkr_devtest_lanes", "gkr_devtest_gate_plan", "gkr_devtest_predicates", "gkr_sumcheck_mle", "gkr_sumcheck_mle_batch_device",
    "gkr_sumcheck_product", "gkr_sumcheck_product_batch_device",
    "gkr_sumcheck_product_verify_batch_device", "gkr_sumcheck_product_verify",
    "gkr_sumcheck_sop_batch_device", "gkr_sumcheck_sop",
    "gkr_sumcheck_sop_verify_batch_device", "gkr_sumcheck_sop_verify",
    "gkr_sumcheck_zerocheck_batch_device", "gkr_sumcheck_zerocheck", "gkr_eq_table_device",
    "gkr_grand_product_batch_device", "gkr_grand_product", "gkr_grand_product_verify_batch_device", "gkr_grand_product_verify",
    "gkr_selftest_grand_product_geometry", "gkr_devtest_grand_product_tree", "gkr_devtest_grand_product_chunk",
    "gkr_fraction_sum_batch_device", "gkr_fraction_sum", "gkr_fraction_sum_verify_batch_device", "gkr_fraction_sum_verify",
    "gkr_selftest_fraction_sum_geometry", "gkr_devtest_fraction_sum_tree", "gkr_devtest_fraction_sum_chunk",
    "gkr_lookup_multiplicities_device", "gkr_lookup_batch_device", "gkr_lookup_verify_batch_device", "gkr_lookup", "gkr_lookup_verify",
    "gkr_selftest_lookup_slot", "gkr_devtest_lookup_pair",
    "gkr_mle_eval_batch_device", "gkr_sumcheck_mle_verify_batch_device", "gkr_sumcheck_mle_verify",
    "gkr_sumcheck_layer", "gkr_sumcheck_layer_sharded", "gkr_sumcheck_layer_device", "gkr_resident_layer_create", "gkr_resident_layer_sumcheck", "gkr_resident_layer_sumcheck_wdev", "gkr_resident_layer_free", "gkr_exchange_limbs", "gkr_resident_layer_sumcheck_dev", "gkr_exchange_limbs_mle", "gkr_sumcheck_mle_sharded_dev", "gkr_exchange_rccl_unique_id", "gkr_exchange_rccl_create", "gkr_exchange_rccl_dev",
    "gkr_exchange_rccl_calls", "gkr_exchange_rccl_destroy", "gkr_exchange_rccl_error", "gkr_fr_widen", "gkr_fr_narrow", "gkr_predicate_tables", "gkr_layer_eval", "gkr_proof_sizes", "gkr_prove", "gkr_prove_batch",
    "gkr_layer_from_wires", "gkr_values_from_terms", "gkr_terms_from_coeffs", "gkr_prove_wires", "gkr_verify",
    "gkr_verify_prepare", "gkr_verify_prepared", "gkr_verify_circuit_free", "gkr_verify_device", "gkr_mimc7_multi_hash_device",
    "gkr_circom_meta", "gkr_circom_input_json", "gkr_circom_verifier_source", "gkr_circom_inject",
    "gkr_r1cs_parse", "gkr_r1cs_build", "gkr_r1cs_info", "gkr_r1cs_export", "gkr_r1cs_serialize", "gkr_r1cs_free",
    "gkr_r1cs_csr_info", "gkr_r1cs_csr_export", "gkr_r1cs_rows_prepare", "gkr_r1cs_rows_info", "gkr_r1cs_rows_free", "gkr_r1cs_rows_device",
    "gkr_r1cs_zerocheck_batch_device", "gkr_r1cs_zerocheck",
    "gkr_r1cs_csc_info", "gkr_r1cs_csc_export", "gkr_r1cs_cols_prepare", "gkr_r1cs_cols_prepare_segment", "gkr_r1cs_cols_info", "gkr_r1cs_cols_free",
    "gkr_r1cs_cols_device", "gkr_r1cs_inner_batch_device", "gkr_r1cs_inner",
    "gkr_r1cs_matrix_evals_device", "gkr_r1cs_verify_batch_device", "gkr_r1cs_verify",
    "gkr_wtns_parse", "gkr_wtns_serialize", "gkr_r1cs_compile", "gkr_layered_count", "gkr_layered_circuit",
    "gkr_layered_input_layer", "gkr_layered_input_values", "gkr_layered_free",
    "gkr_device_alloc", "gkr_device_free", "gkr_device_upload", "gkr_device_download",
    "gkr_device_fill_table", "gkr_device_fill_shard", "gkr_device_synchronize", "gkr_ubench_ceilings", "gkr_ubench_host_hash",
    "gkr_layer_session_open", "gkr_layer_session_open_tables", "gkr_layer_session_dep", "gkr_layer_session_rounds",
    "gkr_layer_session_sums", "gkr_layer_session_bind", "gkr_layer_session_tail", "gkr_layer_session_close",
    "gkr_mle_session_open", "gkr_mle_session_sums", "gkr_mle_session_bind", "gkr_mle_session_value",
    "gkr_mle_session_close", "gkr_device_tables_differ",
]


class CircuitDesc(ctypes.Structure):
    _fields_ = [
        ("depth", ctypes.c_uint32),
        ("k", ctypes.POINTER(ctypes.c_uint32)),
        ("gate_type", ctypes.POINTER(ctypes.c_void_p)),
        ("left", ctypes.POINTER(ctypes.c_void_p)),
        ("right", ctypes.POINTER(ctypes.c_void_p)),
    ]


class ProofBuf(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("sumcheck_coeffs", "sumcheck_len", "sumcheck_r", "q", "q_len", "z", "r", "d_coeffs", "input_coeffs")]


class ProveItem(ctypes.Structure):
    _fields_ = [("circuit", ctypes.c_void_p), ("input_values", ctypes.c_void_p), ("batch", ctypes.c_int),
                ("require_zero_output", ctypes.c_int), ("outs", ctypes.c_void_p), ("status", ctypes.c_int)]


ALLREDUCE_DEV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class ExchangeDev(ctypes.Structure):
    _fields_ = [("fn", ALLREDUCE_DEV_FN), ("user", ctypes.c_void_p), ("d_limbs", ctypes.c_void_p), ("capacity", ctypes.c_size_t)]


class R1csInfo(ctypes.Structure):
    _fields_ = [("n_wires", ctypes.c_uint32), ("n_pub_out", ctypes.c_uint32), ("n_pub_in", ctypes.c_uint32),
                ("n_prv_in", ctypes.c_uint32), ("n_labels", ctypes.c_uint64), ("n_constraints", ctypes.c_size_t),
                ("n_terms", ctypes.c_size_t)]


class R1csCsrInfo(ctypes.Structure):
    """gkr_r1cs_csr_info_t: the CSR form's sizes; tables of 2^n entries."""
    _fields_ = [("n", ctypes.c_uint32), ("n_wires", ctypes.c_uint32), ("n_constraints", ctypes.c_size_t),
                ("n_terms", ctypes.c_size_t * 3), ("n_long_rows", ctypes.c_size_t * 3), ("n_pool", ctypes.c_size_t)]

    def as_dict(self):
        return dict(n=int(self.n), n_wires=int(self.n_wires), n_constraints=int(self.n_constraints), n_terms=[int(x) for x in self.n_terms],
                    n_long_rows=[int(x) for x in self.n_long_rows], n_pool=int(self.n_pool))


class R1csCscInfo(ctypes.Structure):
    """gkr_r1cs_csc_info_t: the column-major form's sizes; eq tables of 2^n_x entries, T and the padded witness of 2^n_y."""
    _fields_ = [("n_x", ctypes.c_uint32), ("n_y", ctypes.c_uint32), ("n_wires", ctypes.c_uint32), ("n_constraints", ctypes.c_size_t),
                ("n_terms", ctypes.c_size_t * 3), ("n_long_cols", ctypes.c_size_t * 3), ("n_pool", ctypes.c_size_t)]

    def as_dict(self):
        return dict(n_x=int(self.n_x), n_y=int(self.n_y), n_wires=int(self.n_wires), n_constraints=int(self.n_constraints),
                    n_terms=[int(x) for x in self.n_terms], n_long_cols=[int(x) for x in self.n_long_cols], n_pool=int(self.n_pool))


class SopTerm(ctypes.Structure):
    """gkr_sop_term: one product of `degree` (1 .. 3) tables, table[j] < n_tables for j < degree."""
    _fields_ = [("degree", ctypes.c_uint8), ("table", ctypes.c_uint8 * 3)]


class ProofSizes(ctypes.Structure):
    _fields_ = [(n, ctypes.c_size_t) for n in ("rounds", "q_slots", "z_values", "d_coeffs", "input_coeffs")]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "gkr_amd: %s is missing -- build it with `make -C gkr_amd/csrc` "
                "(or __graft_entry__.build()); there is no fallback path" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.gkr_strerror.restype = ctypes.c_char_p
        L.gkr_version.restype = ctypes.c_char_p
        L.gkr_last_error.restype = ctypes.c_char_p
        L.gkr_last_error.argtypes = [ctypes.c_void_p]
        L.gkr_resident_layer_free.restype = None
        L.gkr_resident_layer_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.gkr_exchange_limbs.restype = ctypes.c_size_t
        L.gkr_exchange_limbs.argtypes = [ctypes.c_int]
        L.gkr_host_help_while.restype = ctypes.c_long
        L.gkr_host_help_while.argtypes = [ctypes.c_void_p]
        L.gkr_host_accounting.restype = ctypes.c_int
        L.gkr_host_accounting.argtypes = [ctypes.c_int]
        L.gkr_host_accounting_read.restype = ctypes.c_int
        L.gkr_host_accounting_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_size_t]
        L.gkr_ctx_destroy.restype = None
        L.gkr_ctx_destroy.argtypes = [ctypes.c_void_p]
        for fn in (L.gkr_layer_session_close, L.gkr_mle_session_close, L.gkr_verify_circuit_free):
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        # the product sumcheck: (ctx, tables, n, degree[, batch], out_coeffs, out_len, out_r, out_evals)
        L.gkr_sumcheck_product_batch_device.restype = ctypes.c_int
        L.gkr_sumcheck_product_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
        L.gkr_sumcheck_product.restype = ctypes.c_int
        L.gkr_sumcheck_product.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4
        # its verifier: (ctx, tables, n, degree[, batch], claims, coeffs, len, r, accept, failed_round, failed_check[, out_claims, out_evals])
        L.gkr_sumcheck_product_verify_batch_device.restype = ctypes.c_int
        L.gkr_sumcheck_product_verify_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 9
        L.gkr_sumcheck_product_verify.restype = ctypes.c_int
        L.gkr_sumcheck_product_verify.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 7
        # the sum of products: (ctx, tables, n, n_tables, terms, term_coeffs, n_terms[, batch], out_coeffs, out_len, out_r, out_evals)
        L.gkr_sumcheck_sop_batch_device.restype = ctypes.c_int
        L.gkr_sumcheck_sop_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4
        L.gkr_sumcheck_sop.restype = ctypes.c_int
        L.gkr_sumcheck_sop.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 4
        # its verifier: (ctx, tables, n, n_tables, terms, term_coeffs, n_terms[, batch], claims, coeffs, len, r, accept, failed_round,
        # failed_check[, out_claims, out_evals])
        L.gkr_sumcheck_sop_verify_batch_device.restype = ctypes.c_int
        L.gkr_sumcheck_sop_verify_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 9
        L.gkr_sumcheck_sop_verify.restype = ctypes.c_int
        L.gkr_sumcheck_sop_verify.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 7
        # the zero-check: (ctx, tables, n, n_tables, terms, term_coeffs, n_terms[, batch], z, out_coeffs, out_len, out_r, out_evals, out_eq)
        L.gkr_sumcheck_zerocheck_batch_device.restype = ctypes.c_int
        L.gkr_sumcheck_zerocheck_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6
        L.gkr_sumcheck_zerocheck.restype = ctypes.c_int
        L.gkr_sumcheck_zerocheck.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 6
        # the eq-table builder: (ctx, z, n, batch, d_out, stride_elements)
        L.gkr_eq_table_device.restype = ctypes.c_int
        L.gkr_eq_table_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_size_t]
        # the tree arguments, the grand product (one host table) and the fractional sum (two: numerators, denominators):
        #   (ctx, tables, n[, batch], out_root, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims)
        #   their verifiers: (ctx, tables, n[, batch], claimed, head, coeffs, len, r, evals, accept, failed_layer, failed_round,
        #   failed_check[, out_root]);  (n, blocks[n]); (ctx, tables, n, batch, d_layers); (ctx, n, batch, out)
        # the host-table forms differ in the number of leading pointers
        for name, host_tables in (("grand_product", 1), ("fraction_sum", 2)):
            for fn, argtypes in (
                    ("gkr_%s_batch_device", [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 8),
                    ("gkr_%s", [ctypes.c_void_p] * (1 + host_tables) + [ctypes.c_int] + [ctypes.c_void_p] * 8),
                    ("gkr_%s_verify_batch_device", [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 11),
                    ("gkr_%s_verify", [ctypes.c_void_p] * (1 + host_tables) + [ctypes.c_int] + [ctypes.c_void_p] * 10),
                    ("gkr_selftest_%s_geometry", [ctypes.c_int, ctypes.c_void_p]),
                    ("gkr_devtest_%s_tree", [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p]),
                    ("gkr_devtest_%s_chunk", [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.c_void_p])):
                getattr(L, fn % name).restype = ctypes.c_int
                getattr(L, fn % name).argtypes = argtypes
        # the lookup: W = (ctx, d_witness, n_w, d_table, n_t, shared_table); (W, batch, d_mult, out_missing, out_first_missing);
        # (W, d_mult, alpha, batch, the fractional sum's eight outputs); (W, d_mult, alpha, batch, head, coeffs, len, r, evals, accept,
        # failed_layer, failed_round, failed_check, out_sums); the host forms (ctx, witness, n_w, table, n_t, ..); (v, log_slots, slot);
        # (W, d_mult, alpha, batch, d_pair)
        W = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 2
        H = [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        for fn, argtypes in (
                ("gkr_lookup_multiplicities_device", W + [ctypes.c_int] + [ctypes.c_void_p] * 3),
                ("gkr_lookup_batch_device", W + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 8),
                ("gkr_lookup_verify_batch_device", W + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 10),
                ("gkr_lookup", H + [ctypes.c_void_p] * 12),
                ("gkr_lookup_verify", H + [ctypes.c_void_p] * 11),
                ("gkr_selftest_lookup_slot", [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
                ("gkr_devtest_lookup_pair", W + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p])):
            getattr(L, fn).restype = ctypes.c_int
            getattr(L, fn).argtypes = argtypes
        # the R1CS zero-check: the CSR form (host only), the resident handle, the rows, the zero-check on them
        L.gkr_r1cs_csr_info.restype = ctypes.c_int
        L.gkr_r1cs_csr_info.argtypes = [ctypes.c_void_p] * 2
        L.gkr_r1cs_csr_export.restype = ctypes.c_int
        L.gkr_r1cs_csr_export.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
        L.gkr_r1cs_rows_prepare.restype = ctypes.c_int
        L.gkr_r1cs_rows_prepare.argtypes = [ctypes.c_void_p] * 3
        L.gkr_r1cs_rows_info.restype = ctypes.c_int
        L.gkr_r1cs_rows_info.argtypes = [ctypes.c_void_p] * 2
        L.gkr_r1cs_rows_free.restype = None
        L.gkr_r1cs_rows_free.argtypes = [ctypes.c_void_p]
        # (ctx, rows, d_witness, stride_elements, batch, d_out, out_first_bad)
        L.gkr_r1cs_rows_device.restype = ctypes.c_int
        L.gkr_r1cs_rows_device.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 2
        # (ctx, rows, d_witness, stride_elements, batch, z, out_coeffs, out_len, out_r, out_evals, out_eq, out_first_bad)
        L.gkr_r1cs_zerocheck_batch_device.restype = ctypes.c_int
        L.gkr_r1cs_zerocheck_batch_device.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 7
        # (ctx, r1cs, witness, n_witness, z, out_coeffs, out_len, out_r, out_evals, out_eq, out_first_bad)
        L.gkr_r1cs_zerocheck.restype = ctypes.c_int
        L.gkr_r1cs_zerocheck.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 7
        # the R1CS inner sumcheck: the column-major form (host only), the resident handle, the table T, the sumcheck over (T, w)
        L.gkr_r1cs_csc_info.restype = ctypes.c_int
        L.gkr_r1cs_csc_info.argtypes = [ctypes.c_void_p] * 2
        L.gkr_r1cs_csc_export.restype = ctypes.c_int
        L.gkr_r1cs_csc_export.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
        L.gkr_r1cs_cols_prepare.restype = ctypes.c_int
        L.gkr_r1cs_cols_prepare.argtypes = [ctypes.c_void_p] * 3
        L.gkr_r1cs_cols_prepare_segment.restype = ctypes.c_int
        L.gkr_r1cs_cols_prepare_segment.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint32, ctypes.c_void_p]
        L.gkr_r1cs_cols_info.restype = ctypes.c_int
        L.gkr_r1cs_cols_info.argtypes = [ctypes.c_void_p] * 2
        L.gkr_r1cs_cols_free.restype = None
        L.gkr_r1cs_cols_free.argtypes = [ctypes.c_void_p]
        # (ctx, cols, x, rho, batch, d_out, out_stride_elements)
        L.gkr_r1cs_cols_device.restype = ctypes.c_int
        L.gkr_r1cs_cols_device.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
        # (ctx, cols, d_witness, stride_elements, batch, x, rho, out_coeffs, out_len, out_r, out_evals)
        L.gkr_r1cs_inner_batch_device.restype = ctypes.c_int
        L.gkr_r1cs_inner_batch_device.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_int] + [ctypes.c_void_p] * 6
        # (ctx, r1cs, witness, n_witness, x, rho, out_coeffs, out_len, out_r, out_evals)
        L.gkr_r1cs_inner.restype = ctypes.c_int
        L.gkr_r1cs_inner.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t] + [ctypes.c_void_p] * 6
        # (ctx, rows, x, y, batch, out)
        L.gkr_r1cs_matrix_evals_device.restype = ctypes.c_int
        L.gkr_r1cs_matrix_evals_device.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p]
        # (ctx, rows, batch, z, coeffs_x, len_x, r_x, evals_abc, rho, coeffs_y, len_y, r_y, evals_tw, d_witness, stride_elements, accept,
        #  failed_stage, failed_round, failed_check)
        L.gkr_r1cs_verify_batch_device.restype = ctypes.c_int
        L.gkr_r1cs_verify_batch_device.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 11 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
        # (ctx, r1cs, z, coeffs_x, len_x, r_x, evals_abc, rho, coeffs_y, len_y, r_y, evals_tw, witness, n_witness, accept, failed_stage,
        #  failed_round, failed_check)
        L.gkr_r1cs_verify.restype = ctypes.c_int
        L.gkr_r1cs_verify.argtypes = [ctypes.c_void_p] * 13 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4
        L.gkr_selftest_product_geometry.restype = ctypes.c_int
        L.gkr_selftest_product_geometry.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2
        # (n, batch, hash_threads, option_names, option_values, n_options, header, rows, row_capacity, n_rows); (ctx, n, batch, header, ..)
        L.gkr_selftest_mle_plan.restype = ctypes.c_int
        L.gkr_selftest_mle_plan.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
        L.gkr_selftest_mle_plan_ctx.restype = ctypes.c_int
        L.gkr_selftest_mle_plan_ctx.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_size_t, ctypes.c_void_p]
        # (ctx, k_i, k_next, gate_type, left, right, form, counts)
        L.gkr_devtest_gate_plan.restype = ctypes.c_int
        L.gkr_devtest_gate_plan.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
        # (k_next, log_p, round, out[8])
        L.gkr_selftest_layer_dense_geometry.restype = ctypes.c_int
        L.gkr_selftest_layer_dense_geometry.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p]
        # (ctx, k_i, k_next, gate_type, left, right, z, log_p, shard, out_A, out_M)
        L.gkr_devtest_predicates.restype = ctypes.c_int
        L.gkr_devtest_predicates.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 4 + [ctypes.c_uint32] * 2 + [ctypes.c_void_p] * 2
        for fn in (L.gkr_r1cs_free, L.gkr_layered_free):
            fn.restype = None
            fn.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib

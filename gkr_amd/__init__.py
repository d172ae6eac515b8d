"""gkr_amd -- MI355X-native GKR sumcheck prover (hot path of jeong0982/gkr).

The numeric work lives in lib/libgkr_amd.so (hand-written HIP for gfx950 behind
the C ABI of include/gkr_amd.h).  This package is the host-side mirror of the
reference's prover interface; it has no CPU fallback.
"""

from .field import MODULUS, from_limbs, to_limbs
from .prover import (Context, GKRCircuit, GkrError, Layer, Proof, R1csCols, R1csRows, VerifyHandle, default_context, multi_hash, prove,
                     prove_sumcheck, prove_sumcheck_opt, prove_sumcheck_product, prove_sumcheck_sop, prove_zerocheck,
                     prove_r1cs_zerocheck, prove_r1cs_inner, prove_grand_product, prove_fraction_sum, prove_lookup)

from .verifier import mle_eval, verify, verify_sumcheck_product, verify_sumcheck_sop, verify_sumcheck_table, verify_sumcheck_zerocheck, R1CS_ZEROCHECK_TERMS, r1cs_matrix_evals, verify_r1cs_inner, verify_r1cs, verify_grand_product, verify_fraction_sum, verify_lookup
from .aggregate import aggregated_input, circom_input, circom_meta

__all__ = ["verify", "mle_eval", "verify_sumcheck_table", "aggregated_input", "circom_input", "circom_meta", "MODULUS", "from_limbs", "to_limbs", "Context", "GKRCircuit", "GkrError", "Layer", "Proof", "VerifyHandle",
           "default_context", "multi_hash", "prove", "prove_sumcheck", "prove_sumcheck_opt", "prove_sumcheck_product", "verify_sumcheck_product",
           "prove_sumcheck_sop", "verify_sumcheck_sop", "prove_zerocheck", "verify_sumcheck_zerocheck", "prove_r1cs_zerocheck", "R1CS_ZEROCHECK_TERMS", "R1csRows",
           "R1csCols", "prove_r1cs_inner", "r1cs_matrix_evals", "verify_r1cs_inner", "verify_r1cs",
           "prove_grand_product", "verify_grand_product", "prove_fraction_sum", "verify_fraction_sum", "prove_lookup", "verify_lookup"]

// The sumcheck over a product of resident multilinear tables (degree 1 .. GKR_PRODUCT_MAX_DEGREE): prove_sumcheck
// (rust/src/gkr/sumcheck.rs:158-214) on g = mult_poly of the tables' extensions.  One fused pass per round over all factors
// (kernels_product.hip) and the round's hash on the device, in both transcript modes: the entry points, the shape checks and the
// launch geometry; the driver, run_product_batch, is capi_resident.hip's.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

static_assert(gkr::kProductMaxDegree == GKR_PRODUCT_MAX_DEGREE, "the kernels' templates cover the header's degrees");

namespace gkr_host {

// Blocks per sumcheck of round `round` (0-based): mle_blocks_per_table of the round's items (round 1: half a table; later: a quarter
// of the source table), never more than round 1's count, which sizes the partials.  The sum-of-products and zero-check passes
// launch the same.  Host logic only; gkr_selftest_product_geometry reports it.
uint32_t product_round_blocks(int n, int batch, int round) {
    const size_t len = (size_t)1 << n;
    const uint32_t max_nblk = gkr::mle_blocks_per_table((uint32_t)(len / 2), (uint32_t)batch);   // (non-increasing in the items)
    const uint32_t items = (uint32_t)(len >> (round + 1));
    return std::min(gkr::mle_blocks_per_table(items, (uint32_t)batch), max_nblk);
}

// The shape checks the prover's and the verifier's (capi_mle_verify.hip) entry points share, in gkr_sumcheck_mle_batch_device's
// order (ctx and pointers first, then n).  Plain returns, as gkr_mle_eval_batch_device's: they are decided before the context
// is looked at.
bool product_shape_ok(int n, int degree, int batch) {
    if (n < 2 || n > GKR_MAX_MLE_N) return false;                                       // n must be in [2, 30]
    if (degree < 1 || degree > GKR_PRODUCT_MAX_DEGREE) return false;                    // degree must be in [1, 3]
    return (((unsigned long long)batch * (unsigned long long)degree) << n) <= (1ull << 30);   // batch * degree * 2^n values
}

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

int gkr_sumcheck_product_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int degree, int batch, gkr_fr* out_coeffs,
                                      uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    if (!ctx || !d_tables || !out_coeffs || !out_len || !out_r || batch < 1 || batch > 65535) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return run_product_batch(ctx, static_cast<const Fr*>(d_tables), n, degree, batch, out_coeffs, out_len, out_r, out_evals);
}

int gkr_sumcheck_product(gkr_ctx* ctx, const gkr_fr* tables, int n, int degree, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                         gkr_fr* out_evals) {
    if (!ctx || !tables || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, 1)) return GKR_ERR_INVALID;
    return run_on_tables(ctx, tables, (size_t)degree << n,
                         [&](const Fr* d) { return run_product_batch(ctx, d, n, degree, 1, out_coeffs, out_len, out_r, out_evals); });
}

// the launch geometry of run_product_batch and its siblings (host logic only, the process-default options): per round the blocks per sumcheck and
// the chunk the pass kernels derive from them.  batch * 1 table of 2^n values must be a shape the prover admits.
int gkr_selftest_product_geometry(int n, int batch, uint32_t* nblk, uint32_t* chunk) {
    if (!nblk || !chunk || batch < 1 || batch > 65535 || !product_shape_ok(n, 1, batch)) return GKR_ERR_INVALID;
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(((size_t)1 << n) >> (round + 1)), b = product_round_blocks(n, batch, round);
        nblk[round] = b;
        chunk[round] = ((items + b - 1) / b + 255u) & ~255u;
    }
    return GKR_OK;
}

}  // extern "C"

// The grand product P = prod_i V[i] over resident tables as GKR on the binary tree of multiplication gates: the tree on the device
// (kernels_grand_product.hip), then layer by layer the zero-check  L_k(z) = sum_x eq(z, x) L_{k+1}(0, x) L_{k+1}(1, x)  through
// capi_resident.hip's run_zerocheck_batch on the two contiguous halves of the level below -- no sumcheck kernel of this path's
// own -- chained by Fiat-Shamir on the host (grand_product_rounds.h); and the verifier of such proofs.  The driver and the chunk
// verifier are the tree arguments' (tree_argument.h); this file describes the argument to them.  C ABI: include/gkr_amd.h.
#include "tree_argument.h"
#include "grand_product_rounds.h"

namespace {

struct GrandProduct {
    using Gate = gkr::gp::Gate;
    static constexpr const char *kLayers = "gp.layers", *kVer = "gp.ver.", *kTree = "gp_tree";
    static constexpr double kTreeNodeBytes = 2.0 * 32.0;
    static constexpr const char* kNoHash = "grand product verifier: no hash for a well-formed round vector";
    static constexpr auto launch_tree = gkr::launch_gp_tree;
    static constexpr auto layer_offset = gkr::gp_layer_offset;
    static constexpr auto level_blocks = gkr::gp_level_blocks;
    // one term L_{k+1}[0 ..) * L_{k+1}[2^k ..) with coefficient 1; no lambda
    static int run_layer(gkr_ctx* ctx, const Fr* tables, int k, int batch, const gkr_fr* z, const gkr_fr*, gkr_fr* out_coeffs, uint32_t* out_len,
                         gkr_fr* out_r, gkr_fr* out_evals) {
        const gkr_sop_term term = {2, {0, 1, 0}};
        gkr::SopTerms ts;
        gkr::SopCoeffs cf;
        if (!sop_shape(k, 2, &term, 1, batch, &ts) || !sop_coeffs(nullptr, 1, &cf)) return ctx->fail(GKR_ERR_INVALID, "grand product: a layer's shape");
        return run_zerocheck_batch(ctx, tables, k, ts, cf, batch, z, out_coeffs, out_len, out_r, out_evals, nullptr);
    }
};
using GP = TreeArgument<GrandProduct>;

}  // namespace

// =========================================================================== C ABI

extern "C" {

int gkr_grand_product_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_products, gkr_fr* out_head, gkr_fr* out_coeffs,
                                   uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claim) {
    return GP::prove_batch_device(ctx, d_tables, n, batch, out_products, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claim);
}

int gkr_grand_product(gkr_ctx* ctx, const gkr_fr* table, int n, gkr_fr* out_product, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len,
                      gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claim) {
    if (!ctx || !table || !out_product || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!GP::shape(n, 1)) return GKR_ERR_INVALID;
    return run_on_tables(ctx, table, (size_t)1 << n, [&](const Fr* d) {
        return GP::prove(ctx, d, n, 1, out_product, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claim);
    });
}

int gkr_grand_product_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* products, const gkr_fr* head,
                                          const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept,
                                          uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_products) {
    return GP::verify_batch_device(ctx, d_tables, n, batch, {products, head, coeffs, r, evals, len}, accept, failed_layer, failed_round, failed_check,
                                   out_products);
}

int gkr_grand_product_verify(gkr_ctx* ctx, const gkr_fr* table, int n, const gkr_fr* product, const gkr_fr* head, const gkr_fr* coeffs,
                             const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept, uint32_t* failed_layer, uint32_t* failed_round,
                             uint32_t* failed_check) {
    if (!ctx || !table || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!GP::shape(n, 1)) return GKR_ERR_INVALID;
    return run_on_tables(ctx, table, (size_t)1 << n, [&](const Fr* d) {
        return gkr_grand_product_verify_batch_device(ctx, d, n, 1, product, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check,
                                                     nullptr);
    });
}

int gkr_selftest_grand_product_geometry(int n, uint32_t* blocks) { return GP::geometry(n, blocks); }

int gkr_devtest_grand_product_tree(gkr_ctx* ctx, const void* d_tables, int n, int batch, void* d_layers) {
    return GP::devtest_tree(ctx, d_tables, n, batch, d_layers);
}

int gkr_devtest_grand_product_chunk(gkr_ctx* ctx, int n, int batch, uint32_t* out) { return GP::devtest_chunk(ctx, n, batch, out); }

}  // extern "C"

// The fractional sum sum_i N[i] / D[i] = P / Q over resident pairs of tables (LogUp) as GKR on the binary tree of fraction
// additions: the tree on the device (kernels_fraction_sum.hip: nothing is inverted), then layer by layer the zero-check
//   cp_k + lambda_k cq_k = sum_x eq(z^(k), x) (T0 T3 + T1 T2 + lambda_k T2 T3)(x)
// through capi_resident.hip's run_fraction_layer_batch on the four contiguous halves of the level below -- the zero-check's
// passes, a round kernel with the proof's own lambda -- chained by Fiat-Shamir on the host (fraction_sum_rounds.h); and the
// verifier of such proofs, whose device share is the evaluation of N and D at the proof's one point.  The driver and the chunk
// verifier are the tree arguments' (tree_argument.h); this file describes the argument to them.  C ABI: include/gkr_amd.h.
#include "tree_argument.h"
#include "fraction_sum_rounds.h"

namespace {

struct FractionSum {
    using Gate = gkr::fs::Gate;
    static constexpr const char *kLayers = "fs.layers", *kVer = "fs.ver.", *kTree = "fs_tree";
    static constexpr double kTreeNodeBytes = 6.0 * 32.0;
    static constexpr const char* kNoHash = "fraction sum verifier: no hash for a well-formed round vector";
    static constexpr auto launch_tree = gkr::launch_fs_tree;
    static constexpr auto layer_offset = gkr::fs_layer_offset;
    static constexpr auto level_blocks = gkr::fs_level_blocks;
    static int run_layer(gkr_ctx* ctx, const Fr* tables, int k, int batch, const gkr_fr* z, const gkr_fr* lambda, gkr_fr* out_coeffs, uint32_t* out_len,
                         gkr_fr* out_r, gkr_fr* out_evals) {
        return run_fraction_layer_batch(ctx, tables, k, batch, z, lambda, out_coeffs, out_len, out_r, out_evals, nullptr);
    }
};
using FS = TreeArgument<FractionSum>;

}  // namespace

// =========================================================================== C ABI

extern "C" {

int gkr_fraction_sum_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_sums, gkr_fr* out_head, gkr_fr* out_coeffs,
                                  uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    return FS::prove_batch_device(ctx, d_tables, n, batch, out_sums, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims);
}

int gkr_fraction_sum(gkr_ctx* ctx, const gkr_fr* numerators, const gkr_fr* denominators, int n, gkr_fr* out_sum, gkr_fr* out_head, gkr_fr* out_coeffs,
                     uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    if (!ctx || !numerators || !denominators || !out_sum || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!FS::shape(n, 1)) return GKR_ERR_INVALID;
    std::vector<gkr_fr> pair((size_t)2 << n);   // the pair as the device holds it: N then D
    memcpy(pair.data(), numerators, sizeof(gkr_fr) << n);
    memcpy(pair.data() + ((size_t)1 << n), denominators, sizeof(gkr_fr) << n);
    return run_on_tables(ctx, pair.data(), pair.size(), [&](const Fr* d) {
        return FS::prove(ctx, d, n, 1, out_sum, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims);
    });
}

int gkr_fraction_sum_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* sums, const gkr_fr* head,
                                         const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept,
                                         uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_sums) {
    return FS::verify_batch_device(ctx, d_tables, n, batch, {sums, head, coeffs, r, evals, len}, accept, failed_layer, failed_round, failed_check, out_sums);
}

int gkr_fraction_sum_verify(gkr_ctx* ctx, const gkr_fr* numerators, const gkr_fr* denominators, int n, const gkr_fr* sum, const gkr_fr* head,
                            const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept, uint32_t* failed_layer,
                            uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !numerators || !denominators || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!FS::shape(n, 1)) return GKR_ERR_INVALID;
    std::vector<gkr_fr> pair((size_t)2 << n);
    memcpy(pair.data(), numerators, sizeof(gkr_fr) << n);
    memcpy(pair.data() + ((size_t)1 << n), denominators, sizeof(gkr_fr) << n);
    return run_on_tables(ctx, pair.data(), pair.size(), [&](const Fr* d) {
        return gkr_fraction_sum_verify_batch_device(ctx, d, n, 1, sum, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check,
                                                    nullptr);
    });
}

int gkr_selftest_fraction_sum_geometry(int n, uint32_t* blocks) { return FS::geometry(n, blocks); }

int gkr_devtest_fraction_sum_tree(gkr_ctx* ctx, const void* d_tables, int n, int batch, void* d_layers) {
    return FS::devtest_tree(ctx, d_tables, n, batch, d_layers);
}

int gkr_devtest_fraction_sum_chunk(gkr_ctx* ctx, int n, int batch, uint32_t* out) { return FS::devtest_chunk(ctx, n, batch, out); }

}  // extern "C"

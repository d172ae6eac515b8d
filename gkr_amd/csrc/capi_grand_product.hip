// The grand product P = prod_i V[i] over resident tables as GKR on the binary tree of multiplication gates: the tree on the device
// (kernels_grand_product.hip), then layer by layer the zero-check  L_k(z) = sum_x eq(z, x) L_{k+1}(0, x) L_{k+1}(1, x)  through
// capi_resident.hip's run_zerocheck_batch on the two contiguous halves of the level below -- no gather, no copy, no sumcheck kernel
// of this path's own -- chained by Fiat-Shamir on the host (grand_product_rounds.h); and the verifier of such proofs, whose round
// relations are verify_rounds.h's and whose one read of V is kernels_mle_eval.hip's.  C ABI: include/gkr_amd.h.
//
// The verifier builds a chunk of proofs from verify_chunk.h's pieces, which states the plan.  Particular to this file:
//   - one set of round vectors, rows of four slots, all layers of a proof next to each other;
//   - the host's relations (the shape and canonical checks of the whole proof, zeta, every tau_k, c_k and z^(k), the layers' round
//     sums and Horner steps: grand_product_rounds.h) run BEFORE the device's share is queued, because the points z^(n) come out
//     of them: those of the proofs that passed SHAPE and NON_CANONICAL go up, zeros for the others, whose verdict is decided.
//     The host's hashes (if any) run after it is queued, while the device works;
//   - the device's share is the one evaluation of every table; per proof the first failure in order.
#include "verify_chunk.h"
#include "grand_product_rounds.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
namespace GP = gkr::gp;

constexpr size_t kRelPiece = 4;   // proofs per piece of host work

// the shapes both the prover and the verifier admit (plain returns: decided before the context is looked at)
bool gp_shape(int n, int batch) {
    return batch >= 1 && batch <= 65535 && n >= 3 && n <= GKR_MAX_MLE_N && (((unsigned long long)batch) << n) <= (1ull << 30);
}

const auto host_hash = [](const F* v, int len) { return host_multi_hash(v, len, host_mimc_constants64()); };

int queue_tree(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, Fr* d_layers) {
    Timed t(ctx, "gp_tree", (double)batch * 2.0 * 32.0 * (double)((size_t)1 << n));
    gkr::launch_gp_tree(d_tables, (uint32_t)n, (uint32_t)batch, d_layers, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

// the whole of gkr_grand_product_batch_device behind its argument checks
int run_grand_product(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, gkr_fr* out_products, gkr_fr* out_head, gkr_fr* out_coeffs,
                      uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claim) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, R = GP::rounds(n);
    Fr* d_layers = nullptr;
    WS(ctx, "gp.layers", Fr, B * (((size_t)1 << n) - 1), d_layers);
    if (const int rc = queue_tree(ctx, d_tables, n, batch, d_layers)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_head, d_layers + gkr::gp_layer_offset(2, (uint32_t)batch), B * 4 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_products, d_layers, B * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    // the head: z^(2) of every proof (the claim c_2 is the verifier's to form; the prover's chain needs the points alone)
    std::vector<gkr_fr> z(B * 2), z_next;
    for (size_t b = 0; b < B; ++b) {
        F zeta1, zeta2;
        GP::head_point(out_head + 4 * b, host_hash, &zeta1, &zeta2);
        z[2 * b] = GP::abi(zeta1);
        z[2 * b + 1] = GP::abi(zeta2);
    }
    // the layers: one term L_{k+1}[0 ..) * L_{k+1}[2^k ..) with coefficient 1
    const gkr_sop_term term = {2, {0, 1, 0}};
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    std::vector<gkr_fr> coeffs, r, evals(B * 2), claim(B);
    std::vector<uint32_t> len;
    for (int k = 2; k < n; ++k) {
        if (!sop_shape(k, 2, &term, 1, batch, &ts) || !sop_coeffs(nullptr, 1, &cf)) return ctx->fail(GKR_ERR_INVALID, "grand product: a layer's shape");
        const Fr* tables = k + 1 == n ? d_tables : d_layers + gkr::gp_layer_offset((uint32_t)k + 1, (uint32_t)batch);
        coeffs.resize(B * k * 4);
        len.resize(B * k);
        r.resize(B * k);
        if (const int rc = run_zerocheck_batch(ctx, tables, k, ts, cf, batch, z.data(), coeffs.data(), len.data(), r.data(), evals.data(), nullptr))
            return rc;
        const size_t row = GP::layer_row(k);
        z_next.resize(B * (k + 1));
        for (size_t b = 0; b < B; ++b) {
            memcpy(out_coeffs + 4 * (b * R + row), coeffs.data() + 4 * b * k, (size_t)k * 4 * sizeof(gkr_fr));
            memcpy(out_len + b * R + row, len.data() + b * k, (size_t)k * sizeof(uint32_t));
            memcpy(out_r + b * R + row, r.data() + b * k, (size_t)k * sizeof(gkr_fr));
            if (out_evals) memcpy(out_evals + 2 * (b * (n - 2) + (k - 2)), evals.data() + 2 * b, 2 * sizeof(gkr_fr));
            claim[b] = GP::abi(GP::next_claim(k, evals.data() + 2 * b, r.data() + b * k, host_hash, z_next.data() + b * (k + 1)));
        }
        z.swap(z_next);
    }
    if (out_point) memcpy(out_point, z.data(), B * n * sizeof(gkr_fr));
    if (out_claim) memcpy(out_claim, claim.data(), B * sizeof(gkr_fr));
    return GKR_OK;
}

// ---- the verifier

// a chunk's share of the caller's arrays, in the ABI's layouts
struct Proofs {
    const gkr_fr *products, *head, *coeffs, *r, *evals;
    const uint32_t* len;
    GP::Proof at(int n, size_t b) const {
        const size_t R = GP::rounds(n);
        return GP::Proof{products ? products + b : nullptr, head + 4 * b, coeffs + 4 * b * R, r + b * R, evals + 2 * b * (n - 2), len + b * R};
    }
};

// proofs of a chunk: what fits verify_workspace_mb (the evaluation's workspace, the point, the value; with hashes the rows and slots)
size_t chunk_proofs(int n, int batch) {
    const size_t one = gkr::mle_eval_ws_bytes((uint32_t)n, 1, 1) + ((size_t)n + 1) * sizeof(Fr) +
                       GP::rounds(n) * (4 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
    return verify_chunk_size(one, 32768, batch);   // (the table is a grid dimension of the launches)
}

int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, uint32_t nb, const Proofs& t, int* accept, uint32_t* failed_layer, uint32_t* failed_round,
                 uint32_t* failed_check, gkr_fr* out_products) {
    const size_t R = GP::rounds(n);
    // ---- 1. the round vectors' hashes on the side stream: rows of four slots
    RoundHashes hashes(ctx, "gp.ver.", {RowSet{4u, (size_t)nb * R, {{t.coeffs, t.len}}}});
    if (const int rc = hashes.start()) return rc;
    // ---- 2. what needs neither a round vector's hash nor V: the form, the chain of claims and points, the layers' sums
    std::vector<GP::Pre> pre(nb);
    for_pieces(ctx, (nb + kRelPiece - 1) / kRelPiece, 8, [&](size_t a) {
        for (size_t b = a * kRelPiece; b < std::min<size_t>(nb, (a + 1) * kRelPiece); ++b) pre[b] = GP::pre_relations(n, t.at(n, b), host_hash);
    });
    // ---- 3. the device's share: V~(z^(n)) of the proofs still standing, at zero for the others
    Fr *h_pts = nullptr, *h_out = nullptr;
    HIP_TRY(ctx, ctx->pinned_host("gp.ver.pts", (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("gp.ver.out", (size_t)nb * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    memset(h_pts, 0, (size_t)nb * n * sizeof(Fr));
    for (uint32_t b = 0; b < nb; ++b)
        if (pre[b].point) memcpy(h_pts + (size_t)b * n, pre[b].z.data() + GP::layer_row(n), (size_t)n * sizeof(Fr));
    if (const int rc = queue_eval(ctx, "gp.ver.", d_tables, n, nb, 1u, h_pts, h_out)) return rc;
    if (const int rc = hashes.join()) return rc;
    // ---- 4. the host's hashes (if any) while the device works
    for_pieces(ctx, hashes.host_pieces(), 8, [&](size_t a) { hashes.hash_piece(a); });
    if (const int rc = hashes.sync_main()) return rc;
    const V::HashSlot* slots = hashes.slots();
    ctx->drain_events();
    for (uint32_t b = 0; b < nb; ++b) {
        GP::Verdict v;
        F value;
        memcpy(value.l, &h_out[b], 32);
        if (!GP::verdict(n, t.at(n, b), pre[b], slots + (size_t)b * R, value, &v))
            return ctx->fail(GKR_ERR_HIP, "grand product verifier: no hash for a well-formed round vector");
        accept[b] = v.check == 0 ? 1 : 0;
        if (failed_layer) failed_layer[b] = v.layer;
        if (failed_round) failed_round[b] = v.round;
        if (failed_check) failed_check[b] = v.check;
        if (out_products) out_products[b] = pre[b].point ? GP::abi(GP::head_product(t.head + 4 * (size_t)b)) : gkr_fr{{0, 0, 0, 0}};
    }
    return GKR_OK;
}

}  // namespace

// =========================================================================== C ABI

extern "C" {

int gkr_grand_product_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_products, gkr_fr* out_head, gkr_fr* out_coeffs,
                                   uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claim) {
    if (!ctx || !d_tables || !out_products || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!gp_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return run_grand_product(ctx, static_cast<const Fr*>(d_tables), n, batch, out_products, out_head, out_coeffs, out_len, out_r, out_evals, out_point,
                             out_claim);
}

int gkr_grand_product(gkr_ctx* ctx, const gkr_fr* table, int n, gkr_fr* out_product, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len,
                      gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claim) {
    if (!ctx || !table || !out_product || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!gp_shape(n, 1)) return GKR_ERR_INVALID;
    return run_on_tables(ctx, table, (size_t)1 << n, [&](const Fr* d) {
        return run_grand_product(ctx, d, n, 1, out_product, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claim);
    });
}

int gkr_grand_product_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* products, const gkr_fr* head,
                                          const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept,
                                          uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_products) {
    if (!ctx || !d_tables || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!gp_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    const size_t R = GP::rounds(n);
    return for_chunks(batch, chunk_proofs(n, batch), [&](size_t b, uint32_t nb) {
        const Proofs t{products ? products + b : nullptr, head + 4 * b, coeffs + 4 * b * R, r + b * R, evals + 2 * b * (n - 2), len + b * R};
        return verify_chunk(ctx, static_cast<const Fr*>(d_tables) + (b << n), n, nb, t, accept + b, failed_layer ? failed_layer + b : nullptr,
                            failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                            out_products ? out_products + b : nullptr);
    });
}

int gkr_grand_product_verify(gkr_ctx* ctx, const gkr_fr* table, int n, const gkr_fr* product, const gkr_fr* head, const gkr_fr* coeffs,
                             const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept, uint32_t* failed_layer, uint32_t* failed_round,
                             uint32_t* failed_check) {
    if (!ctx || !table || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!gp_shape(n, 1)) return GKR_ERR_INVALID;
    return run_on_tables(ctx, table, (size_t)1 << n, [&](const Fr* d) {
        return gkr_grand_product_verify_batch_device(ctx, d, n, 1, product, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check,
                                                     nullptr);
    });
}

int gkr_selftest_grand_product_geometry(int n, uint32_t* blocks) {
    if (!blocks || n < 3 || n > GKR_MAX_MLE_N) return GKR_ERR_INVALID;
    for (int k = 0; k < n; ++k) blocks[k] = gkr::gp_level_blocks((uint32_t)k);
    return GKR_OK;
}

int gkr_devtest_grand_product_tree(gkr_ctx* ctx, const void* d_tables, int n, int batch, void* d_layers) {
    if (!ctx || !d_tables || !d_layers || !gp_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    if (const int rc = queue_tree(ctx, static_cast<const Fr*>(d_tables), n, batch, static_cast<Fr*>(d_layers))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

int gkr_devtest_grand_product_chunk(gkr_ctx* ctx, int n, int batch, uint32_t* out) {
    if (!ctx || !out || !gp_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    *out = (uint32_t)chunk_proofs(n, batch);
    return GKR_OK;
}

}  // extern "C"

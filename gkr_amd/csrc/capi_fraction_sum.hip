// The fractional sum sum_i N[i] / D[i] = P / Q over resident pairs of tables (LogUp) as GKR on the binary tree of fraction
// additions: the tree on the device (kernels_fraction_sum.hip: nothing is inverted), then layer by layer the zero-check
//   cp_k + lambda_k cq_k = sum_x eq(z^(k), x) (T0 T3 + T1 T2 + lambda_k T2 T3)(x)
// through capi_resident.hip's run_fraction_layer_batch on the four contiguous halves of the level below -- no gather, no copy; the
// zero-check's passes, a round kernel with the proof's own lambda -- chained by Fiat-Shamir on the host (fraction_sum_rounds.h);
// and the verifier of such proofs, whose round relations are verify_rounds.h's and whose one read of N and D is
// kernels_mle_eval.hip's.  C ABI: include/gkr_amd.h.
//
// The verifier builds a chunk of proofs from verify_chunk.h's pieces exactly as capi_grand_product.hip does: one set of round
// vectors, rows of four slots; the host's relations BEFORE the device's share is queued, because the points z^(n) come out of
// them (zeros for the proofs whose verdict SHAPE or NON_CANONICAL has decided); the host's hashes (if any) while the device works;
// the device's share is the evaluation of N and D at the proof's one point (groups of G = 2 tables); per proof the first failure.
#include "verify_chunk.h"
#include "fraction_sum_rounds.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
namespace FS = gkr::fs;

constexpr size_t kRelPiece = 4;   // proofs per piece of host work

// the shapes both the prover and the verifier admit (plain returns: decided before the context is looked at): the zero-check's
// own limit on the top layer's four tables
bool fs_shape(int n, int batch) {
    return batch >= 1 && batch <= 65535 && n >= 3 && n <= GKR_MAX_MLE_N && (((unsigned long long)batch) << (n + 1)) <= (1ull << 30);
}

const auto host_hash = [](const F* v, int len) { return host_multi_hash(v, len, host_mimc_constants64()); };

int queue_tree(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, Fr* d_layers) {
    Timed t(ctx, "fs_tree", (double)batch * 6.0 * 32.0 * (double)((size_t)1 << n));
    gkr::launch_fs_tree(d_tables, (uint32_t)n, (uint32_t)batch, d_layers, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

// the whole of gkr_fraction_sum_batch_device behind its argument checks
int run_fraction_sum(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, gkr_fr* out_sums, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len,
                     gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, R = FS::rounds(n);
    Fr* d_layers = nullptr;
    WS(ctx, "fs.layers", Fr, 2 * B * (((size_t)1 << n) - 1), d_layers);
    if (const int rc = queue_tree(ctx, d_tables, n, batch, d_layers)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_head, d_layers + gkr::fs_layer_offset(2, (uint32_t)batch), B * 8 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_sums, d_layers, B * 2 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    // the head: z^(2) and lambda_2 of every proof (the claims are the verifier's to form; the prover's chain needs these alone)
    std::vector<gkr_fr> z(B * 2), z_next, lambda(B);
    for (size_t b = 0; b < B; ++b) {
        F zeta1, zeta2, lambda2;
        FS::head_point(out_head + 8 * b, host_hash, &zeta1, &zeta2, &lambda2);
        z[2 * b] = FS::abi(zeta1);
        z[2 * b + 1] = FS::abi(zeta2);
        lambda[b] = FS::abi(lambda2);
    }
    std::vector<gkr_fr> coeffs, r, evals(B * 4), claims(B * 2);
    std::vector<uint32_t> len;
    for (int k = 2; k < n; ++k) {
        const Fr* tables = k + 1 == n ? d_tables : d_layers + gkr::fs_layer_offset((uint32_t)k + 1, (uint32_t)batch);
        coeffs.resize(B * k * 4);
        len.resize(B * k);
        r.resize(B * k);
        if (const int rc = run_fraction_layer_batch(ctx, tables, k, batch, z.data(), lambda.data(), coeffs.data(), len.data(), r.data(), evals.data(),
                                                    nullptr))
            return rc;
        const size_t row = FS::layer_row(k);
        z_next.resize(B * (k + 1));
        for (size_t b = 0; b < B; ++b) {
            memcpy(out_coeffs + 4 * (b * R + row), coeffs.data() + 4 * b * k, (size_t)k * 4 * sizeof(gkr_fr));
            memcpy(out_len + b * R + row, len.data() + b * k, (size_t)k * sizeof(uint32_t));
            memcpy(out_r + b * R + row, r.data() + b * k, (size_t)k * sizeof(gkr_fr));
            if (out_evals) memcpy(out_evals + 4 * (b * (n - 2) + (k - 2)), evals.data() + 4 * b, 4 * sizeof(gkr_fr));
            F cp, cq, lambda_next;
            FS::next_claims(k, evals.data() + 4 * b, r.data() + b * k, host_hash, z_next.data() + b * (k + 1), &cp, &cq, &lambda_next);
            claims[2 * b] = FS::abi(cp);
            claims[2 * b + 1] = FS::abi(cq);
            lambda[b] = FS::abi(lambda_next);
        }
        z.swap(z_next);
    }
    if (out_point) memcpy(out_point, z.data(), B * n * sizeof(gkr_fr));
    if (out_claims) memcpy(out_claims, claims.data(), B * 2 * sizeof(gkr_fr));
    return GKR_OK;
}

// ---- the verifier

// a chunk's share of the caller's arrays, in the ABI's layouts
struct Proofs {
    const gkr_fr *sums, *head, *coeffs, *r, *evals;
    const uint32_t* len;
    FS::Proof at(int n, size_t b) const {
        const size_t R = FS::rounds(n);
        return FS::Proof{sums ? sums + 2 * b : nullptr, head + 8 * b, coeffs + 4 * b * R, r + b * R, evals + 4 * b * (n - 2), len + b * R};
    }
};

// proofs of a chunk: what fits verify_workspace_mb (the evaluation's workspace, the point, the two values; with hashes the rows and slots)
size_t chunk_proofs(int n, int batch) {
    const size_t one = gkr::mle_eval_ws_bytes((uint32_t)n, 1, 2) + ((size_t)n + 2) * sizeof(Fr) +
                       FS::rounds(n) * (4 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
    return verify_chunk_size(one, 32768, batch);   // (the pair is a grid dimension of the launches)
}

int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, uint32_t nb, const Proofs& t, int* accept, uint32_t* failed_layer, uint32_t* failed_round,
                 uint32_t* failed_check, gkr_fr* out_sums) {
    const size_t R = FS::rounds(n);
    // ---- 1. the round vectors' hashes on the side stream: rows of four slots
    RoundHashes hashes(ctx, "fs.ver.", {RowSet{4u, (size_t)nb * R, {{t.coeffs, t.len}}}});
    if (const int rc = hashes.start()) return rc;
    // ---- 2. what needs neither a round vector's hash nor the tables: the form, the chain of claims and points, the layers' sums
    std::vector<FS::Pre> pre(nb);
    for_pieces(ctx, (nb + kRelPiece - 1) / kRelPiece, 8, [&](size_t a) {
        for (size_t b = a * kRelPiece; b < std::min<size_t>(nb, (a + 1) * kRelPiece); ++b) pre[b] = FS::pre_relations(n, t.at(n, b), host_hash);
    });
    // ---- 3. the device's share: N~(z^(n)) and D~(z^(n)) of the proofs still standing, at zero for the others
    Fr *h_pts = nullptr, *h_out = nullptr;
    HIP_TRY(ctx, ctx->pinned_host("fs.ver.pts", (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("fs.ver.out", (size_t)nb * 2 * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    memset(h_pts, 0, (size_t)nb * n * sizeof(Fr));
    for (uint32_t b = 0; b < nb; ++b)
        if (pre[b].point) memcpy(h_pts + (size_t)b * n, pre[b].z.data() + FS::layer_row(n), (size_t)n * sizeof(Fr));
    if (const int rc = queue_eval(ctx, "fs.ver.", d_tables, n, nb, 2u, h_pts, h_out)) return rc;
    if (const int rc = hashes.join()) return rc;
    // ---- 4. the host's hashes (if any) while the device works
    for_pieces(ctx, hashes.host_pieces(), 8, [&](size_t a) { hashes.hash_piece(a); });
    if (const int rc = hashes.sync_main()) return rc;
    const V::HashSlot* slots = hashes.slots();
    ctx->drain_events();
    for (uint32_t b = 0; b < nb; ++b) {
        FS::Verdict v;
        F vn, vd;
        memcpy(vn.l, &h_out[2 * (size_t)b], 32);
        memcpy(vd.l, &h_out[2 * (size_t)b + 1], 32);
        if (!FS::verdict(n, t.at(n, b), pre[b], slots + (size_t)b * R, vn, vd, &v))
            return ctx->fail(GKR_ERR_HIP, "fraction sum verifier: no hash for a well-formed round vector");
        accept[b] = v.check == 0 ? 1 : 0;
        if (failed_layer) failed_layer[b] = v.layer;
        if (failed_round) failed_round[b] = v.round;
        if (failed_check) failed_check[b] = v.check;
        if (out_sums) {
            F P = {{0, 0, 0, 0}}, Q = {{0, 0, 0, 0}};
            if (pre[b].point) FS::head_root(t.head + 8 * (size_t)b, &P, &Q);
            out_sums[2 * (size_t)b] = FS::abi(P);
            out_sums[2 * (size_t)b + 1] = FS::abi(Q);
        }
    }
    return GKR_OK;
}

}  // namespace

// =========================================================================== C ABI

extern "C" {

int gkr_fraction_sum_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_sums, gkr_fr* out_head, gkr_fr* out_coeffs,
                                  uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    if (!ctx || !d_tables || !out_sums || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!fs_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return run_fraction_sum(ctx, static_cast<const Fr*>(d_tables), n, batch, out_sums, out_head, out_coeffs, out_len, out_r, out_evals, out_point,
                            out_claims);
}

int gkr_fraction_sum(gkr_ctx* ctx, const gkr_fr* numerators, const gkr_fr* denominators, int n, gkr_fr* out_sum, gkr_fr* out_head, gkr_fr* out_coeffs,
                     uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    if (!ctx || !numerators || !denominators || !out_sum || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!fs_shape(n, 1)) return GKR_ERR_INVALID;
    std::vector<gkr_fr> pair((size_t)2 << n);   // the pair as the device holds it: N then D
    memcpy(pair.data(), numerators, sizeof(gkr_fr) << n);
    memcpy(pair.data() + ((size_t)1 << n), denominators, sizeof(gkr_fr) << n);
    return run_on_tables(ctx, pair.data(), pair.size(), [&](const Fr* d) {
        return run_fraction_sum(ctx, d, n, 1, out_sum, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims);
    });
}

int gkr_fraction_sum_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* sums, const gkr_fr* head,
                                         const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept,
                                         uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_sums) {
    if (!ctx || !d_tables || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!fs_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    const size_t R = FS::rounds(n);
    return for_chunks(batch, chunk_proofs(n, batch), [&](size_t b, uint32_t nb) {
        const Proofs t{sums ? sums + 2 * b : nullptr, head + 8 * b, coeffs + 4 * b * R, r + b * R, evals + 4 * b * (n - 2), len + b * R};
        return verify_chunk(ctx, static_cast<const Fr*>(d_tables) + (b << (n + 1)), n, nb, t, accept + b, failed_layer ? failed_layer + b : nullptr,
                            failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                            out_sums ? out_sums + 2 * b : nullptr);
    });
}

int gkr_fraction_sum_verify(gkr_ctx* ctx, const gkr_fr* numerators, const gkr_fr* denominators, int n, const gkr_fr* sum, const gkr_fr* head,
                            const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept, uint32_t* failed_layer,
                            uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !numerators || !denominators || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!fs_shape(n, 1)) return GKR_ERR_INVALID;
    std::vector<gkr_fr> pair((size_t)2 << n);
    memcpy(pair.data(), numerators, sizeof(gkr_fr) << n);
    memcpy(pair.data() + ((size_t)1 << n), denominators, sizeof(gkr_fr) << n);
    return run_on_tables(ctx, pair.data(), pair.size(), [&](const Fr* d) {
        return gkr_fraction_sum_verify_batch_device(ctx, d, n, 1, sum, head, coeffs, len, r, evals, accept, failed_layer, failed_round, failed_check,
                                                    nullptr);
    });
}

int gkr_selftest_fraction_sum_geometry(int n, uint32_t* blocks) {
    if (!blocks || n < 3 || n > GKR_MAX_MLE_N) return GKR_ERR_INVALID;
    for (int k = 0; k < n; ++k) blocks[k] = gkr::fs_level_blocks((uint32_t)k);
    return GKR_OK;
}

int gkr_devtest_fraction_sum_tree(gkr_ctx* ctx, const void* d_tables, int n, int batch, void* d_layers) {
    if (!ctx || !d_tables || !d_layers || !fs_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    if (const int rc = queue_tree(ctx, static_cast<const Fr*>(d_tables), n, batch, static_cast<Fr*>(d_layers))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

int gkr_devtest_fraction_sum_chunk(gkr_ctx* ctx, int n, int batch, uint32_t* out) {
    if (!ctx || !out || !fs_shape(n, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    *out = (uint32_t)chunk_proofs(n, batch);
    return GKR_OK;
}

}  // extern "C"

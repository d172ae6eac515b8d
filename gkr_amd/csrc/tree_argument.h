// The driver and the device verifier of a GKR TREE ARGUMENT -- the grand product (capi_grand_product.hip) and the fractional sum
// (capi_fraction_sum.hip) -- over resident tables: the tree on the device, then layer by layer k = 2 .. n-1 one zero-check on the
// contiguous halves of the level below -- no gather, no copy -- chained by Fiat-Shamir on the host (tree_rounds.h); and the
// verifier of such proofs, whose round relations are verify_rounds.h's and whose one read of the input tables is
// kernels_mle_eval.hip's.  ONE statement of both, for every argument description A:
//   A::Gate                      the argument's gate (tree_rounds.h); W = Gate::W tables per proof, every width below follows from it;
//   A::kLayers, A::kVer          the workspace slot of the prover's tree and the prefix of the verifier's slots;
//   A::kTree, A::kTreeNodeBytes  the tree launches' Timed label and their bytes per input node;
//   A::kNoHash                   the text of the verifier's error of the call;
//   A::launch_tree, A::layer_offset, A::level_blocks     the argument's tree kernels (kernels.h);
//   A::run_layer(ctx, tables, k, batch, z, lambda, out_coeffs, out_len, out_r, out_evals)    `batch` zero-checks of layer k on the
//                                2 W halves per proof at `tables`, z: batch x k, lambda: batch (empty where the gate draws none).
//
// The verifier builds a chunk of proofs from verify_chunk.h's pieces, which states the plan.  Particular to the tree arguments:
//   - one set of round vectors, rows of four slots, all layers of a proof next to each other;
//   - the host's relations (the shape and canonical checks of the whole proof, zeta, every tau_k, claim and z^(k), the layers' round
//     sums and Horner steps: tree_rounds.h) run BEFORE the device's share is queued, because the points z^(n) come out of them:
//     those of the proofs that passed SHAPE and NON_CANONICAL go up, zeros for the others, whose verdict is decided.
//     The host's hashes (if any) run after it is queued, while the device works;
//   - the device's share is the one evaluation of every proof's W tables at its one point (groups of W tables); per proof the
//     first failure in order.
// Not a public header.
#pragma once
#include "verify_chunk.h"
#include "tree_rounds.h"

namespace gkr_host {

template <class A>
struct TreeArgument {
    using G = typename A::Gate;
    using F = gkr::h64::F;
    static constexpr size_t W = G::W;
    static constexpr size_t kRelPiece = 4;   // proofs per piece of host work

    // the shapes both the prover and the verifier admit (plain returns: decided before the context is looked at): the zero-check's
    // own limit on the top layer's 2 W tables
    static bool shape(int n, int batch) {
        return batch >= 1 && batch <= 65535 && n >= 3 && n <= GKR_MAX_MLE_N && ((W * (unsigned long long)batch) << n) <= (1ull << 30);
    }

    static F host_hash(const F* v, int len) { return host_multi_hash(v, len, host_mimc_constants64()); }

    static int queue_tree(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, Fr* d_layers) {
        Timed t(ctx, A::kTree, (double)batch * A::kTreeNodeBytes * (double)((size_t)1 << n));
        A::launch_tree(d_tables, (uint32_t)n, (uint32_t)batch, d_layers, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        return GKR_OK;
    }

    // the whole of the *_batch_device prover behind its argument checks
    static int prove(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, gkr_fr* out_root, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len,
                     gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
        hipStream_t s = ctx->stream;
        const size_t B = (size_t)batch, R = gkr::tree::rounds(n);
        Fr* d_layers = nullptr;
        WS(ctx, A::kLayers, Fr, W * B * (((size_t)1 << n) - 1), d_layers);
        if (const int rc = queue_tree(ctx, d_tables, n, batch, d_layers)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(out_head, d_layers + A::layer_offset(2, (uint32_t)batch), B * 4 * W * sizeof(Fr), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipMemcpyAsync(out_root, d_layers, B * W * sizeof(Fr), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        // the head: z^(2) and, where drawn, lambda_2 of every proof (the claims are the verifier's to check; the prover's chain
        // needs these alone)
        std::vector<gkr_fr> z(B * 2), z_next, lambda(G::kLambda ? B : 0);
        for (size_t b = 0; b < B; ++b) {
            const auto link = gkr::tree::head_link<G>(out_head + 4 * W * b, host_hash, z.data() + 2 * b);
            if constexpr (G::kLambda) lambda[b] = gkr::tree::abi(link.lambda);
        }
        std::vector<gkr_fr> coeffs, r, evals(B * 2 * W), claims(B * W);
        std::vector<uint32_t> len;
        for (int k = 2; k < n; ++k) {
            const Fr* tables = k + 1 == n ? d_tables : d_layers + A::layer_offset((uint32_t)k + 1, (uint32_t)batch);
            coeffs.resize(B * k * 4);
            len.resize(B * k);
            r.resize(B * k);
            if (const int rc = A::run_layer(ctx, tables, k, batch, z.data(), lambda.data(), coeffs.data(), len.data(), r.data(), evals.data())) return rc;
            const size_t row = gkr::tree::layer_row(k);
            z_next.resize(B * (k + 1));
            for (size_t b = 0; b < B; ++b) {
                memcpy(out_coeffs + 4 * (b * R + row), coeffs.data() + 4 * b * k, (size_t)k * 4 * sizeof(gkr_fr));
                memcpy(out_len + b * R + row, len.data() + b * k, (size_t)k * sizeof(uint32_t));
                memcpy(out_r + b * R + row, r.data() + b * k, (size_t)k * sizeof(gkr_fr));
                if (out_evals) memcpy(out_evals + 2 * W * (b * (n - 2) + (k - 2)), evals.data() + 2 * W * b, 2 * W * sizeof(gkr_fr));
                const auto link = gkr::tree::next_link<G>(k, evals.data() + 2 * W * b, r.data() + b * k, host_hash, z_next.data() + b * (k + 1));
                for (size_t w = 0; w < W; ++w) claims[W * b + w] = gkr::tree::abi(link.c[w]);
                if constexpr (G::kLambda) lambda[b] = gkr::tree::abi(link.lambda);
            }
            z.swap(z_next);
        }
        if (out_point) memcpy(out_point, z.data(), B * n * sizeof(gkr_fr));
        if (out_claims) memcpy(out_claims, claims.data(), B * W * sizeof(gkr_fr));
        return GKR_OK;
    }

    // ---- the verifier

    // proof b of the proofs whose arrays, in the ABI's layouts, start at t's (a chunk's share of the caller's; one proof of a chunk)
    static gkr::tree::Proof at(const gkr::tree::Proof& t, int n, size_t b) {
        const size_t R = gkr::tree::rounds(n);
        return {t.claimed ? t.claimed + W * b : nullptr, t.head + 4 * W * b, t.coeffs + 4 * b * R, t.r + b * R, t.evals + 2 * W * b * (n - 2), t.len + b * R};
    }

    // proofs of a chunk: what fits verify_workspace_mb (the evaluation's workspace, the point, the W values; with hashes the rows and slots)
    static size_t chunk_proofs(int n, int batch) {
        const size_t one = gkr::mle_eval_ws_bytes((uint32_t)n, 1, (uint32_t)W) + ((size_t)n + W) * sizeof(Fr) +
                           gkr::tree::rounds(n) * (4 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
        return verify_chunk_size(one, 32768, batch);   // (the group of W tables is a grid dimension of the launches)
    }

    // out_root: the head's W root values per proof (zeros without a point), or null
    static int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, uint32_t nb, const gkr::tree::Proof& t, int* accept, uint32_t* failed_layer,
                            uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_root) {
        const size_t R = gkr::tree::rounds(n);
        const std::string pts = std::string(A::kVer) + "pts", out = std::string(A::kVer) + "out";
        // ---- 1. the round vectors' hashes on the side stream: rows of four slots
        RoundHashes hashes(ctx, A::kVer, {RowSet{4u, (size_t)nb * R, {{t.coeffs, t.len}}}});
        if (const int rc = hashes.start()) return rc;
        // ---- 2. what needs neither a round vector's hash nor the tables: the form, the chain of claims and points, the layers' sums
        std::vector<gkr::tree::Pre<G>> pre(nb);
        for_pieces(ctx, (nb + kRelPiece - 1) / kRelPiece, 8, [&](size_t a) {
            for (size_t b = a * kRelPiece; b < std::min<size_t>(nb, (a + 1) * kRelPiece); ++b) pre[b] = gkr::tree::pre_relations<G>(n, at(t, n, b), host_hash);
        });
        // ---- 3. the device's share: the W tables at z^(n) of the proofs still standing, at zero for the others
        Fr *h_pts = nullptr, *h_out = nullptr;
        HIP_TRY(ctx, ctx->pinned_host(pts.c_str(), (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
        HIP_TRY(ctx, ctx->pinned_host(out.c_str(), (size_t)nb * W * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
        memset(h_pts, 0, (size_t)nb * n * sizeof(Fr));
        for (uint32_t b = 0; b < nb; ++b)
            if (pre[b].point) memcpy(h_pts + (size_t)b * n, pre[b].z.data() + gkr::tree::layer_row(n), (size_t)n * sizeof(Fr));
        if (const int rc = queue_eval(ctx, A::kVer, d_tables, n, nb, (uint32_t)W, h_pts, h_out)) return rc;
        if (const int rc = hashes.join()) return rc;
        // ---- 4. the host's hashes (if any) while the device works
        for_pieces(ctx, hashes.host_pieces(), 8, [&](size_t a) { hashes.hash_piece(a); });
        if (const int rc = hashes.sync_main()) return rc;
        const gkr::verify::HashSlot* slots = hashes.slots();
        ctx->drain_events();
        for (uint32_t b = 0; b < nb; ++b) {
            gkr::tree::Verdict v;
            F values[W], root[W] = {};
            memcpy(values, &h_out[W * (size_t)b], W * 32);
            if (!gkr::tree::verdict<G>(n, at(t, n, b), pre[b], slots + (size_t)b * R, values, &v)) return ctx->fail(GKR_ERR_HIP, A::kNoHash);
            accept[b] = v.check == 0 ? 1 : 0;
            if (failed_layer) failed_layer[b] = v.layer;
            if (failed_round) failed_round[b] = v.round;
            if (failed_check) failed_check[b] = v.check;
            if (out_root) {
                if (pre[b].point) G::root(t.head + 4 * W * (size_t)b, root);
                memcpy(out_root + W * (size_t)b, root, W * 32);
            }
        }
        return GKR_OK;
    }

    // ---- the bodies of the C ABI's entry points: null pointers, then the shape, then the context

    static int prove_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_root, gkr_fr* out_head, gkr_fr* out_coeffs,
                                  uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
        if (!ctx || !d_tables || !out_root || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
        if (!shape(n, batch)) return GKR_ERR_INVALID;
        GKR_ENTER(ctx);
        return prove(ctx, static_cast<const Fr*>(d_tables), n, batch, out_root, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims);
    }

    static int verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr::tree::Proof& t, int* accept, uint32_t* failed_layer,
                                   uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_root) {
        if (!ctx || !d_tables || !t.head || !t.coeffs || !t.len || !t.r || !t.evals || !accept) return GKR_ERR_INVALID;
        if (!shape(n, batch)) return GKR_ERR_INVALID;
        GKR_ENTER(ctx);
        return for_chunks(batch, chunk_proofs(n, batch), [&](size_t b, uint32_t nb) {
            return verify_chunk(ctx, static_cast<const Fr*>(d_tables) + W * (b << n), n, nb, at(t, n, b), accept + b, failed_layer ? failed_layer + b : nullptr,
                                failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                                out_root ? out_root + W * b : nullptr);
        });
    }

    static int geometry(int n, uint32_t* blocks) {
        if (!blocks || n < 3 || n > GKR_MAX_MLE_N) return GKR_ERR_INVALID;
        for (int k = 0; k < n; ++k) blocks[k] = A::level_blocks((uint32_t)k);
        return GKR_OK;
    }

    static int devtest_tree(gkr_ctx* ctx, const void* d_tables, int n, int batch, void* d_layers) {
        if (!ctx || !d_tables || !d_layers || !shape(n, batch)) return GKR_ERR_INVALID;
        GKR_ENTER(ctx);
        if (const int rc = queue_tree(ctx, static_cast<const Fr*>(d_tables), n, batch, static_cast<Fr*>(d_layers))) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->drain_events();
        return GKR_OK;
    }

    static int devtest_chunk(gkr_ctx* ctx, int n, int batch, uint32_t* out) {
        if (!ctx || !out || !shape(n, batch)) return GKR_ERR_INVALID;
        GKR_ENTER(ctx);
        *out = (uint32_t)chunk_proofs(n, batch);
        return GKR_OK;
    }
};

}  // namespace gkr_host

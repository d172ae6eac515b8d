// The grand product P = prod_i V[i] over resident tables as GKR on the binary tree of multiplication gates: the tree on the device
// (kernels_grand_product.hip), then layer by layer the zero-check  L_k(z) = sum_x eq(z, x) L_{k+1}(0, x) L_{k+1}(1, x)  through
// capi_resident.hip's run_zerocheck_batch on the two contiguous halves of the level below -- no gather, no copy, no sumcheck kernel
// of this path's own -- chained by Fiat-Shamir on the host (grand_product_rounds.h); and the verifier of such proofs, whose round
// relations are verify_rounds.h's and whose one read of V is kernels_mle_eval.hip's.  C ABI: include/gkr_amd.h.
//
// The verifier, per chunk of proofs (as many as fit verify_workspace_mb), in the manner of capi_r1cs_verify.hip:
//   1. the chunk's round vectors start hashing: on the device (the side stream) from verify_device_hash_min of them on, else on
//      the host threads in step 4;
//   2. the host threads run the shape and canonical checks of the whole proof, zeta, every tau_k, c_k and z^(k), and the layers'
//      round sums and Horner steps;
//   3. the points z^(n) of the proofs that passed SHAPE and NON_CANONICAL go up -- zeros for the others, whose verdict is
//      decided -- and the one evaluation of every table is launched;
//   4. the host hashes (if any) run while the device works; ONE synchronisation; then per proof the first failure in order.
#include <atomic>

#include "capi_internal.h"
#include "grand_product_rounds.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
namespace GP = gkr::gp;

constexpr int kRelPiece = 4, kHashPiece = 16;   // proofs / round vectors per piece of host work

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
    long long mb = gkr::opt(gkr::OPT_verify_workspace_mb);
    if (mb <= 0) mb = 2048;
    const size_t one = gkr::mle_eval_ws_bytes((uint32_t)n, 1, 1) + ((size_t)n + 1) * sizeof(Fr) +
                       GP::rounds(n) * (4 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
    const size_t chunk = ((size_t)mb << 20) / one;
    return std::max<size_t>(1, std::min<size_t>({chunk, (size_t)32768, (size_t)batch}));   // (the table is a grid dimension of the launches)
}

int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, uint32_t nb, const Proofs& t, int* accept, uint32_t* failed_layer, uint32_t* failed_round,
                 uint32_t* failed_check, gkr_fr* out_products) {
    hipStream_t st = ctx->stream;
    const size_t R = GP::rounds(n), n_rows = (size_t)nb * R;
    const bool dev_hash = verify_device_hash_wanted(n_rows);
    // the side stream's work is joined on every way out: nothing may still read or write a workspace the next call reuses
    struct SideJoin {
        hipStream_t forked = nullptr;
        ~SideJoin() {
            if (forked) (void)hipStreamSynchronize(forked);
        }
    } side;
    // ---- 1. the round vectors' hashes on the side stream: rows of four slots
    std::vector<V::HashSlot> host_slots(dev_hash ? 0 : n_rows);
    const V::HashSlot* slots = host_slots.data();
    if (dev_hash) {
        const size_t words = n_rows * 33;   // rows, then lengths
        uint32_t *d_hin = nullptr, *h_hin = nullptr;
        gkr::VerifyHashSlot *d_hout = nullptr, *h_hout = nullptr;
        WS(ctx, "gp.ver.hash_in", uint32_t, words, d_hin);
        WS(ctx, "gp.ver.hash_out", gkr::VerifyHashSlot, n_rows, d_hout);
        HIP_TRY(ctx, ctx->pinned_host("gp.ver.hash_in", words * sizeof(uint32_t), reinterpret_cast<void**>(&h_hin)));
        HIP_TRY(ctx, ctx->pinned_host("gp.ver.hash_out", n_rows * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_hout)));
        memcpy(h_hin, t.coeffs, n_rows * 32 * sizeof(uint32_t));
        memcpy(h_hin + n_rows * 32, t.len, n_rows * sizeof(uint32_t));
        HIP_TRY(ctx, ctx->aux_stream(2));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[0], st));             // fork: after whatever the main stream still holds
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->aux_events[0], 0));
        side.forked = ctx->aux;
        HIP_TRY(ctx, hipMemcpyAsync(d_hin, h_hin, words * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->aux));
        if (const int rc = verify_hash_rows_device(ctx, 4, d_hin, d_hin + n_rows * 32, n_rows, d_hout, ctx->aux)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(h_hout, d_hout, n_rows * sizeof(gkr::VerifyHashSlot), hipMemcpyDeviceToHost, ctx->aux));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[1], ctx->aux));
        slots = reinterpret_cast<const V::HashSlot*>(h_hout);
    }
    // ---- 2. what needs neither a round vector's hash nor V: the form, the chain of claims and points, the layers' sums
    std::vector<GP::Pre> pre(nb);
    {
        const size_t pieces = (nb + kRelPiece - 1) / kRelPiece;
        std::atomic<size_t> next{0};
        const std::function<bool()> work = [&] {
            const size_t a = next.fetch_add(1, std::memory_order_relaxed);
            if (a >= pieces) return false;
            for (size_t b = a * kRelPiece; b < std::min<size_t>(nb, (a + 1) * kRelPiece); ++b) pre[b] = GP::pre_relations(n, t.at(n, b), host_hash);
            return true;
        };
        gkr::SpinPool* pool = pieces >= 8 ? ctx->host_pool() : nullptr;
        gkr::SpinPool::Session session(pool, &work);
        while (work()) {
        }
    }
    // ---- 3. the device's share: V~(z^(n)) of the proofs still standing, at zero for the others
    Fr *h_pts = nullptr, *h_out = nullptr, *d_pts = nullptr, *d_out = nullptr;
    void* d_ws = nullptr;
    HIP_TRY(ctx, ctx->pinned_host("gp.ver.points", (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("gp.ver.out", (size_t)nb * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    WS(ctx, "gp.ver.points", Fr, (size_t)nb * n, d_pts);
    WS(ctx, "gp.ver.out", Fr, nb, d_out);
    HIP_TRY(ctx, ctx->workspace("gp.ver.eval_ws", gkr::mle_eval_ws_bytes((uint32_t)n, nb, 1), &d_ws));
    memset(h_pts, 0, (size_t)nb * n * sizeof(Fr));
    for (uint32_t b = 0; b < nb; ++b)
        if (pre[b].point) memcpy(h_pts + (size_t)b * n, pre[b].z.data() + GP::layer_row(n), (size_t)n * sizeof(Fr));
    HIP_TRY(ctx, hipMemcpyAsync(d_pts, h_pts, (size_t)nb * n * sizeof(Fr), hipMemcpyHostToDevice, st));
    {
        Timed tm(ctx, "mle_eval", (double)nb * 32.0 * (double)((size_t)1 << n));
        gkr::launch_mle_eval(d_tables, (uint32_t)n, nb, 1u, d_pts, d_ws, d_out, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)nb * sizeof(Fr), hipMemcpyDeviceToHost, st));
    if (dev_hash) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->aux_events[1], 0));   // join: the main stream's end is the side stream's too
    // ---- 4. the host's hashes while the device works, in pieces of kHashPiece round vectors
    if (!dev_hash) {
        const size_t pieces = (n_rows + kHashPiece - 1) / kHashPiece;
        std::atomic<size_t> next{0};
        const std::function<bool()> work = [&] {
            const size_t a = next.fetch_add(1, std::memory_order_relaxed);
            if (a >= pieces) return false;
            for (size_t s = a * kHashPiece; s < std::min(n_rows, (a + 1) * kHashPiece); ++s) host_hash_slot(t.coeffs + 4 * s, 4u, t.len[s], &host_slots[s]);
            return true;
        };
        gkr::SpinPool* pool = pieces >= 8 ? ctx->host_pool() : nullptr;
        gkr::SpinPool::Session session(pool, &work);
        while (work()) {
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    side.forked = nullptr;
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
    const size_t chunk = chunk_proofs(n, batch), R = GP::rounds(n);
    for (size_t b = 0; b < (size_t)batch; b += chunk) {
        const uint32_t nb = (uint32_t)std::min(chunk, (size_t)batch - b);
        const Proofs t{products ? products + b : nullptr, head + 4 * b, coeffs + 4 * b * R, r + b * R, evals + 2 * b * (n - 2), len + b * R};
        const int rc = verify_chunk(ctx, static_cast<const Fr*>(d_tables) + (b << n), n, nb, t, accept + b, failed_layer ? failed_layer + b : nullptr,
                                    failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                                    out_products ? out_products + b : nullptr);
        if (rc) return rc;
    }
    return GKR_OK;
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

// The verifiers of the plain sumcheck, of the sumcheck over a product and of the one over a sum of products of resident tables, and
// the multilinear evaluation behind them: gkr_mle_eval_batch_device, gkr_sumcheck_mle_verify_batch_device, gkr_sumcheck_mle_verify,
// gkr_sumcheck_product_verify_batch_device, gkr_sumcheck_product_verify, gkr_sumcheck_sop_verify_batch_device,
// gkr_sumcheck_sop_verify.  ONE driver, parametrised by a term structure (Terms): M tables per sumcheck, rows of D + 1 slots (D the
// largest term degree), the last relation g_n(r_n) = sum_k c_k prod_j T_t(k,j)(r_1 .. r_n).  The plain sumcheck is the one term
// {1, {0}}, the product of D tables the one term {D, {0 .. D-1}}, both with coefficient 1; what follows says T for all of them.
//
// verify_sumcheck (python/sumcheck.py:55-70) is O(n) per transcript; what makes a transcript of prove_sumcheck checkable is the
// relation behind it, g_n(r_n) = T(r_1 .. r_n), one pass over the table.  A verifier reads every challenge out of the transcript,
// so nothing on the device waits for the host: per chunk of tables (as many as fit verify_workspace_mb of workspace; verdicts
// do not depend on the chunking)
//   1. the points (the transcripts' challenges, ONE point per sumcheck: its M tables share it) go up in ONE copy and the
//      evaluation is launched (kernels_mle_eval.hip: a few set-up launches over the chunk's points, one streaming read of every
//      table, the second-level sums; one copy back);
//   2. the chunk's batch x n challenge hashes start: a chunk of at least verify_device_hash_min round vectors sends them to the
//      device (verify_chunk.h's RoundHashes, on the side stream beside the evaluation; rows of two slots are repacked to the
//      kernel's three on the way into the staging buffer, rows of three and four go as they are), a smaller one hashes on the
//      context's host threads.  Both fill the same slots by the same rule, so verdicts do not depend on where the hashes ran;
//   3. meanwhile the host threads run everything that needs neither: shape, canonical checks, the round sums and the Horner
//      steps of every transcript (pre_relations; verify_rounds.h holds the round relations, the R1CS verifier uses them too);
//   4. ONE synchronisation, then per transcript the challenge comparisons and the last relation (finish).
// The order of the checks is the reference's; a value computed from unchecked elements (a hash of a malformed row, T at a
// non-canonical point) is never consulted: checks 1 and 2 come first.
#include "verify_chunk.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;

using V::HashSlot;   // (verify_rounds.h)
using V::Pre;
using V::pre_relations;
constexpr size_t kRelPiece = 8;   // transcripts per piece of host work

// ONE driver for all the verifiers, parametrised by the sumcheck's term structure: a transcript's rows have D + 1 right-aligned
// slots and it is tied to M resident tables, next to each other.  The hash kernel's rows have three slots up to D = 2 and four
// at D = 3.
struct Terms {
    int M = 0, D = 0, K = 0;                 // tables per sumcheck, the largest term degree, terms
    uint32_t term[gkr::kSopMaxTerms] = {};   // gkr::SopTerms' form: degree | table 0 << 8 | table 1 << 16 | table 2 << 24
    F coeff[gkr::kSopMaxTerms] = {};         // Montgomery form
};
// the product of `degree` tables (degree 1: the plain sumcheck): one term of coefficient 1 over the tables 0 .. degree - 1
Terms product_terms(int degree) {
    Terms t;
    t.M = t.D = degree;
    t.K = 1;
    t.term[0] = (uint32_t)degree | 0u << 8 | 1u << 16 | 2u << 24;
    t.coeff[0] = gkr::h64::to_mont(F{{1, 0, 0, 0}});
    return t;
}
// the caller's terms as sop_shape / sop_coeffs (capi_sop.hip) took them
Terms sop_terms(const gkr::SopTerms& ts, const gkr::SopCoeffs& cf) {
    Terms t;
    t.M = (int)ts.n_tables;
    t.D = (int)ts.max_degree;
    t.K = (int)ts.n_terms;
    for (int k = 0; k < t.K; ++k) {
        t.term[k] = ts.term[k];
        F c;
        memcpy(c.l, &cf.c[k], 32);
        t.coeff[k] = gkr::h64::to_mont(c);
    }
    return t;
}
inline size_t row_width(int degree) { return (size_t)degree + 1; }
inline int hash_slots(int degree) { return degree <= 2 ? 3 : 4; }

// the verdict of one transcript from what the host found, its hash slots and the device's values T_m(r) of its T.M tables
int finish(gkr_ctx* ctx, int n, const Terms& T, const Pre& p, const HashSlot* slots, const gkr_fr* r, const Fr* values, int* accept,
           uint32_t* failed_round, uint32_t* failed_check) {
    uint32_t check = 0, round = 0;
    if (!V::round_verdict(n, p, slots, r, &check, &round)) return ctx->fail(GKR_ERR_HIP, "sumcheck verifier: no hash for a well-formed round vector");
    if (!check) {
        F total = {{0, 0, 0, 0}};                                    // sum_k c_k prod_j T_t(k,j)(r)
        for (int k = 0; k < T.K; ++k) {
            const uint32_t d = T.term[k] & 0xFFu;
            F prod = T.coeff[k];                                     // Montgomery, then canonical: a b = mont_mul(to_mont(a), b)
            for (uint32_t j = 0; j < d; ++j) {
                F v;
                memcpy(v.l, &values[(T.term[k] >> (8u + 8u * j)) & 0xFFu], 32);
                prod = gkr::h64::mont_mul(j ? gkr::h64::to_mont(prod) : prod, v);
            }
            total = gkr::h64::add(total, prod);
        }
        if (!V::same(p.last, total)) {
            check = GKR_VERIFY_EVALUATION;
            round = (uint32_t)n;
        }
    }
    *accept = check == 0 ? 1 : 0;
    if (failed_round) *failed_round = round;
    if (failed_check) *failed_check = check;
    return GKR_OK;
}

// sumchecks of a chunk: what fits verify_workspace_mb.  Chunks are counted in sumchecks: the M tables of a sumcheck are never
// split over two chunks.  A sumcheck's price is an upper bound of its share, M times what a table evaluated on its own needs
// (plan, weights, half tables, partials, point, value) and its n hash rows: the plan, the weights and the half tables are in fact
// built once per sumcheck (queue_eval allocates that much), but the price per table is what the chunk boundaries of the plain
// and the product verifier have been and stays, so that no call's chunking moves.
size_t chunk_tables(int n, int M, int D, int batch, bool hashes) {
    const size_t hash_row = (size_t)hash_slots(D) * 8 * sizeof(uint32_t);
    const size_t one = (size_t)M * (gkr::mle_eval_ws_bytes((uint32_t)n, 1, 1) + (size_t)n * sizeof(Fr) + sizeof(Fr)) +
                       (hashes ? (size_t)n * (hash_row + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot)) : 0);
    return verify_chunk_size(one, (size_t)32768 / M, batch);   // (the table is a grid dimension of the launches)
}

int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, const Terms& T, uint32_t nb, const gkr_fr* claims, const gkr_fr* coeffs, const uint32_t* len,
                 const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_claims, gkr_fr* out_evals) {
    const int degree = T.D;   // of the round polynomials: the rows' and the hash kernel's form
    const size_t n_rows = (size_t)nb * n, W = row_width(degree), M = (size_t)T.M, nt = (size_t)nb * M;
    RoundHashes hashes(ctx, "mlev_", {RowSet{(uint32_t)W, n_rows, {{coeffs, len}}}});
    // ---- the device's share: hashes on the side stream, the evaluation on the main stream
    Fr *h_pts, *h_out;
    HIP_TRY(ctx, ctx->pinned_host("mlev_pts", n_rows * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("mlev_out", nt * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    if (const int rc = hashes.start()) return rc;
    memcpy(h_pts, r, n_rows * sizeof(Fr));   // a sumcheck's point once: its M tables share it
    if (const int rc = queue_eval(ctx, "mlev_", d_tables, n, nb, (uint32_t)M, h_pts, h_out)) return rc;
    if (const int rc = hashes.join()) return rc;
    // ---- the host's share while the device streams, in ONE job: (host hashing) the pieces of round vectors first -- they are the
    //      long ones -- then the relations of kRelPiece transcripts a piece
    std::vector<Pre> pre(nb);
    const size_t rel_pieces = (nb + kRelPiece - 1) / kRelPiece, hash_pieces = hashes.host_pieces();
    for_pieces(ctx, hash_pieces + rel_pieces, 8, [&](size_t a) {
        if (a < hash_pieces) return hashes.hash_piece(a);
        for (size_t b = (a - hash_pieces) * kRelPiece; b < std::min<size_t>(nb, (a - hash_pieces + 1) * kRelPiece); ++b)
            pre[b] = pre_relations(n, degree, claims ? claims + b : nullptr, coeffs + W * b * n, len + b * n, r + b * n);
    });
    if (const int rc = hashes.sync_main()) return rc;
    const HashSlot* slots = hashes.slots();
    for (uint32_t b = 0; b < nb; ++b) {
        const Fr* values = h_out + (size_t)b * M;
        const int rc = finish(ctx, n, T, pre[b], slots + (size_t)b * n, r + (size_t)b * n, values, &accept[b],
                              failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr);
        if (rc) return rc;
        // the proven sum and the tables' values of a transcript that passed checks 1 and 2; zero otherwise (its point is no point)
        if (out_claims) {
            memset(&out_claims[b], 0, sizeof(gkr_fr));
            if (!pre[b].check) memcpy(out_claims[b].l, pre[b].proved.l, 32);
        }
        if (out_evals) {
            memset(out_evals + (size_t)b * M, 0, M * sizeof(gkr_fr));
            if (!pre[b].check) memcpy(out_evals + (size_t)b * M, values, M * sizeof(gkr_fr));
        }
    }
    return GKR_OK;
}

int verify_batch(gkr_ctx* ctx, const Fr* d_tables, int n, const Terms& T, int batch, const gkr_fr* claims, const gkr_fr* coeffs, const uint32_t* len,
                 const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_claims, gkr_fr* out_evals) {
    const size_t W = row_width(T.D), M = (size_t)T.M;
    return for_chunks(batch, chunk_tables(n, T.M, T.D, batch, true), [&](size_t b, uint32_t nb) {
        return verify_chunk(ctx, d_tables + ((b * M) << n), n, T, nb, claims ? claims + b : nullptr, coeffs + W * b * n, len + b * n, r + b * n,
                            accept + b, failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                            out_claims ? out_claims + b : nullptr, out_evals ? out_evals + b * M : nullptr);
    });
}

}  // namespace

extern "C" {

int gkr_mle_eval_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* points, gkr_fr* out) {
    // (plain returns: these are decided before the context is looked at)
    if (!ctx || !d_tables || !points || !out || batch < 1 || n < 1 || n > 30) return GKR_ERR_INVALID;
    if (!all_canonical(points, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "coordinate of a point >= r");
    GKR_ENTER(ctx);
    return for_chunks(batch, chunk_tables(n, 1, 1, batch, false), [&](size_t b, uint32_t nb) -> int {
        Fr *h_pts, *h_out;
        HIP_TRY(ctx, ctx->pinned_host("mlev_pts", (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
        HIP_TRY(ctx, ctx->pinned_host("mlev_out", (size_t)nb * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
        memcpy(h_pts, points + b * n, (size_t)nb * n * sizeof(Fr));
        if (const int rc = queue_eval(ctx, "mlev_", static_cast<const Fr*>(d_tables) + (b << n), n, nb, 1u, h_pts, h_out)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(out + b, h_out, (size_t)nb * sizeof(Fr));
        return GKR_OK;
    });
}

int gkr_sumcheck_mle_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* claims, const gkr_fr* coeffs,
                                         const uint32_t* len, const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check,
                                         gkr_fr* out_claims) {
    if (!ctx || !d_tables || !coeffs || !len || !r || !accept || batch < 1 || n < 2 || n > 30) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return verify_batch(ctx, static_cast<const Fr*>(d_tables), n, product_terms(1), batch, claims, coeffs, len, r, accept, failed_round, failed_check, out_claims, nullptr);
}

int gkr_sumcheck_mle_verify(gkr_ctx* ctx, const gkr_fr* table, int n, const gkr_fr* claim, const gkr_fr* coeffs, const uint32_t* len,
                            const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !table || !coeffs || !len || !r || !accept || n < 2 || n > 30) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    const size_t count = (size_t)1 << n;
    DevBuf<Fr> d;
    {
        const hipError_t e = d.alloc(count);
        if (e != hipSuccess) return alloc_status(ctx, e, "gkr_sumcheck_mle_verify: the table");
    }
    HIP_TRY(ctx, hipMemcpyAsync(d.p, table, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return verify_batch(ctx, d.p, n, product_terms(1), 1, claim, coeffs, len, r, accept, failed_round, failed_check, nullptr, nullptr);
}

// ---- the product sumcheck's verifier: the same driver with one term of degree 1 .. GKR_PRODUCT_MAX_DEGREE, argument checks as the prover's

int gkr_sumcheck_product_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int degree, int batch, const gkr_fr* claims,
                                             const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, int* accept, uint32_t* failed_round,
                                             uint32_t* failed_check, gkr_fr* out_claims, gkr_fr* out_evals) {
    if (!ctx || !d_tables || !coeffs || !len || !r || !accept || batch < 1 || batch > 65535) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return verify_batch(ctx, static_cast<const Fr*>(d_tables), n, product_terms(degree), batch, claims, coeffs, len, r, accept, failed_round,
                        failed_check, out_claims, out_evals);
}

int gkr_sumcheck_product_verify(gkr_ctx* ctx, const gkr_fr* tables, int n, int degree, const gkr_fr* claim, const gkr_fr* coeffs,
                                const uint32_t* len, const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !tables || !coeffs || !len || !r || !accept) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, 1)) return GKR_ERR_INVALID;
    const size_t count = (size_t)degree << n;
    if (!all_canonical(tables, count)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    {
        const hipError_t e = d.alloc(count);
        if (e != hipSuccess) return alloc_status(ctx, e, "gkr_sumcheck_product_verify: the tables");
    }
    HIP_TRY(ctx, hipMemcpyAsync(d.p, tables, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return verify_batch(ctx, d.p, n, product_terms(degree), 1, claim, coeffs, len, r, accept, failed_round, failed_check, nullptr, nullptr);
}

// ---- the sum-of-products sumcheck's verifier: the same driver with the caller's terms; it refuses what the prover refuses
// (sop_shape, sop_coeffs: capi_sop.hip)

int gkr_sumcheck_sop_verify_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int n_tables, const gkr_sop_term* terms,
                                         const gkr_fr* term_coeffs, int n_terms, int batch, const gkr_fr* claims, const gkr_fr* coeffs,
                                         const uint32_t* len, const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check,
                                         gkr_fr* out_claims, gkr_fr* out_evals) {
    if (!ctx || !d_tables || !terms || !coeffs || !len || !r || !accept) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!sop_shape(n, n_tables, terms, n_terms, batch, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    GKR_ENTER(ctx);
    return verify_batch(ctx, static_cast<const Fr*>(d_tables), n, sop_terms(ts, cf), batch, claims, coeffs, len, r, accept, failed_round,
                        failed_check, out_claims, out_evals);
}

int gkr_sumcheck_sop_verify(gkr_ctx* ctx, const gkr_fr* tables, int n, int n_tables, const gkr_sop_term* terms, const gkr_fr* term_coeffs,
                            int n_terms, const gkr_fr* claim, const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, int* accept,
                            uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !tables || !terms || !coeffs || !len || !r || !accept) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!sop_shape(n, n_tables, terms, n_terms, 1, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    const size_t count = (size_t)n_tables << n;
    if (!all_canonical(tables, count)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    {
        const hipError_t e = d.alloc(count);
        if (e != hipSuccess) return alloc_status(ctx, e, "gkr_sumcheck_sop_verify: the tables");
    }
    HIP_TRY(ctx, hipMemcpyAsync(d.p, tables, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return verify_batch(ctx, d.p, n, sop_terms(ts, cf), 1, claim, coeffs, len, r, accept, failed_round, failed_check, nullptr, nullptr);
}

}  // extern "C"

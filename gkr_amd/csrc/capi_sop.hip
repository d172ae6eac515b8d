// The sumcheck over a sum of products of resident multilinear tables, g = sum_k c_k prod_j T_{t(k, j)}: prove_sumcheck
// (rust/src/gkr/sumcheck.rs:158-214) on add_poly over k of c_k mult_poly(the tables' extensions).  One pass launch (every table
// folded once, every term's values) and one round launch (coefficients, length rule, hash) per round (kernels_sop.hip), in both
// transcript modes.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

static_assert(gkr::kSopMaxTables == GKR_SOP_MAX_TABLES && gkr::kSopMaxTerms == GKR_SOP_MAX_TERMS, "the kernels' term structure holds the header's limits");
static_assert(sizeof(gkr_sop_term) == 4, "a term is four bytes");

namespace gkr_host {

// Workspace slots are this path's own ("sop.*"): a call may follow or precede a plain or a product sumcheck on the same context.
static int run_sop_batch(gkr_ctx* ctx, const Fr* d_tables, int n, const gkr::SopTerms& ts, const gkr::SopCoeffs& cf, int batch,
                         gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    const size_t len = (size_t)1 << n, rounds = (size_t)batch * n, tables = (size_t)batch * ts.n_tables, slots = (size_t)ts.max_degree + 1;
    hipStream_t s = ctx->stream;
    Fr *work = nullptr, *d_coeffs = nullptr, *d_r = nullptr, *d_evals = nullptr;
    uint32_t* d_len = nullptr;
    gkr::FixedMul* d_rtab = nullptr;
    gkr::ProductPartial* partials = nullptr;
    const uint32_t max_nblk = product_round_blocks(n, batch, 0);
    WS(ctx, "sop.work", Fr, tables * (len / 2), work);
    WS(ctx, "sop.partials", gkr::ProductPartial, (size_t)batch * max_nblk * ts.n_terms, partials);
    WS(ctx, "sop.coeffs", Fr, rounds * slots, d_coeffs);
    WS(ctx, "sop.r", Fr, rounds, d_r);
    WS(ctx, "sop.rtab", gkr::FixedMul, rounds, d_rtab);
    WS(ctx, "sop.len", uint32_t, rounds, d_len);
    WS(ctx, "sop.evals", Fr, tables, d_evals);
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(len >> (round + 1));   // round 1: half a table; later: a quarter of the source table
        const uint32_t nblk = product_round_blocks(n, batch, round);
        if (round == 0) {   // round 1: values only
            Timed t(ctx, "sop_first", (double)tables * len * 32.0);
            gkr::launch_sop_first(ts, d_tables, len, items, (uint32_t)batch, nblk, partials, s);
        } else {   // rounds 2..n: every table folded once with r_{j-1}, every term's values of the folded tables in the same pass
            Timed t(ctx, "sop_fold_sum", (double)tables * 6.0 * items * 32.0);
            gkr::launch_sop_fold_sum(ts, round == 1 ? d_tables : work, round == 1 ? len : len / 2, work, len / 2, items, (uint32_t)batch, nblk,
                                     d_rtab + (round - 1), (uint32_t)n, partials, s);
        }
        Timed t(ctx, "sop_round", 0.0);
        gkr::launch_sop_round(ts, cf, partials, nblk, (uint32_t)round, (uint32_t)n, (uint32_t)batch, ctx->d_cts, work, len / 2, d_coeffs, d_len,
                              d_r, d_rtab, d_evals, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_coeffs, d_coeffs, rounds * slots * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, rounds * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_r, d_r, rounds * sizeof(Fr), hipMemcpyDeviceToHost, s));
    if (out_evals) HIP_TRY(ctx, hipMemcpyAsync(out_evals, d_evals, tables * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->drain_events();
    return GKR_OK;
}

// The shape checks of the prover's and the verifier's (capi_mle_verify.hip) entry points (plain returns: decided before the
// context is looked at), and the term structure in the kernels' form.  false: GKR_ERR_INVALID.
bool sop_shape(int n, int n_tables, const gkr_sop_term* terms, int n_terms, int batch, gkr::SopTerms* ts) {
    if (batch < 1 || batch > 65535) return false;
    if (n < 2 || n > GKR_MAX_MLE_N) return false;
    if (n_tables < 1 || n_tables > GKR_SOP_MAX_TABLES || n_terms < 1 || n_terms > GKR_SOP_MAX_TERMS) return false;
    uint32_t used = 0, max_degree = 0;
    for (int k = 0; k < n_terms; ++k) {
        const uint32_t d = terms[k].degree;
        if (d < 1 || d > GKR_PRODUCT_MAX_DEGREE) return false;
        uint32_t packed = d;
        for (uint32_t j = 0; j < d; ++j) {
            if (terms[k].table[j] >= n_tables) return false;
            used |= 1u << terms[k].table[j];
            packed |= (uint32_t)terms[k].table[j] << (8 + 8 * j);
        }
        ts->term[k] = packed;
        max_degree = std::max(max_degree, d);
    }
    if (used != (1u << n_tables) - 1u) return false;   // a table no term references
    if ((((unsigned long long)batch * (unsigned long long)n_tables) << n) > (1ull << 30)) return false;   // batch * n_tables * 2^n values
    for (int k = n_terms; k < gkr::kSopMaxTerms; ++k) ts->term[k] = 0;
    ts->n_tables = (uint32_t)n_tables;
    ts->n_terms = (uint32_t)n_terms;
    ts->max_degree = max_degree;
    return true;
}

// the coefficients in the kernels' form (NULL: all one); false: one is >= r
bool sop_coeffs(const gkr_fr* term_coeffs, int n_terms, gkr::SopCoeffs* cf) {
    memset(cf, 0, sizeof *cf);
    for (int k = 0; k < n_terms; ++k) {
        if (term_coeffs)
            cf->c[k] = to_dev(term_coeffs[k]);
        else
            cf->c[k].l[0] = 1;
        if (!gkr::fr_is_canonical(cf->c[k])) return false;
    }
    return true;
}

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

int gkr_sumcheck_sop_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int n_tables, const gkr_sop_term* terms,
                                  const gkr_fr* term_coeffs, int n_terms, int batch, gkr_fr* out_coeffs, uint32_t* out_len,
                                  gkr_fr* out_r, gkr_fr* out_evals) {
    if (!ctx || !d_tables || !terms || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!sop_shape(n, n_tables, terms, n_terms, batch, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    GKR_ENTER(ctx);
    return run_sop_batch(ctx, static_cast<const Fr*>(d_tables), n, ts, cf, batch, out_coeffs, out_len, out_r, out_evals);
}

int gkr_sumcheck_sop(gkr_ctx* ctx, const gkr_fr* tables, int n, int n_tables, const gkr_sop_term* terms, const gkr_fr* term_coeffs,
                     int n_terms, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    if (!ctx || !tables || !terms || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!sop_shape(n, n_tables, terms, n_terms, 1, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    const size_t count = (size_t)n_tables << n;
    if (!all_canonical(tables, count)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    HIP_TRY(ctx, d.alloc(count));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, tables, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return run_sop_batch(ctx, d.p, n, ts, cf, 1, out_coeffs, out_len, out_r, out_evals);
}

}  // extern "C"

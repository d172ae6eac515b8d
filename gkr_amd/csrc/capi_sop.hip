// The sumcheck over a sum of products of resident multilinear tables, g = sum_k c_k prod_j T_{t(k, j)}: prove_sumcheck
// (rust/src/gkr/sumcheck.rs:158-214) on add_poly over k of c_k mult_poly(the tables' extensions).  One pass launch (every table
// folded once, every term's values) and one round launch (coefficients, length rule, hash) per round (kernels_sop.hip), in both
// transcript modes: the entry points and the shape checks; the driver, run_sop_batch, is capi_resident.hip's.  C ABI:
// include/gkr_amd.h.
#include "capi_internal.h"

static_assert(gkr::kSopMaxTables == GKR_SOP_MAX_TABLES && gkr::kSopMaxTerms == GKR_SOP_MAX_TERMS, "the kernels' term structure holds the header's limits");
static_assert(sizeof(gkr_sop_term) == 4, "a term is four bytes");

namespace gkr_host {

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
    return run_on_tables(ctx, tables, (size_t)n_tables << n,
                         [&](const Fr* d) { return run_sop_batch(ctx, d, n, ts, cf, 1, out_coeffs, out_len, out_r, out_evals); });
}

}  // extern "C"

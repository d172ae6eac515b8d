// The zero-check sumcheck, sum_x eq(z, x) g(x) with g = sum_k c_k prod_j T_{t(k, j)} of term degrees 1 and 2: the transcript of
// the sum-of-products path (capi_sop.hip) on the tables {eq(z, .), T_0 ..} with every term prefixed by the eq table, without
// that table.  The eq factor is a scalar for the bound variables, a linear factor for the round's own and a split weight table of
// 2^(n-8) + 511 entries per sumcheck for the free ones (kernels_zerocheck.hip).  Here: the entry points and the shape check; the
// driver, run_zerocheck_batch, is capi_resident.hip's.  Also gkr_eq_table_device, the eq-table builder for callers of the SOP
// prover and verifier.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// the SOP prover's shape checks, and no term above degree 2 (rows of D + 1 = 4 slots hold inner degree 2)
static bool zerocheck_shape(int n, int n_tables, const gkr_sop_term* terms, int n_terms, int batch, gkr::SopTerms* ts) {
    return sop_shape(n, n_tables, terms, n_terms, batch, ts) && ts->max_degree <= 2;
}

// gkr_eq_table_device with a stride: tables below this size are built densely in a staging buffer of this many elements (32 MiB)
// and copied to their rows; larger ones are written in place, one launch each
constexpr size_t kEqStageElements = (size_t)1 << 20;

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

int gkr_sumcheck_zerocheck_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int n_tables, const gkr_sop_term* terms,
                                        const gkr_fr* term_coeffs, int n_terms, int batch, const gkr_fr* z, gkr_fr* out_coeffs,
                                        uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq) {
    if (!ctx || !d_tables || !terms || !z || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!zerocheck_shape(n, n_tables, terms, n_terms, batch, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    if (!all_canonical(z, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    return run_zerocheck_batch(ctx, static_cast<const Fr*>(d_tables), n, ts, cf, batch, z, out_coeffs, out_len, out_r, out_evals, out_eq);
}

int gkr_sumcheck_zerocheck(gkr_ctx* ctx, const gkr_fr* tables, int n, int n_tables, const gkr_sop_term* terms, const gkr_fr* term_coeffs,
                           int n_terms, const gkr_fr* z, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals,
                           gkr_fr* out_eq) {
    if (!ctx || !tables || !terms || !z || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!zerocheck_shape(n, n_tables, terms, n_terms, 1, &ts)) return GKR_ERR_INVALID;
    if (!sop_coeffs(term_coeffs, n_terms, &cf)) return ctx->fail(GKR_ERR_NON_CANONICAL, "term coefficient >= r");
    if (!all_canonical(z, (size_t)n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    return run_on_tables(ctx, tables, (size_t)n_tables << n, [&](const Fr* d) {
        return run_zerocheck_batch(ctx, d, n, ts, cf, 1, z, out_coeffs, out_len, out_r, out_evals, out_eq);
    });
}

int gkr_eq_table_device(gkr_ctx* ctx, const gkr_fr* z, int n, int batch, void* d_out, size_t stride_elements) {
    if (!ctx || !z || !d_out) return GKR_ERR_INVALID;
    if (n < 1 || n > GKR_MAX_MLE_N || batch < 1 || batch > 65535) return GKR_ERR_INVALID;
    const size_t len = (size_t)1 << n;
    if (stride_elements < len) return GKR_ERR_INVALID;
    if (!all_canonical(z, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    Fr *d_z = nullptr, *out = static_cast<Fr*>(d_out);
    WS(ctx, "zc.points", Fr, (size_t)batch * n, d_z);
    HIP_TRY(ctx, hipMemcpyAsync(d_z, z, (size_t)batch * n * sizeof(Fr), hipMemcpyHostToDevice, s));
    if (stride_elements == len) {   // the tables lie one after the other: launch_eq_table's own layout
        gkr::launch_eq_table(d_z, (uint32_t)n, 0u, (uint32_t)n, out, false, (uint32_t)batch, s);
    } else if (len >= kEqStageElements) {   // large tables: one launch each, in place
        for (int b = 0; b < batch; ++b)
            gkr::launch_eq_table(d_z + (size_t)b * n, (uint32_t)n, 0u, (uint32_t)n, out + (size_t)b * stride_elements, false, 1u, s);
    } else {   // small tables: built densely, a chunk of sumchecks at a time, and copied to their rows
        const size_t per = std::min<size_t>((size_t)batch, kEqStageElements >> n);
        Fr* stage = nullptr;
        WS(ctx, "zc.eq_stage", Fr, per << n, stage);
        for (size_t b0 = 0; b0 < (size_t)batch; b0 += per) {
            const size_t c = std::min(per, (size_t)batch - b0);
            gkr::launch_eq_table(d_z + b0 * n, (uint32_t)n, 0u, (uint32_t)n, stage, false, (uint32_t)c, s);
            gkr::launch_copy_rows(stage, len * 8, out + b0 * stride_elements, stride_elements * 8, (uint32_t)(len * 8), (uint32_t)c, s);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return GKR_OK;
}

}  // extern "C"

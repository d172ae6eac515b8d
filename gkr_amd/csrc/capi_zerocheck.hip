// The zero-check sumcheck, sum_x eq(z, x) g(x) with g = sum_k c_k prod_j T_{t(k, j)} of term degrees 1 and 2: the transcript of
// the sum-of-products path (capi_sop.hip) on the tables {eq(z, .), T_0 ..} with every term prefixed by the eq table, without
// that table.  The eq factor is a scalar for the bound variables, a linear factor for the round's own and a split weight table of
// 2^(n-8) + 511 entries per sumcheck for the free ones (kernels_zerocheck.hip).  Also gkr_eq_table_device, the eq-table builder
// for callers of the SOP prover and verifier.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// Workspace slots are this path's own ("zc.*"): a call may follow or precede a plain, a product or an SOP sumcheck on the same context.
// (Also the second half of the R1CS zero-check, capi_r1cs.hip.)
int run_zerocheck_batch(gkr_ctx* ctx, const Fr* d_tables, int n, const gkr::SopTerms& ts, const gkr::SopCoeffs& cf, int batch,
                        const gkr_fr* z, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq) {
    const size_t len = (size_t)1 << n, rounds = (size_t)batch * n, tables = (size_t)batch * ts.n_tables, slots = (size_t)ts.max_degree + 2;
    hipStream_t s = ctx->stream;
    Fr *work = nullptr, *d_coeffs = nullptr, *d_r = nullptr, *d_evals = nullptr, *d_z = nullptr, *d_s = nullptr, *d_eq = nullptr, *d_w = nullptr;
    uint32_t* d_len = nullptr;
    gkr::FixedMul* d_rtab = nullptr;
    gkr::ProductPartial* partials = nullptr;
    const uint32_t max_nblk = product_round_blocks(n, batch, 0);
    WS(ctx, "zc.work", Fr, tables * (len / 2), work);
    WS(ctx, "zc.partials", gkr::ProductPartial, (size_t)batch * max_nblk * ts.n_terms, partials);
    WS(ctx, "zc.coeffs", Fr, rounds * slots, d_coeffs);
    WS(ctx, "zc.r", Fr, rounds, d_r);
    WS(ctx, "zc.rtab", gkr::FixedMul, rounds, d_rtab);
    WS(ctx, "zc.len", uint32_t, rounds, d_len);
    WS(ctx, "zc.evals", Fr, tables, d_evals);
    WS(ctx, "zc.points", Fr, rounds, d_z);
    WS(ctx, "zc.s", Fr, batch, d_s);
    WS(ctx, "zc.eq", Fr, batch, d_eq);
    WS(ctx, "zc.weights", Fr, gkr::zc_weight_elements((uint32_t)n, (uint32_t)batch), d_w);
    const gkr::ZcWeights w = gkr::zc_weights_layout(d_w, (uint32_t)n, (uint32_t)batch);
    HIP_TRY(ctx, hipMemcpyAsync(d_z, z, rounds * sizeof(Fr), hipMemcpyHostToDevice, s));
    {
        Timed t(ctx, "zc_weights", 0.0, nullptr, true);
        gkr::launch_zc_weights(d_z, (uint32_t)n, (uint32_t)batch, w, s);
    }
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(len >> (round + 1));   // round 1: half a table; later: a quarter of the source table
        const uint32_t nblk = product_round_blocks(n, batch, round);
        const uint32_t free_vars = (uint32_t)(n - 1 - round), kl = free_vars < 8u ? free_vars : 8u, kh = free_vars - kl;
        if (round == 0) {   // round 1: weighted values only
            Timed t(ctx, "zc_first", (double)tables * len * 32.0);
            gkr::launch_zc_first(ts, d_tables, len, items, (uint32_t)batch, nblk, w, kh, kl, partials, s);
        } else {   // rounds 2..n: every table folded once with r_{j-1}, every term's weighted values of the folded tables in the same pass
            Timed t(ctx, "zc_fold_sum", (double)tables * 6.0 * items * 32.0);
            gkr::launch_zc_fold_sum(ts, round == 1 ? d_tables : work, round == 1 ? len : len / 2, work, len / 2, items, (uint32_t)batch, nblk,
                                    d_rtab + (round - 1), (uint32_t)n, w, kh, kl, partials, s);
        }
        Timed t(ctx, "zc_round", 0.0);
        gkr::launch_zc_round(ts, cf, partials, nblk, (uint32_t)round, (uint32_t)n, (uint32_t)batch, ctx->d_cts, d_z, d_s, work, len / 2, d_coeffs,
                             d_len, d_r, d_rtab, d_evals, d_eq, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_coeffs, d_coeffs, rounds * slots * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, rounds * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_r, d_r, rounds * sizeof(Fr), hipMemcpyDeviceToHost, s));
    if (out_evals) HIP_TRY(ctx, hipMemcpyAsync(out_evals, d_evals, tables * sizeof(Fr), hipMemcpyDeviceToHost, s));
    if (out_eq) HIP_TRY(ctx, hipMemcpyAsync(out_eq, d_eq, (size_t)batch * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->drain_events();
    return GKR_OK;
}

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
    const size_t count = (size_t)n_tables << n;
    if (!all_canonical(tables, count)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    HIP_TRY(ctx, d.alloc(count));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, tables, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return run_zerocheck_batch(ctx, d.p, n, ts, cf, 1, z, out_coeffs, out_len, out_r, out_evals, out_eq);
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

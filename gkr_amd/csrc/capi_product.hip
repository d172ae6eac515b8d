// The sumcheck over a product of resident multilinear tables (degree 1 .. GKR_PRODUCT_MAX_DEGREE): prove_sumcheck
// (rust/src/gkr/sumcheck.rs:158-214) on g = mult_poly of the tables' extensions.  One fused pass per round over all factors
// (kernels_product.hip) and the round's hash on the device, in both transcript modes.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

static_assert(gkr::kProductMaxDegree == GKR_PRODUCT_MAX_DEGREE, "the kernels' templates cover the header's degrees");

namespace gkr_host {

// Blocks per sumcheck of round `round` (0-based): mle_blocks_per_table of the round's items (round 1: half a table; later: a quarter
// of the source table), never more than round 1's count, which sizes the partials.  Host logic only; gkr_selftest_product_geometry
// reports it.
uint32_t product_round_blocks(int n, int batch, int round) {
    const size_t len = (size_t)1 << n;
    const uint32_t max_nblk = gkr::mle_blocks_per_table((uint32_t)(len / 2), (uint32_t)batch);   // (non-increasing in the items)
    const uint32_t items = (uint32_t)(len >> (round + 1));
    return std::min(gkr::mle_blocks_per_table(items, (uint32_t)batch), max_nblk);
}

// Workspace slots are this path's own ("product.*"): a call may follow a plain sumcheck on the same context.
int run_product_batch(gkr_ctx* ctx, const Fr* d_tables, int n, int degree, int batch, gkr_fr* out_coeffs, uint32_t* out_len,
                             gkr_fr* out_r, gkr_fr* out_evals) {
    const size_t len = (size_t)1 << n, rounds = (size_t)batch * n, tables = (size_t)batch * degree, slots = (size_t)degree + 1;
    hipStream_t s = ctx->stream;
    Fr *work = nullptr, *d_coeffs = nullptr, *d_r = nullptr, *d_evals = nullptr;
    uint32_t *d_len = nullptr, *d_meta = nullptr;
    gkr::FixedMul* d_rtab = nullptr;
    gkr::ProductPartial* partials = nullptr;
    const uint32_t max_nblk = product_round_blocks(n, batch, 0);
    WS(ctx, "product.work", Fr, tables * (len / 2), work);
    WS(ctx, "product.partials", gkr::ProductPartial, (size_t)batch * max_nblk, partials);
    WS(ctx, "product.coeffs", Fr, rounds * slots, d_coeffs);
    WS(ctx, "product.r", Fr, rounds, d_r);
    WS(ctx, "product.rtab", gkr::FixedMul, rounds, d_rtab);
    WS(ctx, "product.len", uint32_t, rounds, d_len);
    WS(ctx, "product.meta", uint32_t, batch, d_meta);
    WS(ctx, "product.evals", Fr, tables, d_evals);
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(len >> (round + 1));   // round 1: half a table; later: a quarter of the source table
        const uint32_t nblk = product_round_blocks(n, batch, round);
        if (round == 0) {   // round 1: values only
            Timed t(ctx, "product_first", (double)tables * len * 32.0);
            gkr::launch_product_first(degree, d_tables, len, items, (uint32_t)batch, nblk, partials, s);
        } else {   // rounds 2..n: fold every factor with r_{j-1}, the folded tables' values in the same pass
            Timed t(ctx, "product_fold_sum", (double)tables * 6.0 * items * 32.0);
            gkr::launch_product_fold_sum(degree, round == 1 ? d_tables : work, round == 1 ? len : len / 2, work, len / 2, items, (uint32_t)batch,
                                         nblk, d_rtab + (round - 1), (uint32_t)n, partials, s);
        }
        Timed t(ctx, "product_round", 0.0);
        gkr::launch_product_round(degree, partials, nblk, (uint32_t)round, (uint32_t)n, (uint32_t)batch, ctx->d_cts, work, len / 2, d_coeffs,
                                  d_len, d_r, d_rtab, d_meta, d_evals, s);
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

// The shape checks the prover's and the verifier's (capi_mle_verify.hip) entry points share, in gkr_sumcheck_mle_batch_device's
// order (ctx and pointers first, then n).  Plain returns, as gkr_mle_eval_batch_device's: they are decided before the context
// is looked at.
bool product_shape_ok(int n, int degree, int batch) {
    if (n < 2 || n > GKR_MAX_MLE_N) return false;                                       // n must be in [2, 30]
    if (degree < 1 || degree > GKR_PRODUCT_MAX_DEGREE) return false;                    // degree must be in [1, 3]
    return (((unsigned long long)batch * (unsigned long long)degree) << n) <= (1ull << 30);   // batch * degree * 2^n values
}

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

int gkr_sumcheck_product_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int degree, int batch, gkr_fr* out_coeffs,
                                      uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    if (!ctx || !d_tables || !out_coeffs || !out_len || !out_r || batch < 1 || batch > 65535) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return run_product_batch(ctx, static_cast<const Fr*>(d_tables), n, degree, batch, out_coeffs, out_len, out_r, out_evals);
}

int gkr_sumcheck_product(gkr_ctx* ctx, const gkr_fr* tables, int n, int degree, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                         gkr_fr* out_evals) {
    if (!ctx || !tables || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!product_shape_ok(n, degree, 1)) return GKR_ERR_INVALID;
    const size_t count = (size_t)degree << n;
    if (!all_canonical(tables, count)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    HIP_TRY(ctx, d.alloc(count));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, tables, count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return run_product_batch(ctx, d.p, n, degree, 1, out_coeffs, out_len, out_r, out_evals);
}

// the launch geometry of run_product_batch (host logic only, the process-default options): per round the blocks per sumcheck and
// the chunk the pass kernels derive from them.  batch * 1 table of 2^n values must be a shape the prover admits.
int gkr_selftest_product_geometry(int n, int batch, uint32_t* nblk, uint32_t* chunk) {
    if (!nblk || !chunk || batch < 1 || batch > 65535 || !product_shape_ok(n, 1, batch)) return GKR_ERR_INVALID;
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(((size_t)1 << n) >> (round + 1)), b = product_round_blocks(n, batch, round);
        nblk[round] = b;
        chunk[round] = ((items + b - 1) / b + 255u) & ~255u;
    }
    return GKR_OK;
}

}  // extern "C"

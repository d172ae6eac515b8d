// The LOOKUP argument (LogUp): every value of a resident witness column W lies in a resident table T, with multiplicities M, iff
//   sum_i 1 / (alpha - W[i]) - sum_j M[j] / (alpha - T[j]) = 0
// as a rational function of alpha -- the fractional sum (capi_fraction_sum.hip) of a pair (N, D) that this file builds on the
// device (kernels_lookup.hip): the multiplicities by a join through an open-addressing index of the table, then the pair in the
// fractional sum's input layout.  The proof IS gkr_fraction_sum_batch_device's proof of that pair and the verifier IS
// gkr_fraction_sum_verify_batch_device on the rebuilt pair -- both are called through their entry points, so the outputs are theirs
// byte for byte -- with one more check, GKR_VERIFY_LOOKUP: the head's P is 0 (lookup_rules.h).  The index, the counters, alpha and
// the pair live in context workspace under slot names of this path's own (lk.*).  C ABI: include/gkr_amd.h.
#include "capi_internal.h"
#include "lookup_rules.h"

namespace {

// the counters of `batch` columns into d_mult, the miss counters to the host: the whole of gkr_lookup_multiplicities_device behind
// its argument checks
int run_multiplicities(gkr_ctx* ctx, const Fr* d_witness, int n_w, const Fr* d_table, int n_t, bool shared, int batch, Fr* d_mult,
                       uint32_t* out_missing, uint32_t* out_first_missing) {
    hipStream_t s = ctx->stream;
    const size_t B = (size_t)batch, tables = shared ? 1 : B, slots = tables << (n_t + 1), entries = B << n_t;
    uint32_t *d_index = nullptr, *d_counts = nullptr, *d_miss = nullptr;
    WS(ctx, "lk.index", uint32_t, slots, d_index);
    WS(ctx, "lk.counts", uint32_t, entries, d_counts);
    WS(ctx, "lk.miss", uint32_t, 2 * B, d_miss);
    HIP_TRY(ctx, hipMemsetAsync(d_index, 0xFF, slots * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(d_counts, 0, entries * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(d_miss, 0, B * sizeof(uint32_t), s));
    HIP_TRY(ctx, hipMemsetAsync(d_miss + B, 0xFF, B * sizeof(uint32_t), s));
    {
        Timed t(ctx, "lk_build", (double)tables * 36.0 * (double)((size_t)1 << n_t));
        gkr::launch_lk_build(d_table, (uint32_t)n_t, (uint32_t)tables, d_index, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        Timed t(ctx, "lk_count", (double)B * 32.0 * (double)((size_t)1 << n_w));
        gkr::launch_lk_count(d_witness, (uint32_t)n_w, d_table, (uint32_t)n_t, shared, d_index, (uint32_t)batch, d_counts, d_miss, d_miss + B, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        Timed t(ctx, "lk_mult", (double)entries * 36.0);
        gkr::launch_lk_mult(d_counts, (uint32_t)n_t, (uint32_t)batch, d_mult, s);
        HIP_TRY(ctx, hipGetLastError());
    }
    std::vector<uint32_t> miss(2 * B);
    HIP_TRY(ctx, hipMemcpyAsync(miss.data(), d_miss, 2 * B * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->drain_events();
    memcpy(out_missing, miss.data(), B * sizeof(uint32_t));
    memcpy(out_first_missing, miss.data() + B, B * sizeof(uint32_t));
    return GKR_OK;
}

// the pairs of `batch` lookups into d_pair (queued on the context's stream)
int queue_pair(gkr_ctx* ctx, const Fr* d_witness, int n_w, const Fr* d_table, int n_t, bool shared, const Fr* d_mult, const gkr_fr* alpha, int batch,
               int L, Fr* d_pair) {
    if (!all_canonical(alpha, (size_t)batch)) return ctx->fail(GKR_ERR_NON_CANONICAL, "lookup: alpha >= r");
    Fr* d_alpha = nullptr;
    WS(ctx, "lk.alpha", Fr, batch, d_alpha);
    HIP_TRY(ctx, hipMemcpyAsync(d_alpha, alpha, (size_t)batch * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    // one read of W, T and M, one write of N and D
    Timed t(ctx, "lk_pair", (double)batch * 32.0 * ((double)((size_t)1 << n_w) + 2.0 * (double)((size_t)1 << n_t) + (double)((size_t)2 << L)));
    gkr::launch_lk_pair(d_witness, (uint32_t)n_w, d_table, (uint32_t)n_t, shared, d_mult, d_alpha, (uint32_t)L, (uint32_t)batch, d_pair, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

int workspace_pair(gkr_ctx* ctx, const void* d_witness, int n_w, const void* d_table, int n_t, int shared, const void* d_mult, const gkr_fr* alpha,
                   int batch, int L, Fr** d_pair) {
    WS(ctx, "lk.pair", Fr, (size_t)batch << (L + 1), *d_pair);
    return queue_pair(ctx, static_cast<const Fr*>(d_witness), n_w, static_cast<const Fr*>(d_table), n_t, shared != 0, static_cast<const Fr*>(d_mult), alpha,
                      batch, L, *d_pair);
}

}  // namespace

// =========================================================================== C ABI

extern "C" {

int gkr_lookup_multiplicities_device(gkr_ctx* ctx, const void* d_witness, int n_w, const void* d_table, int n_t, int shared_table, int batch,
                                     void* d_mult, uint32_t* out_missing, uint32_t* out_first_missing) {
    if (!ctx || !d_witness || !d_table || !d_mult || !out_missing || !out_first_missing) return GKR_ERR_INVALID;
    if (!gkr::lookup::pair_log2(n_w, n_t, batch)) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    return run_multiplicities(ctx, static_cast<const Fr*>(d_witness), n_w, static_cast<const Fr*>(d_table), n_t, shared_table != 0, batch,
                              static_cast<Fr*>(d_mult), out_missing, out_first_missing);
}

int gkr_lookup_batch_device(gkr_ctx* ctx, const void* d_witness, int n_w, const void* d_table, int n_t, int shared_table, const void* d_mult,
                            const gkr_fr* alpha, int batch, gkr_fr* out_sums, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                            gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    if (!ctx || !d_witness || !d_table || !d_mult || !alpha || !out_sums || !out_head || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    const int L = gkr::lookup::pair_log2(n_w, n_t, batch);
    if (!L) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    Fr* d_pair = nullptr;
    if (const int rc = workspace_pair(ctx, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, L, &d_pair)) return rc;
    return gkr_fraction_sum_batch_device(ctx, d_pair, L, batch, out_sums, out_head, out_coeffs, out_len, out_r, out_evals, out_point, out_claims);
}

int gkr_lookup_verify_batch_device(gkr_ctx* ctx, const void* d_witness, int n_w, const void* d_table, int n_t, int shared_table, const void* d_mult,
                                   const gkr_fr* alpha, int batch, const gkr_fr* head, const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r,
                                   const gkr_fr* evals, int* accept, uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check,
                                   gkr_fr* out_sums) {
    if (!ctx || !d_witness || !d_table || !d_mult || !alpha || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    const int L = gkr::lookup::pair_log2(n_w, n_t, batch);
    if (!L) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    Fr* d_pair = nullptr;
    if (const int rc = workspace_pair(ctx, d_witness, n_w, d_table, n_t, shared_table, d_mult, alpha, batch, L, &d_pair)) return rc;
    const size_t B = (size_t)batch;
    std::vector<gkr_fr> sums(2 * B);
    std::vector<uint32_t> layer(B), round(B), check(B);
    if (const int rc = gkr_fraction_sum_verify_batch_device(ctx, d_pair, L, batch, nullptr, head, coeffs, len, r, evals, accept, layer.data(), round.data(),
                                                            check.data(), sums.data()))
        return rc;
    for (size_t b = 0; b < B; ++b) {
        gkr::lookup::verdict(&sums[2 * b], &accept[b], &layer[b], &round[b], &check[b]);
        if (failed_layer) failed_layer[b] = layer[b];
        if (failed_round) failed_round[b] = round[b];
        if (failed_check) failed_check[b] = check[b];
    }
    if (out_sums) memcpy(out_sums, sums.data(), 2 * B * sizeof(gkr_fr));
    return GKR_OK;
}

int gkr_lookup(gkr_ctx* ctx, const gkr_fr* witness, int n_w, const gkr_fr* table, int n_t, const gkr_fr* alpha, gkr_fr* out_mult,
               uint32_t* out_missing, uint32_t* out_first_missing, gkr_fr* out_sum, gkr_fr* out_head, gkr_fr* out_coeffs, uint32_t* out_len,
               gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_point, gkr_fr* out_claims) {
    if (!ctx || !witness || !table || !alpha || !out_mult || !out_missing || !out_first_missing || !out_sum || !out_head || !out_coeffs || !out_len ||
        !out_r)
        return GKR_ERR_INVALID;
    if (!gkr::lookup::pair_log2(n_w, n_t, 1)) return GKR_ERR_INVALID;
    const size_t nw = (size_t)1 << n_w, nt = (size_t)1 << n_t;
    if (!all_canonical(witness, nw) || !all_canonical(table, nt)) return ctx->fail(GKR_ERR_NON_CANONICAL, "lookup: witness or table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;   // W, T, M
    HIP_TRY(ctx, d.alloc(nw + 2 * nt));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, witness, nw * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d.p + nw, table, nt * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    if (const int rc = run_multiplicities(ctx, d.p, n_w, d.p + nw, n_t, true, 1, d.p + nw + nt, out_missing, out_first_missing)) return rc;
    HIP_TRY(ctx, hipMemcpy(out_mult, d.p + nw + nt, nt * sizeof(Fr), hipMemcpyDeviceToHost));
    return gkr_lookup_batch_device(ctx, d.p, n_w, d.p + nw, n_t, 1, d.p + nw + nt, alpha, 1, out_sum, out_head, out_coeffs, out_len, out_r, out_evals,
                                   out_point, out_claims);
}

int gkr_lookup_verify(gkr_ctx* ctx, const gkr_fr* witness, int n_w, const gkr_fr* table, int n_t, const gkr_fr* mult, const gkr_fr* alpha,
                      const gkr_fr* head, const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r, const gkr_fr* evals, int* accept,
                      uint32_t* failed_layer, uint32_t* failed_round, uint32_t* failed_check) {
    if (!ctx || !witness || !table || !mult || !alpha || !head || !coeffs || !len || !r || !evals || !accept) return GKR_ERR_INVALID;
    if (!gkr::lookup::pair_log2(n_w, n_t, 1)) return GKR_ERR_INVALID;
    const size_t nw = (size_t)1 << n_w, nt = (size_t)1 << n_t;
    if (!all_canonical(witness, nw) || !all_canonical(table, nt) || !all_canonical(mult, nt))
        return ctx->fail(GKR_ERR_NON_CANONICAL, "lookup: witness, table or multiplicity >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    HIP_TRY(ctx, d.alloc(nw + 2 * nt));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, witness, nw * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d.p + nw, table, nt * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(d.p + nw + nt, mult, nt * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return gkr_lookup_verify_batch_device(ctx, d.p, n_w, d.p + nw, n_t, 1, d.p + nw + nt, alpha, 1, head, coeffs, len, r, evals, accept, failed_layer,
                                          failed_round, failed_check, nullptr);
}

int gkr_selftest_lookup_slot(const gkr_fr* v, int log_slots, uint32_t* slot) {
    if (!v || !slot || log_slots < 1 || log_slots > 32) return GKR_ERR_INVALID;
    uint32_t limbs[8];
    memcpy(limbs, v, 32);
    *slot = gkr::lookup::slot_of(limbs, (uint32_t)log_slots);
    return GKR_OK;
}

int gkr_devtest_lookup_pair(gkr_ctx* ctx, const void* d_witness, int n_w, const void* d_table, int n_t, int shared_table, const void* d_mult,
                            const gkr_fr* alpha, int batch, void* d_pair) {
    if (!ctx || !d_witness || !d_table || !d_mult || !alpha || !d_pair) return GKR_ERR_INVALID;
    const int L = gkr::lookup::pair_log2(n_w, n_t, batch);
    if (!L) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    if (const int rc = queue_pair(ctx, static_cast<const Fr*>(d_witness), n_w, static_cast<const Fr*>(d_table), n_t, shared_table != 0,
                                  static_cast<const Fr*>(d_mult), alpha, batch, L, static_cast<Fr*>(d_pair)))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

}  // extern "C"

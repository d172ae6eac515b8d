// THE driver of the sumchecks over resident multilinear tables -- a product (capi_product.hip), a sum of products (capi_sop.hip),
// the zero-check (capi_zerocheck.hip), a layer of the fractional sum (capi_fraction_sum.hip): the workspace, per round one pass
// launch (round 1: values only; later: fold and values) and one round launch, the read-backs.  A family describes itself in a small struct: its slot names and timing labels, its sizes,
// three launch hooks and what it reads back besides; run_product_batch, run_sop_batch, run_zerocheck_batch and run_fraction_layer_batch
// fill one in.
#include "capi_internal.h"

namespace gkr_host {

namespace {

// A family's workspace slots are its own: calls of different kinds on one context do not resize each other's buffers.
struct ResidentNames {
    const char *work, *partials, *coeffs, *r, *rtab, *len, *evals;   // workspace slots
    const char *first, *fold_sum, *round;                            // Timed labels
};

// what the driver hands the launch hooks: the call's shape and the buffers every family has
struct ResidentCall {
    gkr_ctx* ctx;
    hipStream_t s;
    uint32_t n, batch;
    size_t len;   // 2^n; the folded tables lie at strides of len / 2 in work
    Fr *work, *d_coeffs, *d_r, *d_evals;
    uint32_t* d_len;
    gkr::FixedMul* d_rtab;
    gkr::ProductPartial* partials;
};

// Family: names (static), n_tables per sumcheck, slots per output row, partials per block, and the hooks
//   first(call, tables, items, nblk)                       round 1's pass over the input tables
//   fold_sum(call, round, src, src_stride, items, nblk)    the pass of round `round` + 1 >= 2: src -> work, folded with r_round
//   round(call, round, nblk)                               the round kernel
//   read_back(call)                                        the family's own outputs, queued behind the shared ones
template <typename Family>
int run_resident_batch(gkr_ctx* ctx, const Family& fam, const Fr* d_tables, int n, int batch, gkr_fr* out_coeffs, uint32_t* out_len,
                       gkr_fr* out_r, gkr_fr* out_evals) {
    constexpr ResidentNames nm = Family::names;
    const size_t len = (size_t)1 << n, rounds = (size_t)batch * n, tables = (size_t)batch * fam.n_tables, slots = fam.slots;
    ResidentCall c{ctx, ctx->stream, (uint32_t)n, (uint32_t)batch, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const uint32_t max_nblk = product_round_blocks(n, batch, 0);
    WS(ctx, nm.work, Fr, tables * (len / 2), c.work);
    WS(ctx, nm.partials, gkr::ProductPartial, (size_t)batch * max_nblk * fam.partials_per_block, c.partials);
    WS(ctx, nm.coeffs, Fr, rounds * slots, c.d_coeffs);
    WS(ctx, nm.r, Fr, rounds, c.d_r);
    WS(ctx, nm.rtab, gkr::FixedMul, rounds, c.d_rtab);
    WS(ctx, nm.len, uint32_t, rounds, c.d_len);
    WS(ctx, nm.evals, Fr, tables, c.d_evals);
    for (int round = 0; round < n; ++round) {
        const uint32_t items = (uint32_t)(len >> (round + 1));   // round 1: half a table; later: a quarter of the source table
        const uint32_t nblk = product_round_blocks(n, batch, round);
        if (round == 0) {   // round 1: values only
            Timed t(ctx, nm.first, (double)tables * len * 32.0);
            fam.first(c, d_tables, items, nblk);
        } else {   // rounds 2..n: the tables folded with r_{j-1}, the folded tables' values in the same pass
            Timed t(ctx, nm.fold_sum, (double)tables * 6.0 * items * 32.0);
            fam.fold_sum(c, (uint32_t)round, round == 1 ? d_tables : c.work, round == 1 ? len : len / 2, items, nblk);
        }
        Timed t(ctx, nm.round, 0.0);
        fam.round(c, (uint32_t)round, nblk);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_coeffs, c.d_coeffs, rounds * slots * sizeof(Fr), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(ctx, hipMemcpyAsync(out_len, c.d_len, rounds * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(ctx, hipMemcpyAsync(out_r, c.d_r, rounds * sizeof(Fr), hipMemcpyDeviceToHost, c.s));
    if (out_evals) HIP_TRY(ctx, hipMemcpyAsync(out_evals, c.d_evals, tables * sizeof(Fr), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(ctx, fam.read_back(c));
    HIP_TRY(ctx, hipStreamSynchronize(c.s));
    ctx->drain_events();
    return GKR_OK;
}

// one fused pass per round over all `degree` factors; meta: the round kernel's own words (kernels_product.hip)
struct ProductFamily {
    static constexpr ResidentNames names = {"product.work", "product.partials", "product.coeffs", "product.r", "product.rtab", "product.len",
                                            "product.evals", "product_first", "product_fold_sum", "product_round"};
    int degree;
    uint32_t n_tables, slots, partials_per_block;
    uint32_t* d_meta;
    void first(const ResidentCall& c, const Fr* tables, uint32_t items, uint32_t nblk) const {
        gkr::launch_product_first(degree, tables, c.len, items, c.batch, nblk, c.partials, c.s);
    }
    void fold_sum(const ResidentCall& c, uint32_t round, const Fr* src, size_t src_stride, uint32_t items, uint32_t nblk) const {
        gkr::launch_product_fold_sum(degree, src, src_stride, c.work, c.len / 2, items, c.batch, nblk, c.d_rtab + (round - 1), c.n, c.partials, c.s);
    }
    void round(const ResidentCall& c, uint32_t round, uint32_t nblk) const {
        gkr::launch_product_round(degree, c.partials, nblk, round, c.n, c.batch, c.ctx->d_cts, c.work, c.len / 2, c.d_coeffs, c.d_len, c.d_r,
                                  c.d_rtab, d_meta, c.d_evals, c.s);
    }
    hipError_t read_back(const ResidentCall&) const { return hipSuccess; }
};

// every table folded once per round, every term's values of the folded tables in the same pass (kernels_sop.hip)
struct SopFamily {
    static constexpr ResidentNames names = {"sop.work", "sop.partials", "sop.coeffs", "sop.r", "sop.rtab", "sop.len", "sop.evals",
                                            "sop_first", "sop_fold_sum", "sop_round"};
    const gkr::SopTerms& ts;
    const gkr::SopCoeffs& cf;
    uint32_t n_tables, slots, partials_per_block;
    void first(const ResidentCall& c, const Fr* tables, uint32_t items, uint32_t nblk) const {
        gkr::launch_sop_first(ts, tables, c.len, items, c.batch, nblk, c.partials, c.s);
    }
    void fold_sum(const ResidentCall& c, uint32_t round, const Fr* src, size_t src_stride, uint32_t items, uint32_t nblk) const {
        gkr::launch_sop_fold_sum(ts, src, src_stride, c.work, c.len / 2, items, c.batch, nblk, c.d_rtab + (round - 1), c.n, c.partials, c.s);
    }
    void round(const ResidentCall& c, uint32_t round, uint32_t nblk) const {
        gkr::launch_sop_round(ts, cf, c.partials, nblk, round, c.n, c.batch, c.ctx->d_cts, c.work, c.len / 2, c.d_coeffs, c.d_len, c.d_r, c.d_rtab,
                              c.d_evals, c.s);
    }
    hipError_t read_back(const ResidentCall&) const { return hipSuccess; }
};

// the SOP family's passes with the weights of the variables still free (kernels_zerocheck.hip): shared by the zero-check and the
// fractional sum's layers
struct ZcPasses {
    const gkr::SopTerms& ts;
    gkr::ZcWeights w;
    // round `round` has n - 1 - round free variables: the last kl <= 8 of them weigh per thread, the kh in front per iteration
    static uint32_t lo_vars(const ResidentCall& c, uint32_t round) { return std::min(c.n - 1u - round, 8u); }
    void first(const ResidentCall& c, const Fr* tables, uint32_t items, uint32_t nblk) const {
        const uint32_t kl = lo_vars(c, 0);
        gkr::launch_zc_first(ts, tables, c.len, items, c.batch, nblk, w, c.n - 1u - kl, kl, c.partials, c.s);
    }
    void fold_sum(const ResidentCall& c, uint32_t round, const Fr* src, size_t src_stride, uint32_t items, uint32_t nblk) const {
        const uint32_t kl = lo_vars(c, round);
        gkr::launch_zc_fold_sum(ts, src, src_stride, c.work, c.len / 2, items, c.batch, nblk, c.d_rtab + (round - 1), c.n, w, c.n - 1u - round - kl,
                                kl, c.partials, c.s);
    }
};

// those passes, the round with the points and the bound variables' scalar; rows have one slot more: the eq factor's degree
struct ZerocheckFamily : ZcPasses {
    static constexpr ResidentNames names = {"zc.work", "zc.partials", "zc.coeffs", "zc.r", "zc.rtab", "zc.len", "zc.evals",
                                            "zc_first", "zc_fold_sum", "zc_round"};
    const gkr::SopCoeffs& cf;
    uint32_t n_tables, slots, partials_per_block;
    Fr *d_z, *d_s, *d_eq;
    gkr_fr* out_eq;
    void round(const ResidentCall& c, uint32_t round, uint32_t nblk) const {
        gkr::launch_zc_round(ts, cf, c.partials, nblk, round, c.n, c.batch, c.ctx->d_cts, d_z, d_s, c.work, c.len / 2, c.d_coeffs, c.d_len, c.d_r,
                             c.d_rtab, c.d_evals, d_eq, c.s);
    }
    hipError_t read_back(const ResidentCall& c) const {
        return out_eq ? hipMemcpyAsync(out_eq, d_eq, (size_t)c.batch * sizeof(Fr), hipMemcpyDeviceToHost, c.s) : hipSuccess;
    }
};

// a layer of the fractional sum (kernels_fraction_sum.hip): the zero-check's passes over the layer's three terms, its round with
// the third term's coefficient per sumcheck; slots of its own, so that neither resizes the other's buffers
struct FractionFamily : ZcPasses {
    static constexpr ResidentNames names = {"fs.work", "fs.partials", "fs.coeffs", "fs.r", "fs.rtab", "fs.len", "fs.evals",
                                            "fs_first", "fs_fold_sum", "fs_round"};
    uint32_t n_tables, slots, partials_per_block;
    Fr *d_z, *d_lambda, *d_s, *d_eq;
    gkr_fr* out_eq;
    void round(const ResidentCall& c, uint32_t round, uint32_t nblk) const {
        gkr::launch_fs_round(c.partials, nblk, round, c.n, c.batch, d_lambda, c.ctx->d_cts, d_z, d_s, c.work, c.len / 2, c.d_coeffs, c.d_len, c.d_r,
                             c.d_rtab, c.d_evals, d_eq, c.s);
    }
    hipError_t read_back(const ResidentCall& c) const {
        return out_eq ? hipMemcpyAsync(out_eq, d_eq, (size_t)c.batch * sizeof(Fr), hipMemcpyDeviceToHost, c.s) : hipSuccess;
    }
};

}  // namespace

int run_product_batch(gkr_ctx* ctx, const Fr* d_tables, int n, int degree, int batch, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                      gkr_fr* out_evals) {
    ProductFamily fam{degree, (uint32_t)degree, (uint32_t)degree + 1u, 1u, nullptr};
    WS(ctx, "product.meta", uint32_t, batch, fam.d_meta);
    return run_resident_batch(ctx, fam, d_tables, n, batch, out_coeffs, out_len, out_r, out_evals);
}

int run_sop_batch(gkr_ctx* ctx, const Fr* d_tables, int n, const gkr::SopTerms& ts, const gkr::SopCoeffs& cf, int batch, gkr_fr* out_coeffs,
                  uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    const SopFamily fam{ts, cf, ts.n_tables, ts.max_degree + 1u, ts.n_terms};
    return run_resident_batch(ctx, fam, d_tables, n, batch, out_coeffs, out_len, out_r, out_evals);
}

int run_zerocheck_batch(gkr_ctx* ctx, const Fr* d_tables, int n, const gkr::SopTerms& ts, const gkr::SopCoeffs& cf, int batch,
                        const gkr_fr* z, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq) {
    ZerocheckFamily fam{{ts, {}}, cf, ts.n_tables, ts.max_degree + 2u, ts.n_terms, nullptr, nullptr, nullptr, out_eq};
    Fr* d_w = nullptr;
    WS(ctx, "zc.points", Fr, (size_t)batch * n, fam.d_z);
    WS(ctx, "zc.s", Fr, batch, fam.d_s);
    WS(ctx, "zc.eq", Fr, batch, fam.d_eq);
    WS(ctx, "zc.weights", Fr, gkr::zc_weight_elements((uint32_t)n, (uint32_t)batch), d_w);
    fam.w = gkr::zc_weights_layout(d_w, (uint32_t)n, (uint32_t)batch);
    HIP_TRY(ctx, hipMemcpyAsync(fam.d_z, z, (size_t)batch * n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    {
        Timed t(ctx, "zc_weights", 0.0, nullptr, true);
        gkr::launch_zc_weights(fam.d_z, (uint32_t)n, (uint32_t)batch, fam.w, ctx->stream);
    }
    return run_resident_batch(ctx, fam, d_tables, n, batch, out_coeffs, out_len, out_r, out_evals);
}

int run_fraction_layer_batch(gkr_ctx* ctx, const Fr* d_tables, int k, int batch, const gkr_fr* z, const gkr_fr* lambda, gkr_fr* out_coeffs,
                             uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq) {
    // T0 T3 + T1 T2 + lambda T2 T3: the structure the passes read; the coefficients are the round kernel's own
    static const gkr::SopTerms ts = {4u, 3u, 2u, {2u | 0u << 8 | 3u << 16, 2u | 1u << 8 | 2u << 16, 2u | 2u << 8 | 3u << 16}};
    FractionFamily fam{{ts, {}}, ts.n_tables, ts.max_degree + 2u, ts.n_terms, nullptr, nullptr, nullptr, nullptr, out_eq};
    Fr* d_w = nullptr;
    WS(ctx, "fs.points", Fr, (size_t)batch * (k + 1), fam.d_z);   // the points, then the lambdas
    WS(ctx, "fs.s", Fr, batch, fam.d_s);
    WS(ctx, "fs.eq", Fr, batch, fam.d_eq);
    WS(ctx, "fs.weights", Fr, gkr::zc_weight_elements((uint32_t)k, (uint32_t)batch), d_w);
    fam.d_lambda = fam.d_z + (size_t)batch * k;
    fam.w = gkr::zc_weights_layout(d_w, (uint32_t)k, (uint32_t)batch);
    HIP_TRY(ctx, hipMemcpyAsync(fam.d_z, z, (size_t)batch * k * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(fam.d_lambda, lambda, (size_t)batch * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    {
        Timed t(ctx, "fs_weights", 0.0, nullptr, true);
        gkr::launch_zc_weights(fam.d_z, (uint32_t)k, (uint32_t)batch, fam.w, ctx->stream);
    }
    return run_resident_batch(ctx, fam, d_tables, k, batch, out_coeffs, out_len, out_r, out_evals);
}

}  // namespace gkr_host

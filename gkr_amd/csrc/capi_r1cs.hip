// The R1CS zero-check: the CSR form of an R1CS (r1cs.cpp) resident on a context's device, the tables Az, Bz, Cz of a batch of
// resident witnesses (kernels_r1cs.hip), the row check a * b == c, and the zero-check eq(z, .) (A B - C) on those tables
// (run_zerocheck_batch, capi_resident.hip).  And the inner sumcheck that reduces the zero-check's three claims to the witness: the
// column-major form resident, the table T(y) = sum_m rho_m sum_i M_m[i][y] eq(x, i), the product path at degree 2 on (T, w)
// (run_product_batch, capi_resident.hip).  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

static_assert(sizeof(gkr_r1cs_term) == sizeof(uint2), "a record is eight bytes: {wire, pool index}");
static_assert(gkr::kR1csLongRow == GKR_R1CS_LONG_ROW, "the kernels and the host's long-row lists cut at the same length");

// (struct gkr_r1cs_rows, the CSR form resident: capi_internal.h -- the verifier's translation unit reads it too)

static_assert(gkr::kR1csLongCol == GKR_R1CS_LONG_COL, "the kernels and the host's long-column lists cut at the same length");
static_assert(gkr::kR1csColSegment == GKR_R1CS_COL_SEGMENT, "the header names the kernels' segment length");

// The column-major form (r1cs.cpp) resident on a context's device, for the inner sumcheck's table (kernels_r1cs.hip).
struct gkr_r1cs_cols {
    gkr_ctx* ctx = nullptr;
    gkr_r1cs_csc_info_t info{};
    uint32_t* col_ptr[3] = {nullptr, nullptr, nullptr};
    uint2* terms[3] = {nullptr, nullptr, nullptr};
    uint32_t* long_cols[3] = {nullptr, nullptr, nullptr};
    uint4* segs = nullptr;
    uint32_t *comb_cols = nullptr, *comb_ptr = nullptr;
    Fr* pool_mont = nullptr;
    size_t terms_total = 0, n_segs = 0, n_comb = 0;
    void release() {
        for (int m = 0; m < 3; ++m) {
            if (col_ptr[m]) (void)hipFree(col_ptr[m]);
            if (terms[m]) (void)hipFree(terms[m]);
            if (long_cols[m]) (void)hipFree(long_cols[m]);
        }
        if (segs) (void)hipFree(segs);
        if (comb_cols) (void)hipFree(comb_cols);
        if (comb_ptr) (void)hipFree(comb_ptr);
        if (pool_mont) (void)hipFree(pool_mont);
    }
    gkr::R1csCsc csc() const {
        gkr::R1csCsc c;
        for (int m = 0; m < 3; ++m) {
            c.col_ptr[m] = col_ptr[m];
            c.terms[m] = terms[m];
        }
        c.pool_mont = pool_mont;
        c.segs = segs;
        c.comb_cols = comb_cols;
        c.comb_ptr = comb_ptr;
        c.n_segs = (uint32_t)n_segs;
        c.n_comb = (uint32_t)n_comb;
        c.n_wires = info.n_wires;
        c.n_y = info.n_y;
        return c;
    }
};

namespace gkr_host {

// the argument checks of the two resident entry points (plain returns: decided before the context is looked at)
static bool r1cs_rows_args(const gkr_ctx* ctx, const gkr_r1cs_rows* rows, const void* d_witness, size_t stride_elements, int batch) {
    if (!ctx || !rows || !d_witness) return false;
    if (batch < 1 || batch > 65535) return false;
    if (rows->ctx != ctx) return false;
    if (stride_elements < rows->info.n_wires) return false;
    if ((((unsigned long long)batch * 3ull) << rows->info.n) > (1ull << 30)) return false;   // batch * 3 * 2^n values
    return true;
}

template <typename T>
static hipError_t upload_new(T** d, const T* h, size_t count) {
    hipError_t rc = hipMalloc(reinterpret_cast<void**>(d), std::max<size_t>(count, 1) * sizeof(T));
    if (rc == hipSuccess && count) rc = hipMemcpy(*d, h, count * sizeof(T), hipMemcpyHostToDevice);
    return rc;
}

static int upload_rows(gkr_ctx* ctx, const gkr_r1cs* r1cs, gkr_r1cs_rows* rows) {
    const gkr_r1cs_csr_info_t& info = rows->info;
    std::vector<uint32_t> row_ptr(info.n_constraints + 1), long_rows;
    std::vector<gkr_r1cs_term> terms;
    std::vector<gkr_fr> pool(info.n_pool);
    for (int m = 0; m < 3; ++m) {
        terms.resize(info.n_terms[m]);
        long_rows.resize(info.n_long_rows[m]);
        if (const int rc = gkr_r1cs_csr_export(r1cs, m, row_ptr.data(), terms.data(), long_rows.data(), m == 0 ? pool.data() : nullptr))
            return ctx->fail(rc, "gkr_r1cs_csr_export");
        HIP_TRY(ctx, upload_new(&rows->row_ptr[m], row_ptr.data(), row_ptr.size()));
        HIP_TRY(ctx, upload_new(&rows->terms[m], reinterpret_cast<const uint2*>(terms.data()), terms.size()));
        HIP_TRY(ctx, upload_new(&rows->long_rows[m], long_rows.data(), long_rows.size()));
        rows->terms_total += terms.size();
    }
    std::vector<Fr> pool_mont(pool.size());
    for (size_t i = 0; i < pool.size(); ++i) pool_mont[i] = gkr::to_mont(to_dev(pool[i]));   // canonical witness x Montgomery coefficient
    HIP_TRY(ctx, upload_new(&rows->pool_mont, pool_mont.data(), pool_mont.size()));
    return GKR_OK;
}

// The tables of `batch` witnesses into d_out and, with out_first_bad, the row check; everything queued on the context's stream,
// the caller synchronises.  Workspace slots are this path's own ("r1cs.*").
static int run_r1cs_rows(gkr_ctx* ctx, const gkr_r1cs_rows* rows, const Fr* d_witness, size_t stride, int batch, Fr* d_out,
                         uint32_t* out_first_bad) {
    hipStream_t s = ctx->stream;
    const double len = (double)((size_t)1 << rows->info.n);
    {
        Timed t(ctx, "r1cs_rows", (double)batch * (8.0 * rows->terms_total + 32.0 * rows->terms_total + 32.0 * 3.0 * len));
        gkr::launch_r1cs_rows(rows->csr(), d_witness, stride, (uint32_t)batch, d_out, s);
    }
    if (out_first_bad) {
        uint32_t* d_bad = nullptr;
        WS(ctx, "r1cs.first_bad", uint32_t, batch, d_bad);
        {
            Timed t(ctx, "r1cs_check", (double)batch * 3.0 * 32.0 * (double)rows->info.n_constraints);
            HIP_TRY(ctx, gkr::launch_r1cs_check(d_out, rows->info.n, (uint32_t)rows->info.n_constraints, (uint32_t)batch, d_bad, s));
        }
        HIP_TRY(ctx, hipMemcpyAsync(out_first_bad, d_bad, (size_t)batch * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

// eq(z, .) (A B - C) on the tables of `batch` resident witnesses: terms {2, {0, 1}} coefficient 1 and {1, {2}} coefficient r - 1
static int run_r1cs_zerocheck(gkr_ctx* ctx, const gkr_r1cs_rows* rows, const Fr* d_witness, size_t stride, int batch, const gkr_fr* z,
                              gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq,
                              uint32_t* out_first_bad) {
    const int n = (int)rows->info.n;
    const gkr_sop_term terms[2] = {{2, {0, 1, 0}}, {1, {2, 0, 0}}};
    gkr_fr coeffs[2] = {{{1, 0, 0, 0}}, {{0, 0, 0, 0}}};
    memcpy(&coeffs[1], gkr::h64::kMod, 32);
    coeffs[1].l[0] -= 1;   // r - 1 (r is odd: no borrow)
    gkr::SopTerms ts;
    gkr::SopCoeffs cf;
    if (!sop_shape(n, 3, terms, 2, batch, &ts) || !sop_coeffs(coeffs, 2, &cf)) return ctx->fail(GKR_ERR_INVALID, "R1CS zero-check shape");
    Fr* d_tables = nullptr;
    WS(ctx, "r1cs.tables", Fr, ((size_t)batch * 3) << n, d_tables);
    if (const int rc = run_r1cs_rows(ctx, rows, d_witness, stride, batch, d_tables, out_first_bad)) return rc;
    return run_zerocheck_batch(ctx, d_tables, n, ts, cf, batch, z, out_coeffs, out_len, out_r, out_evals, out_eq);
}

// ---- the inner sumcheck: the column-major form, the table T, the product path on (T, w)

// the argument checks of the two resident entry points of the columns (plain returns: decided before the context is looked at)
static bool r1cs_cols_args(const gkr_ctx* ctx, const gkr_r1cs_cols* cols, const gkr_fr* x, const gkr_fr* rho, int batch) {
    if (!ctx || !cols || !x || !rho) return false;
    if (batch < 1 || batch > 65535) return false;
    if (cols->ctx != ctx) return false;
    if (cols->info.n_y > 29 || (((unsigned long long)batch * 2ull) << cols->info.n_y) > (1ull << 30)) return false;   // batch * 2 * 2^n_y values
    if (((unsigned long long)batch << cols->info.n_x) > (1ull << 30)) return false;                                   // batch * 2^n_x values
    return true;
}

// The records go up as the host exports them; the long columns of the three matrices are cut into segments of at most `segment`
// records (0: one segment per long column and matrix), listed column by column so that one column's partials are neighbours.
static int upload_cols(gkr_ctx* ctx, const gkr_r1cs* r1cs, uint32_t segment, gkr_r1cs_cols* cols) {
    const gkr_r1cs_csc_info_t& info = cols->info;
    std::vector<uint32_t> col_ptr((size_t)info.n_wires + 1), long_cols;
    std::vector<gkr_r1cs_term> terms;
    std::vector<gkr_fr> pool(info.n_pool);
    std::vector<uint4> segs;
    for (int m = 0; m < 3; ++m) {
        terms.resize(info.n_terms[m]);
        long_cols.resize(info.n_long_cols[m]);
        if (const int rc = gkr_r1cs_csc_export(r1cs, m, col_ptr.data(), terms.data(), long_cols.data(), m == 0 ? pool.data() : nullptr))
            return ctx->fail(rc, "gkr_r1cs_csc_export");
        HIP_TRY(ctx, upload_new(&cols->col_ptr[m], col_ptr.data(), col_ptr.size()));
        HIP_TRY(ctx, upload_new(&cols->terms[m], reinterpret_cast<const uint2*>(terms.data()), terms.size()));
        HIP_TRY(ctx, upload_new(&cols->long_cols[m], long_cols.data(), long_cols.size()));
        cols->terms_total += terms.size();
        for (const uint32_t col : long_cols) {
            const uint64_t end = col_ptr[(size_t)col + 1], step = segment ? segment : end - col_ptr[col];
            for (uint64_t at = col_ptr[col]; at < end; at += step)
                segs.push_back(make_uint4(col, (uint32_t)m, (uint32_t)at, (uint32_t)std::min(at + step, end)));
        }
    }
    if (segs.size() > 0x7FFFFFFFull) return ctx->fail(GKR_ERR_UNSUPPORTED, "more than 2^31 - 1 segments of long columns");
    std::stable_sort(segs.begin(), segs.end(), [](const uint4& a, const uint4& b) { return a.x < b.x; });
    std::vector<uint32_t> comb_cols, comb_ptr;
    for (size_t i = 0; i < segs.size(); ++i)
        if (i == 0 || segs[i].x != segs[i - 1].x) {
            comb_cols.push_back(segs[i].x);
            comb_ptr.push_back((uint32_t)i);
        }
    comb_ptr.push_back((uint32_t)segs.size());
    cols->n_segs = segs.size();
    cols->n_comb = comb_cols.size();
    HIP_TRY(ctx, upload_new(&cols->segs, segs.data(), segs.size()));
    HIP_TRY(ctx, upload_new(&cols->comb_cols, comb_cols.data(), comb_cols.size()));
    HIP_TRY(ctx, upload_new(&cols->comb_ptr, comb_ptr.data(), comb_ptr.size()));
    std::vector<Fr> pool_mont(pool.size());
    for (size_t i = 0; i < pool.size(); ++i) pool_mont[i] = gkr::to_mont(to_dev(pool[i]));   // canonical eq entry x Montgomery coefficient
    HIP_TRY(ctx, upload_new(&cols->pool_mont, pool_mont.data(), pool_mont.size()));
    return GKR_OK;
}

static int prepare_cols(gkr_ctx* ctx, const gkr_r1cs* r1cs, uint32_t segment, gkr_r1cs_cols** out) {
    if (!ctx || !r1cs || !out) return GKR_ERR_INVALID;
    *out = nullptr;
    if (segment != 0 && segment < 64) return GKR_ERR_INVALID;   // a segment is a wave's work
    std::unique_ptr<gkr_r1cs_cols, void (*)(gkr_r1cs_cols*)> cols(new gkr_r1cs_cols(), gkr_r1cs_cols_free);
    if (const int rc = gkr_r1cs_csc_info(r1cs, &cols->info)) return rc;
    cols->ctx = ctx;
    GKR_ENTER(ctx);
    if (const int rc = upload_cols(ctx, r1cs, segment, cols.get())) return rc;
    *out = cols.release();
    return GKR_OK;
}

// The tables T_b of `batch` sumchecks into d_out (table b at b * out_stride elements); everything queued on the context's stream,
// the caller synchronises -- `stage` holds the points and the weights until then.  Workspace slots are this path's own
// ("r1cs.cols.*").  x and rho are canonical (the caller's check).
static int run_r1cs_cols(gkr_ctx* ctx, const gkr_r1cs_cols* cols, const gkr_fr* x, const gkr_fr* rho, int batch, Fr* d_out, size_t out_stride,
                         std::vector<Fr>& stage) {
    hipStream_t s = ctx->stream;
    const uint32_t n_x = cols->info.n_x;
    const size_t n_pts = (size_t)batch * n_x, n_rho = (size_t)batch * 3;
    stage.resize(n_pts + n_rho);
    for (size_t i = 0; i < n_pts; ++i) stage[i] = to_dev(x[i]);
    for (size_t i = 0; i < n_rho; ++i) stage[n_pts + i] = gkr::to_mont(to_dev(rho[i]));   // canonical column sum x Montgomery rho
    Fr *d_stage = nullptr, *d_eq = nullptr, *d_part = nullptr;
    WS(ctx, "r1cs.cols.points", Fr, stage.size(), d_stage);
    WS(ctx, "r1cs.cols.eq", Fr, (size_t)batch << n_x, d_eq);
    WS(ctx, "r1cs.cols.partials", Fr, std::max<size_t>((size_t)batch * cols->n_segs, 1), d_part);
    HIP_TRY(ctx, hipMemcpyAsync(d_stage, stage.data(), stage.size() * sizeof(Fr), hipMemcpyHostToDevice, s));
    {
        Timed t(ctx, "r1cs_cols_eq", (double)batch * 32.0 * (double)((size_t)1 << n_x));
        gkr::launch_eq_table(d_stage, n_x, 0u, n_x, d_eq, false, (uint32_t)batch, s);
    }
    {
        const double len = (double)((size_t)1 << cols->info.n_y);
        Timed t(ctx, "r1cs_cols", (double)batch * (8.0 * cols->terms_total + 32.0 * cols->terms_total + 32.0 * len));
        gkr::launch_r1cs_cols(cols->csc(), d_eq, n_x, d_stage + n_pts, (uint32_t)batch, d_part, d_out, out_stride, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

// {T_b, w_b zero-padded} in the product path's layout, then that path at degree 2 (which synchronises)
static int run_r1cs_inner(gkr_ctx* ctx, const gkr_r1cs_cols* cols, const Fr* d_witness, size_t stride, int batch, const gkr_fr* x,
                          const gkr_fr* rho, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    const int n_y = (int)cols->info.n_y;
    const size_t len = (size_t)1 << n_y;
    Fr* d_tables = nullptr;
    WS(ctx, "r1cs.cols.tables", Fr, ((size_t)batch * 2) << n_y, d_tables);
    std::vector<Fr> stage;
    if (const int rc = run_r1cs_cols(ctx, cols, x, rho, batch, d_tables, 2 * len, stage)) return rc;
    gkr::launch_r1cs_pad_witness(d_witness, stride, cols->info.n_wires, cols->info.n_y, (uint32_t)batch, d_tables + len, 2 * len, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return run_product_batch(ctx, d_tables, n_y, 2, batch, out_coeffs, out_len, out_r, out_evals);
}

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

int gkr_r1cs_cols_prepare(gkr_ctx* ctx, const gkr_r1cs* r1cs, gkr_r1cs_cols** out) {
    return prepare_cols(ctx, r1cs, GKR_R1CS_COL_SEGMENT, out);
}

int gkr_r1cs_cols_prepare_segment(gkr_ctx* ctx, const gkr_r1cs* r1cs, uint32_t segment, gkr_r1cs_cols** out) {
    return prepare_cols(ctx, r1cs, segment, out);
}

int gkr_r1cs_cols_info(const gkr_r1cs_cols* cols, gkr_r1cs_csc_info_t* out) {
    if (!cols || !out) return GKR_ERR_INVALID;
    *out = cols->info;
    return GKR_OK;
}

void gkr_r1cs_cols_free(gkr_r1cs_cols* cols) {
    if (!cols) return;
    if (cols->ctx) (void)hipSetDevice(cols->ctx->device);
    cols->release();
    delete cols;
}

int gkr_r1cs_cols_device(gkr_ctx* ctx, const gkr_r1cs_cols* cols, const gkr_fr* x, const gkr_fr* rho, int batch, void* d_out,
                         size_t out_stride_elements) {
    if (!r1cs_cols_args(ctx, cols, x, rho, batch) || !d_out) return GKR_ERR_INVALID;
    if (out_stride_elements < ((size_t)1 << cols->info.n_y)) return GKR_ERR_INVALID;
    if (!all_canonical(x, (size_t)batch * cols->info.n_x)) return ctx->fail(GKR_ERR_NON_CANONICAL, "x entry >= r");
    if (!all_canonical(rho, (size_t)batch * 3)) return ctx->fail(GKR_ERR_NON_CANONICAL, "rho entry >= r");
    GKR_ENTER(ctx);
    std::vector<Fr> stage;
    if (const int rc = run_r1cs_cols(ctx, cols, x, rho, batch, static_cast<Fr*>(d_out), out_stride_elements, stage)) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

int gkr_r1cs_inner_batch_device(gkr_ctx* ctx, const gkr_r1cs_cols* cols, const void* d_witness, size_t stride_elements, int batch,
                                const gkr_fr* x, const gkr_fr* rho, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    if (!r1cs_cols_args(ctx, cols, x, rho, batch) || !d_witness || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (stride_elements < cols->info.n_wires) return GKR_ERR_INVALID;
    if (!all_canonical(x, (size_t)batch * cols->info.n_x)) return ctx->fail(GKR_ERR_NON_CANONICAL, "x entry >= r");
    if (!all_canonical(rho, (size_t)batch * 3)) return ctx->fail(GKR_ERR_NON_CANONICAL, "rho entry >= r");
    GKR_ENTER(ctx);
    return run_r1cs_inner(ctx, cols, static_cast<const Fr*>(d_witness), stride_elements, batch, x, rho, out_coeffs, out_len, out_r, out_evals);
}

int gkr_r1cs_inner(gkr_ctx* ctx, const gkr_r1cs* r1cs, const gkr_fr* witness, size_t n_witness, const gkr_fr* x, const gkr_fr* rho,
                   gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals) {
    if (!ctx || !r1cs || !witness || !x || !rho || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr_r1cs_csc_info_t info;
    if (const int rc = gkr_r1cs_csc_info(r1cs, &info)) return rc;
    if (n_witness < info.n_wires) return GKR_ERR_INVALID;
    if (info.n_y > 29 || (2ull << info.n_y) > (1ull << 30) || (1ull << info.n_x) > (1ull << 30)) return GKR_ERR_INVALID;   // the caps of the resident call at batch 1
    if (!all_canonical(x, (size_t)info.n_x)) return ctx->fail(GKR_ERR_NON_CANONICAL, "x entry >= r");
    if (!all_canonical(rho, 3)) return ctx->fail(GKR_ERR_NON_CANONICAL, "rho entry >= r");
    if (!all_canonical(witness, n_witness)) return ctx->fail(GKR_ERR_NON_CANONICAL, "witness entry >= r");
    gkr_r1cs_cols* raw = nullptr;
    if (const int rc = gkr_r1cs_cols_prepare(ctx, r1cs, &raw)) return rc;
    std::unique_ptr<gkr_r1cs_cols, void (*)(gkr_r1cs_cols*)> cols(raw, gkr_r1cs_cols_free);
    return run_on_upload(ctx, witness, info.n_wires, [&](const Fr* d) {
        return run_r1cs_inner(ctx, cols.get(), d, info.n_wires, 1, x, rho, out_coeffs, out_len, out_r, out_evals);
    });
}

int gkr_r1cs_rows_prepare(gkr_ctx* ctx, const gkr_r1cs* r1cs, gkr_r1cs_rows** out) {
    if (!ctx || !r1cs || !out) return GKR_ERR_INVALID;
    *out = nullptr;
    std::unique_ptr<gkr_r1cs_rows, void (*)(gkr_r1cs_rows*)> rows(new gkr_r1cs_rows(), gkr_r1cs_rows_free);
    if (const int rc = gkr_r1cs_csr_info(r1cs, &rows->info)) return rc;
    rows->ctx = ctx;
    GKR_ENTER(ctx);
    if (const int rc = upload_rows(ctx, r1cs, rows.get())) return rc;
    *out = rows.release();
    return GKR_OK;
}

int gkr_r1cs_rows_info(const gkr_r1cs_rows* rows, gkr_r1cs_csr_info_t* out) {
    if (!rows || !out) return GKR_ERR_INVALID;
    *out = rows->info;
    return GKR_OK;
}

void gkr_r1cs_rows_free(gkr_r1cs_rows* rows) {
    if (!rows) return;
    if (rows->ctx) (void)hipSetDevice(rows->ctx->device);
    rows->release();
    delete rows;
}

int gkr_r1cs_rows_device(gkr_ctx* ctx, const gkr_r1cs_rows* rows, const void* d_witness, size_t stride_elements, int batch, void* d_out,
                         uint32_t* out_first_bad) {
    if (!r1cs_rows_args(ctx, rows, d_witness, stride_elements, batch) || !d_out) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    if (const int rc = run_r1cs_rows(ctx, rows, static_cast<const Fr*>(d_witness), stride_elements, batch, static_cast<Fr*>(d_out), out_first_bad))
        return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

int gkr_r1cs_zerocheck_batch_device(gkr_ctx* ctx, const gkr_r1cs_rows* rows, const void* d_witness, size_t stride_elements, int batch,
                                    const gkr_fr* z, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq,
                                    uint32_t* out_first_bad) {
    if (!r1cs_rows_args(ctx, rows, d_witness, stride_elements, batch) || !z || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    if (!all_canonical(z, (size_t)batch * rows->info.n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    return run_r1cs_zerocheck(ctx, rows, static_cast<const Fr*>(d_witness), stride_elements, batch, z, out_coeffs, out_len, out_r, out_evals,
                              out_eq, out_first_bad);
}

int gkr_r1cs_zerocheck(gkr_ctx* ctx, const gkr_r1cs* r1cs, const gkr_fr* witness, size_t n_witness, const gkr_fr* z, gkr_fr* out_coeffs,
                       uint32_t* out_len, gkr_fr* out_r, gkr_fr* out_evals, gkr_fr* out_eq, uint32_t* out_first_bad) {
    if (!ctx || !r1cs || !witness || !z || !out_coeffs || !out_len || !out_r) return GKR_ERR_INVALID;
    gkr_r1cs_csr_info_t info;
    if (const int rc = gkr_r1cs_csr_info(r1cs, &info)) return rc;
    if (n_witness < info.n_wires) return GKR_ERR_INVALID;
    if ((3ull << info.n) > (1ull << 30)) return GKR_ERR_INVALID;   // 3 * 2^n values: the cap of the resident call at batch 1
    if (!all_canonical(z, (size_t)info.n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    if (!all_canonical(witness, n_witness)) return ctx->fail(GKR_ERR_NON_CANONICAL, "witness entry >= r");
    gkr_r1cs_rows* raw = nullptr;
    if (const int rc = gkr_r1cs_rows_prepare(ctx, r1cs, &raw)) return rc;
    std::unique_ptr<gkr_r1cs_rows, void (*)(gkr_r1cs_rows*)> rows(raw, gkr_r1cs_rows_free);
    return run_on_upload(ctx, witness, info.n_wires, [&](const Fr* d) {
        return run_r1cs_zerocheck(ctx, rows.get(), d, info.n_wires, 1, z, out_coeffs, out_len, out_r, out_evals, out_eq, out_first_bad);
    });
}

}  // extern "C"

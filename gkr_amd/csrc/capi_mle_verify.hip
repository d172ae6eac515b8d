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
//      device (k_verify_hash through capi_verify.hip's launcher, on the side stream beside the evaluation; rows of two slots are
//      repacked to the kernel's three on the way into the staging buffer, rows of three and four go as they are), a smaller one
//      hashes on the context's host threads.  Both fill the same slots by the same rule, so verdicts do not depend on where the
//      hashes ran;
//   3. meanwhile the host threads run everything that needs neither: shape, canonical checks, the round sums and the Horner
//      steps of every transcript (pre_relations; verify_rounds.h holds the round relations, the R1CS verifier uses them too);
//   4. ONE synchronisation, then per transcript the challenge comparisons and the last relation (finish).
// The order of the checks is the reference's; a value computed from unchecked elements (a hash of a malformed row, T at a
// non-canonical point) is never consulted: checks 1 and 2 come first.
#include <atomic>

#include "capi_internal.h"
#include "verify_rounds.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;

using V::HashSlot;   // (verify_rounds.h)
using V::Pre;
using V::pre_relations;
static_assert(sizeof(HashSlot) == sizeof(gkr::VerifyHashSlot) && offsetof(HashSlot, valid) == offsetof(gkr::VerifyHashSlot, valid),
              "the kernel writes the slots the relations read");
constexpr int kRelPiece = 8, kHashPiece = 16; // transcripts / round vectors per piece of host work
static_assert(V::kMaxRowWidth == 4, "the hash kernel has rows of three and of four slots");

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

int alloc_status(gkr_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return ctx->fail(GKR_ERR_NOMEM, std::string(what) + ": out of device memory");
    }
    return ctx->hip_fail(e, what);
}
#define MLEV_WS(ctx, slot, bytes, ptr)                                                              \
    do {                                                                                            \
        const hipError_t _e = (ctx)->workspace(slot, (bytes), reinterpret_cast<void**>(&(ptr)));    \
        if (_e != hipSuccess) return alloc_status(ctx, _e, slot);                                   \
    } while (0)

// sumchecks of a chunk: what fits verify_workspace_mb.  Chunks are counted in sumchecks: the M tables of a sumcheck are never
// split over two chunks.  A sumcheck's price is an upper bound of its share, M times what a table evaluated on its own needs
// (plan, weights, half tables, partials, point, value) and its n hash rows: the plan, the weights and the half tables are in fact
// built once per sumcheck (queue_eval allocates that much), but the price per table is what the chunk boundaries of the plain
// and the product verifier have been and stays, so that no call's chunking moves.
size_t chunk_tables(int n, int M, int D, int batch, bool hashes) {
    long long mb = gkr::opt(gkr::OPT_verify_workspace_mb);
    if (mb <= 0) mb = 2048;
    const size_t hash_row = (size_t)hash_slots(D) * 8 * sizeof(uint32_t);
    const size_t one = (size_t)M * (gkr::mle_eval_ws_bytes((uint32_t)n, 1, 1) + (size_t)n * sizeof(Fr) + sizeof(Fr)) +
                       (hashes ? (size_t)n * (hash_row + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot)) : 0);
    const size_t chunk = ((size_t)mb << 20) / one;
    return std::max<size_t>(1, std::min<size_t>({chunk, (size_t)32768 / M, (size_t)batch}));   // (the table is a grid dimension of the launches)
}

// the device side of a chunk, queued on the main stream: points up (h_pts: pinned, one per group of G tables: groups x n), the
// evaluation of the chunk's groups x G tables, values down (h_out: pinned, one per table)
int queue_eval(gkr_ctx* ctx, const Fr* d_tables, int n, uint32_t groups, uint32_t G, const Fr* h_pts, Fr* h_out) {
    Fr *d_pts, *d_out;
    void* d_ws;
    const size_t nt = (size_t)groups * G;
    MLEV_WS(ctx, "mlev_pts", (size_t)groups * n * sizeof(Fr), d_pts);
    MLEV_WS(ctx, "mlev_out", nt * sizeof(Fr), d_out);
    MLEV_WS(ctx, "mlev_ws", gkr::mle_eval_ws_bytes((uint32_t)n, groups, G), d_ws);
    HIP_TRY(ctx, hipMemcpyAsync(d_pts, h_pts, (size_t)groups * n * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    {
        Timed t(ctx, "mle_eval", (double)nt * 32.0 * (double)((size_t)1 << n));
        gkr::launch_mle_eval(d_tables, (uint32_t)n, groups, G, d_pts, d_ws, d_out, ctx->stream);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)nt * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    return GKR_OK;
}

int verify_chunk(gkr_ctx* ctx, const Fr* d_tables, int n, const Terms& T, uint32_t nb, const gkr_fr* claims, const gkr_fr* coeffs, const uint32_t* len,
                 const gkr_fr* r, int* accept, uint32_t* failed_round, uint32_t* failed_check, gkr_fr* out_claims, gkr_fr* out_evals) {
    hipStream_t st = ctx->stream;
    const int degree = T.D;   // of the round polynomials: the rows' and the hash kernel's form
    const size_t n_rows = (size_t)nb * n, W = row_width(degree), M = (size_t)T.M, nt = (size_t)nb * M;
    const bool dev_hash = verify_device_hash_wanted(n_rows);
    // ---- the host's share, in pieces: the relations of kRelPiece transcripts, then (host hashing) kHashPiece round vectors
    std::vector<Pre> pre(nb);
    std::vector<HashSlot> host_slots(dev_hash ? 0 : n_rows);
    const HashSlot* slots = host_slots.data();
    const size_t rel_pieces = (nb + kRelPiece - 1) / kRelPiece, hash_pieces = dev_hash ? 0 : (n_rows + kHashPiece - 1) / kHashPiece;
    std::atomic<size_t> next{0};
    const std::function<bool()> host_work = [&] {
        const size_t a = next.fetch_add(1, std::memory_order_relaxed);
        if (a < hash_pieces) {   // (the hashes first: they are the long pieces)
            for (size_t s = a * kHashPiece; s < std::min(n_rows, (a + 1) * kHashPiece); ++s)
                host_hash_slot(coeffs + W * s, (uint32_t)W, len[s], &host_slots[s]);
            return true;
        }
        if (a < hash_pieces + rel_pieces) {
            for (size_t b = (a - hash_pieces) * kRelPiece; b < std::min<size_t>(nb, (a - hash_pieces + 1) * kRelPiece); ++b)
                pre[b] = pre_relations(n, degree, claims ? claims + b : nullptr, coeffs + W * b * n, len + b * n, r + b * n);
            return true;
        }
        return false;
    };
    // the side stream's work is joined on every way out: nothing may still read or write a workspace the next call reuses
    struct SideJoin {
        hipStream_t forked = nullptr;
        ~SideJoin() {
            if (forked) (void)hipStreamSynchronize(forked);
        }
    } side;
    // ---- the device's share: hashes on the side stream, the evaluation on the main stream
    Fr *h_pts, *h_out;
    HIP_TRY(ctx, ctx->pinned_host("mlev_pts", n_rows * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("mlev_out", nt * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    if (dev_hash) {
        const int hs = hash_slots(degree);
        const size_t hw = (size_t)hs * 8, lead = ((size_t)hs - W) * 8;   // words of a kernel row; of its slots the transcript's rows lack
        uint32_t *d_hin, *h_hin;
        gkr::VerifyHashSlot *d_hout, *h_hout;
        MLEV_WS(ctx, "mlev_hash_in", n_rows * (hw + 1) * sizeof(uint32_t), d_hin);
        MLEV_WS(ctx, "mlev_hash_out", n_rows * sizeof(gkr::VerifyHashSlot), d_hout);
        HIP_TRY(ctx, ctx->pinned_host("mlev_hash_in", n_rows * (hw + 1) * sizeof(uint32_t), reinterpret_cast<void**>(&h_hin)));
        HIP_TRY(ctx, ctx->pinned_host("mlev_hash_out", n_rows * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_hout)));
        if (lead == 0) {
            memcpy(h_hin, coeffs, n_rows * hw * sizeof(uint32_t));
        } else {
            for (size_t s = 0; s < n_rows; ++s) {   // W slots -> the kernel's; the leading ones are never looked at for len <= W
                memset(h_hin + s * hw, 0, lead * sizeof(uint32_t));
                memcpy(h_hin + s * hw + lead, coeffs + W * s, W * sizeof(gkr_fr));
            }
        }
        memcpy(h_hin + n_rows * hw, len, n_rows * sizeof(uint32_t));
        HIP_TRY(ctx, ctx->aux_stream(2));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[0], st));             // fork: after whatever the main stream still holds
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->aux_events[0], 0));
        side.forked = ctx->aux;
        HIP_TRY(ctx, hipMemcpyAsync(d_hin, h_hin, n_rows * (hw + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->aux));
        if (const int rc = verify_hash_rows_device(ctx, hs, d_hin, d_hin + n_rows * hw, n_rows, d_hout, ctx->aux)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(h_hout, d_hout, n_rows * sizeof(gkr::VerifyHashSlot), hipMemcpyDeviceToHost, ctx->aux));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[1], ctx->aux));
        slots = reinterpret_cast<const HashSlot*>(h_hout);
    }
    memcpy(h_pts, r, n_rows * sizeof(Fr));   // a sumcheck's point once: its M tables share it
    if (const int rc = queue_eval(ctx, d_tables, n, nb, (uint32_t)M, h_pts, h_out)) return rc;
    if (dev_hash) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->aux_events[1], 0));   // join: the main stream's end is the side stream's too
    // ---- the host works while the device streams (waking the pool is worth some tens of hashes or transcripts)
    {
        gkr::SpinPool* pool = hash_pieces + rel_pieces >= 8 ? ctx->host_pool() : nullptr;
        gkr::SpinPool::Session session(pool, &host_work);
        while (host_work()) {
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    side.forked = nullptr;
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
    const size_t chunk = chunk_tables(n, T.M, T.D, batch, true), W = row_width(T.D), M = (size_t)T.M;
    for (size_t b = 0; b < (size_t)batch; b += chunk) {
        const uint32_t nb = (uint32_t)std::min(chunk, (size_t)batch - b);
        const int rc = verify_chunk(ctx, d_tables + ((b * M) << n), n, T, nb, claims ? claims + b : nullptr, coeffs + W * b * n, len + b * n,
                                    r + b * n, accept + b, failed_round ? failed_round + b : nullptr, failed_check ? failed_check + b : nullptr,
                                    out_claims ? out_claims + b : nullptr, out_evals ? out_evals + b * M : nullptr);
        if (rc) return rc;
    }
    return GKR_OK;
}

}  // namespace

extern "C" {

int gkr_mle_eval_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, const gkr_fr* points, gkr_fr* out) {
    // (plain returns: these are decided before the context is looked at)
    if (!ctx || !d_tables || !points || !out || batch < 1 || n < 1 || n > 30) return GKR_ERR_INVALID;
    if (!all_canonical(points, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "coordinate of a point >= r");
    GKR_ENTER(ctx);
    const size_t chunk = chunk_tables(n, 1, 1, batch, false);
    for (size_t b = 0; b < (size_t)batch; b += chunk) {
        const uint32_t nb = (uint32_t)std::min(chunk, (size_t)batch - b);
        Fr *h_pts, *h_out;
        HIP_TRY(ctx, ctx->pinned_host("mlev_pts", (size_t)nb * n * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
        HIP_TRY(ctx, ctx->pinned_host("mlev_out", (size_t)nb * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
        memcpy(h_pts, points + b * n, (size_t)nb * n * sizeof(Fr));
        if (const int rc = queue_eval(ctx, static_cast<const Fr*>(d_tables) + (b << n), n, nb, 1u, h_pts, h_out)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(out + b, h_out, (size_t)nb * sizeof(Fr));
    }
    return GKR_OK;
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

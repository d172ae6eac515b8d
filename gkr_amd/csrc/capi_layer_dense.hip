// The dense form of the GKR layer sumcheck: predicate tables of 2^(2 k_next) entries (gkr_predicate_tables), the device
// transcript's rounds over them, and the step-wise sessions of the trailing-variable split (gkr_layer_session_*).  Its kernels:
// kernels_layer_dense.hip.  The linear-time form over gate lists -- the default -- is capi_layer.hip.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// ------------------------------------------------------------- predicate tables
// E[g] = eq(z, g) = E_hi[g >> kl] * E_lo[g & mask]: two small tables per proof, built on the device from the points
// the host left in pinned memory (k_eq_table), E_lo in Montgomery form so that the product of the two is canonical.
static int upload_eq_tables(gkr_ctx* ctx, int k_i, const gkr_fr* z, int batch, Fr** e_hi_out, Fr** e_lo_out) {
    const int kl = k_i / 2, kh = k_i - kl;
    Fr *e_hi = nullptr, *e_lo = nullptr;
    WS(ctx, "pred.ehi", Fr, (size_t)batch << kh, e_hi);
    WS(ctx, "pred.elo", Fr, (size_t)batch << kl, e_lo);
    // the points go to pinned memory, the tables are built on the device from there (k_eq_table): no transfer call
    gkr_fr* hz = nullptr;
    HIP_TRY(ctx, ctx->pinned_host("pred.z", sizeof(gkr_fr) * (size_t)batch * (k_i ? k_i : 1), reinterpret_cast<void**>(&hz)));
    memcpy(hz, z, sizeof(gkr_fr) * (size_t)batch * k_i);
    gkr::launch_eq_table(reinterpret_cast<const Fr*>(hz), (uint32_t)k_i, 0u, (uint32_t)kh, e_hi, false, (uint32_t)batch, ctx->stream);
    gkr::launch_eq_table(reinterpret_cast<const Fr*>(hz), (uint32_t)k_i, (uint32_t)kh, (uint32_t)kl, e_lo, true, (uint32_t)batch, ctx->stream);
    *e_hi_out = e_hi;
    *e_lo_out = e_lo;
    return GKR_OK;
}

// builds canonical A, M (2^{2k} each) in device memory from device gate arrays
// shard (log_p, p) keeps the gates whose right operand has low bits p; tables then have 2^{2k - log_p} entries.
// batch > 1: `batch` proofs of one circuit -- same gates (the cell lists are built once), z is batch x k_i,
// d_A / d_M hold batch tables of N entries each.
static int build_predicates(gkr_ctx* ctx, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r,
                            const gkr_fr* z, Fr* d_A, Fr* d_M, uint32_t log_p = 0, uint32_t shard = 0, int batch = 1) {
    const size_t N = (size_t)1 << (2 * k - log_p);
    hipStream_t s = ctx->stream;
    Fr *e_hi = nullptr, *e_lo = nullptr;
    uint32_t* bad = nullptr;
    const int kl = k_i / 2;
    WS(ctx, "pred.bad", uint32_t, 1, bad);
    {
        const int rc_eq = upload_eq_tables(ctx, k_i, z, batch, &e_hi, &e_lo);
        if (rc_eq) return rc_eq;
    }
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, 4, s));
    const bool use_atomics = gkr::opt(gkr::OPT_predicate_atomics) != 0;
    if (!use_atomics || batch > 1) {
        // counting sort by cell, then one modular sum per cell (per proof)
        uint32_t *counts = nullptr, *offsets = nullptr, *cursor = nullptr, *bsums = nullptr, *list = nullptr;
        WS(ctx, "pred.counts", uint32_t, 2 * N, counts);
        WS(ctx, "pred.offsets", uint32_t, 2 * N, offsets);
        WS(ctx, "pred.cursor", uint32_t, 2 * N, cursor);
        WS(ctx, "pred.bsums", uint32_t, (2 * N + 2047) / 2048 + 1, bsums);
        WS(ctx, "pred.list", uint32_t, (size_t)1 << k_i, list);
        HIP_TRY(ctx, hipMemsetAsync(counts, 0, 2 * N * sizeof(uint32_t), s));
        Timed t(ctx, "predicate_sorted", (double)((size_t)1 << k_i) * (2 * 9.0 + 8.0) + (double)N * 2.0 * (3 * 4.0 + 32.0) * batch);
        gkr::launch_predicate_sorted(k_i, k, d_gt, d_l, d_r, e_hi, e_lo, (uint32_t)kl, log_p, shard, N, counts, offsets, cursor,
                                     bsums, list, bad, d_A, d_M, (uint32_t)batch, s);
    } else {
        // widened-atomic scatter (kept for comparison): 8 u64 limb atomics per gate into 64-byte cells
        unsigned long long *wideA = nullptr, *wideM = nullptr;
        WS(ctx, "pred.wideA", unsigned long long, N * 8, wideA);
        WS(ctx, "pred.wideM", unsigned long long, N * 8, wideM);
        HIP_TRY(ctx, hipMemsetAsync(wideA, 0, N * 64, s));
        HIP_TRY(ctx, hipMemsetAsync(wideM, 0, N * 64, s));
        {
            Timed t(ctx, "predicate_scatter", (double)((size_t)1 << k_i) * (9.0 + 64.0));
            gkr::launch_predicate_scatter(k_i, k, d_gt, d_l, d_r, e_hi, e_lo, (uint32_t)kl, wideA, wideM, bad, log_p, shard, s);
        }
        {
            Timed t(ctx, "predicate_normalise", (double)N * 2.0 * (64.0 + 32.0));
            gkr::launch_predicate_normalise(wideA, d_A, N, s);
            gkr::launch_predicate_normalise(wideM, d_M, N, s);
        }
    }
    uint32_t hbad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));   // also keeps the host tables alive until their upload is done
    if (hbad) return ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range");
    return GKR_OK;
}

// ------------------------------------------------------------- layer sumcheck, device transcript
// One proof: rounds over the dense predicate tables (kernels_layer_dense.hip), hashed by one lane per sumcheck
// (k_layer_round_hash); one uninterrupted stream of launches, one copy-back.  The fold with r_j is deferred into the pass that
// computes round j+1's sums (b-phase: the fused kernel; c-phase: a separate fold of the remaining row).
static int run_layer_dense_proof(gkr_ctx* ctx, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r, const gkr_fr* z,
                                 const Fr* d_W, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    const size_t N = (size_t)1 << (2 * k), wlen = (size_t)1 << k;
    const uint32_t v = 2 * k;
    hipStream_t s = ctx->stream;
    Fr *A = nullptr, *M = nullptr, *Wb = nullptr, *Wc = nullptr, *d_coeffs = nullptr, *d_r_out = nullptr;
    gkr::FixedMul* d_rtab = nullptr;
    uint32_t *d_len = nullptr, *dep = nullptr;
    gkr::LayerPartial* partials = nullptr;
    WS(ctx, "layer.A", Fr, N, A);
    WS(ctx, "layer.M", Fr, N, M);
    WS(ctx, "layer.Wb", Fr, wlen, Wb);
    WS(ctx, "layer.Wc", Fr, wlen, Wc);
    WS(ctx, "layer.coeffs", Fr, (size_t)v * 3, d_coeffs);
    WS(ctx, "layer.r", Fr, v, d_r_out);
    WS(ctx, "layer.rtab", gkr::FixedMul, v, d_rtab);
    WS(ctx, "layer.len", uint32_t, v, d_len);
    WS(ctx, "layer.dep", uint32_t, 32, dep);
    WS(ctx, "layer.partials", gkr::LayerPartial, gkr::kMaxLayerBlocks, partials);
    if (const int rc = build_predicates(ctx, k_i, k, d_gt, d_l, d_r, z, A, M)) return rc;
    const gkr::LayerBatch lb{1u, gkr::kMaxLayerBlocks, N, wlen};
    HIP_TRY(ctx, hipMemsetAsync(dep, 0, sizeof(uint32_t) * 32, s));
    gkr::launch_to_mont(d_W, Wb, (uint32_t)wlen, s);
    gkr::launch_to_mont(d_W, Wc, (uint32_t)wlen, s);
    gkr::launch_depends(d_W, k, dep, 1u, s);
    const gkr::FixedMul* pending = nullptr;   // challenge tables not yet applied to A, M
    const bool no_fused = gkr::opt(gkr::OPT_layer_no_fused) != 0;
    for (uint32_t round = 0; round < v; ++round) {
        const uint32_t h = (uint32_t)(N >> (round + 1));   // half of the table this round sums over
        const uint32_t phase = round < (uint32_t)k ? 0u : 1u;
        const uint32_t hb = phase == 0 ? (h >> k) : 0u;
        uint32_t nblk = 0;
        if (phase == 0 && !no_fused) {
            Timed t(ctx, "layer_round_fused", (pending ? (double)h * 2.0 * 6.0 : (double)h * 2.0 * 2.0) * 32.0);
            nblk = gkr::launch_layer_round_b(pending != nullptr, A, M, A, M, hb, (uint32_t)k, pending, Wb, Wc, partials, lb, s);
            pending = nullptr;
        } else {
            if (pending) {
                Timed t(ctx, "layer_fold", (double)h * 2.0 * 6.0 * 32.0);
                gkr::launch_layer_fold(A, M, 2 * h, pending, lb, s);
                pending = nullptr;
            }
            nblk = gkr::layer_blocks(h);
            if (nblk > 4096u) nblk = 4096u;
            Timed t(ctx, "layer_round", (double)h * 4.0 * 32.0);
            gkr::launch_layer_round(A, M, h, k, phase, hb, Wb, Wc, nblk, partials, lb, s);
        }
        Timed t(ctx, "layer_round_hash", 0.0);
        gkr::launch_layer_round_hash(partials, nblk, round, k, dep, ctx->d_cts, d_coeffs, d_len, d_r_out, d_rtab, Wb, Wc, s);
        pending = d_rtab + round;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_coeffs, d_coeffs, (size_t)v * 3 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, v * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_r, d_r_out, v * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->drain_events();
    return GKR_OK;
}

// The device transcript hashes on one lane per sumcheck and its round kernels take one proof: the proofs of a batch go
// through one after the other (complete and host-free, not fast: ~1 ms per round and proof).
int run_layer_dense(gkr_ctx* ctx, int batch, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r, const gkr_fr* z,
                    const Fr* d_W, gkr_fr* const* out_coeffs, uint32_t* const* out_len, gkr_fr* const* out_r) {
    if (k > kMaxDenseK)
        return ctx->fail(GKR_ERR_INVALID, "the device transcript works on dense 2^(2 k_next)-entry predicate tables: k_next <= 14 (GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT)");
    int rc = GKR_OK;
    for (int b = 0; b < batch && rc == GKR_OK; ++b)
        rc = run_layer_dense_proof(ctx, k_i, k, d_gt, d_l, d_r, z + (size_t)b * k_i, d_W + ((size_t)b << k), out_coeffs[b], out_len[b], out_r[b]);
    return rc;
}
}  // namespace gkr_host

extern "C" {

int gkr_predicate_tables(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gate_type, const uint32_t* left,
                         const uint32_t* right, const gkr_fr* z, gkr_fr* out_A, gkr_fr* out_M) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!out_A || !out_M) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    int rc = check_layer_args(ctx, k_i, k_next, gate_type, left, right, z);
    if (rc) return rc;
    GKR_ENTER(ctx);
    const size_t N = (size_t)1 << (2 * k_next);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> A, M;
    rc = upload_gates(ctx, (size_t)1 << k_i, gate_type, left, right, dgt, dl, dr);
    if (rc) return rc;
    HIP_TRY(ctx, A.alloc(N));
    HIP_TRY(ctx, M.alloc(N));
    rc = build_predicates(ctx, k_i, k_next, dgt.p, dl.p, dr.p, z, A.p, M.p);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_A, A.p, N * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_M, M.p, N * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

// build_predicates with its shard arguments and a copy-back: one shard's tables of 2^(2 k_next - log_p) entries, as
// gkr_layer_session_open builds them (the tests hold every shard to the whole layer's tables sliced by the cell rule)
int gkr_devtest_predicates(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gate_type, const uint32_t* left, const uint32_t* right,
                           const gkr_fr* z, uint32_t log_p, uint32_t shard, gkr_fr* out_A, gkr_fr* out_M) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!out_A || !out_M) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    int rc = check_layer_args(ctx, k_i, k_next, gate_type, left, right, z);
    if (rc) return rc;
    if (k_next > kMaxDenseK || log_p > (uint32_t)k_next || shard >= (1u << log_p))
        return ctx->fail(GKR_ERR_INVALID, "k_next <= GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT, log_p <= k_next and shard < 2^log_p");
    GKR_ENTER(ctx);
    const size_t N = (size_t)1 << (2 * k_next - (int)log_p);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> A, M;
    rc = upload_gates(ctx, (size_t)1 << k_i, gate_type, left, right, dgt, dl, dr);
    if (rc) return rc;
    HIP_TRY(ctx, A.alloc(N));
    HIP_TRY(ctx, M.alloc(N));
    rc = build_predicates(ctx, k_i, k_next, dgt.p, dl.p, dr.p, z, A.p, M.p, log_p, shard);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out_A, A.p, N * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_M, M.p, N * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->drain_events();
    return GKR_OK;
}

// The launch geometry of the dense layer forms at one round, from the functions the launches call (host logic only).
int gkr_selftest_layer_dense_geometry(int k_next, int log_p, int round, uint32_t out[8]) {
    if (!out || k_next < 1 || k_next > kMaxDenseK || log_p < 0 || log_p > k_next || round < 0 || round >= 2 * k_next - log_p)
        return GKR_ERR_INVALID;
    memset(out, 0, 8 * sizeof(uint32_t));
    const size_t N = (size_t)1 << (2 * k_next - log_p);
    const uint32_t h = (uint32_t)(N >> (round + 1));
    if (log_p == 0 && round < k_next) {   // run_layer_dense_proof's fused b-phase round: hb = h >> k row pairs, one proof
        const gkr::LayerRoundBGrid g = gkr::layer_round_b_grid(h >> k_next, (uint32_t)k_next, 1u);
        out[0] = g.col_blocks;
        out[1] = g.chunks;
        out[2] = g.rows_per_chunk;
        out[3] = g.partials;
    }
    // gkr_layer_session_sums / _bind of a shard at this round (log_p = 0: also the device transcript's unfused round)
    out[4] = gkr::layer_blocks(h) | (round < k_next ? 0u : 1u << 31);
    out[5] = gkr::layer_fold_blocks(h, 1u);
    out[6] = gkr::pred_scan_blocks(2 * N);
    out[7] = gkr::pred_sum_blocks(2 * N);
    return GKR_OK;
}

// ---- step-wise sessions: one sumcheck split across GPUs ------------------------
//
// The hypercube is partitioned by its TRAILING log2(P) variables: rank p owns the entries whose
// low index bits are p.  Rounds bind the LEADING variable, so both members of every pair live on
// the same rank for the first v - log2(P) rounds; each round every rank produces partial sums, one
// tiny all-reduce (<= 96 bytes of field elements) gives every rank the round polynomial, every
// rank derives the same challenge and folds its shard.  The library does the table work per rank;
// the collective and the transcript sit in the caller (gkr_amd/parallel.py: torch.distributed over
// RCCL, or gloo in the CPU tests).  P = 1 is the whole sumcheck with an external transcript.

struct gkr_layer_session {
    int k = 0, kc = 0;          // W has 2^k entries; this shard's column index has kc = k - log2(P) bits
    uint32_t round = 0, rounds = 0;
    size_t cells = 0;           // current entries per table half pair (A, M each)
    Fr *A = nullptr, *M = nullptr, *Wb = nullptr, *Wc = nullptr;
    gkr::LayerPartial* partials = nullptr;
    uint32_t* d_dep = nullptr;
    uint32_t dep[32] = {0};
    gkr::LayerHostRec* rec = nullptr;
    gkr::FixedMul* rtab = nullptr;   // pinned
};

static void free_layer_session(gkr_layer_session* s) {
    if (!s) return;
    if (s->A) (void)hipFree(s->A);
    if (s->M) (void)hipFree(s->M);
    if (s->Wb) (void)hipFree(s->Wb);
    if (s->Wc) (void)hipFree(s->Wc);
    if (s->partials) (void)hipFree(s->partials);
    if (s->d_dep) (void)hipFree(s->d_dep);
    if (s->rec) (void)hipHostFree(s->rec);
    if (s->rtab) (void)hipHostFree(s->rtab);
    delete s;
}

static int alloc_layer_session(gkr_ctx* ctx, gkr_layer_session* S, size_t cells, size_t wb, size_t wc) {
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->A), cells * sizeof(Fr)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->M), cells * sizeof(Fr)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->Wb), wb * sizeof(Fr)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->Wc), wc * sizeof(Fr)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->partials), gkr::kMaxLayerBlocks * sizeof(gkr::LayerPartial)));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&S->d_dep), 32 * sizeof(uint32_t)));
    HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&S->rec), sizeof(gkr::LayerHostRec), hipHostMallocCoherent | hipHostMallocMapped));
    HIP_TRY(ctx, hipHostMalloc(reinterpret_cast<void**>(&S->rtab), sizeof(gkr::FixedMul), hipHostMallocCoherent | hipHostMallocMapped));
    memset(S->rec, 0, sizeof(gkr::LayerHostRec));
    return GKR_OK;
}

int gkr_layer_session_open(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gate_type, const uint32_t* left,
                           const uint32_t* right, const gkr_fr* z, const gkr_fr* W, uint32_t nshards, uint32_t shard,
                           gkr_layer_session** out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!out || !W) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    *out = nullptr;
    int rc = check_layer_args(ctx, k_i, k_next, gate_type, left, right, z);
    if (rc) return rc;
    uint32_t log_p = 0;
    while ((1u << log_p) < nshards) ++log_p;
    if (nshards == 0 || (1u << log_p) != nshards || (int)log_p > k_next || shard >= nshards)
        return ctx->fail(GKR_ERR_INVALID, "shard count must be a power of two <= 2^k_next and shard < count");
    if (!all_canonical(W, (size_t)1 << k_next)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    gkr_layer_session* S = new gkr_layer_session();
    S->k = k_next;
    S->kc = k_next - (int)log_p;
    S->rounds = (uint32_t)(2 * k_next) - log_p;
    S->cells = (size_t)1 << (2 * k_next - log_p);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> dW;
    rc = alloc_layer_session(ctx, S, S->cells, (size_t)1 << k_next, (size_t)1 << S->kc);
    if (!rc) rc = upload_gates(ctx, (size_t)1 << k_i, gate_type, left, right, dgt, dl, dr);
    if (rc) {
        free_layer_session(S);
        return rc;
    }
    hipError_t e = dW.alloc((size_t)1 << k_next);
    if (e == hipSuccess) e = hipMemcpyAsync(dW.p, W, sizeof(Fr) << k_next, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        free_layer_session(S);
        return ctx->hip_fail(e, "upload W");
    }
    rc = build_predicates(ctx, k_i, k_next, dgt.p, dl.p, dr.p, z, S->A, S->M, log_p, shard);
    if (rc) {
        free_layer_session(S);
        return rc;
    }
    (void)hipMemsetAsync(S->d_dep, 0, 32 * sizeof(uint32_t), s);
    gkr::launch_to_mont(dW.p, S->Wb, 1u << k_next, s);
    gkr::launch_to_mont_strided(dW.p, S->Wc, 1u << S->kc, nshards, shard, s);
    gkr::launch_depends(dW.p, k_next, S->d_dep, 1, s);
    e = hipMemcpyAsync(S->dep, S->d_dep, 32 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        free_layer_session(S);
        return ctx->hip_fail(e, "layer session setup");
    }
    *out = S;
    return GKR_OK;
}

// the redundant tail after the all-gather: explicit tables of 2^kc entries (A, M, Wc) and the scalar W(b*)
int gkr_layer_session_open_tables(gkr_ctx* ctx, int kc, const gkr_fr* A, const gkr_fr* M, const gkr_fr* wb,
                                  const gkr_fr* Wc, gkr_layer_session** out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!A || !M || !wb || !Wc || !out || kc < 1 || kc > 14) return ctx->fail(GKR_ERR_INVALID, "bad tail tables");
    const size_t n = (size_t)1 << kc;
    if (!all_canonical(A, n) || !all_canonical(M, n) || !all_canonical(Wc, n) || !all_canonical(wb, 1))
        return ctx->fail(GKR_ERR_NON_CANONICAL, "tail table entry >= r");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    gkr_layer_session* S = new gkr_layer_session();
    S->k = kc;           // only c-variables remain: phase 1 from the first round
    S->kc = kc;
    S->round = (uint32_t)kc;   // counts as if k = kc b-rounds were already done
    S->rounds = (uint32_t)(2 * kc);
    S->cells = n;
    int rc = alloc_layer_session(ctx, S, n, 1, n);
    if (rc) {
        free_layer_session(S);
        return rc;
    }
    // W copies are kept in Montgomery form
    std::vector<Fr> wcm(n);
    for (size_t i = 0; i < n; ++i) wcm[i] = gkr::to_mont(to_dev(Wc[i]));
    Fr wbm = gkr::to_mont(to_dev(*wb));
    hipError_t e = hipMemcpyAsync(S->A, A, n * sizeof(Fr), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(S->M, M, n * sizeof(Fr), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(S->Wc, wcm.data(), n * sizeof(Fr), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(S->Wb, &wbm, sizeof(Fr), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        free_layer_session(S);
        return ctx->hip_fail(e, "tail session upload");
    }
    *out = S;
    return GKR_OK;
}

int gkr_layer_session_dep(gkr_ctx* ctx, const gkr_layer_session* S, uint32_t* out_dep, uint32_t count) {
    if (!ctx || !S || !out_dep || count > 32) return GKR_ERR_INVALID;
    for (uint32_t i = 0; i < count; ++i) out_dep[i] = S->dep[i];
    return GKR_OK;
}

int gkr_layer_session_rounds(const gkr_layer_session* S, uint32_t* done, uint32_t* total) {
    if (!S) return GKR_ERR_INVALID;
    if (done) *done = S->round;
    if (total) *total = S->rounds;
    return GKR_OK;
}

// partial sums of the current round over this shard: out = {c0, g(1), c2}, canonical
int gkr_layer_session_sums(gkr_ctx* ctx, gkr_layer_session* S, gkr_fr* out) {
    if (!ctx || !S || !out) return GKR_ERR_INVALID;
    if (S->round >= S->rounds) return ctx->fail(GKR_ERR_INVALID, "no round left in this session");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    const uint32_t h = (uint32_t)(S->cells / 2);
    const uint32_t phase = S->round < (uint32_t)S->k ? 0u : 1u;
    const uint32_t hb = phase == 0 ? (h >> S->kc) : 0u;
    const uint32_t nblk = gkr::layer_blocks(h);
    gkr::launch_layer_round(S->A, S->M, h, (uint32_t)S->kc, phase, hb, S->Wb, S->Wc, nblk, S->partials, gkr::single_layer(), s);
    const uint32_t ticket = ++ctx->ticket;
    gkr::launch_layer_round_reduce(S->partials, nblk, S->rec, ticket, gkr::single_layer(), s);
    HIP_TRY(ctx, hipGetLastError());
    int rc = wait_records(ctx, S->rec, 1, ticket);
    if (rc) return rc;
    memcpy(&out[0], &S->rec->c0, 32);
    memcpy(&out[1], &S->rec->g1, 32);
    memcpy(&out[2], &S->rec->c2, 32);
    return GKR_OK;
}

// bind the current variable to r
int gkr_layer_session_bind(gkr_ctx* ctx, gkr_layer_session* S, const gkr_fr* r) {
    if (!ctx || !S || !r) return GKR_ERR_INVALID;
    if (S->round >= S->rounds) return ctx->fail(GKR_ERR_INVALID, "no round left in this session");
    if (!all_canonical(r, 1)) return ctx->fail(GKR_ERR_NON_CANONICAL, "r >= modulus");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    gkr::h64::F r64;
    memcpy(&r64, r, 32);
    gkr::h64::make_fixed_mul(r64, S->rtab->w);
    const uint32_t h = (uint32_t)(S->cells / 2);
    const bool bphase = S->round < (uint32_t)S->k;
    // the W copy bound in this round: b-rounds fold Wb (2^k entries at the start), c-rounds fold Wc
    const uint32_t idx = bphase ? S->round : S->round - (uint32_t)S->k;
    const uint32_t hw = bphase ? (1u << (S->k - 1 - idx)) : (1u << (S->kc - 1 - idx));
    gkr::launch_fold_small(bphase ? S->Wb : S->Wc, hw, S->rtab, gkr::single_layer(), s);
    gkr::launch_layer_fold(S->A, S->M, h, S->rtab, gkr::single_layer(), s);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));   // rtab is reused by the next bind
    S->cells = h;
    S->round += 1;
    return GKR_OK;
}

// when every local round is done: out = {A, M, Wc (canonical), W(b*) (canonical)} of this shard
int gkr_layer_session_tail(gkr_ctx* ctx, gkr_layer_session* S, gkr_fr* out) {
    if (!ctx || !S || !out) return GKR_ERR_INVALID;
    if (S->round != S->rounds || S->cells != 1) return ctx->fail(GKR_ERR_INVALID, "session still has rounds to run");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    Fr a, m, wc, wb;
    HIP_TRY(ctx, hipMemcpyAsync(&a, S->A, sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&m, S->M, sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&wc, S->Wc, sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(&wb, S->Wb, sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    out[0] = to_abi(a);
    out[1] = to_abi(m);
    out[2] = to_abi(gkr::from_mont(wc));
    out[3] = to_abi(gkr::from_mont(wb));
    return GKR_OK;
}

void gkr_layer_session_close(gkr_ctx* ctx, gkr_layer_session* S) {
    if (ctx) (void)hipSetDevice(ctx->device);
    free_layer_session(S);
}

}  // extern "C"

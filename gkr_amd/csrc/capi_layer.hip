// The GKR layer sumcheck (prove_sumcheck_opt, rust/src/gkr/sumcheck.rs:36-156) in its linear-time form over gate lists with
// product passes: the gate-list build, the gate-sharded form, resident layers.  The dense form (predicate tables, the device
// transcript, step-wise sessions) is capi_layer_dense.hip.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// The host's share of one product pass of the layer sumcheck, scalar form (the IFMA-lane form is gkr_ifma_prod_pass,
// mimc_ifma.cpp; same arguments, same results).  Lane k: the 8 x 8 cross-sum matrix m[a][b] (W sub-block a times X
// sub-block b) and the Y sums sy[a] of its 2^J sub-blocks.  Round t (half = 2^(J-t-1)): with
//     P_xy = sum_{a < half} m[x half + a][y half + a],   S_x = sum_{a < half} sy[x half + a]
// the round polynomial is c2 X^2 + lin X + c0,  c0 = P_00 + S_0,  g(1) = P_11 + S_1,  c2 = P_11 - P_10 - P_01 + P_00,
// lin = g(1) - c0 - c2; the challenge is the hash of [c2, lin, c0] (2 + dep entries); binding the variable folds the
// matrix along both indices and sy along its one.  At the end the 2^J weights of the fold that binds the J variables.
void host_prod_pass_scalar(const uint64_t* recs, size_t rec_row_words, int count, int J, const uint32_t (*vec_len)[16],
                                  uint64_t (*c2)[16][4], uint64_t (*lin)[16][4], uint64_t (*c0)[16][4], uint64_t (*r)[16][4],
                                  uint64_t* weights, size_t w_row_words) {
    using namespace gkr::h64;
    const F* cts = host_mimc_constants64();
    const F one_m = to_mont(F{{1, 0, 0, 0}});
    for (int k = 0; k < count; ++k) {
        F M[64], SY[8], rm[gkr::kProdMaxJ];
        const F* rec = reinterpret_cast<const F*>(recs + (size_t)k * rec_row_words);
        const int n = 1 << J;
        for (int a = 0; a < n; ++a) {
            for (int b = 0; b < n; ++b) M[a * 8 + b] = rec[a * 8 + b];
            SY[a] = rec[64 + a];
        }
        for (int t = 0; t < J; ++t) {
            const int half = 1 << (J - t - 1);
            F p00 = M[0], p01 = M[half], p10 = M[half * 8], p11 = M[half * 8 + half], s0 = SY[0], s1 = SY[half];
            for (int x = 1; x < half; ++x) {
                p00 = add(p00, M[x * 8 + x]);
                p01 = add(p01, M[x * 8 + half + x]);
                p10 = add(p10, M[(half + x) * 8 + x]);
                p11 = add(p11, M[(half + x) * 8 + half + x]);
                s0 = add(s0, SY[x]);
                s1 = add(s1, SY[half + x]);
            }
            const F vc0 = add(p00, s0), g1 = add(p11, s1);
            const F vc2 = sub(add(p11, p00), add(p10, p01));
            const F vlin = sub(sub(g1, vc0), vc2);
            const uint32_t ln = vec_len[t][k];
            const F vec[3] = {vc2, vlin, vc0};
            const F rc = host_multi_hash(vec + (3 - ln), (int)ln, cts);
            memcpy(c2[t][k], &vc2, 32);
            memcpy(lin[t][k], &vlin, 32);
            memcpy(c0[t][k], &vc0, 32);
            memcpy(r[t][k], &rc, 32);
            rm[t] = to_mont(rc);
            for (int ra = 0; ra < half; ++ra)
                for (int cb = 0; cb < 2 * half; ++cb) M[ra * 8 + cb] = add(M[ra * 8 + cb], mont_mul(sub(M[(half + ra) * 8 + cb], M[ra * 8 + cb]), rm[t]));
            for (int ra = 0; ra < half; ++ra)
                for (int cb = 0; cb < half; ++cb) M[ra * 8 + cb] = add(M[ra * 8 + cb], mont_mul(sub(M[ra * 8 + half + cb], M[ra * 8 + cb]), rm[t]));
            for (int ra = 0; ra < half; ++ra) SY[ra] = add(SY[ra], mont_mul(sub(SY[half + ra], SY[ra]), rm[t]));
        }
        if (!weights) continue;
        F tmp[8];
        tmp[0] = one_m;
        int cur = 1;
        for (int t = 0; t < J; ++t) {
            const F nr = sub(one_m, rm[t]);
            for (int b = cur; b-- > 0;) {
                tmp[2 * b + 1] = mont_mul(tmp[b], rm[t]);
                tmp[2 * b] = mont_mul(tmp[b], nr);
            }
            cur <<= 1;
        }
        memcpy(weights + (size_t)k * w_row_words, tmp, sizeof(F) << J);
    }
}

// The HOST TAIL of a phase's product passes.  Once the tables are small (2^host_tail_log2 entries and fewer) a device pass is a
// latency chain -- launch, ~15 us of kernel for a few hundred products, the record's way back -- and costs more than the
// products do on one host core.  The last device pass of the phase therefore also leaves the three tables in pinned memory
// (k_prod_cross's `tail`), and the host does what the later passes' kernels would: binds the previous pass's variables
// (T'[i] = sum_b w_b T[b S + i], the weights in Montgomery form) and forms the next rounds' record (m[a][b] and the sub-block
// sums of Y, as k_prod_cross defines them) -- exact field arithmetic, the same canonical values.  W is in Montgomery form and
// stays so; X and Y are canonical.
// tables: [3][stride] (W, X, Y) of 2^m entries each, folded in place to 2^(m - jp); rec: the record's 72 values
void host_tail_pass_scalar(gkr::h64::F* tables, size_t stride, uint32_t m, uint32_t jp, const gkr::h64::F* weights, uint32_t J, gkr::h64::F* rec) {
    using namespace gkr::h64;
    const uint32_t mf = m - jp, len = 1u << mf;
    if (jp) {   // (sums of 2^jp products with one reduction each: wide_mac / wide_reduce, fr64.h)
        for (int t = 0; t < 3; ++t) {
            F* T = tables + (size_t)t * stride;
            for (uint32_t i = 0; i < len; ++i) {
                Wide acc = wide_zero();
                for (uint32_t b = 0; b < (1u << jp); ++b) wide_mac(acc, T[((size_t)b << mf) + i], weights[b]);
                T[i] = wide_reduce(acc);
            }
        }
    }
    const uint32_t nsub = 1u << J, S = len >> J;
    const F *W = tables, *X = tables + stride, *Y = tables + 2 * stride;
    for (uint32_t a = 0; a < nsub; ++a) {
        for (uint32_t b = 0; b < nsub; ++b) {
            Wide acc = wide_zero();
            for (uint32_t i = 0; i < S; ++i) wide_mac(acc, W[a * S + i], X[b * S + i]);
            rec[a * 8 + b] = wide_reduce(acc);
        }
        F y = Y[a * S];
        for (uint32_t i = 1; i < S; ++i) y = add(y, Y[a * S + i]);
        rec[64 + a] = y;
    }
}

// (eight products per instruction group where the CPU has AVX-512 IFMA: mimc_ifma.cpp, gkr_ifma_tail_pass -- the same values)
void host_tail_pass(gkr::h64::F* tables, size_t stride, uint32_t m, uint32_t jp, const gkr::h64::F* weights, uint32_t J, gkr::h64::F* rec) {
    if (host_ifma_ready())
        gkr::gkr_ifma_tail_pass(&tables[0].l[0], stride, m, jp, weights ? &weights[0].l[0] : nullptr, J, &rec[0].l[0]);
    else
        host_tail_pass_scalar(tables, stride, m, jp, weights, J, rec);
}

// ------------------------------------------------------------- gate lists
// smallest k_next whose layers take the lane-group gate passes of wide layers (kernels_wide.hip)
static bool layer_is_wide(gkr::GateSpan span, int k_i, int k) {
    const int wide_min_k = gkr::opt(gkr::OPT_gate_groups_min_k) >= 0 ? (int)gkr::opt(gkr::OPT_gate_groups_min_k) : (int)gkr::kWideMinK;
    return k >= wide_min_k && gkr::gate_segs_words(span, (uint32_t)k_i, (uint32_t)k) == 0;
}

// Queues the build of a span's lists (and, wide layers, of their item plan) from the device gate arrays into g: a circuit's
// cache, which owns its device allocations, or else pointers into the context's workspace.  *bad: the build's "a gate is out
// of range" word.  Nothing is waited for -- validate_gate_lists does that.
static int queue_gate_lists(gkr_ctx* ctx, gkr::GateSpan span, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r, bool wide,
                            GateLists* g, bool is_cache, uint32_t** bad) {
    hipStream_t s = ctx->stream;
    const size_t nb2 = (size_t)2 << k, list_words = 2 * gkr::gate_list_words(span.count);
    const size_t plan_words = wide ? gkr::gate_plan_words(span.count, (uint32_t)k) : 0, seg_words = gkr::gate_segs_words(span, (uint32_t)k_i, (uint32_t)k);
    uint32_t *counts = nullptr, *bsums = nullptr, *lds_scratch = nullptr, *seg_scratch = nullptr;
    WS(ctx, "pred.bad", uint32_t, 1, *bad);
    WS(ctx, "gates.counts", uint32_t, nb2, counts);
    WS(ctx, "gates.bsums", uint32_t, (nb2 + 2047) / 2048 + 1, bsums);
    if (is_cache) {
        if (!g->offsets) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&g->offsets), nb2 * sizeof(uint32_t)));
        if (!g->cursor) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&g->cursor), nb2 * sizeof(uint32_t)));
        if (!g->list) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&g->list), list_words * sizeof(uint32_t)));
        if (plan_words && !g->plan) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&g->plan), plan_words * sizeof(uint32_t)));
        if (seg_words && !g->segs.words) HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&g->segs.words), seg_words * sizeof(uint32_t)));
    } else {
        WS(ctx, "gates.offsets", uint32_t, nb2, g->offsets);
        WS(ctx, "gates.cursor", uint32_t, nb2, g->cursor);
        WS(ctx, "gates.list", uint32_t, list_words, g->list);
        if (plan_words) WS(ctx, "gates.plan", uint32_t, plan_words, g->plan);
        if (seg_words) WS(ctx, "gates.segs", uint32_t, seg_words, g->segs.words);
    }
    if (const size_t words = gkr::gate_lists_lds_scratch_words(span.count, (uint32_t)k)) WS(ctx, "gates.lds", uint32_t, words, lds_scratch);
    if (seg_words) WS(ctx, "gates.segscratch", uint32_t, gkr::gate_segs_scratch_words(span, (uint32_t)k_i, (uint32_t)k), seg_scratch);
    HIP_TRY(ctx, hipMemsetAsync(*bad, 0, 4, s));
    HIP_TRY(ctx, hipMemsetAsync(counts, 0, nb2 * sizeof(uint32_t), s));
    Timed t(ctx, "gate_lists", (double)span.count * (9.0 + 4 * 4.0));
    gkr::launch_gate_lists(span, (uint32_t)k_i, (uint32_t)k, d_gt, d_l, d_r, counts, g->offsets, g->cursor, bsums, g->list, *bad, lds_scratch, &g->segs, seg_scratch, s);
    if (wide) gkr::launch_gate_plan(span, (uint32_t)k, g->offsets, g->cursor, g->list, g->plan, s);
    return GKR_OK;
}

// Waits for a queued build and fails on a gate out of range.  A wide layer's cache also gets the counts the plan's build left
// in its two half headers (exact grids for the calls that find the lists cached).
static int validate_gate_lists(gkr_ctx* ctx, gkr::GateSpan span, int k, bool wide, const uint32_t* bad, GateLists* g, bool is_cache) {
    uint32_t hbad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    if (wide && is_cache) {
        size_t half1 = 0;
        gkr::gate_plan_counts_offsets(span.count, (uint32_t)k, &half1);
        HIP_TRY(ctx, hipMemcpyAsync(g->plan_counts.hdr[0], g->plan, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(g->plan_counts.hdr[1], g->plan + half1, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hbad) return ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range");
    g->plan_counts.known = wide && is_cache;
    return GKR_OK;
}

int build_cached_gate_lists(gkr_ctx* ctx, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r, GateLists* cached) {
    if (!cached) return ctx->fail(GKR_ERR_INVALID, "no list cache");
    if (cached->ready) return GKR_OK;
    const gkr::GateSpan span{0, (uint64_t)1 << k_i};
    if (gkr::gate_segs_words(span, (uint32_t)k_i, (uint32_t)k) != 0) return ctx->fail(GKR_ERR_INVALID, "a layer of the segment form's size in a lockstep group");
    const bool wide = layer_is_wide(span, k_i, k);
    uint32_t* bad = nullptr;
    if (const int rc = queue_gate_lists(ctx, span, k_i, k, d_gt, d_l, d_r, wide, cached, true, &bad)) return rc;
    if (const int rc = validate_gate_lists(ctx, span, k, wide, bad, cached, true)) return rc;
    cached->ready = true;
    return GKR_OK;
}

// ------------------------------------------------------------- layer sumcheck over gate lists (host transcript)
// The layer polynomial summed in time linear in the gates: no 2^{2k}-entry tables at all, U, V and the c-phase row come
// straight from the gates grouped by left / right operand (kernels.hip, k_gate_* / k_seg_*; kernels_wide.hip for wide layers),
// and the rounds run as product passes.  (The same transcript from the dense predicate tables: capi_layer_dense.hip.)
// What one run works on: the layer's shape, its gate lists and the proofs' device tables (2^k entries per proof each).
struct LayerRun {
    gkr_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    int batch = 0, k_i = 0, k = 0;
    size_t wlen = 0;   // 2^k
    gkr::GateSpan span{0, 0};
    // Wide layers (2^13 buckets and more per half, each with a few gates): the gate passes run with a group of lanes per
    // bucket and the rare long buckets in units (kernels_wide.hip) -- a block per bucket would be 2^20 blocks for a gate apiece.
    // The option gate_groups_min_k moves the switch (tests run the form on small layers too).
    bool wide = false;
    // where eq(z, g) is split into E_hi, E_lo: in the middle, or -- large layers, whose gate passes run over segments
    // of the sorted lists (gate_seg.h) -- where the segments are cut
    uint32_t kl = 0;
    const LayerShardArgs* shard = nullptr;
    const gkr::GateSet* sets = nullptr;   // lockstep group: per-proof gate lists
    const gkr::GatePlanCounts* plan_counts = nullptr;
    gkr::LayerBatch lb{};
    GateLists ws_lists;           // without a circuit's cache: lists in the context's workspace (nothing here owns or frees them)
    GateLists* g = nullptr;       // the cache, or ws_lists
    uint32_t* bad = nullptr;      // the word a list build of this call leaves its verdict on the gates in
    Fr *e_hi = nullptr, *e_lo = nullptr, *E = nullptr;   // eq(z, .): the two halves; wide layers up to 2^20 gates: as one table
    Fr *seg_partials = nullptr, *item_partials = nullptr;   // the segment passes' / the wide layers' item passes' scratch
    uint32_t* gate_arrive = nullptr;                        // ... and the items' combine step's arrival counters (zero between passes)
    Fr *Wb = nullptr, *Wc = nullptr, *U = nullptr, *V = nullptr, *eq = nullptr, *A = nullptr, *M = nullptr, *X = nullptr, *Y = nullptr;
    Fr* wu = nullptr;   // wide layer whose gates are all on this rank: W(u) per proof (the fused c-phase set-up)
    uint32_t* dep = nullptr;
    gkr::GateEq gate_eq() const { return gkr::GateEq{E, e_hi, e_lo, kl}; }
};

// The pinned buffers through which the host and the device hand a run's values to each other.
struct LayerPinned {
    gkr_fr* z = nullptr;     // the proofs' points, from which the device builds eq(z, .)
    uint32_t* dep = nullptr;   // which variables W depends on, per proof; the device leaves it there before round 0
    gkr_fr* u = nullptr;     // u = (r_1 .. r_k) of every proof, from which the device builds eq(u, .)
    gkr::ProdPassRec* prec = nullptr;   // a pass's record per proof
    Fr* pw = nullptr;        // the 2^J fold weights per proof the host derives from it (8 slots)
    Fr* tail = nullptr;      // the host tail's tables, 3 x tail_stride per proof (null: this run has no host tail)
    uint32_t tail_log2 = 0;
    size_t tail_stride() const { return (size_t)1 << tail_log2; }
};

static int alloc_layer_run(LayerRun& R, LayerPinned& P) {
    gkr_ctx* ctx = R.ctx;
    const size_t n = R.wlen * R.batch, batch = (size_t)R.batch;
    WS(ctx, "layer.Arow", Fr, n, R.A);
    WS(ctx, "layer.Mrow", Fr, n, R.M);
    WS(ctx, "layer.Wb", Fr, n, R.Wb);
    WS(ctx, "layer.Wc", Fr, n, R.Wc);
    WS(ctx, "layer.U", Fr, n, R.U);
    WS(ctx, "layer.V", Fr, n, R.V);
    WS(ctx, "layer.eq", Fr, n, R.eq);
    WS(ctx, "layer.X", Fr, n, R.X);
    WS(ctx, "layer.Y", Fr, n, R.Y);
    WS(ctx, "layer.dep", uint32_t, 32 * batch, R.dep);
    WS(ctx, "pred.ehi", Fr, batch << (R.k_i - (int)R.kl), R.e_hi);
    WS(ctx, "pred.elo", Fr, batch << R.kl, R.e_lo);
    if (const size_t pe = gkr::gate_seg_partial_elems(R.span, (uint32_t)R.k_i, (uint32_t)R.k)) WS(ctx, "gates.segpart", Fr, pe * batch, R.seg_partials);
    if (R.wide) {
        WS(ctx, "gates.itempart", Fr, gkr::gate_plan_partial_elems(R.span.count, (uint32_t)R.k) * batch, R.item_partials);
        // eq(z, g) for every gate index of the layer (of the whole layer also when this rank holds a share of the gates: the
        // lists carry indices relative to the share's first gate, the passes add it back), canonical
        if ((uint32_t)R.k_i <= gkr::kGateEqTableMaxKi) WS(ctx, "pred.E", Fr, batch << R.k_i, R.E);
        if (!R.shard) WS(ctx, "layer.wu", Fr, batch, R.wu);
    }
    HIP_TRY(ctx, ctx->pinned_host("pred.z", sizeof(gkr_fr) * batch * (R.k_i ? R.k_i : 1), reinterpret_cast<void**>(&P.z)));
    HIP_TRY(ctx, ctx->pinned_host("layer.hdep", sizeof(uint32_t) * 32 * batch, reinterpret_cast<void**>(&P.dep)));
    HIP_TRY(ctx, ctx->pinned_host("layer.u", sizeof(gkr_fr) * (size_t)R.k * batch, reinterpret_cast<void**>(&P.u)));
    HIP_TRY(ctx, ctx->pinned_host("layer.prec", sizeof(gkr::ProdPassRec) * batch, reinterpret_cast<void**>(&P.prec)));
    HIP_TRY(ctx, ctx->pinned_host("layer.pw", sizeof(Fr) * 8 * batch, reinterpret_cast<void**>(&P.pw)));
    // the host tail (host_tail_pass above): for batches of a few proofs -- where a step waits for its chain of hand-offs, not
    // for its hashing throughput -- the passes over tables of 2^tail_log2 entries and fewer run on the host
    const long long tail_opt = gkr::opt(gkr::OPT_host_tail_log2), tail_batch_opt = gkr::opt(gkr::OPT_host_tail_max_batch);
    P.tail_log2 = tail_opt < 0 ? 0u : tail_opt == 0 ? 6u : (uint32_t)(tail_opt > 12 ? 12 : tail_opt);
    if (P.tail_log2 >= 3u && R.batch <= (tail_batch_opt > 0 ? tail_batch_opt : 8))
        HIP_TRY(ctx, ctx->pinned_host("layer.tail", sizeof(Fr) * 3 * (batch << P.tail_log2), reinterpret_cast<void**>(&P.tail)));
    return GKR_OK;
}

// The sum over all ranks of a gate-sharded layer's two tables that are sums over gates.  One more element travels along:
// "some rank failed" (a bad gate seen on the device, or `local_fail`: this rank's own error status), so that every rank
// enters every collective and all of them leave with an error together instead of one leaving the others inside it.
struct RankExchange {
    gkr_ctx* ctx;
    const LayerShardArgs* shard;
    hipStream_t s;
    uint32_t* h_xflag = nullptr;   // device exchange: where the summed flag lands (pinned)
    int sums = 0;                  // exchanges entered

    // the two tables d_a, d_b (`each` elements) := their sums over all ranks
    int sum(Fr* d_a, Fr* d_b, size_t each, const uint32_t* d_flag, int local_fail) {
        ++sums;
        if (shard->dev) {
            // widen -> the caller's all-reduce on this stream -> narrow, no host copy and no synchronisation; the summed flag
            // lands in pinned memory and is looked at when the next record has landed (check)
            Timed t(ctx, "exchange", 0.0);
            long long* limbs = reinterpret_cast<long long*>(shard->dev->d_limbs);
            gkr::launch_exchange_widen(d_a, d_b, (uint32_t)each, d_flag, local_fail ? 1u : 0u, limbs, s);
            const int arc = shard->dev->fn(shard->dev->user, (2 * each + 1) * 8, static_cast<void*>(s));
            gkr::launch_exchange_narrow(limbs, d_a, d_b, (uint32_t)each, h_xflag, s);
            if (arc) return ctx->fail(GKR_ERR_INVALID, "the device sum-over-ranks hook failed (status " + std::to_string(arc) + ")");
            HIP_TRY(ctx, hipGetLastError());
            return local_fail;
        }
        const auto t0 = std::chrono::steady_clock::now();
        gkr_fr* buf = nullptr;   // pinned, kept by the context: no pageable staging vector per exchange
        HIP_TRY(ctx, ctx->pinned_host("layer.xbuf", sizeof(gkr_fr) * (2 * each + 1), reinterpret_cast<void**>(&buf)));
        uint32_t hflag = local_fail ? 1u : 0u;
        gkr::launch_copy_words(d_a, buf, each * 8, s);
        gkr::launch_copy_words(d_b, buf + each, each * 8, s);
        // (no early return between here and the hook: the peers are on their way into the collective)
        if (d_flag && !local_fail && hipMemcpyAsync(&hflag, d_flag, 4, hipMemcpyDeviceToHost, s) != hipSuccess) hflag = 1u;
        const hipError_t se = hipStreamSynchronize(s);
        if (se != hipSuccess) hflag = 1u;   // still enter the collective: the peers are on their way into it
        buf[2 * each] = gkr_fr{{(uint64_t)(hflag != 0), 0, 0, 0}};
        const int arc = shard->allreduce(shard->user, buf, 2 * each + 1);
        if (se != hipSuccess) return ctx->hip_fail(se, "hipStreamSynchronize before the sum over ranks");
        if (arc) return ctx->fail(GKR_ERR_INVALID, "the sum-over-ranks hook failed (status " + std::to_string(arc) + ")");
        if (!all_canonical(buf, 2 * each + 1)) return ctx->fail(GKR_ERR_NON_CANONICAL, "the sum-over-ranks hook returned a value >= r");
        const bool some_failed = (buf[2 * each].l[0] | buf[2 * each].l[1] | buf[2 * each].l[2] | buf[2 * each].l[3]) != 0;
        gkr::launch_copy_words(buf, d_a, each * 8, s);
        gkr::launch_copy_words(buf + each, d_b, each * 8, s);   // (the next exchange waits for the stream before it rewrites buf)
        if (ctx->profile == 1)
            ctx->add_host_sample("exchange", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (local_fail) return local_fail;
        if (some_failed) return ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range, or another failure, on some rank");
        return GKR_OK;
    }
    // device exchange: has the flag that travelled with the exchanges come back set?  Valid once a kernel queued after
    // the narrow step has published something the host waited for.
    bool flagged() const { return h_xflag && __atomic_load_n(h_xflag, __ATOMIC_ACQUIRE); }
    int check() const { return flagged() ? ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range, or another failure, on some rank") : GKR_OK; }
};

// All of b is bound: the rows of a, m at u = (r_1 .. r_k), then the c-phase's tables X = a_u + W(u) m_u, Y = W(u) a_u.
// W(u) is the last b pass's fold (weights P.pw) of what is left of Wb: 2^jp entries, in P.tail when wu_in_host_tail.
static int queue_c_phase_setup(LayerRun& R, const LayerPinned& P, RankExchange& xch, uint32_t jp, bool wu_in_host_tail, gkr_fr* const* out_r) {
    const uint32_t k = (uint32_t)R.k, k_i = (uint32_t)R.k_i, batch = (uint32_t)R.batch;
    for (uint32_t b = 0; b < batch; ++b) memcpy(P.u + (size_t)b * k, out_r[b], sizeof(gkr_fr) * k);
    // (a wide layer whose gates are all on this rank: the eq-table launch also leaves W(u), and the row pass writes the
    // c-phase's tables X, Y itself -- no k_prod_c_setup launch, no pass over the rows)
    const gkr::CPhaseFuse fuse{wu_in_host_tail ? P.tail : R.Wb, P.pw, R.X, R.Y, jp};
    gkr::launch_eq_table(reinterpret_cast<const Fr*>(P.u), k, 0u, k, R.eq, true, batch, R.s, R.wu ? &fuse : nullptr, R.wu,
                         (uint32_t)(wu_in_host_tail ? 3 * P.tail_stride() : R.wlen));
    bool c_tables_done = false;   // (one rank holds all gates: the row pass writes X, Y too)
    {
        Timed t(R.ctx, "gate_rows", (double)R.span.count * 8.0 * batch);
        if (R.wide) {
            const gkr::WideCFuse wfuse{R.wu, R.X, R.Y};
            gkr::launch_gate_rows_wide(R.span, k_i, k, R.g->plan, R.gate_eq(), R.eq, R.A, R.M, R.lb, R.item_partials, R.gate_arrive, R.s, R.sets, R.plan_counts,
                                       R.wu ? &wfuse : nullptr);
            c_tables_done = R.wu != nullptr;
        } else
            c_tables_done = gkr::launch_gate_rows(R.span, k_i, k, R.g->offsets, R.g->cursor, R.g->list, R.e_hi, R.e_lo, R.kl, R.eq, R.A, R.M, R.lb, &R.g->segs,
                                                  R.seg_partials, R.s, R.shard ? nullptr : &fuse, R.sets);
    }
    if (R.shard)   // every rank summed its own gates: the rows are complete after one exchange
        if (const int rc = xch.sum(R.A, R.M, R.wlen, nullptr, GKR_OK)) return rc;
    if (!c_tables_done) gkr::launch_prod_c_setup(R.Wb, jp, P.pw, R.A, R.M, R.X, R.Y, k, (uint32_t)R.wlen, batch, R.s);
    return GKR_OK;
}

// The host's share of one pass: J rounds of every proof from the pass's records (P.prec), `chunk` proofs per piece.
struct HostPass {
    const LayerPinned* pin;
    int batch, k;
    bool ifma;
    gkr_fr* const* out_coeffs;
    uint32_t* const* out_len;
    gkr_fr* const* out_r;
    // this pass: rounds round0 .. round0 + J - 1; on_host: the records come from the host tail, whose tables have 2^tail_m
    // entries with the previous pass's tail_jp variables still to bind
    uint32_t J, round0, tail_m, tail_jp;
    bool on_host;
    int chunk;
    std::atomic<int> next{0};
};

// claims and runs one piece; false: none left
static bool host_pass_piece(HostPass& hp) {
    const LayerPinned& P = *hp.pin;
    const int first = hp.next.fetch_add(hp.chunk, std::memory_order_relaxed);
    if (first >= hp.batch) return false;
    const int cnt = hp.batch - first < hp.chunk ? hp.batch - first : hp.chunk;
    uint64_t c2[gkr::kProdMaxJ][16][4], lin[gkr::kProdMaxJ][16][4], c0[gkr::kProdMaxJ][16][4], rr[gkr::kProdMaxJ][16][4];
    uint32_t vl[gkr::kProdMaxJ][16];
    const bool acct = accounting_on();
    const double tp0 = acct ? now_us_dbg() : 0.0;
    if (hp.on_host)   // (the weights of the previous pass are still in P.pw: the pass function below replaces them)
        for (int i = 0; i < cnt; ++i)
            host_tail_pass(reinterpret_cast<gkr::h64::F*>(P.tail + (size_t)(first + i) * 3 * P.tail_stride()), P.tail_stride(), hp.tail_m, hp.tail_jp,
                           reinterpret_cast<const gkr::h64::F*>(P.pw + (size_t)(first + i) * 8), hp.J, reinterpret_cast<gkr::h64::F*>(&P.prec[first + i].v[0]));
    for (uint32_t t = 0; t < hp.J; ++t)
        for (int i = 0; i < cnt; ++i) vl[t][i] = 2u + (P.dep[(size_t)(first + i) * 32 + (hp.round0 + t) % hp.k] ? 1u : 0u);
    (hp.ifma && cnt >= 3 ? gkr::gkr_ifma_prod_pass : host_prod_pass_scalar)(
        reinterpret_cast<const uint64_t*>(P.prec + first), sizeof(gkr::ProdPassRec) / 8, cnt, (int)hp.J, vl, c2, lin, c0, rr,
        reinterpret_cast<uint64_t*>(P.pw + (size_t)first * 8), 32);
    const double tp1 = acct ? now_us_dbg() : 0.0;
    for (int i = 0; i < cnt; ++i) {
        const int b = first + i;
        for (uint32_t t = 0; t < hp.J; ++t) {
            const uint32_t round = hp.round0 + t;
            gkr_fr* oc = hp.out_coeffs[b] + (size_t)round * 3;
            memset(&oc[0], 0, 32);
            if (vl[t][i] == 3) memcpy(&oc[0], c2[t][i], 32);
            memcpy(&oc[1], lin[t][i], 32);
            memcpy(&oc[2], c0[t][i], 32);
            hp.out_len[b][round] = vl[t][i];
            memcpy(&hp.out_r[b][round], rr[t][i], 32);
        }
    }
    if (acct) account_piece(cnt, tp1 - tp0, now_us_dbg() - tp0);
    return true;
}

// Product passes (kernels.hip): both phases as sumchecks of W X + Y over three small tables, up to three rounds per
// device round trip.  A pass: launch (or, in the host tail, nothing), wait for the records, look at the travelling flag,
// run the host's pieces, advance.
static int run_layer_passes(LayerRun& R, const LayerPinned& P, RankExchange& xch, gkr_fr* const* out_coeffs, uint32_t* const* out_len, gkr_fr* const* out_r) {
    gkr_ctx* ctx = R.ctx;
    const int batch = R.batch, k = R.k;
    Fr* d_ppart = nullptr;
    WS(ctx, "layer.ppart", Fr, (size_t)batch * gkr::prod_pass_scratch_values((uint32_t)k), d_ppart);
    unsigned char* d_fold_plans = nullptr;   // (wide layers: the later passes' pending folds on the matrix cores)
    if (k >= 14) WS(ctx, "layer.foldplans", unsigned char, (size_t)batch * gkr::prod_fold_plan_bytes(), d_fold_plans);
    // (passes of a few blocks per proof publish from their last block: one arrival counter per proof, zero between passes)
    uint32_t* d_arrivals = nullptr;
    if (!gkr::opt(gkr::OPT_no_fused_publish)) {
        WS(ctx, "layer.arrivals", uint32_t, (size_t)(batch < 4096 ? 4096 : batch), d_arrivals);   // (one size for every batch: zeroed once)
        if (ctx->arrivals_zeroed != d_arrivals) {
            HIP_TRY(ctx, hipMemsetAsync(d_arrivals, 0, sizeof(uint32_t) * (size_t)(batch < 4096 ? 4096 : batch), R.s));
            ctx->arrivals_zeroed = d_arrivals;
        }
    }
    gkr::SpinPool* pool = batch >= 16 ? ctx->host_pool() : nullptr;
    const bool ifma = host_ifma_ready();
    const bool dbg_sections = gkr::debug_timing();
    double us_launch = 0, us_wait = 0, us_pieces = 0, us_phase1 = 0;
    const double t_passes0 = dbg_sections ? now_us_dbg() : 0.0;
    gkr::SpinPool::Session session(pool, nullptr);
    uint32_t round0 = 0, jp = 0, tail_m = 0;   // tail_m: log2 of the host tables' length (before the pending fold), while the tail is active
    bool tail_active = false;
    int rc = GKR_OK;
    for (int phase = 0; phase < 2 && rc == GKR_OK; ++phase) {
        if (phase == 1) {
            // what is left of Wb -- the 2^jp entries the last pass's weights bind into W(u) -- is on the host when the b-phase ended in
            // the host tail.  The wide layers' fused set-up reads it where it is (pinned memory; one wave per proof); the other forms
            // get it back on the device by a copy KERNEL (a hipMemcpyAsync here cost ~25 us of the chain: the round path makes no
            // transfer call of the runtime).
            const bool wu_in_host_tail = tail_active && R.wu;
            if (tail_active && !wu_in_host_tail) gkr::launch_copy_rows(P.tail, 3 * P.tail_stride() * 8, R.Wb, R.wlen * 8, 8u << jp, (uint32_t)batch, R.s);
            const double t_ph1 = dbg_sections ? now_us_dbg() : 0.0;
            rc = queue_c_phase_setup(R, P, xch, jp, wu_in_host_tail, out_r);
            if (dbg_sections) us_phase1 += now_us_dbg() - t_ph1;
            if (rc) break;
            jp = 0;
            tail_active = false;
        }
        Fr *const Tw = phase ? R.Wc : R.Wb, *const Tx = phase ? R.X : R.U, *const Ty = phase ? R.Y : R.V;
        uint32_t m = (uint32_t)k;   // log2 of the tables' length before the pending fold
        for (uint32_t rem = (uint32_t)k; rem > 0 && rc == GKR_OK;) {
            // (the rounds that do not fill a pass of three come LAST.  First -- so that the pass over the whole table forms
            // 4^J = 4 or 16 cross sums per index instead of 64 -- was measured on wide layers and is slower: k = 20 0.61 ->
            // 0.80 ms of product passes per sumcheck, k = 22 1.44 -> 3.33: the second pass then folds into a table four or
            // two times larger and crosses THAT with J = 3.)
            const uint32_t J = rem < (uint32_t)gkr::kProdMaxJ ? rem : (uint32_t)gkr::kProdMaxJ;
            const bool on_host = tail_active;
            // (this pass exports the tables if they are small enough and a later pass of the phase is there to be saved)
            const bool exports = P.tail && !on_host && m - jp <= P.tail_log2 && rem > J;
            if (!on_host) {
                const uint32_t ticket = ++ctx->ticket;
                const double tl0 = dbg_sections ? now_us_dbg() : 0.0;
                {
                    Timed t(ctx, "layer_prod_pass", 0.0);
                    gkr::launch_prod_pass(Tw, Tx, Ty, m, jp, P.pw, J, d_ppart, (uint32_t)R.wlen, P.prec, ticket, (uint32_t)batch, R.s, d_arrivals, d_fold_plans,
                                          exports ? P.tail : nullptr, (uint32_t)P.tail_stride());
                }
                if (hipError_t le = hipGetLastError(); le != hipSuccess) {
                    rc = ctx->hip_fail(le, "launch of a layer pass");
                    break;
                }
                const double tl1 = dbg_sections ? now_us_dbg() : 0.0;
                rc = wait_records(ctx, P.prec, batch, ticket);
                if (dbg_sections) {
                    us_launch += tl1 - tl0;
                    us_wait += now_us_dbg() - tl1;
                }
                if (!rc) rc = xch.check();
                if (rc) break;
            }
            const int chunk = hash_chunk_size(batch, pool ? pool->workers() + 1 : 1, ctx->crew_member ? ctx->help_share : 0);
            HostPass hp{&P, batch, k, ifma, out_coeffs, out_len, out_r, J, round0, on_host ? tail_m : 0u, jp, on_host, chunk};
            const std::function<bool()> work = [&hp]() -> bool { return host_pass_piece(hp); };
            m -= jp;
            const double tw0 = dbg_sections ? now_us_dbg() : 0.0;
            run_pieces(pool, &work, batch > chunk, ctx->rounds_ahead + (int)(2 * k - round0));
            if (dbg_sections) us_pieces += now_us_dbg() - tw0;
            if (exports) tail_active = true;
            if (exports || on_host) tail_m = m;   // (the host's tables: 2^m entries, this pass's J variables pending)
            jp = J;
            round0 += J;
            rem -= J;
        }
    }
    session.close();
    if (dbg_sections)
        fprintf(stderr, "[gkr timing] layer k_i=%d k=%d batch=%d passes: %.0f us = launch calls %.0f + waiting for records %.0f + hashing pieces %.0f + c-phase set-up calls %.0f + other %.0f\n",
                R.k_i, k, batch, now_us_dbg() - t_passes0, us_launch, us_wait, us_pieces, us_phase1,
                now_us_dbg() - t_passes0 - us_launch - us_wait - us_pieces - us_phase1);
    return rc;
}

// `batch` layer sumchecks that share their gates (the same layer of `batch` proofs of one circuit) or, in a lockstep group,
// their shape; one rank's share of a layer split by gates (shard).  Arguments as run_layer_batch, which has checked them.
static int run_layer_gates(gkr_ctx* ctx, int batch, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r, const gkr_fr* z,
                           const Fr* d_W, gkr_fr* const* out_coeffs, uint32_t* const* out_len, gkr_fr* const* out_r, const LayerShardArgs* shard,
                           GateLists* cached, const LayerGroup* group) {
    hipStream_t s = ctx->stream;
    const bool lists_fresh = !(cached && cached->ready);   // the gate lists are built (and the gates validated) in this call
    LayerRun R{ctx, s, batch, k_i, k, (size_t)1 << k, gkr::GateSpan{shard ? shard->gate_base : 0, shard ? shard->gate_count : (uint64_t)1 << k_i}};
    LayerPinned P;
    R.wide = layer_is_wide(R.span, k_i, k);
    R.kl = gkr::gate_seg_shift(R.span, (uint32_t)k_i, (uint32_t)k);
    R.shard = shard;
    R.sets = group ? group->d_sets : nullptr;
    R.plan_counts = group ? &group->plan_counts : (lists_fresh ? nullptr : &cached->plan_counts);
    R.lb = gkr::LayerBatch{(uint32_t)batch, 0u, R.wlen, R.wlen};   // (pstride: the dense form's partial sums only)
    R.g = cached ? cached : &R.ws_lists;
    // (lists found ready are the circuit's from an earlier call, validated then)
    if (!lists_fresh && R.wide && !R.g->plan) return ctx->fail(GKR_ERR_INVALID, "cached gate lists were built without the wide layer's item plan");
    if (const int rc = alloc_layer_run(R, P)) return rc;
    // the eq tables of z (built on the device from the points in pinned memory), the Montgomery copies of W and the
    // dependence flags: one launch (k_layer_prologue)
    memcpy(P.z, z, sizeof(gkr_fr) * (size_t)batch * k_i);
    // (the dependence flags of a table beyond 2^13 values are found over a grid, not by the prologue's one block)
    const bool dep_wide = k > 13;
    uint32_t* dep_bits = nullptr;
    if (dep_wide) WS(ctx, "layer.depbits", uint32_t, (size_t)batch, dep_bits);
    gkr::launch_layer_prologue(reinterpret_cast<const Fr*>(P.z), (uint32_t)k_i, (uint32_t)k_i - R.kl, R.kl, R.e_hi, R.e_lo, d_W, R.Wb, R.Wc, (uint32_t)k,
                               dep_wide ? nullptr : R.dep, P.dep, (uint32_t)batch, s, dep_bits);
    // (the prologue's last block has stored what the table's first 256 entries show: a generic table's grid scan finds
    // every bit set and leaves at once)
    if (dep_wide) gkr::launch_depends_wide(d_W, (uint32_t)k, dep_bits, R.dep, P.dep, (uint32_t)batch, s, true);
    if (R.wide) {
        const size_t words = gkr::gate_plan_arrive_words(R.span.count, (uint32_t)k) * (size_t)batch;
        const size_t alloc = words < 4096 ? 4096 : words;   // (one size for the small cases: zeroed once)
        WS(ctx, "gates.arrive", uint32_t, alloc, R.gate_arrive);
        if (ctx->gate_arrive_zeroed != R.gate_arrive || words > 4096) {
            HIP_TRY(ctx, hipMemsetAsync(R.gate_arrive, 0, alloc * sizeof(uint32_t), s));
            ctx->gate_arrive_zeroed = R.gate_arrive;
        }
        if (R.E) {
            Timed t(ctx, "eq_table_z", ((double)batch * 32.0) * (double)((size_t)1 << k_i));
            gkr::launch_eq_outer(R.e_hi, R.e_lo, (uint32_t)k_i, R.kl, R.E, (uint32_t)batch, s);   // (the prologue above built the halves)
        }
    }
    if (lists_fresh) {
        if (const int rc = queue_gate_lists(ctx, R.span, k_i, k, d_gt, d_l, d_r, R.wide, R.g, cached != nullptr, &R.bad)) return rc;
        if (cached) cached->ready = true;   // a bad gate fails the call below and the prepared circuit is dropped
    }
    {
        Timed t(ctx, "gate_uv", (double)R.span.count * 8.0 * batch);   // HBM: the 8-byte list entry per gate (operands are L2 gathers)
        if (R.wide)
            gkr::launch_gate_uv_wide(R.span, (uint32_t)k_i, (uint32_t)k, R.g->plan, R.gate_eq(), R.Wc, R.U, R.V, R.lb, R.item_partials, R.gate_arrive, s, R.sets, R.plan_counts);
        else
            gkr::launch_gate_uv(R.span, (uint32_t)k_i, (uint32_t)k, R.g->offsets, R.g->cursor, R.g->list, R.e_hi, R.e_lo, R.kl, R.Wc, R.U, R.V, R.lb, &R.g->segs, R.seg_partials, s, R.sets);
    }
    RankExchange xch{ctx, shard, s};
    if (shard && shard->dev) {
        HIP_TRY(ctx, ctx->pinned_host("layer.xflag", 64, reinterpret_cast<void**>(&xch.h_xflag)));
        *xch.h_xflag = 0;
    }
    if (shard)
        if (const int rc = xch.sum(R.U, R.V, R.wlen, lists_fresh ? R.bad : nullptr, GKR_OK)) return rc;
    // Lists found in the circuit cache were validated when they were built.  Gate-sharded with the device exchange: the flag
    // travels with the first exchange and is looked at after the first round's record, on every rank alike -- a rank that left
    // here would leave its peers inside a collective.
    // (P.dep is read when round 0 is hashed, i.e. after a LATER kernel of this stream has released that round's record: the
    // prologue launch wrote it)
    if (lists_fresh && !(shard && shard->dev))
        if (const int rc = validate_gate_lists(ctx, R.span, k, R.wide, R.bad, R.g, cached != nullptr)) return rc;
    int rc = run_layer_passes(R, P, xch, out_coeffs, out_len, out_r);
    // a rank that failed between the exchanges still enters the second one (flag set): its peers are waiting in it.
    // (Not when the failure is the travelling flag itself: then every rank is leaving at this very point.)
    if (rc && shard && xch.sums == 1 && !xch.flagged()) (void)xch.sum(R.A, R.M, R.wlen, nullptr, rc);
    if (rc) {
        (void)hipStreamSynchronize(s);
        ctx->arrivals_zeroed = nullptr;   // (a pass that was given up may have left its counters half way)
        return rc;
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if ((rc = xch.check())) return rc;
    ctx->drain_events();
    return GKR_OK;
}

// z: batch x k_i challenges (host); d_W: batch tables of 2^k canonical values; outputs: per proof 2k rows (out_coeffs 3 slots
// per row), laid out [proof][round].  shard, group: capi_internal.h.  Argument checks come before anything is queued: a rank
// that returns here has not left its peers inside a collective -- the same arguments fail on every rank.
// Gate lists that this call built (cached->ready false on entry) count as ready only if the whole call succeeded: a bad
// gate, a HIP error or a timeout after the sort was queued must not leave half-validated lists marked usable.
int run_layer_batch(gkr_ctx* ctx, int batch, int k_i, int k, const uint8_t* d_gt, const uint32_t* d_l, const uint32_t* d_r,
                    const gkr_fr* z, const Fr* d_W, gkr_fr* const* out_coeffs, uint32_t* const* out_len, gkr_fr* const* out_r,
                    const LayerShardArgs* shard, GateLists* cached, const LayerGroup* group) {
    const bool was_ready = cached && cached->ready, host_tx = ctx->transcript == GKR_TRANSCRIPT_HOST;
    if (group && (!host_tx || shard || !was_ready)) return ctx->fail(GKR_ERR_INVALID, "a lockstep group needs the host transcript and prepared gate lists");
    if (k < 1) return ctx->fail(GKR_ERR_DEGENERATE, "k_next == 0: v = 0 underflows in the reference (sumcheck.rs:49)");
    if (shard && (!host_tx || batch != 1)) return ctx->fail(GKR_ERR_INVALID, "a gate-sharded layer needs the host transcript and one proof");
    if (shard && shard->dev && (shard->dev->capacity < gkr_exchange_limbs(k) || !shard->dev->d_limbs || !shard->dev->fn))
        return ctx->fail(GKR_ERR_INVALID, "the exchange buffer is smaller than gkr_exchange_limbs(k_next) int64");
    if (k > kMaxLayerK || k_i > kMaxLayerKi) return ctx->fail(GKR_ERR_INVALID, "layer wider than the library's limits (gkr_amd.h: GKR_MAX_K_NEXT, GKR_MAX_K_I)");
    const int rc = host_tx ? run_layer_gates(ctx, batch, k_i, k, d_gt, d_l, d_r, z, d_W, out_coeffs, out_len, out_r, shard, cached, group)
                           : run_layer_dense(ctx, batch, k_i, k, d_gt, d_l, d_r, z, d_W, out_coeffs, out_len, out_r);
    if (rc && cached && !was_ready) cached->ready = false;
    return rc;
}

int upload_gates(gkr_ctx* ctx, size_t gates, const uint8_t* gt, const uint32_t* l, const uint32_t* r,
                 DevBuf<uint8_t>& dgt, DevBuf<uint32_t>& dl, DevBuf<uint32_t>& dr) {
    HIP_TRY(ctx, dgt.alloc(gates));
    HIP_TRY(ctx, dl.alloc(gates));
    HIP_TRY(ctx, dr.alloc(gates));
    HIP_TRY(ctx, hipMemcpyAsync(dgt.p, gt, gates, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dl.p, l, gates * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dr.p, r, gates * 4, hipMemcpyHostToDevice, ctx->stream));
    return GKR_OK;
}

int check_layer_args(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gt, const uint32_t* l, const uint32_t* r,
                     const gkr_fr* z) {
    if (!gt || !l || !r || (k_i > 0 && !z)) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (k_i < 0 || k_i > 28) return ctx->fail(GKR_ERR_INVALID, "k_i must be in [0, 28]");
    if (k_next == 0) return ctx->fail(GKR_ERR_DEGENERATE, "k_next == 0: v = 0 underflows in the reference (sumcheck.rs:49)");
    if (k_next < 0 || k_next > kMaxLayerK || k_i > kMaxLayerKi) return ctx->fail(GKR_ERR_INVALID, "k_next must be in [1, GKR_MAX_K_NEXT], k_i in [0, GKR_MAX_K_I]");
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    // every gate is validated on the device by the scatter kernel; small layers are also checked here
    // so that the error names the cause
    const size_t gates = (size_t)1 << k_i;
    for (size_t g = 0; g < gates && gates <= ((size_t)1 << 16); ++g) {
        if (gt[g] > 1) return ctx->fail(GKR_ERR_INVALID, "gate_type must be 0 (add) or 1 (mult)");
        if ((l[g] >> k_next) || (r[g] >> k_next)) return ctx->fail(GKR_ERR_INVALID, "gate operand index out of range");
    }
    return GKR_OK;
}

}  // namespace gkr_host

extern "C" {

int gkr_sumcheck_layer(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gate_type, const uint32_t* left,
                       const uint32_t* right, const gkr_fr* z, const gkr_fr* W, gkr_fr* out_coeffs, uint32_t* out_len,
                       gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!W || !out_coeffs || !out_len || !out_r) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    int rc = check_layer_args(ctx, k_i, k_next, gate_type, left, right, z);
    if (rc) return rc;
    if (!all_canonical(W, (size_t)1 << k_next)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    GKR_ENTER(ctx);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> dW;
    rc = upload_gates(ctx, (size_t)1 << k_i, gate_type, left, right, dgt, dl, dr);
    if (rc) return rc;
    HIP_TRY(ctx, dW.alloc((size_t)1 << k_next));
    HIP_TRY(ctx, hipMemcpyAsync(dW.p, W, sizeof(Fr) << k_next, hipMemcpyHostToDevice, ctx->stream));
    return run_layer_batch(ctx, 1, k_i, k_next, dgt.p, dl.p, dr.p, z, dW.p, &out_coeffs, &out_len, &out_r);
}

// What the list build of a whole layer decides (tests pin the thresholds of the gate passes on it): the build that
// run_layer_gates queues, into lists of their own as a circuit's cache holds them, and the counts it left.
int gkr_devtest_gate_plan(gkr_ctx* ctx, int k_i, int k_next, const uint8_t* gate_type, const uint32_t* left, const uint32_t* right,
                          uint32_t* form, uint32_t* counts) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!gate_type || !left || !right || !form || !counts) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (k_i < 0 || k_i > kMaxLayerKi || k_next < 1 || k_next > kMaxLayerK)
        return ctx->fail(GKR_ERR_INVALID, "k_next must be in [1, GKR_MAX_K_NEXT], k_i in [0, GKR_MAX_K_I]");
    GKR_ENTER(ctx);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    int rc = upload_gates(ctx, (size_t)1 << k_i, gate_type, left, right, dgt, dl, dr);
    if (rc) return rc;
    const gkr::GateSpan span{0, (uint64_t)1 << k_i};
    const bool wide = layer_is_wide(span, k_i, k_next);
    GateLists g;
    uint32_t* bad = nullptr;
    uint32_t seg_items[2] = {0, 0};
    rc = queue_gate_lists(ctx, span, k_i, k_next, dgt.p, dl.p, dr.p, wide, &g, true, &bad);
    if (!rc) rc = validate_gate_lists(ctx, span, k_next, wide, bad, &g, true);
    if (!rc && g.segs.shift) {
        uint32_t ends[2] = {0, 0};   // the items before the second half's first bucket, and all of them
        const hipError_t e0 = hipMemcpy(&ends[0], g.segs.bucket_begin() + g.segs.nb, 4, hipMemcpyDeviceToHost);
        const hipError_t e1 = hipMemcpy(&ends[1], g.segs.bucket_begin() + 2 * (size_t)g.segs.nb, 4, hipMemcpyDeviceToHost);
        if (e0 != hipSuccess || e1 != hipSuccess) rc = ctx->hip_fail(e0 != hipSuccess ? e0 : e1, "reading the segments' item counts");
        seg_items[0] = ends[0];
        seg_items[1] = ends[1] - ends[0];
    }
    memset(counts, 0, 16 * sizeof(uint32_t));
    if (!rc) {
        *form = g.segs.shift ? 2u : wide ? 1u : 0u;
        for (int half = 0; half < 2; ++half) {
            uint32_t* c = counts + 8 * half;
            if (g.segs.shift) {
                c[0] = g.segs.shift;
                c[1] = g.segs.runs;
                c[2] = (uint32_t)((((uint64_t)1 << g.segs.shift) * gkr::gate_lists_lds_blocks(span.count, (uint32_t)k_next)) >> k_i);
                c[3] = seg_items[half];
            } else if (wide) {
                for (int w = 0; w < 6; ++w) c[w] = g.plan_counts.hdr[half][w];
            }
        }
    }
    (void)hipStreamSynchronize(ctx->stream);
    g.release();
    return rc;
}

int gkr_sumcheck_layer_sharded(gkr_ctx* ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count,
                               const uint8_t* gate_type, const uint32_t* left, const uint32_t* right, const gkr_fr* z,
                               const gkr_fr* W, gkr_allreduce_fn allreduce, void* user, gkr_fr* out_coeffs, uint32_t* out_len,
                               gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!W || !out_coeffs || !out_len || !out_r || !allreduce || (k_i > 0 && !z)) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (gate_count && (!gate_type || !left || !right)) return ctx->fail(GKR_ERR_INVALID, "null gate array");
    if (k_i < 0 || k_i > 28) return ctx->fail(GKR_ERR_INVALID, "k_i must be in [0, 28]");
    if (k_next == 0) return ctx->fail(GKR_ERR_DEGENERATE, "k_next == 0: v = 0 underflows in the reference (sumcheck.rs:49)");
    if (k_next < 0 || k_next > kMaxLayerK) return ctx->fail(GKR_ERR_INVALID, "k_next must be in [1, GKR_MAX_K_NEXT]");
    if (gate_first + gate_count > ((uint64_t)1 << k_i)) return ctx->fail(GKR_ERR_INVALID, "gate range exceeds the layer's 2^k_i gates");
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    if (!all_canonical(W, (size_t)1 << k_next)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    // gates are validated on the device (k_gate_count); a bad one fails every rank through the first exchange
    GKR_ENTER(ctx);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> dW;
    const size_t n_alloc = gate_count ? (size_t)gate_count : 1;
    HIP_TRY(ctx, dgt.alloc(n_alloc));
    HIP_TRY(ctx, dl.alloc(n_alloc));
    HIP_TRY(ctx, dr.alloc(n_alloc));
    if (gate_count) {
        HIP_TRY(ctx, hipMemcpyAsync(dgt.p, gate_type, gate_count, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dl.p, left, gate_count * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dr.p, right, gate_count * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, dW.alloc((size_t)1 << k_next));
    HIP_TRY(ctx, hipMemcpyAsync(dW.p, W, sizeof(Fr) << k_next, hipMemcpyHostToDevice, ctx->stream));
    const LayerShardArgs sh{gate_first, gate_count, allreduce, user};
    return run_layer_batch(ctx, 1, k_i, k_next, dgt.p, dl.p, dr.p, z, dW.p, &out_coeffs, &out_len, &out_r, &sh);
}

int gkr_sumcheck_layer_device(gkr_ctx* ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count, const void* d_gate_type,
                              const void* d_left, const void* d_right, const gkr_fr* z, const gkr_fr* W, gkr_allreduce_fn allreduce,
                              void* user, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!W || !out_coeffs || !out_len || !out_r || (k_i > 0 && !z)) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (!d_gate_type || !d_left || !d_right) return ctx->fail(GKR_ERR_INVALID, "null device gate array");
    if (k_i < 0 || k_i > 28) return ctx->fail(GKR_ERR_INVALID, "k_i must be in [0, 28]");
    if (k_next == 0) return ctx->fail(GKR_ERR_DEGENERATE, "k_next == 0: v = 0 underflows in the reference (sumcheck.rs:49)");
    if (k_next < 0 || k_next > (allreduce ? 13 : 14)) return ctx->fail(GKR_ERR_INVALID, "k_next out of range");
    if (gate_first + gate_count > ((uint64_t)1 << k_i)) return ctx->fail(GKR_ERR_INVALID, "gate range exceeds the layer's 2^k_i gates");
    if (!allreduce && (gate_first != 0 || gate_count != ((uint64_t)1 << k_i)))
        return ctx->fail(GKR_ERR_INVALID, "without an exchange hook the arrays must hold the whole layer");
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    if (!all_canonical(W, (size_t)1 << k_next)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    GKR_ENTER(ctx);
    Fr* dW = nullptr;
    HIP_TRY(ctx, ctx->workspace("layer.Win", sizeof(Fr) << k_next, reinterpret_cast<void**>(&dW)));
    HIP_TRY(ctx, hipMemcpyAsync(dW, W, sizeof(Fr) << k_next, hipMemcpyHostToDevice, ctx->stream));
    const uint8_t* gt = static_cast<const uint8_t*>(d_gate_type);
    const uint32_t* dl = static_cast<const uint32_t*>(d_left);
    const uint32_t* dr = static_cast<const uint32_t*>(d_right);
    const LayerShardArgs sh{gate_first, gate_count, allreduce, user};
    return run_layer_batch(ctx, 1, k_i, k_next, gt, dl, dr, z, dW, &out_coeffs, &out_len, &out_r, allreduce ? &sh : nullptr);
}

struct gkr_resident_layer {
    int k_i = 0, k = 0;
    uint64_t first = 0, count = 0;
    uint8_t* gt = nullptr;
    uint32_t *l = nullptr, *r = nullptr;
    GateLists lists;
};

void gkr_resident_layer_free(gkr_ctx* ctx, gkr_resident_layer* layer) {
    if (!layer) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (layer->gt) (void)hipFree(layer->gt);
    if (layer->l) (void)hipFree(layer->l);
    if (layer->r) (void)hipFree(layer->r);
    layer->lists.release();
    delete layer;
}

int gkr_resident_layer_create(gkr_ctx* ctx, int k_i, int k_next, uint64_t gate_first, uint64_t gate_count, const uint8_t* gate_type,
                              const uint32_t* left, const uint32_t* right, gkr_resident_layer** out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!out) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    *out = nullptr;
    if ((!gate_type || !left || !right) && gate_count) return ctx->fail(GKR_ERR_INVALID, "null gate array");
    if (k_i < 0 || k_i > 28) return ctx->fail(GKR_ERR_INVALID, "k_i must be in [0, 28]");
    if (k_next == 0) return ctx->fail(GKR_ERR_DEGENERATE, "k_next == 0: v = 0 underflows in the reference (sumcheck.rs:49)");
    if (k_next < 0 || k_next > kMaxLayerK || k_i > kMaxLayerKi) return ctx->fail(GKR_ERR_INVALID, "k_next must be in [1, GKR_MAX_K_NEXT], k_i in [0, GKR_MAX_K_I]");
    if (gate_first + gate_count > ((uint64_t)1 << k_i)) return ctx->fail(GKR_ERR_INVALID, "gate range exceeds the layer's 2^k_i gates");
    GKR_ENTER(ctx);
    std::unique_ptr<gkr_resident_layer, void (*)(gkr_resident_layer*)> L(new gkr_resident_layer(), [](gkr_resident_layer* p) {
        gkr_resident_layer_free(nullptr, p);
    });
    L->k_i = k_i;
    L->k = k_next;
    L->first = gate_first;
    L->count = gate_count;
    const size_t n = gate_count ? (size_t)gate_count : 1;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&L->gt), n));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&L->l), n * 4));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&L->r), n * 4));
    if (gate_count) {
        HIP_TRY(ctx, hipMemcpy(L->gt, gate_type, gate_count, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(L->l, left, gate_count * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(L->r, right, gate_count * 4, hipMemcpyHostToDevice));
    }
    *out = L.release();
    return GKR_OK;
}

// A layer's W from host memory into the context's workspace, validated (every entry < r, sumcheck.rs:16,21 unwrap()s): small
// tables through pinned memory and a copy kernel (no transfer call on a small proof's path, see k_copy_words), tables of 2^16
// entries and more by the copy engine with the check on the device -- the host loop and the staging copy of a 2^20-entry W
// took longer than the layer's gate passes.
static int upload_W(gkr_ctx* ctx, const gkr_fr* W, int k, Fr** out) {
    const size_t n = (size_t)1 << k;
    Fr* dW = nullptr;
    HIP_TRY(ctx, ctx->workspace("layer.Win", sizeof(Fr) << k, reinterpret_cast<void**>(&dW)));
    if (k < 16) {
        if (!all_canonical(W, n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
        gkr_fr* hW = nullptr;
        HIP_TRY(ctx, ctx->pinned_host("layer.hWin", sizeof(gkr_fr) << k, reinterpret_cast<void**>(&hW)));
        memcpy(hW, W, sizeof(gkr_fr) << k);
        gkr::launch_copy_words(hW, dW, ((size_t)8) << k, ctx->stream);
    } else {
        uint32_t* d_flag = nullptr;
        WS(ctx, "layer.Wflag", uint32_t, 1, d_flag);
        uint32_t hflag = 0;
        HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dW, W, sizeof(Fr) << k, hipMemcpyHostToDevice, ctx->stream));
        gkr::launch_check_canonical(dW, n, d_flag, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(&hflag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (hflag) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    }
    *out = dW;
    return GKR_OK;
}

int gkr_resident_layer_sumcheck(gkr_ctx* ctx, gkr_resident_layer* layer, const gkr_fr* z, const gkr_fr* W, gkr_allreduce_fn allreduce,
                                void* user, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!layer || !W || !out_coeffs || !out_len || !out_r || (layer->k_i > 0 && !z)) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    const int k_i = layer->k_i, k = layer->k;
    if (!allreduce && (layer->first != 0 || layer->count != ((uint64_t)1 << k_i)))
        return ctx->fail(GKR_ERR_INVALID, "without an exchange hook the layer must be whole");
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    Fr* dW = nullptr;
    if (const int urc = upload_W(ctx, W, k, &dW)) return urc;
    const LayerShardArgs sh{layer->first, layer->count, allreduce, user};
    const int rc = run_layer_batch(ctx, 1, k_i, k, layer->gt, layer->l, layer->r, z, dW, &out_coeffs, &out_len, &out_r, allreduce ? &sh : nullptr,
                                   &layer->lists);
    if (rc) layer->lists.ready = false;   // a failed first use may have left half-built lists behind
    return rc;
}

// gkr_resident_layer_sumcheck with W ALREADY in device memory (inside prover::prove the next layer's values come from the
// forward evaluation, prover.rs:38-43: they never were host data; a host that drives prove_sumcheck_opt itself keeps them on
// the device the same way): nothing but z and the transcript crosses PCIe.  W is checked where it lies; the status of that
// check is looked at after the sumcheck (no synchronisation before it).
int gkr_resident_layer_sumcheck_wdev(gkr_ctx* ctx, gkr_resident_layer* layer, const gkr_fr* z, const void* d_W, gkr_fr* out_coeffs, uint32_t* out_len,
                                     gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!layer || !d_W || !out_coeffs || !out_len || !out_r || (layer->k_i > 0 && !z)) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    const int k_i = layer->k_i, k = layer->k;
    if (layer->first != 0 || layer->count != ((uint64_t)1 << k_i)) return ctx->fail(GKR_ERR_INVALID, "the layer must be whole");
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    uint32_t* d_flag = nullptr;
    uint32_t* h_flag = nullptr;
    WS(ctx, "layer.Wflag", uint32_t, 1, d_flag);
    HIP_TRY(ctx, ctx->pinned_host("layer.hWflag", 64, reinterpret_cast<void**>(&h_flag)));
    *h_flag = 0;
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, 4, ctx->stream));
    gkr::launch_check_canonical(static_cast<const Fr*>(d_W), (size_t)1 << k, d_flag, ctx->stream);
    gkr::launch_copy_words(d_flag, h_flag, 1, ctx->stream);
    const int rc = run_layer_batch(ctx, 1, k_i, k, layer->gt, layer->l, layer->r, z, static_cast<const Fr*>(d_W), &out_coeffs, &out_len, &out_r, nullptr,
                                   &layer->lists);
    if (rc) {
        layer->lists.ready = false;
        return rc;
    }
    if (__atomic_load_n(h_flag, __ATOMIC_ACQUIRE)) return ctx->fail(GKR_ERR_NON_CANONICAL, "W entry >= r");
    return GKR_OK;
}

size_t gkr_exchange_limbs(int k_next) {
    if (k_next < 0 || k_next > kMaxLayerK) return 0;
    return (((size_t)2 << k_next) + 1) * 8;
}

int gkr_resident_layer_sumcheck_dev(gkr_ctx* ctx, gkr_resident_layer* layer, const gkr_fr* z, const gkr_fr* W, const gkr_exchange_dev* exchange,
                                    gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!layer || !W || !out_coeffs || !out_len || !out_r || (layer->k_i > 0 && !z) || !exchange) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    const int k_i = layer->k_i, k = layer->k;
    if (k_i > 0 && !all_canonical(z, k_i)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    GKR_ENTER(ctx);
    Fr* dW = nullptr;
    if (const int urc = upload_W(ctx, W, k, &dW)) return urc;
    const LayerShardArgs sh{layer->first, layer->count, nullptr, nullptr, exchange};
    const int rc = run_layer_batch(ctx, 1, k_i, k, layer->gt, layer->l, layer->r, z, dW, &out_coeffs, &out_len, &out_r, &sh, &layer->lists);
    if (rc) layer->lists.ready = false;
    return rc;
}

int gkr_fr_widen(const gkr_fr* values, size_t count, int64_t* limbs) {
    if ((!values || !limbs) && count) return GKR_ERR_INVALID;
    for (size_t i = 0; i < count; ++i)
        for (int j = 0; j < 4; ++j) {
            limbs[8 * i + 2 * j] = (int64_t)(values[i].l[j] & 0xffffffffull);
            limbs[8 * i + 2 * j + 1] = (int64_t)(values[i].l[j] >> 32);
        }
    return GKR_OK;
}

int gkr_fr_narrow(const int64_t* limbs, size_t count, gkr_fr* values) {
    if ((!values || !limbs) && count) return GKR_ERR_INVALID;
    for (size_t i = 0; i < count; ++i) {
        gkr::Acc<10> a = gkr::acc_zero<10>();
        uint64_t carry = 0;
        for (int j = 0; j < 8; ++j) {
            if (limbs[8 * i + j] < 0) return GKR_ERR_INVALID;
            const uint64_t w = (uint64_t)limbs[8 * i + j];
            const uint64_t lo = (w & 0xffffffffull) + (carry & 0xffffffffull);
            a.l[j] = (uint32_t)lo;
            carry = (w >> 32) + (carry >> 32) + (lo >> 32);
        }
        a.l[8] = (uint32_t)carry;
        a.l[9] = (uint32_t)(carry >> 32);
        values[i] = to_abi(gkr::acc_reduce(a));
    }
    return GKR_OK;
}

int gkr_layer_eval(gkr_ctx* ctx, size_t gates, const uint8_t* gate_type, const uint32_t* left, const uint32_t* right,
                   const gkr_fr* prev, size_t n_prev, gkr_fr* out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!gate_type || !left || !right || !prev || !out || !gates || !n_prev || gates > ((size_t)1 << 30))
        return ctx->fail(GKR_ERR_INVALID, "null pointer or empty layer");
    for (size_t g = 0; g < gates; ++g)
        if (gate_type[g] > 1 || left[g] >= n_prev || right[g] >= n_prev)
            return ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range");
    if (!all_canonical(prev, n_prev)) return ctx->fail(GKR_ERR_NON_CANONICAL, "prev entry >= r");
    GKR_ENTER(ctx);
    DevBuf<uint8_t> dgt;
    DevBuf<uint32_t> dl, dr;
    DevBuf<Fr> dprev, dout;
    int rc = upload_gates(ctx, gates, gate_type, left, right, dgt, dl, dr);
    if (rc) return rc;
    HIP_TRY(ctx, dprev.alloc(n_prev));
    HIP_TRY(ctx, dout.alloc(gates));
    HIP_TRY(ctx, hipMemcpyAsync(dprev.p, prev, n_prev * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    gkr::launch_layer_eval((uint32_t)gates, dgt.p, dl.p, dr.p, dprev.p, dout.p, 1, 0, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, dout.p, gates * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

}  // extern "C"

// The plain multilinear sumcheck (prove_sumcheck, rust/src/gkr/sumcheck.rs:158-214) on the multi-round schedule with the host
// transcript: the tables of a run and THE pass launcher, the schedule of a batch, the driver of whole tables (run_mle_batch_passes)
// and of one table split over ranks (gkr_sumcheck_mle_sharded_dev).  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// ------------------------------------------------------------- plain MLE sumcheck, multi-round passes
// The host's share of one multi-round pass, scalar form (the IFMA-lane form is gkr_ifma_pass, mimc_ifma.cpp; same
// arguments, same results): per lane k and round t the round polynomial's coefficients from the sub-block sums, the
// vector's length, the challenge, then the sums with that variable bound; at the end the 2^J weights of the fold pass
// that binds the J variables, w_b = prod_t (bit_t(b) ? r_t : 1 - r_t), bit_0 = most significant, Montgomery form.
void host_pass_scalar(const uint64_t* sums, size_t sums_row_words, int count, int J, const uint32_t* final_len,
                             uint64_t (*c0)[16][4], uint64_t (*c1)[16][4], uint64_t (*r)[16][4], uint32_t (*len)[16],
                             uint64_t* weights, size_t w_row_words) {
    using gkr::h64::F;
    const F* cts = host_mimc_constants64();
    const F one_m = gkr::h64::to_mont(F{{1, 0, 0, 0}});
    for (int k = 0; k < count; ++k) {
        F S[gkr::kMleMaxSub], rm[gkr::kMlePassMaxRounds];
        memcpy(S, sums + (size_t)k * sums_row_words, sizeof(F) << J);
        for (int t = 0; t < J; ++t) {
            const int half = 1 << (J - t - 1);
            F lo = S[0], hi = S[half];
            for (int b = 1; b < half; ++b) {
                lo = gkr::h64::add(lo, S[b]);
                hi = gkr::h64::add(hi, S[half + b]);
            }
            const F d = gkr::h64::sub(hi, lo);
            const uint32_t ln = (final_len && t == J - 1) ? final_len[k] : (gkr::h64::is_zero(d) ? 1u : 2u);
            const F vec[2] = {d, lo};
            const F rc = host_multi_hash(vec + (2 - ln), (int)ln, cts);
            memcpy(c0[t][k], &lo, 32);
            memcpy(c1[t][k], &d, 32);
            memcpy(r[t][k], &rc, 32);
            len[t][k] = ln;
            rm[t] = gkr::h64::to_mont(rc);
            for (int b = 0; b < half; ++b) S[b] = gkr::h64::add(S[b], gkr::h64::mont_mul(gkr::h64::sub(S[half + b], S[b]), rm[t]));
        }
        if (!weights) continue;
        F* w = reinterpret_cast<F*>(weights + (size_t)k * w_row_words);
        F tmp[gkr::kMleMaxSub];
        tmp[0] = one_m;
        int cur = 1;
        for (int t = 0; t < J; ++t) {
            const F nr = gkr::h64::sub(one_m, rm[t]);
            for (int b = cur; b-- > 0;) {
                tmp[2 * b + 1] = gkr::h64::mont_mul(tmp[b], rm[t]);
                tmp[2 * b] = gkr::h64::mont_mul(tmp[b], nr);
            }
            cur <<= 1;
        }
        memcpy(w, tmp, sizeof(F) << J);
    }
}

// ------------------------------------------------------------- the tables a run's passes work on, and THE pass launcher
struct MlePassTables {
    const Fr* input = nullptr;   // the caller's tables, in_stride = 2^n entries apart: pass 0 and the first fold read them
    size_t in_stride = 0;
    Fr* work = nullptr;          // every fold's output, work_len entries (the first folded table) apart
    size_t work_len = 0;
    gkr::MleSubPartial* partials = nullptr;
    unsigned char* plans = nullptr;        // per sumcheck: the digit matrix of the matrix-core fold pass
    Fr* h_w = nullptr;                     // pinned: up to 32 Montgomery weights per sumcheck
    Fr *h_w2 = nullptr, *d_w2 = nullptr;   // the two-level first fold: the weights of rounds 6-10 as the host writes them (pinned), and on the device
    gkr::MleHostRecSub* h_rec = nullptr;   // pinned: the records the host reads
    gkr::MleHostRecSub* rec = nullptr;     // the records the passes publish to: h_rec, or device records on their way through an exchange
    uint32_t* arrivals = nullptr;          // zeroed counters of passes that publish from their last block; null: no pass does
    Fr* h_tail = nullptr;                  // pinned: the host tail's tables, 2^kMleTailLog2 entries apart; null: no host tail
    // pinned: flag-in-word records (flagged_rec.h), kFlagRecsPerTable per sumcheck, which the blocks of a publishing streaming pass
    // write and the hashing threads total into h_rec; null: every streaming pass publishes through k_mle_sub_reduce
    uint64_t* h_flag = nullptr;
    uint64_t* flag_rec(int b) const { return h_flag + (size_t)b * gkr::kFlagRecsPerTable * gkr::kFlagRecWords; }
};
// (slots `prefix`.work / .partials / .plans / .rec / .w: the context caches the allocations by these names)
static int mle_pass_tables(gkr_ctx* ctx, const std::string& prefix, const Fr* input, size_t len, size_t work_len, int batch, MlePassTables& T) {
    T.input = input;
    T.in_stride = len;
    T.work_len = work_len;
    WS(ctx, (prefix + ".work").c_str(), Fr, (size_t)batch * (work_len ? work_len : 1), T.work);
    WS(ctx, (prefix + ".partials").c_str(), gkr::MleSubPartial, (size_t)batch * gkr::kMaxBlocksPerTable, T.partials);
    WS(ctx, (prefix + ".plans").c_str(), unsigned char, (size_t)batch * gkr::mle_fold_plan_bytes(), T.plans);
    HIP_TRY(ctx, ctx->pinned_host((prefix + ".rec").c_str(), sizeof(gkr::MleHostRecSub) * batch, reinterpret_cast<void**>(&T.h_rec)));
    HIP_TRY(ctx, ctx->pinned_host((prefix + ".w").c_str(), sizeof(Fr) * gkr::kMleMaxSub * batch, reinterpret_cast<void**>(&T.h_w)));
    T.rec = T.h_rec;
    return GKR_OK;
}

// Latency-bound passes (a few sumchecks of moderate size: at most kFusedPublishBytes read per launch) publish from their
// last block instead of through k_mle_sub_reduce: one launch and one dependent-launch gap less per pass on the round
// path of a lone sumcheck.  Streaming passes keep the second launch (see mle_publish_from_last_block).
constexpr double kFusedPublishBytes = 64.0 * 1024 * 1024;
constexpr uint32_t kFusedPublishBlocks = 256;   // blocks per launch: each pays one L2 write-back (~30 ns, one after the other)
constexpr size_t kArrivalCounters = 4096;       // (one size: zeroed once per allocation, every pass leaves them zero)
// ---- the launch plan: every decision below as a value (gkr_selftest_mle_plan reports them; include/gkr_amd.h GKR_MLE_*).  Host
// arithmetic only: the launches call these functions and do what they say, the self-test walks them without a device.
enum : uint32_t {
    kMleKindSmall0 = GKR_MLE_KIND_SMALL0, kMleKindSub0 = GKR_MLE_KIND_SUB_SUMS /* + the form, 0 .. 3 */, kMleKindRollPub = GKR_MLE_KIND_ROLL_PUB,
    kMleKindFineSums = GKR_MLE_KIND_FINE_SUMS, kMleKindFold2 = GKR_MLE_KIND_FOLD2, kMleKindFoldSmall = GKR_MLE_KIND_FOLD_SMALL,
    kMleKindFoldMfma = GKR_MLE_KIND_FOLD_MFMA, kMleKindFoldValu = GKR_MLE_KIND_FOLD_VALU, kMleKindHostFold = GKR_MLE_KIND_HOST_FOLD
};
struct MleLaunchPlan {
    uint32_t kind = 0, nblk = 1, chunk = 0;   // the kernel form, blocks per table, entries per block
    uint32_t publisher = GKR_MLE_PUB_SELF;
};
// the arrival counters of passes that publish from their last block: wanted at all?
static bool mle_wants_arrivals(size_t len) { return gkr::opt(gkr::OPT_no_fused_reduce) == 0 && (double)len * 32.0 <= kFusedPublishBytes; }
static int mle_arrival_counters(gkr_ctx* ctx, size_t len, MlePassTables& T) {
    if (!mle_wants_arrivals(len)) return GKR_OK;
    WS(ctx, "mlep.arrivals", uint32_t, kArrivalCounters, T.arrivals);
    if (ctx->mle_arrivals_zeroed != T.arrivals) {
        HIP_TRY(ctx, hipMemsetAsync(T.arrivals, 0, sizeof(uint32_t) * kArrivalCounters, ctx->stream));
        ctx->mle_arrivals_zeroed = T.arrivals;
    }
    return GKR_OK;
}
static bool fused_publish_applies(bool arrivals, int b0, int nb, uint32_t nblk, double bytes_read) {
    return arrivals && (size_t)(b0 + nb) <= kArrivalCounters && bytes_read <= kFusedPublishBytes && (uint64_t)nblk * nb <= kFusedPublishBlocks && nblk <= 128u;
}
static gkr::MlePublish fused_publish(const MlePassTables& T, int b0, uint32_t ticket, int jout) {
    gkr::MlePublish pub;
    pub.rec = T.rec + b0;
    pub.arrivals = T.arrivals + b0;
    pub.ticket = ticket;
    pub.jout = (uint32_t)jout;
    return pub;
}

constexpr uint32_t kMleTailLog2 = 7;   // the host tail (run_mle_batch_passes): tables of 2^7 entries and fewer
// What differs between the callers of a pass (the stream is an argument): a scheduling group, the device-hashed chain, the
// driver of a table split over ranks.
struct MlePassPolicy {
    const char* row = nullptr;   // profile row of the streaming kernel
    int plan_event = -1;         // >= 0: the fold's digit matrices on the side stream, ordered by this aux event; -1: on the pass's own stream, untimed
    Fr* export_tail = nullptr;   // a one-block fold leaves its tables here as well (the host tail's slice of h_tail)
    int blocks_jout = 0;         // pass 0, > 0: blocks per table as for 2^blocks_jout sub-blocks (the two-level first fold's fine sums)
    uint32_t src_planes = 1;     // a one-block fold: its source is the sum of this many planes, 2^m_src entries apart
    bool flagged = false;        // pass 0: its blocks may publish flag-in-word records (T.h_flag) instead of a reduce launch
};
// pass 0's blocks per table; ahead of a two-level first fold a multiple of 1024 (every fine sum a run of partials) of whole 256-entry chunks
static uint32_t pass0_blocks(size_t len, int jout, int nb, const MlePassPolicy& P) {
    uint32_t nblk = gkr::mle_pass_blocks((uint32_t)len, (uint32_t)(P.blocks_jout > 0 ? P.blocks_jout : jout), nb);
    if (P.blocks_jout > 0 && len / nblk < 256u) nblk = (uint32_t)(len / 256u);
    return nblk;
}
static void queue_sub_reduce(gkr_ctx* ctx, const MlePassTables& T, int b0, int nb, uint32_t nblk, int jout, uint32_t ticket, hipStream_t st) {
    Timed t(ctx, "mle_sub_reduce", 0.0, st, true);
    gkr::launch_mle_sub_reduce(T.partials + (size_t)b0 * gkr::kMaxBlocksPerTable, nblk, (uint32_t)jout, nb, T.rec + b0, ticket, st);
}
// pass 0 of the sumchecks [b0, b0 + nb) of tables of `len` entries, as a plan: arrivals = the run has arrival counters (T.arrivals)
static MleLaunchPlan plan_pass0(size_t len, bool arrivals, int b0, int nb, int jout, const MlePassPolicy& P) {
    MleLaunchPlan L;
    if (len <= gkr::kSmallPassEntries) {
        L.kind = kMleKindSmall0;
        L.chunk = (uint32_t)len;
        return L;
    }
    L.nblk = pass0_blocks(len, jout, nb, P);
    L.chunk = (uint32_t)(len / L.nblk);
    const bool fused = fused_publish_applies(arrivals, b0, nb, L.nblk, (double)nb * len * 32.0);
    const int form = gkr::mle_sub_sums_stream_form((uint32_t)len, (uint32_t)nb, L.nblk, fused);
    const bool flagged = P.flagged && !fused && gkr::mle_sub_sums_publishes_flagged(form, L.nblk);
    L.kind = flagged ? kMleKindRollPub : kMleKindSub0 + (uint32_t)form;
    L.publisher = fused ? GKR_MLE_PUB_FUSED : (flagged ? GKR_MLE_PUB_FLAGGED : GKR_MLE_PUB_REDUCE);
    return L;
}
// pass 0 of the sumchecks [b0, b0 + nb): the 2^jout sub-block sums of the input tables.  true: its blocks publish flag-in-word
// records (P.flagged and a launch that takes the publishing kernel), which the host totals -- no reduce launch was queued
static bool queue_pass0(gkr_ctx* ctx, const MlePassTables& T, int b0, int nb, int jout, uint32_t ticket, hipStream_t st, const MlePassPolicy& P) {
    const size_t len = T.in_stride;
    const Fr* src = T.input + (size_t)b0 * len;
    const double bytes = (double)nb * len * 32.0;
    const MleLaunchPlan L = plan_pass0(len, T.arrivals != nullptr, b0, nb, jout, P);
    if (L.kind == kMleKindSmall0) {
        Timed t(ctx, "mle_pass_small", bytes, st, true);
        gkr::launch_mle_multifold_small(0, src, len, nullptr, 0, (uint32_t)len, (uint32_t)jout, nb, T.h_w + (size_t)b0 * gkr::kMleMaxSub, T.rec + b0, ticket, st);
        return false;
    }
    const uint32_t nblk = L.nblk;
    const bool fused = L.publisher == GKR_MLE_PUB_FUSED;
    const gkr::MlePublish pub = fused ? fused_publish(T, b0, ticket, jout) : gkr::MlePublish{};
    bool flagged;
    {
        Timed t(ctx, P.row, bytes, st, fused);
        flagged = gkr::launch_mle_sub_sums(src, len, (uint32_t)len, nb, nblk, T.partials + (size_t)b0 * gkr::kMaxBlocksPerTable, st, fused ? &pub : nullptr,
                                           P.flagged && !fused ? T.flag_rec(b0) : nullptr, ticket);
    }
    if (!fused && !flagged) queue_sub_reduce(ctx, T, b0, nb, nblk, jout, ticket, st);
    return flagged;
}
// a fold pass of tables of 2^m_src entries that binds jin variables, as a plan
static MleLaunchPlan plan_fold(bool arrivals, int b0, int nb, int m_src, int jin, int jout) {
    MleLaunchPlan L;
    const size_t src_len = (size_t)1 << m_src, S = src_len >> jin;
    if (S <= gkr::kSmallPassEntries) {
        L.kind = kMleKindFoldSmall;
        L.chunk = (uint32_t)S;
        return L;
    }
    L.nblk = gkr::mle_multifold_blocks((uint32_t)S, (uint32_t)jout, nb);
    L.chunk = (uint32_t)(S / L.nblk);
    L.kind = gkr::mle_multifold_uses_mfma((uint32_t)S, L.nblk) ? kMleKindFoldMfma : kMleKindFoldValu;
    L.publisher = fused_publish_applies(arrivals, b0, nb, L.nblk, (double)nb * (double)src_len * 32.0) ? GKR_MLE_PUB_FUSED : GKR_MLE_PUB_REDUCE;
    return L;
}
// a fold pass: bind the jin variables just hashed of tables of 2^m_src entries (the input, or work), produce the sums of the next jout rounds
static void queue_fold(gkr_ctx* ctx, const MlePassTables& T, int b0, int nb, bool from_input, int m_src, int jin, int jout, uint32_t ticket,
                       hipStream_t st, const MlePassPolicy& P) {
    const size_t src_len = (size_t)1 << m_src, S = src_len >> jin;
    const Fr* src = from_input ? T.input + (size_t)b0 * T.in_stride : T.work + (size_t)b0 * T.work_len;
    const size_t src_stride = from_input ? T.in_stride : T.work_len;
    Fr* dst = T.work + (size_t)b0 * T.work_len;
    const Fr* w = T.h_w + (size_t)b0 * gkr::kMleMaxSub;
    const double bytes = (double)nb * ((double)src_len * P.src_planes + (double)S) * 32.0;
    const MleLaunchPlan L = plan_fold(T.arrivals != nullptr, b0, nb, m_src, jin, jout);
    if (L.kind == kMleKindFoldSmall) {
        Timed t(ctx, "mle_pass_small", bytes, st, true);
        gkr::launch_mle_multifold_small(jin, src, src_stride, dst, T.work_len, (uint32_t)S, (uint32_t)jout, nb, w, T.rec + b0, ticket, st, P.export_tail,
                                        1u << kMleTailLog2, P.src_planes, (uint32_t)src_len);
        return;
    }
    const uint32_t nblk = L.nblk;
    unsigned char* plan = T.plans + (size_t)b0 * gkr::mle_fold_plan_bytes();
    if (L.kind == kMleKindFoldMfma) {
        // the digit matrices only depend on the weights the host just wrote: built on the side stream, the main stream (busy
        // with another group's pass) pays one event wait, not a launch round trip -- where the caller asks for it
        if (P.plan_event < 0) {
            gkr::launch_mle_fold_plan(jin, w, plan, nb, st);
        } else {
            {
                Timed t(ctx, "mle_fold_plan", 0.0, ctx->aux, true);
                gkr::launch_mle_fold_plan(jin, w, plan, nb, ctx->aux);
            }
            (void)hipEventRecord(ctx->aux_events[P.plan_event], ctx->aux);
            (void)hipStreamWaitEvent(st, ctx->aux_events[P.plan_event], 0);
        }
    }
    const bool fused = L.publisher == GKR_MLE_PUB_FUSED;
    const gkr::MlePublish pub = fused ? fused_publish(T, b0, ticket, jout) : gkr::MlePublish{};
    {
        Timed t(ctx, P.row, bytes, st, fused);
        gkr::launch_mle_multifold(jin, src, src_stride, dst, T.work_len, (uint32_t)S, nb, nblk, w, plan, T.partials + (size_t)b0 * gkr::kMaxBlocksPerTable, st,
                                  fused ? &pub : nullptr);
    }
    if (!fused) queue_sub_reduce(ctx, T, b0, nb, nblk, jout, ticket, st);
}

// ------------------------------------------------------------- the schedule of a batch: arithmetic only, no device
struct MleSchedule {
    int jmax = 0, j_first = 0;    // rounds per pass at most; rounds of pass 0
    int n_dev = 0;                // sumchecks [0, n_dev) are hashed on the device, as one chain on a stream of its own
    int groups = 0, depth = 0;    // scheduling groups of the host-hashed rest; groups whose pass 0 is queued up front
    int bound[kMaxGroups + 1];    // group g: sumchecks [bound[g], bound[g + 1])
    uint32_t chunk[kMaxGroups];   // sumchecks a hashing thread takes at a time from group g
    bool tail_on = false;         // the host finishes tables of 2^kMleTailLog2 entries and fewer
    bool two_level = false;       // the host-hashed groups' first fold binds ten variables (capi_internal.h mle_two_level_first_fold)
};
static MleSchedule mle_schedule(int n, int batch, int hash_threads, bool is_tail, const gkr::Options& o) {
    MleSchedule sc;
    const double len = (double)((size_t)1 << n);
    // rounds per pass: up to 5 with the matrix-core fold (fewer passes, ~2.07 N elements moved instead of 2.29 N),
    // up to 3 with the v_mad_u64_u32 fold (option no_mfma_fold)
    const int jcap = o.v[gkr::OPT_no_mfma_fold] ? 3 : gkr::kMlePassMaxRounds;
    const int jwant = o.v[gkr::OPT_rounds_per_pass] > 0 ? (int)o.v[gkr::OPT_rounds_per_pass] : jcap;
    sc.jmax = jwant > jcap ? jcap : jwant;
    sc.j_first = mle_pass_rounds(n, n, sc.jmax);
    // (the driver of a table split over ranks finishes on a gathered tail table: its schedule stays what it was)
    sc.two_level = !is_tail && mle_two_level_first_fold(n, o);
    // Groups of ~4 GiB of tables, at least four and at most eight (1024 x 2^20: eight groups of 128); sixteen for batches
    // beyond 96 GiB (4096 x 2^20: 4.64e11 field-ops/s with sixteen groups of 256, 4.48e11 with eight of 512).  Larger launches
    // stream slightly better, smaller groups feed the host's hashing more evenly and leave a shorter exposed tail (the
    // last group's late passes); measured on MI355X, 1024 x 2^20, interleaved repeats on one box, ms per step with
    // 14 / 3 / 2 host threads: 4 groups, all pass 0s queued first 12.3-12.9 / 15.0-16.3 / 18.5-19.0; 8 groups, pass 0
    // queue depth 2 (below) 12.0-12.5 / 13.5-14.0 / 16.5-17.8; 6, 10 and 12 groups in between.
    // Sumchecks hashed ON THE DEVICE (kernels_transcript.hip): the first n_dev of the batch run as one chain of kernels on
    // a stream of their own -- pass, the pass's rounds with MiMC7 on eight lanes per element, fold, ... -- without the host;
    // the host hashes the rest as always.  A device-hashed pass takes 0.33 ms per round whatever the number of sumchecks
    // (the chain of 2 x 91 x 4 dependent products), so this is for steps that are bound by the host's hashing: a rank with
    // two or three host threads, tables so small that the GPU is mostly idle.  Option device_hash_percent = share of the batch
    // (0 = none, the default).
    const long long dp = o.v[gkr::OPT_device_hash_percent];
    const int dev_percent = dp < 0 ? 0 : (dp > 90 ? 90 : (int)dp);
    if (dev_percent > 0 && !is_tail && batch >= 64 && sc.j_first >= 1) {
        sc.n_dev = (int)((long long)batch * dev_percent / 100) & ~7;
        if (batch - sc.n_dev < 16) sc.n_dev = (batch - 16) & ~7;
        if (sc.n_dev < 8) sc.n_dev = 0;
    }
    const int host_batch = batch - sc.n_dev;
    const double batch_bytes = (double)host_batch * len * 32.0;
    int want_groups = (int)(batch_bytes / (4.0 * 1024 * 1024 * 1024));
    want_groups = want_groups < 4 ? 4 : (want_groups > 8 ? (batch_bytes > 96.0 * 1024 * 1024 * 1024 ? 16 : 8) : want_groups);
    // Small tables (BASELINE configs[1]: 4096 x 2^16) are bound by the host's hashing, not by the stream: sixteen groups
    // with pass 0 of four of them queued ahead keep the hashing threads fed from start to end (MI355X, 14 threads, ms per
    // 4096 x 2^16: 4 groups 8.1 - 8.2, 8 groups 8.1, 16 groups 7.2, 16 groups / depth 4 7.0 - 7.2, 32 groups / depth 8 7.1;
    // profiles/r03/f_n16_groups*.jsonl)
    const bool small_tables = n <= 17 && host_batch >= 256;
    if (small_tables) want_groups = 16;
    // A rank with two or three host threads (eight ranks on a 16-core host) is bound by its hashing: smaller groups shorten
    // the stretch before the first hashes and after the last fold (1024 x 2^20, two threads: 16.3 - 16.7 ms with eight
    // groups, 16.0 with sixteen; profiles/r03/w_two_host_threads_group_size.jsonl)
    if (hash_threads <= 3 && host_batch >= 256 && want_groups < 16) want_groups = 16;
    int group_size = host_batch >= 128 ? (host_batch + want_groups - 1) / want_groups : (host_batch >= 16 ? (host_batch + 1) / 2 : host_batch);
    if (sc.n_dev && hash_threads <= 3 && host_batch >= 256) group_size = 64;   // (whole sixteen-lane chunks for both threads, as without a device share)
    if (o.v[gkr::OPT_group_size] > 0) group_size = (int)o.v[gkr::OPT_group_size];
    sc.groups = (host_batch + group_size - 1) / group_size;
    if (sc.groups > kMaxGroups) sc.groups = kMaxGroups;
    // Sumchecks a hashing thread takes at a time, per group: sixteen (full IFMA calls: throughput) when the group has plenty
    // for every thread; otherwise ONE chunk per thread where that fits the sixteen lanes -- a pass's J hashes of a sumcheck
    // are a serial chain, so a group of 128 on 14 threads is done in one chain of 16-lane calls filled to 10 (J x 20 us)
    // instead of two chains of 8-lane calls (2 x J x 16 us), at the same cost per hash; the option hash_chunk forces 8 or 16
    const long long forced = o.v[gkr::OPT_hash_chunk];
    for (int g = 0; g <= sc.groups; ++g) sc.bound[g] = sc.n_dev + (int)((long long)host_batch * g / sc.groups);
    for (int g = 0; g < sc.groups; ++g) {
        const int nb = sc.bound[g + 1] - sc.bound[g], per = (nb + hash_threads - 1) / hash_threads;
        sc.chunk[g] = forced == 8 || forced == 16 ? (uint32_t)forced : (nb >= 32 * hash_threads ? 16u : (uint32_t)(per <= 8 ? 8 : (per <= 16 ? per : 16)));
    }
    // Pass 0 of the first `depth` groups is queued up front, pass 0 of a later group right behind the first fold of an
    // earlier one: the stream then alternates between pass 0 of later groups and the first fold of earlier ones
    // (P0 P0 F0 P0 F1 P0 F2 F3 with four groups), and the host's hashing -- which with few threads takes as long as the
    // GPU's work -- is fed from the first millisecond to the last instead of in one burst after all the pass 0s.
    // (All pass 0s first: 2 host threads 19.0 ms per 1024 x 2^20 at 77 % hashing occupancy, 3 threads 15.6 ms at 63 %.)
    sc.depth = o.v[gkr::OPT_pass_queue_depth] > 0 ? (int)o.v[gkr::OPT_pass_queue_depth] : (small_tables ? 4 : 2);
    // The host tail: the last fold pass of a sumcheck works on a table of 2^7 entries and fewer -- 128 products, and ~30 us as a
    // device pass (launch, 15 us of kernel, the record's way back).  For a few sumchecks at a time (a latency chain, not a
    // throughput problem) the pass before it leaves its folded table in pinned memory as well, and the host binds the remaining
    // variables itself: exact field arithmetic, the same canonical sums.
    sc.tail_on = o.v[gkr::OPT_host_tail_log2] >= 0 && sc.n_dev == 0 && batch <= (o.v[gkr::OPT_host_tail_max_batch] > 0 ? o.v[gkr::OPT_host_tail_max_batch] : 8);
    return sc;
}
// ---- what the driver decides per pass from the schedule (host arithmetic; the driver and the launch plan both call these)
// a group's small late passes have a stream of their own
static bool mle_late_stream(const MleSchedule& sc) { return !gkr::opt(gkr::OPT_no_late_stream) && sc.groups > 1; }
// the small launches beside the streaming passes (the fold's digit matrices, the fine sums, the second level's weights) go to the side stream
static bool mle_side_launches(const MleSchedule& sc) { return !gkr::opt(gkr::OPT_plan_main) && sc.groups != 1; }
// flag-in-word records (option stream_publish): where another group's launch waits behind a streaming pass's reduce -- several
// host-hashed groups on the two-level schedule
static bool mle_flag_records(const MleSchedule& sc) { return gkr::opt(gkr::OPT_stream_publish) != 1 && sc.two_level && sc.groups > 1; }
static bool mle_group_two_level(const MleSchedule& sc, bool chain) { return sc.two_level && !chain; }
// pass 0 of a group is offered the flag-in-word records
static bool mle_pass0_flagged(const MleSchedule& sc, bool chain, int j) {
    return mle_flag_records(sc) && mle_group_two_level(sc, chain) && j == gkr::kMlePassMaxRounds;
}
// the stream of a fold pass over tables of 2^m_src entries (GKR_MLE_STREAM_*): small source tables make a latency-bound late pass, not to
// be queued behind other groups' streaming passes
static uint32_t mle_fold_stream(const MleSchedule& sc, int n, bool chain, int m_src) {
    if (chain) return GKR_MLE_STREAM_CHAIN;
    return m_src != n && m_src <= 16 && mle_late_stream(sc) ? GKR_MLE_STREAM_LATE : GKR_MLE_STREAM_MAIN;
}
// its digit matrices on the side stream?  (one group: nothing else is streaming, and the event between the two streams costs the
// round path ~10 us more than a second launch on the same stream -- 15 us against 5 between the plan and the fold)
static bool mle_fold_plan_on_side(const MleSchedule& sc, uint32_t stream) { return stream == GKR_MLE_STREAM_MAIN && mle_side_launches(sc); }
// the fold leaves tables of 2^m entries whose sums cover j rounds: small enough for the host to finish, and there is a pass left to save
static bool mle_fold_exports_tail(const MleSchedule& sc, bool chain, int m, int j) {
    return sc.tail_on && !chain && m <= (int)kMleTailLog2 && m - j > 0;
}

// ---- the launch plan of a call (gkr_selftest_mle_plan, include/gkr_amd.h): the passes of every group in the order the driver
// (MlePassRun::step, queue_device_chain) takes them, each decided by the functions above.
// SHARED with the launches: every value of a row -- pass0_blocks, plan_pass0, plan_fold, mle_multifold2_blocks, the stream, plan,
// tail and record predicates, mle_pass_rounds.  RESTATED here, and so not held by the plan's tests: the ORDER of a group's passes
// (pass 0, then fine sums and the two-level fold where the group takes them, then folds until the sums cover the last round; step,
// launch_fine_sums, launch_fold2, host_fold, queue_device_chain), with what they carry from pass to pass (m, j, `planes` set by
// launch_fold2 and cleared by the fold behind it, `on_host` set by launch_fold and kept by host_fold).  A change to that sequencing
// has to be made here too; the byte comparisons of tests/test_gpu_mle_plan.py hold the driver's own.
struct MlePlanRow {
    uint32_t w[GKR_MLE_PLAN_ROW_WORDS];
};
static MlePlanRow mle_plan_row(int g, size_t pass, const MleLaunchPlan& L, int m_src, int jin, int jout, uint32_t stream, int b0, int nb) {
    MlePlanRow r{};
    const uint32_t v[] = {(uint32_t)g, (uint32_t)pass, L.kind, (uint32_t)m_src, (uint32_t)jin, (uint32_t)jout, L.nblk, L.chunk, L.publisher, stream};
    memcpy(r.w, v, sizeof(v));
    r.w[12] = 1;
    r.w[13] = (uint32_t)b0;
    r.w[14] = (uint32_t)nb;
    return r;
}
static void mle_plan_group(const MleSchedule& sc, int n, int g, int b0, int nb, bool chain, std::vector<MlePlanRow>& rows) {
    const size_t len = (size_t)1 << n, first = rows.size();
    const bool arrivals = mle_wants_arrivals(len), two = mle_group_two_level(sc, chain);
    const uint32_t own = chain ? GKR_MLE_STREAM_CHAIN : GKR_MLE_STREAM_MAIN;
    int m = n, j = sc.j_first;
    bool planes = false, on_host = false;
    MlePassPolicy P0;
    if (two) P0.blocks_jout = kMleTwoLevelRounds;
    P0.flagged = mle_pass0_flagged(sc, chain, j);
    rows.push_back(mle_plan_row(g, 0, plan_pass0(len, arrivals, b0, nb, j, P0), n, 0, j, own, b0, nb));
    while (m - j > 0) {
        const size_t pass = rows.size() - first;
        if (m == n && two) {
            // the fine sums and the digit matrices of rounds 1-5 (launch_fine_sums), then the fold of ten variables (launch_fold2)
            const bool side = mle_side_launches(sc);
            MlePassPolicy Pb;
            Pb.blocks_jout = kMleTwoLevelRounds;
            MleLaunchPlan F;
            F.kind = kMleKindFineSums;
            F.nblk = pass0_blocks(len, j, nb, Pb);
            F.chunk = (uint32_t)(len / F.nblk);
            rows.push_back(mle_plan_row(g, pass, F, n, j, gkr::kMlePassMaxRounds, side ? GKR_MLE_STREAM_SIDE : GKR_MLE_STREAM_MAIN, b0, nb));
            rows.back().w[10] = side ? GKR_MLE_PLAN_SIDE_STREAM : GKR_MLE_PLAN_OWN_STREAM;
            const uint32_t S = 1u << (n - gkr::kMlePassMaxRounds);
            MleLaunchPlan L;
            L.kind = kMleKindFold2;
            L.nblk = gkr::mle_multifold2_blocks(S);
            L.chunk = S / L.nblk;
            L.publisher = mle_flag_records(sc) && gkr::mle_multifold2_publishes_flagged(S) ? GKR_MLE_PUB_FLAGGED : GKR_MLE_PUB_REDUCE;
            rows.push_back(mle_plan_row(g, pass + 1, L, n, kMleTwoLevelRounds, gkr::kMlePassMaxRounds, GKR_MLE_STREAM_MAIN, b0, nb));
            m = n - kMleTwoLevelRounds;
            j = gkr::kMlePassMaxRounds;
            planes = true;
            on_host = false;
            continue;
        }
        const int m_src = m, jin = j;
        m -= jin;
        j = mle_pass_rounds(m, n, sc.jmax);
        if (on_host) {
            MleLaunchPlan H;
            H.kind = kMleKindHostFold;
            H.chunk = 1u << m;
            H.publisher = GKR_MLE_PUB_HOST;
            rows.push_back(mle_plan_row(g, pass, H, m_src, jin, j, GKR_MLE_STREAM_HOST, b0, nb));
            continue;
        }
        const uint32_t stream = mle_fold_stream(sc, n, chain, m_src);
        const MleLaunchPlan L = plan_fold(arrivals, b0, nb, m_src, jin, j);
        on_host = mle_fold_exports_tail(sc, chain, m, j);
        rows.push_back(mle_plan_row(g, pass, L, m_src, jin, j, stream, b0, nb));
        MlePlanRow& r = rows.back();
        if (L.kind == kMleKindFoldMfma) r.w[10] = mle_fold_plan_on_side(sc, stream) ? GKR_MLE_PLAN_SIDE_STREAM : GKR_MLE_PLAN_OWN_STREAM;
        r.w[11] = on_host && L.kind == kMleKindFoldSmall;   // (launch_mle_multifold_small is what takes the tail pointer)
        r.w[12] = planes ? gkr::kMleFold2Planes : 1u;
        planes = false;
    }
}
// (the options are the calling thread's: an OptionScope around the call)
static int mle_plan(int n, int batch, int hash_threads, uint32_t* header, uint32_t* out_rows, size_t row_capacity, size_t* n_rows) {
    if (!header || !n_rows || (!out_rows && row_capacity) || n < 2 || n > GKR_MAX_MLE_N || batch < 1 || batch > 65535 ||
        ((unsigned long long)batch << n) > (1ull << 30) || hash_threads < 1)
        return GKR_ERR_INVALID;
    const gkr::Options* o = gkr::current_options();
    const MleSchedule sc = mle_schedule(n, batch, hash_threads, false, o ? *o : gkr::default_options());
    std::vector<MlePlanRow> rows;
    for (int g = 0; g < sc.groups; ++g) mle_plan_group(sc, n, g, sc.bound[g], sc.bound[g + 1] - sc.bound[g], false, rows);
    if (sc.n_dev) mle_plan_group(sc, n, sc.groups, 0, sc.n_dev, true, rows);
    memset(header, 0, sizeof(uint32_t) * GKR_MLE_PLAN_HEADER_WORDS);
    const bool flags = mle_flag_records(sc) && gkr::mle_multifold2_publishes_flagged(1u << (n - gkr::kMlePassMaxRounds));
    const uint32_t h[] = {(uint32_t)sc.jmax, (uint32_t)sc.j_first, (uint32_t)sc.n_dev, (uint32_t)sc.groups, (uint32_t)sc.depth, sc.tail_on, sc.two_level,
                          flags ? (uint32_t)sc.groups - 1u : 0u, sc.two_level ? (flags ? 1u : (uint32_t)sc.groups) : 0u, (uint32_t)hash_threads};
    memcpy(header, h, sizeof(h));
    static_assert(10 + kMaxGroups + 1 + kMaxGroups <= GKR_MLE_PLAN_HEADER_WORDS, "the header holds every bound and chunk");
    for (int g = 0; g <= sc.groups; ++g) header[10 + g] = (uint32_t)sc.bound[g];
    for (int g = 0; g < sc.groups; ++g) header[10 + kMaxGroups + 1 + g] = sc.chunk[g];
    *n_rows = rows.size();
    for (size_t i = 0; i < rows.size() && i < row_capacity; ++i) memcpy(out_rows + i * GKR_MLE_PLAN_ROW_WORDS, rows[i].w, sizeof(rows[i].w));
    return GKR_OK;
}

// ------------------------------------------------------------- the driver
namespace {
struct PassGroup : GroupHandoff {   // (generation of the hand-off = pass number + 1)
    int m = 0;        // variables left in the current table
    int j = 0;        // rounds the landed sums cover (the pass in flight produces 2^j sums)
    int round0 = 0;   // global index of the first of those rounds
    int pass = 0, index = 0;
    hipStream_t chain = nullptr;   // a device-hashed group: the stream its whole chain runs on
    bool on_host = false;          // the host tail: the group's tables (2^m entries each) are in h_tail, the device is done with them
    // the two-level first fold: rounds 1-5 hashed -> launch_fine_sums -> (mid) its record landed, rounds 6-10 hashed ->
    // launch_fold2, which leaves the table in planes for the one pass after it
    bool mid = false, planes = false;
    // the pass in flight published flag-in-word records under this ticket, and its tables are still being totalled by the hashing
    // threads (try_total); 0: nothing to total.  Set by the driving thread with the launch, cleared by whoever totals the last table.
    std::atomic<uint32_t> flag_ticket{0};
    std::atomic<int> flag_left{0};   // tables of that pass not totalled yet
    int pub_index = -1;              // ... as launch pubs[pub_index] of the main stream, until what depends on its end is queued (after_stream_pass)
    bool end_bound = false;          // that launch fires the group's end event with its completion
};
// a table's records while a hashing thread looks at them: one thread at a time (busy), from where the last look stopped
struct FlagScan {
    std::atomic<uint32_t> busy{0};
    std::atomic<uint32_t> done{0};   // the ticket whose records were totalled last
    std::atomic<uint32_t> cursor{0}, cursor_ticket{0};   // written by the owner, under busy; read by anyone as a hint of where to peek
};
// GKR_DEBUG_TIMING: the phases of a call on the host clock
struct MlePassClock {
    const bool on = gkr::debug_timing();
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double a = 0, b = 0, c = 0, d = 0, e = 0;
    std::atomic<uint64_t> busy_ns{0};   // time inside process_chunk, all threads
    double us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); }
    void report(int threads) const {
        if (!on) return;
        fprintf(stderr,
                "[gkr timing] setup %.0f us, first launches %.0f, loop %.0f, end_session %.0f, sync %.0f, drain %.0f; hashing %.0f us "
                "over %d threads = %.0f%% of the loop\n",
                a, b - a, c - b, d - c, e - d, us() - e, busy_ns.load() * 1e-3, threads, busy_ns.load() * 1e-3 / ((c - b) * threads) * 100.0);
    }
};

struct MlePassRun {
    gkr_ctx* ctx;
    const int n, batch;
    const MleTailArgs* tail;
    gkr_fr* out_coeffs;
    uint32_t* out_len;
    gkr_fr* out_r;
    MleSchedule sc;
    MlePassTables T;
    hipStream_t s = nullptr, late = nullptr, chain = nullptr;
    std::vector<PassGroup> grp;
    std::vector<uint32_t> dep_last;
    int next_first = 0;   // groups [next_first, groups): pass 0 still to launch
    int folds_queued = 0;   // two-level first folds launched so far
    struct PubLaunch {
        int b0;
        uint32_t ticket;
    };
    std::vector<PubLaunch> pubs;   // the main stream's publishing launches, in order ...
    int pubs_started = -1;         // ... the last of them that is known to have started
    hipError_t order_err = hipSuccess;   // the first failure of an event record / wait that orders a dependent launch (after_stream_pass)
    std::unique_ptr<FlagScan[]> scan;   // per sumcheck; null: no pass of this call publishes flag-in-word records
    gkr_fr *stage_c = nullptr, *stage_r = nullptr;   // pinned: the device-hashed sumchecks' outputs, in the caller's layout
    uint32_t* stage_len = nullptr;
    MlePassClock clock;

    int rounds_for(int m) const { return mle_pass_rounds(m, n, sc.jmax); }
    void advance(PassGroup& G, int jin) {
        G.m -= jin;
        G.round0 += jin;
        G.j = rounds_for(G.m);
        G.ticket = gkr::next_ticket(ctx->ticket);
    }
    // the group's pass in flight published flag-in-word records: its tables are the hashing threads' to total from here on
    void arm_totals(PassGroup& G, bool end_bound) {
        G.pub_index = (int)pubs.size();
        G.end_bound = end_bound;
        pubs.push_back({G.b0, G.ticket});
        G.flag_left.store(G.nb, std::memory_order_relaxed);
        G.flag_ticket.store(G.ticket, std::memory_order_release);
    }
    // The records say that every block of a publishing kernel has stored its sums, not that the kernel has ENDED: what it left in device
    // memory (pass 0's partials, the fold's planes) is another stream's to read only behind its end.  The host settles that too, without
    // a packet on the main stream: the stream runs its kernels in order, so the kernel has ended -- and its writes are out of the caches
    // -- once a LATER publishing launch of the main stream has started, which the first word of that launch's first record shows
    // (a block of the first wave of blocks writes it, ~30 us into the kernel; the dependent launch comes J hashes, 100 us and more,
    // behind the records).  ASSUMED, as the single-copy-atomic store is (flagged_rec.h): the runtime queues every kernel of a stream with
    // the AQL barrier bit, so no wave of a kernel runs before the kernel ahead of it on the stream has completed, its end-of-kernel
    // write-back included -- what the parent relied on too, through the reduce launch's record.  Where no later launch shows (none queued: pass_queue_depth 1; the one behind it is the call's last, which
    // does not publish), the dependent stream waits for an event: the one bound to the kernel's completion (end_bound; it costs the
    // launch behind it ~5 us, so only the fold ahead of the call's last one gets it), or, if the main stream is not already empty, one
    // recorded now behind whatever the main stream holds.
    hipEvent_t ended_event(const PassGroup& G) const { return ctx->ended_events[G.index]; }
    bool later_launch_started(int index) {
        for (int q = (int)pubs.size() - 1; q > index && q > pubs_started; --q)
            if ((uint32_t)(__atomic_load_n(T.flag_rec(pubs[q].b0), __ATOMIC_RELAXED) >> 32) == pubs[q].ticket) pubs_started = q;
        return pubs_started > index;
    }
    void after_stream_pass(PassGroup& G, hipStream_t st) {
        const int index = G.pub_index;
        G.pub_index = -1;
        if (index < 0 || st == s) return;   // (no publishing pass in flight; or the same stream, which orders it)
        // (a failure here would leave the dependent launch unordered: it ends the call -- loop())
        hipError_t e = hipSuccess;
        if (!G.end_bound) {
            if (later_launch_started(index) || hipStreamQuery(s) == hipSuccess) return;
            e = hipEventRecord(ended_event(G), s);
        }
        if (e == hipSuccess) e = hipStreamWaitEvent(st, ended_event(G), 0);
        if (e != hipSuccess && order_err == hipSuccess) order_err = e;
    }
    // pass 0: sub-block sums of the input tables
    void launch_first(PassGroup& G) {
        G.ticket = gkr::next_ticket(ctx->ticket);
        MlePassPolicy P;
        P.row = G.chain ? "mle_sub_sums_dev" : "mle_sub_sums";
        if (two_level(G)) P.blocks_jout = kMleTwoLevelRounds;
        P.flagged = scan && mle_pass0_flagged(sc, G.chain != nullptr, G.j);
        if (queue_pass0(ctx, T, G.b0, G.nb, G.j, G.ticket, G.chain ? G.chain : s, P)) arm_totals(G, false);
    }
    void launch_next_first() {
        if (next_first < sc.groups) launch_first(grp[next_first++]);
    }
    // a fold pass: bind the jin variables just hashed, produce the sums of the next rounds
    void launch_fold(PassGroup& G, int jin) {
        const int m_src = G.m;
        const bool from_input = m_src == n;
        const uint32_t where = mle_fold_stream(sc, n, G.chain != nullptr, m_src);
        hipStream_t st = where == GKR_MLE_STREAM_CHAIN ? G.chain : (where == GKR_MLE_STREAM_LATE ? late : s);
        after_stream_pass(G, st);
        advance(G, jin);
        MlePassPolicy P;
        // late passes run beside other groups' streaming passes: their elapsed time is not their own cost, so they
        // are booked under their own name and stay out of the streaming fold pass's bandwidth figure
        P.row = G.chain ? "mle_multifold_dev" : (st == s ? "mle_multifold" : "mle_multifold_late");
        if (mle_fold_plan_on_side(sc, where)) P.plan_event = G.index;
        G.on_host = mle_fold_exports_tail(sc, G.chain != nullptr, G.m, G.j);
        if (G.on_host) P.export_tail = T.h_tail + ((size_t)G.b0 << kMleTailLog2);
        if (G.planes) P.src_planes = gkr::kMleFold2Planes;
        G.planes = false;
        queue_fold(ctx, T, G.b0, G.nb, from_input, m_src, jin, G.j, G.ticket, st, P);
    }
    // ---- the two-level first fold of a host-hashed group (kernels.hip, capi_internal.h mle_two_level_first_fold)
    bool two_level(const PassGroup& G) const { return mle_group_two_level(sc, G.chain != nullptr); }
    // the small launches beside the streaming passes: on the side stream, as the fold's digit matrices are (launch_fold)
    bool side_launches() const { return mle_side_launches(sc); }
    // rounds 1-5 are hashed: the digit matrices of their weights, and the sums of rounds 6-10 from pass 0's partials, which
    // stay as they are until the record of these sums has landed (the fold writes its own only after that)
    void launch_fine_sums(PassGroup& G) {
        const int J = G.j;
        G.mid = true;
        G.round0 += J;
        G.ticket = gkr::next_ticket(ctx->ticket);
        hipStream_t side = side_launches() ? ctx->aux : s;
        MlePassPolicy P0;
        P0.blocks_jout = kMleTwoLevelRounds;
        const uint32_t nblk0 = pass0_blocks(T.in_stride, J, G.nb, P0);
        const Fr* w = T.h_w + (size_t)G.b0 * gkr::kMleMaxSub;
        after_stream_pass(G, side);
        Timed t(ctx, "mle_fold_plan", 0.0, side, true);
        // (the sums first: the host waits for them, the fold for the matrices only five hashes later)
        gkr::launch_mle_fine_sums(T.partials + (size_t)G.b0 * gkr::kMaxBlocksPerTable, nblk0, w, G.nb, T.rec + G.b0, G.ticket, side);
        gkr::launch_mle_fold_plan(J, w, T.plans + (size_t)G.b0 * gkr::mle_fold_plan_bytes(), G.nb, side, side == s ? 0u : 256u);
    }
    // rounds 6-10 are hashed: their weights to the device, then the fold that binds all ten variables and the sums of the five
    // rounds after them
    void launch_fold2(PassGroup& G) {
        const bool side = side_launches();
        {
            Timed t(ctx, "mle_fold_plan", 0.0, side ? ctx->aux : s, true);
            gkr::launch_mle_copy_weights(T.h_w2 + (size_t)G.b0 * gkr::kMleMaxSub, T.d_w2 + (size_t)G.b0 * gkr::kMleMaxSub, G.nb, side ? ctx->aux : s);
        }
        if (side) {   // (one stream: this event is behind the digit matrices too)
            (void)hipEventRecord(ctx->aux_events[G.index], ctx->aux);
            (void)hipStreamWaitEvent(s, ctx->aux_events[G.index], 0);
        }
        const uint32_t S = 1u << (n - gkr::kMlePassMaxRounds), npart = gkr::mle_multifold2_partials(S);
        G.mid = false;
        G.planes = true;
        G.on_host = false;
        G.m = n - kMleTwoLevelRounds;
        G.round0 += G.j;
        G.j = gkr::kMlePassMaxRounds;   // (the fold's partials are fine enough at every n it takes, whatever rounds_for says of a streaming fold)
        G.ticket = gkr::next_ticket(ctx->ticket);
        // The LAST streaming launch of the call (every pass 0 is queued and this is the last group's fold) keeps its reduce launch:
        // nothing is queued behind it on the main stream, and the 11 us kernel is shorter than a host scan on the critical path.
        ++folds_queued;
        const bool last_streaming = next_first == sc.groups && folds_queued == sc.groups;
        const bool before_last = scan && folds_queued == sc.groups - 1;   // (what is launched behind it will not show its start: after_stream_pass)
        bool flagged;
        {
            Timed t(ctx, "mle_multifold", (double)G.nb * ((double)T.in_stride + (double)(gkr::kMleFold2Planes * (S >> gkr::kMlePassMaxRounds))) * 32.0, s);
            flagged = gkr::launch_mle_multifold2(T.input + (size_t)G.b0 * T.in_stride, T.in_stride, T.work + (size_t)G.b0 * T.work_len, T.work_len, S, G.nb,
                                                 T.plans + (size_t)G.b0 * gkr::mle_fold_plan_bytes(), T.d_w2 + (size_t)G.b0 * gkr::kMleMaxSub,
                                                 T.partials + (size_t)G.b0 * gkr::kMaxBlocksPerTable, s, scan && !last_streaming ? T.flag_rec(G.b0) : nullptr,
                                                 G.ticket, before_last ? ended_event(G) : nullptr);
        }
        if (flagged)
            arm_totals(G, before_last);
        else
            queue_sub_reduce(ctx, T, G.b0, G.nb, npart, G.j, G.ticket, s);
    }
    // A hashing thread (or the driving one, when it has nothing to launch): one look at the tables of the passes that published
    // flag-in-word records; true: it totalled one -- its record in h_rec is what k_mle_sub_reduce would have written, seq last.
    // A table whose records have not all landed keeps its cursor and is looked at again, by whoever comes next.
    bool try_total() {
        if (!scan) return false;
        constexpr uint32_t kWords = gkr::kFlagRecsPerTable * gkr::kFlagRecWords;
        for (int g = 0; g < sc.groups; ++g) {
            PassGroup& G = grp[g];
            const uint32_t t = G.flag_ticket.load(std::memory_order_acquire);
            if (!t) continue;
            for (int b = G.b0; b < G.b0 + G.nb; ++b) {
                FlagScan& F = scan[b];
                if (F.done.load(std::memory_order_relaxed) == t || F.busy.load(std::memory_order_relaxed)) continue;
                // (a peek before the claim: the word the last look stopped at.  An idle thread's poll then only READS lines that stay
                // shared until the device writes them; claiming every table on every poll made the threads' hashing 17 % slower)
                const uint32_t at = F.cursor_ticket.load(std::memory_order_relaxed) == t ? F.cursor.load(std::memory_order_relaxed) : 0u;
                if (at < kWords && (uint32_t)(__atomic_load_n(T.flag_rec(b) + at, __ATOMIC_RELAXED) >> 32) != t) continue;
                if (F.busy.exchange(1u, std::memory_order_acquire)) continue;
                bool totalled = false;
                if (F.done.load(std::memory_order_relaxed) != t) {
                    uint32_t cursor = F.cursor_ticket.load(std::memory_order_relaxed) == t ? F.cursor.load(std::memory_order_relaxed) : 0u;
                    gkr::MleHostRecSub& R = T.h_rec[b];
                    uint32_t dep = 0;
                    static_assert(sizeof(R.sums) == gkr::kMleMaxSub * 32, "a sum is four 64-bit words");
                    const bool landed = gkr::flagged_scan(T.flag_rec(b), kWords, t, &cursor);
                    F.cursor.store(cursor, std::memory_order_relaxed);
                    F.cursor_ticket.store(t, std::memory_order_relaxed);
                    if (landed &&
                        gkr::flagged_total(T.flag_rec(b), gkr::kFlagRecsPerTable, gkr::kMleMaxSub, t, reinterpret_cast<uint64_t*>(R.sums), &dep)) {
                        R.dep = dep;
                        __atomic_store_n(&R.seq, t, __ATOMIC_RELEASE);
                        F.done.store(t, std::memory_order_relaxed);
                        totalled = true;
                    }
                }
                F.busy.store(0u, std::memory_order_release);
                if (!totalled) continue;
                if (G.flag_left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                    uint32_t expect = t;   // (the group's next publishing pass is launched only after these records were read)
                    G.flag_ticket.compare_exchange_strong(expect, 0u, std::memory_order_acq_rel);
                }
                return true;
            }
        }
        return false;
    }
    // the same pass on the host (the group's tables are in h_tail): T'[i] = sum_t w_t T[t S + i], then the sub-block sums of the
    // next rounds into the record the device pass would have written
    void host_fold(PassGroup& G, int jin) {
        using gkr::h64::F;
        advance(G, jin);
        const size_t S = (size_t)1 << G.m, nsub = (size_t)1 << G.j, sub = S >> G.j;
        for (int b = G.b0; b < G.b0 + G.nb; ++b) {
            F* tab = reinterpret_cast<F*>(T.h_tail + ((size_t)b << kMleTailLog2));
            const F* w = reinterpret_cast<const F*>(T.h_w + (size_t)b * gkr::kMleMaxSub);
            for (size_t i = 0; i < S; ++i) {
                gkr::h64::Wide acc = gkr::h64::wide_zero();
                for (size_t t = 0; t < ((size_t)1 << jin); ++t) gkr::h64::wide_mac(acc, tab[t * S + i], w[t]);
                tab[i] = gkr::h64::wide_reduce(acc);
            }
            F* sums = reinterpret_cast<F*>(T.h_rec[b].sums);
            for (size_t a = 0; a < nsub; ++a) {
                F v = tab[a * sub];
                for (size_t i = 1; i < sub; ++i) v = gkr::h64::add(v, tab[a * sub + i]);
                sums[a] = v;
            }
            __atomic_store_n(&T.h_rec[b].seq, G.ticket, __ATOMIC_RELEASE);
        }
    }
    // the J rounds of up to sixteen sumchecks whose sub-block sums have landed
    void process_chunk(const PassGroup& G, int b_first, int count) {
        static const bool scalar_book = gkr::process_switch("GKR_HOST_PASS_SCALAR");   // A/B switch: host_pass_scalar even where the CPU has IFMA
        const int J = G.j, n_out = tail ? tail->n_total : n, r_off = tail ? tail->round_offset : 0;
        uint64_t c0[gkr::kMlePassMaxRounds][16][4], c1[gkr::kMlePassMaxRounds][16][4], r[gkr::kMlePassMaxRounds][16][4];
        uint32_t ln[gkr::kMlePassMaxRounds][16], final_len[16];
        const bool final_pass = G.round0 + J == n;
        for (int i = 0; i < count; ++i) {
            if (G.round0 == 0) dep_last[b_first + i] = tail && tail->dep_last ? tail->dep_last[b_first + i] : T.h_rec[b_first + i].dep;
            final_len[i] = dep_last[b_first + i] ? 2u : 1u;
        }
        static_assert(sizeof(gkr::MleHostRecSub) % 8 == 0, "hand-off records are addressed in 64-bit words");
        const uint64_t* sums = reinterpret_cast<const uint64_t*>(T.h_rec[b_first].sums);
        // (the sums of rounds 6-10 ahead of a two-level first fold: their weights go beside those of rounds 1-5, which the fold needs too)
        uint64_t* weights = G.m - J > 0 ? reinterpret_cast<uint64_t*>((G.mid ? T.h_w2 : T.h_w) + (size_t)b_first * gkr::kMleMaxSub) : nullptr;
        (host_ifma_ready() && count >= 3 && !scalar_book ? gkr::gkr_ifma_pass : host_pass_scalar)(
            sums, sizeof(gkr::MleHostRecSub) / 8, count, J, final_pass ? final_len : nullptr, c0, c1, r, ln, weights, 4 * gkr::kMleMaxSub);
        for (int i = 0; i < count; ++i)
            for (int t = 0; t < J; ++t)
                write_round_output(out_coeffs, out_len, out_r, (size_t)(b_first + i) * n_out + r_off + G.round0 + t, c0[t][i], c1[t][i], ln[t][i], r[t][i]);
    }
    // A hashing thread takes its next chunk from the group that is EARLIEST in its schedule (generation = pass number):
    // the hashes of an early pass release the next streaming pass, whose results are most of the host work still to
    // come, while the late passes' hashes release microseconds of GPU work -- they fill the time in between.
    bool try_work() {
        for (;;) {
            int best = -1;
            uint32_t best_gen = 0;
            for (int g = 0; g < sc.groups; ++g)
                if (const uint32_t gen = grp[g].open_generation(); gen && (best < 0 || gen < best_gen)) best = g, best_gen = gen;
            if (best < 0) return try_total();   // (hashes first: they release the next launch)
            PassGroup& G = grp[best];
            uint32_t first, take;
            if (!G.try_claim(sc.chunk[best], &first, &take)) continue;   // the others took the rest meanwhile: look again
            const double t_in = clock.on ? clock.us() : 0.0;
            process_chunk(G, G.b0 + (int)first, (int)take);
            G.finish(take);
            if (clock.on) clock.busy_ns.fetch_add((uint64_t)((clock.us() - t_in) * 1e3), std::memory_order_relaxed);
            return true;
        }
    }
    // the device-hashed sumchecks [0, n_dev): their whole chain is queued here, on its own stream
    int queue_device_chain() {
        const int n_dev = sc.n_dev;
        HIP_TRY(ctx, ctx->chain_stream(&chain));
        uint32_t* dep_dev = nullptr;
        WS(ctx, "mlep.dev_dep", uint32_t, (size_t)n_dev, dep_dev);
        HIP_TRY(ctx, ctx->pinned_host("mlep.stage_c", sizeof(gkr_fr) * 2 * (size_t)n_dev * n, reinterpret_cast<void**>(&stage_c)));
        HIP_TRY(ctx, ctx->pinned_host("mlep.stage_r", sizeof(gkr_fr) * (size_t)n_dev * n, reinterpret_cast<void**>(&stage_r)));
        HIP_TRY(ctx, ctx->pinned_host("mlep.stage_len", sizeof(uint32_t) * (size_t)n_dev * n, reinterpret_cast<void**>(&stage_len)));
        PassGroup dev;
        dev.nb = n_dev;
        dev.m = n;
        dev.j = sc.j_first;
        dev.index = sc.groups;
        dev.chain = chain;
        launch_first(dev);
        for (bool first = true;; first = false) {
            const int J = dev.j;
            {
                Timed t(ctx, "mle_pass_hash_dev", 0.0, chain);
                gkr::launch_mle_pass_hash_lanes(T.rec, (uint32_t)n_dev, (uint32_t)J, (uint32_t)dev.round0, (uint32_t)n, dev.round0 + J == n, first, ctx->d_cts,
                                                dep_dev, dev.m - J > 0 ? T.h_w : nullptr, reinterpret_cast<Fr*>(stage_c), stage_len,
                                                reinterpret_cast<Fr*>(stage_r), chain);
            }
            if (dev.m - J <= 0) return GKR_OK;
            launch_fold(dev, J);
        }
    }
    // one look at a group by the driving thread; true: it moved on
    bool step(PassGroup& G, int& active) {
        if (G.state == 0 && G.records_landed(T.h_rec)) {
            G.open((uint32_t)++G.pass);
            return true;
        }
        if (G.state != 1 || !G.all_done()) return false;
        if (G.m - G.j > 0) {
            const bool first_fold = G.m == n;
            if (first_fold && two_level(G) && !G.mid) {
                launch_fine_sums(G);
                G.state = 0;
                return true;
            }
            if (first_fold && two_level(G))
                launch_fold2(G);
            else if (G.on_host)
                host_fold(G, G.j);
            else
                launch_fold(G, G.j);
            G.state = 0;
            if (first_fold) launch_next_first();
        } else {
            G.state = 2;
            --active;
            launch_next_first();   // single-pass sumchecks: no fold to ride on
        }
        return true;
    }
    int loop() {
        int rc = GKR_OK, active = sc.groups;
        HandoffWatch watch{ctx, s, "pass"};
        while (active > 0 && rc == GKR_OK) {
            bool progress = false;
            for (int g = 0; g < next_first; ++g) progress |= step(grp[g], active);
            if (order_err != hipSuccess)
                rc = ctx->hip_fail(order_err, "ordering a launch behind a publishing pass");
            else if (progress)
                rc = watch.progressed();
            else if (!try_work())
                rc = watch.idled();
        }
        return rc;
    }
};
}  // namespace

// Host transcript, default schedule (kernels.hip "Multi-round passes"): a pass hands the host the
// 2^J sub-block sums of the current table; the host runs J rounds on them (J <= 5 hashes in a row,
// eight or sixteen sumchecks per IFMA call), derives the 2^J fold weights, and the next pass binds all J
// variables at once.  Length rules as in run_mle_batch.
// Tables of 2^18 .. 2^24 points (MleSchedule::two_level): the first fold binds TEN variables in its one read of the table -- the
// host hashes rounds 1-5, the device forms the sums of rounds 6-10 from pass 0's partials and those weights (launch_fine_sums),
// the host hashes rounds 6-10, then the fold (launch_fold2) -- so that n = 20 is 10 | 5 | 5 instead of 5 | 3 | 5 | 5 | 2.
int run_mle_batch_passes(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                         const MleTailArgs* tail) {
    MlePassRun R{ctx, n, batch, tail, out_coeffs, out_len, out_r};
    const size_t len = (size_t)1 << n;
    hipStream_t s = R.s = R.late = ctx->stream;
    gkr::SpinPool* pool = ctx->host_pool();
    const gkr::Options* o = gkr::current_options();
    const MleSchedule& sc = R.sc = mle_schedule(n, batch, pool->workers() + 1, tail != nullptr, o ? *o : gkr::default_options());
    if (int rc = mle_pass_tables(ctx, "mlep", d_tables, len, len >> sc.j_first, batch, R.T)) return rc;
    if (int rc = mle_arrival_counters(ctx, len, R.T)) return rc;
    if (sc.two_level) {
        HIP_TRY(ctx, ctx->pinned_host("mlep.w2", sizeof(Fr) * gkr::kMleMaxSub * batch, reinterpret_cast<void**>(&R.T.h_w2)));
        WS(ctx, "mlep.d_w2", Fr, (size_t)batch * gkr::kMleMaxSub, R.T.d_w2);
    }
    // Flag-in-word records (mle_flag_records): the pass's blocks publish their sums themselves and the hashing threads total them
    if (mle_flag_records(sc)) {
        HIP_TRY(ctx, ctx->pinned_host("mlep.flag", sizeof(uint64_t) * gkr::kFlagRecWords * gkr::kFlagRecsPerTable * batch, reinterpret_cast<void**>(&R.T.h_flag)));
        R.scan.reset(new FlagScan[batch]);
    }
    HIP_TRY(ctx, ctx->aux_stream(sc.groups));
    if (R.scan) HIP_TRY(ctx, ctx->stream_end_events(sc.groups));
    if (sc.tail_on) HIP_TRY(ctx, ctx->pinned_host("mlep.tail", sizeof(Fr) * ((size_t)batch << kMleTailLog2), reinterpret_cast<void**>(&R.T.h_tail)));
    if (mle_late_stream(sc)) HIP_TRY(ctx, ctx->late_stream(&R.late));
    R.dep_last = std::vector<uint32_t>(batch, 0);
    R.grp = std::vector<PassGroup>(sc.groups);
    for (int g = 0; g < sc.groups; ++g) {
        PassGroup& G = R.grp[g];
        G.index = g;
        G.b0 = sc.bound[g];
        G.nb = sc.bound[g + 1] - sc.bound[g];
        G.m = n;
        G.j = sc.j_first;
    }
    const std::function<bool()> try_work = [&R] { return R.try_work(); };
    R.clock.a = R.clock.us();
    gkr::SpinPool::Session session(pool, &try_work);
    R.launch_next_first();   // (the host's first sums before the device chain's first pass)
    if (sc.n_dev)
        if (int rc = R.queue_device_chain()) return rc;
    while (R.next_first < sc.groups && R.next_first < sc.depth) R.launch_next_first();
    R.clock.b = R.clock.us();
    const int rc = R.loop();
    R.clock.c = R.clock.us();
    session.close();
    if (rc) {   // wait for every stream the call used
        (void)hipStreamSynchronize(s);
        if (R.late != s) (void)hipStreamSynchronize(R.late);
        if (R.chain) (void)hipStreamSynchronize(R.chain);
        ctx->mle_arrivals_zeroed = nullptr;   // (a pass that was given up may have left its counters half way)
        return rc;
    }
    R.clock.d = R.clock.us();
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (R.late != s) HIP_TRY(ctx, hipStreamSynchronize(R.late));
    if (sc.n_dev) {
        HIP_TRY(ctx, hipStreamSynchronize(R.chain));
        // (tail == nullptr here: n_out = n, r_off = 0 -- the staging arrays have the caller's layout)
        memcpy(out_coeffs, R.stage_c, sizeof(gkr_fr) * 2 * (size_t)sc.n_dev * n);
        memcpy(out_r, R.stage_r, sizeof(gkr_fr) * (size_t)sc.n_dev * n);
        memcpy(out_len, R.stage_len, sizeof(uint32_t) * (size_t)sc.n_dev * n);
    }
    R.clock.e = R.clock.us();
    if (ctx->pending.size() > 8192) ctx->drain_events();   // otherwise when the profile is read
    R.clock.report(pool->workers() + 1);
    return GKR_OK;
}

// One rank's run of a sumcheck split over ranks.  Everything that can fail locally is set up BEFORE the first exchange; from
// there on a failure is carried through the remaining exchanges as a flag (rc), so that no rank is left waiting inside a collective.
namespace {
struct MleShardRun {
    gkr_ctx* ctx;
    const gkr_exchange_dev* exchange;
    const int n, batch;
    gkr_fr* out_coeffs;
    uint32_t* out_len;
    gkr_fr* out_r;
    MlePassTables T;   // (rec: device records -- a pass's sums go through the exchange before the host sees them in h_rec)
    uint32_t* h_fail = nullptr;
    std::vector<uint32_t> dep_last;
    gkr::SpinPool* pool = nullptr;
    int rc = GKR_OK;   // this rank's own failure
    uint32_t exchanges = 0;

    long long* limbs() const { return reinterpret_cast<long long*>(exchange->d_limbs); }
    void hook_failed(int arc) {
        if (arc && !rc) rc = ctx->fail(GKR_ERR_INVALID, "the device sum-over-ranks hook failed (status " + std::to_string(arc) + ")");
    }
    bool some_rank_failed() const { return __atomic_load_n(h_fail, __ATOMIC_ACQUIRE) != 0; }
    void exchange_sums(int J, uint32_t ticket) {
        hipStream_t s = ctx->stream;
        Timed t(ctx, "exchange", 0.0);
        gkr::launch_mle_xwiden(T.rec, (uint32_t)J, (uint32_t)batch, rc ? 1u : 0u, limbs(), s);
        const int arc = exchange->fn(exchange->user, (size_t)batch * (((size_t)1 << J) + 2) * 8, static_cast<void*>(s));
        gkr::launch_mle_xnarrow(limbs(), (uint32_t)J, (uint32_t)batch, T.h_rec, ticket, h_fail, s);
        ++exchanges;
        hook_failed(arc);
    }
    // the 2^m entries every shard has left (rows `stride` apart) -> the tail table of 2^(m + lp) entries, on every rank
    void gather_tail(const Fr* rest, size_t stride, int m, int lp, int shard, Fr* d_tail) {
        hipStream_t s = ctx->stream;
        Timed t(ctx, "exchange", 0.0);
        gkr::launch_mle_gather_widen(rest, stride, (uint32_t)m, (uint32_t)lp, (uint32_t)shard, rc ? 1u : 0u, (uint32_t)batch, limbs(), s);
        const int arc = exchange->fn(exchange->user, ((size_t)batch << (m + lp)) * 8 + 8, static_cast<void*>(s));
        gkr::launch_mle_gather_narrow(limbs(), (uint32_t)(m + lp), (uint32_t)batch, d_tail, h_fail, s);
        ++exchanges;
        hook_failed(arc);
    }
    // a chunk of sixteen tables: their J rounds on the summed sub-block sums (the same on every rank), and the fold weights
    void rounds_chunk(int first, int J, int round0) {
        const int count = batch - first < 16 ? batch - first : 16;
        uint64_t c0[gkr::kMlePassMaxRounds][16][4], c1[gkr::kMlePassMaxRounds][16][4], r[gkr::kMlePassMaxRounds][16][4];
        uint32_t ln[gkr::kMlePassMaxRounds][16];
        (host_ifma_ready() && count >= 3 ? gkr::gkr_ifma_pass : host_pass_scalar)(
            reinterpret_cast<const uint64_t*>(T.h_rec[first].sums), sizeof(gkr::MleHostRecSub) / 8, count, J, nullptr, c0, c1, r, ln,
            reinterpret_cast<uint64_t*>(T.h_w + (size_t)first * gkr::kMleMaxSub), 4 * gkr::kMleMaxSub);
        for (int i = 0; i < count; ++i) {
            if (round0 == 0) dep_last[first + i] = T.h_rec[first + i].dep;
            for (int t = 0; t < J; ++t)
                write_round_output(out_coeffs, out_len, out_r, (size_t)(first + i) * n + round0 + t, c0[t][i], c1[t][i], ln[t][i], r[t][i]);
        }
    }
    void host_rounds(int J, int round0) {
        std::atomic<int> next{0};
        const std::function<bool()> work_fn = [&]() -> bool {
            const int first = next.fetch_add(16, std::memory_order_relaxed);
            if (first < batch) rounds_chunk(first, J, round0);
            return first < batch;
        };
        gkr::SpinPool::Session session(pool, nullptr);
        run_pieces(pool, &work_fn, batch > 16);
    }
    // one pass (its launches only while this rank is well), its exchange, its rounds
    void pass(bool pass0, bool from_input, int m_src, int jin, int J, int round0) {
        const uint32_t ticket = gkr::next_ticket(ctx->ticket);
        if (!rc) {
            MlePassPolicy P;   // (no pass publishes from its last block: arrivals == nullptr; the plan on the pass's own stream)
            P.row = pass0 ? "mle_sub_sums" : "mle_multifold";
            if (pass0)
                queue_pass0(ctx, T, 0, batch, J, ticket, ctx->stream, P);
            else
                queue_fold(ctx, T, 0, batch, from_input, m_src, jin, J, ticket, ctx->stream, P);
            if (hipError_t le = hipGetLastError(); le != hipSuccess) rc = ctx->hip_fail(le, "launch of a sumcheck pass");
        }
        exchange_sums(J, ticket);
        if (!rc) rc = wait_records(ctx, T.h_rec, batch, ticket);
        if (!rc && some_rank_failed()) rc = ctx->fail(GKR_ERR_HIP, "another rank failed during the sumcheck");
        if (!rc) host_rounds(J, round0);
    }
};
}  // namespace

}  // namespace gkr_host

extern "C" {

// ---- the launch plan of the multi-round driver, without a device (mle_plan above)
int gkr_selftest_mle_plan(int n, int batch, int hash_threads, const char* const* option_names, const long long* option_values, size_t n_options,
                          uint32_t* header, uint32_t* rows, size_t row_capacity, size_t* n_rows) {
    if ((n_options && (!option_names || !option_values)) || hash_threads > 256) return GKR_ERR_INVALID;
    gkr::Options o;
    for (int i = 0; i < gkr::OPT_COUNT; ++i) o.v[i] = gkr::option_table()[i].def;
    for (size_t i = 0; i < n_options; ++i) {
        const int at = gkr::option_index(option_names[i]);
        if (at < 0) return GKR_ERR_INVALID;
        o.v[at] = option_values[i];
    }
    gkr::OptionScope scope(&o);
    return mle_plan(n, batch, hash_threads, header, rows, row_capacity, n_rows);
}

int gkr_selftest_mle_plan_ctx(gkr_ctx* ctx, int n, int batch, uint32_t* header, uint32_t* rows, size_t row_capacity, size_t* n_rows) {
    if (!ctx) return GKR_ERR_INVALID;
    if (ctx->transcript != GKR_TRANSCRIPT_HOST || ctx->options.v[gkr::OPT_mle_per_round])
        return ctx->fail(GKR_ERR_INVALID, "the launch plan is the multi-round driver's: host transcript, option mle_per_round off");
    gkr::OptionScope scope(&ctx->options);
    // (the threads the driver would hash with: its pool's workers and the driving thread)
    const int rc = mle_plan(n, batch, (int)ctx->host_pool()->workers() + 1, header, rows, row_capacity, n_rows);
    return rc ? ctx->fail(rc, "gkr_selftest_mle_plan_ctx: NULL pointer or a shape gkr_sumcheck_mle_batch_device refuses") : GKR_OK;
}

// ---- one plain sumcheck split over ranks, on the multi-round schedule -----------------------------------------------
// prove_sumcheck (sumcheck.rs:158-214) with the reduce over the hypercube (the rayon reduce of :62) split over P = 2^lp
// ranks.  Rank p holds, of every table T (2^n entries, variable 1 = most significant index bit), the shard
//     T_p[h * 2 + x_n] = T[h * 2P + 2p + x_n],   h < 2^(n - lp - 1):
// the index bits lp .. 1 are the rank, the last variable stays inside every shard.  Rounds bind the leading variable,
// so every pair (i, i + half) is rank-local while bits of h are bound; the sub-block sums a pass hands the host are
// linear in the table, so the whole table's 2^J sums are the sums over ranks of the shards' -- ONE all-reduce of
// 2^J (+ 2 flags) field elements per pass of J <= 5 rounds (n = 20 on 8 ranks: 3 exchanges + the gather, not 20), queued
// on the library's stream through the caller's gkr_exchange_dev; every rank then runs the same J rounds on the same
// sums and derives the same weights, no broadcast.  When 2^6 entries per shard are left they are gathered (one more
// all-reduce, of zero-padded buffers) into a tail table of 2^(6 + lp) entries on which every rank finishes the last
// rounds redundantly.  "Does T depend on x_n" (the last round's length, sumcheck.rs:206-207) is the OR over ranks of
// a neighbour compare inside each shard -- exact, no shard is compared across ranks.
size_t gkr_exchange_limbs_mle(int n, int log2_shards, int batch) {
    if (n < 2 || log2_shards < 0 || log2_shards > 16 || n - log2_shards < 1 || n - log2_shards > GKR_MAX_MLE_N || batch < 1) return 0;
    const int nl = n - log2_shards, t = nl < kMleShardTailLog2 ? nl : kMleShardTailLog2;
    const size_t per_pass = (size_t)batch * (gkr::kMleMaxSub + 2) * 8, gather = ((size_t)batch << (t + log2_shards)) * 8 + 8;
    return per_pass > gather ? per_pass : gather;
}

int gkr_sumcheck_mle_sharded_dev(gkr_ctx* ctx, const void* d_shards, int n, int log2_shards, int shard, int batch,
                                 const gkr_exchange_dev* exchange, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r,
                                 uint32_t* out_exchanges) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!d_shards || !exchange || !exchange->fn || !exchange->d_limbs || !out_coeffs || !out_len || !out_r || batch < 1 || batch > 65535)
        return ctx->fail(GKR_ERR_INVALID, "null pointer or batch out of range [1, 65535]");
    const int lp = log2_shards, nl = n - lp;
    if (lp < 0 || lp > 16 || shard < 0 || shard >= (1 << lp)) return ctx->fail(GKR_ERR_INVALID, "shard must be in [0, 2^log2_shards), log2_shards in [0, 16]");
    if (n < 2 || nl < 1 || nl > GKR_MAX_MLE_N) return ctx->fail(GKR_ERR_INVALID, "n >= 2 and 1 <= n - log2_shards <= GKR_MAX_MLE_N needed");
    if (ctx->transcript != GKR_TRANSCRIPT_HOST) return ctx->fail(GKR_ERR_INVALID, "a sumcheck split over ranks needs the host transcript");
    if (exchange->capacity < gkr_exchange_limbs_mle(n, lp, batch)) return ctx->fail(GKR_ERR_INVALID, "the exchange buffer is smaller than gkr_exchange_limbs_mle(n, log2_shards, batch) int64");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    const size_t len = (size_t)1 << nl;
    const int t_stop = nl < kMleShardTailLog2 ? nl : kMleShardTailLog2;   // variables every shard keeps for the gathered tail
    const int jmax = gkr::opt(gkr::OPT_no_mfma_fold) ? 3 : gkr::kMlePassMaxRounds;
    auto rounds_for = [&](int m) {
        int j = mle_pass_rounds(m, nl, jmax);
        if (m - j < t_stop) j = m - t_stop;
        return j;
    };
    MleShardRun R{ctx, exchange, n, batch, out_coeffs, out_len, out_r};
    MlePassTables& T = R.T;
    Fr* d_tail = nullptr;
    const int j_first = nl > t_stop ? rounds_for(nl) : 0;
    if (int rc = mle_pass_tables(ctx, "mlex", static_cast<const Fr*>(d_shards), len, j_first ? len >> j_first : 1, batch, T)) return rc;
    WS(ctx, "mlex.tail", Fr, (size_t)batch << (t_stop + lp), d_tail);
    WS(ctx, "mlex.drec", gkr::MleHostRecSub, (size_t)batch, T.rec);
    HIP_TRY(ctx, ctx->pinned_host("mlex.fail", 64, reinterpret_cast<void**>(&R.h_fail)));
    *R.h_fail = 0;
    R.dep_last = std::vector<uint32_t>(batch, 0);
    R.pool = batch >= 32 ? ctx->host_pool() : nullptr;
    // ---- the rank-local rounds: n - lp - t_stop of them, in passes
    int m = nl, round0 = 0, jin = 0;
    while (m - jin > t_stop) {
        m -= jin;
        const int J = rounds_for(m);
        R.pass(jin == 0, round0 == jin, m + jin, jin, J, round0);   // (pass 0 -- sums only -- and the first fold read the input shards)
        round0 += J;
        jin = J;
    }
    // ---- bind the last pass's variables (2^t_stop entries per shard are left), gather the tail
    m -= jin;
    const bool folded = jin && !R.rc;
    if (folded) {
        MlePassPolicy P;
        P.row = "mle_multifold";
        queue_fold(ctx, T, 0, batch, round0 == jin, m + jin, jin, 1, gkr::next_ticket(ctx->ticket), s, P);   // (one pass so far: its sums came from the input shards)
        if (hipError_t le = hipGetLastError(); le != hipSuccess) R.rc = ctx->hip_fail(le, "launch of the last rank-local fold");
    }
    R.gather_tail(folded ? T.work : T.input, folded ? T.work_len : len, m, lp, shard, d_tail);
    if (out_exchanges) *out_exchanges = R.exchanges;
    {
        const hipError_t se = hipStreamSynchronize(s);   // the tail is complete, the flag has landed
        if (se != hipSuccess && !R.rc) R.rc = ctx->hip_fail(se, "hipStreamSynchronize after the gather");
    }
    if (!R.rc && R.some_rank_failed()) R.rc = ctx->fail(GKR_ERR_HIP, "another rank failed during the sumcheck");
    if (R.rc) return R.rc;
    ctx->drain_events();
    // ---- the last t_stop + lp rounds on the gathered tail, the same on every rank
    MleTailArgs tail;
    tail.n_total = n;
    tail.round_offset = round0;
    tail.dep_last = round0 ? R.dep_last.data() : nullptr;   // (no rank-local round: the tail is the whole table, its own neighbour compare decides)
    return run_mle_batch_passes(ctx, d_tail, m + lp, batch, out_coeffs, out_len, out_r, &tail);
}

}  // extern "C"

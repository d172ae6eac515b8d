// The plain multilinear sumcheck (prove_sumcheck, rust/src/gkr/sumcheck.rs:158-214): the entry points and their dispatch, the
// per-round schedules (host transcript, device transcript), the step-wise sessions.  The multi-round schedule and a table split
// over ranks: capi_mle_passes.hip.  C ABI: include/gkr_amd.h.
#include "capi_internal.h"

namespace gkr_host {

// ------------------------------------------------------------- plain MLE sumcheck, one round per pass
// Length rule of prove_sumcheck (sumcheck.rs:158-214): rounds 1..n-1 drop a zero
// linear coefficient (add_poly, poly.rs:324-327); the last round has two
// coefficients iff the table depends on x_n (no merge, sumcheck.rs:206-207).
//
// Host transcript (option mle_per_round).  The batch is cut into groups that advance through their rounds independently:
//   GPU (one in-order stream):  sums/fold of group g, round j  ->  reduce -> pinned records
//   host workers:               MiMC7 of every sumcheck of a group whose records have landed
//   this thread:                notices landed records, hands them to the workers, launches the
//                               next round of a group as soon as its hashes are done
// so one group's hash-bound late rounds overlap another group's bandwidth-bound early rounds.
// Few, large groups: every group-round costs two launches.  (Measured on MI355X + 16 host CPUs: starting every group at once is best.)
namespace {
struct MleRoundRun {
    struct Group : GroupHandoff {   // (generation of the hand-off = round + 1)
        int round = 0;
    };
    gkr_ctx* ctx;
    const Fr* d_tables;
    const int n, batch;
    gkr_fr* out_coeffs;
    uint32_t* out_len;
    gkr_fr* out_r;
    Fr* work;
    gkr::MlePartial* partials;
    uint32_t max_nblk;
    gkr::MleHostRec* rec = nullptr;
    gkr::FixedMul* h_rtab = nullptr;   // pinned: host writes r_j's multiplier table, the next fold kernel reads it
    std::vector<uint32_t> dep_last;
    std::vector<Group> grp;
    uint32_t chunk_tables = 8;

    void launch_reduce(Group& G, uint32_t nblk) {
        G.ticket = ++ctx->ticket;
        Timed t(ctx, "mle_round_reduce", 0.0);
        gkr::launch_mle_round_reduce(partials + (size_t)G.b0 * max_nblk, nblk, G.nb, rec + G.b0, G.ticket, ctx->stream);
    }
    void launch_round(Group& G, int round) {
        const int b0 = G.b0, nb = G.nb;
        const size_t len = (size_t)1 << n;
        hipStream_t s = ctx->stream;
        gkr::MlePartial* part = partials + (size_t)b0 * max_nblk;
        if (round == 0) {
            const uint32_t h = (uint32_t)(len / 2), nblk = gkr::mle_blocks_per_table(h, nb);
            {
                Timed t(ctx, "mle_sum_first", (double)nb * len * 32.0);
                gkr::launch_mle_sum_first(d_tables + (size_t)b0 * len, len, h, nb, nblk, part, s);
            }
            return launch_reduce(G, nblk);
        }
        const uint32_t q = (uint32_t)(len >> (round + 1));
        const Fr* src = (round == 1) ? d_tables + (size_t)b0 * len : work + (size_t)b0 * (len / 2);
        const size_t src_stride = (round == 1) ? len : len / 2;
        if (q <= gkr::kSmallFoldQuarter) {
            // small table: fold + sums + publish in one launch
            G.ticket = ++ctx->ticket;
            Timed t(ctx, "mle_fold_sum_small", (double)nb * 6.0 * q * 32.0);
            gkr::launch_mle_fold_sum_small(src, src_stride, work + (size_t)b0 * (len / 2), len / 2, q, nb, h_rtab + b0, rec + b0, G.ticket, s);
            return;
        }
        const uint32_t nblk = gkr::mle_blocks_per_table(q, nb);
        {
            Timed t(ctx, "mle_fold_sum", (double)nb * 6.0 * q * 32.0);
            gkr::launch_mle_fold_sum(src, src_stride, work + (size_t)b0 * (len / 2), len / 2, q, nb, nblk, h_rtab + b0, 1, part, s);
        }
        launch_reduce(G, nblk);
    }
    // one sumcheck's round, given its challenge: the outputs, and the multiplier table of the next fold
    void publish(int b, int round, const gkr::h64::F& c0, const gkr::h64::F& c1, uint32_t ln, const gkr::h64::F& r) {
        write_round_output(out_coeffs, out_len, out_r, (size_t)b * n + round, &c0, &c1, ln, &r);
        if (round + 1 < n) gkr::h64::make_fixed_mul(r, h_rtab[b].w);
    }
    // up to sixteen sumchecks of one group: IFMA-lane hash when there are enough lanes to pay
    // for it, the scalar 4x64-bit code otherwise
    void hash_chunk(int b_first, int count, int round) {
        gkr::h64::F c0[kHashChunkMax], c1[kHashChunkMax], r;
        uint32_t ln[kHashChunkMax] = {};
        uint64_t vec[kHashChunkMax][3][4], out[kHashChunkMax][4];
        const bool lanes = host_ifma_ready() && count >= 3;
        if (lanes) memset(vec, 0, sizeof vec);
        for (int i = 0; i < count; ++i) {
            const int b = b_first + i;
            memcpy(&c0[i], &rec[b].c0, 32);
            memcpy(&c1[i], &rec[b].c1, 32);
            if (round == 0) dep_last[b] = rec[b].dep;
            ln[i] = round + 1 < n ? (gkr::h64::is_zero(c1[i]) ? 1u : 2u) : (dep_last[b] ? 2u : 1u);   // the length rule
            memcpy(vec[i][1], &c1[i], 32);
            memcpy(vec[i][2], &c0[i], 32);
        }
        if (lanes) ifma_hash_chunk(vec, ln, count, out);
        for (int i = 0; i < count; ++i) {
            if (lanes)
                memcpy(&r, out[i], 32);
            else
                r = host_multi_hash(reinterpret_cast<const gkr::h64::F*>(vec[i]) + (3 - ln[i]), (int)ln[i], host_mimc_constants64());
            publish(b_first + i, round, c0[i], c1[i], ln[i], r);
        }
    }
    // one unit of work = up to sixteen sumchecks' hashes of the round their group is in, first group first
    bool try_work() {
        for (Group& G : grp) {
            uint32_t first, take, generation;
            if (!G.try_claim(chunk_tables, &first, &take, &generation)) continue;
            hash_chunk(G.b0 + (int)first, (int)take, (int)generation - 1);
            G.finish(take);
            return true;
        }
        return false;
    }
    bool step(Group& G, int& active) {
        if (G.state == 0 && G.records_landed(rec)) {
            G.open((uint32_t)G.round + 1);
            return true;
        }
        if (G.state != 1 || !G.all_done()) return false;
        if (++G.round < n) {
            launch_round(G, G.round);
            G.state = 0;
        } else {
            G.state = 2;
            --active;
        }
        return true;
    }
    int run() {
        hipStream_t s = ctx->stream;
        HIP_TRY(ctx, ctx->pinned_host("mle.rec", sizeof(gkr::MleHostRec) * batch, reinterpret_cast<void**>(&rec)));
        HIP_TRY(ctx, ctx->pinned_host("mle.rtab", sizeof(gkr::FixedMul) * batch, reinterpret_cast<void**>(&h_rtab)));
        dep_last = std::vector<uint32_t>(batch, 0);
        gkr::SpinPool* pool = ctx->host_pool();
        chunk_tables = (uint32_t)hash_chunk_size(batch, pool->workers() + 1);
        int group_size = batch >= 128 ? (batch + 3) / 4 : (batch >= 16 ? (batch + 1) / 2 : batch);
        if (gkr::opt(gkr::OPT_group_size) > 0) group_size = (int)gkr::opt(gkr::OPT_group_size);
        const int groups = std::min((batch + group_size - 1) / group_size, kMaxGroups);
        grp = std::vector<Group>(groups);
        for (int g = 0; g < groups; ++g) {
            grp[g].b0 = (int)((long long)batch * g / groups);
            grp[g].nb = (int)((long long)batch * (g + 1) / groups) - grp[g].b0;
        }
        const std::function<bool()> work_fn = [this] { return try_work(); };
        gkr::SpinPool::Session session(pool, &work_fn);
        int rc = GKR_OK, started = 0, active = groups;
        HandoffWatch watch{ctx, s, "round"};
        while (active > 0 && rc == GKR_OK) {
            bool progress = started < groups;
            if (progress) launch_round(grp[started++], 0);   // one group per turn of the loop
            for (int g = 0; g < started; ++g) progress |= step(grp[g], active);
            if (progress)
                rc = watch.progressed();
            else if (!try_work())   // nothing to schedule: help with the hashing
                rc = watch.idled();
        }
        session.close();
        if (rc) {
            (void)hipStreamSynchronize(s);   // (the only stream this driver uses)
            return rc;
        }
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(s));
        ctx->drain_events();
        return GKR_OK;
    }
};
}  // namespace

// Device transcript: sums (round 1) or fold + sums of the folded table in one pass, then the round's hash on the device
static int run_mle_device_transcript(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, Fr* work, gkr::MlePartial* partials, gkr_fr* out_coeffs,
                                     uint32_t* out_len, gkr_fr* out_r) {
    const size_t len = (size_t)1 << n, rounds = (size_t)batch * n;
    hipStream_t s = ctx->stream;
    Fr *d_coeffs = nullptr, *d_r = nullptr;
    uint32_t *d_len = nullptr, *d_dep = nullptr;
    gkr::FixedMul* d_rtab = nullptr;
    WS(ctx, "mle.coeffs", Fr, rounds * 2, d_coeffs);
    WS(ctx, "mle.r", Fr, rounds, d_r);
    WS(ctx, "mle.rtab", gkr::FixedMul, rounds, d_rtab);
    WS(ctx, "mle.len", uint32_t, rounds, d_len);
    WS(ctx, "mle.dep", uint32_t, batch, d_dep);
    for (int round = 0; round < n; ++round) {
        uint32_t nblk;
        if (round == 0) {   // round 1: sums only
            const uint32_t h = (uint32_t)(len / 2);
            nblk = gkr::mle_blocks_per_table(h, batch);
            Timed t(ctx, "mle_sum_first", (double)batch * len * 32.0);
            gkr::launch_mle_sum_first(d_tables, len, h, batch, nblk, partials, s);
        } else {   // rounds 2..n: fold with r_{j-1}, sum T_j in the same pass
            const uint32_t q = (uint32_t)(len >> (round + 1));   // quarter of the source table
            nblk = gkr::mle_blocks_per_table(q, batch);
            Timed t(ctx, "mle_fold_sum", (double)batch * 6.0 * q * 32.0);
            gkr::launch_mle_fold_sum(round == 1 ? d_tables : work, round == 1 ? len : len / 2, work, len / 2, q, batch, nblk, d_rtab + (round - 1), n,
                                     partials, s);
        }
        Timed t(ctx, "mle_round_hash", 0.0);
        gkr::launch_mle_round_hash(partials, nblk, round, n, batch, ctx->d_cts, d_coeffs, d_len, d_r, d_rtab, d_dep, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_coeffs, d_coeffs, rounds * 2 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_len, d_len, rounds * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipMemcpyAsync(out_r, d_r, rounds * sizeof(Fr), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    ctx->drain_events();
    return GKR_OK;
}

int run_mle_batch(gkr_ctx* ctx, const Fr* d_tables, int n, int batch, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    const size_t len = (size_t)1 << n;
    const bool host_tx = ctx->transcript == GKR_TRANSCRIPT_HOST;
    if (host_tx && !gkr::opt(gkr::OPT_mle_per_round)) return run_mle_batch_passes(ctx, d_tables, n, batch, out_coeffs, out_len, out_r);
    Fr* work = nullptr;
    gkr::MlePartial* partials = nullptr;
    // groups of the host pipeline are smaller than the batch and may use more blocks per table
    const uint32_t max_nblk = gkr::mle_blocks_per_table((uint32_t)(len / 2), 1u);
    WS(ctx, "mle.work", Fr, (size_t)batch * (len / 2), work);
    WS(ctx, "mle.partials", gkr::MlePartial, (size_t)batch * max_nblk, partials);
    if (!host_tx) return run_mle_device_transcript(ctx, d_tables, n, batch, work, partials, out_coeffs, out_len, out_r);
    MleRoundRun R{ctx, d_tables, n, batch, out_coeffs, out_len, out_r, work, partials, max_nblk};
    return R.run();
}

}  // namespace gkr_host

// =========================================================================== C ABI

extern "C" {

// ---- plain multilinear sumcheck -------------------------------------------------

int gkr_sumcheck_mle_batch_device(gkr_ctx* ctx, const void* d_tables, int n, int batch, gkr_fr* out_coeffs,
                                  uint32_t* out_len, gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!d_tables || !out_coeffs || !out_len || !out_r || batch < 1 || batch > 65535)
        return ctx->fail(GKR_ERR_INVALID, "null pointer or batch out of range [1, 65535]");
    if (n < 2 || n > 30) return ctx->fail(GKR_ERR_INVALID, "n must be in [2, 30]");
    GKR_ENTER(ctx);
    return run_mle_batch(ctx, static_cast<const Fr*>(d_tables), n, batch, out_coeffs, out_len, out_r);
}

int gkr_sumcheck_mle(gkr_ctx* ctx, const gkr_fr* table, int n, gkr_fr* out_coeffs, uint32_t* out_len, gkr_fr* out_r) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!table || !out_coeffs || !out_len || !out_r) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (n < 2 || n > 30) return ctx->fail(GKR_ERR_INVALID, "n must be in [2, 30]");
    const size_t len = (size_t)1 << n;
    if (!all_canonical(table, len)) return ctx->fail(GKR_ERR_NON_CANONICAL, "table entry >= r");
    GKR_ENTER(ctx);
    DevBuf<Fr> d;
    HIP_TRY(ctx, d.alloc(len));
    HIP_TRY(ctx, hipMemcpyAsync(d.p, table, len * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    return run_mle_batch(ctx, d.p, n, 1, out_coeffs, out_len, out_r);
}

struct gkr_mle_session {
    int n = 0;                  // variables of this shard's table
    uint32_t round = 0;
    const Fr* input = nullptr;  // not owned
    Fr* work = nullptr;
    gkr::MlePartial* partials = nullptr;
    gkr::MleHostRec* rec = nullptr;
    gkr::FixedMul* rtab = nullptr;
    uint32_t dep = 0;
    bool have_sums = false;
};


// ---- plain MLE sumcheck, step-wise ----

static void free_mle_session(gkr_mle_session* S) {
    if (!S) return;
    if (S->work) (void)hipFree(S->work);
    if (S->partials) (void)hipFree(S->partials);
    if (S->rec) (void)hipHostFree(S->rec);
    if (S->rtab) (void)hipHostFree(S->rtab);
    delete S;
}

// d_table: 2^n entries in device memory (this rank's shard, or the whole table); not modified
int gkr_mle_session_open(gkr_ctx* ctx, const void* d_table, int n, gkr_mle_session** out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!d_table || !out || n < 1 || n > 30) return ctx->fail(GKR_ERR_INVALID, "null pointer or n out of [1, 30]");
    GKR_ENTER(ctx);
    gkr_mle_session* S = new gkr_mle_session();
    S->n = n;
    S->input = static_cast<const Fr*>(d_table);
    const size_t len = (size_t)1 << n;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&S->work), (len / 2 ? len / 2 : 1) * sizeof(Fr));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&S->partials), gkr::kMaxBlocksPerTable * sizeof(gkr::MlePartial));
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&S->rec), sizeof(gkr::MleHostRec), hipHostMallocCoherent | hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&S->rtab), sizeof(gkr::FixedMul), hipHostMallocCoherent | hipHostMallocMapped);
    if (e != hipSuccess) {
        free_mle_session(S);
        return ctx->hip_fail(e, "mle session allocation");
    }
    memset(S->rec, 0, sizeof(gkr::MleHostRec));
    *out = S;
    return GKR_OK;
}

// out = {sum of the low half, sum of the high half} of the current table (canonical);
// *out_dep (first round only, may be null): does this shard's table depend on its own last variable
int gkr_mle_session_sums(gkr_ctx* ctx, gkr_mle_session* S, gkr_fr* out, uint32_t* out_dep) {
    if (!ctx || !S || !out) return GKR_ERR_INVALID;
    if ((int)S->round >= S->n) return ctx->fail(GKR_ERR_INVALID, "no round left in this session");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    if (!S->have_sums) {   // only the very first round computes sums without a fold
        const size_t len = (size_t)1 << S->n;
        const uint32_t h = (uint32_t)(len / 2);
        const uint32_t nblk = gkr::mle_blocks_per_table(h, 1);
        gkr::launch_mle_sum_first(S->input, len, h, 1, nblk, S->partials, s);
        const uint32_t ticket = ++ctx->ticket;
        gkr::launch_mle_round_reduce(S->partials, nblk, 1, S->rec, ticket, s);
        HIP_TRY(ctx, hipGetLastError());
        int rc = wait_records(ctx, S->rec, 1, ticket);
        if (rc) return rc;
        {
            // a 2-entry table has no neighbour pairs inside a half: it depends on its variable iff T[1] != T[0]
            gkr::h64::F d1;
            memcpy(&d1, &S->rec->c1, 32);
            S->dep = S->n == 1 ? (gkr::h64::is_zero(d1) ? 0u : 1u) : S->rec->dep;
        }
        S->have_sums = true;
    }
    gkr::h64::F c0, c1;
    memcpy(&c0, &S->rec->c0, 32);
    memcpy(&c1, &S->rec->c1, 32);
    gkr::h64::F hi = gkr::h64::add(c0, c1);   // the record holds (low sum, high - low)
    memcpy(&out[0], &c0, 32);
    memcpy(&out[1], &hi, 32);
    if (out_dep) *out_dep = S->dep;
    return GKR_OK;
}

// bind the leading variable to r; the sums of the folded table are ready for the next _sums call
int gkr_mle_session_bind(gkr_ctx* ctx, gkr_mle_session* S, const gkr_fr* r) {
    if (!ctx || !S || !r) return GKR_ERR_INVALID;
    if ((int)S->round >= S->n) return ctx->fail(GKR_ERR_INVALID, "no round left in this session");
    if (!all_canonical(r, 1)) return ctx->fail(GKR_ERR_NON_CANONICAL, "r >= modulus");
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    gkr::h64::F r64;
    memcpy(&r64, r, 32);
    gkr::h64::make_fixed_mul(r64, S->rtab->w);
    const size_t len = (size_t)1 << (S->n - S->round);   // current table
    const Fr* src = S->round == 0 ? S->input : S->work;
    if (len == 2) {
        gkr::launch_fold_pair(src, S->work, S->rtab, s);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipStreamSynchronize(s));
    } else {
        const uint32_t q = (uint32_t)(len / 4);
        const uint32_t nblk = gkr::mle_blocks_per_table(q, 1);
        gkr::launch_mle_fold_sum(src, len, S->work, len / 2, q, 1, nblk, S->rtab, 0, S->partials, s);
        const uint32_t ticket = ++ctx->ticket;
        gkr::launch_mle_round_reduce(S->partials, nblk, 1, S->rec, ticket, s);
        HIP_TRY(ctx, hipGetLastError());
        int rc = wait_records(ctx, S->rec, 1, ticket);
        if (rc) return rc;
    }
    S->round += 1;
    return GKR_OK;
}

// the single remaining entry once all n local variables are bound
int gkr_mle_session_value(gkr_ctx* ctx, gkr_mle_session* S, gkr_fr* out) {
    if (!ctx || !S || !out) return GKR_ERR_INVALID;
    if ((int)S->round != S->n) return ctx->fail(GKR_ERR_INVALID, "session still has rounds to run");
    GKR_ENTER(ctx);
    Fr v;
    HIP_TRY(ctx, hipMemcpyAsync(&v, S->work, sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *out = to_abi(v);
    return GKR_OK;
}

void gkr_mle_session_close(gkr_ctx* ctx, gkr_mle_session* S) {
    if (ctx) (void)hipSetDevice(ctx->device);
    free_mle_session(S);
}

// *out_differ = 1 iff the two device tables differ somewhere (a table's dependence on a variable
// that is a rank bit: compare the shards of ranks p and p ^ 1)
int gkr_device_tables_differ(gkr_ctx* ctx, const void* d_a, const void* d_b, size_t count, uint32_t* out_differ) {
    if (!ctx || !d_a || !d_b || !out_differ || !count) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    DevBuf<uint32_t> flag;
    HIP_TRY(ctx, flag.alloc(1));
    HIP_TRY(ctx, hipMemsetAsync(flag.p, 0, 4, ctx->stream));
    gkr::launch_tables_differ(static_cast<const Fr*>(d_a), static_cast<const Fr*>(d_b), count, flag.p, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_differ, flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}


}  // extern "C"

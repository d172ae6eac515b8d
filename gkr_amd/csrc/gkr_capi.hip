// C ABI (include/gkr_amd.h) and host driver of the MI355X GKR sumcheck prover.
//
// Host-side mirror of the reference's prover loop (rust/src/gkr/prover.rs:6-96):
// per layer  predicate build -> 2k sumcheck rounds -> q_i -> r* -> z_{i+1}.
// All table work is launched on the context's HIP stream; the per-round MiMC7
// hash runs on the device by default, so a whole sumcheck is one uninterrupted
// stream of launches with a single copy-back at the end.
#include "capi_internal.h"

// =========================================================================== C ABI

extern "C" {

const char* gkr_strerror(int status) {
    switch (status) {
        case GKR_OK: return "ok";
        case GKR_ERR_INVALID: return "invalid argument";
        case GKR_ERR_NON_CANONICAL: return "field element is not canonical (>= r)";
        case GKR_ERR_NO_DEVICE: return "no gfx950 device available";
        case GKR_ERR_HIP: return "HIP runtime error";
        case GKR_ERR_NOMEM: return "out of memory";
        case GKR_ERR_DEGENERATE: return "degenerate sumcheck (v == 0)";
        case GKR_ERR_UNSUPPORTED: return "R1CS shape the reference's compiler does not support";
        default: return "unknown status";
    }
}

const char* gkr_version(void) { return "gkr_amd 0.1 (gfx950)"; }

int gkr_ctx_create(int device_id, gkr_ctx** out) {
    if (!out) return GKR_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GKR_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return GKR_ERR_INVALID;
    // the calling thread's current device is the caller's business (a host with several GPUs mixes its own HIP calls
    // with the library's): whatever it was, it is current again when this returns
    struct RestoreDevice {
        int prev = -1;
        RestoreDevice() {
            if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        }
        ~RestoreDevice() {
            if (prev >= 0) (void)hipSetDevice(prev);
        }
    } restore_device;
    if (hipSetDevice(device_id) != hipSuccess) return GKR_ERR_HIP;
    gkr_ctx* c = new gkr_ctx();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess)
        snprintf(c->name, sizeof c->name, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return GKR_ERR_HIP;
    }
    if (hipMalloc(reinterpret_cast<void**>(&c->d_cts), sizeof(Fr) * gkr::kMimcRounds) != hipSuccess ||
        hipMemcpy(c->d_cts, host_mimc_constants(), sizeof(Fr) * gkr::kMimcRounds, hipMemcpyHostToDevice) != hipSuccess) {
        gkr_ctx_destroy(c);
        return GKR_ERR_HIP;
    }
    *out = c;
    return GKR_OK;
}

// One host process driving several GPUs -- the reference is ONE process whose par_iter fans prover::prove out over the
// (circuit, input) pairs of a step (aggregator.rs:350-355, 411-416): the context lives on device_ids[0], and
// gkr_prove_many deals its items over child contexts created round-robin on ALL the listed devices (a device may be
// listed more than once: that many child contexts on it per round).  Every other entry point runs on device_ids[0].
int gkr_ctx_create_multi(const int* device_ids, int n_devices, gkr_ctx** out) {
    if (!out) return GKR_ERR_INVALID;
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return GKR_ERR_INVALID;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return GKR_ERR_NO_DEVICE;
    for (int i = 0; i < n_devices; ++i)
        if (device_ids[i] < 0 || device_ids[i] >= count) return GKR_ERR_INVALID;
    gkr_ctx* c = nullptr;
    const int rc = gkr_ctx_create(device_ids[0], &c);
    if (rc) return rc;
    c->devices.assign(device_ids, device_ids + n_devices);
    *out = c;
    return GKR_OK;
}

int gkr_ctx_device_count(const gkr_ctx* ctx) { return ctx ? (ctx->devices.empty() ? 1 : (int)ctx->devices.size()) : 0; }

void gkr_ctx_destroy(gkr_ctx* ctx) {
    if (!ctx) return;
    ctx->crew.reset();   // joins gkr_prove_many's threads and destroys their contexts
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->aux) (void)hipStreamSynchronize(ctx->aux);
    if (ctx->late) (void)hipStreamSynchronize(ctx->late);
    ctx->drain_events();
    ctx->drain_events();
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    ctx->release_buffers();
    if (ctx->d_cts) (void)hipFree(ctx->d_cts);
    for (hipEvent_t e : ctx->aux_events) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ended_events) (void)hipEventDestroy(e);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->late) (void)hipStreamDestroy(ctx->late);
    if (ctx->chain) (void)hipStreamDestroy(ctx->chain);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* gkr_last_error(const gkr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int gkr_ctx_set_transcript(gkr_ctx* ctx, int mode) {
    if (!ctx || (mode != GKR_TRANSCRIPT_DEVICE && mode != GKR_TRANSCRIPT_HOST)) return GKR_ERR_INVALID;
    ctx->transcript = mode;
    return GKR_OK;
}

// ---- options (csrc/options.h: the one table of the library's switches) ----
int gkr_option_count(void) { return (int)gkr::OPT_COUNT; }
const char* gkr_option_name(int index) { return index >= 0 && index < (int)gkr::OPT_COUNT ? gkr::option_table()[index].name : nullptr; }
const char* gkr_option_doc(int index) { return index >= 0 && index < (int)gkr::OPT_COUNT ? gkr::option_table()[index].doc : nullptr; }
const char* gkr_option_env(int index) { return index >= 0 && index < (int)gkr::OPT_COUNT ? gkr::option_table()[index].env : nullptr; }

int gkr_ctx_get_option(const gkr_ctx* ctx, const char* name, long long* value) {
    const int i = gkr::option_index(name);
    if (!ctx || !value || i < 0) return GKR_ERR_INVALID;
    *value = ctx->options.v[i];
    return GKR_OK;
}

int gkr_ctx_set_option(gkr_ctx* ctx, const char* name, long long value) {
    if (!ctx) return GKR_ERR_INVALID;
    const int i = gkr::option_index(name);
    if (i < 0) return ctx->fail(GKR_ERR_INVALID, std::string("unknown option: ") + (name ? name : "(null)"));
    if (ctx->crew_member) return ctx->fail(GKR_ERR_INVALID, "options of a context that is proving are not changed");
    if (ctx->options.v[i] == value) return GKR_OK;
    // Cached per-circuit state (gate lists, segment layout) was built under the old value: dropped, rebuilt on next use.
    // Resident layers (gkr_resident_layer_create) keep the layout they were created with: set options before creating them.
    // gkr_prove_many's child contexts (idle between calls: crew_member stays set on them, their threads wait for the next call)
    // hold PreparedCircuits built under the old value as well, and prove with the options of this context: theirs go too,
    // each on its own device (only the calling context's cache was dropped -- a changed gate_segment_log2 then met
    // cached segment lists of the old shift).
    int prev_device = -1;
    if (hipGetDevice(&prev_device) != hipSuccess) prev_device = -1;
    auto drop_cache = [](gkr_ctx* c) {
        if (hipSetDevice(c->device) != hipSuccess) return;
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->aux) (void)hipStreamSynchronize(c->aux);
        for (auto& pc : c->circuits) pc->release();
        c->circuits.clear();
    };
    drop_cache(ctx);
    ctx->options.v[i] = value;
    if (ctx->crew)
        for (size_t m = 1; m < ctx->crew->members.size(); ++m) {
            gkr_ctx* child = ctx->crew->members[m]->ctx;
            if (!child) continue;
            drop_cache(child);
            child->options = ctx->options;
        }
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
    return GKR_OK;
}

int gkr_ctx_set_host_threads(gkr_ctx* ctx, int threads) {
    if (!ctx || threads < 0 || threads > 256) return GKR_ERR_INVALID;
    if (threads != ctx->host_threads) {
        ctx->pool.reset();   // joins the workers; the next call that needs them starts the new number
        ctx->host_threads = threads;
    }
    return GKR_OK;
}

long gkr_host_help_while(const volatile int32_t* busy) {
    if (!busy) return 0;
    long pieces = 0;
    unsigned idle = 0;
    const bool account = accounting_on();
    const double t0 = account ? now_us_dbg() : 0.0;
    double lent_us = 0;
    while (__atomic_load_n(busy, __ATOMIC_ACQUIRE) != 0) {
        const double th = account ? now_us_dbg() : 0.0;
        if (help_enabled() && gkr::HelpBoard::instance().help()) {
            if (account) lent_us += now_us_dbg() - th;
            ++pieces;
            idle = 0;
            continue;
        }
        GKR_CPU_RELAX();
        if (++idle > 4096) {   // nothing posted for a while: give the core away for a moment rather than spin at full rate
            std::this_thread::yield();
            idle = 0;
        }
    }
    if (account) {
        HostAccountTotals& tot = host_account_totals();
        const double all = now_us_dbg() - t0;
        tot.lent_ns.fetch_add((uint64_t)(lent_us * 1e3), std::memory_order_relaxed);
        tot.lent_idle_ns.fetch_add((uint64_t)((all > lent_us ? all - lent_us : 0) * 1e3), std::memory_order_relaxed);
    }
    return pieces;
}

int gkr_host_accounting(int enable) {
    HostAccountTotals& tot = host_account_totals();
    if (enable) {
        tot.own_ns = 0;
        tot.helped_ns = 0;
        tot.spin_ns = 0;
        tot.rest_ns = 0;
        tot.lent_ns = 0;
        tot.lent_idle_ns = 0;
        tot.calls = 0;
        tot.wake_ns = 0;
        tot.pieces = 0;
        tot.piece_ns = 0;
        tot.piece_pass_ns = 0;
        for (auto& l : tot.lanes) l = 0;
    }
    tot.on.store(enable != 0, std::memory_order_relaxed);
    return GKR_OK;
}

int gkr_host_accounting_read(double* out_us, size_t count) {
    if (!out_us || count < 7) return GKR_ERR_INVALID;
    if (count >= 8) out_us[7] = host_account_totals().wake_ns.load() * 1e-3;
    const HostAccountTotals& tot = host_account_totals();
    out_us[0] = tot.own_ns.load() * 1e-3;
    out_us[1] = tot.helped_ns.load() * 1e-3;
    out_us[2] = tot.spin_ns.load() * 1e-3;
    out_us[3] = tot.rest_ns.load() * 1e-3;
    out_us[4] = tot.lent_ns.load() * 1e-3;
    out_us[5] = tot.lent_idle_ns.load() * 1e-3;
    out_us[6] = (double)tot.calls.load();
    if (count >= 28) {   // the hashing pieces: [8] how many, [9] their time, [10] of it inside the pass function, [11 + n] pieces of n + 1 transcripts
        out_us[8] = (double)tot.pieces.load();
        out_us[9] = tot.piece_ns.load() * 1e-3;
        out_us[10] = tot.piece_pass_ns.load() * 1e-3;
        for (int n = 1; n <= 16; ++n) out_us[10 + n] = (double)tot.lanes[n].load();
        out_us[27] = 0.0;
    }
    return GKR_OK;
}

int gkr_ctx_device_name(const gkr_ctx* ctx, char* buf, size_t len) {
    if (!ctx || !buf || !len) return GKR_ERR_INVALID;
    snprintf(buf, len, "%s", ctx->name);
    return GKR_OK;
}

int gkr_ctx_profile(gkr_ctx* ctx, int enable) {
    if (!ctx) return GKR_ERR_INVALID;
    ctx->profile = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
    return GKR_OK;
}

int gkr_ctx_profile_get(gkr_ctx* ctx, const char* kernel, uint64_t* launches, double* total_ms, double* bytes) {
    if (!ctx || !kernel) return GKR_ERR_INVALID;
    ctx->drain_events();
    auto it = ctx->prof.find(kernel);
    ProfileRow r = it == ctx->prof.end() ? ProfileRow() : it->second;
    if (launches) *launches = r.launches;
    if (total_ms) *total_ms = r.total_ms;
    if (bytes) *bytes = r.bytes;
    return GKR_OK;
}

int gkr_ctx_profile_samples(gkr_ctx* ctx, const char* kernel, double* ms, double* bytes, size_t capacity, size_t* count) {
    if (!ctx || !kernel || !count) return GKR_ERR_INVALID;
    ctx->drain_events();
    auto it = ctx->prof.find(kernel);
    const size_t n = it == ctx->prof.end() ? 0 : it->second.samples.size();
    *count = n;
    for (size_t i = 0; i < n && i < capacity; ++i) {
        if (ms) ms[i] = it->second.samples[i].first;
        if (bytes) bytes[i] = it->second.samples[i].second;
    }
    return GKR_OK;
}

int gkr_ctx_profile_reset(gkr_ctx* ctx) {
    if (!ctx) return GKR_ERR_INVALID;
    ctx->drain_events();
    ctx->prof.clear();
    return GKR_OK;
}

// ---- MiMC7 on the host ------------------------------------------------------

int gkr_mimc7_multi_hash(const gkr_fr* arr, size_t n, const gkr_fr* key, gkr_fr* out) {
    if ((!arr && n) || !out) return GKR_ERR_INVALID;
    if (!all_canonical(arr, n) || (key && !all_canonical(key, 1))) return GKR_ERR_NON_CANONICAL;
    const Fr* cts = host_mimc_constants();
    Fr r = key ? gkr::to_mont(to_dev(*key)) : gkr::fr_zero();
    for (size_t i = 0; i < n; ++i) {
        Fr a = gkr::to_mont(to_dev(arr[i]));
        Fr h = gkr::mimc7_hash_mont(a, r, cts);
        r = gkr::fr_add(gkr::fr_add(r, a), h);
    }
    *out = to_abi(gkr::from_mont(r));
    return GKR_OK;
}

int gkr_mimc7_hash(const gkr_fr* x, const gkr_fr* k, gkr_fr* out) {
    if (!x || !k || !out) return GKR_ERR_INVALID;
    if (!all_canonical(x, 1) || !all_canonical(k, 1)) return GKR_ERR_NON_CANONICAL;
    Fr h = gkr::mimc7_hash_mont(gkr::to_mont(to_dev(*x)), gkr::to_mont(to_dev(*k)), host_mimc_constants());
    *out = to_abi(gkr::from_mont(h));
    return GKR_OK;
}

int gkr_mimc7_constant(int i, gkr_fr* out) {
    if (i < 0 || i >= gkr::kMimcRounds || !out) return GKR_ERR_INVALID;
    *out = to_abi(gkr::from_mont(host_mimc_constants()[i]));
    return GKR_OK;
}

int gkr_selftest_mul(const gkr_fr* a, const gkr_fr* b, gkr_fr* out) {
    if (!a || !b || !out) return GKR_ERR_INVALID;
    if (!all_canonical(a, 1) || !all_canonical(b, 1)) return GKR_ERR_NON_CANONICAL;
    *out = to_abi(gkr::fr_mul(to_dev(*a), to_dev(*b)));
    return GKR_OK;
}

int gkr_selftest_fold(const gkr_fr* lo, const gkr_fr* hi, const gkr_fr* r, gkr_fr* out) {
    if (!lo || !hi || !r || !out) return GKR_ERR_INVALID;
    if (!all_canonical(lo, 1) || !all_canonical(hi, 1) || !all_canonical(r, 1)) return GKR_ERR_NON_CANONICAL;
    // the round's fixed-multiplier table built both ways (8x32-bit and the host's 4x64-bit code) must agree
    const gkr::FixedMul T = gkr::make_fixed_mul(to_dev(*r));
    gkr::FixedMul T64;
    gkr::h64::F r64;
    memcpy(&r64, r, 32);
    gkr::h64::make_fixed_mul(r64, T64.w);
    if (memcmp(&T, &T64, sizeof T) != 0) return GKR_ERR_INVALID;
    const Fr single = gkr::fr_fold_fixed(to_dev(*lo), to_dev(*hi), T);
    Fr y0, y1;   // the paired form the kernels use: (lo, hi) and (hi, lo) together
    gkr::fr_fold_fixed2(to_dev(*lo), to_dev(*hi), to_dev(*hi), to_dev(*lo), T, y0, y1);
    if (!gkr::fr_eq(y0, single) || !gkr::fr_eq(y1, gkr::fr_fold_fixed(to_dev(*hi), to_dev(*lo), T))) return GKR_ERR_INVALID;
    *out = to_abi(single);
    return GKR_OK;
}

// the pass schedule of a 2^n-point sumcheck (host logic only): rounds[i] = rounds covered by pass i, *passes = how many.
// mfma != 0: the matrix-core fold's schedule (up to 5 rounds per pass), 0: the v_mad_u64_u32 fold's (up to 3).  mfma == 2: with the
// first fold at two levels where it applies (18 <= n <= 24: 10 | 5 | ..., the ten rounds of the sweep reported as one entry) --
// what a batch of host-hashed sumchecks runs under option first_fold_levels = 2.
int gkr_selftest_pass_schedule(int n, int mfma, uint32_t* rounds, size_t capacity, size_t* passes) {
    if (n < 1 || n > 40 || !passes) return GKR_ERR_INVALID;
    const int jmax = mfma ? gkr::kMlePassMaxRounds : 3;
    gkr::Options two = gkr::default_options();
    two.v[gkr::OPT_first_fold_levels] = 2;
    two.v[gkr::OPT_no_mfma_fold] = two.v[gkr::OPT_rounds_per_pass] = 0;
    const bool two_level = mfma == 2 && mle_two_level_first_fold(n, two);
    size_t count = 0;
    for (int m = n; m > 0;) {
        // (behind the two-level fold one pass of five rounds: its partials are fine enough at every n it takes)
        const int j = two_level && m == n ? kMleTwoLevelRounds : (two_level && m == n - kMleTwoLevelRounds ? gkr::kMlePassMaxRounds : mle_pass_rounds(m, n, jmax));
        if (rounds && count < capacity) rounds[count] = (uint32_t)j;
        ++count;
        m -= j;
    }
    *passes = count;
    return (rounds && count > capacity) ? GKR_ERR_NOMEM : GKR_OK;
}

// The host's share of one multi-round pass (host logic only): `count` <= 16 sumchecks, each with 2^J sub-block sums
// (rows of 32: sums[k * 32 + b]) -> per round t < J the coefficients c0[t * count + k], c1[..], the vector length
// len[..] (final_len non-null: the last round's lengths are given, as in a sumcheck's final round), the challenge
// r[..]; and w[k * 32 + b], b < 2^J: the weights eq((r_0..r_{J-1}), b) of the fold pass that follows, canonical.
// Scalar code always; the IFMA-lane form runs beside it when the CPU has it (*used_ifma = 1) and any difference is
// GKR_ERR_INVALID.
int gkr_selftest_host_pass(const gkr_fr* sums, int count, int J, const uint32_t* final_len, gkr_fr* c0, gkr_fr* c1, uint32_t* len,
                           gkr_fr* r, gkr_fr* w, int* used_ifma) {
    using gkr::h64::F;
    if (!sums || !c0 || !c1 || !len || !r || !w || count < 1 || count > kHashChunkMax || J < 1 || J > gkr::kMlePassMaxRounds)
        return GKR_ERR_INVALID;
    static_assert(gkr::kMleMaxSub == 32 && kHashChunkMax == 16, "shapes of the self-test's arrays");
    if (!all_canonical(sums, (size_t)count * 32)) return GKR_ERR_NON_CANONICAL;
    if (final_len)
        for (int k = 0; k < count; ++k)
            if (final_len[k] != 1 && final_len[k] != 2) return GKR_ERR_INVALID;
    struct Out {
        uint64_t c0[gkr::kMlePassMaxRounds][16][4], c1[gkr::kMlePassMaxRounds][16][4], r[gkr::kMlePassMaxRounds][16][4];
        uint32_t len[gkr::kMlePassMaxRounds][16];
        std::vector<F> w;
    } a, b;
    a.w.assign((size_t)count * 32, F{{0, 0, 0, 0}});
    host_pass_scalar(reinterpret_cast<const uint64_t*>(sums), 4 * 32, count, J, final_len, a.c0, a.c1, a.r, a.len, &a.w[0].l[0], 4 * 32);
    const bool ifma = host_ifma_ready();
    if (used_ifma) *used_ifma = ifma ? 1 : 0;
    if (ifma) {
        b.w.assign((size_t)count * 32, F{{0, 0, 0, 0}});
        gkr::gkr_ifma_pass(reinterpret_cast<const uint64_t*>(sums), 4 * 32, count, J, final_len, b.c0, b.c1, b.r, b.len, &b.w[0].l[0], 4 * 32);
        for (int t = 0; t < J; ++t)
            for (int k = 0; k < count; ++k)
                if (memcmp(a.c0[t][k], b.c0[t][k], 32) || memcmp(a.c1[t][k], b.c1[t][k], 32) || memcmp(a.r[t][k], b.r[t][k], 32) ||
                    a.len[t][k] != b.len[t][k])
                    return GKR_ERR_INVALID;
        if (memcmp(a.w.data(), b.w.data(), sizeof(F) * a.w.size()) != 0) return GKR_ERR_INVALID;
    }
    for (int t = 0; t < J; ++t)
        for (int k = 0; k < count; ++k) {
            memcpy(&c0[(size_t)t * count + k], a.c0[t][k], 32);
            memcpy(&c1[(size_t)t * count + k], a.c1[t][k], 32);
            memcpy(&r[(size_t)t * count + k], a.r[t][k], 32);
            len[(size_t)t * count + k] = a.len[t][k];
        }
    for (size_t i = 0; i < a.w.size(); ++i) {
        const F wc = gkr::h64::from_mont(a.w[i]);
        memcpy(&w[i], &wc, 32);
    }
    return GKR_OK;
}

// The host's share of one product pass of the layer sumcheck (host logic only): `count` <= 16 sumchecks; recs: per
// sumcheck 72 values (cross sums m[a * 8 + b], a, b < 2^J, then the Y sums at 64 + a); vec_len[t * count + k]: 2 or 3.
// -> per round t < J (index t * count + k) the coefficients c2, lin, c0 and the challenge; w[k * 8 + b], b < 2^J: the
// weights eq(r, b) of the fold that follows, canonical.  Scalar code always; the IFMA-lane form runs beside it when
// the CPU has it (*used_ifma = 1) and any difference is GKR_ERR_INVALID.
int gkr_selftest_host_prod_pass(const gkr_fr* recs, int count, int J, const uint32_t* vec_len, gkr_fr* c2, gkr_fr* lin, gkr_fr* c0,
                                gkr_fr* r, gkr_fr* w, int* used_ifma) {
    using gkr::h64::F;
    if (!recs || !vec_len || !c2 || !lin || !c0 || !r || !w || count < 1 || count > kHashChunkMax || J < 1 || J > gkr::kProdMaxJ)
        return GKR_ERR_INVALID;
    if (!all_canonical(recs, (size_t)count * gkr::kProdRecValues)) return GKR_ERR_NON_CANONICAL;
    uint32_t vl[gkr::kProdMaxJ][16] = {};
    for (int t = 0; t < J; ++t)
        for (int k = 0; k < count; ++k) {
            vl[t][k] = vec_len[(size_t)t * count + k];
            if (vl[t][k] != 2 && vl[t][k] != 3) return GKR_ERR_INVALID;
        }
    struct Out {
        uint64_t c2[gkr::kProdMaxJ][16][4], lin[gkr::kProdMaxJ][16][4], c0[gkr::kProdMaxJ][16][4], r[gkr::kProdMaxJ][16][4];
        F w[16][8];
    } a, b;
    memset(&a, 0, sizeof a);
    memset(&b, 0, sizeof b);
    host_prod_pass_scalar(reinterpret_cast<const uint64_t*>(recs), 4 * gkr::kProdRecValues, count, J, vl, a.c2, a.lin, a.c0, a.r, &a.w[0][0].l[0], 32);
    const bool ifma = host_ifma_ready();
    if (used_ifma) *used_ifma = ifma ? 1 : 0;
    if (ifma) {
        gkr::gkr_ifma_prod_pass(reinterpret_cast<const uint64_t*>(recs), 4 * gkr::kProdRecValues, count, J, vl, b.c2, b.lin, b.c0, b.r, &b.w[0][0].l[0], 32);
        for (int t = 0; t < J; ++t)
            for (int k = 0; k < count; ++k)
                if (memcmp(a.c2[t][k], b.c2[t][k], 32) || memcmp(a.lin[t][k], b.lin[t][k], 32) || memcmp(a.c0[t][k], b.c0[t][k], 32) ||
                    memcmp(a.r[t][k], b.r[t][k], 32))
                    return GKR_ERR_INVALID;
        for (int k = 0; k < count; ++k)
            if (memcmp(a.w[k], b.w[k], sizeof(F) << J) != 0) return GKR_ERR_INVALID;
    }
    for (int t = 0; t < J; ++t)
        for (int k = 0; k < count; ++k) {
            memcpy(&c2[(size_t)t * count + k], a.c2[t][k], 32);
            memcpy(&lin[(size_t)t * count + k], a.lin[t][k], 32);
            memcpy(&c0[(size_t)t * count + k], a.c0[t][k], 32);
            memcpy(&r[(size_t)t * count + k], a.r[t][k], 32);
        }
    for (int k = 0; k < count; ++k)
        for (int bb = 0; bb < 8; ++bb) {
            const F wc = bb < (1 << J) ? gkr::h64::from_mont(a.w[k][bb]) : F{{0, 0, 0, 0}};
            memcpy(&w[(size_t)k * 8 + bb], &wc, 32);
        }
    return GKR_OK;
}

// the host tail of a phase's product passes (capi_layer.hip, host_tail_pass) on tables the caller gives: W, X, Y of 2^m canonical
// entries each, the previous pass's 2^jp canonical weights (jp = 0: none), the next pass's J rounds -> the 72 values of the
// record the device pass would have left (cross sums of the folded tables' 2^J sub-blocks, then the sub-block sums of Y)
int gkr_selftest_host_tail(const gkr_fr* tables, int m, int jp, const gkr_fr* weights, int J, gkr_fr* rec, int* used_ifma) {
    using gkr::h64::F;
    if (!tables || !rec || m < 0 || m > 12 || jp < 0 || jp > gkr::kProdMaxJ || jp > m || J < 1 || J > gkr::kProdMaxJ || J > m - jp || (jp && !weights))
        return GKR_ERR_INVALID;
    const size_t len = (size_t)1 << m;
    if (!all_canonical(tables, 3 * len) || (jp && !all_canonical(weights, (size_t)1 << jp))) return GKR_ERR_NON_CANONICAL;
    std::vector<F> t(3 * len);
    memcpy(t.data(), tables, sizeof(F) * 3 * len);
    for (size_t i = 0; i < len; ++i) t[i] = gkr::h64::to_mont(t[i]);   // W is in Montgomery form on the device, and stays so
    F w[8] = {};
    for (int b = 0; jp && b < (1 << jp); ++b) {   // (jp = 0: nothing pending, no weights)
        memcpy(&w[b], &weights[b], sizeof(F));
        w[b] = gkr::h64::to_mont(w[b]);
    }
    F out[gkr::kProdRecValues] = {};
    const bool ifma = host_ifma_ready();
    if (used_ifma) *used_ifma = ifma ? 1 : 0;
    if (ifma) {   // the eight-lane form beside the scalar one: the same record and the same folded tables
        std::vector<F> t2(t);
        F out2[gkr::kProdRecValues] = {};
        gkr::gkr_ifma_tail_pass(&t2[0].l[0], len, (uint32_t)m, (uint32_t)jp, &w[0].l[0], (uint32_t)J, &out2[0].l[0]);
        host_tail_pass_scalar(t.data(), len, (uint32_t)m, (uint32_t)jp, w, (uint32_t)J, out);
        const size_t folded = (size_t)1 << (m - jp);
        for (int tb = 0; tb < 3; ++tb)
            if (memcmp(&t[(size_t)tb * len], &t2[(size_t)tb * len], folded * sizeof(F)) != 0) return GKR_ERR_INVALID;
        const int n = 1 << J;
        for (int a = 0; a < n; ++a) {
            if (memcmp(&out[a * 8], &out2[a * 8], sizeof(F) * n) != 0) return GKR_ERR_INVALID;
            if (memcmp(&out[64 + a], &out2[64 + a], sizeof(F)) != 0) return GKR_ERR_INVALID;
        }
    } else {
        host_tail_pass_scalar(t.data(), len, (uint32_t)m, (uint32_t)jp, w, (uint32_t)J, out);
    }
    memcpy(rec, out, sizeof out);
    return GKR_OK;
}

// eight right-aligned round vectors (3 slots each, the last len[k] slots count) hashed the way the
// host transcript does: the eight-lane IFMA code when the CPU has it (*used_ifma = 1; its sixteen-lane
// form is cross-checked on the way), else scalar
int gkr_selftest_hash8(const gkr_fr* vecs, const uint32_t* len, gkr_fr* out, int* used_ifma) {
    if (!vecs || !len || !out) return GKR_ERR_INVALID;
    if (!all_canonical(vecs, 24)) return GKR_ERR_NON_CANONICAL;
    for (int k = 0; k < 8; ++k)
        if (len[k] > 3) return GKR_ERR_INVALID;
    const bool ifma = host_ifma_ready();
    if (used_ifma) *used_ifma = ifma ? 1 : 0;
    if (ifma) {
        uint64_t v[8][3][4], o[8][4];
        memcpy(v, vecs, sizeof v);
        gkr::gkr_ifma_multi_hash8(v, len, 3, o);
        memcpy(out, o, sizeof o);
        // the sixteen-lane interleaved form on the same vectors (second half in reverse order) must agree
        uint64_t v16[16][3][4], o16[16][4];
        uint32_t len16[16];
        for (int k = 0; k < 8; ++k) {
            memcpy(v16[k], v[k], sizeof v[k]);
            memcpy(v16[15 - k], v[k], sizeof v[k]);
            len16[k] = len16[15 - k] = len[k];
        }
        gkr::gkr_ifma_multi_hash16(v16, len16, 3, o16);
        for (int k = 0; k < 8; ++k)
            if (memcmp(o16[k], o[k], 32) != 0 || memcmp(o16[15 - k], o[k], 32) != 0) return GKR_ERR_INVALID;
    } else {
        const gkr::h64::F* cts = host_mimc_constants64();
        for (int k = 0; k < 8; ++k) {
            gkr::h64::F v[3];
            memcpy(v, vecs + 3 * k, 96);
            const gkr::h64::F r = host_multi_hash(v + (3 - len[k]), (int)len[k], cts);
            memcpy(&out[k], &r, 32);
        }
    }
    return GKR_OK;
}

// the transcript's own ceiling on this host: microseconds per MiMC7 multi_hash of a `len`-element round vector (len 2:
// plain sumcheck; 3: layer sumcheck) on one thread -- sixteen transcripts side by side in IFMA lanes (per hash, i.e.
// call time / 16; 0 where the CPU has no IFMA) and one transcript on the scalar 4 x 64-bit code
int gkr_ubench_host_hash(int len, double* us_per_hash_lanes16, double* us_per_hash_scalar) {
    if (len < 1 || len > 3 || !us_per_hash_lanes16 || !us_per_hash_scalar) return GKR_ERR_INVALID;
    uint64_t v16[16][3][4], o16[16][4];
    uint32_t len16[16];
    for (int k = 0; k < 16; ++k) {
        len16[k] = (uint32_t)len;
        for (int e = 0; e < 3; ++e)
            for (int j = 0; j < 4; ++j) v16[k][e][j] = j == 3 ? 0x0123456789abcdefull >> 4 : 0x9E3779B97F4A7C15ull * (uint64_t)(k * 12 + e * 4 + j + 1);
    }
    auto now = [] { return std::chrono::steady_clock::now(); };
    *us_per_hash_lanes16 = 0.0;
    if (host_ifma_ready()) {
        double best = 1e30;
        for (int rep = 0; rep < 5; ++rep) {
            const auto t0 = now();
            for (int i = 0; i < 64; ++i) {
                gkr::gkr_ifma_multi_hash16(v16, len16, 3, o16);
                memcpy(v16[i & 15][2], o16[(i + 1) & 15], 32);   // (keeps the calls dependent)
            }
            const double us = std::chrono::duration<double, std::micro>(now() - t0).count() / (64.0 * 16.0);
            if (us < best) best = us;
        }
        *us_per_hash_lanes16 = best;
    }
    const gkr::h64::F* cts = host_mimc_constants64();
    gkr::h64::F v[3];
    memcpy(v, v16[0], 96);
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        const auto t0 = now();
        for (int i = 0; i < 32; ++i) v[2] = host_multi_hash(v + (3 - len), len, cts);
        const double us = std::chrono::duration<double, std::micro>(now() - t0).count() / 32.0;
        if (us < best) best = us;
    }
    *us_per_hash_scalar = best;
    return GKR_OK;
}

int gkr_selftest_dot(const gkr_fr* a, const gkr_fr* b, size_t n, gkr_fr* out) {
    if ((!a || !b) && n) return GKR_ERR_INVALID;
    if (!out) return GKR_ERR_INVALID;
    if (!all_canonical(a, n) || !all_canonical(b, n)) return GKR_ERR_NON_CANONICAL;
    // sum a_i b_i the way the fused layer kernel does: b in Montgomery form, full products
    // accumulated unreduced, one reduction at the end
    gkr::Lazy17 acc = gkr::lazy_zero(), t0 = gkr::lazy_zero(), t1 = gkr::lazy_zero(), t2 = gkr::lazy_zero();
    for (size_t i = 0; i < n; ++i) {
        const Fr x = to_dev(a[i]), y = gkr::to_mont(to_dev(b[i]));
        gkr::lazy_mac_s(acc, x, y);
        gkr::lazy_mac3_s(t0, x, y, t1, y, x, t2, x, y);   // the tripled form the fused layer kernel uses
    }
    const Fr r = gkr::lazy_reduce(acc);
    if (!gkr::fr_eq(gkr::lazy_reduce(t0), r) || !gkr::fr_eq(gkr::lazy_reduce(t1), r) || !gkr::fr_eq(gkr::lazy_reduce(t2), r))
        return GKR_ERR_INVALID;
    if (n <= 8) {   // the multi-round fold's form: four accumulators advanced together, short reduction
        gkr::Lazy17 q[4] = {gkr::lazy_zero(), gkr::lazy_zero(), gkr::lazy_zero(), gkr::lazy_zero()};
        Fr xs[8], ys[8];
        for (size_t i = 0; i < 8; ++i) {
            xs[i] = i < n ? to_dev(a[i]) : gkr::fr_zero();
            ys[i] = i < n ? gkr::to_mont(to_dev(b[i])) : gkr::fr_zero();
        }
        gkr::lazy_mac4_s(q[0], xs[0], ys[0], q[1], xs[1], ys[1], q[2], xs[2], ys[2], q[3], xs[3], ys[3]);
        gkr::lazy_mac4_s(q[0], xs[4], ys[4], q[1], xs[5], ys[5], q[2], xs[6], ys[6], q[3], xs[7], ys[7]);
        gkr::lazy_add(q[0], q[1]);
        gkr::lazy_add(q[2], q[3]);
        gkr::lazy_add(q[0], q[2]);
        if (!gkr::fr_eq(gkr::lazy_reduce_k8(q[0]), r)) return GKR_ERR_INVALID;
        gkr::Lazy17 ws;   // the one-shot column form the multifold kernel uses
        gkr::weighted_sum_s<8>(xs, ys, ws);
        if (!gkr::fr_eq(gkr::lazy_reduce_k8(ws), r)) return GKR_ERR_INVALID;
        if (n <= 4) {
            Fr x4[4] = {xs[0], xs[1], xs[2], xs[3]};
            gkr::weighted_sum_s<4>(x4, ys, ws);
            if (!gkr::fr_eq(gkr::lazy_reduce_k8(ws), r)) return GKR_ERR_INVALID;
        }
    }
    *out = to_abi(r);
    return GKR_OK;
}

// One item of a gate-list segment and its bucket's combine step, on the host twins of the device code (gate_seg.h):
// out0 / out1 = E_hi * sum over the item's gates, canonical.
int gkr_selftest_seg_item(const gkr_fr* e_lo, const gkr_fr* t, const uint8_t* is_mult, size_t n, const gkr_fr* e_hi, int rows,
                          gkr_fr* out0, gkr_fr* out1) {
    if (!e_lo || !t || !is_mult || !e_hi || !out0 || !out1 || n > gkr::kSegCap) return GKR_ERR_INVALID;
    if (!all_canonical(e_lo, n) || !all_canonical(t, n) || !all_canonical(e_hi, 1)) return GKR_ERR_NON_CANONICAL;
    // both forms of the item arithmetic (gate_seg.h): a select per gate in the order given, and -- what k_seg_pass runs -- the
    // add gates first with one exchange of the accumulators; they must leave the same two sums
    gkr::Lazy17 L0 = gkr::lazy_zero(), L1 = gkr::lazy_zero(), R0 = gkr::lazy_zero(), R1 = gkr::lazy_zero(), O0, O1;
    bool sw = false;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = 0; i < n; ++i) {
            const Fr e = gkr::to_mont(to_dev(e_lo[i])), w = gkr::to_mont(to_dev(t[i]));
            const bool m = is_mult[i] != 0;
            if (pass == 0) {
                if (rows)
                    gkr::seg_gate<true>(L0, L1, e, w, m);
                else
                    gkr::seg_gate<false>(L0, L1, e, w, m);
            }
            if (m != (pass == 1)) continue;   // pass 0: the add gates, pass 1: the mult gates
            if (rows)
                gkr::seg_gate_ordered<true>(R0, R1, sw, e, w, m);
            else
                gkr::seg_gate_ordered<false>(R0, R1, sw, e, w, m);
        }
    if (rows)
        gkr::seg_item_sums<true>(R0, R1, sw, O0, O1);
    else
        gkr::seg_item_sums<false>(R0, R1, sw, O0, O1);
    for (int c = 0; c < 17; ++c)
        if (O0.l[c] != L0.l[c] || O1.l[c] != L1.l[c]) return GKR_ERR_INVALID;
    const Fr x = gkr::lazy_reduce_partial32(L0), y = gkr::lazy_reduce_partial32(L1);
    gkr::Lazy17 A = gkr::lazy_zero(), B = gkr::lazy_zero();
    gkr::lazy_mac_v(A, x, to_dev(*e_hi));
    gkr::lazy_mac_v(B, y, to_dev(*e_hi));
    *out0 = to_abi(gkr::lazy_reduce(A));
    *out1 = to_abi(gkr::lazy_reduce(B));
    return GKR_OK;
}

// q(t) = W(b + t (c - b)) the way gkr_prove computes it on the host (Moebius transform for the length, variable-by-
// variable binding for the coefficients); out: k + 1 slots right-aligned
int gkr_selftest_line_restriction(int k, const gkr_fr* W, const gkr_fr* b, const gkr_fr* c, gkr_fr* out, uint32_t* out_len) {
    if (k < 1 || k > 20 || !W || !b || !c || !out || !out_len) return GKR_ERR_INVALID;
    const size_t n = (size_t)1 << k;
    if (!all_canonical(W, n) || !all_canonical(b, k) || !all_canonical(c, k)) return GKR_ERR_NON_CANONICAL;
    std::vector<gkr::h64::F> vals(n);
    memcpy(vals.data(), W, n * 32);
    std::vector<gkr::h64::F> co(vals);
    mobius_msb(co, k);
    line_restriction(vals, co, k, b, c, out, out_len);
    return GKR_OK;
}

int gkr_selftest_wide_sum(const gkr_fr* vals, size_t n, gkr_fr* out) {
    if ((!vals && n) || !out) return GKR_ERR_INVALID;
    if (!all_canonical(vals, n)) return GKR_ERR_NON_CANONICAL;
    // the kernels' accumulation scheme: 288-bit partials, 320-bit totals, one reduction
    gkr::Acc<10> total = gkr::acc_zero<10>();
    gkr::Acc<9> part = gkr::acc_zero<9>();
    for (size_t i = 0; i < n; ++i) {
        gkr::acc_add_fr(part, to_dev(vals[i]));
        if ((i & 1023) == 1023) {
            gkr::acc_add_acc(total, part);
            part = gkr::acc_zero<9>();
        }
    }
    gkr::acc_add_acc(total, part);
    *out = to_abi(gkr::acc_reduce(total));
    return GKR_OK;
}

// ---- device memory helpers ---------------------------------------------------------------

int gkr_device_alloc(gkr_ctx* ctx, size_t bytes, void** d_ptr) {
    if (!ctx || !d_ptr || !bytes) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    hipError_t e = device_malloc(d_ptr, bytes);
    if (e == hipErrorOutOfMemory) return ctx->fail(GKR_ERR_NOMEM, "hipMalloc: out of memory");
    HIP_TRY(ctx, e);
    return GKR_OK;
}

int gkr_device_free(gkr_ctx* ctx, void* d_ptr) {
    if (!ctx) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    HIP_TRY(ctx, device_free(d_ptr));
    return GKR_OK;
}

int gkr_device_upload(gkr_ctx* ctx, void* d_dst, const void* h_src, size_t bytes) {
    if (!ctx || !d_dst || !h_src) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

int gkr_device_download(gkr_ctx* ctx, void* h_dst, const void* d_src, size_t bytes) {
    if (!ctx || !h_dst || !d_src) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

int gkr_device_fill_table(gkr_ctx* ctx, void* d_table, size_t count, uint64_t seed) {
    if (!ctx || !d_table || !count) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    gkr::launch_fill_table(static_cast<Fr*>(d_table), count, seed, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

int gkr_device_fill_shard(gkr_ctx* ctx, void* d_shard, int n, int log2_shards, int shard, uint64_t seed) {
    if (!ctx || !d_shard || log2_shards < 0 || log2_shards > 16 || n - log2_shards < 1 || n - log2_shards > GKR_MAX_MLE_N || shard < 0 ||
        shard >= (1 << log2_shards))
        return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    gkr::launch_fill_shard(static_cast<Fr*>(d_shard), (size_t)1 << (n - log2_shards), (uint32_t)log2_shards, (uint32_t)shard, seed, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    return GKR_OK;
}

int gkr_ubench_ceilings(gkr_ctx* ctx, size_t bytes, double* copy_GBps, double* read_GBps, double* modmul_per_sec) {
    if (!ctx) return GKR_ERR_INVALID;
    if (!copy_GBps || !read_GBps || !modmul_per_sec) return ctx->fail(GKR_ERR_INVALID, "null pointer");
    if (bytes < ((size_t)64 << 20)) bytes = (size_t)64 << 20;
    bytes &= ~(size_t)4095;
    GKR_ENTER(ctx);
    hipStream_t s = ctx->stream;
    char *a = nullptr, *b = nullptr;
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&a), bytes));
    if (hipMalloc(reinterpret_cast<void**>(&b), bytes) != hipSuccess) {
        (void)hipFree(a);
        return ctx->fail(GKR_ERR_NOMEM, "device memory for the copy probe");
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = GKR_OK;
    auto best_ms = [&](auto&& launch, int reps) -> double {
        double best = 1e30;
        for (int r = 0; r < reps; ++r) {
            if (hipEventRecord(e0, s) != hipSuccess) return -1.0;
            launch();
            if (hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return -1.0;
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return -1.0;
            if (r > 0 && ms < best) best = ms;   // the first repetition touches the pages
        }
        return best;
    };
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) rc = ctx->fail(GKR_ERR_HIP, "hipEventCreate");
    if (!rc) {
        gkr::launch_fill_table(reinterpret_cast<Fr*>(a), bytes / 32, 1, s);
        const double c = best_ms([&] { gkr::launch_ubench_copy(a, b, bytes, s); }, 6);
        const double rd = best_ms([&] { gkr::launch_ubench_read(a, b, bytes, s); }, 6);
        const int waves = 16384, reps = 128;   // 16 waves per SIMD: the rate no longer grows with more
        const double mm = best_ms([&] { gkr::launch_ubench_modmul(reinterpret_cast<Fr*>(a), 1u << 20, waves, reps, s); }, 4);
        if (c <= 0 || rd <= 0 || mm <= 0 || hipGetLastError() != hipSuccess) {
            rc = ctx->fail(GKR_ERR_HIP, "the ceiling probes failed");
        } else {
            *copy_GBps = 2.0 * (double)bytes / (c * 1e-3) / 1e9;
            *read_GBps = (double)bytes / (rd * 1e-3) / 1e9;
            *modmul_per_sec = (double)waves * 64.0 * reps / (mm * 1e-3);
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    return rc;
}

int gkr_device_synchronize(gkr_ctx* ctx) {
    if (!ctx) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}


}  // extern "C"

// The device verifier of the C ABI: gkr_verify_prepare / gkr_verify_prepared / gkr_verify_circuit_free / gkr_verify_device.
//
// gkr_verify (dropin.cpp) checks a proof on the host's threads, and almost all of its time goes into three sums: the wiring
// predicates over every gate, the input layer's coefficient table at z[L], and the canonical scans of the two coefficient
// tables.  Here those run on the device (kernels_verify.hip) and everything that is O(rounds) -- the relations themselves, in
// the reference's order -- stays on the host, in the ONE routine both verifiers share (verify_core.h).
//
// A call, per chunk of proofs (as many as fit verify_workspace_mb of device workspace; verdicts do not depend on the chunking):
//   1. the chunk's challenge hashes (2 k per layer and proof) start.  A lone hash is 3.6 us on a host core and hundreds on the
//      device, but a verifier's hashes are a flat array of independent jobs, known before the first launch: a chunk of at
//      least verify_device_hash_min round vectors sends them to the device (k_verify_hash, kernels_verify_hash.hip: eight lanes
//      per vector) on the context's side stream, forked from the main stream and joined in front of the result copy, so the
//      long, narrow hash launch runs beside everything in 2.  A smaller chunk hashes on the context's host threads, 16 vectors
//      a piece, while the device works;
//   2. the calling thread uploads z, the challenges and the two coefficient tables of every proof, then launches, for ALL
//      layers and proofs at once (a verifier reads every challenge out of the proof: nothing waits for a hash):
//      eq(z_i, .) as two half tables, eq(b*, .), eq(c*, .) per layer (launch_eq_table, one launch per table for the chunk), the
//      wiring pass as ONE launch over (layer, proof) driven by a layer table in device memory plus its second-level sums,
//      the canonical scans, and the two coefficient-table evaluations; one copy brings every result back;
//   3. it joins the hashing (the side stream's event, or the host pool), synchronises ONCE, and runs the shared relations per
//      proof with the device's values.  Verdicts do not depend on where the hashes ran: both sides fill the same HashSlot array
//      by the same rule (hash_piece below is that rule; the kernel restates it).
//
// gkr_mimc7_multi_hash_device is the same kernel through the same launcher for a caller's own rows.
//
// Requirement (verify_core.h states it where the order lives): the device computes from proof elements nobody has checked yet,
// so some of its values may be garbage; the relations consult a value only after the elements behind it passed their own checks.
#include <atomic>

#include "capi_internal.h"
#include "verify_core.h"

struct gkr_verify_circuit {
    int device = 0;
    std::vector<uint32_t> k;       // the handle's own copy: L + 1 entries
    std::vector<uint2*> gates;     // per layer 2^k[i] packed records (kernels_verify.hip, k_verify_pack)
};

namespace {

using gkr::h64::F;
namespace V = gkr::verify;

int alloc_status(gkr_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return ctx->fail(GKR_ERR_NOMEM, std::string(what) + ": out of device memory");
    }
    return ctx->hip_fail(e, what);
}
#define VERIFY_WS(ctx, slot, type, count, ptr)                                                                        \
    do {                                                                                                              \
        const hipError_t _e = (ctx)->workspace(slot, (size_t)(count) * sizeof(type), reinterpret_cast<void**>(&(ptr))); \
        if (_e != hipSuccess) return alloc_status(ctx, _e, slot);                                                     \
    } while (0)

void release(gkr_verify_circuit* vc) {
    for (uint2* p : vc->gates)
        if (p) (void)hipFree(p);
    delete vc;
}

// the circuit checks that need neither a context nor a device, in gkr_verify's order
int check_circuit_args(const gkr_circuit_desc* circuit) {
    if (!circuit || !circuit->k || circuit->depth < 1 || circuit->depth > 4096) return GKR_ERR_INVALID;
    if (!circuit->gate_type || !circuit->left || !circuit->right) return GKR_ERR_INVALID;
    return V::check_k_list(circuit);
}

// the challenge hashes of a chunk, computed while the device works: slot (proof, row) holds multi_hash of that round vector
// when the row is well-formed (1 .. 3 canonical coefficients); the relations reject a malformed row before they ask for its hash
struct HashSlot {
    gkr_fr h;
    uint32_t valid;
};
static_assert(sizeof(HashSlot) == sizeof(gkr::VerifyHashSlot) && offsetof(HashSlot, valid) == offsetof(gkr::VerifyHashSlot, valid),
              "the kernel writes the slots the relations read");
// one piece of 16 slots; false when none is left (safe to call from many threads: the shape of a SpinPool job)
bool hash_piece(const gkr_proof_buf* proofs, size_t rounds, size_t n, std::atomic<size_t>& next, HashSlot* slots) {
    const F* cts = host_mimc_constants64();
    {
        const size_t a = next.fetch_add(16, std::memory_order_relaxed);
        if (a >= n) return false;
        for (size_t s = a; s < std::min(n, a + 16); ++s) {
            const gkr_proof_buf& p = proofs[s / rounds];
            const size_t row = s % rounds;
            const uint32_t len = p.sumcheck_len[row];
            slots[s].valid = 0;
            if (len < 1 || len > 3) continue;
            const gkr_fr* g = p.sumcheck_coeffs + row * 3 + (3 - len);
            F v[3];
            bool ok = true;
            for (uint32_t t = 0; t < len; ++t) {
                ok = ok && V::canonical(g[t]);
                v[t] = V::load(g[t]);
            }
            if (!ok) continue;
            const F h = host_multi_hash(v, (int)len, cts);
            memcpy(slots[s].h.l, h.l, 32);
            slots[s].valid = 1;
        }
    }
    return true;
}

// Smallest number of round vectors in a chunk that are hashed on the device when verify_device_hash_min is 0; 0: never.
// Measured (profiles/r08, tools/bench_verify.py --hash both --sweep: the demo circuit k = [5,6,7,7,7,7], 68 vectors per proof,
// MI355X, 16 host CPUs, median (interquartile range) of 20 alternating calls, ms):
//     vectors      68     136     272     544    1088    4352   17408   69632  278528
//     host      0.305   0.318   0.499   0.761   1.616   4.826  18.411  70.622 285.474
//     device    0.483   0.489   0.518   0.563   0.630   1.058   2.960  10.478  59.930
// From 544 vectors on, at every larger point, the device median is below the host median by more than the sum of the two
// interquartile ranges (at 272: 0.019 ms in favour of the host); rounded up to a power of two.
constexpr long long kVerifyDeviceHashMinRows = 1024;
constexpr size_t kHashRowWords = 24, kHashLaunchRows = (size_t)1 << 24;   // (rows per launch: the grid stays far below 2^31 blocks)
constexpr double kHashRowBytes = 96.0 + 4.0 + 36.0;                       // a row in, its length, hash and valid word out

bool device_hash_wanted(size_t rows) {
    long long min_rows = gkr::opt(gkr::OPT_verify_device_hash_min);
    if (min_rows == 0) min_rows = kVerifyDeviceHashMinRows;
    return min_rows > 0 && rows >= (size_t)min_rows;
}

// n rows and their lengths, in device memory -> their slots in device memory, on stream s: THE launcher of both entry points
// (slots: 3, this file's rows, or 4, the degree-3 product sumcheck's)
int hash_rows_device(gkr_ctx* ctx, int slots, const uint32_t* d_rows, const uint32_t* d_len, size_t n, gkr::VerifyHashSlot* d_slots, hipStream_t s) {
    const size_t row_words = (size_t)slots * 8;
    for (size_t a = 0; a < n; a += kHashLaunchRows) {
        const size_t m = std::min(kHashLaunchRows, n - a);
        {
            Timed t(ctx, "verify_hash", (double)m * (kHashRowBytes + 32.0 * (slots - 3)), s);
            gkr::launch_verify_hash(slots, d_rows + a * row_words, d_len + a, (uint32_t)m, ctx->d_cts, d_slots + a, s);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    return GKR_OK;
}

// gkr_verify_prepared's provider of the shared relations: what the kernels left, read back (pinned host memory)
struct DeviceProvider {
    uint32_t L;
    size_t rounds;
    const size_t* last_row;    // per layer: the row of its last round vector (r* hashes the same vector)
    const HashSlot* slots;     // this proof's
    const Fr* wiring_out;      // this proof's: L x (add, mult), Montgomery
    const Fr* evals;           // this proof's: D(z[0]), input_func(z[L]), canonical
    const uint32_t* flags;     // this proof's: d_coeffs, input_coeffs hold an element >= r

    static F as_f(const Fr& x) {
        F f;
        memcpy(f.l, &x, 32);
        return f;
    }
    int layer_ready(uint32_t) const { return GKR_OK; }
    bool table_canonical(int which) const { return flags[which] == 0; }
    F table_eval(int which, const std::vector<F>&) const { return as_f(evals[which]); }
    int hash(size_t slot, const gkr_fr*, uint32_t, gkr_fr* h) const {
        const HashSlot& s = slots[slot < rounds ? slot : last_row[slot - rounds]];
        if (!s.valid) return GKR_ERR_INVALID;
        *h = s.h;
        return GKR_OK;
    }
    int wiring(uint32_t i, const std::vector<F>&, const std::vector<F>&, const std::vector<F>&, F* add_m, F* mult_m) const {
        *add_m = as_f(wiring_out[2 * (size_t)i]);
        *mult_m = as_f(wiring_out[2 * (size_t)i + 1]);
        return GKR_OK;
    }
};

// per-proof shape of a circuit's proofs and of the device workspace a proof takes
struct Shape {
    uint32_t L = 0, max_k_i = 0;
    size_t zlen = 0, rounds = 0, n_d = 0, n_in = 0;
    size_t table_elems = 0;    // all layers' e_hi, e_lo, eq_b, eq_c
    size_t mono_elems = 0;     // the half tables of both coefficient tables
    size_t partial_elems = 0;  // wiring + both evaluations
    size_t out_elems = 0;      // 2 L + 2
    std::vector<size_t> z_off, row_off, last_row;
    size_t bytes_per_proof() const {
        // (the last term: a round vector, its length and its hash slot, for the chunks whose hashes run on the device)
        return (zlen + rounds + n_d + n_in + table_elems + mono_elems + partial_elems + out_elems) * sizeof(Fr) + 2 * sizeof(uint32_t) +
               rounds * (kHashRowWords * sizeof(uint32_t) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
    }
};
Shape shape_of(const std::vector<uint32_t>& k) {
    Shape s;
    s.L = (uint32_t)k.size() - 1;
    s.n_d = (size_t)1 << k[0];
    s.n_in = (size_t)1 << k[s.L];
    for (uint32_t i = 0; i <= s.L; ++i) {
        s.z_off.push_back(s.zlen);
        s.zlen += k[i];
    }
    for (uint32_t i = 0; i < s.L; ++i) {
        s.row_off.push_back(s.rounds);
        s.rounds += 2 * (size_t)k[i + 1];
        s.last_row.push_back(s.rounds - 1);
        const uint32_t kl = k[i] / 2, kh = k[i] - kl;
        s.table_elems += ((size_t)1 << kh) + ((size_t)1 << kl) + ((size_t)2 << k[i + 1]);
        s.max_k_i = std::max(s.max_k_i, k[i]);
    }
    for (uint32_t kk : {k[0], k[s.L]}) s.mono_elems += ((size_t)1 << (kk - kk / 2)) + ((size_t)1 << (kk / 2));
    s.partial_elems = (size_t)s.L * 2 * gkr::verify_wiring_blocks(s.max_k_i) + gkr::verify_mono_blocks(k[0]) + gkr::verify_mono_blocks(k[s.L]);
    s.out_elems = 2 * (size_t)s.L + 2;
    return s;
}

constexpr size_t kStageMaxBytes = (size_t)8 << 20;   // coefficient tables of a chunk up to this size go through one pinned staging copy

int verify_chunk(gkr_ctx* ctx, const gkr_verify_circuit* vc, const Shape& sh, const gkr_proof_buf* proofs, uint32_t nb, int* accept,
                 uint32_t* failed_layer, uint32_t* failed_check) {
    const std::vector<uint32_t>& k = vc->k;
    const uint32_t L = sh.L;
    hipStream_t st = ctx->stream;
    // ---- 1. the hashes start: on the context's host pool (its workers take pieces for as long as the session is open; the
    //         guard closes it on every way out, before `host_slots` goes), or -- a chunk of enough round vectors -- on the device,
    //         further down, once the workspaces are there (no piece is left for the pool then)
    const size_t n_rows = (size_t)nb * sh.rounds;
    const bool dev_hash = device_hash_wanted(n_rows);
    std::vector<HashSlot> host_slots(dev_hash ? 0 : n_rows);
    const HashSlot* slots = host_slots.data();
    std::atomic<size_t> next{dev_hash ? n_rows : 0};
    const std::function<bool()> hash_work = [&] { return hash_piece(proofs, sh.rounds, n_rows, next, host_slots.data()); };
    gkr::SpinPool* pool = !dev_hash && n_rows >= 64 ? ctx->host_pool() : nullptr;   // waking the pool is worth some tens of hashes
    gkr::SpinPool::Session hashing(pool, &hash_work);
    // the side stream's work is joined on every way out: nothing may still read or write a workspace the next call reuses
    struct SideJoin {
        hipStream_t forked = nullptr;
        ~SideJoin() {
            if (forked) (void)hipStreamSynchronize(forked);
        }
    } side;
    // ---- 2. upload, every launch, one copy back
    const uint32_t pstride = (uint32_t)(sh.zlen + sh.rounds);
    Fr *d_pts, *d_dco, *d_ico, *d_tables, *d_mono, *d_partials, *d_out;
    gkr::VerifyLayer* d_layers;
    VERIFY_WS(ctx, "verify_pts", Fr, (size_t)nb * pstride + 1, d_pts);
    VERIFY_WS(ctx, "verify_dco", Fr, (size_t)nb * sh.n_d, d_dco);
    VERIFY_WS(ctx, "verify_ico", Fr, (size_t)nb * sh.n_in, d_ico);
    VERIFY_WS(ctx, "verify_tables", Fr, (size_t)nb * sh.table_elems, d_tables);
    VERIFY_WS(ctx, "verify_mono", Fr, (size_t)nb * sh.mono_elems, d_mono);
    VERIFY_WS(ctx, "verify_partials", Fr, (size_t)nb * sh.partial_elems, d_partials);
    VERIFY_WS(ctx, "verify_out", Fr, (size_t)nb * sh.out_elems + (2 * (size_t)nb * sizeof(uint32_t) + sizeof(Fr) - 1) / sizeof(Fr), d_out);
    VERIFY_WS(ctx, "verify_layers", gkr::VerifyLayer, L, d_layers);
    uint32_t* d_flags = reinterpret_cast<uint32_t*>(d_out + (size_t)nb * sh.out_elems);
    const size_t out_bytes = (size_t)nb * sh.out_elems * sizeof(Fr) + 2 * (size_t)nb * sizeof(uint32_t);
    const size_t coeff_bytes = (size_t)nb * (sh.n_d + sh.n_in) * sizeof(Fr);
    const bool stage = coeff_bytes <= kStageMaxBytes;
    Fr *h_pts, *h_out, *h_co = nullptr;
    gkr::VerifyLayer* h_layers;
    HIP_TRY(ctx, ctx->pinned_host("verify_pts", ((size_t)nb * pstride + 1) * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("verify_out", out_bytes, reinterpret_cast<void**>(&h_out)));
    HIP_TRY(ctx, ctx->pinned_host("verify_layers", (size_t)L * sizeof(gkr::VerifyLayer), reinterpret_cast<void**>(&h_layers)));
    if (stage) HIP_TRY(ctx, ctx->pinned_host("verify_coeffs", coeff_bytes, reinterpret_cast<void**>(&h_co)));
    if (dev_hash) {
        // round vectors, then lengths, in ONE staging buffer and one copy up; the slots come back into pinned memory on the side
        // stream, whose last event the main stream waits for in front of its own result copy
        uint32_t *d_hin, *h_hin;
        gkr::VerifyHashSlot *d_hout, *h_hout;
        VERIFY_WS(ctx, "verify_hash_in", uint32_t, n_rows * (kHashRowWords + 1), d_hin);
        VERIFY_WS(ctx, "verify_hash_out", gkr::VerifyHashSlot, n_rows, d_hout);
        HIP_TRY(ctx, ctx->pinned_host("verify_hash_in", n_rows * (kHashRowWords + 1) * sizeof(uint32_t), reinterpret_cast<void**>(&h_hin)));
        HIP_TRY(ctx, ctx->pinned_host("verify_hash_out", n_rows * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_hout)));
        uint32_t* h_hlen = h_hin + n_rows * kHashRowWords;
        for (uint32_t p = 0; p < nb; ++p) {
            memcpy(h_hin + (size_t)p * sh.rounds * kHashRowWords, proofs[p].sumcheck_coeffs, sh.rounds * kHashRowWords * sizeof(uint32_t));
            memcpy(h_hlen + (size_t)p * sh.rounds, proofs[p].sumcheck_len, sh.rounds * sizeof(uint32_t));
        }
        HIP_TRY(ctx, ctx->aux_stream(2));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[0], st));             // fork: after whatever the main stream still holds
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->aux_events[0], 0));
        side.forked = ctx->aux;
        HIP_TRY(ctx, hipMemcpyAsync(d_hin, h_hin, n_rows * (kHashRowWords + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->aux));
        if (const int rc = hash_rows_device(ctx, 3, d_hin, d_hin + n_rows * kHashRowWords, n_rows, d_hout, ctx->aux)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(h_hout, d_hout, n_rows * sizeof(gkr::VerifyHashSlot), hipMemcpyDeviceToHost, ctx->aux));
        HIP_TRY(ctx, hipEventRecord(ctx->aux_events[1], ctx->aux));
        slots = reinterpret_cast<const HashSlot*>(h_hout);
    }
    for (uint32_t p = 0; p < nb; ++p) {
        if (sh.zlen) memcpy(h_pts + (size_t)p * pstride, proofs[p].z, sh.zlen * sizeof(Fr));
        memcpy(h_pts + (size_t)p * pstride + sh.zlen, proofs[p].sumcheck_r, sh.rounds * sizeof(Fr));
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_pts, h_pts, (size_t)nb * pstride * sizeof(Fr), hipMemcpyHostToDevice, st));
    if (stage) {
        for (uint32_t p = 0; p < nb; ++p) {
            memcpy(h_co + (size_t)p * sh.n_d, proofs[p].d_coeffs, sh.n_d * sizeof(Fr));
            memcpy(h_co + (size_t)nb * sh.n_d + (size_t)p * sh.n_in, proofs[p].input_coeffs, sh.n_in * sizeof(Fr));
        }
        HIP_TRY(ctx, hipMemcpyAsync(d_dco, h_co, (size_t)nb * sh.n_d * sizeof(Fr), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_ico, h_co + (size_t)nb * sh.n_d, (size_t)nb * sh.n_in * sizeof(Fr), hipMemcpyHostToDevice, st));
    } else {
        for (uint32_t p = 0; p < nb; ++p) {
            HIP_TRY(ctx, hipMemcpyAsync(d_dco + (size_t)p * sh.n_d, proofs[p].d_coeffs, sh.n_d * sizeof(Fr), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_ico + (size_t)p * sh.n_in, proofs[p].input_coeffs, sh.n_in * sizeof(Fr), hipMemcpyHostToDevice, st));
        }
    }
    // the layers' tables and the layer table of the wiring pass
    {
        Fr* t = d_tables;
        for (uint32_t i = 0; i < L; ++i) {
            const uint32_t k_i = k[i], kn = k[i + 1], kl = k_i / 2, kh = k_i - kl;
            Fr* e_hi = t;
            Fr* e_lo = e_hi + ((size_t)nb << kh);
            Fr* eq_b = e_lo + ((size_t)nb << kl);
            Fr* eq_c = eq_b + ((size_t)nb << kn);
            t = eq_c + ((size_t)nb << kn);
            h_layers[i] = gkr::VerifyLayer{vc->gates[i], e_hi, e_lo, eq_b, eq_c, k_i, kl, kn, 0u};
            gkr::launch_eq_table(d_pts, pstride, (uint32_t)sh.z_off[i], kh, e_hi, true, nb, st);
            gkr::launch_eq_table(d_pts, pstride, (uint32_t)sh.z_off[i] + kh, kl, e_lo, true, nb, st);
            gkr::launch_eq_table(d_pts, pstride, (uint32_t)(sh.zlen + sh.row_off[i]), kn, eq_b, true, nb, st);
            gkr::launch_eq_table(d_pts, pstride, (uint32_t)(sh.zlen + sh.row_off[i]) + kn, kn, eq_c, true, nb, st);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_layers, h_layers, (size_t)L * sizeof(gkr::VerifyLayer), hipMemcpyHostToDevice, st));
    Fr* d_wiring_out = d_out;
    Fr* d_evals = d_out + (size_t)nb * 2 * L;
    gkr::launch_verify_wiring(d_layers, L, sh.max_k_i, nb, d_partials, d_wiring_out, st);
    // the coefficient tables: canonical scans (one flag per table) and the evaluations at z[0] and z[L]
    HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, 2 * (size_t)nb * sizeof(uint32_t), st));
    gkr::launch_verify_canonical(d_dco, k[0], d_flags, 2u, nb, st);
    gkr::launch_verify_canonical(d_ico, k[L], d_flags + 1, 2u, nb, st);
    {
        Fr* part = d_partials + (size_t)nb * L * 2 * gkr::verify_wiring_blocks(sh.max_k_i);
        Fr* mono = d_mono;
        const uint32_t k0 = k[0], kL = k[L];
        Fr* d_ev = d_evals;   // nb values of D, then nb values of the input function
        gkr::launch_verify_mono_eval(d_pts, pstride, 0u, k0, d_dco, mono, mono + ((size_t)nb << (k0 - k0 / 2)), part, d_ev, nb, st);
        mono += ((size_t)nb << (k0 - k0 / 2)) + ((size_t)nb << (k0 / 2));
        part += (size_t)nb * gkr::verify_mono_blocks(k0);
        gkr::launch_verify_mono_eval(d_pts, pstride, (uint32_t)sh.z_off[L], kL, d_ico, mono, mono + ((size_t)nb << (kL - kL / 2)), part, d_ev + nb, nb, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (dev_hash) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->aux_events[1], 0));   // join: the slots are back before the results are
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    // ---- 3. this thread hashes too (the host's pieces, if there are any), then the one synchronisation and the relations
    while (hash_work()) {
    }
    hashing.close();
    HIP_TRY(ctx, hipStreamSynchronize(st));
    side.forked = nullptr;   // (joined: the main stream waited for the side stream's last event)
    const Fr* h_evals = h_out + (size_t)nb * 2 * L;
    const uint32_t* h_flags = reinterpret_cast<const uint32_t*>(h_out + (size_t)nb * sh.out_elems);
    for (uint32_t p = 0; p < nb; ++p) {
        const Fr evals[2] = {h_evals[p], h_evals[nb + p]};
        DeviceProvider prov{L, sh.rounds, sh.last_row.data(), slots + (size_t)p * sh.rounds, h_out + (size_t)p * 2 * L, evals, h_flags + 2 * (size_t)p};
        uint32_t fl = 0, fc = 0;
        const int rc = V::relations(L, k.data(), &proofs[p], prov, &accept[p], &fl, &fc);
        if (rc) return ctx->fail(rc, "gkr_verify_prepared: the relations of a proof could not be evaluated");
        if (failed_layer) failed_layer[p] = fl;
        if (failed_check) failed_check[p] = fc;
    }
    return GKR_OK;
}

}  // namespace

// the plain and the product sumcheck's verifier (capi_mle_verify.hip) hash their round vectors through the same threshold and the same launcher
namespace gkr_host {
bool verify_device_hash_wanted(size_t rows) { return device_hash_wanted(rows); }
int verify_hash_rows_device(gkr_ctx* ctx, int slots, const uint32_t* d_rows, const uint32_t* d_len, size_t n, gkr::VerifyHashSlot* d_slots,
                            hipStream_t s) {
    return hash_rows_device(ctx, slots, d_rows, d_len, n, d_slots, s);
}
}  // namespace gkr_host

extern "C" {

int gkr_verify_prepare(gkr_ctx* ctx, const gkr_circuit_desc* circuit, gkr_verify_circuit** out) {
    if (!out) return GKR_ERR_INVALID;
    *out = nullptr;
    if (const int rc = check_circuit_args(circuit)) return rc;
    if (!ctx) return GKR_ERR_INVALID;
    const uint32_t L = circuit->depth;
    for (uint32_t i = 0; i < L; ++i)
        if (!circuit->gate_type[i] || !circuit->left[i] || !circuit->right[i]) return ctx->fail(GKR_ERR_INVALID, "null gate array");
    GKR_ENTER(ctx);
    struct Guard {
        gkr_verify_circuit* vc;
        ~Guard() {
            if (vc) release(vc);
        }
    } guard{new gkr_verify_circuit()};
    gkr_verify_circuit* vc = guard.vc;
    vc->device = ctx->device;
    vc->k.assign(circuit->k, circuit->k + L + 1);
    vc->gates.assign(L, nullptr);
    uint32_t max_k_i = 0;
    for (uint32_t i = 0; i < L; ++i) max_k_i = std::max(max_k_i, circuit->k[i]);
    // the raw arrays of one layer at a time (9 bytes per gate) -> packed and range-checked on the device
    DevBuf<uint8_t> raw_gt;
    DevBuf<uint32_t> raw_l, raw_r, bad;
    hipError_t e;
    if ((e = raw_gt.alloc((size_t)1 << max_k_i)) != hipSuccess || (e = raw_l.alloc((size_t)1 << max_k_i)) != hipSuccess ||
        (e = raw_r.alloc((size_t)1 << max_k_i)) != hipSuccess || (e = bad.alloc(1)) != hipSuccess)
        return alloc_status(ctx, e, "gkr_verify_prepare: staging of the gate arrays");
    HIP_TRY(ctx, hipMemsetAsync(bad.p, 0, sizeof(uint32_t), ctx->stream));
    for (uint32_t i = 0; i < L; ++i) {
        const size_t gates = (size_t)1 << circuit->k[i];
        if ((e = hipMalloc(reinterpret_cast<void**>(&vc->gates[i]), gates * sizeof(uint2))) != hipSuccess)
            return alloc_status(ctx, e, "gkr_verify_prepare: packed gates");
        HIP_TRY(ctx, hipMemcpyAsync(raw_gt.p, circuit->gate_type[i], gates, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(raw_l.p, circuit->left[i], gates * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(raw_r.p, circuit->right[i], gates * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        gkr::launch_verify_pack(raw_gt.p, raw_l.p, raw_r.p, (uint32_t)gates, circuit->k[i + 1], vc->gates[i], bad.p, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint32_t h_bad = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&h_bad, bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (h_bad) return ctx->fail(GKR_ERR_INVALID, "gate type or operand index out of range");   // (the handle goes with the guard: no pass ever reads it)
    guard.vc = nullptr;
    *out = vc;
    return GKR_OK;
}

int gkr_verify_prepared(gkr_ctx* ctx, const gkr_verify_circuit* vc, const gkr_proof_buf* proofs, int batch, int* accept, uint32_t* failed_layer,
                        uint32_t* failed_check) {
    if (!ctx || !vc || !proofs || !accept || batch < 1) return GKR_ERR_INVALID;
    for (int b = 0; b < batch; ++b)
        if (!V::proof_pointers_set(&proofs[b])) return ctx->fail(GKR_ERR_INVALID, "null pointer in a proof buffer");
    if (vc->device != ctx->device) return ctx->fail(GKR_ERR_INVALID, "the handle was prepared on another device");
    GKR_ENTER(ctx);
    const Shape sh = shape_of(vc->k);
    long long mb = gkr::opt(gkr::OPT_verify_workspace_mb);
    if (mb <= 0) mb = 2048;
    size_t chunk = ((size_t)mb << 20) / sh.bytes_per_proof();
    chunk = std::max<size_t>(1, std::min<size_t>(chunk, 32768));   // (the proof is a grid dimension of the launches)
    for (int b = 0; b < batch; b += (int)chunk) {
        const uint32_t nb = (uint32_t)std::min<size_t>(chunk, (size_t)(batch - b));
        const int rc = verify_chunk(ctx, vc, sh, proofs + b, nb, accept + b, failed_layer ? failed_layer + b : nullptr,
                                    failed_check ? failed_check + b : nullptr);
        if (rc) return rc;
    }
    return GKR_OK;
}

int gkr_mimc7_multi_hash_device(gkr_ctx* ctx, const gkr_fr* rows, const uint32_t* len, size_t n, gkr_fr* out, uint32_t* valid) {
    if (!ctx || !rows || !len || !out || !valid || n == 0) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    constexpr size_t kPieceRows = (size_t)1 << 18;   // 25 MiB up, 10 MiB back per piece
    const size_t cap = std::min(n, kPieceRows);
    uint32_t *d_in, *h_in;
    gkr::VerifyHashSlot *d_out, *h_out;
    VERIFY_WS(ctx, "verify_hash_in", uint32_t, cap * (kHashRowWords + 1), d_in);
    VERIFY_WS(ctx, "verify_hash_out", gkr::VerifyHashSlot, cap, d_out);
    HIP_TRY(ctx, ctx->pinned_host("verify_hash_in", cap * (kHashRowWords + 1) * sizeof(uint32_t), reinterpret_cast<void**>(&h_in)));
    HIP_TRY(ctx, ctx->pinned_host("verify_hash_out", cap * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_out)));
    for (size_t a = 0; a < n; a += cap) {
        const size_t m = std::min(cap, n - a);
        memcpy(h_in, rows + a * 3, m * kHashRowWords * sizeof(uint32_t));
        memcpy(h_in + m * kHashRowWords, len + a, m * sizeof(uint32_t));
        HIP_TRY(ctx, hipMemcpyAsync(d_in, h_in, m * (kHashRowWords + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if (const int rc = hash_rows_device(ctx, 3, d_in, d_in + m * kHashRowWords, m, d_out, ctx->stream)) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, m * sizeof(gkr::VerifyHashSlot), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < m; ++i) {
            memcpy(out[a + i].l, h_out[i].h, 32);
            valid[a + i] = h_out[i].valid;
        }
    }
    return GKR_OK;
}

void gkr_verify_circuit_free(gkr_ctx* ctx, gkr_verify_circuit* vc) {
    if (!vc) return;
    int prev = -1;
    const bool switched = hipGetDevice(&prev) == hipSuccess && prev != vc->device && hipSetDevice(vc->device) == hipSuccess;
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    release(vc);
    if (switched) (void)hipSetDevice(prev);
}

int gkr_verify_device(gkr_ctx* ctx, const gkr_circuit_desc* circuit, const gkr_proof_buf* proofs, int batch, int* accept, uint32_t* failed_layer,
                      uint32_t* failed_check) {
    if (const int rc = check_circuit_args(circuit)) return rc;
    if (!ctx || !proofs || !accept || batch < 1) return GKR_ERR_INVALID;
    gkr_verify_circuit* vc = nullptr;
    int rc = gkr_verify_prepare(ctx, circuit, &vc);
    if (rc) return rc;
    rc = gkr_verify_prepared(ctx, vc, proofs, batch, accept, failed_layer, failed_check);
    gkr_verify_circuit_free(ctx, vc);
    return rc;
}

}  // extern "C"

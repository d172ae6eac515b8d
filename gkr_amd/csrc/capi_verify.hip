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
//      by the same rule.
// The hashing, the chunk size and the host's pieces are verify_chunk.h's, shared with the other batch verifiers; particular to
// this one: the host's session opens BEFORE the uploads of 2 are queued and is drained after.
//
// gkr_mimc7_multi_hash_device is the same kernel through the same launcher for a caller's own rows.
//
// Requirement (verify_core.h states it where the order lives): the device computes from proof elements nobody has checked yet,
// so some of its values may be garbage; the relations consult a value only after the elements behind it passed their own checks.
#include "verify_chunk.h"
#include "verify_core.h"

struct gkr_verify_circuit {
    int device = 0;
    std::vector<uint32_t> k;       // the handle's own copy: L + 1 entries
    std::vector<uint2*> gates;     // per layer 2^k[i] packed records (kernels_verify.hip, k_verify_pack)
};

namespace {

using gkr::h64::F;
namespace V = gkr::verify;

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

using V::HashSlot;                     // (verify_rounds.h)
constexpr size_t kHashRowWords = 24;   // a round vector of the layer sumcheck: three slots

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
    // ---- 1. the hashes start: on the context's host pool, whose workers take pieces from here on (the job's guard closes the
    //         session on every way out, before the slots go), or -- a chunk of enough round vectors -- on the device, further down,
    //         once the workspaces are there (no piece is left for the pool then)
    RowSet rows{3u, sh.rounds, {}};
    for (uint32_t p = 0; p < nb; ++p) rows.spans.push_back({proofs[p].sumcheck_coeffs, proofs[p].sumcheck_len});
    RoundHashes hashes(ctx, "verify_", {std::move(rows)});
    gkr::PieceJob hashing(hashes.host_pieces() && hashes.rows() >= 64 ? ctx->host_pool() : nullptr,   // waking the pool is worth some tens of hashes
                          hashes.host_pieces(), [&](size_t a) { hashes.hash_piece(a); });
    // ---- 2. upload, every launch, one copy back
    const uint32_t pstride = (uint32_t)(sh.zlen + sh.rounds);
    Fr *d_pts, *d_dco, *d_ico, *d_tables, *d_mono, *d_partials, *d_out;
    gkr::VerifyLayer* d_layers;
    WS_OR_NOMEM(ctx, "verify_pts", Fr, (size_t)nb * pstride + 1, d_pts);
    WS_OR_NOMEM(ctx, "verify_dco", Fr, (size_t)nb * sh.n_d, d_dco);
    WS_OR_NOMEM(ctx, "verify_ico", Fr, (size_t)nb * sh.n_in, d_ico);
    WS_OR_NOMEM(ctx, "verify_tables", Fr, (size_t)nb * sh.table_elems, d_tables);
    WS_OR_NOMEM(ctx, "verify_mono", Fr, (size_t)nb * sh.mono_elems, d_mono);
    WS_OR_NOMEM(ctx, "verify_partials", Fr, (size_t)nb * sh.partial_elems, d_partials);
    WS_OR_NOMEM(ctx, "verify_out", Fr, (size_t)nb * sh.out_elems + (2 * (size_t)nb * sizeof(uint32_t) + sizeof(Fr) - 1) / sizeof(Fr), d_out);
    WS_OR_NOMEM(ctx, "verify_layers", gkr::VerifyLayer, L, d_layers);
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
    if (const int rc = hashes.start()) return rc;   // (the device's share of 1)
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
    if (const int rc = hashes.join()) return rc;   // the slots are back before the results are
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    // ---- 3. this thread hashes too (the host's pieces, if there are any), then the one synchronisation and the relations
    hashing.drain();
    if (const int rc = hashes.sync_main()) return rc;
    const Fr* h_evals = h_out + (size_t)nb * 2 * L;
    const uint32_t* h_flags = reinterpret_cast<const uint32_t*>(h_out + (size_t)nb * sh.out_elems);
    for (uint32_t p = 0; p < nb; ++p) {
        const Fr evals[2] = {h_evals[p], h_evals[nb + p]};
        DeviceProvider prov{L, sh.rounds, sh.last_row.data(), hashes.slots() + (size_t)p * sh.rounds, h_out + (size_t)p * 2 * L, evals, h_flags + 2 * (size_t)p};
        uint32_t fl = 0, fc = 0;
        const int rc = V::relations(L, k.data(), &proofs[p], prov, &accept[p], &fl, &fc);
        if (rc) return ctx->fail(rc, "gkr_verify_prepared: the relations of a proof could not be evaluated");
        if (failed_layer) failed_layer[p] = fl;
        if (failed_check) failed_check[p] = fc;
    }
    return GKR_OK;
}

}  // namespace

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
    return for_chunks(batch, verify_chunk_size(sh.bytes_per_proof(), 32768, batch), [&](size_t b, uint32_t nb) {
        return verify_chunk(ctx, vc, sh, proofs + b, nb, accept + b, failed_layer ? failed_layer + b : nullptr,
                            failed_check ? failed_check + b : nullptr);
    });
}

int gkr_mimc7_multi_hash_device(gkr_ctx* ctx, const gkr_fr* rows, const uint32_t* len, size_t n, gkr_fr* out, uint32_t* valid) {
    if (!ctx || !rows || !len || !out || !valid || n == 0) return GKR_ERR_INVALID;
    GKR_ENTER(ctx);
    constexpr size_t kPieceRows = (size_t)1 << 18;   // 25 MiB up, 10 MiB back per piece
    const size_t cap = std::min(n, kPieceRows);
    uint32_t *d_in, *h_in;
    gkr::VerifyHashSlot *d_out, *h_out;
    WS_OR_NOMEM(ctx, "verify_hash_in", uint32_t, cap * (kHashRowWords + 1), d_in);
    WS_OR_NOMEM(ctx, "verify_hash_out", gkr::VerifyHashSlot, cap, d_out);
    HIP_TRY(ctx, ctx->pinned_host("verify_hash_in", cap * (kHashRowWords + 1) * sizeof(uint32_t), reinterpret_cast<void**>(&h_in)));
    HIP_TRY(ctx, ctx->pinned_host("verify_hash_out", cap * sizeof(gkr::VerifyHashSlot), reinterpret_cast<void**>(&h_out)));
    for (size_t a = 0; a < n; a += cap) {
        const size_t m = std::min(cap, n - a);
        memcpy(h_in, rows + a * 3, m * kHashRowWords * sizeof(uint32_t));
        memcpy(h_in + m * kHashRowWords, len + a, m * sizeof(uint32_t));
        HIP_TRY(ctx, hipMemcpyAsync(d_in, h_in, m * (kHashRowWords + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        if (const int rc = verify_hash_rows_device(ctx, 3, d_in, d_in + m * kHashRowWords, m, d_out, ctx->stream)) return rc;
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

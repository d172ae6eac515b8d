// The verifier of the R1CS argument's two sumchecks (capi_r1cs.hip proves them): gkr_r1cs_matrix_evals_device, the three matrices'
// multilinear extensions at a point in one pass over the resident CSR records (kernels_r1cs.hip), and gkr_r1cs_verify_batch_device
// / gkr_r1cs_verify, which hold the zero-check's and the inner sumcheck's transcripts against z, rho, the public matrices and --
// where the caller has it -- the witness.  C ABI: include/gkr_amd.h.
//
// A verifier holds no table: the last relation of either transcript is a value formed on the host (eq(z, r_x) (v_A v_B - v_C);
// e_T e_w), and what ties the claims to the R1CS is e_T = sum_m rho_m M_m~(r_x, r_y), the device's share.  The round relations are
// the sumcheck verifiers' own (verify_rounds.h).  A chunk of proofs is built from verify_chunk.h's pieces, which states the plan.
// Particular to this file:
//   - two sets of round vectors, the zero-check's rows of four slots and the inner sumcheck's of three: two hash launches;
//   - the host's relations (shape, canonical checks, round sums and Horner steps of both transcripts; the inner one's claim is
//     sum_m rho_m v_m, so it follows the zero-check's canonical checks) run BEFORE the device's share is queued: only the points
//     (r_x, r_y) of the proofs that passed SHAPE and NON_CANONICAL go up, zeros for the others, whose verdict is decided.  The
//     host's hashes (if any) run after it is queued, while the device works;
//   - the device's share: the eq tables, the matrix pass and, with a witness, its padded copy and its evaluation (whose points are
//     on the device already);
//   - per proof the first failure in the order of the stages.
#include "verify_chunk.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
using V::HashSlot;
using V::Pre;

constexpr uint32_t kEqMaxVars = 28;   // launch_eq_table's limit
constexpr size_t kRelPiece = 8;       // proofs per piece of host work

// the CSC info's rule for the columns' variables, from the rows handle's n_wires
uint32_t n_y_of(uint32_t n_wires) {
    uint32_t n_y = 2;
    while (((uint64_t)1 << n_y) < n_wires) ++n_y;
    return n_y;
}

// the argument checks every entry point shares (plain returns: decided before the context is looked at)
bool matrix_args(const gkr_ctx* ctx, const gkr_r1cs_rows* rows, int batch) {
    if (!ctx || !rows) return false;
    if (batch < 1 || batch > 65535) return false;
    if (rows->ctx != ctx) return false;
    const uint32_t n = rows->info.n, n_y = n_y_of(rows->info.n_wires);
    if (n > kEqMaxVars || n_y > kEqMaxVars) return false;
    if ((unsigned long long)batch * (((unsigned long long)1 << n) + ((unsigned long long)1 << n_y)) > (1ull << 30)) return false;
    return true;
}

// proofs of a chunk: what fits verify_workspace_mb (the eq tables, the partials, the points; with a witness its padded copy and
// the evaluation's workspace; with hashes both transcripts' rows and slots)
size_t chunk_proofs(const gkr_r1cs_rows* rows, int batch, bool witness, bool hashes) {
    const uint32_t n = rows->info.n, n_y = n_y_of(rows->info.n_wires);
    size_t one = sizeof(Fr) * (((size_t)1 << n) + ((size_t)1 << n_y) + 3 * (size_t)gkr::r1cs_matrix_eval_slots(rows->csr()) + n + n_y + 3);
    if (witness) one += sizeof(Fr) * (((size_t)1 << n_y) + 1) + gkr::mle_eval_ws_bytes(n_y, 1, 1);
    if (hashes) one += (size_t)n * (4 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot)) +
                       (size_t)n_y * (3 * sizeof(Fr) + sizeof(uint32_t) + sizeof(gkr::VerifyHashSlot));
    return verify_chunk_size(one, 32768, batch);   // (the proof is a grid dimension of the launches)
}

// The device side of `nb` proofs, queued on the main stream: h_pts (pinned: nb x n coordinates x_b, then nb x n_y coordinates
// y_b) up, the two eq tables per proof, the matrix pass, h_out (pinned: nb x 3) down.  *d_y: the y points on the device.
int queue_matrix_evals(gkr_ctx* ctx, const gkr_r1cs_rows* rows, uint32_t nb, const Fr* h_pts, Fr* h_out, const Fr** d_y) {
    hipStream_t s = ctx->stream;
    const uint32_t n = rows->info.n, n_y = n_y_of(rows->info.n_wires);
    const gkr::R1csCsr csr = rows->csr();
    const size_t n_pts = (size_t)nb * (n + n_y), slots = gkr::r1cs_matrix_eval_slots(csr);
    Fr *d_pts = nullptr, *d_ex = nullptr, *d_ey = nullptr, *d_part = nullptr, *d_out = nullptr;
    WS_OR_NOMEM(ctx, "r1cs.mat.points", Fr, n_pts, d_pts);
    WS_OR_NOMEM(ctx, "r1cs.mat.ex", Fr, (size_t)nb << n, d_ex);
    WS_OR_NOMEM(ctx, "r1cs.mat.ey", Fr, (size_t)nb << n_y, d_ey);
    WS_OR_NOMEM(ctx, "r1cs.mat.partials", Fr, (size_t)nb * 3 * slots, d_part);
    WS_OR_NOMEM(ctx, "r1cs.mat.out", Fr, (size_t)nb * 3, d_out);
    HIP_TRY(ctx, hipMemcpyAsync(d_pts, h_pts, n_pts * sizeof(Fr), hipMemcpyHostToDevice, s));
    {
        Timed t(ctx, "r1cs_mat_eq", (double)nb * 32.0 * (double)(((size_t)1 << n) + ((size_t)1 << n_y)));
        gkr::launch_eq_table(d_pts, n, 0u, n, d_ex, true, nb, s);                            // Montgomery: ex[i] * s_i is one product
        gkr::launch_eq_table(d_pts + (size_t)nb * n, n_y, 0u, n_y, d_ey, false, nb, s);     // canonical: the gathered vector
    }
    {
        Timed t(ctx, "r1cs_mat", (double)nb * (8.0 * rows->terms_total + 32.0 * rows->terms_total + 32.0 * 3.0 * (double)rows->info.n_constraints));
        gkr::launch_r1cs_matrix_evals(csr, d_ex, d_ey, n_y, nb, d_part, d_out, s);
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_out, (size_t)nb * 3 * sizeof(Fr), hipMemcpyDeviceToHost, s));
    if (d_y) *d_y = d_pts + (size_t)nb * n;
    return GKR_OK;
}

// ---- the verifier

// a chunk's share of the caller's arrays, in the ABI's layouts (proof b of the chunk at b x its rows)
struct Transcripts {
    const gkr_fr *z, *coeffs_x, *r_x, *evals_abc, *rho, *coeffs_y, *r_y, *evals_tw;
    const uint32_t *len_x, *len_y;
};

// what the host knows about a proof before the hashes and the device's values are there
struct ProofPre {
    Pre x, y;                  // the two transcripts' (y only where stage 1 passed SHAPE and NON_CANONICAL)
    uint32_t check1 = 0, round1 = 0, check2 = 0, round2 = 0;   // SHAPE / NON_CANONICAL of the two stages, the evaluations included
    bool point = false;        // both passed: (r_x, r_y) is a point and goes to the device
};

inline F mul(const F& a, const F& b) { return gkr::h64::mont_mul(gkr::h64::to_mont(a), b); }   // canonical x canonical -> canonical

ProofPre proof_pre(int n, int n_y, const Transcripts& t, size_t b) {
    static const gkr_fr kZero = {{0, 0, 0, 0}};
    ProofPre p;
    p.x = V::pre_relations(n, 3, &kZero, t.coeffs_x + 4 * b * n, t.len_x + b * n, t.r_x + b * n);
    p.check1 = p.x.check;
    p.round1 = p.x.round;
    const gkr_fr* abc = t.evals_abc + 3 * b;
    if (!p.check1 && !(V::canonical(abc[0]) && V::canonical(abc[1]) && V::canonical(abc[2]))) {
        p.check1 = GKR_VERIFY_NON_CANONICAL;
        p.round1 = (uint32_t)n;
    }
    if (p.check1) return p;
    F claim = {{0, 0, 0, 0}};                                        // sum_m rho_m v_m
    for (int m = 0; m < 3; ++m) claim = gkr::h64::add(claim, mul(V::load(t.rho[3 * b + m]), V::load(abc[m])));
    gkr_fr claim_abi;
    memcpy(claim_abi.l, claim.l, 32);
    p.y = V::pre_relations(n_y, 2, &claim_abi, t.coeffs_y + 3 * b * n_y, t.len_y + b * n_y, t.r_y + b * n_y);
    p.check2 = p.y.check;
    p.round2 = p.y.round;
    const gkr_fr* tw = t.evals_tw + 2 * b;
    if (!p.check2 && !(V::canonical(tw[0]) && V::canonical(tw[1]))) {
        p.check2 = GKR_VERIFY_NON_CANONICAL;
        p.round2 = (uint32_t)n_y;
    }
    p.point = !p.check2;
    return p;
}

struct Verdict {
    uint32_t stage = 0, round = 0, check = 0;
};

// the first failure of one proof, in the order of the stages; mats: M_m~(r_x, r_y), w_eval: w~(r_y) or null (no witness given)
int proof_verdict(gkr_ctx* ctx, int n, int n_y, const Transcripts& t, size_t b, const ProofPre& p, const HashSlot* slots_x, const HashSlot* slots_y,
                  const Fr* mats, const Fr* w_eval, Verdict* out) {
    const char* no_hash = "R1CS verifier: no hash for a well-formed round vector";
    // stage 1: the zero-check's transcript against claim 0 and eq(z, r_x) (v_A v_B - v_C)
    Pre x = p.x;
    x.check = p.check1;
    x.round = p.round1;
    out->stage = 1;
    if (!V::round_verdict(n, x, slots_x, t.r_x + b * n, &out->check, &out->round)) return ctx->fail(GKR_ERR_HIP, no_hash);
    if (out->check) return GKR_OK;
    const gkr_fr* abc = t.evals_abc + 3 * b;
    const F one = {{1, 0, 0, 0}};
    F eq = one;                                                      // the n-factor product prod_j (z_j r_j + (1 - z_j)(1 - r_j))
    for (int j = 0; j < n; ++j) {
        const F zj = V::load(t.z[b * n + j]), rj = V::load(t.r_x[b * n + j]), zr = mul(zj, rj);
        eq = mul(eq, gkr::h64::add(gkr::h64::sub(gkr::h64::sub(one, zj), rj), gkr::h64::add(zr, zr)));
    }
    if (!V::same(x.last, mul(eq, gkr::h64::sub(mul(V::load(abc[0]), V::load(abc[1])), V::load(abc[2]))))) {
        out->check = GKR_VERIFY_EVALUATION;
        out->round = (uint32_t)n;
        return GKR_OK;
    }
    // stage 2: the inner transcript against sum_m rho_m v_m and e_T e_w
    Pre y = p.y;
    y.check = p.check2;
    y.round = p.round2;
    out->stage = 2;
    if (!V::round_verdict(n_y, y, slots_y, t.r_y + b * n_y, &out->check, &out->round)) return ctx->fail(GKR_ERR_HIP, no_hash);
    if (out->check) return GKR_OK;
    const F e_t = V::load(t.evals_tw[2 * b]), e_w = V::load(t.evals_tw[2 * b + 1]);
    if (!V::same(y.last, mul(e_t, e_w))) {
        out->check = GKR_VERIFY_EVALUATION;
        out->round = (uint32_t)n_y;
        return GKR_OK;
    }
    // stage 3: e_T against the public matrices
    F total = {{0, 0, 0, 0}};
    for (int m = 0; m < 3; ++m) {
        F v;
        memcpy(v.l, &mats[m], 32);
        total = gkr::h64::add(total, mul(V::load(t.rho[3 * b + m]), v));
    }
    out->round = (uint32_t)n_y;
    if (!V::same(e_t, total)) {
        out->stage = 3;
        out->check = GKR_VERIFY_MATRIX;
        return GKR_OK;
    }
    // stage 4: e_w against the witness
    if (w_eval) {
        F w;
        memcpy(w.l, w_eval, 32);
        if (!V::same(e_w, w)) {
            out->stage = 4;
            out->check = GKR_VERIFY_WITNESS;
            return GKR_OK;
        }
    }
    *out = Verdict();
    return GKR_OK;
}

int verify_chunk(gkr_ctx* ctx, const gkr_r1cs_rows* rows, uint32_t nb, const Transcripts& t, const Fr* d_witness, size_t stride, int* accept,
                 uint32_t* failed_stage, uint32_t* failed_round, uint32_t* failed_check) {
    hipStream_t st = ctx->stream;
    const int n = (int)rows->info.n, n_y = (int)n_y_of(rows->info.n_wires);
    const size_t rows_x = (size_t)nb * n, rows_y = (size_t)nb * n_y, n_rows = rows_x + rows_y;
    // ---- 1. the hashes on the side stream: the zero-check's rows of four slots, then the inner sumcheck's of three
    RoundHashes hashes(ctx, "r1cs.ver.", {RowSet{4u, rows_x, {{t.coeffs_x, t.len_x}}}, RowSet{3u, rows_y, {{t.coeffs_y, t.len_y}}}});
    if (const int rc = hashes.start()) return rc;
    // ---- 2. the relations that need neither a hash nor a device value, in pieces of kRelPiece proofs
    std::vector<ProofPre> pre(nb);
    for_pieces(ctx, (nb + kRelPiece - 1) / kRelPiece, 8, [&](size_t a) {
        for (size_t b = a * kRelPiece; b < std::min<size_t>(nb, (a + 1) * kRelPiece); ++b) pre[b] = proof_pre(n, n_y, t, b);
    });
    // ---- 3. the device's share: the points of the proofs still standing, zeros for the others
    Fr *h_pts = nullptr, *h_out = nullptr;
    HIP_TRY(ctx, ctx->pinned_host("r1cs.mat.points", n_rows * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
    HIP_TRY(ctx, ctx->pinned_host("r1cs.mat.out", (size_t)nb * 4 * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
    memset(h_pts, 0, n_rows * sizeof(Fr));
    for (uint32_t b = 0; b < nb; ++b)
        if (pre[b].point) {
            memcpy(h_pts + (size_t)b * n, t.r_x + (size_t)b * n, (size_t)n * sizeof(Fr));
            memcpy(h_pts + rows_x + (size_t)b * n_y, t.r_y + (size_t)b * n_y, (size_t)n_y * sizeof(Fr));
        }
    const Fr* d_y = nullptr;
    if (const int rc = queue_matrix_evals(ctx, rows, nb, h_pts, h_out, &d_y)) return rc;
    Fr* h_w = nullptr;
    if (d_witness) {   // stage 4's value: the witness zero-padded to 2^n_y, evaluated at r_y
        const size_t len = (size_t)1 << n_y;
        Fr *d_pad = nullptr, *d_w = nullptr;
        unsigned char* d_ws = nullptr;
        WS_OR_NOMEM(ctx, "r1cs.ver.witness", Fr, (size_t)nb * len, d_pad);
        WS_OR_NOMEM(ctx, "r1cs.ver.w_out", Fr, nb, d_w);
        WS_OR_NOMEM(ctx, "r1cs.ver.eval_ws", unsigned char, gkr::mle_eval_ws_bytes((uint32_t)n_y, nb, 1), d_ws);
        gkr::launch_r1cs_pad_witness(d_witness, stride, rows->info.n_wires, (uint32_t)n_y, nb, d_pad, len, st);
        {
            Timed tm(ctx, "mle_eval", (double)nb * 32.0 * (double)len);
            gkr::launch_mle_eval(d_pad, (uint32_t)n_y, nb, 1u, d_y, d_ws, d_w, st);
        }
        HIP_TRY(ctx, hipGetLastError());
        h_w = h_out + (size_t)nb * 3;
        HIP_TRY(ctx, hipMemcpyAsync(h_w, d_w, (size_t)nb * sizeof(Fr), hipMemcpyDeviceToHost, st));
    }
    if (const int rc = hashes.join()) return rc;
    // ---- 4. the host's hashes (if any) while the device works
    for_pieces(ctx, hashes.host_pieces(), 8, [&](size_t a) { hashes.hash_piece(a); });
    if (const int rc = hashes.sync_main()) return rc;
    const HashSlot* slots = hashes.slots();
    ctx->drain_events();
    for (uint32_t b = 0; b < nb; ++b) {
        Verdict v;
        if (const int rc = proof_verdict(ctx, n, n_y, t, b, pre[b], slots + (size_t)b * n, slots + rows_x + (size_t)b * n_y, h_out + (size_t)b * 3,
                                         h_w ? h_w + b : nullptr, &v))
            return rc;
        accept[b] = v.check == 0 ? 1 : 0;
        if (failed_stage) failed_stage[b] = v.stage;
        if (failed_round) failed_round[b] = v.round;
        if (failed_check) failed_check[b] = v.check;
    }
    return GKR_OK;
}

}  // namespace

extern "C" {

int gkr_r1cs_matrix_evals_device(gkr_ctx* ctx, const gkr_r1cs_rows* rows, const gkr_fr* x, const gkr_fr* y, int batch, gkr_fr* out) {
    if (!x || !y || !out || !matrix_args(ctx, rows, batch)) return GKR_ERR_INVALID;
    const uint32_t n = rows->info.n, n_y = n_y_of(rows->info.n_wires);
    if (!all_canonical(x, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "x entry >= r");
    if (!all_canonical(y, (size_t)batch * n_y)) return ctx->fail(GKR_ERR_NON_CANONICAL, "y entry >= r");
    GKR_ENTER(ctx);
    return for_chunks(batch, chunk_proofs(rows, batch, false, false), [&](size_t b, uint32_t nb) -> int {
        Fr *h_pts = nullptr, *h_out = nullptr;
        HIP_TRY(ctx, ctx->pinned_host("r1cs.mat.points", (size_t)nb * (n + n_y) * sizeof(Fr), reinterpret_cast<void**>(&h_pts)));
        HIP_TRY(ctx, ctx->pinned_host("r1cs.mat.out", (size_t)nb * 3 * sizeof(Fr), reinterpret_cast<void**>(&h_out)));
        memcpy(h_pts, x + b * n, (size_t)nb * n * sizeof(Fr));
        memcpy(h_pts + (size_t)nb * n, y + b * n_y, (size_t)nb * n_y * sizeof(Fr));
        if (const int rc = queue_matrix_evals(ctx, rows, nb, h_pts, h_out, nullptr)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->drain_events();
        memcpy(out + b * 3, h_out, (size_t)nb * 3 * sizeof(Fr));
        return GKR_OK;
    });
}

int gkr_r1cs_verify_batch_device(gkr_ctx* ctx, const gkr_r1cs_rows* rows, int batch, const gkr_fr* z, const gkr_fr* coeffs_x, const uint32_t* len_x,
                                 const gkr_fr* r_x, const gkr_fr* evals_abc, const gkr_fr* rho, const gkr_fr* coeffs_y, const uint32_t* len_y,
                                 const gkr_fr* r_y, const gkr_fr* evals_tw, const void* d_witness, size_t stride_elements, int* accept,
                                 uint32_t* failed_stage, uint32_t* failed_round, uint32_t* failed_check) {
    if (!z || !coeffs_x || !len_x || !r_x || !evals_abc || !rho || !coeffs_y || !len_y || !r_y || !evals_tw || !accept) return GKR_ERR_INVALID;
    if (!matrix_args(ctx, rows, batch)) return GKR_ERR_INVALID;
    if (d_witness && stride_elements < rows->info.n_wires) return GKR_ERR_INVALID;
    const size_t n = rows->info.n, n_y = n_y_of(rows->info.n_wires);
    // z and rho are the verifier's own: an entry >= r is an error of the call, not a verdict
    if (!all_canonical(z, (size_t)batch * n)) return ctx->fail(GKR_ERR_NON_CANONICAL, "z entry >= r");
    if (!all_canonical(rho, (size_t)batch * 3)) return ctx->fail(GKR_ERR_NON_CANONICAL, "rho entry >= r");
    GKR_ENTER(ctx);
    return for_chunks(batch, chunk_proofs(rows, batch, d_witness != nullptr, true), [&](size_t b, uint32_t nb) {
        Transcripts t;
        t.z = z + b * n;
        t.coeffs_x = coeffs_x + 4 * b * n;
        t.len_x = len_x + b * n;
        t.r_x = r_x + b * n;
        t.evals_abc = evals_abc + 3 * b;
        t.rho = rho + 3 * b;
        t.coeffs_y = coeffs_y + 3 * b * n_y;
        t.len_y = len_y + b * n_y;
        t.r_y = r_y + b * n_y;
        t.evals_tw = evals_tw + 2 * b;
        return verify_chunk(ctx, rows, nb, t, d_witness ? static_cast<const Fr*>(d_witness) + b * stride_elements : nullptr, stride_elements,
                            accept + b, failed_stage ? failed_stage + b : nullptr, failed_round ? failed_round + b : nullptr,
                            failed_check ? failed_check + b : nullptr);
    });
}

int gkr_r1cs_verify(gkr_ctx* ctx, const gkr_r1cs* r1cs, const gkr_fr* z, const gkr_fr* coeffs_x, const uint32_t* len_x, const gkr_fr* r_x,
                    const gkr_fr* evals_abc, const gkr_fr* rho, const gkr_fr* coeffs_y, const uint32_t* len_y, const gkr_fr* r_y,
                    const gkr_fr* evals_tw, const gkr_fr* witness, size_t n_witness, int* accept, uint32_t* failed_stage, uint32_t* failed_round,
                    uint32_t* failed_check) {
    if (!ctx || !r1cs || !z || !coeffs_x || !len_x || !r_x || !evals_abc || !rho || !coeffs_y || !len_y || !r_y || !evals_tw || !accept)
        return GKR_ERR_INVALID;
    gkr_r1cs_csr_info_t info;
    if (const int rc = gkr_r1cs_csr_info(r1cs, &info)) return rc;
    if (witness && n_witness < info.n_wires) return GKR_ERR_INVALID;
    if (witness && !all_canonical(witness, info.n_wires)) return ctx->fail(GKR_ERR_NON_CANONICAL, "witness entry >= r");
    gkr_r1cs_rows* raw = nullptr;
    if (const int rc = gkr_r1cs_rows_prepare(ctx, r1cs, &raw)) return rc;
    std::unique_ptr<gkr_r1cs_rows, void (*)(gkr_r1cs_rows*)> rows(raw, gkr_r1cs_rows_free);
    DevBuf<Fr> d;
    if (witness) {
        GKR_ENTER(ctx);
        HIP_TRY(ctx, d.alloc(info.n_wires));
        HIP_TRY(ctx, hipMemcpy(d.p, witness, (size_t)info.n_wires * sizeof(Fr), hipMemcpyHostToDevice));
    }
    return gkr_r1cs_verify_batch_device(ctx, rows.get(), 1, z, coeffs_x, len_x, r_x, evals_abc, rho, coeffs_y, len_y, r_y, evals_tw, d.p,
                                        info.n_wires, accept, failed_stage, failed_round, failed_check);
}

}  // extern "C"

// The verifier's relations that cost O(rounds) -- ONE copy, shared by gkr_verify (dropin.cpp: everything on the host) and
// gkr_verify_prepared (capi_verify.hip: the O(gates) and O(2^k) sums on the device).  The relations and their ORDER are the
// reference's (python/gkr.py:202-231, python/sumcheck.py:55-70): Z0, the canonical scan and D(z[0]) of the output table; per
// layer and round the shape, the canonical checks, the round sum, the challenge hash and the Horner step; q, the final claim
// against add_i / mult_i, r*, the next z; at the end the canonical scan and the evaluation of the input table.
//
// What is O(gates) or O(2^k) comes from a PROVIDER:
//     int  layer_ready(i)                               status of the CALL before layer i is looked at (GKR_OK to go on)
//     bool table_canonical(which)                       every coefficient of d_coeffs (0) / input_coeffs (1) below r?
//     F    table_eval(which, z_m)                       sum_S c[S] prod_{j in S} z_j, canonical (z_m Montgomery)
//     int  hash(slot, g, len, &h)                       multi_hash of a round vector; slot = its row, or rounds + i for r* of layer i
//     int  wiring(i, z_m, b_m, c_m, &add_m, &mult_m)    add_i(z, b*, c*), mult_i(z, b*, c*) in Montgomery form; a status of the call
//
// THE ORDER IS A REQUIREMENT, not a habit.  A provider that computed its values on the device computed them from proof
// elements BEFORE anything was checked -- Montgomery arithmetic on elements >= r gives garbage.  Such a value is never
// consulted: a non-canonical challenge is caught at its own round, before that layer's final claim asks for wiring(); z[i+1]
// is checked (canonical, and equal to l(r*)) at layer i, before layer i + 1 or the input table uses it; table_eval() is asked
// only after table_canonical() said yes, and D(z[0]) only after z[0] was found to be zero.  Keep it that way.
//
// Plain C++: compiled by g++ (dropin.cpp) and by hipcc as host code (capi_verify.hip).
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/gkr_amd.h"
#include "fr64.h"

namespace gkr {
namespace verify {

using gkr::h64::F;

inline F load(const gkr_fr& x) {
    F f;
    memcpy(f.l, x.l, 32);
    return f;
}
inline bool canonical(const gkr_fr& x) { return !gkr::h64::geq_mod(load(x)); }
inline bool is_one(const gkr_fr& x) { return x.l[0] == 1 && !(x.l[1] | x.l[2] | x.l[3]); }
inline bool is_zero(const gkr_fr& x) { return !(x.l[0] | x.l[1] | x.l[2] | x.l[3]); }
inline bool same(const F& a, const F& b) { return memcmp(a.l, b.l, 32) == 0; }

// Horner, highest degree first (poly.rs:260-267); coefficients canonical, x Montgomery -> canonical
inline F horner(const gkr_fr* c, int n, const F& x_m) {
    F acc = {{0, 0, 0, 0}};
    for (int i = 0; i < n; ++i) acc = gkr::h64::add(gkr::h64::mont_mul(acc, x_m), load(c[i]));
    return acc;
}

// the argument checks every verifier entry point applies to a circuit's k list (nothing but depth and k is read)
inline int check_k_list(const gkr_circuit_desc* circuit) {
    if (!circuit || !circuit->k || circuit->depth < 1 || circuit->depth > 4096) return GKR_ERR_INVALID;
    for (uint32_t i = 0; i <= circuit->depth; ++i) {
        // k[i+1] == 0: a layer with no sumcheck rounds, which gkr_prove refuses as well (check_circuit)
        if (i > 0 && circuit->k[i] == 0) return GKR_ERR_DEGENERATE;
        if (circuit->k[i] > (i == 0 ? (uint32_t)GKR_MAX_K_I : (uint32_t)GKR_MAX_K_NEXT)) return GKR_ERR_INVALID;
    }
    return GKR_OK;
}
inline bool proof_pointers_set(const gkr_proof_buf* proof) {
    return proof->sumcheck_coeffs && proof->sumcheck_len && proof->sumcheck_r && proof->q && proof->q_len && proof->z && proof->r &&
           proof->d_coeffs && proof->input_coeffs;
}

template <class Provider>
int relations(uint32_t L, const uint32_t* ks, const gkr_proof_buf* proof, Provider& prov, int* accept, uint32_t* failed_layer,
              uint32_t* failed_check) {
    *accept = 0;
    auto reject = [&](uint32_t layer, uint32_t check) {
        if (failed_layer) *failed_layer = layer;
        if (failed_check) *failed_check = check;
        return GKR_OK;
    };
    const F zero = {{0, 0, 0, 0}};
    size_t rounds = 0;
    for (uint32_t i = 0; i < L; ++i) rounds += 2 * (size_t)ks[i + 1];
    // z[0] = 0 (prover.rs:16-21) and m_0 = D(z[0])
    const gkr_fr* z = proof->z;
    std::vector<F> zi_m(ks[0]);
    for (uint32_t j = 0; j < ks[0]; ++j) {
        if (!is_zero(z[j])) return reject(0, GKR_VERIFY_Z0);
        zi_m[j] = zero;
    }
    if (!prov.table_canonical(0)) return reject(0, GKR_VERIFY_NON_CANONICAL);
    F m = prov.table_eval(0, zi_m);
    size_t row = 0, qo = 0, zo = ks[0];
    for (uint32_t i = 0; i < L; ++i) {
        const int k = (int)ks[i + 1];
        if (const int rc = prov.layer_ready(i)) return rc;
        // the sumcheck's rounds (python/sumcheck.py:55-70)
        F expected = m;
        std::vector<F> rs_m(2 * (size_t)k);
        for (int j = 0; j < 2 * k; ++j, ++row) {
            const uint32_t len = proof->sumcheck_len[row];
            if (len < 1 || len > 3) return reject(i, GKR_VERIFY_SHAPE);
            const gkr_fr* g = proof->sumcheck_coeffs + row * 3 + (3 - len);
            for (uint32_t t = 0; t < len; ++t)
                if (!canonical(g[t])) return reject(i, GKR_VERIFY_NON_CANONICAL);
            if (!canonical(proof->sumcheck_r[row])) return reject(i, GKR_VERIFY_NON_CANONICAL);
            F at1 = zero;                                    // g(1) = sum of the coefficients, g(0) = the constant term
            for (uint32_t t = 0; t < len; ++t) at1 = gkr::h64::add(at1, load(g[t]));
            if (!same(gkr::h64::add(at1, load(g[len - 1])), expected)) return reject(i, GKR_VERIFY_ROUND_SUM);
            gkr_fr h;
            if (prov.hash(row, g, len, &h) != GKR_OK) return GKR_ERR_INVALID;
            if (memcmp(h.l, proof->sumcheck_r[row].l, 32) != 0) return reject(i, GKR_VERIFY_CHALLENGE);
            rs_m[j] = gkr::h64::to_mont(load(proof->sumcheck_r[row]));
            expected = horner(g, (int)len, rs_m[j]);
        }
        // q(0), q(1), and the last claim against add(z,b*,c*) (q0 + q1) + mult(z,b*,c*) q0 q1 (python/gkr.py:213-219)
        const uint32_t qlen = proof->q_len[i];
        if (qlen < 1 || qlen > (uint32_t)k + 1) return reject(i, GKR_VERIFY_SHAPE);
        const gkr_fr* q = proof->q + qo + ((size_t)k + 1 - qlen);
        for (uint32_t t = 0; t < qlen; ++t)
            if (!canonical(q[t])) return reject(i, GKR_VERIFY_NON_CANONICAL);
        const F q0 = load(q[qlen - 1]);
        F q1 = zero;
        for (uint32_t t = 0; t < qlen; ++t) q1 = gkr::h64::add(q1, load(q[t]));
        std::vector<F> b_m(rs_m.begin(), rs_m.begin() + k), c_m(rs_m.begin() + k, rs_m.end());
        F add_m = zero, mult_m = zero;                        // Montgomery forms of add_i, mult_i at (z, b*, c*)
        if (const int rc = prov.wiring(i, zi_m, b_m, c_m, &add_m, &mult_m)) return rc;
        const F q01 = gkr::h64::mont_mul(gkr::h64::to_mont(q0), q1);             // canonical q0 q1
        const F want = gkr::h64::add(gkr::h64::mont_mul(add_m, gkr::h64::add(q0, q1)), gkr::h64::mont_mul(mult_m, q01));
        if (!same(want, expected)) return reject(i, GKR_VERIFY_FINAL_CLAIM);
        // r* = hash of the last round vector (prover.rs:74-78), z[i+1] = l(r*) (poly.rs:538-551), m = q(r*)
        {
            const size_t last = row - 1;
            const uint32_t len = proof->sumcheck_len[last];
            gkr_fr h;
            if (prov.hash(rounds + i, proof->sumcheck_coeffs + last * 3 + (3 - len), len, &h) != GKR_OK) return GKR_ERR_INVALID;
            if (memcmp(h.l, proof->r[i].l, 32) != 0) return reject(i, GKR_VERIFY_R_STAR);
        }
        const F rstar_m = gkr::h64::to_mont(load(proof->r[i]));
        zi_m.assign((size_t)k, zero);
        for (int j = 0; j < k; ++j) {
            const F bj = load(proof->sumcheck_r[row - 2 * (size_t)k + j]), cj = load(proof->sumcheck_r[row - (size_t)k + j]);
            const F zj = gkr::h64::add(bj, gkr::h64::mont_mul(rstar_m, gkr::h64::sub(cj, bj)));
            if (!canonical(z[zo + j]) || !same(zj, load(z[zo + j]))) return reject(i, GKR_VERIFY_NEXT_Z);
            zi_m[j] = gkr::h64::to_mont(zj);
        }
        m = horner(q, (int)qlen, rstar_m);
        qo += (size_t)k + 1;
        zo += (size_t)k;
    }
    if (!prov.table_canonical(1)) return reject(L, GKR_VERIFY_NON_CANONICAL);
    if (!same(m, prov.table_eval(1, zi_m))) return reject(L, GKR_VERIFY_INPUT);
    *accept = 1;
    if (failed_layer) *failed_layer = 0;
    if (failed_check) *failed_check = GKR_VERIFY_OK;
    return GKR_OK;
}

}  // namespace verify
}  // namespace gkr

// The FRACTIONAL SUM (LogUp) argument's chain of claims (include/gkr_amd.h, gkr_fraction_sum*) as the driver
// (capi_fraction_sum.hip) and its verifier use it -- ONE copy of the Fiat-Shamir steps between the layers and of the order of the
// checks.  Over tables N, D of 2^n values, (p_n, q_n) = (N, D), p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i],
// q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k]:
//   head      the prover publishes level 2, p_2[0..3] then q_2[0..3] (eight values); (P, Q) follow by the tree rule;
//             zeta_1 = multi_hash(the eight, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2),
//             lambda_2 = multi_hash([zeta_2], 0), cp_2 = p_2~(z^(2)), cq_2 = q_2~(z^(2)), variable 1 the most significant index bit;
//   layer k   = 2 .. n-1: the zero-check at z^(k) of T0 T3 + T1 T2 + lambda_k T2 T3 (T0, T1 the halves of p_{k+1}, T2, T3 of q_{k+1})
//             with claim cp_k + lambda_k cq_k: k rows of four slots, k challenges r^(k), the four values (a0, a1, b0, b1);
//             tau_k = multi_hash([a0, a1, b0, b1], 0), cp_{k+1} = a0 + tau_k (a1 - a0), cq_{k+1} = b0 + tau_k (b1 - b0),
//             z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k), lambda_{k+1} = multi_hash([tau_k], 0);
//   end       cp_n = N~(z^(n)), cq_n = D~(z^(n)).
// The layers' rows lie one after the other, layer k from row k (k - 1) / 2 - 1 on; R = n (n - 1) / 2 - 1 rows in all: the grand
// product's bookkeeping (grand_product_rounds.h), whose field helpers are used here.  The round relations are verify_rounds.h's.
// A value computed from unchecked elements is never consulted (verify_core.h): the shape and canonical checks of the WHOLE proof
// come first, and the layers' relations are consulted in ascending order.  Plain C++: no device, no context
// (tests/fraction_sum_rounds_selfcheck.cpp drives it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "grand_product_rounds.h"

namespace gkr {
namespace fs {

using verify::F;
using gp::abi;
using gp::eq_point;
using gp::lerp;
using gp::mul;

inline size_t rounds(int n) { return gp::rounds(n); }
inline size_t layer_row(int k) { return gp::layer_row(k); }   // the first row of layer k; also where z^(k) starts in Pre::z

// hash(v, len) = multi_hash of len canonical values, key 0
template <class Hash>
inline void head_point(const gkr_fr* head, const Hash& hash, F* zeta1, F* zeta2, F* lambda2) {
    F h[8];
    for (int t = 0; t < 8; ++t) h[t] = verify::load(head[t]);
    *zeta1 = hash(h, 8);
    *zeta2 = hash(zeta1, 1);
    *lambda2 = hash(zeta2, 1);
}
// (P, Q) of the head by the tree rule: level 2 -> level 1 -> level 0
inline void head_root(const gkr_fr* head, F* P, F* Q) {
    F p[4], q[4], p1[2], q1[2];
    for (int t = 0; t < 4; ++t) {
        p[t] = verify::load(head[t]);
        q[t] = verify::load(head[4 + t]);
    }
    for (int i = 0; i < 2; ++i) {
        p1[i] = gkr::h64::add(mul(p[i], q[i + 2]), mul(p[i + 2], q[i]));
        q1[i] = mul(q[i], q[i + 2]);
    }
    *P = gkr::h64::add(mul(p1[0], q1[1]), mul(p1[1], q1[0]));
    *Q = mul(q1[0], q1[1]);
}
inline void head_claims(const gkr_fr* head, const F& zeta1, const F& zeta2, F* cp, F* cq) {
    F v[8];
    for (int t = 0; t < 8; ++t) v[t] = verify::load(head[t]);
    *cp = lerp(lerp(v[0], v[2], zeta1), lerp(v[1], v[3], zeta1), zeta2);
    *cq = lerp(lerp(v[4], v[6], zeta1), lerp(v[5], v[7], zeta1), zeta2);
}
// the step behind layer k: evals = (a0, a1, b0, b1), r = r^(k) (k challenges) -> cp_{k+1}, cq_{k+1}, z^(k+1) (k + 1 coordinates)
// and lambda_{k+1}
template <class Hash>
inline void next_claims(int k, const gkr_fr* evals, const gkr_fr* r, const Hash& hash, gkr_fr* z_next, F* cp, F* cq, F* lambda_next) {
    const F v[4] = {verify::load(evals[0]), verify::load(evals[1]), verify::load(evals[2]), verify::load(evals[3])};
    const F tau = hash(v, 4);
    z_next[0] = abi(tau);
    memcpy(z_next + 1, r, (size_t)k * sizeof(gkr_fr));
    *cp = lerp(v[0], v[1], tau);
    *cq = lerp(v[2], v[3], tau);
    *lambda_next = hash(&tau, 1);
}

// one proof in the ABI's arrays: head 8, coeffs R x 4, len R, r R, evals (n - 2) x 4; sums: the claimed (P, Q) or null
struct Proof {
    const gkr_fr *sums, *head, *coeffs, *r, *evals;
    const uint32_t* len;
};
using Verdict = gp::Verdict;

// what the host knows about a proof before the round vectors' hashes and N~(z^(n)), D~(z^(n)) are there
struct Pre {
    Verdict form;                     // the first failure among SHAPE, NON_CANONICAL, ZERO_DENOMINATOR and FRACTION_SUM (check 0: none)
    bool point = false;               // SHAPE and NON_CANONICAL passed: z holds points, z^(n) may go to the device
    std::vector<verify::Pre> layer;   // layer k at k - 2
    std::vector<gkr_fr> z;            // z^(2) .. z^(n), z^(k) at layer_row(k)
    std::vector<F> cp, cq, lambda;    // cp_2 .. cp_n, cq_2 .. cq_n, lambda_2 .. lambda_n at k - 2
};

template <class Hash>
inline Pre pre_relations(int n, const Proof& p, const Hash& hash) {
    Pre out;
    auto fail = [&](uint32_t check, int layer, int round) {
        out.form.check = check;
        out.form.layer = (uint32_t)layer;
        out.form.round = (uint32_t)round;
        return out;
    };
    for (int k = 2; k < n; ++k)
        for (int j = 0; j < k; ++j)
            if (const uint32_t len = p.len[layer_row(k) + j]; len < 1 || len > 4) return fail(GKR_VERIFY_SHAPE, k, j);
    for (int t = 0; t < 8; ++t)
        if (!verify::canonical(p.head[t])) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    if (p.sums && (!verify::canonical(p.sums[0]) || !verify::canonical(p.sums[1]))) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    for (int k = 2; k < n; ++k) {
        for (int j = 0; j < k; ++j) {
            const size_t row = layer_row(k) + j;
            bool ok = verify::canonical(p.r[row]);
            for (uint32_t t = 4 - p.len[row]; t < 4; ++t) ok = ok && verify::canonical(p.coeffs[4 * row + t]);
            if (!ok) return fail(GKR_VERIFY_NON_CANONICAL, k, j);
        }
        for (int t = 0; t < 4; ++t)
            if (!verify::canonical(p.evals[4 * (k - 2) + t])) return fail(GKR_VERIFY_NON_CANONICAL, k, k);
    }
    out.point = true;
    out.z.resize(rounds(n) + (size_t)n);
    F zeta1, zeta2, lambda, cp, cq;
    head_point(p.head, hash, &zeta1, &zeta2, &lambda);
    out.z[0] = abi(zeta1);
    out.z[1] = abi(zeta2);
    head_claims(p.head, zeta1, zeta2, &cp, &cq);
    for (int k = 2;; ++k) {
        out.cp.push_back(cp);
        out.cq.push_back(cq);
        out.lambda.push_back(lambda);
        if (k == n) break;
        const size_t row = layer_row(k);
        const gkr_fr c = abi(gkr::h64::add(cp, mul(lambda, cq)));
        out.layer.push_back(verify::pre_relations(k, 3, &c, p.coeffs + 4 * row, p.len + row, p.r + row));
        next_claims(k, p.evals + 4 * (k - 2), p.r + row, hash, out.z.data() + layer_row(k + 1), &cp, &cq, &lambda);
    }
    F P, Q;
    head_root(p.head, &P, &Q);
    if (gkr::h64::is_zero(Q))
        out.form.check = GKR_VERIFY_ZERO_DENOMINATOR;
    else if (p.sums && !(verify::same(verify::load(p.sums[0]), P) && verify::same(verify::load(p.sums[1]), Q)))
        out.form.check = GKR_VERIFY_FRACTION_SUM;
    return out;
}

// The first failure of a proof: pre's own, else layer by layer the rounds (CHALLENGE / ROUND_SUM at (k, j)) and the layer's last
// relation g_k(r_k) = eq(z^(k), r^(k)) (a0 b1 + a1 b0 + lambda_k b0 b1) (FINAL_CLAIM at (k, k)), else cp_n against vn = N~(z^(n)) and
// cq_n against vd = D~(z^(n)) (EVALUATION at (n, n)).  slots: the hash slots of the proof's R rows.  false: a well-formed round
// vector has no hash (an error of the CALL).
inline bool verdict(int n, const Proof& p, const Pre& pre, const verify::HashSlot* slots, const F& vn, const F& vd, Verdict* out) {
    *out = pre.form;
    if (out->check) return true;
    for (int k = 2; k < n; ++k) {
        const size_t row = layer_row(k);
        const verify::Pre& lp = pre.layer[k - 2];
        out->layer = (uint32_t)k;
        if (!verify::round_verdict(k, lp, slots + row, p.r + row, &out->check, &out->round)) return false;
        if (out->check) return true;
        const gkr_fr* e = p.evals + 4 * (k - 2);
        const F a0 = verify::load(e[0]), a1 = verify::load(e[1]), b0 = verify::load(e[2]), b1 = verify::load(e[3]);
        const F g = gkr::h64::add(gkr::h64::add(mul(a0, b1), mul(a1, b0)), mul(pre.lambda[k - 2], mul(b0, b1)));
        if (!verify::same(lp.last, mul(eq_point(k, pre.z.data() + row, p.r + row), g))) {
            out->check = GKR_VERIFY_FINAL_CLAIM;
            out->round = (uint32_t)k;
            return true;
        }
    }
    if (!verify::same(pre.cp.back(), vn) || !verify::same(pre.cq.back(), vd)) {
        out->check = GKR_VERIFY_EVALUATION;
        out->layer = out->round = (uint32_t)n;
        return true;
    }
    *out = Verdict();
    return true;
}

}  // namespace fs
}  // namespace gkr

// The GRAND PRODUCT argument's chain of claims (include/gkr_amd.h, gkr_grand_product*) as the driver (capi_grand_product.hip) and
// its verifier use it -- ONE copy of the Fiat-Shamir steps between the layers and of the order of the checks.  Over a table V of
// 2^n values, L_n = V, L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k]:
//   head      the prover publishes L_2 (four values); P = their product; zeta_1 = multi_hash(L_2, 0), zeta_2 = multi_hash([zeta_1], 0),
//             z^(2) = (zeta_1, zeta_2), c_2 = L_2~(z^(2)), variable 1 the most significant index bit;
//   layer k   = 2 .. n-1: the zero-check of eq(z^(k), .) L_{k+1}[0 ..) L_{k+1}[2^k ..) with claim c_k: k rows of four slots, k
//             challenges r^(k), the two values (a_k, b_k); tau_k = multi_hash([a_k, b_k], 0), c_{k+1} = a_k + tau_k (b_k - a_k),
//             z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k);
//   end       c_n = V~(z^(n)).
// The layers' rows lie one after the other, layer k from row k (k - 1) / 2 - 1 on; R = n (n - 1) / 2 - 1 rows in all.
// The round relations are verify_rounds.h's.  A value computed from unchecked elements is never consulted (verify_core.h): the
// shape and canonical checks of the WHOLE proof come first, so every c_k and z^(k) below is formed from canonical elements, and
// the layers' relations are consulted in ascending order.  Plain C++: no device, no context
// (tests/grand_product_rounds_selfcheck.cpp drives it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "verify_rounds.h"

namespace gkr {
namespace gp {

using verify::F;

inline size_t rounds(int n) { return (size_t)n * (size_t)(n - 1) / 2 - 1; }
inline size_t layer_row(int k) { return (size_t)k * (size_t)(k - 1) / 2 - 1; }   // the first row of layer k; also where z^(k) starts in Pre::z

inline F mul(const F& a, const F& b) { return gkr::h64::mont_mul(gkr::h64::to_mont(a), b); }   // canonical x canonical -> canonical
inline F lerp(const F& a, const F& b, const F& t) { return gkr::h64::add(a, mul(t, gkr::h64::sub(b, a))); }   // a + t (b - a)
inline gkr_fr abi(const F& f) {
    gkr_fr x;
    memcpy(x.l, f.l, 32);
    return x;
}

// hash(v, len) = multi_hash of len canonical values, key 0
template <class Hash>
inline void head_point(const gkr_fr* head, const Hash& hash, F* zeta1, F* zeta2) {
    const F h[4] = {verify::load(head[0]), verify::load(head[1]), verify::load(head[2]), verify::load(head[3])};
    *zeta1 = hash(h, 4);
    *zeta2 = hash(zeta1, 1);
}
inline F head_product(const gkr_fr* head) {
    return mul(mul(verify::load(head[0]), verify::load(head[1])), mul(verify::load(head[2]), verify::load(head[3])));
}
inline F head_claim(const gkr_fr* head, const F& zeta1, const F& zeta2) {
    return lerp(lerp(verify::load(head[0]), verify::load(head[2]), zeta1), lerp(verify::load(head[1]), verify::load(head[3]), zeta1), zeta2);
}
// the step behind layer k: evals = (a_k, b_k), r = r^(k) (k challenges) -> c_{k+1} and z^(k+1) (k + 1 coordinates)
template <class Hash>
inline F next_claim(int k, const gkr_fr* evals, const gkr_fr* r, const Hash& hash, gkr_fr* z_next) {
    const F ab[2] = {verify::load(evals[0]), verify::load(evals[1])};
    const F tau = hash(ab, 2);
    z_next[0] = abi(tau);
    memcpy(z_next + 1, r, (size_t)k * sizeof(gkr_fr));
    return lerp(ab[0], ab[1], tau);
}
inline F eq_point(int k, const gkr_fr* z, const gkr_fr* r) {   // prod_j (z_j r_j + (1 - z_j)(1 - r_j))
    const F one = {{1, 0, 0, 0}};
    F eq = one;
    for (int j = 0; j < k; ++j) {
        const F zj = verify::load(z[j]), rj = verify::load(r[j]), zr = mul(zj, rj);
        eq = mul(eq, gkr::h64::add(gkr::h64::sub(gkr::h64::sub(one, zj), rj), gkr::h64::add(zr, zr)));
    }
    return eq;
}

// one proof in the ABI's arrays: head 4, coeffs R x 4, len R, r R, evals (n - 2) x 2; product: the claimed P or null
struct Proof {
    const gkr_fr *product, *head, *coeffs, *r, *evals;
    const uint32_t* len;
};
struct Verdict {
    uint32_t check = 0, layer = 0, round = 0;
};

// what the host knows about a proof before the round vectors' hashes and V~(z^(n)) are there
struct Pre {
    Verdict form;                     // the first failure among SHAPE, NON_CANONICAL and PRODUCT (check 0: none)
    bool point = false;               // SHAPE and NON_CANONICAL passed: z holds points, z^(n) may go to the device
    std::vector<verify::Pre> layer;   // layer k at k - 2
    std::vector<gkr_fr> z;            // z^(2) .. z^(n), z^(k) at layer_row(k)
    std::vector<F> claim;             // c_2 .. c_n, c_k at k - 2
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
    for (int t = 0; t < 4; ++t)
        if (!verify::canonical(p.head[t])) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    if (p.product && !verify::canonical(*p.product)) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    for (int k = 2; k < n; ++k) {
        for (int j = 0; j < k; ++j) {
            const size_t row = layer_row(k) + j;
            bool ok = verify::canonical(p.r[row]);
            for (uint32_t t = 4 - p.len[row]; t < 4; ++t) ok = ok && verify::canonical(p.coeffs[4 * row + t]);
            if (!ok) return fail(GKR_VERIFY_NON_CANONICAL, k, j);
        }
        if (!verify::canonical(p.evals[2 * (k - 2)]) || !verify::canonical(p.evals[2 * (k - 2) + 1])) return fail(GKR_VERIFY_NON_CANONICAL, k, k);
    }
    out.point = true;
    out.z.resize(rounds(n) + (size_t)n);
    F zeta1, zeta2;
    head_point(p.head, hash, &zeta1, &zeta2);
    out.z[0] = abi(zeta1);
    out.z[1] = abi(zeta2);
    out.claim.push_back(head_claim(p.head, zeta1, zeta2));
    for (int k = 2; k < n; ++k) {
        const size_t row = layer_row(k);
        const gkr_fr c = abi(out.claim.back());
        out.layer.push_back(verify::pre_relations(k, 3, &c, p.coeffs + 4 * row, p.len + row, p.r + row));
        out.claim.push_back(next_claim(k, p.evals + 2 * (k - 2), p.r + row, hash, out.z.data() + layer_row(k + 1)));
    }
    if (p.product && !verify::same(verify::load(*p.product), head_product(p.head))) out.form.check = GKR_VERIFY_PRODUCT;
    return out;
}

// The first failure of a proof: pre's own, else layer by layer the rounds (CHALLENGE / ROUND_SUM at (k, j)) and the layer's last
// relation g_k(r_k) = eq(z^(k), r^(k)) a_k b_k (FINAL_CLAIM at (k, k)), else c_n against v = V~(z^(n)) (EVALUATION at (n, n)).
// slots: the hash slots of the proof's R rows.  false: a well-formed round vector has no hash (an error of the CALL).
inline bool verdict(int n, const Proof& p, const Pre& pre, const verify::HashSlot* slots, const F& v, Verdict* out) {
    *out = pre.form;
    if (out->check) return true;
    for (int k = 2; k < n; ++k) {
        const size_t row = layer_row(k);
        const verify::Pre& lp = pre.layer[k - 2];
        out->layer = (uint32_t)k;
        if (!verify::round_verdict(k, lp, slots + row, p.r + row, &out->check, &out->round)) return false;
        if (out->check) return true;
        const F ab = mul(verify::load(p.evals[2 * (k - 2)]), verify::load(p.evals[2 * (k - 2) + 1]));
        if (!verify::same(lp.last, mul(eq_point(k, pre.z.data() + row, p.r + row), ab))) {
            out->check = GKR_VERIFY_FINAL_CLAIM;
            out->round = (uint32_t)k;
            return true;
        }
    }
    if (!verify::same(pre.claim.back(), v)) {
        out->check = GKR_VERIFY_EVALUATION;
        out->layer = out->round = (uint32_t)n;
        return true;
    }
    *out = Verdict();
    return true;
}

}  // namespace gp
}  // namespace gkr

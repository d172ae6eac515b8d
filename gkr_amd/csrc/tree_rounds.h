// The chain of claims of a GKR TREE ARGUMENT (the grand product, the fractional sum: include/gkr_amd.h) as the driver
// (tree_argument.h) and its verifier use it -- ONE copy of the Fiat-Shamir steps between the layers and of the order of the
// checks, for every gate.  A gate G (grand_product_rounds.h, fraction_sum_rounds.h: each states its argument's mathematics)
// combines W tables of 2^n values level by level, level n the input, level k of W x 2^k values from the halves [0 ..) and
// [2^k ..) of level k + 1:
//   head      the prover publishes level 2, four values of each of the W tables (4 W values); zeta_1 = multi_hash(the 4 W, 0),
//             zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2), variable 1 the most significant index bit; lambda_2 =
//             multi_hash([zeta_2], 0) where the gate draws a lambda; the claims c_2[w] = (table w of level 2)~(z^(2));
//   layer k   = 2 .. n-1: the zero-check at z^(k) of the gate over the halves of level k + 1 with claim G::claim(link_k): k rows of
//             four slots, k challenges r^(k), the 2 W end values (lower, upper half of table w at 2 w, 2 w + 1);
//             tau_k = multi_hash(the 2 W, 0), c_{k+1}[w] = lower + tau_k (upper - lower), z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k),
//             lambda_{k+1} = multi_hash([tau_k], 0) where the gate draws one;
//   end       c_n[w] = (input table w)~(z^(n)).
// The layers' rows lie one after the other, layer k from row k (k - 1) / 2 - 1 on; R = n (n - 1) / 2 - 1 rows in all.
// The round relations are verify_rounds.h's.  A value computed from unchecked elements is never consulted (verify_core.h): the
// shape and canonical checks of the WHOLE proof come first, so every claim and z^(k) below is formed from canonical elements, and
// the layers' relations are consulted in ascending order.  Plain C++: no device, no context
// (tests/grand_product_rounds_selfcheck.cpp and tests/fraction_sum_rounds_selfcheck.cpp drive it alone).
//
// A gate supplies: W; kLambda (whether it draws a lambda per layer: a gate that draws none costs no hash for one); claim(link), the
// zero-check's claim; gate(e, link), the gate on a layer's 2 W end values; root(head, out), the W root values from the head by the
// tree rule; form(claimed, head), the first failed check of the head against the claimed root values (null: none claimed), 0: none.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "verify_rounds.h"

namespace gkr {
namespace tree {

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
inline F eq_point(int k, const gkr_fr* z, const gkr_fr* r) {   // prod_j (z_j r_j + (1 - z_j)(1 - r_j))
    const F one = {{1, 0, 0, 0}};
    F eq = one;
    for (int j = 0; j < k; ++j) {
        const F zj = verify::load(z[j]), rj = verify::load(r[j]), zr = mul(zj, rj);
        eq = mul(eq, gkr::h64::add(gkr::h64::sub(gkr::h64::sub(one, zj), rj), gkr::h64::add(zr, zr)));
    }
    return eq;
}

// one proof in the ABI's arrays: head 4 W, coeffs R x 4, len R, r R, evals (n - 2) x 2 W; claimed: the W claimed root values or null
struct Proof {
    const gkr_fr *claimed, *head, *coeffs, *r, *evals;
    const uint32_t* len;
};
struct Verdict {
    uint32_t check = 0, layer = 0, round = 0;
};

// what layer k starts from besides z^(k): the claims of the W tables of level k at z^(k), and lambda_k (zero where none is drawn)
template <int W>
struct Link {
    F c[W];
    F lambda;
};

// hash(v, len) = multi_hash of len canonical values, key 0
// the head -> z^(2) (two coordinates) and the link of layer 2
template <class G, class Hash>
inline Link<G::W> head_link(const gkr_fr* head, const Hash& hash, gkr_fr* z) {
    F h[4 * G::W];
    for (int t = 0; t < 4 * G::W; ++t) h[t] = verify::load(head[t]);
    const F zeta1 = hash(h, 4 * G::W), zeta2 = hash(&zeta1, 1);
    z[0] = abi(zeta1);
    z[1] = abi(zeta2);
    Link<G::W> out{};
    if constexpr (G::kLambda) out.lambda = hash(&zeta2, 1);
    for (int w = 0; w < G::W; ++w) out.c[w] = lerp(lerp(h[4 * w], h[4 * w + 2], zeta1), lerp(h[4 * w + 1], h[4 * w + 3], zeta1), zeta2);
    return out;
}
// the step behind layer k: evals = its 2 W end values, r = r^(k) (k challenges) -> z^(k+1) (k + 1 coordinates) and the link of
// layer k + 1
template <class G, class Hash>
inline Link<G::W> next_link(int k, const gkr_fr* evals, const gkr_fr* r, const Hash& hash, gkr_fr* z_next) {
    F e[2 * G::W];
    for (int t = 0; t < 2 * G::W; ++t) e[t] = verify::load(evals[t]);
    const F tau = hash(e, 2 * G::W);
    z_next[0] = abi(tau);
    memcpy(z_next + 1, r, (size_t)k * sizeof(gkr_fr));
    Link<G::W> out{};
    for (int w = 0; w < G::W; ++w) out.c[w] = lerp(e[2 * w], e[2 * w + 1], tau);
    if constexpr (G::kLambda) out.lambda = hash(&tau, 1);
    return out;
}

// what the host knows about a proof before the round vectors' hashes and the input tables' values at z^(n) are there
template <class G>
struct Pre {
    Verdict form;                     // the first failure among SHAPE, NON_CANONICAL and the gate's form checks (check 0: none)
    bool point = false;               // SHAPE and NON_CANONICAL passed: z holds points, z^(n) may go to the device
    std::vector<verify::Pre> layer;   // layer k at k - 2
    std::vector<gkr_fr> z;            // z^(2) .. z^(n), z^(k) at layer_row(k)
    std::vector<Link<G::W>> link;     // the links of k = 2 .. n at k - 2
};

template <class G, class Hash>
inline Pre<G> pre_relations(int n, const Proof& p, const Hash& hash) {
    constexpr int W = G::W;
    Pre<G> out;
    auto fail = [&](uint32_t check, int layer, int round) {
        out.form.check = check;
        out.form.layer = (uint32_t)layer;
        out.form.round = (uint32_t)round;
        return out;
    };
    for (int k = 2; k < n; ++k)
        for (int j = 0; j < k; ++j)
            if (const uint32_t len = p.len[layer_row(k) + j]; len < 1 || len > 4) return fail(GKR_VERIFY_SHAPE, k, j);
    for (int t = 0; t < 4 * W; ++t)
        if (!verify::canonical(p.head[t])) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    for (int w = 0; p.claimed && w < W; ++w)
        if (!verify::canonical(p.claimed[w])) return fail(GKR_VERIFY_NON_CANONICAL, 0, 0);
    for (int k = 2; k < n; ++k) {
        for (int j = 0; j < k; ++j) {
            const size_t row = layer_row(k) + j;
            bool ok = verify::canonical(p.r[row]);
            for (uint32_t t = 4 - p.len[row]; t < 4; ++t) ok = ok && verify::canonical(p.coeffs[4 * row + t]);
            if (!ok) return fail(GKR_VERIFY_NON_CANONICAL, k, j);
        }
        for (int t = 0; t < 2 * W; ++t)
            if (!verify::canonical(p.evals[2 * W * (k - 2) + t])) return fail(GKR_VERIFY_NON_CANONICAL, k, k);
    }
    out.point = true;
    out.z.resize(rounds(n) + (size_t)n);
    out.link.push_back(head_link<G>(p.head, hash, out.z.data()));
    for (int k = 2; k < n; ++k) {
        const size_t row = layer_row(k);
        const gkr_fr c = abi(G::claim(out.link.back()));
        out.layer.push_back(verify::pre_relations(k, 3, &c, p.coeffs + 4 * row, p.len + row, p.r + row));
        out.link.push_back(next_link<G>(k, p.evals + 2 * W * (k - 2), p.r + row, hash, out.z.data() + layer_row(k + 1)));
    }
    out.form.check = G::form(p.claimed, p.head);
    return out;
}

// The first failure of a proof: pre's own, else layer by layer the rounds (CHALLENGE / ROUND_SUM at (k, j)) and the layer's last
// relation g_k(r_k) = eq(z^(k), r^(k)) G::gate(the end values, link_k) (FINAL_CLAIM at (k, k)), else c_n[w] against values[w], the
// input table w at z^(n) (EVALUATION at (n, n)).  slots: the hash slots of the proof's R rows.  false: a well-formed round
// vector has no hash (an error of the CALL).
template <class G>
inline bool verdict(int n, const Proof& p, const Pre<G>& pre, const verify::HashSlot* slots, const F* values, Verdict* out) {
    constexpr int W = G::W;
    *out = pre.form;
    if (out->check) return true;
    for (int k = 2; k < n; ++k) {
        const size_t row = layer_row(k);
        const verify::Pre& lp = pre.layer[k - 2];
        out->layer = (uint32_t)k;
        if (!verify::round_verdict(k, lp, slots + row, p.r + row, &out->check, &out->round)) return false;
        if (out->check) return true;
        F e[2 * W];
        for (int t = 0; t < 2 * W; ++t) e[t] = verify::load(p.evals[2 * W * (k - 2) + t]);
        if (!verify::same(lp.last, mul(eq_point(k, pre.z.data() + row, p.r + row), G::gate(e, pre.link[k - 2])))) {
            out->check = GKR_VERIFY_FINAL_CLAIM;
            out->round = (uint32_t)k;
            return true;
        }
    }
    for (int w = 0; w < W; ++w)
        if (!verify::same(pre.link.back().c[w], values[w])) {
            out->check = GKR_VERIFY_EVALUATION;
            out->layer = out->round = (uint32_t)n;
            return true;
        }
    *out = Verdict();
    return true;
}

}  // namespace tree
}  // namespace gkr

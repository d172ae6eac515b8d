// The FRACTIONAL SUM (LogUp) argument (include/gkr_amd.h, gkr_fraction_sum*) as a gate of the tree arguments' one chain of claims
// (tree_rounds.h, which states the Fiat-Shamir steps, the rows' bookkeeping and the order of the checks).  Over tables N, D of
// 2^n values, (p_n, q_n) = (N, D), p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i],
// q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k]:
//   head      the prover publishes level 2, p_2[0..3] then q_2[0..3] (eight values); (P, Q) follow by the tree rule;
//             zeta_1 = multi_hash(the eight, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2),
//             lambda_2 = multi_hash([zeta_2], 0), cp_2 = p_2~(z^(2)), cq_2 = q_2~(z^(2)), variable 1 the most significant index bit;
//   layer k   = 2 .. n-1: the zero-check at z^(k) of T0 T3 + T1 T2 + lambda_k T2 T3 (T0, T1 the halves of p_{k+1}, T2, T3 of q_{k+1})
//             with claim cp_k + lambda_k cq_k: k rows of four slots, k challenges r^(k), the four values (a0, a1, b0, b1);
//             tau_k = multi_hash([a0, a1, b0, b1], 0), cp_{k+1} = a0 + tau_k (a1 - a0), cq_{k+1} = b0 + tau_k (b1 - b0),
//             z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k), lambda_{k+1} = multi_hash([tau_k], 0);
//   end       cp_n = N~(z^(n)), cq_n = D~(z^(n)).
// In a link, c[0] = cp_k and c[1] = cq_k.  The form checks: ZERO_DENOMINATOR, the head's Q, then FRACTION_SUM, the claimed (P, Q)
// (if any) against the head's.  Plain C++: no device, no context (tests/fraction_sum_rounds_selfcheck.cpp drives it alone).
#pragma once
#include "tree_rounds.h"

namespace gkr {
namespace fs {

struct Gate {
    static constexpr int W = 2;
    static constexpr bool kLambda = true;
    using Link = tree::Link<W>;
    using F = tree::F;
    static F claim(const Link& l) { return gkr::h64::add(l.c[0], tree::mul(l.lambda, l.c[1])); }
    static F gate(const F* e, const Link& l) {   // e = (a0, a1, b0, b1): a0 b1 + a1 b0 + lambda_k b0 b1
        return gkr::h64::add(gkr::h64::add(tree::mul(e[0], e[3]), tree::mul(e[1], e[2])), tree::mul(l.lambda, tree::mul(e[2], e[3])));
    }
    // (P, Q) of the head by the tree rule: level 2 -> level 1 -> level 0
    static void root(const gkr_fr* head, F* out) {
        F p[4], q[4], p1[2], q1[2];
        for (int t = 0; t < 4; ++t) {
            p[t] = verify::load(head[t]);
            q[t] = verify::load(head[4 + t]);
        }
        for (int i = 0; i < 2; ++i) {
            p1[i] = gkr::h64::add(tree::mul(p[i], q[i + 2]), tree::mul(p[i + 2], q[i]));
            q1[i] = tree::mul(q[i], q[i + 2]);
        }
        out[0] = gkr::h64::add(tree::mul(p1[0], q1[1]), tree::mul(p1[1], q1[0]));
        out[1] = tree::mul(q1[0], q1[1]);
    }
    static uint32_t form(const gkr_fr* claimed, const gkr_fr* head) {
        F PQ[2];
        root(head, PQ);
        if (gkr::h64::is_zero(PQ[1])) return GKR_VERIFY_ZERO_DENOMINATOR;
        return claimed && !(verify::same(verify::load(claimed[0]), PQ[0]) && verify::same(verify::load(claimed[1]), PQ[1])) ? GKR_VERIFY_FRACTION_SUM : 0;
    }
};

}  // namespace fs
}  // namespace gkr

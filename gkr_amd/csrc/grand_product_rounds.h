// The GRAND PRODUCT argument (include/gkr_amd.h, gkr_grand_product*) as a gate of the tree arguments' one chain of claims
// (tree_rounds.h, which states the Fiat-Shamir steps, the rows' bookkeeping and the order of the checks).  Over a table V of
// 2^n values, L_n = V, L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k]:
//   head      the prover publishes L_2 (four values); P = their product; zeta_1 = multi_hash(L_2, 0), zeta_2 = multi_hash([zeta_1], 0),
//             z^(2) = (zeta_1, zeta_2), c_2 = L_2~(z^(2)), variable 1 the most significant index bit;
//   layer k   = 2 .. n-1: the zero-check of eq(z^(k), .) L_{k+1}[0 ..) L_{k+1}[2^k ..) with claim c_k: k rows of four slots, k
//             challenges r^(k), the two values (a_k, b_k); tau_k = multi_hash([a_k, b_k], 0), c_{k+1} = a_k + tau_k (b_k - a_k),
//             z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k);
//   end       c_n = V~(z^(n)).
// No lambda is drawn.  The form check: PRODUCT, the claimed P (if any) against the head's.  Plain C++: no device, no context
// (tests/grand_product_rounds_selfcheck.cpp drives it alone).
#pragma once
#include "tree_rounds.h"

namespace gkr {
namespace gp {

struct Gate {
    static constexpr int W = 1;
    static constexpr bool kLambda = false;
    using Link = tree::Link<W>;
    using F = tree::F;
    static F claim(const Link& l) { return l.c[0]; }
    static F gate(const F* e, const Link&) { return tree::mul(e[0], e[1]); }   // e = (a_k, b_k)
    static void root(const gkr_fr* head, F* out) {
        *out = tree::mul(tree::mul(verify::load(head[0]), verify::load(head[1])), tree::mul(verify::load(head[2]), verify::load(head[3])));
    }
    static uint32_t form(const gkr_fr* claimed, const gkr_fr* head) {
        F P;
        root(head, &P);
        return claimed && !verify::same(verify::load(*claimed), P) ? GKR_VERIFY_PRODUCT : 0;
    }
};

}  // namespace gp
}  // namespace gkr

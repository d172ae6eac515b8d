// The round relations of ONE sumcheck transcript (python/sumcheck.py:55-70) as the device verifiers of the sumchecks use them --
// ONE copy, shared by capi_mle_verify.hip (the plain, product and sum-of-products verifiers: the last relation is a combination of
// the tables' values) and capi_r1cs_verify.hip (the R1CS verifier: two transcripts, the last relations are values the caller
// supplies).  Rows of `degree` + 1 right-aligned slots, highest degree first.  In the order of the checks:
//   pre_relations   what needs neither a hash nor a device value: shape, canonical checks, the round sums, the Horner steps;
//   hash_slot       the rule of a round vector's hash slot (k_verify_hash's, restated for rows of `width` slots);
//   round_verdict   the first failure among SHAPE, NON_CANONICAL and, round by round, ROUND_SUM and CHALLENGE;
// the caller compares Pre::last with its last relation when round_verdict found nothing.  A value computed from unchecked elements
// is never consulted (verify_core.h).  Plain C++: no device, no context (tests/verify_rounds_selfcheck.cpp drives it alone).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "verify_core.h"

namespace gkr {
namespace verify {

struct HashSlot {
    gkr_fr h;
    uint32_t valid;
};
constexpr int kMaxRowWidth = GKR_PRODUCT_MAX_DEGREE + 1;

// what the host knows about a transcript before the hashes and the device's values are there
struct Pre {
    uint32_t check = 0, round = 0;   // the first failure among checks 1 and 2 (check 0: none)
    uint32_t sum_round = 0;          // the first round whose sum check fails (n: none)
    F last = {{0, 0, 0, 0}};         // g_n(r_n)
    F proved = {{0, 0, 0, 0}};       // g_1(0) + g_1(1)
};

inline Pre pre_relations(int n, int degree, const gkr_fr* claim, const gkr_fr* coeffs, const uint32_t* len, const gkr_fr* r) {
    const uint32_t W = (uint32_t)degree + 1;
    Pre p;
    p.sum_round = (uint32_t)n;
    for (int j = 0; j < n; ++j)
        if (len[j] < 1 || len[j] > W) {
            p.check = GKR_VERIFY_SHAPE;
            p.round = (uint32_t)j;
            return p;
        }
    if (claim && !canonical(*claim)) {
        p.check = GKR_VERIFY_NON_CANONICAL;
        return p;
    }
    for (int j = 0; j < n; ++j) {
        bool ok = canonical(r[j]);
        for (uint32_t t = W - len[j]; t < W; ++t) ok = ok && canonical(coeffs[W * j + t]);
        if (!ok) {
            p.check = GKR_VERIFY_NON_CANONICAL;
            p.round = (uint32_t)j;
            return p;
        }
    }
    F running = claim ? load(*claim) : F{{0, 0, 0, 0}};
    for (int j = 0; j < n; ++j) {
        const gkr_fr* g = coeffs + W * j + (W - len[j]);
        F sum = load(g[len[j] - 1]);                                  // g(0) + g(1) = 2 c_0 + c_1 + .. over the used slots
        for (uint32_t t = 0; t < len[j]; ++t) sum = gkr::h64::add(sum, load(g[t]));
        if (j == 0) p.proved = sum;
        if ((j > 0 || claim) && !same(sum, running)) {
            p.sum_round = (uint32_t)j;
            return p;   // (challenges of earlier rounds are still compared: round_verdict)
        }
        running = horner(g, (int)len[j], gkr::h64::to_mont(load(r[j])));
    }
    p.last = running;
    return p;
}

// the host's rule for a slot -- the kernel's, restated for rows of `width` slots; hash(v, len) = multi_hash of len canonical values
template <class Hash>
inline void hash_slot(const gkr_fr* row, uint32_t width, uint32_t len, HashSlot* slot, const Hash& hash) {
    slot->valid = 0;
    if (len < 1 || len > width || width > (uint32_t)kMaxRowWidth) return;
    F v[kMaxRowWidth];
    for (uint32_t t = 0; t < len; ++t) {
        if (!canonical(row[width - len + t])) return;
        v[t] = load(row[width - len + t]);
    }
    const F h = hash(v, (int)len);
    memcpy(slot->h.l, h.l, 32);
    slot->valid = 1;
}

// The first failure of a transcript's rounds from what pre_relations found and its hash slots: p's own check, else round by round
// the challenge comparisons up to the first failed sum, then that sum.  *check = 0: the rounds hold and p.last is to be compared
// with the last relation.  false: a well-formed round vector has no hash (an error of the CALL, not a verdict).
inline bool round_verdict(int n, const Pre& p, const HashSlot* slots, const gkr_fr* r, uint32_t* check, uint32_t* round) {
    *check = p.check;
    *round = p.round;
    if (*check) return true;
    for (uint32_t j = 0; j < (uint32_t)n && j < p.sum_round; ++j) {
        if (!slots[j].valid) return false;
        if (memcmp(slots[j].h.l, r[j].l, 32) != 0) {
            *check = GKR_VERIFY_CHALLENGE;
            *round = j;
            return true;
        }
    }
    if (p.sum_round < (uint32_t)n) {
        *check = GKR_VERIFY_ROUND_SUM;
        *round = p.sum_round;
    }
    return true;
}

}  // namespace verify
}  // namespace gkr

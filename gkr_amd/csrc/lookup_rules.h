// The two rules of the LOOKUP argument (include/gkr_amd.h, gkr_lookup*) that are plain logic: the slot function h of the table
// index, which the kernels of kernels_lookup.hip and gkr_selftest_lookup_slot both call, and the verdict rule that puts
// GKR_VERIFY_LOOKUP in its place among the fractional sum's checks.  Plain C++: no device, no context
// (tests/lookup_rules_selfcheck.cpp drives it alone).
//
//   h(v, s)   v = (v0, v1, v2, v3), the four 64-bit limbs of the canonical value, least significant first; arithmetic modulo 2^64:
//                 x = 0x9E3779B97F4A7C15
//                 for i = 0 .. 3:   x = (x ^ v_i) * 0xFF51AFD7ED558CCD;   x = x ^ (x >> 32)
//                 x = x * 0xC4CEB9FE1A85EC53;   x = x ^ (x >> 29)
//                 slot = x >> (64 - s)                                   (the s most significant bits, 1 <= s <= 32)
//             Every step is a bijection of x, so two values that differ in any one limb leave different x; the multiplications
//             carry a small integer's low bits, and a high limb's, into the bits the slot is taken from.
//   verdict   the fractional sum's verdict on the rebuilt pair stands where it is SHAPE, NON_CANONICAL or ZERO_DENOMINATOR;
//             otherwise a head whose P is not 0 is GKR_VERIFY_LOOKUP at (0, 0) -- before every layer's relation and the evaluation.
#pragma once
#include <stdint.h>

#include "../../include/gkr_amd.h"

#if defined(__HIPCC__)
#define GKR_LOOKUP_HD __host__ __device__ inline
#else
#define GKR_LOOKUP_HD inline
#endif

namespace gkr {
namespace lookup {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// limbs: the eight 32-bit words of the value, least significant first
GKR_LOOKUP_HD uint32_t slot_of(const uint32_t* limbs, uint32_t log_slots) {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 4; ++i) {
        const uint64_t v = (uint64_t)limbs[2 * i] | ((uint64_t)limbs[2 * i + 1] << 32);
        x = (x ^ v) * 0xFF51AFD7ED558CCDull;
        x ^= x >> 32;
    }
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 29;
    return (uint32_t)(x >> (64u - log_slots));
}

// L = max(n_w, n_t) + 1, or 0 for a shape the lookup calls refuse (plain logic: decided before the context is looked at)
inline int pair_log2(int n_w, int n_t, int batch) {
    if (n_w < 2 || n_t < 2 || n_w > GKR_MAX_MLE_N || n_t > GKR_MAX_MLE_N || batch < 1 || batch > 65535) return 0;
    const int L = (n_w > n_t ? n_w : n_t) + 1;
    if (L > GKR_MAX_MLE_N || (((unsigned long long)batch) << (L + 1)) > (1ull << 30)) return 0;
    return L;
}

// the inner verdict of proof b and the head's root (P, Q) the inner verifier returned for it -> the lookup's verdict, in place
inline void verdict(const gkr_fr* root, int* accept, uint32_t* layer, uint32_t* round, uint32_t* check) {
    if (*check == GKR_VERIFY_SHAPE || *check == GKR_VERIFY_NON_CANONICAL || *check == GKR_VERIFY_ZERO_DENOMINATOR) return;
    uint64_t any = 0;
    for (int i = 0; i < 4; ++i) any |= root[0].l[i];
    if (!any) return;
    *accept = 0;
    *check = GKR_VERIFY_LOOKUP;
    *layer = *round = 0;
}

}  // namespace lookup
}  // namespace gkr

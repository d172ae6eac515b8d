// Stand-alone check of the sumcheck verifiers' round relations (gkr_amd/csrc/verify_rounds.h: pre_relations, hash_slot,
// round_verdict) without a device or a context, meant to be built under -fsanitize=address,undefined
// (tests/test_r1cs_verify_host.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/verify_rounds_selfcheck.cpp gkr_amd/csrc/keccak.cpp
// Transcripts of 1 .. 6 rounds with rows of 2, 3 and 4 slots are made here -- arbitrary coefficients, the constant term solved from
// the running claim, the challenge the MiMC7 hash of the used slots -- with every length 1 .. width in turn and the UNUSED leading
// slots filled with r (not canonical: they must never be read).  Every array is allocated at its exact size.  The honest
// transcript passes; one change at a time gives the verdict the rules state for its position.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../gkr_amd/csrc/keccak.h"
#include "../gkr_amd/csrc/mimc7.h"
#include "../gkr_amd/csrc/verify_rounds.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;

F g_cts[gkr::kMimcRounds];

F hash(const F* v, int n) { return gkr::h64::mimc7_multi_hash(v, n, g_cts, nullptr); }
F mul(const F& a, const F& b) { return gkr::h64::mont_mul(gkr::h64::to_mont(a), b); }
gkr_fr abi(const F& f) {
    gkr_fr x;
    memcpy(x.l, f.l, 32);
    return x;
}
gkr_fr modulus() {
    gkr_fr x;
    memcpy(x.l, gkr::h64::kMod, 32);
    return x;
}
gkr_fr plus_one(const gkr_fr& x) { return abi(gkr::h64::add(V::load(x), F{{1, 0, 0, 0}})); }

int fail(const char* what, int a, int b, int c) {
    printf("verify_rounds_selfcheck: FAILED: %s (width %d, rounds %d, position %d)\n", what, a, b, c);
    return 1;
}

struct Transcript {
    int n = 0, W = 0;
    gkr_fr claim{};
    std::vector<gkr_fr> coeffs, r;
    std::vector<uint32_t> len;
};

// g_j has len_j = 1 + (j + shift) % W coefficients; c_0 = (claim - the others) / 2
Transcript make(int n, int W, int shift, uint64_t seed) {
    Transcript t;
    t.n = n;
    t.W = W;
    t.coeffs.assign((size_t)n * W, modulus());
    t.r.resize(n);
    t.len.resize(n);
    F inv2;   // (r + 1) / 2
    memcpy(inv2.l, gkr::h64::kMod, 32);
    for (int i = 0; i < 4; ++i) inv2.l[i] = (inv2.l[i] >> 1) | (i < 3 ? gkr::h64::kMod[i + 1] << 63 : 0);
    inv2 = gkr::h64::add(inv2, F{{1, 0, 0, 0}});
    F x = {{seed, seed * 3 + 1, seed * 7 + 5, 0x1234}};
    F running = mul(x, x);
    t.claim = abi(running);
    for (int j = 0; j < n; ++j) {
        const uint32_t len = 1u + (uint32_t)((j + shift) % W);
        t.len[j] = len;
        gkr_fr* g = t.coeffs.data() + (size_t)W * j + (W - len);
        F rest = {{0, 0, 0, 0}};
        for (uint32_t k = 0; k + 1 < len; ++k) {
            x = gkr::h64::add(mul(x, x), F{{(uint64_t)j + 2, k, 0, 0}});
            g[k] = abi(x);
            rest = gkr::h64::add(rest, x);
        }
        g[len - 1] = abi(mul(gkr::h64::sub(running, rest), inv2));
        F used[V::kMaxRowWidth];
        for (uint32_t k = 0; k < len; ++k) used[k] = V::load(g[k]);
        const F rj = hash(used, (int)len);
        t.r[j] = abi(rj);
        running = V::horner(g, (int)len, gkr::h64::to_mont(rj));
    }
    return t;
}

// (check, round) of a transcript, or (-1, 0) where round_verdict reports a missing hash
void verdict(const Transcript& t, bool with_claim, int* check, int* round, F* last) {
    const V::Pre p = V::pre_relations(t.n, t.W - 1, with_claim ? &t.claim : nullptr, t.coeffs.data(), t.len.data(), t.r.data());
    std::vector<V::HashSlot> slots(t.n);
    for (int j = 0; j < t.n; ++j) V::hash_slot(t.coeffs.data() + (size_t)t.W * j, (uint32_t)t.W, t.len[j], &slots[j], hash);
    uint32_t c = 0, r = 0;
    if (!V::round_verdict(t.n, p, slots.data(), t.r.data(), &c, &r)) {
        *check = -1;
        *round = 0;
        return;
    }
    *check = (int)c;
    *round = (int)r;
    if (last) *last = p.last;
}

}  // namespace

int main() {
    {
        gkr::Fr cts[gkr::kMimcRounds];
        gkr::mimc7_make_constants(cts);
        static_assert(sizeof(cts) == sizeof(g_cts), "the same 91 constants in both limb widths");
        memcpy(g_cts, cts, sizeof cts);
    }
    int cases = 0;
    for (int W = 2; W <= 4; ++W)
        for (int n = 1; n <= 6; ++n)
            for (int shift = 0; shift < W; ++shift) {
                const Transcript t = make(n, W, shift, (uint64_t)(100 * W + 10 * n + shift));
                int check, round;
                F last;
                verdict(t, true, &check, &round, &last);
                if (check != 0) return fail("the honest transcript is rejected", W, n, check);
                {   // g_n(r_n) as the Horner step of the last row gives it
                    const uint32_t len = t.len[n - 1];
                    const F want = V::horner(t.coeffs.data() + (size_t)W * (n - 1) + (W - len), (int)len, gkr::h64::to_mont(V::load(t.r[n - 1])));
                    if (!V::same(last, want)) return fail("the last claim", W, n, 0);
                }
                for (int j = 0; j < n; ++j) {
                    const uint32_t len = t.len[j];
                    for (uint32_t k = 0; k < len; ++k) {   // a used slot: the round's sum
                        Transcript u = t;
                        gkr_fr& slot = u.coeffs[(size_t)W * j + (W - len) + k];
                        slot = plus_one(slot);
                        verdict(u, true, &check, &round, nullptr);
                        if (check != GKR_VERIFY_ROUND_SUM || round != j) return fail("a changed slot", W, n, j);
                        if (j == 0) {   // without a claim round 0's sum is not checked: the hash is
                            verdict(u, false, &check, &round, nullptr);
                            if (check != GKR_VERIFY_CHALLENGE || round != 0) return fail("a changed slot of round 0, no claim", W, n, j);
                        }
                        slot = modulus();
                        verdict(u, true, &check, &round, nullptr);
                        if (check != GKR_VERIFY_NON_CANONICAL || round != j) return fail("a slot >= r", W, n, j);
                    }
                    Transcript u = t;
                    u.r[j] = plus_one(u.r[j]);
                    verdict(u, true, &check, &round, nullptr);
                    if (check != GKR_VERIFY_CHALLENGE || round != j) return fail("a changed challenge", W, n, j);
                    u.r[j] = modulus();
                    verdict(u, true, &check, &round, nullptr);
                    if (check != GKR_VERIFY_NON_CANONICAL || round != j) return fail("a challenge >= r", W, n, j);
                    for (const uint32_t bad : {0u, (uint32_t)W + 1u, 0xFFFFFFFFu}) {
                        u = t;
                        u.len[j] = bad;
                        verdict(u, true, &check, &round, nullptr);
                        if (check != GKR_VERIFY_SHAPE || round != j) return fail("a length outside 1 .. width", W, n, j);
                    }
                }
                Transcript u = t;
                u.claim = plus_one(u.claim);
                verdict(u, true, &check, &round, nullptr);
                if (check != GKR_VERIFY_ROUND_SUM || round != 0) return fail("a changed claim", W, n, 0);
                u.claim = modulus();
                verdict(u, true, &check, &round, nullptr);
                if (check != GKR_VERIFY_NON_CANONICAL || round != 0) return fail("a claim >= r", W, n, 0);
                {   // a well-formed round vector without a hash is an error of the call
                    const V::Pre p = V::pre_relations(n, W - 1, &t.claim, t.coeffs.data(), t.len.data(), t.r.data());
                    std::vector<V::HashSlot> none(n);
                    for (auto& s : none) s.valid = 0;
                    uint32_t c = 0, r = 0;
                    if (V::round_verdict(n, p, none.data(), t.r.data(), &c, &r)) return fail("a missing hash goes unnoticed", W, n, 0);
                }
                ++cases;
            }
    printf("verify_rounds_selfcheck: ok (%d transcripts)\n", cases);
    return 0;
}

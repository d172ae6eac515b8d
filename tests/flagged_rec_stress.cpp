// Stand-alone stress of the flag-in-word records' host side (gkr_amd/csrc/flagged_rec.h), built by tests/test_mle_flagged_records.py
// under -fsanitize=address,undefined and under -fsanitize=thread.  A writer thread plays the device: it fills the records of a few
// tables word by word, in shuffled order, with pauses; the reader polls as the driver does (flagged_scan with a cursor per table, then
// flagged_total) and must never total a table early and must end with the sums of a plain big-integer addition.  The same arrays
// are used round after round, so every round starts on the stale words of the one before; the ticket counter starts just below
// 2^32 and wraps during the run.  Prints "OK" and returns 0, or says what went wrong and returns 1.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <thread>
#include <vector>

#include "flagged_rec.h"

using namespace gkr;

namespace {
constexpr uint32_t kTables = 3, kSub = 32, kWords = kFlagRecsPerTable * kFlagRecWords;

int fail(const char* what, uint32_t a = 0, uint32_t b = 0) {
    printf("FAILED: %s (%u, %u)\n", what, a, b);
    return 1;
}

// ---- the reference: 320-bit integers on five 64-bit limbs, schoolbook
struct Big {
    uint64_t l[5] = {0, 0, 0, 0, 0};
};
void big_add(Big& a, const Big& b) {
    unsigned __int128 c = 0;
    for (int i = 0; i < 5; ++i) {
        c += (unsigned __int128)a.l[i] + b.l[i];
        a.l[i] = (uint64_t)c;
        c >>= 64;
    }
}
bool big_geq(const Big& a, const Big& b) {
    for (int i = 4; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
    return true;
}
void big_sub(Big& a, const Big& b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 5; ++i) {
        const unsigned __int128 d = (unsigned __int128)a.l[i] - b.l[i] - borrow;
        a.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
}
Big big_shl(const Big& a, int k) {   // k < 64
    Big r;
    for (int i = 4; i >= 0; --i) r.l[i] = (a.l[i] << k) | (k && i ? a.l[i - 1] >> (64 - k) : 0);
    return r;
}
// a mod r by shift and subtract: a < 2^292 (eight records of 288 bits) and r > 2^253, so the quotient is below 2^40
Big big_mod_r(Big a) {
    Big r;
    for (int i = 0; i < 4; ++i) r.l[i] = h64::kMod[i];
    for (int k = 40; k >= 0; --k) {
        const Big m = big_shl(r, k);
        if (big_geq(a, m)) big_sub(a, m);
    }
    return a;
}

struct Round {
    std::vector<uint32_t> data;   // [table][record][word]: what the device would publish
    std::vector<Big> want;        // [table][sub-block], reduced
    std::vector<uint32_t> dep;    // [table]
};
Round make_round(std::mt19937_64& rng, int kind) {
    Round R;
    R.data.resize((size_t)kTables * kWords);
    R.want.resize((size_t)kTables * kSub);
    R.dep.assign(kTables, 0);
    for (uint32_t t = 0; t < kTables; ++t)
        for (uint32_t rec = 0; rec < kFlagRecsPerTable; ++rec) {
            uint32_t* w = &R.data[((size_t)t * kFlagRecsPerTable + rec) * kFlagRecWords];
            // kind 0: random limbs; 1: every limb all ones (the carries); 2: all zero (valid records that carry zero data)
            for (uint32_t l = 0; l < 9; ++l) w[l] = kind == 0 ? (uint32_t)rng() : (kind == 1 ? 0xFFFFFFFFu : 0u);
            w[9] = kind == 0 && rec == 17 * t + 3 ? 1u : 0u;   // dep from exactly one record of a table
            R.dep[t] |= w[9];
            Big v;
            for (uint32_t l = 0; l < 9; ++l) v.l[l / 2] |= (uint64_t)w[l] << (32 * (l & 1));
            big_add(R.want[(size_t)t * kSub + rec / (kFlagRecsPerTable / kSub)], v);
        }
    for (Big& b : R.want) b = big_mod_r(b);
    return R;
}
bool sums_match(const uint64_t* sums, const Big* want) {
    for (uint32_t s = 0; s < kSub; ++s) {
        if (want[s].l[4]) return false;
        for (int i = 0; i < 4; ++i)
            if (sums[4 * s + i] != want[s].l[i]) return false;
    }
    return true;
}
}  // namespace

int main() {
    std::mt19937_64 rng(20261020);
    // ---- the ticket counter: 0 is never issued, also where it wraps
    {
        uint32_t c = 0xFFFFFFFEu;
        if (next_ticket(c) != 0xFFFFFFFFu || next_ticket(c) != 1u || next_ticket(c) != 2u) return fail("next_ticket at the wrap");
        uint32_t z = 0;
        if (next_ticket(z) != 1u) return fail("next_ticket from a fresh counter");
    }
    std::vector<uint64_t> words((size_t)kTables * kWords, 0);
    uint64_t sums[4 * kSub];
    uint32_t dep = 0;
    // ---- zeroed records are valid for no ticket that is ever issued
    {
        uint32_t cursor = 0;
        if (flagged_scan(words.data(), kWords, 1u, &cursor) || cursor != 0 || flagged_total(words.data(), kFlagRecsPerTable, kSub, 1u, sums, &dep))
            return fail("zeroed records validated");
    }
    // ---- a record left with ONE old word never validates
    {
        const Round R = make_round(rng, 0);
        for (uint32_t i = 0; i < kWords; ++i) words[i] = flag_word(R.data[i], 7u);
        const uint32_t old = 10u * 200u + 4u;
        words[old] = flag_word(R.data[old], 6u);
        uint32_t cursor = 0;
        for (int again = 0; again < 3; ++again)
            if (flagged_scan(words.data(), kWords, 7u, &cursor) || cursor != old) return fail("scan passed an old word", cursor, old);
        if (flagged_total(words.data(), kFlagRecsPerTable, kSub, 7u, sums, &dep)) return fail("total took an old word");
        words[old] = flag_word(R.data[old], 7u);
        if (!flagged_scan(words.data(), kWords, 7u, &cursor) || !flagged_total(words.data(), kFlagRecsPerTable, kSub, 7u, sums, &dep) ||
            !sums_match(sums, R.want.data()))
            return fail("complete records did not total");
    }
    // ---- writer against reader, round after round on the same words, tickets across the 32-bit wrap
    uint32_t counter = 0xFFFFFFFCu;
    for (int round = 0; round < 7; ++round) {
        const uint32_t ticket = next_ticket(counter);
        if (ticket == 0) return fail("ticket 0 issued");
        const Round R = make_round(rng, round % 3);
        std::vector<uint32_t> order((size_t)kTables * kWords);
        for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
        std::shuffle(order.begin(), order.end(), rng);
        std::thread writer([&] {
            for (size_t k = 0; k < order.size(); ++k) {
                __atomic_store_n(&words[order[k]], flag_word(R.data[order[k]], ticket), __ATOMIC_RELAXED);
                if (k % 97 == 0) std::this_thread::yield();
            }
        });
        uint32_t cursor[kTables] = {0, 0, 0};
        bool done[kTables] = {false, false, false};
        uint32_t left = kTables, polls = 0;
        int bad = 0;
        while (left && !bad) {
            for (uint32_t t = 0; t < kTables && !bad; ++t) {
                if (done[t]) continue;
                const uint64_t* w = &words[(size_t)t * kWords];
                // (a total at any time: it may only succeed on complete records, and then with the right sums)
                if ((++polls & 63u) == 0 && flagged_total(w, kFlagRecsPerTable, kSub, ticket, sums, &dep) &&
                    (!sums_match(sums, &R.want[(size_t)t * kSub]) || dep != R.dep[t]))
                    bad = 1;
                if (!flagged_scan(w, kWords, ticket, &cursor[t])) continue;
                if (!flagged_total(w, kFlagRecsPerTable, kSub, ticket, sums, &dep))
                    bad = 2;
                else if (!sums_match(sums, &R.want[(size_t)t * kSub]) || dep != R.dep[t])
                    bad = 3;
                done[t] = true;
                --left;
            }
        }
        writer.join();
        if (bad) return fail(bad == 1 ? "a table was totalled early" : (bad == 2 ? "scanned records did not total" : "wrong sums"), (uint32_t)round, ticket);
    }
    if (counter != 4u) return fail("the counter did not wrap as expected", counter);
    printf("OK\n");
    return 0;
}

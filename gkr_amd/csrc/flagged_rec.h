// Flag-in-word records: how a streaming pass of the plain sumcheck hands its partial sums to the host without a reduce launch,
// a fence or an arrival counter (the protocol of RCCL's LL transport).  No HIP in this file: the host side is tested alone.
//
// A published 64-bit word is { low 32 bits: a data limb, high 32 bits: the pass's ticket }.
//   * the device stores it with ONE relaxed, system-scope atomic store of 8 bytes to pinned host memory (kernels.hip mle_flag_store);
//   * the host reads it with a relaxed 8-byte load;
//   * a word is valid if and only if its high half is the ticket the host expects.
// Data and flag travel in one single-copy-atomic store, so nothing orders one store against another and a word is never seen
// half written.  ASSUMED, not verified here: an aligned 8-byte store of the device to pinned host memory is single-copy atomic
// (one PCIe write that is not split) -- what RCCL's LL protocol relies on on this hardware.
// Tickets are never 0 (next_ticket), so the zeroed words of a fresh allocation are valid for no pass; a word left by an earlier
// pass carries that pass's ticket.  A 32-bit ticket comes round again after 2^32 passes of a context: a word would have to
// survive that long unwritten to be taken for a new one.
//
// A record is the partial of one block: the nine limbs of an Acc<9> (fr32.h: a 288-bit sum of canonical elements) and the
// block's "depends on x_n" bit.  A table has `nrec` records, sub-block s of `nsub` being records [s nrec / nsub, (s + 1) nrec / nsub).
#pragma once
#include <stdint.h>

#include "fr64.h"

namespace gkr {

constexpr uint32_t kFlagRecWords = 10;       // nine limbs and the dep bit
constexpr uint32_t kFlagRecsPerTable = 256;  // what both publishing kernels leave per table: 8 records per sub-block of 32

inline uint64_t flag_word(uint32_t data, uint32_t ticket) { return ((uint64_t)ticket << 32) | data; }

// the next ticket of a context's counter: never 0
inline uint32_t next_ticket(uint32_t& counter) {
    if (++counter == 0u) ++counter;
    return counter;
}

// Moves *cursor over the words that carry `ticket`, from where the last call stopped; true: all `nwords` do.  A table is scanned
// once, not once per poll: a word that was valid stays so until the table's next pass, which the host itself starts.
inline bool flagged_scan(const uint64_t* words, uint32_t nwords, uint32_t ticket, uint32_t* cursor) {
    uint32_t c = *cursor;
    while (c < nwords && (uint32_t)(__atomic_load_n(words + c, __ATOMIC_RELAXED) >> 32) == ticket) ++c;
    *cursor = c;
    return c == nwords;
}

// lo + hi 2^256 mod r, canonical (lo < 2^256 < 6 r: at most five subtractions; hi 2^256 = hi R is hi in Montgomery form)
inline h64::F flagged_reduce(h64::F lo, uint64_t hi) {
    while (h64::geq_mod(lo)) h64::sub_mod(lo);
    return h64::add(lo, h64::to_mont(h64::F{{hi, 0, 0, 0}}));
}

// The records of one table -> its `nsub` canonical sub-block sums (4 x 64-bit words each) and the OR of the dep bits: the value
// k_mle_sub_reduce writes for the same partials.  false (nothing usable written): some word does not carry `ticket`.
// nrec / nsub <= 2^28 records per sub-block.
inline bool flagged_total(const uint64_t* words, uint32_t nrec, uint32_t nsub, uint32_t ticket, uint64_t* sums, uint32_t* dep) {
    const uint32_t per = nrec / nsub;
    uint32_t d = 0;
    for (uint32_t s = 0; s < nsub; ++s) {
        uint64_t limb[kFlagRecWords - 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (uint32_t k = 0; k < per; ++k) {
            const uint64_t* rec = words + (size_t)(s * per + k) * kFlagRecWords;
            for (uint32_t l = 0; l < kFlagRecWords; ++l) {
                const uint64_t w = __atomic_load_n(rec + l, __ATOMIC_RELAXED);
                if ((uint32_t)(w >> 32) != ticket) return false;
                if (l + 1 < kFlagRecWords)
                    limb[l] += (uint32_t)w;
                else
                    d |= (uint32_t)w;
            }
        }
        uint32_t v[kFlagRecWords];
        uint64_t carry = 0;
        for (uint32_t l = 0; l + 1 < kFlagRecWords; ++l) {
            const uint64_t t = limb[l] + carry;   // (< 2^60 + 2^28)
            v[l] = (uint32_t)t;
            carry = t >> 32;
        }
        v[kFlagRecWords - 1] = (uint32_t)carry;
        h64::F lo;
        for (int i = 0; i < 4; ++i) lo.l[i] = (uint64_t)v[2 * i] | ((uint64_t)v[2 * i + 1] << 32);
        const h64::F r = flagged_reduce(lo, (uint64_t)v[8] | ((uint64_t)v[9] << 32));
        for (int i = 0; i < 4; ++i) sums[4 * s + i] = r.l[i];
    }
    *dep = d ? 1u : 0u;
    return true;
}

}  // namespace gkr

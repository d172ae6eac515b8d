// CDNA4 (gfx950) kernels of the LOOKUP argument (gkr_lookup*): from a resident witness column W (2^n_w canonical values) and a
// resident table T (2^n_t canonical values) the multiplicities M -- M[j] = how often T[j] occurs in W, the LOWEST index of a
// repeated table value taking the whole count -- and the pair (N, D) of the fractional sum that proves the lookup,
//   witness side  (N, D)[i] = (1, alpha - W[i]),                   table side  (N, D)[2^(L-1) + j] = (-M[j], alpha - T[j]),
// (0, 1) on the padding of either side, L = max(n_w, n_t) + 1.  Counting is a join of 256-bit keys: an open-addressing index of the
// table (linear probing, 2^(n_t+1) slots of one 32-bit word, so the load factor is at most 1/2; lookup_rules.h states the slot
// function h), built by one launch and read by the next.  Nothing here relies on an order inside a launch.
//
// k_lk_build   a thread per table entry j: from slot h(T[j]) on, atomicCAS(slot, EMPTY, j); a slot that holds an index of an EQUAL
//              entry (all eight limbs) takes atomicMin(slot, j); any other slot is passed, wrapping at the end.  A claimed slot's
//              KEY never changes (only its index, among equal entries), so value -> lowest index is the same for every order of
//              arrival, and every probe chain of a value ends at the value's slot or at an empty one.
// k_lk_count   a launch of its own: T and the index are read-only.  A thread per witness entry probes until the keys are equal,
//              then adds one to the 32-bit counter of that index (counts are at most 2^30); at an empty slot the entry is a miss:
//              the column's miss counter and atomicMin on its first-miss index.  Lanes of a wave that found the index of the
//              wave's first hit add their number in ONE atomic (kLkWaveCombine): a column that repeats one value would send 64
//              atomics to one word otherwise; lanes with another index add on their own.  Measured (profiles/r31, 2^20 entries of
//              one value): 0.19 ms against 11.9 ms with an atomic per lane; on a uniform column the two forms are equal.
// k_lk_mult    counters -> canonical elements M (a thread per entry, one 32-byte store).
// k_lk_pair    a thread per pair entry: one modular subtraction (D) or negation (N), two coalesced 32-byte stores; the padding of
//              both sides is written by the same launch.  All element offsets are 64-bit.
// The probes are bounded by the number of slots: a table that broke the load factor could not hang a launch.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"
#include "lookup_rules.h"

namespace gkr {

namespace {

constexpr bool kLkWaveCombine = true;
constexpr uint32_t kLkThreads = 256;

__device__ __forceinline__ uint32_t lk_slot(const Fr& v, uint32_t log_slots) { return lookup::slot_of(v.l, log_slots); }

// grid = (lk_blocks(n_t), tables), block = 256
__global__ void __launch_bounds__(kLkThreads) k_lk_build(const Fr* __restrict__ table, uint32_t n_t, uint32_t* __restrict__ index) {
    const uint32_t j = blockIdx.x * kLkThreads + threadIdx.x;
    if (j >= (1u << n_t)) return;
    const Fr* T = table + ((size_t)blockIdx.y << n_t);
    uint32_t* idx = index + ((size_t)blockIdx.y << (n_t + 1));
    const uint32_t log_slots = n_t + 1, mask = (1u << log_slots) - 1u;
    const Fr key = load_fr(T + j);
    uint32_t slot = lk_slot(key, log_slots);
    for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1u) & mask) {
        const uint32_t prev = atomicCAS(idx + slot, lookup::kEmpty, j);
        if (prev == lookup::kEmpty) return;
        if (fr_eq(load_fr(T + prev), key)) {
            atomicMin(idx + slot, j);
            return;
        }
    }
}

// grid = (lk_blocks(n_w), batch), block = 256; table_stride / index_stride: 0 for a shared table
__global__ void __launch_bounds__(kLkThreads) k_lk_count(const Fr* __restrict__ witness, uint32_t n_w, const Fr* __restrict__ table, uint32_t n_t,
                                                         size_t table_stride, const uint32_t* __restrict__ index, size_t index_stride,
                                                         uint32_t* __restrict__ counts, uint32_t* __restrict__ missing,
                                                         uint32_t* __restrict__ first_missing) {
    const uint32_t i = blockIdx.x * kLkThreads + threadIdx.x;
    const size_t b = blockIdx.y;
    const bool live = i < (1u << n_w);
    const Fr* T = table + b * table_stride;
    const uint32_t* idx = index + b * index_stride;
    const uint32_t log_slots = n_t + 1, mask = (1u << log_slots) - 1u;
    uint32_t hit = lookup::kEmpty;
    if (live) {
        const Fr key = load_fr(witness + (b << n_w) + i);
        uint32_t slot = lk_slot(key, log_slots);
        for (uint32_t probe = 0; probe <= mask; ++probe, slot = (slot + 1u) & mask) {
            const uint32_t e = idx[slot];
            if (e == lookup::kEmpty) break;
            if (fr_eq(load_fr(T + e), key)) {
                hit = e;
                break;
            }
        }
    }
    uint32_t* cnt = counts + (b << n_t);
    if (kLkWaveCombine) {
        // the lanes that share the first hit's index add their number at once; the others on their own
        const bool has = hit != lookup::kEmpty;
        const unsigned long long hits = __ballot(has);
        if (hits) {
            const int leader = __ffsll((long long)hits) - 1;
            const uint32_t lead = __shfl(hit, leader, 64);
            const bool same = has && hit == lead;
            const unsigned long long group = __ballot(same);
            if ((int)(threadIdx.x & 63u) == leader)
                atomicAdd(cnt + lead, (uint32_t)__popcll(group));
            else if (has && !same)
                atomicAdd(cnt + hit, 1u);
        }
    } else if (hit != lookup::kEmpty) {
        atomicAdd(cnt + hit, 1u);
    }
    if (live && hit == lookup::kEmpty) {
        atomicAdd(missing + b, 1u);
        atomicMin(first_missing + b, i);
    }
}

// grid = (blocks over batch * 2^n_t), block = 256
__global__ void __launch_bounds__(kLkThreads) k_lk_mult(const uint32_t* __restrict__ counts, size_t total, Fr* __restrict__ mult) {
    const size_t e = (size_t)blockIdx.x * kLkThreads + threadIdx.x;
    if (e >= total) return;
    Fr m = fr_zero();
    m.l[0] = counts[e];
    store_fr(mult + e, m);
}

// grid = (lk_blocks(L), batch), block = 256; pair b: N then D, 2^L each
__global__ void __launch_bounds__(kLkThreads) k_lk_pair(const Fr* __restrict__ witness, uint32_t n_w, const Fr* __restrict__ table, uint32_t n_t,
                                                        size_t table_stride, const Fr* __restrict__ mult, const Fr* __restrict__ alpha, uint32_t L,
                                                        Fr* __restrict__ pair) {
    const uint32_t e = blockIdx.x * kLkThreads + threadIdx.x;
    if (e >= (1u << L)) return;
    const size_t b = blockIdx.y;
    const uint32_t half = 1u << (L - 1), i = e & (half - 1u);
    Fr num = fr_zero(), den = fr_zero();
    den.l[0] = 1u;
    if (e < half) {
        if (i < (1u << n_w)) {
            num.l[0] = 1u;
            den = fr_sub(load_fr(alpha + b), load_fr(witness + (b << n_w) + i));
        }
    } else if (i < (1u << n_t)) {
        num = fr_sub(fr_zero(), load_fr(mult + (b << n_t) + i));
        den = fr_sub(load_fr(alpha + b), load_fr(table + b * table_stride + i));
    }
    Fr* out = pair + (b << (L + 1)) + e;
    store_fr(out, num);
    store_fr(out + ((size_t)1 << L), den);
}

}  // namespace

uint32_t lk_blocks(uint32_t log2_items) { return blocks_for((uint64_t)1 << log2_items, 0xFFFFFFFFu); }

void launch_lk_build(const Fr* table, uint32_t n_t, uint32_t tables, uint32_t* index, hipStream_t s) {
    hipLaunchKernelGGL(k_lk_build, dim3(lk_blocks(n_t), tables), dim3(kLkThreads), 0, s, table, n_t, index);
}

void launch_lk_count(const Fr* witness, uint32_t n_w, const Fr* table, uint32_t n_t, bool shared_table, const uint32_t* index, uint32_t batch,
                     uint32_t* counts, uint32_t* missing, uint32_t* first_missing, hipStream_t s) {
    hipLaunchKernelGGL(k_lk_count, dim3(lk_blocks(n_w), batch), dim3(kLkThreads), 0, s, witness, n_w, table, n_t,
                       shared_table ? (size_t)0 : (size_t)1 << n_t, index, shared_table ? (size_t)0 : (size_t)2 << n_t, counts, missing, first_missing);
}

void launch_lk_mult(const uint32_t* counts, uint32_t n_t, uint32_t batch, Fr* mult, hipStream_t s) {
    const size_t total = (size_t)batch << n_t;
    hipLaunchKernelGGL(k_lk_mult, dim3(blocks_for(total, 0xFFFFFFFFu)), dim3(kLkThreads), 0, s, counts, total, mult);
}

void launch_lk_pair(const Fr* witness, uint32_t n_w, const Fr* table, uint32_t n_t, bool shared_table, const Fr* mult, const Fr* alpha, uint32_t L,
                    uint32_t batch, Fr* pair, hipStream_t s) {
    hipLaunchKernelGGL(k_lk_pair, dim3(lk_blocks(L), batch), dim3(kLkThreads), 0, s, witness, n_w, table, n_t,
                       shared_table ? (size_t)0 : (size_t)1 << n_t, mult, alpha, L, pair);
}

}  // namespace gkr

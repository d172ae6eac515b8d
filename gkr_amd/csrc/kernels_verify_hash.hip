// CDNA4 (gfx950) kernel of the verifiers' challenge hashes (gkr_verify_prepared, gkr_mimc7_multi_hash_device: capi_verify.hip;
// gkr_sumcheck_mle_verify*, gkr_sumcheck_product_verify*: capi_mle_verify.hip): the round vectors of a chunk of proofs or
// transcripts, hashed where the rest of the chunk is checked.
//
//   k_verify_hash<S>    n rows of S right-aligned slots and n lengths -> per row multi_hash(row's trailing len slots, key 0)
//                       and a `valid` word: hash_piece's semantics (capi_verify.hip), row for row.  S = 3: the round vectors
//                       of a GKR proof and of product sumchecks up to degree 2; S = 4: the degree-3 product sumcheck's
//
// A prover hashes round j before it can form round j + 1; a verifier reads every challenge out of the proof, so the hashes of
// a chunk are a flat array of independent jobs.  Eight lanes per row (one 32-bit limb per lane, mimc_lanes.h), eight rows per
// wave, the layout of k_mle_pass_hash_lanes.
//
// Validity is decided per group from the raw limbs, before any Montgomery arithmetic: len outside 1 .. S, or a USED slot
// >= r, makes the row invalid.  An invalid row (and a group past the last row) hashes nothing: its length counts as zero and
// every element it would feed to the arithmetic is replaced by zero -- unused leading slots are replaced the same way, so a
// non-canonical value there is never an operand.
//
// Divergence: there is none.  The ballot carry lookahead and the DPP moves of mimc_lanes.h need every lane of the wave at the
// same instruction, so the wave runs the LONGEST length of its eight groups (a scalar trip count) with all 64 lanes active; a
// group whose own length is shorter (or zero) computes along on zeros and keeps the state it had.  The lookahead masks stop
// every carry at its group's top lane and the DPP moves stay inside a group, so what a group computes along on cannot reach
// the seven others.
#include <hip/hip_runtime.h>

#include "dev_util.h"
#include "kernels.h"
#include "mimc_lanes.h"

namespace gkr {

namespace {

// is the group's value (limb j in lane j) below r?  Lanes whose limb is below r's against lanes whose limb is above it, as
// two 8-bit integers: the most significant differing limb decides, so the value is below r iff the first is the larger.
// Every lane of the group gets the answer; every lane of the wave must be here.
__device__ __forceinline__ bool group_below_r(uint32_t x, const lanes::Ctx& c) {
    const uint64_t lt = __ballot(x < c.pj), gt = __ballot(x > c.pj);
    const uint32_t sh = ((threadIdx.x & 63u) >> 3) * 8u;
    return (uint32_t)((lt >> sh) & 0xffull) > (uint32_t)((gt >> sh) & 0xffull);
}

}  // namespace

// grid = ceil(n / 8), block = 64: group g of the block = row blockIdx.x * 8 + g.  rows: SLOTS * 8 words per row (SLOTS slots of
// 8 little-endian limbs: 24 words for the GKR round vectors, 32 for the degree-3 product sumcheck's), len: one word per row,
// out: one VerifyHashSlot per row.  Slot t of a row is held in s[t]; every index into s is a constant after unrolling, and
// the slot of element i is SELECTED BY VALUE (a chain of ?:), never by a run-time index into a private array.
template <int SLOTS>
__global__ void __launch_bounds__(64) k_verify_hash(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ len, uint32_t n,
                                                    const Fr* __restrict__ cts, VerifyHashSlot* __restrict__ out) {
    static_assert(SLOTS == 3 || SLOTS == 4, "rows of three or four slots");
    const lanes::Ctx c = lanes::make_ctx();
    const uint32_t grp = (threadIdx.x & 63u) >> 3, j = c.j;
    const uint32_t row_raw = blockIdx.x * 8u + grp;
    const bool live = row_raw < n;
    const uint32_t row = live ? row_raw : n - 1u;   // (a group past the end reads the last row and stores nothing)
    const uint32_t* src = rows + (size_t)row * (SLOTS * 8u) + j;
    uint32_t s[SLOTS];
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) s[t] = src[8 * t];
    const uint32_t ln_raw = len[row];
    const bool len_ok = live && ln_raw >= 1u && ln_raw <= (uint32_t)SLOTS;
    // the canonical tests run for every group (ballots); only the used slots' answers count: slot t is used iff len >= SLOTS - t
    bool valid = len_ok;
#pragma unroll
    for (int t = SLOTS - 1; t >= 0; --t) {
        const bool below = group_below_r(s[t], c);
        valid = valid && (ln_raw < (uint32_t)(SLOTS - t) || below);
    }
    const uint32_t ln = valid ? ln_raw : 0u;
    uint32_t longest = ln;
#pragma unroll
    for (int off = 8; off <= 32; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)longest, off, 64);
        longest = o > longest ? o : longest;
    }
    longest = (uint32_t)__builtin_amdgcn_readfirstlane((int)longest);
    uint32_t r = 0;
    for (uint32_t i = 0; i < longest; ++i) {
        // element i of this row's vector is slot SLOTS - ln + i; zero once the row's own vector has ended (or never began)
        const uint32_t slot = (uint32_t)SLOTS - ln + i;
        uint32_t pick = s[SLOTS - 1];
#pragma unroll
        for (int t = SLOTS - 2; t >= 0; --t) pick = slot == (uint32_t)t ? s[t] : pick;
        const uint32_t elem = i < ln ? pick : 0u;
        const uint32_t a = lanes::cond_sub(lanes::mont_mul(elem, c.r2j, c), c.pj, c);
        const uint32_t h = lanes::permutation(a, r, cts, c);
        uint32_t nr = lanes::add3(r, a, h, c);
        nr = lanes::cond_sub(lanes::cond_sub(nr, c.two_pj, c), c.pj, c);
        r = i < ln ? nr : r;
    }
    const uint32_t one = j == 0 ? 1u : 0u;
    const uint32_t hj = lanes::cond_sub(lanes::mont_mul(r, one, c), c.pj, c);
    if (live) {
        VerifyHashSlot* o = out + row;
        o->h[j] = valid ? hj : 0u;
        if (j == 0) o->valid = valid ? 1u : 0u;
    }
}

void launch_verify_hash(int slots, const uint32_t* rows, const uint32_t* len, uint32_t n, const Fr* cts, VerifyHashSlot* out, hipStream_t s) {
    if (slots == 4)
        hipLaunchKernelGGL(k_verify_hash<4>, dim3((n + 7u) / 8u), dim3(64), 0, s, rows, len, n, cts, out);
    else
        hipLaunchKernelGGL(k_verify_hash<3>, dim3((n + 7u) / 8u), dim3(64), 0, s, rows, len, n, cts, out);
}

}  // namespace gkr

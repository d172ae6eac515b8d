// CDNA4 (gfx950) kernels of the sumcheck over a SUM OF PRODUCTS of resident multilinear tables
// (gkr_sumcheck_sop_batch_device): prove_sumcheck (rust/src/gkr/sumcheck.rs:158-214) on
//   g = sum_k c_k prod_{j < d_k} T_{t(k, j)},   d_k <= 3,
// add_poly (poly.rs:293-334) over k of c_k mult_poly(..) of the tables' extensions, worked on the M tables themselves.  A table
// may stand in several terms and several times in one; it is folded ONCE per round.
//
// A pass (one launch, grid = (blocks per sumcheck, batch), the product path's geometry: blocked chunks at multiples of 256):
//   1. rounds 2..n: every table's entries of the block's chunk are folded with r_{j-1} and stored (fr_fold_fixed2; in place
//      from round 3 on, a thread writes only slots it alone has read);
//   2. term after term, the block walks its chunk again: a thread re-reads ITS OWN folded pairs of the term's d_k tables (its
//      own stores: program order, no barrier; they are in L2) and accumulates the term's d_k + 1 values of kernels_product.hip
//      (product_accumulate<d_k>) -- one term's lanes are live at a time, at most four lazy accumulators;
//   3. the term's block partial goes to partials[(b nblk + block) K + k].
// The round kernel (one wave per sumcheck) totals term after term, undoes the term's 2^(-256 (d_k - 1)) scaling, forms its
// coefficients, multiplies by c_k and adds them right-aligned into four slots; then the length rule, the hash, the next fold's
// multiplier table and, after round n, the tables' values at the challenges.  The chunk, the fold of the tables and the round
// kernel's steps are product_common.h's, shared with the zero-check (kernels_zerocheck.hip).
//
// The term structure is a kernel argument (SopTerms, SopCoeffs): wave-uniform, read with scalar loads; nothing indexes a
// per-thread array with a runtime value.  Term bounds: those of kernels_product.hip per term (the lanes start at zero for every
// term); the sum over terms is taken on reduced elements.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"
#include "mimc7.h"
#include "product_common.h"

namespace gkr {

namespace {

// one term's D + 1 values over entries begin .. end of the block's chunk: lo = T[i], hi = T[i + hi_off] of the term's D tables
// (t: table 0 of this sumcheck)
template <int D>
__device__ __forceinline__ void sop_term_values(const Fr* t, size_t stride, uint32_t term, uint32_t hi_off, uint32_t begin,
                                                uint32_t end, Acc<9>* smem, ProductPartial* out) {
    const Fr* tf[D];
#pragma unroll
    for (int j = 0; j < D; ++j) tf[j] = t + (size_t)sop_term_table(term, j) * stride;
    ProductLane<D> lane[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) lane[k] = product_lane_zero<D>();
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        Fr lo[D], hi[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            lo[j] = load_fr(tf[j] + i);
            hi[j] = load_fr(tf[j] + i + hi_off);
        }
        product_accumulate<D>(lane, lo, hi);
    }
    product_store_partial<D>(lane, smem, 0u, out);
}

// every term's partial of this block, term after term (the term is wave-uniform: the branches are scalar)
__device__ __forceinline__ void sop_terms_pass(const Fr* t, size_t stride, uint32_t hi_off, uint32_t begin, uint32_t end,
                                               const SopTerms& ts, Acc<9>* smem, ProductPartial* out) {
    for (uint32_t k = 0; k < ts.n_terms; ++k) {
        const uint32_t term = ts.term[k], d = sop_term_degree(term);
        if (d == 1)
            sop_term_values<1>(t, stride, term, hi_off, begin, end, smem, out + k);
        else if (d == 2)
            sop_term_values<2>(t, stride, term, hi_off, begin, end, smem, out + k);
        else
            sop_term_values<3>(t, stride, term, hi_off, begin, end, smem, out + k);
        __syncthreads();   // thread 0 has read the waves' sums before the next term's are written
    }
}

}  // namespace

// Round 1: every term's values over the input tables (not modified).  Table m of sumcheck b: tables + (b M + m) * stride.
// grid = (blocks per sumcheck, batch)
__global__ void __launch_bounds__(256) k_sop_first(const Fr* __restrict__ tables, size_t table_stride, uint32_t h, SopTerms ts,
                                                   ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * (kProductMaxDegree + 1)];
    const Fr* t = tables + (size_t)blockIdx.y * ts.n_tables * table_stride;
    uint32_t begin, end;
    block_chunk(h, begin, end);
    sop_terms_pass(t, table_stride, h, begin, end, ts, smem, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ts.n_terms);
}

// Rounds 2..n: fold every table ONCE with r_{j-1} (src 4q entries per table -> dst 2q), then every term's values over the folded
// tables.  src and dst may be the same buffer with equal strides (in place), hence no __restrict__ on either.
// grid = (blocks per sumcheck, batch)
__global__ void __launch_bounds__(256) k_sop_fold_sum(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q,
                                                      const FixedMul* __restrict__ rtab, uint32_t r_stride, SopTerms ts,
                                                      ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * (kProductMaxDegree + 1)];
    const Fr* s = src + (size_t)blockIdx.y * ts.n_tables * src_stride;
    Fr* d = dst + (size_t)blockIdx.y * ts.n_tables * dst_stride;
    const FixedMul T = rtab[(size_t)blockIdx.y * r_stride];   // wave-uniform -> scalar loads, lives in SGPRs
    uint32_t begin, end;
    block_chunk(q, begin, end);
    fold_tables_chunk(s, src_stride, d, dst_stride, ts.n_tables, q, T, begin, end);
    sop_terms_pass(d, dst_stride, q, begin, end, ts, smem, partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ts.n_terms);
}

// One wave per sumcheck and round: term after term the blocks' partials are totalled, the lazy sums' scaling undone, the term's
// coefficients formed (product_values_to_coeffs<d_k>), multiplied by c_k and added right-aligned into four slots.  Then, in EVERY
// round: leading zero coefficients dropped, one kept at least (add_poly merges by exponent and drops zero sums; g identically
// zero gives [0], the library's own choice), MiMC7 of the used slots, r published canonical and as the next fold's multiplier
// table.  Rows of out_coeffs have D + 1 slots, D = ts.max_degree.  After round n: evals[b M + m] = T_m~(r_1 .. r_n).
// grid = (batch), block = 64
__global__ void __launch_bounds__(64) k_sop_round(const ProductPartial* __restrict__ partials, uint32_t nblk, uint32_t round,
                                                  uint32_t n, SopTerms ts, SopCoeffs cf, const Fr* __restrict__ cts,
                                                  const Fr* __restrict__ work, size_t work_stride, Fr* __restrict__ out_coeffs,
                                                  uint32_t* __restrict__ out_len, Fr* __restrict__ out_r, FixedMul* __restrict__ rtab,
                                                  Fr* __restrict__ evals) {
    constexpr int S = kProductMaxDegree + 1;
    const uint32_t b = blockIdx.x, K = ts.n_terms;
    const ProductPartial* p = partials + (size_t)b * nblk * K;
    Fr sum[S];   // highest degree first, right-aligned (thread 0's)
    terms_total<kProductMaxDegree>(p, nblk, ts, cf, sum);
    if (threadIdx.x != 0) return;
    const size_t row = (size_t)b * n + round;   // (the slots above the call's degree hold zero: no term reaches them)
    const Fr r = round_publish<S>(sum, round_length<S>(sum), ts.max_degree, row, cts, out_coeffs, out_len, out_r);
    if (round + 1 < n)
        store_fixed_mul(rtab + row, r);
    else
        fold_last_entries(work, work_stride, b, ts.n_tables, to_mont(r), evals);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void launch_sop_first(const SopTerms& ts, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk,
                      ProductPartial* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_sop_first, dim3(nblk, batch), dim3(256), 0, s, tables, table_stride, h, ts, partials);
}

void launch_sop_fold_sum(const SopTerms& ts, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                         uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, ProductPartial* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_sop_fold_sum, dim3(nblk, batch), dim3(256), 0, s, src, src_stride, dst, dst_stride, q, rtab, r_stride, ts, partials);
}

void launch_sop_round(const SopTerms& ts, const SopCoeffs& cf, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n,
                      uint32_t batch, const Fr* cts, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                      FixedMul* rtab, Fr* evals, hipStream_t s) {
    hipLaunchKernelGGL(k_sop_round, dim3(batch), dim3(64), 0, s, partials, nblk, round, n, ts, cf, cts, work, work_stride, out_coeffs, out_len,
                       out_r, rtab, evals);
}

}  // namespace gkr

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
// multiplier table and, after round n, the tables' values at the challenges.
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

__device__ __forceinline__ uint32_t sop_term_degree(uint32_t term) { return term & 0xFFu; }
__device__ __forceinline__ uint32_t sop_term_table(uint32_t term, int j) { return (term >> (8 + 8 * j)) & 0xFFu; }

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
    const uint32_t chunk = ((h + gridDim.x - 1) / gridDim.x + 255u) & ~255u;   // blocked distribution, see k_mle_sum_first
    const uint32_t begin = blockIdx.x * chunk;
    const uint32_t end = begin + chunk < h ? begin + chunk : h;
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
    const uint32_t chunk = ((q + gridDim.x - 1) / gridDim.x + 255u) & ~255u;
    const uint32_t begin = blockIdx.x * chunk;
    const uint32_t end = begin + chunk < q ? begin + chunk : q;
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        for (uint32_t m = 0; m < ts.n_tables; ++m) {
            const Fr* sm = s + (size_t)m * src_stride;
            Fr* dm = d + (size_t)m * dst_stride;
            const Fr x0 = load_fr(sm + i), x1 = load_fr(sm + i + 2 * (size_t)q);
            const Fr x2 = load_fr(sm + i + q), x3 = load_fr(sm + i + 3 * (size_t)q);
            Fr lo, hi;
            fr_fold_fixed2(x0, x1, x2, x3, T, lo, hi);
            store_fr(dm + i, lo);
            store_fr(dm + i + q, hi);
        }
    }
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
#pragma unroll
    for (int k = 0; k < S; ++k) sum[k] = fr_zero();
    for (uint32_t t = 0; t < K; ++t) {
        const uint32_t d = sop_term_degree(ts.term[t]);
        Acc<10> tot[S];
#pragma unroll
        for (int k = 0; k < S; ++k) tot[k] = acc_zero<10>();
        for (uint32_t i = threadIdx.x; i < nblk; i += 64) {
            const ProductPartial* pp = p + (size_t)i * K + t;
#pragma unroll
            for (int k = 0; k < S; ++k)
                if ((uint32_t)k <= d) acc_add_acc(tot[k], pp->s[k]);
        }
#pragma unroll
        for (int k = 0; k < S; ++k) tot[k] = wave_sum(tot[k]);
        if (threadIdx.x == 0) {
            Fr v[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                v[k] = acc_reduce(tot[k]);
#pragma unroll
                for (int m = 1; m < kProductMaxDegree; ++m)
                    if ((uint32_t)m < d) v[k] = mont_mul(v[k], fr_r2());   // x 2^256 per lazy or Montgomery reduction taken
            }
            Fr c[S];
#pragma unroll
            for (int k = 0; k < S; ++k) c[k] = fr_zero();
            if (d == 1) {
                const Fr v1[2] = {v[0], v[1]};
                Fr c1[2];
                product_values_to_coeffs<1>(v1, c1);
                c[2] = c1[0];
                c[3] = c1[1];
            } else if (d == 2) {
                const Fr v2[3] = {v[0], v[1], v[2]};
                Fr c2[3];
                product_values_to_coeffs<2>(v2, c2);
                c[1] = c2[0];
                c[2] = c2[1];
                c[3] = c2[2];
            } else {
                product_values_to_coeffs<3>(v, c);
            }
            const Fr ck = to_mont(cf.c[t]);
#pragma unroll
            for (int k = 0; k < S; ++k) sum[k] = fr_add(sum[k], mont_mul(c[k], ck));
        }
    }
    if (threadIdx.x != 0) return;
    uint32_t lead = 0;
    bool leading = true;
#pragma unroll
    for (int k = 0; k < S - 1; ++k) {   // (slots above the call's degree hold zero: no term reaches them)
        leading = leading && fr_is_zero(sum[k]);
        lead += leading ? 1u : 0u;
    }
    const uint32_t len = (uint32_t)S - lead, D = ts.max_degree;
    const size_t row = (size_t)b * n + round;
    Fr* oc = out_coeffs + row * (D + 1);
    // multi_hash(used slots, key 0) as mimc7_multi_hash does it, the slots indexed statically (no private array in memory)
    Fr h = fr_zero();
#pragma unroll
    for (int k = 0; k < S; ++k) {
        if ((uint32_t)k + D >= (uint32_t)S - 1u) oc[(uint32_t)k + D - ((uint32_t)S - 1u)] = sum[k];   // (an unused slot holds zero)
        if ((uint32_t)k + len >= (uint32_t)S) {
            const Fr a = to_mont(sum[k]);
            h = fr_add(fr_add(h, a), mimc7_hash_mont(a, h, cts));
        }
    }
    const Fr r = from_mont(h);
    out_len[row] = len;
    out_r[row] = r;
    if (round + 1 < n) {
        store_fixed_mul(rtab + row, r);
    } else {
        const Fr r_mont = to_mont(r);
        for (uint32_t m = 0; m < ts.n_tables; ++m) {
            const Fr* t = work + ((size_t)b * ts.n_tables + m) * work_stride;
            evals[(size_t)b * ts.n_tables + m] = fr_fold(t[0], t[1], r_mont);
        }
    }
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

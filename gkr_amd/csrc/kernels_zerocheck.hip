// CDNA4 (gfx950) kernels of the ZERO-CHECK sumcheck (gkr_sumcheck_zerocheck_batch_device): prove_sumcheck on
//   eq(z, x) g(x),   g = sum_k c_k prod_{f < d_k} T_{t(k, f)},   d_k <= 2,
// with the transcript the sum-of-products path (kernels_sop.hip) writes when eq(z, .) is handed to it as one more table and
// every term is prefixed by it -- but eq(z, .) is never a table of 2^n entries here.  In round j, on the current (folded) tables
// of 2^(n-j+1) entries (lo_f = T_f[i], hi_f = T_f[i + 2^(n-j)], i < 2^(n-j)),
//   h_j(X) = sum_i w_j(i) sum_k c_k prod_f (lo_f + X (hi_f - lo_f)),     w_j(i) = eq((z_{j+1} .. z_n), i),
//   g_j(X) = s_j ((1 - z_j) + (2 z_j - 1) X) h_j(X),                     s_j = prod_{l < j} eq(z_l, r_l):
// the eq factor of the variables already bound is the scalar s_j, of the round's own variable a linear factor, of the variables
// still free the weight w_j.  Nothing divides: z_j in {0, 1} is an ordinary point.
//
// The weights.  w_j is not a table of 2^(n-j) entries either:  w_j(i) = E_hi,j[i >> 8] * E_lo[i & 255].  A pass has the SOP
// kernels' geometry (blocked chunks at multiples of 256, a thread strides by 256), so
//   E_lo[i & 255]   is ONE element per thread: applied once per thread and term, after the lazy sum is reduced;
//   E_hi,j[i >> 8]  is the same on every thread of the block in an iteration: a scalar load, its limbs multiply from SGPRs.
// E_lo = eq((z_{n-7} .. z_n), .) serves every round with eight or more free variables; E_hi,j = eq((z_{j+1} .. z_{n-8}), .) has
// 2^(n-j-8) entries, 2^(n-8) - 1 over all rounds.  A round with k < 8 free variables takes E_hi = [1] and the 2^k-entry
// eq((z_{n-k+1} .. z_n), .) for E_lo (255 entries over all k).  All of them come from launch_eq_table, once per call, in
// Montgomery form.
//
// What a thread accumulates (every value of a term is linear in the term's first factor pair):
//   d_k = 1:  P(0), P(1): lazy sums of T[i] * E_hi[c] (one unreduced multiply-add with a scalar operand per value and index);
//   d_k = 2:  the first pair is scaled, lo_0' = lo_0 E_hi[c], hi_0' = hi_0 E_hi[c] (two Montgomery products with a scalar
//             operand), then P(0), P(1), P(inf) are the lazy sums of kernels_product.hip's degree 2.
// Inner degree <= 2 needs three values at most: no P(-1), no halving.  Scaling: a degree-1 value is exact (the lazy reduction's
// 2^-256 meets E_lo's Montgomery form), a degree-2 value carries 2^-256 as on the SOP path; the round kernel undoes it.
//
// The term structure is a kernel argument (SopTerms, SopCoeffs): wave-uniform, read with scalar loads; nothing indexes a
// per-thread array with a runtime value.  The chunk, the fold of the tables and the round kernel's steps (a term's total, the
// length rule, the row and its hash, the tables' last values) are product_common.h's, shared with kernels_sop.hip.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"
#include "mimc7.h"
#include "product_common.h"

namespace gkr {

namespace {

constexpr int kZcValues = 3;   // values (and coefficients) of h_j: inner degree <= 2

// one term's D + 1 WEIGHTED values over entries begin .. end of the block's chunk (begin a multiple of 256, blockDim.x = 256):
// e_hi this sumcheck's E_hi of the round, e_lo this thread's E_lo entry (both Montgomery)
template <int D>
__device__ __forceinline__ void zc_term_values(const Fr* t, size_t stride, uint32_t term, uint32_t hi_off, uint32_t begin, uint32_t end,
                                               const Fr* __restrict__ e_hi, const Fr& e_lo, Acc<9>* smem, ProductPartial* out) {
    static_assert(D == 1 || D == 2, "inner degree 1 or 2");
    const Fr* tf[D];
#pragma unroll
    for (int j = 0; j < D; ++j) tf[j] = t + (size_t)sop_term_table(term, j) * stride;
    Lazy17 lane[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) lane[k] = lazy_zero();
    for (uint32_t c = begin >> 8; (c << 8) < end; ++c) {   // c = i >> 8: block-uniform
        const Fr w = load_fr(e_hi + c);
        const uint32_t i = (c << 8) + threadIdx.x;
        if (i < end) {   // (false only in a round with fewer than 256 entries)
            if constexpr (D == 1) {
                lazy_mac_s(lane[0], load_fr(tf[0] + i), w);
                lazy_mac_s(lane[1], load_fr(tf[0] + i + hi_off), w);
            } else {
                const Fr lo0 = mont_mul(load_fr(tf[0] + i), w), hi0 = mont_mul(load_fr(tf[0] + i + hi_off), w);
                const Fr lo1 = load_fr(tf[1] + i), hi1 = load_fr(tf[1] + i + hi_off);
                lazy_mac_v(lane[0], lo0, lo1);
                lazy_mac_v(lane[1], hi0, hi1);
                lazy_mac_v(lane[2], fr_sub(hi0, lo0), fr_sub(hi1, lo1));
            }
        }
    }
    Acc<9> acc[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        acc[k] = acc_zero<9>();
        acc_add_fr(acc[k], mont_mul(lazy_reduce(lane[k]), e_lo));
    }
    block_sum<9, D + 1>(acc, smem);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k <= D; ++k) out->s[k] = acc[k];
        out->flags = 0u;
    }
}

// every term's weighted partial of this block, term after term (the term is wave-uniform: the branches are scalar).
// q = 2^(kh + kl) entries per half table; e_hi, e_lo: the round's tables of ALL sumchecks (sumcheck b at b << kh, b << kl)
__device__ __forceinline__ void zc_terms_pass(const Fr* t, size_t stride, uint32_t hi_off, uint32_t begin, uint32_t end, const SopTerms& ts,
                                              const Fr* __restrict__ e_hi, uint32_t kh, const Fr* __restrict__ e_lo, uint32_t kl, Acc<9>* smem,
                                              ProductPartial* out) {
    const Fr* hi = e_hi + ((size_t)blockIdx.y << kh);
    const Fr lo = threadIdx.x < (1u << kl) ? load_fr(e_lo + ((size_t)blockIdx.y << kl) + threadIdx.x) : fr_zero();
    for (uint32_t k = 0; k < ts.n_terms; ++k) {
        const uint32_t term = ts.term[k];
        if (sop_term_degree(term) == 1)
            zc_term_values<1>(t, stride, term, hi_off, begin, end, hi, lo, smem, out + k);
        else
            zc_term_values<2>(t, stride, term, hi_off, begin, end, hi, lo, smem, out + k);
        __syncthreads();   // thread 0 has read the waves' sums before the next term's are written
    }
}

}  // namespace

// Round 1: every term's weighted values over the input tables (not modified).  Table m of sumcheck b: tables + (b M + m) * stride.
// grid = (blocks per sumcheck, batch), block = 256
__global__ void __launch_bounds__(256) k_zc_first(const Fr* __restrict__ tables, size_t table_stride, uint32_t h, SopTerms ts,
                                                  const Fr* __restrict__ e_hi, uint32_t kh, const Fr* __restrict__ e_lo, uint32_t kl,
                                                  ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * kZcValues];
    const Fr* t = tables + (size_t)blockIdx.y * ts.n_tables * table_stride;
    uint32_t begin, end;
    block_chunk(h, begin, end);
    zc_terms_pass(t, table_stride, h, begin, end, ts, e_hi, kh, e_lo, kl, smem,
                  partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ts.n_terms);
}

// Rounds 2..n: fold every table ONCE with r_{j-1} (src 4q entries per table -> dst 2q), then every term's weighted values over the
// folded tables.  src and dst may be the same buffer with equal strides (in place), hence no __restrict__ on either.
// grid = (blocks per sumcheck, batch), block = 256
__global__ void __launch_bounds__(256) k_zc_fold_sum(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q,
                                                     const FixedMul* __restrict__ rtab, uint32_t r_stride, SopTerms ts,
                                                     const Fr* __restrict__ e_hi, uint32_t kh, const Fr* __restrict__ e_lo, uint32_t kl,
                                                     ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * kZcValues];
    const Fr* s = src + (size_t)blockIdx.y * ts.n_tables * src_stride;
    Fr* d = dst + (size_t)blockIdx.y * ts.n_tables * dst_stride;
    const FixedMul T = rtab[(size_t)blockIdx.y * r_stride];   // wave-uniform -> scalar loads, lives in SGPRs
    uint32_t begin, end;
    block_chunk(q, begin, end);
    fold_tables_chunk(s, src_stride, d, dst_stride, ts.n_tables, q, T, begin, end);
    zc_terms_pass(d, dst_stride, q, begin, end, ts, e_hi, kh, e_lo, kl, smem,
                  partials + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ts.n_terms);
}

// One wave per sumcheck and round: term after term the blocks' partials are totalled, a degree-2 term's 2^-256 undone, the term's
// coefficients formed (product_values_to_coeffs<d_k>), multiplied by c_k and added right-aligned into h_j's three slots.  Then
// (from here on zc_round_tail, product_common.h, shared with k_fs_round) g_j = (a + b X) h_j with a = s_j (1 - z_j),
// b = s_j (2 z_j - 1), written out slot by slot, and the sum-of-products path's steps
// of EVERY round (product_common.h): leading zero coefficients dropped, one kept at least, MiMC7 of the used slots, r published
// canonical and as the next fold's multiplier table.  s_{j+1} = a + b r_j goes to the sumcheck's slot s_slot[b] (Montgomery).  Rows of out_coeffs have
// D + 1 slots, D = ts.max_degree + 1.  After round n: evals[b M + m] = T_m~(r_1 .. r_n) and eq_out[b] = s_{n+1} = eq(z, r).
// grid = (batch), block = 64
__global__ void __launch_bounds__(64) k_zc_round(const ProductPartial* __restrict__ partials, uint32_t nblk, uint32_t round, uint32_t n,
                                                 SopTerms ts, SopCoeffs cf, const Fr* __restrict__ cts, const Fr* __restrict__ z,
                                                 Fr* __restrict__ s_slot, const Fr* __restrict__ work, size_t work_stride,
                                                 Fr* __restrict__ out_coeffs, uint32_t* __restrict__ out_len, Fr* __restrict__ out_r,
                                                 FixedMul* __restrict__ rtab, Fr* __restrict__ evals, Fr* __restrict__ eq_out) {
    constexpr int V = kZcValues;
    const uint32_t b = blockIdx.x, K = ts.n_terms;
    const ProductPartial* p = partials + (size_t)b * nblk * K;
    Fr h[V];   // h_j, highest degree first, right-aligned (thread 0's)
    terms_total<V - 1>(p, nblk, ts, cf, h);
    if (threadIdx.x != 0) return;
    zc_round_tail(h, b, round, n, ts.n_tables, ts.max_degree, cts, z, s_slot, work, work_stride, out_coeffs, out_len, out_r, rtab, evals, eq_out);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

size_t zc_weight_elements(uint32_t n, uint32_t batch) {
    const uint32_t mh = n > 9u ? n - 9u : 0u, ml = n - 1u < 8u ? n - 1u : 8u;
    return (size_t)batch * ((((size_t)2 << mh) - 1u) + (((size_t)2 << ml) - 1u));
}

ZcWeights zc_weights_layout(Fr* base, uint32_t n, uint32_t batch) {
    const uint32_t mh = n > 9u ? n - 9u : 0u;
    ZcWeights w;
    w.hi = base;
    w.lo = base + (size_t)batch * (((size_t)2 << mh) - 1u);
    w.batch = batch;
    return w;
}

void launch_zc_weights(const Fr* points, uint32_t n, uint32_t batch, const ZcWeights& w, hipStream_t s) {
    const uint32_t mh = n > 9u ? n - 9u : 0u, ml = n - 1u < 8u ? n - 1u : 8u;
    for (uint32_t k = 0; k <= ml; ++k) launch_eq_table(points, n, n - k, k, w.lo + (size_t)batch * ((1u << k) - 1u), true, batch, s);
    // (m = 0: the one-entry table [1] of the rounds with eight free variables or fewer; at n < 8 `first` is not looked at)
    for (uint32_t m = 0; m <= mh; ++m)
        launch_eq_table(points, n, n >= 8u + m ? n - 8u - m : 0u, m, w.hi + (size_t)batch * ((1u << m) - 1u), true, batch, s);
}

void launch_zc_first(const SopTerms& ts, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk, const ZcWeights& w,
                     uint32_t kh, uint32_t kl, ProductPartial* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_zc_first, dim3(nblk, batch), dim3(256), 0, s, tables, table_stride, h, ts, w.hi_table(kh), kh, w.lo_table(kl), kl, partials);
}

void launch_zc_fold_sum(const SopTerms& ts, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                        uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, const ZcWeights& w, uint32_t kh, uint32_t kl,
                        ProductPartial* partials, hipStream_t s) {
    hipLaunchKernelGGL(k_zc_fold_sum, dim3(nblk, batch), dim3(256), 0, s, src, src_stride, dst, dst_stride, q, rtab, r_stride, ts, w.hi_table(kh), kh,
                       w.lo_table(kl), kl, partials);
}

void launch_zc_round(const SopTerms& ts, const SopCoeffs& cf, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n,
                     uint32_t batch, const Fr* cts, const Fr* z, Fr* s_slot, const Fr* work, size_t work_stride, Fr* out_coeffs,
                     uint32_t* out_len, Fr* out_r, FixedMul* rtab, Fr* evals, Fr* eq_out, hipStream_t s) {
    hipLaunchKernelGGL(k_zc_round, dim3(batch), dim3(64), 0, s, partials, nblk, round, n, ts, cf, cts, z, s_slot, work, work_stride, out_coeffs,
                       out_len, out_r, rtab, evals, eq_out);
}

}  // namespace gkr

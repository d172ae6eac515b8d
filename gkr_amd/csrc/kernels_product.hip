// CDNA4 (gfx950) kernels of the sumcheck over a PRODUCT of D <= 3 resident multilinear tables
// (gkr_sumcheck_product_batch_device): prove_sumcheck (rust/src/gkr/sumcheck.rs:158-214) on
// g = mult_poly(get_multi_ext(T_0), .., get_multi_ext(T_{D-1})) (poly.rs:349-386), worked on the tables themselves.
//
// Round j's polynomial is  P(t) = sum_{i < h} prod_f (T_f[i] + t (T_f[i + h] - T_f[i])),  degree D.  A pass accumulates D + 1
// exact VALUES of it -- P(0), P(1), the leading coefficient P(inf) = sum prod_f (hi_f - lo_f), and for D = 3 also P(-1) --
// and the round kernel turns them into the coefficients (division by two only; exact in the field).
//
// A value is a sum of products of D canonical elements.  The first D - 2 factors are multiplied with mont_mul (each leaves a
// factor 2^-256), the last product of every term goes unreduced into a Lazy17 accumulator (lazy_mac_v), whose one reduction
// per thread leaves another 2^-256: a thread hands block_sum the value times 2^(-256 (D - 1)), and the round kernel multiplies
// the totals back (D - 1 Montgomery products by 2^512).
// Term bounds: a Lazy17 takes 2^36 products; a thread adds one per table pair it visits, at most ceil(chunk / 256) <= 2^21
// (one block of a 2^29-entry half) and 1024 with the launch geometry of mle_blocks_per_table.  An Acc<9> takes 2^32 canonical
// addends and gets 256 per block; the round kernel's Acc<10> takes 2^32 Acc<9> and gets at most kMaxBlocksPerTable.
//
// Launch geometry: that of the plain sumcheck (k_mle_sum_first / k_mle_fold_sum): grid (blocks per sumcheck, batch), blocked
// distribution with chunk starts at multiples of 256; one block walks all D factors of its chunk.
// The chunk, the lanes, the values -> coefficients step and the round's publication (row, hash, r) are product_common.h's, shared
// with kernels_sop.hip and kernels_zerocheck.hip; the length rule of round n and the zero-factor rule are this path's own.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"
#include "mimc7.h"
#include "product_common.h"

namespace gkr {

namespace {

constexpr uint32_t kProductNonZeroShift = 8;   // ProductPartial::flags: bit f "factor f depends on x_n", bit 8 + f "factor f has a non-zero entry"

}  // namespace

// Round 1: the D + 1 values of P over the input tables, and per factor "depends on x_n" (the last round's length rule) and
// "has a non-zero entry" (a zero factor makes g the empty term list).  Factor f of sumcheck b: tables + (b D + f) * stride.
// grid = (blocks per sumcheck, batch)
template <int D>
__global__ void __launch_bounds__(256) k_product_first(const Fr* __restrict__ tables, size_t table_stride, uint32_t h,
                                                       ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * (D + 1)];
    __shared__ uint32_t s_flags;
    const Fr* t = tables + (size_t)blockIdx.y * D * table_stride;
    ProductLane<D> lane[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) lane[k] = product_lane_zero<D>();
    uint32_t flags = 0;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();
    // h is a power of two >= 2 and chunk starts are multiples of 256: lanes i and i ^ 1 are neighbours of one wave, both active
    uint32_t begin, end;
    block_chunk(h, begin, end);
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        Fr lo[D], hi[D];
#pragma unroll
        for (int f = 0; f < D; ++f) {
            const Fr* tf = t + (size_t)f * table_stride;
            lo[f] = load_fr(tf + i);
            hi[f] = load_fr(tf + i + h);
            uint32_t diff = 0, any = 0;   // element 2m against 2m + 1 (DPP quad_perm [1,0,3,2], see k_mle_sum_first)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                diff |= lo[f].l[k] ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)lo[f].l[k], 0xB1, 0xF, 0xF, true);
                diff |= hi[f].l[k] ^ (uint32_t)__builtin_amdgcn_mov_dpp((int)hi[f].l[k], 0xB1, 0xF, 0xF, true);
                any |= lo[f].l[k] | hi[f].l[k];
            }
            flags |= (diff ? 1u : 0u) << f;
            flags |= (any ? 1u : 0u) << (kProductNonZeroShift + f);
        }
        product_accumulate<D>(lane, lo, hi);
    }
    if (flags) atomicOr(&s_flags, flags);
    __syncthreads();
    product_store_partial<D>(lane, smem, s_flags, partials + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// Rounds 2..n: fold every factor with r_{j-1} (src 4q entries per factor -> dst 2q) and accumulate the D + 1 values of the
// folded tables' P in the same pass.  In place (dst == src, equal strides) is safe: a thread writes only slots it alone has read.
// grid = (blocks per sumcheck, batch)
template <int D>
__global__ void __launch_bounds__(256) k_product_fold_sum(const Fr* __restrict__ src, size_t src_stride, Fr* __restrict__ dst,
                                                          size_t dst_stride, uint32_t q, const FixedMul* __restrict__ rtab,
                                                          uint32_t r_stride, ProductPartial* __restrict__ partials) {
    __shared__ Acc<9> smem[4 * (D + 1)];
    const Fr* s = src + (size_t)blockIdx.y * D * src_stride;
    Fr* d = dst + (size_t)blockIdx.y * D * dst_stride;
    const FixedMul T = rtab[(size_t)blockIdx.y * r_stride];   // wave-uniform -> scalar loads, lives in SGPRs
    ProductLane<D> lane[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) lane[k] = product_lane_zero<D>();
    uint32_t begin, end;
    block_chunk(q, begin, end);
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        Fr lo[D], hi[D];
#pragma unroll
        for (int f = 0; f < D; ++f) {
            const Fr* sf = s + (size_t)f * src_stride;
            Fr* df = d + (size_t)f * dst_stride;
            const Fr x0 = load_fr(sf + i), x1 = load_fr(sf + i + 2 * (size_t)q);
            const Fr x2 = load_fr(sf + i + q), x3 = load_fr(sf + i + 3 * (size_t)q);
            fr_fold_fixed2(x0, x1, x2, x3, T, lo[f], hi[f]);
            store_fr(df + i, lo[f]);
            store_fr(df + i + q, hi[f]);
        }
        product_accumulate<D>(lane, lo, hi);
    }
    product_store_partial<D>(lane, smem, 0u, partials + (size_t)blockIdx.y * gridDim.x + blockIdx.x);
}

// One wave per sumcheck and round: total the blocks' partials, undo the lazy sums' scaling, values -> coefficients c_D .. c_0,
// the reference's length rule, MiMC7 of the round vector, r published canonical and as the next fold's multiplier table.
//   rounds 1..n-1: leading zero coefficients dropped, one kept at least (add_poly merges by exponent and drops zero sums,
//                  poly.rs:324-327);
//   round n:       1 + (factors that depend on x_n) coefficients (no merge, sumcheck.rs:206-207);
//   a zero factor: every round vector is [0] (the library's own choice: the reference panics on the empty term list).
// After round n the last fold of every factor's two remaining entries: evals[b D + f] = T_f~(r_1 .. r_n).
// meta[b] (written in round 1): bits 0..7 the number of factors that depend on x_n, bit 8 "a factor is the zero table".
// grid = (batch), block = 64
template <int D>
__global__ void __launch_bounds__(64) k_product_round(const ProductPartial* __restrict__ partials, uint32_t nblk, uint32_t round,
                                                      uint32_t n, const Fr* __restrict__ cts, const Fr* __restrict__ work,
                                                      size_t work_stride, Fr* __restrict__ out_coeffs,
                                                      uint32_t* __restrict__ out_len, Fr* __restrict__ out_r,
                                                      FixedMul* __restrict__ rtab, uint32_t* __restrict__ meta,
                                                      Fr* __restrict__ evals) {
    const uint32_t b = blockIdx.x;
    const ProductPartial* p = partials + (size_t)b * nblk;
    Acc<10> tot[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) tot[k] = acc_zero<10>();
    uint32_t flags = 0;
    for (uint32_t i = threadIdx.x; i < nblk; i += 64) {
#pragma unroll
        for (int k = 0; k <= D; ++k) acc_add_acc(tot[k], p[i].s[k]);
        flags |= p[i].flags;
    }
#pragma unroll
    for (int k = 0; k <= D; ++k) tot[k] = wave_sum(tot[k]);
#pragma unroll
    for (int f = 0; f < D; ++f) {   // OR over the wave, bit by bit
        const uint32_t dep_bit = 1u << f, nz_bit = 1u << (kProductNonZeroShift + f);
        flags = (flags & ~(dep_bit | nz_bit)) | (__any(flags & dep_bit) ? dep_bit : 0u) | (__any(flags & nz_bit) ? nz_bit : 0u);
    }
    if (threadIdx.x != 0) return;
    if (round == 0) {
        uint32_t ndep = 0, zero = 0;
#pragma unroll
        for (int f = 0; f < D; ++f) {
            ndep += (flags >> f) & 1u;
            zero |= ((flags >> (kProductNonZeroShift + f)) & 1u) ^ 1u;
        }
        meta[b] = ndep | (zero << 8);
    }
    Fr v[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        v[k] = acc_reduce(tot[k]);
#pragma unroll
        for (int m = 1; m < D; ++m) v[k] = mont_mul(v[k], fr_r2());   // x 2^256 per lazy or Montgomery reduction taken
    }
    Fr c[D + 1];   // highest degree first
    product_values_to_coeffs<D>(v, c);
    uint32_t len;
    if (round + 1 < n) {
        len = round_length<D + 1>(c);
    } else {   // this path's own rule; the slots in front of the last len are cleared (zero already, by the rule's own argument)
        const uint32_t m = meta[b];
        len = (m >> 8) ? 1u : 1u + (m & 0xFFu);
#pragma unroll
        for (int k = 0; k < D; ++k)
            if ((uint32_t)k + len < (uint32_t)D + 1u) c[k] = fr_zero();
    }
    const size_t row = (size_t)b * n + round;
    const Fr r = round_publish<D + 1>(c, len, (uint32_t)D, row, cts, out_coeffs, out_len, out_r);
    if (round + 1 < n)
        store_fixed_mul(rtab + row, r);
    else
        fold_last_entries(work, work_stride, b, (uint32_t)D, to_mont(r), evals);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

void launch_product_first(int degree, const Fr* tables, size_t table_stride, uint32_t h, uint32_t batch, uint32_t nblk,
                          ProductPartial* partials, hipStream_t s) {
    const dim3 grid(nblk, batch), block(256);
    if (degree == 1)
        hipLaunchKernelGGL(k_product_first<1>, grid, block, 0, s, tables, table_stride, h, partials);
    else if (degree == 2)
        hipLaunchKernelGGL(k_product_first<2>, grid, block, 0, s, tables, table_stride, h, partials);
    else
        hipLaunchKernelGGL(k_product_first<3>, grid, block, 0, s, tables, table_stride, h, partials);
}

void launch_product_fold_sum(int degree, const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t q, uint32_t batch,
                             uint32_t nblk, const FixedMul* rtab, uint32_t r_stride, ProductPartial* partials, hipStream_t s) {
    const dim3 grid(nblk, batch), block(256);
    if (degree == 1)
        hipLaunchKernelGGL(k_product_fold_sum<1>, grid, block, 0, s, src, src_stride, dst, dst_stride, q, rtab, r_stride, partials);
    else if (degree == 2)
        hipLaunchKernelGGL(k_product_fold_sum<2>, grid, block, 0, s, src, src_stride, dst, dst_stride, q, rtab, r_stride, partials);
    else
        hipLaunchKernelGGL(k_product_fold_sum<3>, grid, block, 0, s, src, src_stride, dst, dst_stride, q, rtab, r_stride, partials);
}

void launch_product_round(int degree, const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n, uint32_t batch,
                          const Fr* cts, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r,
                          FixedMul* rtab, uint32_t* meta, Fr* evals, hipStream_t s) {
    const dim3 grid(batch), block(64);
    if (degree == 1)
        hipLaunchKernelGGL(k_product_round<1>, grid, block, 0, s, partials, nblk, round, n, cts, work, work_stride, out_coeffs,
                           out_len, out_r, rtab, meta, evals);
    else if (degree == 2)
        hipLaunchKernelGGL(k_product_round<2>, grid, block, 0, s, partials, nblk, round, n, cts, work, work_stride, out_coeffs,
                           out_len, out_r, rtab, meta, evals);
    else
        hipLaunchKernelGGL(k_product_round<3>, grid, block, 0, s, partials, nblk, round, n, cts, work, work_stride, out_coeffs,
                           out_len, out_r, rtab, meta, evals);
}

}  // namespace gkr

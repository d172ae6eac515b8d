// CDNA4 (gfx950) kernels of the FRACTIONAL SUM (LogUp) argument (gkr_fraction_sum_batch_device): over `batch` resident pairs of
// tables N (numerators) and D (denominators) of 2^n canonical values the binary tree of fraction additions,
//   (p_n, q_n) = (N, D),   p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i],   q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k]
//   (i < 2^k, k = n-1 .. 0),   (P, Q) = (p_0[0], q_0[0]),   sum_i N[i] / D[i] = P / Q;   nothing is inverted,
// and the round kernel of its layers' zero-checks.  Variable 1 = the most significant index bit, so a node's operands are entry
// i of the two contiguous halves of p_{k+1} and of q_{k+1}.  Every level is stored, canonical, in the INPUT'S OWN LAYOUT: level k
// of pair b is p_k (2^k) then q_k (2^k) at layers + fs_layer_offset(k, batch) + b * 2^(k+1), so the four halves of level k + 1 --
// T0 = p lo, T1 = p hi, T2 = q lo, T3 = q hi -- lie at (4 b + m) * 2^k: the zero-check's batch layout of four tables, in place.
//
// k_fs_level: ONE LAUNCH PER LEVEL, a thread per node: four coalesced loads, two coalesced stores, FIVE Montgomery products -- q lo
// and q hi are lifted to Montgomery form once, then p lo * q hi, p hi * q lo and q lo * q hi each take one.  68 VGPRs, 24 SGPRs,
// scratch 0, 7 waves per SIMD; no LDS, no barrier; all element offsets are 64-bit.  Fused levels are not built: they lost for the product tree
// (profiles/r27), which has less arithmetic per byte than this node.
//
// k_fs_round: k_zc_round for g = T0 T3 + T1 T2 + lambda_b T2 T3, the third coefficient read per sumcheck from a device array (a
// layer's two claims are combined with a lambda of that proof's own transcript; SopCoeffs is one kernel argument for the whole
// batch).  term_total_coeffs<2> is called three times with the coefficient given explicitly: no per-thread coefficient array
// exists.  Behind h_j every step is zc_round_tail (product_common.h), the one k_zc_round runs.  162 VGPRs, 76 SGPRs, 144 B of
// scratch -- the one-lane hash's, as in k_zc_round (150 VGPRs, 66 SGPRs, 144 B: unchanged by the shared tail).
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"
#include "mimc7.h"
#include "product_common.h"

namespace gkr {

namespace {

constexpr uint32_t kFsTables = 4, kFsTerms = 3, kFsDegree = 2;

// level k of every pair from level k + 1: src and dst are the levels' bases (pair b at + b * 2^(k+2) and + b * 2^(k+1))
__global__ void __launch_bounds__(256) k_fs_level(const Fr* __restrict__ src, Fr* __restrict__ dst, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (1u << k)) return;
    const size_t b = blockIdx.y, h = (size_t)1 << k;
    const Fr* in = src + (b << (k + 2)) + i;
    const Fr a0 = load_fr(in), a1 = load_fr(in + h), b0 = load_fr(in + 2 * h), b1 = load_fr(in + 3 * h);
    const Fr b0m = to_mont(b0), b1m = to_mont(b1);
    Fr* out = dst + (b << (k + 1)) + i;
    store_fr(out, fr_add(mont_mul(a0, b1m), mont_mul(a1, b0m)));   // canonical x Montgomery -> canonical
    store_fr(out + h, mont_mul(b0, b1m));
}

// One wave per sumcheck and round of a layer: the three terms' totals with the coefficients 1, 1, lambda[b] (canonical), then the
// zero-check's own round.  partials: batch x nblk x 3; rows of four slots; evals: batch x 4.
// grid = (batch), block = 64
__global__ void __launch_bounds__(64) k_fs_round(const ProductPartial* __restrict__ partials, uint32_t nblk, uint32_t round, uint32_t n,
                                                 const Fr* __restrict__ lambda, const Fr* __restrict__ cts, const Fr* __restrict__ z,
                                                 Fr* __restrict__ s_slot, const Fr* __restrict__ work, size_t work_stride,
                                                 Fr* __restrict__ out_coeffs, uint32_t* __restrict__ out_len, Fr* __restrict__ out_r,
                                                 FixedMul* __restrict__ rtab, Fr* __restrict__ evals, Fr* __restrict__ eq_out) {
    const uint32_t b = blockIdx.x;
    const ProductPartial* p = partials + (size_t)b * nblk * kFsTerms;
    Fr one = fr_zero();
    one.l[0] = 1u;
    Fr c0[3], c1[3], c2[3];   // (thread 0's)
    term_total_coeffs<2>(p, nblk, kFsTerms, 0u, kFsDegree, one, c0);
    term_total_coeffs<2>(p, nblk, kFsTerms, 1u, kFsDegree, one, c1);
    term_total_coeffs<2>(p, nblk, kFsTerms, 2u, kFsDegree, load_fr(lambda + b), c2);
    if (threadIdx.x != 0) return;
    Fr h[3];   // h_j, highest degree first
#pragma unroll
    for (int k = 0; k < 3; ++k) h[k] = fr_add(fr_add(c0[k], c1[k]), c2[k]);
    zc_round_tail(h, b, round, n, kFsTables, kFsDegree, cts, z, s_slot, work, work_stride, out_coeffs, out_len, out_r, rtab, evals, eq_out);
}

}  // namespace

uint32_t fs_level_blocks(uint32_t k) { return blocks_for((uint64_t)1 << k, 0xFFFFFFFFu); }

void launch_fs_tree(const Fr* tables, uint32_t n, uint32_t batch, Fr* layers, hipStream_t s) {
    for (uint32_t k = n; k-- > 0;) {
        const Fr* src = k + 1 == n ? tables : layers + fs_layer_offset(k + 1, batch);
        hipLaunchKernelGGL(k_fs_level, dim3(fs_level_blocks(k), batch), dim3(256), 0, s, src, layers + fs_layer_offset(k, batch), k);
    }
}

void launch_fs_round(const ProductPartial* partials, uint32_t nblk, uint32_t round, uint32_t n, uint32_t batch, const Fr* lambda, const Fr* cts,
                     const Fr* z, Fr* s_slot, const Fr* work, size_t work_stride, Fr* out_coeffs, uint32_t* out_len, Fr* out_r, FixedMul* rtab,
                     Fr* evals, Fr* eq_out, hipStream_t s) {
    hipLaunchKernelGGL(k_fs_round, dim3(batch), dim3(64), 0, s, partials, nblk, round, n, lambda, cts, z, s_slot, work, work_stride, out_coeffs,
                       out_len, out_r, rtab, evals, eq_out);
}

}  // namespace gkr

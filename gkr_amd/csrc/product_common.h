// Device helpers shared by the kernels of the sumchecks over resident tables -- a product (kernels_product.hip), a sum of products
// (kernels_sop.hip), the zero-check (kernels_zerocheck.hip): a block's chunk, the fold of every table of a chunk, what a thread
// accumulates a round polynomial's values in, one index's terms of the D + 1 values, the block's partial, the term structure's
// decoders, and the round kernels' steps: a term's partials -> its scaled coefficients, the length rule, the row with its hash
// and challenge, the tables' values after the last round, and the zero-check's round behind h_j (k_zc_round and
// kernels_fraction_sum.hip's k_fs_round).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "dev_util.h"
#include "mimc7.h"

namespace gkr {

namespace {

// SopTerms::term
__device__ __forceinline__ uint32_t sop_term_degree(uint32_t term) { return term & 0xFFu; }
__device__ __forceinline__ uint32_t sop_term_table(uint32_t term, int j) { return (term >> (8 + 8 * j)) & 0xFFu; }

// this block's entries begin .. end of a pass over `items` per sumcheck, grid.x blocks each: blocked distribution, chunk starts at
// multiples of 256 (see k_mle_sum_first)
__device__ __forceinline__ void block_chunk(uint32_t items, uint32_t& begin, uint32_t& end) {
    const uint32_t chunk = ((items + gridDim.x - 1) / gridDim.x + 255u) & ~255u;
    begin = blockIdx.x * chunk;
    end = begin + chunk < items ? begin + chunk : items;
}

// entries begin .. end of every one of a sumcheck's tables folded ONCE with the round's multiplier T: src 4q entries per table
// -> dst 2q.  src and dst may be the same buffer with equal strides: a thread writes only slots it alone has read.
__device__ __forceinline__ void fold_tables_chunk(const Fr* src, size_t src_stride, Fr* dst, size_t dst_stride, uint32_t n_tables, uint32_t q,
                                                  const FixedMul& T, uint32_t begin, uint32_t end) {
    for (uint32_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
        for (uint32_t m = 0; m < n_tables; ++m) {
            const Fr* sm = src + (size_t)m * src_stride;
            Fr* dm = dst + (size_t)m * dst_stride;
            const Fr x0 = load_fr(sm + i), x1 = load_fr(sm + i + 2 * (size_t)q);
            const Fr x2 = load_fr(sm + i + q), x3 = load_fr(sm + i + 3 * (size_t)q);
            Fr lo, hi;
            fr_fold_fixed2(x0, x1, x2, x3, T, lo, hi);
            store_fr(dm + i, lo);
            store_fr(dm + i + q, hi);
        }
    }
}

// what one thread accumulates a value in: a wide sum of elements at degree 1, a lazy sum of products above
template <int D>
using ProductLane = std::conditional_t<D == 1, Acc<9>, Lazy17>;

template <int D>
__device__ __forceinline__ ProductLane<D> product_lane_zero() {
    if constexpr (D == 1)
        return acc_zero<9>();
    else
        return lazy_zero();
}

// the D + 1 values' terms of one index: lo[f] = T_f[i], hi[f] = T_f[i + h].  Slots: 0 P(0), 1 P(1), 2 P(inf), 3 P(-1).
template <int D>
__device__ __forceinline__ void product_accumulate(ProductLane<D> (&acc)[D + 1], const Fr (&lo)[D], const Fr (&hi)[D]) {
    if constexpr (D == 1) {
        acc_add_fr(acc[0], lo[0]);
        acc_add_fr(acc[1], hi[0]);
    } else if constexpr (D == 2) {
        lazy_mac_v(acc[0], lo[0], lo[1]);
        lazy_mac_v(acc[1], hi[0], hi[1]);
        lazy_mac_v(acc[2], fr_sub(hi[0], lo[0]), fr_sub(hi[1], lo[1]));
    } else {
        static_assert(D == 3, "degree 1 .. 3");
        lazy_mac_v(acc[0], mont_mul(lo[0], lo[1]), lo[2]);
        lazy_mac_v(acc[1], mont_mul(hi[0], hi[1]), hi[2]);
        const Fr d0 = fr_sub(hi[0], lo[0]), d1 = fr_sub(hi[1], lo[1]), d2 = fr_sub(hi[2], lo[2]);
        lazy_mac_v(acc[2], mont_mul(d0, d1), d2);
        lazy_mac_v(acc[3], mont_mul(fr_sub(lo[0], d0), fr_sub(lo[1], d1)), fr_sub(lo[2], d2));   // T_f(-1) = lo - (hi - lo)
    }
}

// the thread's lanes -> one Acc<9> each (the lazy sums reduced once), block total to thread 0, stored as the block's partial
template <int D>
__device__ __forceinline__ void product_store_partial(ProductLane<D> (&lane)[D + 1], Acc<9>* smem, uint32_t flags, ProductPartial* out) {
    Acc<9> acc[D + 1];
#pragma unroll
    for (int k = 0; k <= D; ++k) {
        if constexpr (D == 1) {
            acc[k] = lane[k];
        } else {
            acc[k] = acc_zero<9>();
            acc_add_fr(acc[k], lazy_reduce(lane[k]));
        }
    }
    block_sum<9, D + 1>(acc, smem);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k <= D; ++k) out->s[k] = acc[k];
        out->flags = flags;
    }
}

__device__ __forceinline__ Fr fr_half(const Fr& x) {
    constexpr uint32_t p[8] = GKR_MOD_LIMBS;
    const uint32_t odd = 0u - (x.l[0] & 1u);
    uint32_t s[8];
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // x + p < 2^255: no carry out of the eight limbs
        c += (uint64_t)x.l[i] + (p[i] & odd);
        s[i] = (uint32_t)c;
        c >>= 32;
    }
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; ++i) r.l[i] = (s[i] >> 1) | (i < 7 ? s[i + 1] << 31 : 0u);
    return r;
}

// the D + 1 values (slots as above, the lazy sums' scaling undone) -> the coefficients c_D .. c_0, highest degree first
template <int D>
__device__ __forceinline__ void product_values_to_coeffs(const Fr (&v)[D + 1], Fr (&c)[D + 1]) {
    if constexpr (D == 1) {
        c[0] = fr_sub(v[1], v[0]);
        c[1] = v[0];
    } else if constexpr (D == 2) {
        c[0] = v[2];
        c[1] = fr_sub(fr_sub(v[1], v[0]), v[2]);
        c[2] = v[0];
    } else {
        static_assert(D == 3, "degree 1 .. 3");
        const Fr c2 = fr_sub(fr_half(fr_add(v[1], v[3])), v[0]);   // (P(1) + P(-1)) / 2 = c_2 + c_0
        c[0] = v[2];
        c[1] = c2;
        c[2] = fr_sub(fr_sub(fr_sub(v[1], v[0]), c2), v[2]);
        c[3] = v[0];
    }
}

// the same into V >= D + 1 slots, right-aligned: zeros in front
template <int D, int V>
__device__ __forceinline__ void product_values_to_coeffs_right(const Fr (&v)[V], Fr (&c)[V]) {
    if constexpr (V == D + 1) {
        product_values_to_coeffs<D>(v, c);
    } else {
        Fr vd[D + 1], cd[D + 1];
#pragma unroll
        for (int k = 0; k <= D; ++k) vd[k] = v[k];
        product_values_to_coeffs<D>(vd, cd);
#pragma unroll
        for (int k = 0; k < V; ++k) c[k] = k < V - D - 1 ? fr_zero() : cd[k - (V - D - 1)];
    }
}

// ---- the round kernels' steps (one wave per sumcheck and round)

// One term of a sum of products with term degrees <= MAXD: the blocks' partials of term t (degree d) of this sumcheck (p: block
// 0's, K terms per block) totalled over the wave, the 2^(-256 (d - 1)) of the lazy and Montgomery reductions undone, values ->
// coefficients, times c_k: thread 0's out, right-aligned in MAXD + 1 slots (highest degree first).  The other threads' is not set.
template <int MAXD>
__device__ __forceinline__ void term_total_coeffs(const ProductPartial* p, uint32_t nblk, uint32_t K, uint32_t t, uint32_t d, const Fr& ck,
                                                  Fr (&out)[MAXD + 1]) {
    static_assert(MAXD == 2 || MAXD == 3, "the zero-check's inner degree or the product path's");
    constexpr int V = MAXD + 1;
    Acc<10> tot[V];
#pragma unroll
    for (int k = 0; k < V; ++k) tot[k] = acc_zero<10>();
    for (uint32_t i = threadIdx.x; i < nblk; i += 64) {
        const ProductPartial* pp = p + (size_t)i * K + t;
#pragma unroll
        for (int k = 0; k < V; ++k)
            if ((uint32_t)k <= d) acc_add_acc(tot[k], pp->s[k]);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) tot[k] = wave_sum(tot[k]);
    if (threadIdx.x != 0) return;
    Fr v[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
        v[k] = acc_reduce(tot[k]);
#pragma unroll
        for (int m = 1; m < MAXD; ++m)
            if ((uint32_t)m < d) v[k] = mont_mul(v[k], fr_r2());   // x 2^256 per lazy or Montgomery reduction taken
    }
    Fr c[V];
    if (d == 1)
        product_values_to_coeffs_right<1>(v, c);
    else if (MAXD == 2 || d == 2)
        product_values_to_coeffs_right<2>(v, c);
    else if constexpr (MAXD == 3)
        product_values_to_coeffs_right<3>(v, c);
    const Fr ck_mont = to_mont(ck);
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = mont_mul(c[k], ck_mont);
}

// every term's, added up: thread 0's sum
template <int MAXD>
__device__ __forceinline__ void terms_total(const ProductPartial* p, uint32_t nblk, const SopTerms& ts, const SopCoeffs& cf, Fr (&sum)[MAXD + 1]) {
#pragma unroll
    for (int k = 0; k <= MAXD; ++k) sum[k] = fr_zero();
    for (uint32_t t = 0; t < ts.n_terms; ++t) {
        Fr c[MAXD + 1];
        term_total_coeffs<MAXD>(p, nblk, ts.n_terms, t, sop_term_degree(ts.term[t]), cf.c[t], c);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int k = 0; k <= MAXD; ++k) sum[k] = fr_add(sum[k], c[k]);
        }
    }
}

// the length rule of a merged polynomial (add_poly merges by exponent and drops zero sums, poly.rs:324-327): leading zero
// coefficients dropped, one kept at least.  sum: S coefficients, highest degree first.
template <int S>
__device__ __forceinline__ uint32_t round_length(const Fr (&sum)[S]) {
    uint32_t lead = 0;
    bool leading = true;
#pragma unroll
    for (int k = 0; k < S - 1; ++k) {
        leading = leading && fr_is_zero(sum[k]);
        lead += leading ? 1u : 0u;
    }
    return (uint32_t)S - lead;
}

// Thread 0 publishes a round: the last D + 1 <= S of the slots (right-aligned; the ones in front hold zero) to the row, the row's
// length, and r = multi_hash(the last len slots, key 0) as mimc7_multi_hash does it -- the slots indexed statically (no private
// array in memory).  Returns r (canonical).
template <int S>
__device__ __forceinline__ Fr round_publish(const Fr (&sum)[S], uint32_t len, uint32_t D, size_t row, const Fr* __restrict__ cts,
                                            Fr* __restrict__ out_coeffs, uint32_t* __restrict__ out_len, Fr* __restrict__ out_r) {
    Fr* oc = out_coeffs + row * (D + 1);
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
    return r;
}

// after round n, the last fold of every table's two remaining entries: evals[b M + m] = T_m~(r_1 .. r_n)
__device__ __forceinline__ void fold_last_entries(const Fr* __restrict__ work, size_t work_stride, uint32_t b, uint32_t n_tables,
                                                  const Fr& r_mont, Fr* __restrict__ evals) {
    for (uint32_t m = 0; m < n_tables; ++m) {
        const Fr* t = work + ((size_t)b * n_tables + m) * work_stride;
        evals[(size_t)b * n_tables + m] = fr_fold(t[0], t[1], r_mont);
    }
}

// The zero-check's round behind h_j (thread 0 alone; h: three coefficients, highest degree first, Montgomery), shared by
// k_zc_round and k_fs_round: g_j = (a + b X) h_j with a = s_j (1 - z_j), b = s_j (2 z_j - 1), the length rule, the row with its hash
// and challenge, s_{j+1} = a + b r_j to s_slot[b] (Montgomery) and r as the next fold's multiplier table; behind round n the
// tables' last values and eq_out[b] = eq(z, r) instead.  Rows have max_degree + 2 slots.
__device__ __forceinline__ void zc_round_tail(const Fr (&h)[3], uint32_t b, uint32_t round, uint32_t n, uint32_t n_tables, uint32_t max_degree,
                                              const Fr* __restrict__ cts, const Fr* __restrict__ z, Fr* __restrict__ s_slot,
                                              const Fr* __restrict__ work, size_t work_stride, Fr* __restrict__ out_coeffs,
                                              uint32_t* __restrict__ out_len, Fr* __restrict__ out_r, FixedMul* __restrict__ rtab,
                                              Fr* __restrict__ evals, Fr* __restrict__ eq_out) {
    constexpr int S = 4;
    // the linear factor of the round's own variable times the bound variables' scalar, in Montgomery form
    const Fr zj = load_fr(z + (size_t)b * n + round);
    Fr one = fr_zero();
    one.l[0] = 1u;
    const Fr s_j = round == 0 ? fr_mont_one() : load_fr(s_slot + b);
    const Fr fa = mont_mul(to_mont(fr_sub(one, zj)), s_j);                    // s_j (1 - z_j)
    const Fr fb = mont_mul(to_mont(fr_sub(fr_add(zj, zj), one)), s_j);        // s_j (2 z_j - 1)
    Fr sum[S];   // g_j = (fa + fb X) h_j, highest degree first
    sum[0] = mont_mul(h[0], fb);
    sum[1] = fr_add(mont_mul(h[0], fa), mont_mul(h[1], fb));
    sum[2] = fr_add(mont_mul(h[1], fa), mont_mul(h[2], fb));
    sum[3] = mont_mul(h[2], fa);
    const size_t row = (size_t)b * n + round;
    const Fr r = round_publish<S>(sum, round_length<S>(sum), max_degree + 1u, row, cts, out_coeffs, out_len, out_r);
    const Fr r_mont = to_mont(r);
    const Fr s_next = fr_add(fa, mont_mul(fb, r_mont));   // s_j eq(z_j, r_j)
    if (round + 1 < n) {
        store_fixed_mul(rtab + row, r);
        store_fr(s_slot + b, s_next);
    } else {
        fold_last_entries(work, work_stride, b, n_tables, r_mont, evals);
        store_fr(eq_out + b, from_mont(s_next));
    }
}

}  // namespace

}  // namespace gkr

// Device helpers shared by the kernels of the sumcheck over a product of resident tables (kernels_product.hip) and over a sum of
// such products (kernels_sop.hip): what a thread accumulates a round polynomial's values in, one index's terms of the D + 1
// values, the block's partial, and the values -> coefficients step of the round kernels.  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kernels.h"
#include "dev_util.h"

namespace gkr {

namespace {

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

}  // namespace

}  // namespace gkr

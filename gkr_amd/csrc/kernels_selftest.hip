// Device unit tests of the field arithmetic (C ABI gkr_devtest_*, include/gkr_amd.h).  Each entry point copies the caller's
// inputs to the device, runs ONE small kernel that calls the production inline functions themselves -- the gfx950 forms of
// fr32.h, the lane MiMC of mimc_lanes.h, the short reductions of mfma_fold.h / mfma_cross.h -- and copies the results back.
// Nothing is re-implemented here.  Sumcheck parity on random tables reaches a carry or borrow edge with probability ~2^-32
// per operation; these entry points let a test put a limb exactly on it.  Inputs outside a primitive's stated bound are
// rejected on the host (GKR_ERR_INVALID), never run.
#include "capi_internal.h"
#include "mfma_cross.h"
#include "mfma_fold.h"
#include "mimc_lanes.h"

namespace gkr {
namespace {

// ---------------------------------------------------------------- one element per thread
// Operands the production code takes wave-uniform (the FixedMul table, the `_s` multipliers) are read per wave
// (block = 64 threads): index blockIdx.x.
__global__ void __launch_bounds__(64) k_devtest_field(int op, const Fr* __restrict__ a, const Fr* __restrict__ b,
                                                      const Fr* __restrict__ r, uint32_t n, Fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool live = i < n;
    const uint32_t k = live ? i : n - 1u;   // (a lane past the end repeats the last element and stores nothing)
    const Fr x = load_fr(&a[k]), y = load_fr(&b[k]);
    Fr o = fr_zero(), o2 = fr_zero();
    switch (op) {
        case GKR_DEVTEST_FR_ADD: o = fr_add(x, y); break;
        case GKR_DEVTEST_FR_SUB: o = fr_sub(x, y); break;
        case GKR_DEVTEST_MONT_MUL: o = mont_mul(x, y); break;
        case GKR_DEVTEST_FR_MUL: o = fr_mul(x, y); break;
        case GKR_DEVTEST_TO_MONT: o = to_mont(x); break;
        case GKR_DEVTEST_FROM_MONT: o = from_mont(x); break;
        default: {
            const FixedMul T = make_fixed_mul(r[blockIdx.x]);
            if (op == GKR_DEVTEST_MUL_FIXED) o = mul_fixed(x, T);
            else if (op == GKR_DEVTEST_MUL_FIXED2) mul_fixed2(x, y, T, o, o2);
            else if (op == GKR_DEVTEST_FOLD_FIXED) o = fr_fold_fixed(x, y, T);
            else fr_fold_fixed2(x, y, y, x, T, o, o2);
        }
    }
    if (live) {
        store_fr(&out[i], o);
        if (op == GKR_DEVTEST_MUL_FIXED2 || op == GKR_DEVTEST_FOLD_FIXED2) store_fr(&out[n + i], o2);
    }
}

// ---------------------------------------------------------------- one dot product per thread
template <typename Red>
__device__ __forceinline__ void devtest_lazy_row(int op, const Fr* __restrict__ a, const Fr* __restrict__ bv,
                                                 const Fr* __restrict__ u, uint32_t row, uint32_t len, Fr (&o)[4], Red red) {
    Lazy17 A = lazy_zero(), B = lazy_zero(), C = lazy_zero(), D = lazy_zero();
    switch (op) {
        case GKR_DEVTEST_LAZY_MAC_S:
            for (uint32_t t = 0; t < len; ++t) lazy_mac_s(A, load_fr(&a[t]), u[t]);
            break;
        case GKR_DEVTEST_LAZY_MAC_V:
            for (uint32_t t = 0; t < len; ++t) lazy_mac_v(A, load_fr(&a[t]), load_fr(&bv[t]));
            break;
        case GKR_DEVTEST_LAZY_MAC_SEL:   // term t goes to A iff (row + t) % 3 != 0
            for (uint32_t t = 0; t < len; ++t) lazy_mac_sel(A, B, (row + t) % 3u != 0u, load_fr(&a[t]), load_fr(&bv[t]));
            break;
        case GKR_DEVTEST_LAZY_MAC_V_HI:  // + a_t * 2^256 where (row + t) is odd
            for (uint32_t t = 0; t < len; ++t) {
                const Fr x = load_fr(&a[t]);
                lazy_mac_v(A, x, load_fr(&bv[t]));
                lazy_add_hi(A, x, ((row + t) & 1u) != 0u);
            }
            break;
        // chains c = 0 .. C-1 advanced together: chain c is sum_t a_t * u_{(t + c) % len}
        case GKR_DEVTEST_LAZY_MAC2_S:
            for (uint32_t t = 0; t < len; ++t) {
                const Fr x = load_fr(&a[t]);
                lazy_mac2_s(A, x, u[t], B, x, u[(t + 1u) % len]);
            }
            break;
        case GKR_DEVTEST_LAZY_MAC3_S:
            for (uint32_t t = 0; t < len; ++t) {
                const Fr x = load_fr(&a[t]);
                lazy_mac3_s(A, x, u[t], B, x, u[(t + 1u) % len], C, x, u[(t + 2u) % len]);
            }
            break;
        case GKR_DEVTEST_LAZY_MAC4_S:
            for (uint32_t t = 0; t < len; ++t) {
                const Fr x = load_fr(&a[t]);
                lazy_mac4_s(A, x, u[t], B, x, u[(t + 1u) % len], C, x, u[(t + 2u) % len], D, x, u[(t + 3u) % len]);
            }
            break;
        case GKR_DEVTEST_WEIGHTED_SUM_4: {
            Fr x[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) x[t] = load_fr(&a[t]);
            weighted_sum_s<4>(x, u, A);
            break;
        }
        case GKR_DEVTEST_WEIGHTED_SUM_8: {
            Fr x[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) x[t] = load_fr(&a[t]);
            weighted_sum_s<8>(x, u, A);
            break;
        }
        default: {   // GKR_DEVTEST_ACC_SUM: sum_t a_t through the 288-bit accumulator
            Acc<9> s = acc_zero<9>();
            for (uint32_t t = 0; t < len; ++t) acc_add_fr(s, load_fr(&a[t]));
            o[0] = acc_reduce(s);
            return;
        }
    }
    o[0] = red(A);
    o[1] = red(B);
    o[2] = red(C);
    o[3] = red(D);
}

__global__ void __launch_bounds__(64) k_devtest_lazy(int op, int red, const Fr* __restrict__ a, const Fr* __restrict__ b,
                                                     uint32_t rows, uint32_t len, Fr* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    const bool live = i < rows;
    const uint32_t row = live ? i : rows - 1u;
    const Fr* ar = a + (size_t)row * len;
    const Fr* bv = b + (size_t)row * len;           // per-row multipliers (_v, _sel, _v_hi)
    const Fr* u = b + (size_t)blockIdx.x * len;      // per-wave multipliers (_s, weighted_sum)
    Fr o[4];
    if (red == GKR_DEVTEST_RED_K8) devtest_lazy_row(op, ar, bv, u, row, len, o, [](const Lazy17& x) { return lazy_reduce_k8(x); });
    else if (red == GKR_DEVTEST_RED_PARTIAL32) devtest_lazy_row(op, ar, bv, u, row, len, o, [](const Lazy17& x) { return lazy_reduce_partial32(x); });
    else devtest_lazy_row(op, ar, bv, u, row, len, o, [](const Lazy17& x) { return lazy_reduce(x); });
    if (live) {
        const int used = op == GKR_DEVTEST_ACC_SUM ? 1 : 4;
        for (int c = 0; c < 4; ++c) store_fr(&out[(size_t)i * 4u + c], c < used ? o[c] : fr_zero());
    }
}

// ---------------------------------------------------------------- raw limbs in and out, one element per thread
__global__ void __launch_bounds__(64) k_devtest_reduce(int op, const uint32_t* __restrict__ in, uint32_t n, uint32_t sin,
                                                       uint32_t sout, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const uint32_t* x = in + (size_t)i * sin;
    uint32_t* y = out + (size_t)i * sout;
    switch (op) {
        case GKR_DEVTEST_MF_REDUCE_274: {
            uint32_t l[9];
            for (int k = 0; k < 9; ++k) l[k] = x[k];
            const Fr r = mf_reduce_274(l);
            for (int k = 0; k < 8; ++k) y[k] = r.l[k];
            break;
        }
        case GKR_DEVTEST_CROSS_REDUCE:
        case GKR_DEVTEST_LAZY_REDUCE:
        case GKR_DEVTEST_LAZY_REDUCE_K8:
        case GKR_DEVTEST_LAZY_REDUCE_PARTIAL32: {
            Lazy17 v;
            for (int k = 0; k < 17; ++k) v.l[k] = x[k];
            const Fr r = op == GKR_DEVTEST_CROSS_REDUCE ? cross_reduce(v)
                         : op == GKR_DEVTEST_LAZY_REDUCE ? lazy_reduce(v)
                         : op == GKR_DEVTEST_LAZY_REDUCE_K8 ? lazy_reduce_k8(v)
                                                             : lazy_reduce_partial32(v);
            for (int k = 0; k < 8; ++k) y[k] = r.l[k];
            break;
        }
        case GKR_DEVTEST_LAZY_ADD_HI: {   // in: acc (17 limbs), x (8), on (1)
            Lazy17 v;
            Fr f;
            for (int k = 0; k < 17; ++k) v.l[k] = x[k];
            for (int k = 0; k < 8; ++k) f.l[k] = x[17 + k];
            lazy_add_hi(v, f, x[25] != 0u);
            for (int k = 0; k < 17; ++k) y[k] = v.l[k];
            break;
        }
        case GKR_DEVTEST_ACC_ADD_FR9: {   // in: acc (9 limbs), x (8)
            Acc<9> s;
            Fr f;
            for (int k = 0; k < 9; ++k) s.l[k] = x[k];
            for (int k = 0; k < 8; ++k) f.l[k] = x[9 + k];
            acc_add_fr(s, f);
            for (int k = 0; k < 9; ++k) y[k] = s.l[k];
            break;
        }
        case GKR_DEVTEST_ACC_REDUCE9: {
            Acc<9> s;
            for (int k = 0; k < 9; ++k) s.l[k] = x[k];
            const Fr r = acc_reduce(s);
            for (int k = 0; k < 8; ++k) y[k] = r.l[k];
            break;
        }
        case GKR_DEVTEST_ADD256:
        case GKR_DEVTEST_SUB256: {   // in: a (8 limbs), b (8); sub256 also writes its borrow mask (limb 8)
            uint32_t p[8], q[8], o[8], bm = 0;
            for (int k = 0; k < 8; ++k) {
                p[k] = x[k];
                q[k] = x[8 + k];
            }
            if (op == GKR_DEVTEST_ADD256) add256(o, p, q);
            else sub256(o, bm, p, q);
            for (int k = 0; k < 8; ++k) y[k] = o[k];
            if (op == GKR_DEVTEST_SUB256) y[8] = bm;
            break;
        }
        default: {   // GKR_DEVTEST_COND_SUB_MOD
            uint32_t s[8];
            for (int k = 0; k < 8; ++k) s[k] = x[k];
            const Fr r = cond_sub_mod(s);
            for (int k = 0; k < 8; ++k) y[k] = r.l[k];
        }
    }
}

// ---------------------------------------------------------------- eight lanes per element (mimc_lanes.h)
// The layout of k_mle_pass_hash_lanes: block = 64, group g of eight lanes (limb j in lane j) = element blockIdx.x * 8 + g;
// a group past the end repeats the last element and stores nothing.  GROUP_SUM: every lane holds a whole value
// (x[8 * element + j]) and every lane's result is stored.
__global__ void __launch_bounds__(64) k_devtest_lanes(int op, const Fr* __restrict__ xs, const Fr* __restrict__ ys,
                                                      const Fr* __restrict__ zs, uint32_t count, const Fr* __restrict__ cts,
                                                      Fr* __restrict__ out) {
    const lanes::Ctx c = lanes::make_ctx();
    const uint32_t grp = (threadIdx.x & 63u) >> 3, j = c.j;
    const uint32_t e_raw = blockIdx.x * 8u + grp;
    const bool live = e_raw < count;
    const uint32_t e = live ? e_raw : count - 1u;
    if (op == GKR_DEVTEST_LANES_GROUP_SUM) {
        const Fr s = group_sum(load_fr(&xs[(size_t)e * 8u + j]));
        if (live) store_fr(&out[(size_t)e * 8u + j], s);
        return;
    }
    const uint32_t x = xs[e].l[j], y = ys ? ys[e].l[j] : 0u, z = zs ? zs[e].l[j] : 0u;
    uint32_t r = 0;
    switch (op) {
        case GKR_DEVTEST_LANES_MONT_MUL: r = lanes::mont_mul(x, y, c); break;
        case GKR_DEVTEST_LANES_ADD3: r = lanes::add3(x, y, z, c); break;
        case GKR_DEVTEST_LANES_COND_SUB_P: r = lanes::cond_sub(x, c.pj, c); break;
        case GKR_DEVTEST_LANES_COND_SUB_2P: r = lanes::cond_sub(x, c.two_pj, c); break;
        case GKR_DEVTEST_LANES_RESOLVE: r = lanes::resolve_carries((uint64_t)x | ((uint64_t)y << 32), j); break;
        case GKR_DEVTEST_LANES_PERMUTATION: r = lanes::permutation(x, y, cts, c); break;
        default: {   // GKR_DEVTEST_LANES_MULTI_HASH1 .. 3: multi_hash(x[, y[, z]], 0)
            const int len = op - GKR_DEVTEST_LANES_MULTI_HASH1 + 1;
            r = lanes::multi_hash(len, [&](int t) { return t == 0 ? x : (t == 1 ? y : z); }, cts, c);
        }
    }
    if (live) out[e].l[j] = r;
}

}  // namespace
}  // namespace gkr

namespace gkr_host {
namespace {

// a < b over n little-endian limbs
bool limbs_less(const uint32_t* a, const uint32_t* b, int n) {
    for (int i = n - 1; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}

// out (n + 1 limbs) = a (n limbs) * k
void limbs_mul_small(const uint32_t* a, int n, uint32_t k, uint32_t* out) {
    uint64_t c = 0;
    for (int i = 0; i < n; ++i) {
        c += (uint64_t)a[i] * k;
        out[i] = (uint32_t)c;
        c >>= 32;
    }
    out[n] = (uint32_t)c;
}

// out (17 limbs) = k * p^2
void k_p_squared(uint32_t k, uint32_t (&out)[17]) {
    constexpr uint32_t p[8] = GKR_MOD_LIMBS;
    uint32_t sq[17] = {0};
    for (int i = 0; i < 8; ++i) {
        uint64_t c = 0;
        for (int j = 0; j < 8; ++j) {
            c += (uint64_t)sq[i + j] + (uint64_t)p[i] * p[j];
            sq[i + j] = (uint32_t)c;
            c >>= 32;
        }
        sq[i + 8] = (uint32_t)c;
    }
    uint32_t t[18];
    limbs_mul_small(sq, 17, k, t);
    for (int i = 0; i < 17; ++i) out[i] = t[i];   // (k <= 32: t[17] == 0)
}

// every Fr of v (n of them) below k * p
bool all_below_kp(const gkr_fr* v, size_t n, uint32_t k) {
    constexpr uint32_t p[8] = GKR_MOD_LIMBS;
    uint32_t kp[9];
    limbs_mul_small(p, 8, k, kp);
    for (size_t i = 0; i < n; ++i) {
        uint32_t x[9];
        memcpy(x, &v[i], 32);
        x[8] = 0;
        if (!limbs_less(x, kp, 9)) return false;
    }
    return true;
}

// copy in, run, copy out: the inputs' device copies and the output buffer live for one call
struct DevtestBufs {
    DevBuf<unsigned char> in[3];
    DevBuf<unsigned char> out;
};

}  // namespace
}  // namespace gkr_host

extern "C" {

int gkr_devtest_field(gkr_ctx* ctx, int op, const gkr_fr* a, const gkr_fr* b, const gkr_fr* r, size_t n, gkr_fr* out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (op < 0 || op > GKR_DEVTEST_FOLD_FIXED2 || !a || !b || !out || n < 1 || n > ((size_t)1 << 24))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_field: bad arguments");
    const size_t waves = (n + 63) / 64;
    const bool fixed = op >= GKR_DEVTEST_MUL_FIXED;
    if (fixed && !r) return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_field: the fixed-multiplier ops need r");
    // mont_mul's inputs may be any values below p (Montgomery or not); every op takes canonical operands
    if (!all_canonical(a, n) || !all_canonical(b, n) || (fixed && !all_canonical(r, waves)))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_field: operands must be canonical");
    const bool two = op == GKR_DEVTEST_MUL_FIXED2 || op == GKR_DEVTEST_FOLD_FIXED2;
    GKR_ENTER(ctx);
    DevtestBufs B;
    HIP_TRY(ctx, B.in[0].alloc(n * 32));
    HIP_TRY(ctx, B.in[1].alloc(n * 32));
    HIP_TRY(ctx, B.in[2].alloc(waves * 32));
    HIP_TRY(ctx, B.out.alloc((two ? 2 : 1) * n * 32));
    HIP_TRY(ctx, hipMemcpyAsync(B.in[0].p, a, n * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(B.in[1].p, b, n * 32, hipMemcpyHostToDevice, ctx->stream));
    if (fixed) HIP_TRY(ctx, hipMemcpyAsync(B.in[2].p, r, waves * 32, hipMemcpyHostToDevice, ctx->stream));
    else HIP_TRY(ctx, hipMemsetAsync(B.in[2].p, 0, waves * 32, ctx->stream));
    hipLaunchKernelGGL(gkr::k_devtest_field, dim3((unsigned)waves), dim3(64), 0, ctx->stream, op, reinterpret_cast<const Fr*>(B.in[0].p),
                       reinterpret_cast<const Fr*>(B.in[1].p), reinterpret_cast<const Fr*>(B.in[2].p), (uint32_t)n, reinterpret_cast<Fr*>(B.out.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, B.out.p, (two ? 2 : 1) * n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

int gkr_devtest_lazy(gkr_ctx* ctx, int op, int red, const gkr_fr* a, const gkr_fr* b, size_t rows, size_t len, gkr_fr* out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (op < 0 || op > GKR_DEVTEST_ACC_SUM || red < 0 || red > GKR_DEVTEST_RED_PARTIAL32 || !a || !out || rows < 1 ||
        rows > ((size_t)1 << 20) || len < 1 || len > 4096 || rows * len > ((size_t)1 << 22) || (op != GKR_DEVTEST_ACC_SUM && !b))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lazy: bad arguments");
    if ((op == GKR_DEVTEST_WEIGHTED_SUM_4 && len != 4) || (op == GKR_DEVTEST_WEIGHTED_SUM_8 && len != 8))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lazy: weighted_sum_s takes exactly 4 / 8 terms");
    const size_t waves = (rows + 63) / 64;
    const bool uniform = op == GKR_DEVTEST_LAZY_MAC_S || (op >= GKR_DEVTEST_LAZY_MAC2_S && op <= GKR_DEVTEST_WEIGHTED_SUM_8);
    const size_t nb = op == GKR_DEVTEST_ACC_SUM ? 0 : (uniform ? waves : rows) * len;
    // the reductions' bounds: lazy_reduce_k8 at most eight products, lazy_reduce_partial32 at most 32 terms (a product or a
    // value times 2^256 -- what lazy_add_hi adds), lazy_reduce / acc_reduce far more than a call can hold
    if (red == GKR_DEVTEST_RED_K8 && (len > 8 || op == GKR_DEVTEST_LAZY_MAC_V_HI))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lazy: lazy_reduce_k8 takes at most eight products");
    if (red == GKR_DEVTEST_RED_PARTIAL32 && (op == GKR_DEVTEST_LAZY_MAC_V_HI ? 2 * len : len) > 32)
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lazy: lazy_reduce_partial32 takes at most 32 terms");
    if (!all_canonical(a, rows * len) || !all_canonical(b, nb))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lazy: operands must be canonical");
    GKR_ENTER(ctx);
    DevtestBufs B;
    HIP_TRY(ctx, B.in[0].alloc(rows * len * 32));
    HIP_TRY(ctx, B.in[1].alloc((nb > rows * len ? nb : rows * len) * 32));
    HIP_TRY(ctx, B.out.alloc(rows * 4 * 32));
    HIP_TRY(ctx, hipMemcpyAsync(B.in[0].p, a, rows * len * 32, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(B.in[1].p, 0, rows * len * 32, ctx->stream));
    if (nb) HIP_TRY(ctx, hipMemcpyAsync(B.in[1].p, b, nb * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(gkr::k_devtest_lazy, dim3((unsigned)waves), dim3(64), 0, ctx->stream, op, red, reinterpret_cast<const Fr*>(B.in[0].p),
                       reinterpret_cast<const Fr*>(B.in[1].p), (uint32_t)rows, (uint32_t)len, reinterpret_cast<Fr*>(B.out.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, B.out.p, rows * 4 * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

int gkr_devtest_reduce(gkr_ctx* ctx, int op, const uint32_t* limbs, size_t n, uint32_t* out) {
    static const uint32_t kIn[] = {9, 17, 17, 17, 17, 26, 17, 9, 16, 16, 8};
    static const uint32_t kOut[] = {8, 8, 8, 8, 8, 17, 9, 8, 8, 9, 8};
    if (!ctx) return GKR_ERR_INVALID;
    if (op < 0 || op > GKR_DEVTEST_COND_SUB_MOD || !limbs || !out || n < 1 || n > ((size_t)1 << 20))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_reduce: bad arguments");
    const uint32_t sin = kIn[op], sout = kOut[op];
    constexpr uint32_t p[8] = GKR_MOD_LIMBS;
    uint32_t bound[17], p32[9], p2[9];
    k_p_squared(8, bound);
    limbs_mul_small(p, 8, 32, p32);
    limbs_mul_small(p, 8, 2, p2);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t* x = limbs + i * sin;
        bool ok = true;
        switch (op) {
            case GKR_DEVTEST_MF_REDUCE_274: ok = x[8] < (1u << 18); break;                   // x < 2^274
            case GKR_DEVTEST_CROSS_REDUCE: ok = x[16] < (1u << 7); break;                    // x < 2^519 > 2^11 p^2
            case GKR_DEVTEST_LAZY_REDUCE_K8: ok = limbs_less(x, bound, 17); break;           // x < 8 p^2
            case GKR_DEVTEST_LAZY_REDUCE_PARTIAL32: ok = limbs_less(x + 8, p32, 9); break;   // x < 32 p 2^256
            case GKR_DEVTEST_LAZY_ADD_HI: ok = limbs_less(x + 17, p, 8); break;             // the addend below p
            case GKR_DEVTEST_ACC_ADD_FR9: ok = limbs_less(x + 9, p, 8); break;              // a canonical addend
            case GKR_DEVTEST_COND_SUB_MOD: {                                                 // s < 2p
                uint32_t s[9];
                memcpy(s, x, 32);
                s[8] = 0;
                ok = limbs_less(s, p2, 9);
                break;
            }
            default: break;   // lazy_reduce, acc_reduce<9>, add256, sub256: any value
        }
        if (!ok) return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_reduce: input outside the primitive's bound");
    }
    GKR_ENTER(ctx);
    DevtestBufs B;
    HIP_TRY(ctx, B.in[0].alloc(n * sin * 4));
    HIP_TRY(ctx, B.out.alloc(n * sout * 4));
    HIP_TRY(ctx, hipMemcpyAsync(B.in[0].p, limbs, n * sin * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(gkr::k_devtest_reduce, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, op,
                       reinterpret_cast<const uint32_t*>(B.in[0].p), (uint32_t)n, sin, sout, reinterpret_cast<uint32_t*>(B.out.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, B.out.p, n * sout * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

int gkr_devtest_lanes(gkr_ctx* ctx, int op, const gkr_fr* x, const gkr_fr* y, const gkr_fr* z, size_t n, gkr_fr* out) {
    if (!ctx) return GKR_ERR_INVALID;
    if (op < 0 || op > GKR_DEVTEST_LANES_GROUP_SUM || !x || !out || n < 1 || n > ((size_t)1 << 20))
        return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lanes: bad arguments");
    const bool group_sum = op == GKR_DEVTEST_LANES_GROUP_SUM;
    const bool needs_y = !group_sum && op != GKR_DEVTEST_LANES_COND_SUB_P && op != GKR_DEVTEST_LANES_COND_SUB_2P && op != GKR_DEVTEST_LANES_MULTI_HASH1;
    const bool needs_z = op == GKR_DEVTEST_LANES_ADD3 || op == GKR_DEVTEST_LANES_MULTI_HASH3;
    if ((needs_y && !y) || (needs_z && !z)) return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lanes: missing operand");
    if (!needs_y) y = nullptr;
    if (!needs_z) z = nullptr;
    const size_t nx = group_sum ? 8 * n : n;
    // the bounds of mimc_lanes.h: products of operands below 3p, sums below 2^256, hash inputs below p
    bool ok = true;
    switch (op) {
        case GKR_DEVTEST_LANES_MONT_MUL: ok = all_below_kp(x, n, 3) && all_below_kp(y, n, 3); break;
        case GKR_DEVTEST_LANES_ADD3:
        case GKR_DEVTEST_LANES_RESOLVE:
            for (size_t i = 0; i < n && ok; ++i) {   // x + y + z (RESOLVE: x + y * 2^32, y the lanes' carries) below 2^256
                uint32_t a[8], b[8], c[8] = {0};
                memcpy(a, &x[i], 32);
                memcpy(b, &y[i], 32);
                if (z) memcpy(c, &z[i], 32);
                uint64_t s = 0;
                for (int k = 0; k < 8; ++k) {
                    s += (uint64_t)a[k] + (z ? (uint64_t)b[k] + c[k] : (k ? (uint64_t)b[k - 1] : 0u));
                    s >>= 32;
                }
                if (!z) s += b[7];
                ok = s == 0;
            }
            break;
        case GKR_DEVTEST_LANES_COND_SUB_P:
        case GKR_DEVTEST_LANES_COND_SUB_2P: break;   // any 256-bit value
        default: ok = all_canonical(x, nx) && (!y || all_canonical(y, n)) && (!z || all_canonical(z, n));   // hashes, group_sum
    }
    if (!ok) return ctx->fail(GKR_ERR_INVALID, "gkr_devtest_lanes: input outside the primitive's bound");
    GKR_ENTER(ctx);
    DevtestBufs B;
    const gkr_fr* src[3] = {x, y, z};
    for (int k = 0; k < 3; ++k) {
        if (k && !src[k]) continue;
        const size_t cnt = k ? n : nx;
        HIP_TRY(ctx, B.in[k].alloc(cnt * 32));
        HIP_TRY(ctx, hipMemcpyAsync(B.in[k].p, src[k], cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    HIP_TRY(ctx, B.out.alloc(nx * 32));
    hipLaunchKernelGGL(gkr::k_devtest_lanes, dim3((unsigned)((n + 7) / 8)), dim3(64), 0, ctx->stream, op, reinterpret_cast<const Fr*>(B.in[0].p),
                       reinterpret_cast<const Fr*>(B.in[1].p), reinterpret_cast<const Fr*>(B.in[2].p), (uint32_t)n, ctx->d_cts,
                       reinterpret_cast<Fr*>(B.out.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, B.out.p, nx * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GKR_OK;
}

}  // extern "C"

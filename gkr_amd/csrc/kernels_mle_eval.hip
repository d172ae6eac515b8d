// The multilinear extension of a resident table at ONE point, in one read of the table (gkr_mle_eval_batch_device, and the
// last relation of gkr_sumcheck_mle_verify_batch_device: g_n(r_n) = T(r_1 .. r_n)):
//
//     T(r) = sum_i eq(r, i) T[i],      eq(r, i) = prod_j (bit_j(i) ? r_j : 1 - r_j),  variable 1 = most significant index bit.
//
// A prover's pass writes a folded table for the next pass; a verifier needs one value, so nothing is written here.
//
//   k_mle_eval_mfma   tables of 2^11 entries and more.  The five leading variables are bound on the matrix cores exactly as a
//                     prover's fold pass binds them (mfma_fold.h: the plan of the weights eq((r_1..r_5), b), 32 streams of
//                     stride S = 2^(n-5), non-temporal loads, two staging buffers) -- the SAME code, mfma_multifold_stream, with
//                     another sink: where the fold stores its output y = T'[i], this kernel accumulates y eq((r_6..r_n), i).
//                     A wave turns 64 consecutive outputs per iteration, lane l always the output e0 + l with e0 a multiple of
//                     64, so the weight splits into a WAVE-UNIFORM factor and a factor that is constant per lane:
//                         eq((r_6..r_n), i) = E_up[i >> 6] * E_63[i & 63],
//                     E_up over the n - 11 variables in the middle (2^(n-11) entries per table: 1/2048 of the table's size),
//                     E_63 over the last six.  Per output: ONE unreduced 256 x 256 multiply-add with a scalar operand
//                     (lazy_mac_s, 64 v_mad_u64_u32) beside the fold's ~250 VALU instructions; per lane and BLOCK: one
//                     reduction and one product with E_63[lane].  (Split at the middle of the n - 5 variables instead, a run of
//                     constant i >> lo is shorter than the 256 outputs a block turns per iteration up to n = 21: every output
//                     would pay the reduction and the second product, ~1000 instructions.)  Output: one Acc<9> per block.
//   k_mle_eval_reduce the blocks' partials of a table -> its canonical value: a second small launch, as k_mle_sub_reduce /
//                     k_verify_reduce are (publishing from the last block costs a streaming pass 15 % in fences: DESIGN.md).
//   k_mle_eval_small  everything below: one block per table, the weights built in LDS from the point, three levels of lazy sums.
//
// Set-up per chunk of tables (launch_mle_eval): the leading weights and the two tables E_up, E_63 come from launch_eq_table
// (its layout is the one needed: proof-major, MSB-first, Montgomery), the plans from launch_mle_fold_plan -- the prover's kernels.
// Tables come in GROUPS of G that share one point (the M tables of a sumcheck; G = 1: every table its own point): table g G + m
// is evaluated at point g, and everything that depends on the point alone -- weights, plan, E_up, E_63 -- is built once per
// group.  The partials, the second-level sums and the values stay per table, and each is computed exactly as at G = 1.
// Table entries are read as 256-bit integers: any value is taken modulo r (the byte-wise fold and the lazy sums are exact).
#include "dev_util.h"
#include "kernels.h"
#include "mfma_fold.h"
#include "options.h"

namespace gkr {

namespace {

constexpr uint32_t kEvalChunk = 2048;       // outputs per block the launch aims for: 8 iterations, 1/8 of the per-block epilogue per output
constexpr uint32_t kEvalMinChunk = 256;     // one iteration of the block's four waves
constexpr uint32_t kEvalFillBlocks = 2048;  // blocks over the batch below which the chunks are made shorter (8 per CU)
constexpr uint32_t kEvalMaxBlocks = 4096;   // per table

// grid = (nblk, tables), block = 256; chunk = 2^(n-5) / nblk a multiple of 64; plans, e_up, e_63: one per group of G tables
__global__ void __launch_bounds__(256) k_mle_eval_mfma(const Fr* __restrict__ tables, uint32_t n, uint32_t G, const MfmaFoldPlan* __restrict__ plans,
                                                       const Fr* __restrict__ e_up, const Fr* __restrict__ e_63, Acc<9>* __restrict__ partials) {
    __shared__ Acc<9> smem[4];
    __shared__ __attribute__((aligned(16))) unsigned char digits[32 * 32 * (1 << kMfmaMaxJ)];
    const uint32_t m = n - (uint32_t)kMfmaMaxJ, S = 1u << m;
    const Fr* s = tables + ((size_t)blockIdx.y << n);
    // (the table's group: the same on every lane, and said so -- the quotient of two scalars is computed on the vector unit, and
    // E_up's entries and the plan are scalar loads only from an address in scalar registers)
    const uint32_t grp = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.y / G));
    const Fr* up = e_up + ((size_t)grp << (m - 6u));
    const uint32_t chunk = S / gridDim.x;
    const uint32_t begin = blockIdx.x * chunk;
    Lazy17 sum = lazy_zero();   // sum over this lane's outputs of y * E_up[i >> 6] (E_up Montgomery), unreduced
    mfma_multifold_stream<kMfmaMaxJ>(s, S, plans + grp, begin, begin + chunk, blockIdx.x * 5u + blockIdx.y * 3u, digits,
                                     [&](uint32_t e0, uint32_t, uint32_t, const Fr& y) { lazy_mac_s(sum, y, load_fr(up + (e0 >> 6))); });
    // (the waves a short chunk leaves idle arrive here with a zero sum)
    Acc<9> acc[1] = {acc_zero<9>()};
    acc_add_fr(acc[0], mont_mul(lazy_reduce(sum), load_fr(e_63 + (size_t)grp * 64u + (threadIdx.x & 63u))));
    block_sum<9, 1>(acc, smem);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
}

// grid = (batch), block = 256
__global__ void __launch_bounds__(256) k_mle_eval_reduce(const Acc<9>* __restrict__ partials, uint32_t nblk, Fr* __restrict__ out) {
    __shared__ Acc<10> smem[4];
    const Acc<9>* p = partials + (size_t)blockIdx.x * nblk;
    Acc<10> acc[1] = {acc_zero<10>()};
    for (uint32_t i = threadIdx.x; i < nblk; i += blockDim.x) acc_add_acc(acc[0], p[i]);
    block_sum<10, 1>(acc, smem);
    if (threadIdx.x == 0) store_fr(out + blockIdx.x, acc_reduce(acc[0]));
}

// One block per table, any n >= 1.  The index splits into (top | mid | low): thread t owns the entries whose low
// nl = min(n, 8) bits are t; per value of the top bits it sums its 2^nm (nm <= 8) entries against the mid table unreduced, reduces,
// and adds the result times the top bits' weight to a second unreduced sum; its own low weight comes last, once.
// grid = (tables), block = 256; points: one per group of G tables
__global__ void __launch_bounds__(256) k_mle_eval_small(const Fr* __restrict__ tables, uint32_t n, uint32_t G, const Fr* __restrict__ points,
                                                        Fr* __restrict__ out) {
    __shared__ Fr s_f[2][32];   // Montgomery forms of 1 - r_j and r_j
    __shared__ Fr s_lo[256], s_mid[256];
    __shared__ Acc<9> smem[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t nl = n < 8u ? n : 8u, nm = n - nl < 8u ? n - nl : 8u, nt = n - nl - nm;
    const Fr* t = tables + ((size_t)blockIdx.x << n);
    if (tid < n) {
        const Fr x = load_fr(points + (size_t)(blockIdx.x / G) * n + tid);
        Fr one = fr_zero();
        one.l[0] = 1u;
        s_f[1][tid] = to_mont(x);
        s_f[0][tid] = to_mont(fr_sub(one, x));
    }
    __syncthreads();
    {
        Fr lo = fr_mont_one(), mid = fr_mont_one();
        for (uint32_t i = 0; i < nl; ++i) lo = mont_mul(lo, s_f[(tid >> (nl - 1u - i)) & 1u][nt + nm + i]);
        for (uint32_t i = 0; i < nm; ++i) mid = mont_mul(mid, s_f[(tid >> (nm - 1u - i)) & 1u][nt + i]);
        s_lo[tid] = lo;     // (entries past 2^nl / 2^nm are never read)
        s_mid[tid] = mid;
    }
    __syncthreads();
    Acc<9> acc[1] = {acc_zero<9>()};
    if (tid < (1u << nl)) {
        Lazy17 outer = lazy_zero();
        for (uint32_t g = 0; g < (1u << nt); ++g) {
            Fr top = fr_mont_one();
            for (uint32_t i = 0; i < nt; ++i) top = mont_mul(top, s_f[(g >> (nt - 1u - i)) & 1u][i]);
            Lazy17 inner = lazy_zero();
            for (uint32_t mi = 0; mi < (1u << nm); ++mi)
                lazy_mac_v(inner, load_fr(t + ((((size_t)g << nm) | mi) << nl) + tid), s_mid[mi]);
            lazy_mac_v(outer, lazy_reduce(inner), top);
        }
        acc_add_fr(acc[0], mont_mul(lazy_reduce(outer), s_lo[tid]));
    }
    block_sum<9, 1>(acc, smem);
    if (tid == 0) store_fr(out + blockIdx.x, acc_reduce(acc[0]));
}

struct EvalWs {
    Fr *weights, *e_up, *e_63;
    MfmaFoldPlan* plans;
    Acc<9>* partials;
    size_t bytes;
};
// the streaming form's workspace of a chunk, carved out of one allocation (every part 16-byte aligned): what belongs to a point
// once per group, the partials per table
EvalWs eval_ws(void* base, uint32_t n, uint32_t groups, uint32_t G, uint32_t nblk) {
    auto up16 = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
    char* p = static_cast<char*>(base);
    EvalWs w;
    size_t off = 0;
    w.plans = reinterpret_cast<MfmaFoldPlan*>(p + off);
    off += up16((size_t)groups * sizeof(MfmaFoldPlan));
    w.weights = reinterpret_cast<Fr*>(p + off);
    off += (size_t)groups * kMleMaxSub * sizeof(Fr);
    w.e_up = reinterpret_cast<Fr*>(p + off);
    off += ((size_t)groups << (n - 11u)) * sizeof(Fr);
    w.e_63 = reinterpret_cast<Fr*>(p + off);
    off += (size_t)groups * 64u * sizeof(Fr);
    w.partials = reinterpret_cast<Acc<9>*>(p + off);
    off += up16((size_t)groups * G * nblk * sizeof(Acc<9>));
    w.bytes = off;
    return w;
}

}  // namespace

bool mle_eval_uses_mfma(uint32_t n) {
    const long long o = opt(OPT_mle_eval_mfma_min_n);
    const uint32_t min_n = o > 0 ? (o < (long long)kMleEvalMfmaValidN ? kMleEvalMfmaValidN : (o > 64 ? 64u : (uint32_t)o)) : kMleEvalMfmaMinN;
    return n >= min_n || n > kMleEvalSmallMaxN;
}

// blocks per table of the streaming form: chunks of kEvalChunk outputs, shorter ones (down to one iteration) while the batch
// does not fill the chip, longer ones for the largest tables
uint32_t mle_eval_blocks(uint32_t n, uint32_t batch) {
    const uint32_t S = 1u << (n - (uint32_t)kMfmaMaxJ);
    uint32_t b = S / kEvalChunk ? S / kEvalChunk : 1u;
    while ((uint64_t)b * batch < kEvalFillBlocks && S / (2u * b) >= kEvalMinChunk) b <<= 1;
    return b > kEvalMaxBlocks ? kEvalMaxBlocks : b;
}

size_t mle_eval_ws_bytes(uint32_t n, uint32_t groups, uint32_t G) {
    if (!mle_eval_uses_mfma(n)) return 16;
    return eval_ws(nullptr, n, groups, G, mle_eval_blocks(n, groups * G)).bytes;
}

void launch_mle_eval(const Fr* tables, uint32_t n, uint32_t groups, uint32_t G, const Fr* points, void* ws, Fr* out, hipStream_t s) {
    const uint32_t batch = groups * G;   // tables
    if (!mle_eval_uses_mfma(n)) {
        hipLaunchKernelGGL(k_mle_eval_small, dim3(batch), dim3(256), 0, s, tables, n, G, points, out);
        return;
    }
    const uint32_t nblk = mle_eval_blocks(n, batch);
    const EvalWs w = eval_ws(ws, n, groups, G, nblk);
    launch_eq_table(points, n, 0u, (uint32_t)kMfmaMaxJ, w.weights, true, groups, s);
    launch_eq_table(points, n, (uint32_t)kMfmaMaxJ, n - 11u, w.e_up, true, groups, s);
    launch_eq_table(points, n, n - 6u, 6u, w.e_63, true, groups, s);
    launch_mle_fold_plan(kMfmaMaxJ, w.weights, w.plans, groups, s);
    hipLaunchKernelGGL(k_mle_eval_mfma, dim3(nblk, batch), dim3(256), 0, s, tables, n, G, w.plans, w.e_up, w.e_63, w.partials);
    hipLaunchKernelGGL(k_mle_eval_reduce, dim3(batch), dim3(256), 0, s, w.partials, nblk, out);
}

}  // namespace gkr

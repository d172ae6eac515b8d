// CDNA4 (gfx950) kernels of the device verifier (gkr_verify_prepare / gkr_verify_prepared, capi_verify.hip): the three sums of
// gkr_verify (dropin.cpp) that are O(gates) or O(2^k), everything else of a verification stays on the host (verify_core.h).
//
//   k_verify_pack       prepare: a layer's gate arrays -> one 8-byte record per gate, every operand and type range-checked
//   k_verify_wiring     add_i(z, b*, c*) and mult_i(z, b*, c*) of EVERY layer of EVERY proof of a chunk in one launch:
//                       sum over the gates of eq(z, g) eq(b*, left(g)) eq(c*, right(g)), split by gate type
//   k_verify_mono_tables / k_verify_mono_dot
//                       sum_S c[S] prod_{j in S} z_j over a table of 2^k monomial coefficients (index MSB-first, as
//                       eval_monomial_table has it), as a dot product with the table (x)_j (1, z_j) -- itself the outer
//                       product of two half tables of <= 2^14 entries, never materialised
//   k_verify_canonical  every coefficient of the chunk's tables below r?  one flag per proof and table
//   k_verify_reduce     the second level of both: one wave per row of block partials
//
// A verifier reads every challenge out of the proof, so nothing here waits for a hash: the host uploads z, the challenges and
// the two coefficient tables of a chunk of proofs, launches everything, and synchronises once.  All sums are exact integer
// arithmetic mod r: any order of the reduction gives the same field element.
//
// Elements >= r in a proof make some of these sums garbage (Montgomery arithmetic assumes operands below r) -- never an
// out-of-range access (every gathered index is masked to its table's size), and never a verdict: verify_core.h consults a
// device value only after the elements it was computed from passed their own checks.
#include <hip/hip_runtime.h>

#include "dev_util.h"
#include "kernels.h"

namespace gkr {

// ---------------------------------------------------------------------------
// prepare: pack and range-check a layer's gates
// ---------------------------------------------------------------------------
// record = {left | type << 31, right}: left, right < 2^k, k <= GKR_MAX_K_NEXT = 24.  *bad |= 1 on an operand >= 2^k or a
// type > 1 (the record of such a gate is masked like any other; the handle is never used).  grid = blocks, block = 256
__global__ void __launch_bounds__(256) k_verify_pack(const uint8_t* __restrict__ gate_type, const uint32_t* __restrict__ left,
                                                     const uint32_t* __restrict__ right, uint32_t gates, uint32_t k,
                                                     uint2* __restrict__ packed, uint32_t* __restrict__ bad) {
    const uint32_t limit = 1u << k;
    bool b = false;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < gates; g += gridDim.x * blockDim.x) {
        const uint32_t t = gate_type[g], l = left[g], r = right[g];
        b |= t > 1u || l >= limit || r >= limit;
        packed[g] = make_uint2((l & (limit - 1u)) | ((t & 1u) << 31), r & (limit - 1u));
    }
    if (__any(b) && (threadIdx.x & 63u) == 0) atomicOr(bad, 1u);
}

void launch_verify_pack(const uint8_t* gate_type, const uint32_t* left, const uint32_t* right, uint32_t gates, uint32_t k, uint2* packed,
                        uint32_t* bad, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_pack, dim3(blocks_for(gates, 2048)), dim3(256), 0, s, gate_type, left, right, gates, k, packed, bad);
}

// ---------------------------------------------------------------------------
// the wiring pass
// ---------------------------------------------------------------------------
// grid = (blocks, layers, proofs), block = 256.  A thread strides over the layer's gates: the record and the two halves of
// eq(z, g) = E_hi[g >> kl] E_lo[g & mask] are coalesced (E_lo) or wave-uniform-ish (E_hi) loads, eq_b[left] and eq_c[right]
// are 32-byte gathers from tables of up to 32 MiB that the Infinity Cache holds.  Every table is in Montgomery form, so are
// the three products and the sums.  Two Acc<9> per thread, one reduction per block (wave shuffles, then LDS), partial
// (layer, proof, add | mult, block) -> partials; blocks beyond a small layer's gates store zeros, so that the second level
// reads whole rows.
__global__ void __launch_bounds__(256) k_verify_wiring(const VerifyLayer* __restrict__ layers, uint32_t n_layers, Fr* __restrict__ partials) {
    __shared__ Acc<9> s_acc[4 * 2];
    const uint32_t layer = blockIdx.y, proof = blockIdx.z;
    const VerifyLayer L = layers[layer];
    const uint32_t gates = 1u << L.k_i, lo_mask = (1u << L.kl) - 1u, op_mask = (1u << L.k) - 1u;
    const Fr* e_hi = L.e_hi + ((size_t)proof << (L.k_i - L.kl));
    const Fr* e_lo = L.e_lo + ((size_t)proof << L.kl);
    const Fr* eq_b = L.eq_b + ((size_t)proof << L.k);
    const Fr* eq_c = L.eq_c + ((size_t)proof << L.k);
    Acc<9> acc[2] = {acc_zero<9>(), acc_zero<9>()};
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < gates; g += gridDim.x * blockDim.x) {
        const uint2 rec = L.gates[g];
        const uint32_t left = rec.x & op_mask, right = rec.y & op_mask;   // masked again: a missed check cannot read outside a table
        const Fr b = load_fr(eq_b + left), c = load_fr(eq_c + right);
        const Fr ez = mont_mul(load_fr(e_hi + (g >> L.kl)), load_fr(e_lo + (g & lo_mask)));
        const Fr t = mont_mul(ez, mont_mul(b, c));
        if (rec.x >> 31)
            acc_add_fr(acc[1], t);
        else
            acc_add_fr(acc[0], t);
    }
    block_sum<9, 2>(acc, s_acc);
    if (threadIdx.x == 0) {
        Fr* out = partials + (((size_t)proof * n_layers + layer) * 2u) * gridDim.x + blockIdx.x;
        store_fr(out, acc_reduce(acc[0]));
        store_fr(out + gridDim.x, acc_reduce(acc[1]));
    }
}

// out[row] = sum of partials[row * width .. + width): one wave per row.  grid = rows, block = 64
__global__ void __launch_bounds__(64) k_verify_reduce(const Fr* __restrict__ partials, uint32_t width, Fr* __restrict__ out) {
    const Fr* p = partials + (size_t)blockIdx.x * width;
    Acc<9> a = acc_zero<9>();
    for (uint32_t i = threadIdx.x; i < width; i += 64u) acc_add_fr(a, load_fr(p + i));
    a = wave_sum(a);
    if (threadIdx.x == 0) store_fr(out + blockIdx.x, acc_reduce(a));
}

uint32_t verify_wiring_blocks(uint32_t max_k_i) { return blocks_for((uint64_t)1 << max_k_i, 1024); }

void launch_verify_wiring(const VerifyLayer* layers, uint32_t n_layers, uint32_t max_k_i, uint32_t batch, Fr* partials, Fr* out, hipStream_t s) {
    const uint32_t nblk = verify_wiring_blocks(max_k_i);
    hipLaunchKernelGGL(k_verify_wiring, dim3(nblk, n_layers, batch), dim3(256), 0, s, layers, n_layers, partials);
    hipLaunchKernelGGL(k_verify_reduce, dim3(batch * n_layers * 2u), dim3(64), 0, s, partials, nblk, out);
}

// ---------------------------------------------------------------------------
// monomial-coefficient tables at a point
// ---------------------------------------------------------------------------
// The half tables of (x)_j (1, z_j), Montgomery: T_hi over the kh leading variables of the point, T_lo over the kl trailing
// ones; entry e = the product of the z_j whose bit is set in e (variable j <-> bit nvars - 1 - j: MSB-first).  A thread per
// entry, at most 14 products.  points: `stride` elements per proof, the point at `first`.  grid = (blocks, proofs), block = 256
__global__ void __launch_bounds__(256) k_verify_mono_tables(const Fr* __restrict__ points, uint32_t stride, uint32_t first, uint32_t kh, uint32_t kl,
                                                            Fr* __restrict__ t_hi, Fr* __restrict__ t_lo) {
    const uint32_t proof = blockIdx.y, nh = 1u << kh, nl = 1u << kl;
    const Fr* pt = points + (size_t)proof * stride + first;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < nh + nl; e += gridDim.x * blockDim.x) {
        const bool hi = e < nh;
        const uint32_t idx = hi ? e : e - nh, nv = hi ? kh : kl, v0 = hi ? 0u : kh;
        Fr p = fr_mont_one();
        for (uint32_t j = 0; j < nv; ++j)
            if ((idx >> (nv - 1u - j)) & 1u) p = mont_mul(p, to_mont(load_fr(pt + v0 + j)));
        store_fr((hi ? t_hi + ((size_t)proof << kh) : t_lo + ((size_t)proof << kl)) + idx, p);
    }
}

// partial[proof][block] = sum over the block's entries of c[S] (T_hi[S >> kl] T_lo[S & mask]): coefficients canonical, the
// half tables Montgomery -> canonical sums.  grid = (blocks, proofs), block = 256
__global__ void __launch_bounds__(256) k_verify_mono_dot(const Fr* __restrict__ coeffs, uint32_t k, uint32_t kl, const Fr* __restrict__ t_hi,
                                                         const Fr* __restrict__ t_lo, Fr* __restrict__ partials) {
    __shared__ Acc<9> s_acc[4];
    const uint32_t proof = blockIdx.y, n = 1u << k, lo_mask = (1u << kl) - 1u;
    const Fr* c = coeffs + ((size_t)proof << k);
    const Fr* th = t_hi + ((size_t)proof << (k - kl));
    const Fr* tl = t_lo + ((size_t)proof << kl);
    Acc<9> acc[1] = {acc_zero<9>()};
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const Fr t = mont_mul(load_fr(th + (i >> kl)), load_fr(tl + (i & lo_mask)));
        acc_add_fr(acc[0], mont_mul(load_fr(c + i), t));
    }
    block_sum<9, 1>(acc, s_acc);
    if (threadIdx.x == 0) store_fr(partials + (size_t)proof * gridDim.x + blockIdx.x, acc_reduce(acc[0]));
}

// every coefficient of a chunk's tables < r?  coeffs: 2^k elements per proof; flags[proof * flag_stride] |= 1 on an element
// >= r (k_check_canonical with the proof as a grid dimension: one launch per kind of table, not one per proof).
// grid = (blocks, proofs), block = 256
__global__ void __launch_bounds__(256) k_verify_canonical(const Fr* __restrict__ coeffs, uint32_t k, uint32_t* __restrict__ flags, uint32_t flag_stride) {
    const uint32_t proof = blockIdx.y, n = 1u << k;
    const Fr* c = coeffs + ((size_t)proof << k);
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bad |= !fr_is_canonical(load_fr(c + i));
    if (__any(bad) && (threadIdx.x & 63u) == 0) atomicOr(flags + (size_t)proof * flag_stride, 1u);
}

void launch_verify_canonical(const Fr* coeffs, uint32_t k, uint32_t* flags, uint32_t flag_stride, uint32_t batch, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_canonical, dim3(blocks_for((uint64_t)1 << k, 2048), batch), dim3(256), 0, s, coeffs, k, flags, flag_stride);
}

uint32_t verify_mono_blocks(uint32_t k) { return blocks_for((uint64_t)1 << k, 1024); }

void launch_verify_mono_eval(const Fr* points, uint32_t stride, uint32_t first, uint32_t k, const Fr* coeffs, Fr* t_hi, Fr* t_lo, Fr* partials,
                             Fr* out, uint32_t batch, hipStream_t s) {
    const uint32_t kl = k / 2u, kh = k - kl, nblk = verify_mono_blocks(k);
    hipLaunchKernelGGL(k_verify_mono_tables, dim3(blocks_for(((uint64_t)1 << kh) + ((uint64_t)1 << kl), 256), batch), dim3(256), 0, s, points, stride,
                       first, kh, kl, t_hi, t_lo);
    hipLaunchKernelGGL(k_verify_mono_dot, dim3(nblk, batch), dim3(256), 0, s, coeffs, k, kl, t_hi, t_lo, partials);
    hipLaunchKernelGGL(k_verify_reduce, dim3(batch), dim3(64), 0, s, partials, nblk, out);
}

}  // namespace gkr

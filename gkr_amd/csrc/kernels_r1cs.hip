// CDNA4 (gfx950) kernels of the R1CS zero-check's tables (gkr_r1cs_rows_device): Az, Bz, Cz of a witness as sparse matrix-vector
// products over BN254 Fr, and the row-wise check a * b == c; and of the R1CS inner sumcheck's table (gkr_r1cs_cols_device): the
// same records gathered by COLUMN against the eq table of a point (the second half of this file); and of the verifier's last
// relation (gkr_r1cs_matrix_evals_device): the three matrices' multilinear extensions at a point, one pass over the CSR records
// (the last part).
//
//   out[(b * 3 + m) * 2^n + i] = sum_t pool[coeff_t] * w_b[wire_t]   over the records of row i of matrix m, canonical;
//   rows >= n_constraints are zero.
//
// The matrices are CSR (r1cs.cpp): 32-bit row offsets, 8-byte records {wire, pool index}, one pool of distinct coefficients in
// MONTGOMERY form.  A witness entry is canonical; canonical x Montgomery summed unreduced in a Lazy17 and reduced once
// (lazy_reduce takes a factor 2^-256) is the canonical sum.  Pool entries 0 (one) and 1 (r - 1) take no product: w, or r - w,
// joins the sum as w * 2^256 (lazy_add_hi), nine additions.
// Term bounds: a term is a product of two values below r < 2^254, below 2^508, or w * 2^256 < 2^510 (about 5.3 r^2); a row has
// fewer than 2^32 terms (the offsets are 32 bits wide), so a row's sum stays below 2^542 < 2^544: NO row needs an intermediate
// reduction of its Lazy17, in either kernel.
//
// The witness gather is 32 bytes out of a 128-byte line per term, the pattern of the wide gate passes (DESIGN.md section 3
// prices it at 3.8x the algorithmic bytes); the records and the row offsets stream.
// Every element offset (witness, tables) is 64 bits wide; 32-bit values index rows (< 2^30) and records (< 2^32) only.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "dev_util.h"

namespace gkr {

namespace {

// matrix m's arrays picked with selects (m is wave-uniform: scalar selects, no indexed copy of the argument struct in memory)
template <typename T>
__device__ __forceinline__ T pick3(const T (&a)[3], uint32_t m) {
    return m == 0 ? a[0] : (m == 1 ? a[1] : a[2]);
}

// One record's contribution.  The branch is per lane.  In the ISA (hipcc -O3, gfx950) the +-1 side is 78 instructions (the
// negation, eight selects, the nine-limb carry chain) and the product side about 320 (64 v_mad_u64_u32 with their carries and the
// 32-byte pool load), behind a common head of 17 (the record and the witness entry).  A branch-free form in the manner of
// lazy_mac_sel (every term a product, +-1 as pool entries) costs every wave the 320; with the branch a wave whose lanes are all
// +-1 -- all but a few waves of a circom matrix -- never issues the product, and a mixed wave pays both sides, a quarter over the
// product alone.  So: the branch.
__device__ __forceinline__ void r1cs_term(Lazy17& acc, const uint2 rec, const Fr* __restrict__ wit, const Fr* __restrict__ pool_mont) {
    const Fr w = load_fr(wit + rec.x);
    if (rec.y < 2u) {
        const Fr neg = fr_sub(fr_zero(), w);   // r - w; 0 stays 0
        Fr x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.l[i] = rec.y ? neg.l[i] : w.l[i];
        lazy_add_hi(acc, x, true);
    } else {
        lazy_mac_v(acc, w, load_fr(pool_mont + rec.y));
    }
}

}  // namespace

// One thread per row.  Rows with more than kR1csLongRow records are left to k_r1cs_rows_long (a thread-per-row wave runs as
// long as its longest row); rows past n_constraints store zero.  One lazy_reduce per row (see the term bounds above).
// grid = (ceil(2^n / 256), 3, batch)
__global__ void __launch_bounds__(256) k_r1cs_rows_short(const R1csCsr csr, const Fr* __restrict__ witness, size_t witness_stride,
                                                         Fr* __restrict__ out) {
    const uint32_t m = blockIdx.y, row = blockIdx.x * 256u + threadIdx.x;
    const size_t len = (size_t)1 << csr.n;
    if (row >= len) return;
    Fr* dst = out + ((size_t)blockIdx.z * 3 + m) * len + row;
    if (row >= csr.n_constraints) {
        store_fr(dst, fr_zero());
        return;
    }
    const uint32_t* __restrict__ rp = pick3(csr.row_ptr, m);
    const uint2* __restrict__ terms = pick3(csr.terms, m);
    const uint32_t begin = rp[row], end = rp[row + 1];
    if (end - begin > kR1csLongRow) return;
    const Fr* wit = witness + (size_t)blockIdx.z * witness_stride;
    Lazy17 acc = lazy_zero();
    for (uint32_t t = begin; t < end; ++t) r1cs_term(acc, terms[t], wit, csr.pool_mont);
    store_fr(dst, lazy_reduce(acc));
}

// One wave per long row: the lanes stride over the row's records, each with its own Lazy17 and one reduction; the wave totals
// the 64 canonical values through Acc<9> and shuffles (the block reductions of kernels_product.hip), lane 0 stores.  Launched only
// where a matrix has long rows; a matrix with fewer of them than the grid is wide leaves its surplus blocks at once.
// grid = (the largest number of long rows of a matrix, 3, batch), block = 64
__global__ void __launch_bounds__(64) k_r1cs_rows_long(const R1csCsr csr, const Fr* __restrict__ witness, size_t witness_stride,
                                                       Fr* __restrict__ out) {
    const uint32_t m = blockIdx.y;
    if (blockIdx.x >= pick3(csr.n_long, m)) return;   // (block-uniform: before any shuffle)
    const uint32_t* __restrict__ rp = pick3(csr.row_ptr, m);
    const uint2* __restrict__ terms = pick3(csr.terms, m);
    const uint32_t row = pick3(csr.long_rows, m)[blockIdx.x];
    const uint32_t begin = rp[row], end = rp[row + 1];
    const Fr* wit = witness + (size_t)blockIdx.z * witness_stride;
    Lazy17 acc = lazy_zero();
    for (uint64_t t = (uint64_t)begin + threadIdx.x; t < end; t += 64u) r1cs_term(acc, terms[t], wit, csr.pool_mont);   // (64 bits: begin + 63 may pass 2^32)
    Acc<9> sum = acc_zero<9>();
    acc_add_fr(sum, lazy_reduce(acc));
    sum = wave_sum(sum);
    if (threadIdx.x == 0) store_fr(out + (((size_t)blockIdx.z * 3 + m) << csr.n) + row, acc_reduce(sum));
}

// a * b == c at every row below n_constraints of every witness's three tables; first_bad[b] = the lowest row where it fails
// (preset to UINT32_MAX by the launcher).  The block's minimum by wave shuffle and LDS, ONE atomicMin per block that found one.
// grid = (ceil(n_constraints / 256), batch)
__global__ void __launch_bounds__(256) k_r1cs_check(const Fr* __restrict__ tables, uint32_t n, uint32_t n_constraints,
                                                    uint32_t* __restrict__ first_bad) {
    __shared__ uint32_t s_min[4];
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    const size_t len = (size_t)1 << n;
    const Fr* t = tables + (size_t)blockIdx.y * 3 * len;
    uint32_t bad = 0xFFFFFFFFu;
    if (row < n_constraints) {
        const Fr a = load_fr(t + row), b = load_fr(t + len + row), c = load_fr(t + 2 * len + row);
        if (!fr_eq(mont_mul(to_mont(a), b), c)) bad = row;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_down(bad, off, 64);
        bad = o < bad ? o : bad;
    }
    if ((threadIdx.x & 63u) == 0) s_min[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) bad = s_min[w] < bad ? s_min[w] : bad;
        if (bad != 0xFFFFFFFFu) atomicMin(first_bad + blockIdx.y, bad);
    }
}

// ---------------------------------------------------------------------------
// the inner sumcheck's table: T(y) = sum_m rho_m sum_{records (i, c) of column y of matrix m} pool[c] * eq(x, i)
// ---------------------------------------------------------------------------
// The same records gathered the other way: the vector is the canonical eq table of the sumcheck's point, a record's first field
// the ROW, and r1cs_term's arithmetic and term bounds carry over unchanged (a column has fewer than 2^32 records: the offsets are
// 32 bits wide).  Column lengths are heavy-tailed where row lengths are not -- wire 0, the constant, may stand in every
// constraint -- so a long column is cut into SEGMENTS (the host's list) and a wave takes a segment, not a column.
//
// The rho scaling: ONE eq table per sumcheck, one Lazy17 and one lazy_reduce per (column, matrix), then one Montgomery product
// with rho_m (Montgomery form) on the canonical sum and a modular addition.  The other form -- three eq tables pre-scaled by
// rho_m, one accumulator and one reduce per column -- has no product and one reduce per column.  In the ISA (hipcc -O3, gfx950)
// lazy_reduce is about 1400 instructions (192 v_mad_u64_u32) and the product with its addition about 650 (128): a column with
// records in k of the three matrices pays k x 2050 here against 1400 there.  But that form builds, stores and gathers three
// tables of 2^n_x entries where this one has one: three times the eq pass and three times the footprint of the 32-byte gather,
// the access DESIGN.md section 3 prices highest.  An empty (column, matrix) skips its reduce and product here, and a wire of a
// circom system stands in one or two of the three matrices.  So: one table, a product per matrix.  (The other form is not
// measured.)

// One thread per column, the three matrices in turn (m is not unrolled: one copy of r1cs_term's two sides).  A matrix in which
// the column has more than kR1csLongCol records is left to the segment waves; the thread stores the sum of the others -- zero if
// there is none -- which k_r1cs_cols_combine completes.  Columns past n_wires store zero.
// grid = (ceil(2^n_y / 256), batch)
__global__ void __launch_bounds__(256) k_r1cs_cols_short(const R1csCsc csc, const Fr* __restrict__ eq, uint32_t n_x,
                                                         const Fr* __restrict__ rho_mont, Fr* __restrict__ out, size_t out_stride) {
    const size_t y = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (y >= ((size_t)1 << csc.n_y)) return;
    Fr* dst = out + (size_t)blockIdx.y * out_stride + y;
    if (y >= csc.n_wires) {
        store_fr(dst, fr_zero());
        return;
    }
    const Fr* e = eq + ((size_t)blockIdx.y << n_x);
    const Fr* rho = rho_mont + (size_t)blockIdx.y * 3;
    Fr total = fr_zero();
#pragma unroll 1
    for (uint32_t m = 0; m < 3; ++m) {
        const uint32_t* __restrict__ cp = pick3(csc.col_ptr, m);
        const uint2* __restrict__ terms = pick3(csc.terms, m);
        const uint32_t begin = cp[y], end = cp[y + 1];
        if (begin == end || end - begin > kR1csLongCol) continue;
        Lazy17 acc = lazy_zero();
        for (uint32_t t = begin; t < end; ++t) r1cs_term(acc, terms[t], e, csc.pool_mont);
        total = fr_add(total, mont_mul(lazy_reduce(acc), load_fr(rho + m)));
    }
    store_fr(dst, total);
}

// One wave per segment of a long column: the lanes stride over the segment's records, each with its own Lazy17 and one
// reduction; the wave totals the 64 canonical values through Acc<9> and shuffles, lane 0 scales the total by the matrix's rho
// and stores the canonical partial.  No atomics: every segment has a slot of its own.
// grid = (n_segs, batch), block = 64
__global__ void __launch_bounds__(64) k_r1cs_cols_long(const R1csCsc csc, const Fr* __restrict__ eq, uint32_t n_x,
                                                       const Fr* __restrict__ rho_mont, Fr* __restrict__ partials) {
    const uint4 sg = csc.segs[blockIdx.x];   // {column, matrix, first record, one past the last}: block-uniform
    const uint2* __restrict__ terms = pick3(csc.terms, sg.y);
    const Fr* e = eq + ((size_t)blockIdx.y << n_x);
    Lazy17 acc = lazy_zero();
    for (uint64_t t = (uint64_t)sg.z + threadIdx.x; t < sg.w; t += 64u) r1cs_term(acc, terms[t], e, csc.pool_mont);   // (64 bits: first + 63 may pass 2^32)
    Acc<9> sum = acc_zero<9>();
    acc_add_fr(sum, lazy_reduce(acc));
    sum = wave_sum(sum);
    if (threadIdx.x == 0)
        store_fr(partials + (size_t)blockIdx.y * csc.n_segs + blockIdx.x, mont_mul(acc_reduce(sum), load_fr(rho_mont + (size_t)blockIdx.y * 3 + sg.y)));
}

// One wave per column that has segments: the partials of its segments, of all three matrices, added to what the short pass
// stored.  Stream order puts this launch behind both.
// grid = (n_comb, batch), block = 64
__global__ void __launch_bounds__(64) k_r1cs_cols_combine(const R1csCsc csc, const Fr* __restrict__ partials, Fr* __restrict__ out,
                                                          size_t out_stride) {
    const uint32_t col = csc.comb_cols[blockIdx.x], p0 = csc.comb_ptr[blockIdx.x], p1 = csc.comb_ptr[blockIdx.x + 1];
    const Fr* part = partials + (size_t)blockIdx.y * csc.n_segs;
    Acc<9> sum = acc_zero<9>();
    for (uint64_t p = (uint64_t)p0 + threadIdx.x; p < p1; p += 64u) acc_add_fr(sum, load_fr(part + p));
    sum = wave_sum(sum);
    if (threadIdx.x == 0) {
        Fr* dst = out + (size_t)blockIdx.y * out_stride + col;
        acc_add_fr(sum, load_fr(dst));
        store_fr(dst, acc_reduce(sum));
    }
}

// the witness as the product path's second factor: copied, zero behind n_wires
// grid = (ceil(2^n_y / 256), batch)
__global__ void __launch_bounds__(256) k_r1cs_pad_witness(const Fr* __restrict__ witness, size_t witness_stride, uint32_t n_wires, uint32_t n_y,
                                                          Fr* __restrict__ dst, size_t dst_stride) {
    const size_t y = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (y >= ((size_t)1 << n_y)) return;
    store_fr(dst + (size_t)blockIdx.y * dst_stride + y, y < n_wires ? load_fr(witness + (size_t)blockIdx.y * witness_stride + y) : fr_zero());
}

// ---------------------------------------------------------------------------
// the matrices' extensions at a point: M_m~(x, y) = sum_{records (i, w, c) of M_m} pool[c] eq(x, i) eq(y, w)
// ---------------------------------------------------------------------------
// The rows kernels once more with ey = eq(y, .) (canonical, 2^n_y entries) as the gathered vector -- r1cs_term's arithmetic and
// term bounds unchanged -- but a row's sum s_i is not stored: it is multiplied by ex[i] = eq(x, i) (MONTGOMERY form, so that
// mont_mul(ex[i], s_i) is the canonical product) and added to an Acc<9>.  Bound: a partial is a sum of canonical values below
// r < 2^254, an Acc<9> holds 288 bits: 2^34 of them, more than the 2^30 rows a table can have.  Nothing of 2^n entries is written;
// the padding rows i >= n_constraints take no thread.  Slots of (matrix m, proof b), `slots` = short blocks + long blocks apart:
// [0, short blocks) the blocks of k_r1cs_mat_short, behind them one per block of k_r1cs_mat_long.  Every slot is written by the
// block that owns it, on every launch: no atomics, no memset.

// One thread per row below n_constraints; rows with more than kR1csLongRow records are left to k_r1cs_mat_long, an empty row
// takes neither the reduction nor the product.  One canonical partial per block.
// grid = (ceil(n_constraints / 256), 3, batch)
__global__ void __launch_bounds__(256) k_r1cs_mat_short(const R1csCsr csr, const Fr* __restrict__ ex_mont, const Fr* __restrict__ ey, uint32_t n_y,
                                                        Fr* __restrict__ partials, uint32_t slots) {
    __shared__ Acc<9> s_acc[4];
    const uint32_t m = blockIdx.y, row = blockIdx.x * 256u + threadIdx.x;
    Acc<9> sum[1] = {acc_zero<9>()};
    if (row < csr.n_constraints) {
        const uint32_t* __restrict__ rp = pick3(csr.row_ptr, m);
        const uint32_t begin = rp[row], end = rp[row + 1];
        if (begin != end && end - begin <= kR1csLongRow) {
            const uint2* __restrict__ terms = pick3(csr.terms, m);
            const Fr* e = ey + ((size_t)blockIdx.z << n_y);
            Lazy17 acc = lazy_zero();
            for (uint32_t t = begin; t < end; ++t) r1cs_term(acc, terms[t], e, csr.pool_mont);
            acc_add_fr(sum[0], mont_mul(load_fr(ex_mont + ((size_t)blockIdx.z << csr.n) + row), lazy_reduce(acc)));
        }
    }
    block_sum<9, 1>(sum, s_acc);
    if (threadIdx.x == 0) store_fr(partials + ((size_t)blockIdx.z * 3 + m) * slots + blockIdx.x, acc_reduce(sum[0]));
}

// One wave per long row, the loop of k_r1cs_rows_long; lane 0 multiplies the row's sum by ex[row].  A matrix with fewer long rows
// than the grid is wide has its surplus blocks store zero: the sum kernel reads every slot.
// grid = (the largest number of long rows of a matrix, 3, batch), block = 64
__global__ void __launch_bounds__(64) k_r1cs_mat_long(const R1csCsr csr, const Fr* __restrict__ ex_mont, const Fr* __restrict__ ey, uint32_t n_y,
                                                      Fr* __restrict__ partials, uint32_t slots, uint32_t first_slot) {
    const uint32_t m = blockIdx.y;
    Fr* dst = partials + ((size_t)blockIdx.z * 3 + m) * slots + first_slot + blockIdx.x;
    if (blockIdx.x >= pick3(csr.n_long, m)) {   // (block-uniform: before any shuffle)
        if (threadIdx.x == 0) store_fr(dst, fr_zero());
        return;
    }
    const uint32_t* __restrict__ rp = pick3(csr.row_ptr, m);
    const uint2* __restrict__ terms = pick3(csr.terms, m);
    const uint32_t row = pick3(csr.long_rows, m)[blockIdx.x];
    const uint32_t begin = rp[row], end = rp[row + 1];
    const Fr* e = ey + ((size_t)blockIdx.z << n_y);
    Lazy17 acc = lazy_zero();
    for (uint64_t t = (uint64_t)begin + threadIdx.x; t < end; t += 64u) r1cs_term(acc, terms[t], e, csr.pool_mont);   // (64 bits: begin + 63 may pass 2^32)
    Acc<9> sum = acc_zero<9>();
    acc_add_fr(sum, lazy_reduce(acc));
    sum = wave_sum(sum);
    if (threadIdx.x == 0) store_fr(dst, mont_mul(load_fr(ex_mont + ((size_t)blockIdx.z << csr.n) + row), acc_reduce(sum)));
}

// out[b * 3 + m] = the sum of the pair's slots, canonical
// grid = (3, batch), block = 256
__global__ void __launch_bounds__(256) k_r1cs_mat_sum(const Fr* __restrict__ partials, uint32_t slots, Fr* __restrict__ out) {
    __shared__ Acc<9> s_acc[4];
    const size_t pair = (size_t)blockIdx.y * 3 + blockIdx.x;
    const Fr* p = partials + pair * slots;
    Acc<9> sum[1] = {acc_zero<9>()};
    for (uint32_t i = threadIdx.x; i < slots; i += 256u) acc_add_fr(sum[0], load_fr(p + i));
    block_sum<9, 1>(sum, s_acc);
    if (threadIdx.x == 0) store_fr(out + pair, acc_reduce(sum[0]));
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

uint32_t r1cs_matrix_eval_slots(const R1csCsr& csr) {
    return (csr.n_constraints + 255u) / 256u + std::max(csr.n_long[0], std::max(csr.n_long[1], csr.n_long[2]));
}

void launch_r1cs_matrix_evals(const R1csCsr& csr, const Fr* ex_mont, const Fr* ey, uint32_t n_y, uint32_t batch, Fr* partials, Fr* out,
                              hipStream_t s) {
    const uint32_t blocks = (csr.n_constraints + 255u) / 256u, slots = r1cs_matrix_eval_slots(csr), max_long = slots - blocks;
    hipLaunchKernelGGL(k_r1cs_mat_short, dim3(blocks, 3, batch), dim3(256), 0, s, csr, ex_mont, ey, n_y, partials, slots);
    if (max_long) hipLaunchKernelGGL(k_r1cs_mat_long, dim3(max_long, 3, batch), dim3(64), 0, s, csr, ex_mont, ey, n_y, partials, slots, blocks);
    hipLaunchKernelGGL(k_r1cs_mat_sum, dim3(3, batch), dim3(256), 0, s, partials, slots, out);
}

void launch_r1cs_rows(const R1csCsr& csr, const Fr* witness, size_t witness_stride, uint32_t batch, Fr* out, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((((size_t)1 << csr.n) + 255) / 256);
    hipLaunchKernelGGL(k_r1cs_rows_short, dim3(blocks, 3, batch), dim3(256), 0, s, csr, witness, witness_stride, out);
    const uint32_t max_long = std::max(csr.n_long[0], std::max(csr.n_long[1], csr.n_long[2]));
    if (max_long) hipLaunchKernelGGL(k_r1cs_rows_long, dim3(max_long, 3, batch), dim3(64), 0, s, csr, witness, witness_stride, out);
}

hipError_t launch_r1cs_check(const Fr* tables, uint32_t n, uint32_t n_constraints, uint32_t batch, uint32_t* first_bad, hipStream_t s) {
    const hipError_t rc = hipMemsetAsync(first_bad, 0xFF, (size_t)batch * sizeof(uint32_t), s);
    if (rc != hipSuccess) return rc;
    hipLaunchKernelGGL(k_r1cs_check, dim3((n_constraints + 255u) / 256u, batch), dim3(256), 0, s, tables, n, n_constraints, first_bad);
    return hipSuccess;
}

void launch_r1cs_cols(const R1csCsc& csc, const Fr* eq, uint32_t n_x, const Fr* rho_mont, uint32_t batch, Fr* partials, Fr* out,
                      size_t out_stride, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((((size_t)1 << csc.n_y) + 255) / 256);
    hipLaunchKernelGGL(k_r1cs_cols_short, dim3(blocks, batch), dim3(256), 0, s, csc, eq, n_x, rho_mont, out, out_stride);
    if (!csc.n_segs) return;
    hipLaunchKernelGGL(k_r1cs_cols_long, dim3(csc.n_segs, batch), dim3(64), 0, s, csc, eq, n_x, rho_mont, partials);
    hipLaunchKernelGGL(k_r1cs_cols_combine, dim3(csc.n_comb, batch), dim3(64), 0, s, csc, partials, out, out_stride);
}

void launch_r1cs_pad_witness(const Fr* witness, size_t witness_stride, uint32_t n_wires, uint32_t n_y, uint32_t batch, Fr* dst,
                             size_t dst_stride, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((((size_t)1 << n_y) + 255) / 256);
    hipLaunchKernelGGL(k_r1cs_pad_witness, dim3(blocks, batch), dim3(256), 0, s, witness, witness_stride, n_wires, n_y, dst, dst_stride);
}

}  // namespace gkr

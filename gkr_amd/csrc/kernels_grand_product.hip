// CDNA4 (gfx950) kernel of the GRAND PRODUCT's tree (gkr_grand_product_batch_device): the binary tree of multiplication gates over
// `batch` resident tables V of 2^n canonical values,
//   L_n = V,   L_k[i] = L_{k+1}[i] * L_{k+1}[i + 2^k] mod r  (i < 2^k, k = n-1 .. 0),   P = L_0[0],
// variable 1 = the most significant index bit, so the two operands of L_k[i] are entry i of the two contiguous halves of L_{k+1}:
// exactly the two tables the zero-check of layer k reads, where they lie.  Every level is stored, canonical; level k of table b
// at layers + gp_layer_offset(k, batch) + b * 2^k, so each level of the batch is the zero-check's own batch layout.
//
// ONE LAUNCH PER LEVEL, a thread per product: consecutive threads read consecutive elements of either half and write consecutive
// elements (coalesced); a product of two canonical values is two Montgomery products (fr_mul).  55 VGPRs, no scratch, 8 waves per
// SIMD; no LDS, no barrier; all element offsets are 64-bit.
//
// Levels fused in registers -- a thread owning residue i mod 2^(m-L) loads 2^L entries, forms L levels and stores their 2^L - 1
// values, so that the tree reads V once instead of twice -- were built and measured against this form (profiles/r27, MI355X,
// median of 20 alternating launches per form, every level byte-equal): the tree is bound by the products, not by the bytes (at
// n = 20, batch 64, 1.35 ms against 1.19 ms for its 2 (2^n - 1) Montgomery products per table at the box's product rate and 0.68 ms
// for one read and one write of the tables at its copy rate, 1.04 ms for this form's two reads and one write), so the bytes fusion
// saves buy nothing, and a fused thread is a chain of 2^L - 1 dependent products on 2^-L of the threads: L = 3 took 1.39 x this form's
// time at batch 1 (0.138 against 0.099 ms), 1.13 x at batch 8 and the same at batch 64; L = 2 1.06 x and L = 4 2.2 x at batch 1;
// fusing only the small levels (one launch for three levels below 2^10, 2^14 or 2^17 products) lost as well (1.29 x .. 1.48 x at
// batch 1, nothing gained at batch 64).  Only at n = 24, batch 8 (4 GiB of tables) was L = 3 ahead, by 2 % (1.6 interquartile
// ranges).  The fused forms are not kept.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "dev_util.h"

namespace gkr {

namespace {

// level k of every table from level k + 1: src and dst are the levels' bases (table b at + b * 2^(k+1) and + b * 2^k)
__global__ void __launch_bounds__(256) k_gp_level(const Fr* __restrict__ src, Fr* __restrict__ dst, uint32_t k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (1u << k)) return;
    const size_t b = blockIdx.y;
    const Fr* in = src + (b << (k + 1)) + i;
    store_fr(dst + (b << k) + i, fr_mul(load_fr(in), load_fr(in + ((size_t)1 << k))));
}

}  // namespace

uint32_t gp_level_blocks(uint32_t k) { return blocks_for((uint64_t)1 << k, 0xFFFFFFFFu); }

void launch_gp_tree(const Fr* tables, uint32_t n, uint32_t batch, Fr* layers, hipStream_t s) {
    for (uint32_t k = n; k-- > 0;) {
        const Fr* src = k + 1 == n ? tables : layers + gp_layer_offset(k + 1, batch);
        hipLaunchKernelGGL(k_gp_level, dim3(gp_level_blocks(k), batch), dim3(256), 0, s, src, layers + gp_layer_offset(k, batch), k);
    }
}

}  // namespace gkr

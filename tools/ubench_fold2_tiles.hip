// Micro-benchmark of the two-level first fold alone (k_mle_multifold2_mfma, csrc/kernels.hip) over the tiles a block takes:
// `batch` tables of 2^n entries (default 128 x 2^20, the headline's launch), T = 1, 2, 4, 8, 16.  Every T's planes and
// partials are compared with T = 1 first; then `reps` timed launches per T, interleaved, over two alternating sets of tables.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I gkr_amd/csrc tools/ubench_fold2_tiles.hip -o tools/bin/ubench_fold2_tiles
//   tools/bin/ubench_fold2_tiles [n] [batch] [reps]
// -DUBENCH_ONE_TILE -I <an older csrc>: the same program around a kernels.hip from before the option fold2_tiles (T = 1 only).
#ifdef UBENCH_ONE_TILE
#include "kernels.hip"
#else
#include "../gkr_amd/csrc/kernels.hip"
#endif

#include <algorithm>
#include <stdio.h>
#include <vector>

using namespace gkr;
// (kernels.hip calls into kernels_wide.hip from a launcher this program never reaches)
namespace gkr {
void launch_line_setup_wide(const Fr*, uint32_t, Fr*, uint32_t*, uint32_t, hipStream_t) {}
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// canonical entries below 2^252, a different value in every limb
__global__ void __launch_bounds__(256) k_ubench_fill(uint32_t* __restrict__ out, size_t words, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t z = seed + i * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        out[i] = (i & 7u) == 7u ? (uint32_t)z & 0x0FFFFFFFu : (uint32_t)z;
    }
}

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 20, batch = argc > 2 ? atoi(argv[2]) : 128, reps = argc > 3 ? atoi(argv[3]) : 21;
    if (n < 18 || n > 24 || batch < 1) return printf("18 <= n <= 24, batch >= 1\n"), 1;
    const size_t len = (size_t)1 << n;
    const uint32_t S = (uint32_t)(len >> 5), I = S >> 5, npart = mle_multifold2_partials(S);
    Fr* tables[2];
    for (int b = 0; b < 2; ++b) {
        CK(hipMalloc(&tables[b], (size_t)batch * len * sizeof(Fr)));
        hipLaunchKernelGGL(k_ubench_fill, dim3(4096), dim3(256), 0, 0, reinterpret_cast<uint32_t*>(tables[b]), (size_t)batch * len * 8, 1000u + b);
    }
    Fr *w, *w2, *planes;
    unsigned char* plans;
    MleSubPartial* partials;
    CK(hipMalloc(&w, (size_t)batch * kMleMaxSub * sizeof(Fr)));
    CK(hipMalloc(&w2, (size_t)batch * kMleMaxSub * sizeof(Fr)));
    CK(hipMalloc(&plans, (size_t)batch * mle_fold_plan_bytes()));
    CK(hipMalloc(&planes, (size_t)batch * kMleFold2Planes * I * sizeof(Fr)));
    CK(hipMalloc(&partials, (size_t)batch * npart * sizeof(MleSubPartial)));
    hipLaunchKernelGGL(k_ubench_fill, dim3(64), dim3(256), 0, 0, reinterpret_cast<uint32_t*>(w), (size_t)batch * kMleMaxSub * 8, 7u);
    hipLaunchKernelGGL(k_ubench_fill, dim3(64), dim3(256), 0, 0, reinterpret_cast<uint32_t*>(w2), (size_t)batch * kMleMaxSub * 8, 8u);
    launch_mle_fold_plan(kMfmaMaxJ, w, plans, batch, 0);
    CK(hipDeviceSynchronize());

#ifdef UBENCH_ONE_TILE
    const uint32_t tiles[] = {1};
    auto launch = [&](uint32_t, int set) {
#else
    const uint32_t tiles[] = {1, 2, 4, 8, 16};
    Options o = default_options();
    auto launch = [&](uint32_t T, int set) {
        o.v[OPT_fold2_tiles] = T;
        OptionScope scope(&o);
#endif
        launch_mle_multifold2(tables[set], len, planes, (size_t)kMleFold2Planes * I, S, batch, plans, w2, partials, 0);
    };
    // ---- the same planes and partials whatever T
    const size_t plane_bytes = (size_t)batch * kMleFold2Planes * I * sizeof(Fr), part_bytes = (size_t)batch * npart * sizeof(MleSubPartial);
    std::vector<unsigned char> ref_planes(plane_bytes), ref_part(part_bytes), got_planes(plane_bytes), got_part(part_bytes);
    for (uint32_t T : tiles) {
        CK(hipMemset(planes, 0xA5, plane_bytes));
        CK(hipMemset(partials, 0xA5, part_bytes));
        launch(T, 0);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(T == 1 ? ref_planes.data() : got_planes.data(), planes, plane_bytes, hipMemcpyDeviceToHost));
        CK(hipMemcpy(T == 1 ? ref_part.data() : got_part.data(), partials, part_bytes, hipMemcpyDeviceToHost));
        if (T == 1) continue;
        const bool same = !memcmp(ref_planes.data(), got_planes.data(), plane_bytes) && !memcmp(ref_part.data(), got_part.data(), part_bytes);
        printf("T = %2u: planes and partials %s T = 1\n", T, same ? "identical to" : "DIFFER from");
        if (!same) return 1;
    }
    // ---- timed, interleaved
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<std::vector<float>> ms(sizeof(tiles) / sizeof(tiles[0]));
    for (int r = -2; r < reps; ++r)
        for (size_t v = 0; v < ms.size(); ++v) {
            CK(hipEventRecord(e0));
            launch(tiles[v], (r + (int)v) & 1);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r >= 0) ms[v].push_back(t);
        }
    const double bytes = (double)batch * len * sizeof(Fr);
    for (size_t v = 0; v < ms.size(); ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const float med = ms[v][ms[v].size() / 2];
        printf("T = %2u: median %.4f ms (min %.4f .. max %.4f), %.0f GB/s of table\n", tiles[v], med, ms[v].front(), ms[v].back(), bytes / med / 1e6);
    }
    return 0;
}

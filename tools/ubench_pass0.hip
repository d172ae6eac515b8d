// Micro-benchmark of pass 0 of a streaming launch alone (csrc/kernels.hip): `batch` tables of 2^n entries, `nblk` partials per table
// (default 128 x 2^20 x 1024, the headline's launch).  Every variant's partials -- sums and dep flags -- are compared with
// k_mle_sub_sums' first; then `reps` timed launches per variant, interleaved, over two alternating sets of tables.
// Every fourth table has all pairs (2m, 2m + 1) equal but for one odd entry in each of three partials, so the flags differ per partial.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_pass0.hip -o tools/bin/ubench_pass0
//   tools/bin/ubench_pass0 [n] [batch] [reps] [nblk]
// Variants: the two-set form <16, 2> (the baseline); the rolling form (U, PPW) = (16, 1), (16, 2), (16, 4), (32, 2) as blocks of four
// waves, (16, 2) as blocks of two and of ONE wave; the same with every XCD's blocks on a contiguous eighth of the launch ("runs");
// U = 8 for the launches of few tables; and <16, 1> with runs as the PUBLISHING instance (k_mle_sub_sums_roll_pub: every block also stores
// a flag-in-word record to pinned host memory, whose words are checked against the sum of the block's four reference partials).
// Only variants whose conditions the shape meets are run.
#include "../gkr_amd/csrc/kernels.hip"

#include <algorithm>
#include <stdio.h>
#include <vector>

using namespace gkr;
// (kernels.hip calls into kernels_wide.hip from a launcher this program never reaches)
namespace gkr {
void launch_line_setup_wide(const Fr*, uint32_t, Fr*, uint32_t*, uint32_t, hipStream_t) {}
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

// canonical entries below 2^252, a different value in every limb; table b with b % 4 == 1 takes entry 2m's words for entry 2m + 1 too
__global__ void __launch_bounds__(256) k_ubench_fill(uint32_t* __restrict__ out, size_t words, size_t words_per_table, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const bool flat = (i / words_per_table) % 4u == 1u;
        uint64_t z = seed + (flat ? i & ~(size_t)8 : i) * 0x9E3779B97F4A7C15ULL;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        z ^= z >> 31;
        out[i] = (i & 7u) == 7u ? (uint32_t)z & 0x0FFFFFFFu : (uint32_t)z;
    }
}

// one bit of one odd entry of three partials of every flat table: a partial's first pair, a partial's last pair, the table's last pair
__global__ void k_ubench_poke(uint32_t* __restrict__ out, size_t words_per_table, uint32_t batch, uint32_t nblk) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || b % 4u != 1u) return;
    const size_t chunk = words_per_table / 8u / nblk;
    uint32_t* t = out + (size_t)b * words_per_table;
    const size_t e[3] = {(size_t)((7u * b + 3u) % nblk) * chunk + 1u, (size_t)((11u * b + 6u) % nblk + 1u) * chunk - 1u, words_per_table / 8u - 1u};
    for (int k = 0; k < 3; ++k) t[e[k] * 8u + (b + 3u * k) % 8u] ^= 8u;
}

struct Variant {
    const char* name;
    void (*kernel)(const Fr*, size_t, uint32_t, uint32_t, MleSubPartial*);
    uint32_t u, ppw, waves;   // loads per lane, partials per wave, waves per block
    bool pub = false;         // the publishing instance (kernel == nullptr: it has two more arguments)
};

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 20, batch = argc > 2 ? atoi(argv[2]) : 128, reps = argc > 3 ? atoi(argv[3]) : 21;
    const uint32_t nblk = argc > 4 ? (uint32_t)atoi(argv[4]) : 1024u;
    if (n < 12 || n > 26 || batch < 1 || reps < 1 || nblk == 0 || (nblk & (nblk - 1)) || nblk > kMaxBlocksPerTable)
        return printf("12 <= n <= 26, batch >= 1, reps >= 1, nblk a power of two up to %u\n", kMaxBlocksPerTable), 1;
    const size_t len = (size_t)1 << n;
    const uint32_t chunk = (uint32_t)(len / nblk);
    const Variant all[] = {
        {"two sets <16, 2>, 4 waves      ", k_mle_sub_sums_stream<16, 2>, 16, 2, 4},
        {"rolling  <16, 1>, 4 waves      ", k_mle_sub_sums_roll<16, 1, false>, 16, 1, 4},
        {"rolling  <16, 2>, 4 waves      ", k_mle_sub_sums_roll<16, 2, false>, 16, 2, 4},
        {"rolling  <16, 4>, 4 waves      ", k_mle_sub_sums_roll<16, 4, false>, 16, 4, 4},
        {"rolling  <32, 2>, 4 waves      ", k_mle_sub_sums_roll<32, 2, false>, 32, 2, 4},
        {"rolling  <16, 2>, 2 waves      ", k_mle_sub_sums_roll<16, 2, false>, 16, 2, 2},
        {"rolling  <16, 2>, 1 wave       ", k_mle_sub_sums_roll<16, 2, false>, 16, 2, 1},
        {"rolling  <16, 2>, 4 waves, runs", k_mle_sub_sums_roll<16, 2, true>, 16, 2, 4},
        {"rolling  <16, 2>, 2 waves, runs", k_mle_sub_sums_roll<16, 2, true>, 16, 2, 2},
        {"rolling  <16, 2>, 1 wave,  runs", k_mle_sub_sums_roll<16, 2, true>, 16, 2, 1},
        {"rolling  <16, 1>, 4 waves, runs", k_mle_sub_sums_roll<16, 1, true>, 16, 1, 4},
        {"rolling  <16, 1>, 4 w, runs, PUB", nullptr, 16, 1, 4, true},
        {"rolling  <32, 2>, 4 waves, runs", k_mle_sub_sums_roll<32, 2, true>, 32, 2, 4},
        {"rolling  <8, 1>,  4 waves      ", k_mle_sub_sums_roll<8, 1, false>, 8, 1, 4},
        {"rolling  <8, 1>,  4 waves, runs", k_mle_sub_sums_roll<8, 1, true>, 8, 1, 4},
        {"two sets <8, 1>,  4 waves      ", k_mle_sub_sums_stream<8, 1>, 8, 1, 4},
    };
    std::vector<Variant> vars;
    for (const Variant& v : all)   // whole rounds of loads per partial, whole blocks of waves: the launcher's conditions
        if (chunk % (32u * v.u) == 0 && nblk % (v.ppw * v.waves) == 0) vars.push_back(v);
    if (vars.empty()) return printf("no variant takes chunks of %u entries\n", chunk), 1;

    Fr* tables[2];
    const size_t words_per_table = len * 8;
    for (int b = 0; b < 2; ++b) {
        CK(hipMalloc(&tables[b], (size_t)batch * len * sizeof(Fr)));
        hipLaunchKernelGGL(k_ubench_fill, dim3(4096), dim3(256), 0, 0, reinterpret_cast<uint32_t*>(tables[b]), (size_t)batch * words_per_table,
                           words_per_table, 1000u + b);
        hipLaunchKernelGGL(k_ubench_poke, dim3((batch + 63) / 64), dim3(64), 0, 0, reinterpret_cast<uint32_t*>(tables[b]), words_per_table,
                           (uint32_t)batch, nblk);
    }
    MleSubPartial* partials;
    const size_t npart = (size_t)batch * nblk, part_bytes = npart * sizeof(MleSubPartial);
    CK(hipMalloc(&partials, part_bytes));
    CK(hipDeviceSynchronize());
    uint64_t* flagged;   // nblk / 4 records per table
    const size_t nrec = npart / 4u;
    CK(hipHostMalloc(&flagged, nrec * kFlagRecWords * sizeof(uint64_t), hipHostMallocCoherent | hipHostMallocMapped));
    memset(flagged, 0, nrec * kFlagRecWords * sizeof(uint64_t));
    uint32_t ticket = 0;
    auto launch = [&](const Variant& v, int set) {
        if (v.pub)
            hipLaunchKernelGGL((k_mle_sub_sums_roll_pub<16, true>), dim3(nblk / 4u, batch), dim3(256), 0, 0, tables[set], len, chunk, nblk, partials, flagged,
                               next_ticket(ticket));
        else
            hipLaunchKernelGGL(v.kernel, dim3(nblk / (v.ppw * v.waves), batch), dim3(64u * v.waves), 0, 0, tables[set], len, chunk, nblk, partials);
    };
    // every word of every record: the ticket, and the limb of the sum of the block's four reference partials (the OR of their flags)
    auto records_same = [&](const std::vector<MleSubPartial>& ref) {
        for (size_t r = 0; r < nrec; ++r) {
            Acc<9> tot = acc_zero<9>();
            uint32_t dep = 0;
            for (int w = 0; w < 4; ++w) acc_add_acc(tot, ref[4 * r + w].sum), dep |= ref[4 * r + w].dep;
            for (uint32_t l = 0; l < kFlagRecWords; ++l)
                if (flagged[r * kFlagRecWords + l] != flag_word(l < 9u ? tot.l[l] : dep, ticket)) return false;
        }
        return true;
    };

    // ---- the same partials as k_mle_sub_sums, flags included
    std::vector<MleSubPartial> ref(npart), got(npart);
    auto same = [&]() {
        for (size_t i = 0; i < npart; ++i)
            if (memcmp(&ref[i].sum, &got[i].sum, sizeof(ref[i].sum)) || ref[i].dep != got[i].dep) return false;
        return true;
    };
    for (int set = 0; set < 2; ++set) {
        CK(hipMemset(partials, 0xA5, part_bytes));
        hipLaunchKernelGGL(k_mle_sub_sums, dim3(nblk, batch), dim3(256), 0, 0, tables[set], len, (uint32_t)len, partials, MlePublish{});
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(ref.data(), partials, part_bytes, hipMemcpyDeviceToHost));
        size_t deps = 0;
        for (size_t i = 0; i < npart; ++i) deps += ref[i].dep;
        if (set == 0) printf("%zu partials of %u entries, %zu of them with the dep flag set\n", npart, chunk, deps);
        for (const Variant& v : vars) {
            CK(hipMemset(partials, 0xA5, part_bytes));
            launch(v, set);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(got.data(), partials, part_bytes, hipMemcpyDeviceToHost));
            const bool ok = same() && (!v.pub || records_same(ref));
            if (set == 0 || !ok) printf("%s: partials and flags %s k_mle_sub_sums'\n", v.name, ok ? "identical to" : "DIFFER from");
            if (!ok) return 1;
        }
    }
    // ---- timed, interleaved
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<std::vector<float>> ms(vars.size());
    for (int r = -2; r < reps; ++r)
        for (size_t v = 0; v < vars.size(); ++v) {
            CK(hipEventRecord(e0));
            launch(vars[v], (r + (int)v) & 1);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            if (r >= 0) ms[v].push_back(t);
        }
    const double bytes = (double)batch * len * sizeof(Fr);
    for (size_t v = 0; v < vars.size(); ++v) {
        std::sort(ms[v].begin(), ms[v].end());
        const float med = ms[v][ms[v].size() / 2];
        printf("%s: median %.4f ms (min %.4f .. max %.4f), %.0f GB/s of table\n", vars[v].name, med, ms[v].front(), ms[v].back(), bytes / med / 1e6);
    }
    return 0;
}

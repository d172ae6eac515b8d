// Stand-alone check of the CSR flattening of an R1CS (gkr_r1cs_csr_info / gkr_r1cs_csr_export, csrc/r1cs.cpp) against a loop over
// gkr_r1cs_export, meant to be built with r1cs.cpp under -fsanitize=address,undefined (tests/test_r1cs_rows_host.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tests/r1cs_csr_selfcheck.cpp gkr_amd/csrc/r1cs.cpp
// Two systems: a chain with +-1 and a few other coefficients, and one with empty combinations, zero coefficients, repeated wires
// and rows of GKR_R1CS_LONG_ROW - 1 .. GKR_R1CS_LONG_ROW + 1 and 200 terms.  Every output array is allocated at its exact size.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../include/gkr_amd.h"

namespace {

const uint64_t kMod[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};

gkr_fr small(uint64_t v) { return gkr_fr{{v, 0, 0, 0}}; }
gkr_fr minus(uint64_t v) {   // r - v for a small v >= 1
    gkr_fr x;
    memcpy(&x, kMod, 32);
    x.l[0] -= v;             // the low limb of r is far above any v used here
    return x;
}
bool same(const gkr_fr& a, const gkr_fr& b) { return memcmp(&a, &b, 32) == 0; }

struct Flat {
    uint32_t n_wires = 0;
    std::vector<uint32_t> counts, wires;
    std::vector<gkr_fr> coeffs;
    void row(const std::vector<std::pair<gkr_fr, uint32_t>>& lc) {
        counts.push_back((uint32_t)lc.size());
        for (const auto& t : lc) {
            coeffs.push_back(t.first);
            wires.push_back(t.second);
        }
    }
};

int fail(const char* what, size_t a = 0, size_t b = 0) {
    printf("r1cs_csr_selfcheck: FAILED: %s (%zu, %zu)\n", what, a, b);
    return 1;
}

int check(const Flat& f) {
    gkr_r1cs* r = nullptr;
    const size_t nc = f.counts.size() / 3;
    if (gkr_r1cs_build(f.n_wires, 1, 1, 1, nc, f.counts.data(), f.wires.data(), f.coeffs.data(), &r) != GKR_OK) return fail("build");
    gkr_r1cs_info_t inf;
    gkr_r1cs_csr_info_t ci;
    if (gkr_r1cs_info(r, &inf) != GKR_OK || gkr_r1cs_csr_info(r, &ci) != GKR_OK) return fail("info");
    if (ci.n_constraints != nc || ci.n_wires != f.n_wires || ci.n < 2 || ((size_t)1 << ci.n) < nc || (ci.n > 2 && ((size_t)1 << (ci.n - 1)) >= nc))
        return fail("sizes", ci.n, nc);
    // the file's form, by the existing export
    std::vector<uint32_t> counts(3 * nc), wires(inf.n_terms ? inf.n_terms : 1);
    std::vector<gkr_fr> coeffs(inf.n_terms ? inf.n_terms : 1);
    if (gkr_r1cs_export(r, counts.data(), wires.data(), coeffs.data()) != GKR_OK) return fail("export");
    std::vector<gkr_fr> pool(ci.n_pool), pool_m(ci.n_pool);
    if (ci.n_pool < 2) return fail("pool size");
    for (int m = 0; m < 3; ++m) {
        std::vector<uint32_t> row_ptr(nc + 1), long_rows(ci.n_long_rows[m]);
        std::vector<gkr_r1cs_term> terms(ci.n_terms[m]);
        if (gkr_r1cs_csr_export(r, m, row_ptr.data(), terms.data(), long_rows.data(), pool_m.data()) != GKR_OK) return fail("csr export", m);
        if (m == 0)
            pool = pool_m;
        else if (memcmp(pool.data(), pool_m.data(), pool.size() * sizeof(gkr_fr)) != 0)
            return fail("one pool for the three matrices", m);
        // each output alone (the others NULL) gives the same
        std::vector<uint32_t> rp2(nc + 1);
        if (gkr_r1cs_csr_export(r, m, rp2.data(), nullptr, nullptr, nullptr) != GKR_OK || rp2 != row_ptr) return fail("row_ptr alone", m);
        size_t pos = 0, kept_total = 0, n_long = 0;
        if (row_ptr[0] != 0) return fail("row_ptr[0]");
        for (size_t i = 0; i < nc; ++i)
            for (int j = 0; j < 3; ++j) {
                const uint32_t cnt = counts[3 * i + j];
                if (j == m) {
                    size_t kept = 0;
                    for (uint32_t t = 0; t < cnt; ++t) {
                        const gkr_fr& c = coeffs[pos + t];
                        if (!(c.l[0] | c.l[1] | c.l[2] | c.l[3])) continue;   // dropped
                        if (kept_total >= terms.size()) return fail("too few terms", m, i);
                        const gkr_r1cs_term& rec = terms[kept_total];
                        if (rec.wire != wires[pos + t]) return fail("wire", m, i);
                        if (rec.coeff >= pool.size() || !same(pool[rec.coeff], c)) return fail("coefficient", m, i);
                        ++kept_total;
                        ++kept;
                    }
                    if (row_ptr[i + 1] != kept_total) return fail("row_ptr", m, i);
                    if (kept > GKR_R1CS_LONG_ROW) {
                        if (n_long >= long_rows.size() || long_rows[n_long] != i) return fail("long row list", m, i);
                        ++n_long;
                    }
                }
                pos += cnt;
            }
        if (kept_total != terms.size() || n_long != long_rows.size()) return fail("counts", kept_total, n_long);
    }
    if (!same(pool[0], small(1)) || !same(pool[1], minus(1))) return fail("pool[0] = 1, pool[1] = r - 1");
    for (size_t a = 0; a < pool.size(); ++a)
        for (size_t b = a + 1; b < pool.size(); ++b)
            if (same(pool[a], pool[b])) return fail("pool entries are distinct", a, b);
    if (gkr_r1cs_csr_export(r, 3, nullptr, nullptr, nullptr, nullptr) != GKR_ERR_INVALID || gkr_r1cs_csr_export(r, -1, nullptr, nullptr, nullptr, nullptr) != GKR_ERR_INVALID)
        return fail("matrix outside 0 .. 2");
    gkr_r1cs_free(r);
    return 0;
}

}  // namespace

int main() {
    // 1. a chain: x_{i+1} = (x_i + k_i) * (-x_i), coefficients 1, r - 1 and k_i
    Flat chain;
    chain.n_wires = 301;
    for (uint32_t i = 0; i < 300; ++i) {
        chain.row({{small(1), i}, {small(3 + i % 7), 0}});
        chain.row({{minus(1), i}});
        chain.row({{small(1), i + 1}});
    }
    if (check(chain)) return 1;
    // 2. empty combinations, zero coefficients, repeated wires, rows around the long-row length
    Flat odd;
    odd.n_wires = 17;
    const uint32_t lens[] = {0, 1, GKR_R1CS_LONG_ROW - 1, GKR_R1CS_LONG_ROW, GKR_R1CS_LONG_ROW + 1, 200};
    for (uint32_t a : lens)
        for (uint32_t shift = 0; shift < 3; ++shift) {
            for (uint32_t j = 0; j < 3; ++j) {
                const uint32_t len = j == shift ? a : (j == (shift + 1) % 3 ? 2u : 0u);
                std::vector<std::pair<gkr_fr, uint32_t>> lc;
                for (uint32_t t = 0; t < len; ++t) lc.push_back({t % 5 == 4 ? minus(1 + t % 3) : small(1 + t % 4), (t * 7) % 17});
                if (len > 2) lc.insert(lc.begin() + 1, {small(0), 3u});   // a zero coefficient: not a term
                odd.row(lc);
            }
        }
    if (check(odd)) return 1;
    // the refusals that need no large system
    gkr_r1cs* empty = nullptr;
    gkr_r1cs_csr_info_t ci;
    if (gkr_r1cs_build(4, 1, 1, 1, 0, nullptr, nullptr, nullptr, &empty) != GKR_OK) return fail("build of the empty system");
    if (gkr_r1cs_csr_info(empty, &ci) != GKR_ERR_INVALID || gkr_r1cs_csr_info(nullptr, &ci) != GKR_ERR_INVALID) return fail("n_constraints == 0");
    gkr_r1cs_free(empty);
    printf("r1cs_csr_selfcheck: ok\n");
    return 0;
}

// Stand-alone check of the column-major flattening of an R1CS (gkr_r1cs_csc_info / gkr_r1cs_csc_export, csrc/r1cs.cpp) against the
// CSR export, meant to be built with r1cs.cpp under -fsanitize=address,undefined (tests/test_r1cs_cols_host.py):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread tests/r1cs_csc_selfcheck.cpp gkr_amd/csrc/r1cs.cpp
// Two systems: eight wires and 33 constraints with wire 0 in every constraint of all three matrices, columns of exactly
// GKR_R1CS_LONG_COL and GKR_R1CS_LONG_COL + 1 records, a repeated wire in one row, zero coefficients, an unused wire; and a system
// of one wire.  Every output array is allocated at its exact size (an empty one is NULL), and every optional output is also
// passed as NULL.
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
    x.l[0] -= v;
    return x;
}

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
    printf("r1cs_csc_selfcheck: FAILED: %s (%zu, %zu)\n", what, a, b);
    return 1;
}

template <typename T>
T* exact(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }   // an empty array is no array

int check(const Flat& f, const size_t (*want_len)[3], size_t n_want) {
    gkr_r1cs* r = nullptr;
    const size_t nc = f.counts.size() / 3;
    if (gkr_r1cs_build(f.n_wires, 1, 1, 1, nc, f.counts.data(), f.wires.data(), f.coeffs.data(), &r) != GKR_OK) return fail("build");
    gkr_r1cs_csr_info_t ri;
    gkr_r1cs_csc_info_t ci;
    if (gkr_r1cs_csr_info(r, &ri) != GKR_OK || gkr_r1cs_csc_info(r, &ci) != GKR_OK) return fail("info");
    if (ci.n_x != ri.n || ci.n_wires != f.n_wires || ci.n_constraints != nc || ci.n_pool != ri.n_pool) return fail("sizes");
    if (ci.n_y < 2 || ((size_t)1 << ci.n_y) < f.n_wires || (ci.n_y > 2 && ((size_t)1 << (ci.n_y - 1)) >= f.n_wires)) return fail("n_y", ci.n_y);
    std::vector<gkr_fr> pool(ci.n_pool), csr_pool(ri.n_pool);
    for (int m = 0; m < 3; ++m) {
        if (ci.n_terms[m] != ri.n_terms[m]) return fail("n_terms", m);
        std::vector<uint32_t> col_ptr((size_t)f.n_wires + 1), long_cols(ci.n_long_cols[m]), row_ptr(nc + 1);
        std::vector<gkr_r1cs_term> terms(ci.n_terms[m]), csr_terms(ri.n_terms[m]);
        if (gkr_r1cs_csc_export(r, m, col_ptr.data(), exact(terms), exact(long_cols), pool.data()) != GKR_OK) return fail("csc export", m);
        if (gkr_r1cs_csr_export(r, m, row_ptr.data(), exact(csr_terms), nullptr, csr_pool.data()) != GKR_OK) return fail("csr export", m);
        if (memcmp(pool.data(), csr_pool.data(), pool.size() * sizeof(gkr_fr)) != 0) return fail("the pool is the CSR form's", m);
        // each output alone (the others NULL) gives the same
        std::vector<uint32_t> cp2((size_t)f.n_wires + 1), lc2(long_cols.size());
        std::vector<gkr_r1cs_term> t2(terms.size());
        if (gkr_r1cs_csc_export(r, m, cp2.data(), nullptr, nullptr, nullptr) != GKR_OK || cp2 != col_ptr) return fail("col_ptr alone", m);
        if (gkr_r1cs_csc_export(r, m, nullptr, exact(t2), nullptr, nullptr) != GKR_OK) return fail("terms alone", m);
        if (!terms.empty() && memcmp(t2.data(), terms.data(), terms.size() * sizeof(gkr_r1cs_term)) != 0) return fail("terms alone differ", m);
        if (gkr_r1cs_csc_export(r, m, nullptr, nullptr, exact(lc2), nullptr) != GKR_OK || lc2 != long_cols) return fail("long_cols alone", m);
        if (gkr_r1cs_csc_export(r, m, nullptr, nullptr, nullptr, nullptr) != GKR_OK) return fail("no output at all", m);
        if (col_ptr[0] != 0 || col_ptr[f.n_wires] != terms.size()) return fail("col_ptr ends", m);
        // a stable counting sort of the CSR records by wire, restated
        std::vector<uint32_t> next(col_ptr.begin(), col_ptr.end() - 1);
        for (size_t i = 0; i < nc; ++i)
            for (uint32_t t = row_ptr[i]; t < row_ptr[i + 1]; ++t) {
                const gkr_r1cs_term& rec = csr_terms[t];
                if (rec.wire >= f.n_wires) return fail("CSR wire", m, t);
                const uint32_t at = next[rec.wire]++;
                if (at >= col_ptr[rec.wire + 1]) return fail("column overflows", m, rec.wire);
                if (terms[at].wire != i || terms[at].coeff != rec.coeff) return fail("record", m, at);
            }
        size_t n_long = 0;
        for (uint32_t w = 0; w < f.n_wires; ++w) {
            if (next[w] != col_ptr[w + 1]) return fail("column underfull", m, w);
            const size_t len = col_ptr[w + 1] - col_ptr[w];
            if (w < n_want && len != want_len[w][m]) return fail("column length", m, w);
            if (len > GKR_R1CS_LONG_COL) {
                if (n_long >= long_cols.size() || long_cols[n_long] != w) return fail("long column list", m, w);
                ++n_long;
            }
        }
        if (n_long != long_cols.size()) return fail("long column count", m);
    }
    if (gkr_r1cs_csc_export(r, 3, nullptr, nullptr, nullptr, nullptr) != GKR_ERR_INVALID || gkr_r1cs_csc_export(r, -1, nullptr, nullptr, nullptr, nullptr) != GKR_ERR_INVALID)
        return fail("matrix outside 0 .. 2");
    gkr_r1cs_free(r);
    return 0;
}

}  // namespace

int main() {
    // 1. the hand-built system of tests/test_r1cs_cols_host.py
    Flat hand;
    hand.n_wires = 8;
    for (uint32_t i = 0; i < 33; ++i) {
        std::vector<std::pair<gkr_fr, uint32_t>> a = {{small(1), 0}}, b = {{minus(1), 0}, {small(7), 1}}, c = {{small(0), 6}, {small(3 + i % 2), 0}, {small(1), 4 + i % 2}};
        if (i < 32) a.push_back({i % 2 ? small(5 + i) : minus(1), 1});
        a.push_back({small(0), 3});
        if (i == 7) b.push_back({small(9), 1});
        if (i == 5) {
            a.push_back({small(11), 2});
            a.push_back({small(1), 3});
            a.push_back({small(12), 2});
        }
        hand.row(a);
        hand.row(b);
        hand.row(c);
    }
    const size_t want[8][3] = {{33, 33, 33}, {GKR_R1CS_LONG_COL, GKR_R1CS_LONG_COL + 2, 0}, {2, 0, 0}, {1, 0, 0}, {0, 0, 17}, {0, 0, 16}, {0, 0, 0}, {0, 0, 0}};
    if (check(hand, want, 8)) return 1;
    // 2. one wire
    Flat one;
    one.n_wires = 1;
    for (uint32_t i = 0; i < 5; ++i) {
        one.row({{small(1), 0}});
        one.row({{small(2), 0}, {minus(1), 0}});
        one.row({{small(i + 3), 0}});
    }
    const size_t want_one[1][3] = {{5, 10, 5}};
    if (check(one, want_one, 1)) return 1;
    // the refusals that need no large system
    gkr_r1cs* empty = nullptr;
    gkr_r1cs_csc_info_t ci;
    if (gkr_r1cs_build(4, 1, 1, 1, 0, nullptr, nullptr, nullptr, &empty) != GKR_OK) return fail("build of the empty system");
    if (gkr_r1cs_csc_info(empty, &ci) != GKR_ERR_INVALID || gkr_r1cs_csc_info(nullptr, &ci) != GKR_ERR_INVALID) return fail("n_constraints == 0");
    if (gkr_r1cs_csc_export(empty, 0, nullptr, nullptr, nullptr, nullptr) != GKR_ERR_INVALID) return fail("export of the empty system");
    gkr_r1cs_free(empty);
    printf("r1cs_csc_selfcheck: ok\n");
    return 0;
}

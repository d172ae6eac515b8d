// Stand-alone check of the grand product's chain of claims (gkr_amd/csrc/tree_rounds.h with the gate of grand_product_rounds.h:
// pre_relations, verdict and the Fiat-Shamir steps the driver shares with them) without a device or a context, meant to be built under
// -fsanitize=address,undefined (tests/test_grand_product_host.py; make -C gkr_amd/csrc asan_gp):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/grand_product_rounds_selfcheck.cpp gkr_amd/csrc/keccak.cpp
// Proofs over tables of 2^3 .. 2^6 values are made here by a plain prover -- the tree, then per layer the zero-check's round
// polynomials summed entry by entry -- with the UNUSED leading slots of every row filled with r (not canonical: they must never be
// read) and every array allocated at its exact size.  The honest proof passes and its last claim is V~(z^(n)); one change at a
// time gives the verdict the header states for its position.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../gkr_amd/csrc/grand_product_rounds.h"
#include "../gkr_amd/csrc/keccak.h"
#include "../gkr_amd/csrc/mimc7.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
namespace T = gkr::tree;
using Gate = gkr::gp::Gate;
using gkr::h64::add;
using gkr::h64::sub;
using T::mul;

F g_cts[gkr::kMimcRounds];
size_t g_hashes = 0;   // multi-hash calls so far
const F kZero = {{0, 0, 0, 0}}, kOne = {{1, 0, 0, 0}};

F hash(const F* v, int n) {
    ++g_hashes;
    return gkr::h64::mimc7_multi_hash(v, n, g_cts, nullptr);
}
gkr_fr modulus() {
    gkr_fr x;
    memcpy(x.l, gkr::h64::kMod, 32);
    return x;
}
gkr_fr plus_one(const gkr_fr& x) { return T::abi(add(V::load(x), kOne)); }

struct Made {
    int n = 0;
    std::vector<F> table;
    gkr_fr product{};
    std::vector<gkr_fr> head, coeffs, r, evals;
    std::vector<uint32_t> len;
    T::Proof view(bool with_product) const { return T::Proof{with_product ? &product : nullptr, head.data(), coeffs.data(), r.data(), evals.data(), len.data()}; }
};

std::vector<F> eq_table(const std::vector<F>& z, size_t from) {
    std::vector<F> t{kOne};
    for (size_t j = from; j < z.size(); ++j) {
        std::vector<F> u;
        for (const F& v : t) {
            u.push_back(mul(v, sub(kOne, z[j])));
            u.push_back(mul(v, z[j]));
        }
        t.swap(u);
    }
    return t;
}

F mle(std::vector<F> t, const gkr_fr* point, int n) {
    for (int j = 0; j < n; ++j) {
        const size_t h = t.size() / 2;
        for (size_t i = 0; i < h; ++i) t[i] = T::lerp(t[i], t[i + h], V::load(point[j]));
        t.resize(h);
    }
    return t[0];
}

Made make(int n, int kind, uint64_t seed) {
    Made m;
    m.n = n;
    F x = {{seed, seed * 5 + 3, seed * 11 + 7, 0x2345}};
    for (size_t i = 0; i < ((size_t)1 << n); ++i) {
        x = add(mul(x, x), F{{(uint64_t)i + 1, 0, 0, 0}});
        m.table.push_back(kind == 1 && i >= ((size_t)1 << (n - 1)) ? kZero : x);
    }
    std::vector<std::vector<F>> level((size_t)n + 1);
    level[n] = m.table;
    for (int k = n - 1; k >= 0; --k)
        for (size_t i = 0; i < ((size_t)1 << k); ++i) level[k].push_back(mul(level[k + 1][i], level[k + 1][i + ((size_t)1 << k)]));
    m.product = T::abi(level[0][0]);
    for (const F& v : level[2]) m.head.push_back(T::abi(v));
    const size_t R = T::rounds(n);
    m.coeffs.assign(R * 4, modulus());
    m.r.resize(R);
    m.len.resize(R);
    m.evals.resize(2 * (size_t)(n - 2));
    gkr_fr z2[2];
    T::head_link<Gate>(m.head.data(), hash, z2);
    std::vector<F> z{V::load(z2[0]), V::load(z2[1])};
    for (int k = 2; k < n; ++k) {
        const size_t half = (size_t)1 << k, row = T::layer_row(k);
        std::vector<F> A(level[k + 1].begin(), level[k + 1].begin() + half), B(level[k + 1].begin() + half, level[k + 1].end());
        F s = kOne;
        for (int j = 0; j < k; ++j) {
            const std::vector<F> w = eq_table(z, (size_t)j + 1);
            const size_t h = A.size() / 2;
            F c0 = kZero, c1 = kZero, c2 = kZero;
            for (size_t i = 0; i < h; ++i) {
                const F dA = sub(A[i + h], A[i]), dB = sub(B[i + h], B[i]);
                c0 = add(c0, mul(w[i], mul(A[i], B[i])));
                c1 = add(c1, mul(w[i], add(mul(A[i], dB), mul(dA, B[i]))));
                c2 = add(c2, mul(w[i], mul(dA, dB)));
            }
            const F a = mul(s, sub(kOne, z[j])), b = mul(s, sub(add(z[j], z[j]), kOne));
            const F g[4] = {mul(b, c2), add(mul(a, c2), mul(b, c1)), add(mul(a, c1), mul(b, c0)), mul(a, c0)};   // highest degree first
            uint32_t lead = 0;
            while (lead < 3 && gkr::h64::is_zero(g[lead])) ++lead;
            m.len[row + j] = 4 - lead;
            for (uint32_t t = lead; t < 4; ++t) m.coeffs[4 * (row + j) + t] = T::abi(g[t]);
            const F rj = hash(g + lead, (int)(4 - lead));
            m.r[row + j] = T::abi(rj);
            s = add(a, mul(b, rj));
            for (size_t i = 0; i < h; ++i) {
                A[i] = T::lerp(A[i], A[i + h], rj);
                B[i] = T::lerp(B[i], B[i + h], rj);
            }
            A.resize(h);
            B.resize(h);
        }
        m.evals[2 * (k - 2)] = T::abi(A[0]);
        m.evals[2 * (k - 2) + 1] = T::abi(B[0]);
        std::vector<gkr_fr> zn((size_t)k + 1);
        T::next_link<Gate>(k, m.evals.data() + 2 * (k - 2), m.r.data() + row, hash, zn.data());
        z.clear();
        for (const gkr_fr& c : zn) z.push_back(V::load(c));
    }
    return m;
}

struct Got {
    int check, layer, round;
    bool operator==(const Got& o) const { return check == o.check && layer == o.layer && round == o.round; }
};

// the verdict of a proof against its own table (value: V~(z^(n)) where the proof has a point, else zero); check -1: a missing hash
Got run(const Made& m, bool with_product, bool hashes = true) {
    const T::Proof p = m.view(with_product);
    const T::Pre<Gate> pre = T::pre_relations<Gate>(m.n, p, hash);
    const size_t R = T::rounds(m.n);
    std::vector<V::HashSlot> slots(R);
    for (size_t s = 0; s < R; ++s) {
        slots[s].valid = 0;
        if (hashes) V::hash_slot(m.coeffs.data() + 4 * s, 4u, m.len[s], &slots[s], hash);
    }
    const F value = pre.point ? mle(m.table, pre.z.data() + T::layer_row(m.n), m.n) : kZero;
    T::Verdict v;
    if (!T::verdict<Gate>(m.n, p, pre, slots.data(), &value, &v)) return Got{-1, 0, 0};
    return Got{(int)v.check, (int)v.layer, (int)v.round};
}

int fail(const char* what, int n, int kind, int a, int b) {
    printf("grand_product_rounds_selfcheck: FAILED: %s (n %d, table %d, at %d, %d)\n", what, n, kind, a, b);
    return 1;
}

}  // namespace

int main() {
    {
        gkr::Fr cts[gkr::kMimcRounds];
        gkr::mimc7_make_constants(cts);
        static_assert(sizeof(cts) == sizeof(g_cts), "the same 91 constants in both limb widths");
        memcpy(g_cts, cts, sizeof cts);
    }
    const Got ok{0, 0, 0};
    int cases = 0;
    for (int n = 3; n <= 6; ++n)
        for (int kind = 0; kind < 2; ++kind) {   // 0: a sharp table; 1: the upper half zero (every vector [0], lengths 1)
            const Made m = make(n, kind, (uint64_t)(1000 * n + kind));
            if (!(run(m, true) == ok) || !(run(m, false) == ok)) return fail("the honest proof is rejected", n, kind, run(m, true).check, 0);
            if (!(run(m, true, false) == Got{-1, 0, 0})) return fail("a missing hash goes unnoticed", n, kind, 0, 0);
            F root;
            Gate::root(m.head.data(), &root);
            if (!V::same(V::load(m.product), root)) return fail("the head's product", n, kind, 0, 0);
            {   // the chain's hashes: the head's two and one tau per layer -- no lambda is drawn
                const size_t before = g_hashes;
                T::pre_relations<Gate>(n, m.view(true), hash);
                if (g_hashes - before != 2 + (size_t)(n - 2)) return fail("the number of multi-hash calls of pre_relations", n, kind, (int)(g_hashes - before), 0);
            }
            {   // another table: the chain holds, the evaluation does not
                Made u = m;
                u.table[1] = add(u.table[1], kOne);
                if (!(run(u, true) == Got{GKR_VERIFY_EVALUATION, n, n})) return fail("a changed table entry", n, kind, 1, 0);
            }
            for (int t = 0; t < 4; ++t) {
                Made u = m;
                u.head[t] = plus_one(u.head[t]);
                const Got want = kind == 0 ? Got{GKR_VERIFY_PRODUCT, 0, 0} : Got{GKR_VERIFY_ROUND_SUM, 2, 0};   // (table 1: the other three are zero)
                if (!(run(u, true) == want)) return fail("a changed head entry, product claimed", n, kind, t, 0);
                if (!(run(u, false) == Got{GKR_VERIFY_ROUND_SUM, 2, 0})) return fail("a changed head entry", n, kind, t, 0);
                u.head[t] = modulus();
                if (!(run(u, true) == Got{GKR_VERIFY_NON_CANONICAL, 0, 0})) return fail("a head entry >= r", n, kind, t, 0);
            }
            {
                Made u = m;
                u.product = plus_one(u.product);
                if (!(run(u, true) == Got{GKR_VERIFY_PRODUCT, 0, 0}) || !(run(u, false) == ok)) return fail("a changed product", n, kind, 0, 0);
                u.product = modulus();
                if (!(run(u, true) == Got{GKR_VERIFY_NON_CANONICAL, 0, 0})) return fail("a product >= r", n, kind, 0, 0);
            }
            for (int k = 2; k < n; ++k) {
                for (int j = 0; j < k; ++j) {
                    const size_t row = T::layer_row(k) + (size_t)j;
                    for (uint32_t t = 4 - m.len[row]; t < 4; ++t) {
                        Made u = m;
                        u.coeffs[4 * row + t] = plus_one(u.coeffs[4 * row + t]);
                        if (!(run(u, true) == Got{GKR_VERIFY_ROUND_SUM, k, j})) return fail("a changed slot", n, kind, k, j);
                        u.coeffs[4 * row + t] = modulus();
                        if (!(run(u, true) == Got{GKR_VERIFY_NON_CANONICAL, k, j})) return fail("a slot >= r", n, kind, k, j);
                    }
                    Made u = m;
                    u.r[row] = plus_one(u.r[row]);
                    if (!(run(u, true) == Got{GKR_VERIFY_CHALLENGE, k, j})) return fail("a changed challenge", n, kind, k, j);
                    u.r[row] = modulus();
                    if (!(run(u, true) == Got{GKR_VERIFY_NON_CANONICAL, k, j})) return fail("a challenge >= r", n, kind, k, j);
                    for (const uint32_t bad : {0u, 5u, 0xFFFFFFFFu}) {
                        u = m;
                        u.len[row] = bad;
                        if (!(run(u, true) == Got{GKR_VERIFY_SHAPE, k, j})) return fail("a length outside 1 .. 4", n, kind, k, j);
                    }
                }
                for (int w = 0; w < 2; ++w) {
                    Made u = m;
                    gkr_fr& e = u.evals[2 * (k - 2) + w];
                    e = plus_one(e);
                    Got want{GKR_VERIFY_FINAL_CLAIM, k, k};
                    if (gkr::h64::is_zero(V::load(m.evals[2 * (k - 2) + 1 - w])))   // the other value is zero: the next claim moves instead
                        want = k < n - 1 ? Got{GKR_VERIFY_ROUND_SUM, k + 1, 0} : Got{GKR_VERIFY_EVALUATION, n, n};
                    if (!(run(u, true) == want)) return fail("a changed value", n, kind, k, w);
                    e = modulus();
                    if (!(run(u, true) == Got{GKR_VERIFY_NON_CANONICAL, k, k})) return fail("a value >= r", n, kind, k, w);
                }
            }
            ++cases;
        }
    printf("grand_product_rounds_selfcheck: ok (%d proofs)\n", cases);
    return 0;
}

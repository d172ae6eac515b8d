// Stand-alone check of the fractional sum's chain of claims (gkr_amd/csrc/tree_rounds.h with the gate of fraction_sum_rounds.h:
// pre_relations, verdict and the Fiat-Shamir steps the driver shares with them) without a device or a context, meant to be built under
// -fsanitize=address,undefined (tests/test_fraction_sum_host.py; make -C gkr_amd/csrc asan_fs):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/fraction_sum_rounds_selfcheck.cpp gkr_amd/csrc/keccak.cpp
//   ./a.out CASES
// CASES is a text file the test writes from the integer model (tests/fraction_sum_model.py): proofs and single-element changes of
// them with the verdict each must get.  Per case, tokens separated by white space, field elements as 64 hex digits:
//   case N WITH_SUMS HONEST CHECK LAYER ROUND
//   sums[2] head[8] coeffs[R * 4] len[R] r[R] evals[(N - 2) * 4] numerators[2^N] denominators[2^N]
//   and for an honest case: P Q point[N] cp_N cq_N
// Every array is allocated at its exact size; the values N~(z^(n)), D~(z^(n)) are computed here from the tables at the point the
// relations produce.  The verdict must be the case's; an honest case's root, point and end claims must be the model's.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "../gkr_amd/csrc/fraction_sum_rounds.h"
#include "../gkr_amd/csrc/keccak.h"
#include "../gkr_amd/csrc/mimc7.h"

namespace {

using gkr::h64::F;
namespace V = gkr::verify;
namespace T = gkr::tree;
using Gate = gkr::fs::Gate;

F g_cts[gkr::kMimcRounds];
size_t g_hashes = 0;   // multi-hash calls so far
const F kZero = {{0, 0, 0, 0}};

F hash(const F* v, int n) {
    ++g_hashes;
    return gkr::h64::mimc7_multi_hash(v, n, g_cts, nullptr);
}

bool read_fr(std::ifstream& in, gkr_fr* out) {
    std::string s;
    if (!(in >> s) || s.size() != 64) return false;
    for (int limb = 0; limb < 4; ++limb) out->l[3 - limb] = strtoull(s.substr(16 * (size_t)limb, 16).c_str(), nullptr, 16);
    return true;
}
bool read_frs(std::ifstream& in, size_t count, std::vector<gkr_fr>* out) {
    out->resize(count);
    for (gkr_fr& x : *out)
        if (!read_fr(in, &x)) return false;
    return true;
}
bool same(const gkr_fr& a, const gkr_fr& b) { return memcmp(a.l, b.l, 32) == 0; }

F reduced(gkr_fr x) {   // a 256-bit integer modulo r
    while (!V::canonical(x)) {
        unsigned __int128 borrow = 0;
        for (int i = 0; i < 4; ++i) {
            const unsigned __int128 d = (unsigned __int128)x.l[i] - gkr::h64::kMod[i] - borrow;
            x.l[i] = (uint64_t)d;
            borrow = (d >> 64) & 1;
        }
    }
    return V::load(x);
}

F mle(const std::vector<gkr_fr>& table, const gkr_fr* point, int n) {   // entries read modulo r
    std::vector<F> t;
    for (const gkr_fr& x : table) t.push_back(reduced(x));
    for (int j = 0; j < n; ++j) {
        const size_t h = t.size() / 2;
        for (size_t i = 0; i < h; ++i) t[i] = T::lerp(t[i], t[i + h], V::load(point[j]));
        t.resize(h);
    }
    return t[0];
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        printf("usage: fraction_sum_rounds_selfcheck CASES\n");
        return 2;
    }
    {
        gkr::Fr cts[gkr::kMimcRounds];
        gkr::mimc7_make_constants(cts);
        static_assert(sizeof(cts) == sizeof(g_cts), "the same 91 constants in both limb widths");
        memcpy(g_cts, cts, sizeof cts);
    }
    std::ifstream in(argv[1]);
    std::string word;
    int cases = 0, honest_cases = 0;
    while (in >> word) {
        int n = 0, with_sums = 0, honest = 0, check = 0, layer = 0, round = 0;
        if (word != "case" || !(in >> n >> with_sums >> honest >> check >> layer >> round) || n < 3 || n > 12) {
            printf("fraction_sum_rounds_selfcheck: FAILED: case %d is malformed\n", cases);
            return 1;
        }
        const size_t R = T::rounds(n), size = (size_t)1 << n;
        std::vector<gkr_fr> sums, head, coeffs, r, evals, num, den;
        std::vector<uint32_t> len(R);
        bool ok = read_frs(in, 2, &sums) && read_frs(in, 8, &head) && read_frs(in, R * 4, &coeffs);
        for (size_t s = 0; ok && s < R; ++s) ok = (bool)(in >> len[s]);
        ok = ok && read_frs(in, R, &r) && read_frs(in, 4 * (size_t)(n - 2), &evals) && read_frs(in, size, &num) && read_frs(in, size, &den);
        std::vector<gkr_fr> want;   // P, Q, point, cp_n, cq_n
        if (honest) ok = ok && read_frs(in, (size_t)n + 4, &want);
        if (!ok) {
            printf("fraction_sum_rounds_selfcheck: FAILED: case %d is cut short\n", cases);
            return 1;
        }
        const T::Proof p{with_sums ? sums.data() : nullptr, head.data(), coeffs.data(), r.data(), evals.data(), len.data()};
        const size_t hashes_before = g_hashes;
        const T::Pre<Gate> pre = T::pre_relations<Gate>(n, p, hash);
        const size_t pre_hashes = g_hashes - hashes_before;
        std::vector<V::HashSlot> slots(R);
        for (size_t s = 0; s < R; ++s) V::hash_slot(coeffs.data() + 4 * s, 4u, len[s], &slots[s], hash);
        const F values[2] = {pre.point ? mle(num, pre.z.data() + T::layer_row(n), n) : kZero,
                             pre.point ? mle(den, pre.z.data() + T::layer_row(n), n) : kZero};
        T::Verdict v;
        if (!T::verdict<Gate>(n, p, pre, slots.data(), values, &v)) {
            printf("fraction_sum_rounds_selfcheck: FAILED: case %d: a well-formed round vector without a hash\n", cases);
            return 1;
        }
        if ((int)v.check != check || (int)v.layer != layer || (int)v.round != round) {
            printf("fraction_sum_rounds_selfcheck: FAILED: case %d (n %d): verdict (%u, %u, %u), expected (%d, %d, %d)\n", cases, n, v.check, v.layer,
                   v.round, check, layer, round);
            return 1;
        }
        if (honest) {
            F root[2];
            Gate::root(head.data(), root);
            bool good = pre.point && same(T::abi(root[0]), want[0]) && same(T::abi(root[1]), want[1]);
            good = good && pre_hashes == 3 + 2 * (size_t)(n - 2);   // the head's three, then tau and lambda per layer
            for (int j = 0; good && j < n; ++j) good = same(pre.z[T::layer_row(n) + (size_t)j], want[2 + (size_t)j]);
            good = good && pre.link.size() == (size_t)n - 1 && same(T::abi(pre.link.back().c[0]), want[(size_t)n + 2]) &&
                   same(T::abi(pre.link.back().c[1]), want[(size_t)n + 3]);
            if (check == 0) {   // a missing hash is an error of the call, not a verdict
                std::vector<V::HashSlot> none(R);
                for (V::HashSlot& s : none) s.valid = 0;
                T::Verdict u;
                good = good && !T::verdict<Gate>(n, p, pre, none.data(), values, &u);
            }
            if (!good) {
                printf("fraction_sum_rounds_selfcheck: FAILED: case %d (n %d): the honest proof's root, point, end claims or number of multi-hash calls\n", cases, n);
                return 1;
            }
            ++honest_cases;
        }
        ++cases;
    }
    if (cases == 0 || honest_cases == 0) {
        printf("fraction_sum_rounds_selfcheck: FAILED: no cases\n");
        return 1;
    }
    printf("fraction_sum_rounds_selfcheck: ok (%d cases, %d honest)\n", cases, honest_cases);
    return 0;
}

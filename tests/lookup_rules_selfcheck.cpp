// csrc/lookup_rules.h driven alone (no device, no library): the slot function h, the shapes the lookup calls admit and the verdict
// rule, on the cases tests/test_lookup_host.py writes out from the integer model (tests/lookup_model.py).  Built under
// AddressSanitizer and UBSan (make -C gkr_amd/csrc asan_lk, or the test's own g++ line).  One case per line:
//   slot <64 hex digits> <log_slots> <want>
//   shape <n_w> <n_t> <batch> <want L, 0: refused>
//   verdict <P, 64 hex digits> <check> <layer> <round> <want check> <want layer> <want round>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../gkr_amd/csrc/lookup_rules.h"

static bool parse_fr(const std::string& hex, gkr_fr* out) {
    if (hex.size() != 64) return false;
    for (int i = 0; i < 4; ++i) out->l[3 - i] = strtoull(hex.substr(16 * (size_t)i, 16).c_str(), nullptr, 16);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    size_t cases = 0, failed = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string kind, hex;
        ss >> kind;
        if (kind == "slot") {
            gkr_fr v;
            int log_slots = 0;
            unsigned long want = 0;
            ss >> hex >> log_slots >> want;
            if (!ss || !parse_fr(hex, &v)) return 2;
            uint32_t limbs[8];
            memcpy(limbs, &v, 32);
            const uint32_t got = gkr::lookup::slot_of(limbs, (uint32_t)log_slots);
            if (got != want) {
                printf("slot %s %d: got %u, want %lu\n", hex.c_str(), log_slots, got, want);
                ++failed;
            }
        } else if (kind == "shape") {
            int n_w = 0, n_t = 0, batch = 0, want = 0;
            ss >> n_w >> n_t >> batch >> want;
            if (!ss) return 2;
            if (gkr::lookup::pair_log2(n_w, n_t, batch) != want) {
                printf("shape %d %d %d: got %d, want %d\n", n_w, n_t, batch, gkr::lookup::pair_log2(n_w, n_t, batch), want);
                ++failed;
            }
        } else if (kind == "verdict") {
            gkr_fr root[2] = {};
            uint32_t check = 0, layer = 0, round = 0, wc = 0, wl = 0, wr = 0;
            ss >> hex >> check >> layer >> round >> wc >> wl >> wr;
            if (!ss || !parse_fr(hex, &root[0])) return 2;
            root[1].l[0] = 1;
            int accept = check == 0 ? 1 : 0;
            gkr::lookup::verdict(root, &accept, &layer, &round, &check);
            if (check != wc || layer != wl || round != wr || accept != (wc == 0 ? 1 : 0)) {
                printf("verdict %s: got (%u, %u, %u) accept %d, want (%u, %u, %u)\n", hex.c_str(), check, layer, round, accept, wc, wl, wr);
                ++failed;
            }
        } else if (!kind.empty()) {
            return 2;
        }
        cases += !kind.empty();
    }
    if (failed || !cases) {
        printf("lookup_rules_selfcheck: %zu of %zu cases FAILED\n", failed, cases);
        return 1;
    }
    printf("lookup_rules_selfcheck: ok (%zu cases)\n", cases);
    return 0;
}

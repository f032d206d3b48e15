// Host-only harness around headtrackr_amd/csrc/ht_bp_pairs_plan.h (the group plan of ht_camshift_backproject_pairs), built by
// tests/test_bp_pairs_cpu.py with g++ -fsanitize=address,undefined.
//
//   bp_pairs_plan_harness <cases>   one case per line: G followed by the frame of every pair, in call order; one JSON object per line out:
//       {"groups": [{"frame": f, "slot": s, "count": c, "pairs": [..]}, ...]}
//   The slots (index of a frame among the distinct frames, by first appearance) are derived here the way csp_plan derives them.  The
//   invariants the kernels rely on without checking them are asserted here as well: every pair in exactly one group, 1 <= count <= G, the
//   pairs of a group name the group's frame and ascend, unused entries are -1.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "ht_bp_pairs_plan.h"

static std::string g_case;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s: %s: ", g_case.c_str(), #cond);  \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, "\n");                                \
            exit(3);                                              \
        }                                                         \
    } while (0)

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    while (std::getline(in, g_case)) {
        if (g_case.empty()) continue;
        std::istringstream ls(g_case);
        int G = 0;
        ls >> G;
        std::vector<int32_t> frames, slots;
        std::map<int32_t, int32_t> slot_of;
        for (int32_t f; ls >> f;) {
            if (!slot_of.count(f)) {
                const int32_t s = (int32_t)slot_of.size();
                slot_of[f] = s;
            }
            frames.push_back(f);
            slots.push_back(slot_of[f]);
        }
        const int32_t n = (int32_t)frames.size();
        // exactly-sized heap copies: a read past either end is a sanitizer report
        std::vector<int32_t> fr(frames.begin(), frames.end()), sl(slots.begin(), slots.end());
        const std::vector<HtBppGroup> groups = ht_bpp_plan(fr.data(), sl.data(), n, G);
        if (G < 1 || G > BPP_MAXG || n == 0) CHECK(groups.empty(), "%zu groups", groups.size());
        std::vector<int> seen((size_t)n, 0);
        int32_t last_first = -1;
        for (const HtBppGroup &g : groups) {
            CHECK(g.count >= 1 && g.count <= G, "count %d", g.count);
            CHECK(g.pad == 0, "pad %d", g.pad);
            CHECK(g.pair[0] > last_first, "group order: %d after %d", g.pair[0], last_first);
            last_first = g.pair[0];
            for (int q = 0; q < BPP_MAXG; q++) {
                if (q >= g.count) {
                    CHECK(g.pair[q] == -1, "unused entry %d", g.pair[q]);
                    continue;
                }
                const int32_t i = g.pair[q];
                CHECK(i >= 0 && i < n, "pair %d", i);
                CHECK(q == 0 || i > g.pair[q - 1], "pairs of a group ascend: %d after %d", i, g.pair[q - 1]);
                CHECK(frames[(size_t)i] == g.frame && slots[(size_t)i] == g.slot, "pair %d: frame %d slot %d in a group of frame %d slot %d", i, frames[(size_t)i],
                      slots[(size_t)i], g.frame, g.slot);
                seen[(size_t)i]++;
            }
        }
        if (G >= 1 && G <= BPP_MAXG)
            for (int32_t i = 0; i < n; i++) CHECK(seen[(size_t)i] == 1, "pair %d is in %d groups", i, seen[(size_t)i]);
        printf("{\"groups\": [");
        for (size_t k = 0; k < groups.size(); k++) {
            const HtBppGroup &g = groups[k];
            printf("%s{\"frame\": %d, \"slot\": %d, \"count\": %d, \"pairs\": [", k ? ", " : "", g.frame, g.slot, g.count);
            for (int q = 0; q < g.count; q++) printf("%s%d", q ? ", " : "", g.pair[q]);
            printf("]}");
        }
        printf("]}\n");
    }
    return 0;
}

// ht_bp_pairs_plan.h — the group plan of ht_camshift_backproject_pairs, without HIP: which pairs of a call share one pass over a frame.
// A GROUP is up to G pairs of the call that name the same frame; one k_bpp_project workgroup row reads the frame's pixels once and
// writes every output of its group (G = 4 LUTs of RGBA8 pixels or 2 LUTs of binary64 weights fill the 64 KB of LDS a workgroup may
// declare).  ht_bp_pairs.hip uploads the records this function writes as they are; the kernels index them by blockIdx.y.  Plain C++17:
// the CPU suite compiles this header alone (tests/host/bp_pairs_plan_harness.cc) with AddressSanitizer + UBSan.
#pragma once

#include <stdint.h>

#include <vector>

constexpr int BPP_MAXG = 4;  // pairs per group at most (HT_BP_RGBA8); HT_BP_F64 takes 2

struct HtBppGroup {
    int32_t frame;           // the bound frame every pair of the group names
    int32_t slot;            // its index among the call's distinct frames = its chunk histograms in the scratch
    int32_t count;           // pairs of the group: 1 .. G
    int32_t pad;
    int32_t pair[BPP_MAXG];  // their positions in the call (= LUT slot = output index), ascending; unused entries are -1
};
static_assert(sizeof(HtBppGroup) == 32, "HtBppGroup");

// pair i names frame frames[i], which is distinct frame slots[i] of the call.  Groups come in the order in which their first pair
// appears in the call; a pair joins the open group of its frame, and a frame opens a new group when its open one holds G pairs.
// Every pair is in exactly one group.  G outside 1 .. BPP_MAXG or a negative slot: no groups.
inline std::vector<HtBppGroup> ht_bpp_plan(const int32_t *frames, const int32_t *slots, int32_t n, int G) {
    std::vector<HtBppGroup> groups;
    if (G < 1 || G > BPP_MAXG || n <= 0) return groups;
    std::vector<int32_t> open;  // per slot: index of the group that still has room, or -1
    for (int32_t i = 0; i < n; i++) {
        const int32_t s = slots[i];
        if (s < 0) return std::vector<HtBppGroup>();
        if ((size_t)s >= open.size()) open.resize((size_t)s + 1, -1);
        if (open[(size_t)s] < 0) {
            open[(size_t)s] = (int32_t)groups.size();
            groups.push_back(HtBppGroup{frames[i], s, 0, 0, {-1, -1, -1, -1}});
        }
        HtBppGroup &g = groups[(size_t)open[(size_t)s]];
        g.pair[g.count++] = i;
        if (g.count == G) open[(size_t)s] = -1;
    }
    return groups;
}

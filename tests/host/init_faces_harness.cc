// init_faces_harness.cc — the rule and the host plan of ht_camshift_init_faces (headtrackr_amd/csrc/ht_cs_faces_plan.h: the predicates,
// the overlap and the slot fill are the very lines k_csf_resolve compiles for the device) on the host, plain and under AddressSanitizer +
// UBSan (tests/test_init_faces_cpu.py builds and runs it).
//   init_faces_harness in.bin out.bin
// in.bin: a sequence of cases, each led by an int32 tag.
//   tag 1, a frame: {i32 k, m; u32 flags, status, nhits, bad, hit_capacity; i32 collected; f64 min_confidence}, m ht_rect, k windows of 4 i32
//          -> k ht_csf_record
//   tag 2, a plan:  {i32 n, grouped; u32 flags; i32 pad; f64 min_confidence}, n ht_cs_pair (a list that has passed csp_plan: n >= 1)
//          -> i32 status, i32 ngroups, 3 i32 per group, n i32 order (status != 0: ngroups = 0 and nothing else)
#include <cstdio>
#include <cstring>
#include <vector>

#include "ht_cs_faces_plan.h"

struct FrameHead {
    int32_t k, m;
    uint32_t flags, status, nhits, bad, hit_capacity;
    int32_t collected;
    double min_confidence;
};
static_assert(sizeof(FrameHead) == 40, "FrameHead");
struct PlanHead {
    int32_t n, grouped;
    uint32_t flags;
    int32_t pad;
    double min_confidence;
};
static_assert(sizeof(PlanHead) == 24, "PlanHead");

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<int32_t> out;
    size_t frames = 0, plans = 0, refused = 0;
    int32_t tag;
    while (std::fread(&tag, sizeof(tag), 1, f) == 1) {
        if (tag == 1) {
            FrameHead h;
            if (std::fread(&h, sizeof(h), 1, f) != 1 || h.k < 1 || h.k > HT_CSF_MAX_SLOTS || h.m < 0) return 6;
            // exactly as large as the inputs are: a read behind either is the sanitizer's to find
            std::vector<ht_rect> G((size_t)h.m);
            std::vector<int32_t> sw((size_t)h.k * 4);
            if (h.m && std::fread(G.data(), sizeof(ht_rect), G.size(), f) != G.size()) return 6;
            if (std::fread(sw.data(), sizeof(int32_t), sw.size(), f) != sw.size()) return 6;
            std::vector<ht_csf_record> rec((size_t)h.k);
            std::memset(rec.data(), 0xff, rec.size() * sizeof(ht_csf_record));
            ht_csf_frame(G.data(), (uint32_t)h.m, sw.data(), h.k, ht_csf_not_final(h.status, h.nhits, h.bad, h.hit_capacity, h.collected != 0), h.min_confidence, h.flags,
                         rec.data());
            const int32_t *w = reinterpret_cast<const int32_t *>(rec.data());
            out.insert(out.end(), w, w + rec.size() * 8);
            frames++;
        } else if (tag == 2) {
            PlanHead h;
            if (std::fread(&h, sizeof(h), 1, f) != 1 || h.n < 1) return 7;
            std::vector<ht_cs_pair> pairs((size_t)h.n);
            if (h.n && std::fread(pairs.data(), sizeof(ht_cs_pair), pairs.size(), f) != pairs.size()) return 7;
            HtCsfPlan plan;
            std::string why;
            const ht_status st = ht_csf_plan(pairs.data(), h.n, h.grouped, h.min_confidence, h.flags, &plan, &why);
            out.push_back((int32_t)st);
            if (st != HT_OK) {
                if (why.empty()) return 8;  // every refusal says why
                out.push_back(0);
                refused++;
            } else {
                out.push_back(plan.ngroups());
                out.insert(out.end(), plan.groups.begin(), plan.groups.end());
                out.insert(out.end(), plan.order.begin(), plan.order.end());
            }
            plans++;
        } else {
            return 9;
        }
    }
    std::fclose(f);
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(int32_t), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("frames %zu plans %zu refused %zu\n", frames, plans, refused);
    return ok ? 0 : 5;
}

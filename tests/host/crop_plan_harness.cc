// crop_plan_harness.cc — the rule of the face crops (headtrackr_amd/csrc/ht_crop_plan.h: the very lines k_crop_list compiles for the device)
// on the host, plain and under AddressSanitizer + UBSan (tests/test_crop_cpu.py builds and runs it).
//   crop_plan_harness in.bin out.bin
// in.bin: cases of 80 bytes {f64 x, y, width, height; i32 W, H, SW, SH, mx, my, mw, mh, margin_q8; u32 flags; i32 pad[2]}
// out.bin: per case i32 code, i32 rect[4]
#include <cstdio>
#include <vector>

#include "ht_crop_plan.h"

struct Case {
    double x, y, width, height;
    int32_t W, H, SW, SH, mx, my, mw, mh, margin_q8;
    uint32_t flags;
    int32_t pad[2];
};
static_assert(sizeof(Case) == 80, "Case");
static_assert(sizeof(ht_crop_record) == 40 && sizeof(ht_crop_params) == 16, "the C ABI's structs");

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Case> cases;
    Case c;
    while (std::fread(&c, sizeof(c), 1, f) == 1) cases.push_back(c);
    std::fclose(f);
    std::vector<int32_t> out;
    out.reserve(cases.size() * 5);
    for (const Case &k : cases) {
        ht_cs_rect r = {-1, -1, -1, -1};
        const int32_t code = ht_crop_rule(k.x, k.y, k.width, k.height, k.W, k.H, k.SW, k.SH, k.mx, k.my, k.mw, k.mh, k.margin_q8, k.flags, &r);
        out.push_back(code);
        out.push_back(r.x), out.push_back(r.y), out.push_back(r.width), out.push_back(r.height);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(int32_t), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("cases %zu\n", cases.size());
    return ok ? 0 : 5;
}

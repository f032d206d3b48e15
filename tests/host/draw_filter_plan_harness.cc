// draw_filter_plan_harness.cc — the host plan of ht_draw_list_filtered_device (headtrackr_amd/csrc/ht_draw_filter_plan.h) as a program of
// its own, plain and under AddressSanitizer + UBSan (tests/test_draw_filter_cpu.py builds and runs it).  Plane pointers are numbers here:
// the plan never dereferences them.
//   draw_filter_plan_harness in.bin out.bin
// in.bin: cases of 88 bytes {u64 p0, p1, p2, pitch0, pitch1; i32 W, H, max_factor, width, height, format, matrix, rx, ry, rw, rh, lead}: ONE
//         call of ht_draw_filter_plan on a W x H canvas whose list is `lead` copies of a good entry (NV12 23 x 23) and then the case's entry
// out.bin: per case 13 i64: status, bad, and — status 0, of the LAST descriptor — Nx, Ny, the bits of rx and ry, sx, sy, sw, sh, pitch0, pitch1,
//          cw (zeros otherwise).  The descriptor and extent arrays hold exactly lead + 1 entries: a write past them is a sanitizer report, and
//          so is a descriptor the plan left unwritten (the arrays are filled with 0xEE, and a refused entry must still hold it)
#include <cstdio>
#include <cstring>
#include <vector>

#include "ht_draw_filter_plan.h"

struct Case {
    uint64_t p0, p1, p2, pitch0, pitch1;
    int32_t W, H, max_factor, width, height, format, matrix, rx, ry, rw, rh, lead;
};
static_assert(sizeof(Case) == 88, "Case");

static const void *ptr_of(uint64_t v) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(v)); }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Case> cases;
    Case c;
    while (std::fread(&c, sizeof(c), 1, f) == 1) cases.push_back(c);
    std::fclose(f);
    std::vector<int64_t> out;
    out.reserve(cases.size() * 13);
    for (const Case &k : cases) {
        if (k.lead < 0 || k.lead > 1000) return 6;
        ht_draw_source good;
        std::memset(&good, 0, sizeof(good));
        good.p0 = ptr_of(0x10000), good.p1 = ptr_of(0x90000), good.width = good.height = 23, good.format = HT_YUV_FMT_NV12;
        ht_draw_source s;
        std::memset(&s, 0, sizeof(s));
        s.p0 = ptr_of(k.p0), s.p1 = ptr_of(k.p1), s.p2 = ptr_of(k.p2), s.pitch0 = (size_t)k.pitch0, s.pitch1 = (size_t)k.pitch1;
        s.width = k.width, s.height = k.height, s.format = k.format, s.matrix = k.matrix;
        s.rect = ht_cs_rect{k.rx, k.ry, k.rw, k.rh};
        std::vector<ht_draw_source> srcs((size_t)k.lead, good);
        srcs.push_back(s);
        const size_t n = srcs.size();
        std::vector<HtDrawMeanDesc> desc(n);
        std::vector<HtDrawExtent> ext(n);
        std::memset(desc.data(), 0xEE, n * sizeof(HtDrawMeanDesc)), std::memset(ext.data(), 0xEE, n * sizeof(HtDrawExtent));
        int32_t bad = -7;
        const int st = ht_draw_filter_plan(srcs.data(), (int32_t)n, k.W, k.H, k.max_factor, desc.data(), ext.data(), &bad);
        if (std::strlen(ht_draw_filter_message(st)) < 8 && st != HT_DRAW_LIST_OK) return 7;
        const HtDrawMeanDesc &m = desc[n - 1];
        out.push_back(st), out.push_back(bad);
        if (st == HT_DRAW_LIST_OK) {
            int64_t bx, by;
            std::memcpy(&bx, &m.d.rx, 8), std::memcpy(&by, &m.d.ry, 8);
            const int64_t v[11] = {m.nx, m.ny, bx, by, m.d.sx, m.d.sy, m.d.sw, m.d.sh, (int64_t)m.d.pitch0, (int64_t)m.d.pitch1, m.d.cw};
            out.insert(out.end(), v, v + 11);
        } else {
            const unsigned char *raw = reinterpret_cast<const unsigned char *>(&m);
            for (size_t b = 0; b < sizeof(m); b++)
                if (raw[b] != 0xEE) return 8;  // a refused entry's descriptor is not written
            out.insert(out.end(), 11, 0);
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(int64_t), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("cases %zu\n", cases.size());
    return ok ? 0 : 5;
}

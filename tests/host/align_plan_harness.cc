// align_plan_harness.cc — the rule of the aligned crops (headtrackr_amd/csrc/ht_align_plan.h: the very lines k_align_list compiles for the
// device) on the host, plain and under AddressSanitizer + UBSan (tests/test_align_cpu.py builds and runs it).
//   align_plan_harness in.bin out.bin
//   align_plan_harness --pixels in.bin out.bin
// in.bin: cases of 88 bytes {f64 x, y, width, height, angle; i32 W, H, SW, SH, mx, my, mw, mh, margin_q8; u32 flags; i32 P, Q}
// out.bin: per case i64 code, a12, Cx, Cy, UxS, UyS, VxS, VyS; then, if P > 0, the P column terms of x, the P of y, the Q row terms of x, the Q of y
// --pixels: in.bin holds samples of 40 bytes {i64 fx, fy; i32 SW, SH; u32 p00, p01, p10, p11}; out.bin per sample u32 inside (ht_align_inside),
// u32 pixel (the four ht_align_channel of the taps under tx, ty as the kernel forms them; 0 when outside)
#include <cstdio>
#include <cstring>
#include <vector>

#include "ht_align_plan.h"

struct Case {
    double x, y, width, height, angle;
    int32_t W, H, SW, SH, mx, my, mw, mh, margin_q8;
    uint32_t flags;
    int32_t P, Q;
};
static_assert(sizeof(Case) == 88, "Case");
static_assert(sizeof(ht_align_record) == 64 && sizeof(ht_align_params) == 16, "the C ABI's structs");

struct Sample {
    int64_t fx, fy;
    int32_t SW, SH;
    uint32_t p00, p01, p10, p11;
};
static_assert(sizeof(Sample) == 40, "Sample");

static int pixels(const char *in, const char *outname) {
    FILE *f = std::fopen(in, "rb");
    if (!f) return 3;
    std::vector<uint32_t> out;
    Sample s;
    while (std::fread(&s, sizeof(s), 1, f) == 1) {
        const bool inside = ht_align_inside(s.fx, s.fy, s.SW, s.SH);
        uint32_t o = 0;
        if (inside) {
            const uint32_t tx = ((uint32_t)(int32_t)s.fx & 65535u) >> 8, ty = ((uint32_t)(int32_t)s.fy & 65535u) >> 8;
            for (int ch = 0; ch < 4; ch++) o |= ht_align_channel(s.p00, s.p01, s.p10, s.p11, 8 * ch, tx, ty);
        }
        out.push_back(inside ? 1u : 0u), out.push_back(o);
    }
    std::fclose(f);
    f = std::fopen(outname, "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(uint32_t), out.size(), f) == out.size();
    std::fclose(f);
    return ok ? 0 : 5;
}

int main(int argc, char **argv) {
    if (argc == 4 && std::strcmp(argv[1], "--pixels") == 0) return pixels(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<Case> cases;
    Case c;
    while (std::fread(&c, sizeof(c), 1, f) == 1) cases.push_back(c);
    std::fclose(f);
    std::vector<int64_t> out;
    out.reserve(cases.size() * 8);
    for (const Case &k : cases) {
        HtAlignPlan p;
        p.code = p.a12 = -1, p.cx = p.cy = p.ux = p.uy = p.vx = p.vy = -1;
        const int32_t code = ht_align_rule(k.x, k.y, k.width, k.height, k.angle, k.W, k.H, k.SW, k.SH, k.mx, k.my, k.mw, k.mh, k.margin_q8, k.flags, &p);
        if (code != p.code) return 6;
        out.push_back(code), out.push_back(p.a12);
        out.push_back(p.cx), out.push_back(p.cy), out.push_back(p.ux), out.push_back(p.uy), out.push_back(p.vx), out.push_back(p.vy);
        if (k.P <= 0) continue;
        for (int32_t i = 0; i < k.P; i++) out.push_back(ht_align_term(i, k.P, p.ux));
        for (int32_t i = 0; i < k.P; i++) out.push_back(ht_align_term(i, k.P, p.uy));
        for (int32_t j = 0; j < k.Q; j++) out.push_back(ht_align_term(j, k.Q, p.vx));
        for (int32_t j = 0; j < k.Q; j++) out.push_back(ht_align_term(j, k.Q, p.vy));
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = out.empty() || std::fwrite(out.data(), sizeof(int64_t), out.size(), f) == out.size();
    std::fclose(f);
    std::printf("cases %zu\n", cases.size());
    return ok ? 0 : 5;
}

// Host-only harness around headtrackr_amd/csrc/ht_yuv_plan.h and ht_draw_list_plan.h for the packed 4:2:2 formats (HT_YUV_YUYV = 4,
// HT_YUV_UYVY = 5), built by tests/test_ingest_422_cpu.py twice: plain, and with g++ -fsanitize=address,undefined (run directly, a program
// of its own).  Plane pointers are numbers here: the plans never dereference them.
//
//   yuv422_plan_harness plan <cases>    one case per line: width height format matrix y_pitch c_pitch frame_stride n; one JSON object per
//                                       line out: {"status": s} and, for status 0, the plan's fields
//   yuv422_plan_harness entry <cases>   one case per line: p0 p1 p2 pitch0 pitch1 width height format matrix rx ry rw rh W H; one JSON
//                                       object per line out: {"status": s} and, for status 0, the descriptor's and the extent's fields
//                                       (the ratios as their binary64 bit patterns)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "ht_draw_list_plan.h"

static int run_plan(const char *path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        long long w, h, fmt, mat, n;
        unsigned long long yp, cp, st;
        if (!(ls >> w >> h >> fmt >> mat >> yp >> cp >> st >> n)) return 2;
        HtYuvPlan p;
        std::memset(&p, 0xEE, sizeof(p));
        const int s = ht_yuv_plan((int32_t)w, (int32_t)h, (int32_t)fmt, (int32_t)mat, (size_t)yp, (size_t)cp, (size_t)st, (int32_t)n, &p);
        printf("{\"status\": %d", s);
        if (s == HT_YUV_PLAN_OK)
            printf(", \"cw\": %d, \"ch\": %d, \"c_row\": %zu, \"y_pitch\": %zu, \"c_pitch\": %zu, \"stride\": %zu, \"y_extent\": %zu, \"c_extent\": %zu, \"packed_frame\": %zu",
                   p.cw, p.ch, p.c_row, p.y_pitch, p.c_pitch, p.stride, p.y_extent, p.c_extent, p.packed_frame);
        printf("}\n");
    }
    return 0;
}

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

static int run_entry(const char *path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        unsigned long long p0, p1, p2, pitch0, pitch1;
        long long w, h, fmt, mat, rx, ry, rw, rh, W, H;
        if (!(ls >> p0 >> p1 >> p2 >> pitch0 >> pitch1 >> w >> h >> fmt >> mat >> rx >> ry >> rw >> rh >> W >> H)) return 2;
        ht_draw_source s;
        std::memset(&s, 0, sizeof(s));
        s.p0 = (const void *)(uintptr_t)p0, s.p1 = (const void *)(uintptr_t)p1, s.p2 = (const void *)(uintptr_t)p2;
        s.pitch0 = (size_t)pitch0, s.pitch1 = (size_t)pitch1, s.width = (int32_t)w, s.height = (int32_t)h, s.format = (int32_t)fmt, s.matrix = (int32_t)mat;
        s.rect.x = (int32_t)rx, s.rect.y = (int32_t)ry, s.rect.width = (int32_t)rw, s.rect.height = (int32_t)rh;
        HtDrawDesc d;
        HtDrawExtent e;
        std::memset(&d, 0xEE, sizeof(d));
        std::memset(&e, 0xEE, sizeof(e));
        const int st = ht_draw_list_plan_entry(s, (int32_t)W, (int32_t)H, &d, &e);
        printf("{\"status\": %d", st);
        if (st == HT_DRAW_LIST_OK) {
            printf(", \"p\": [%" PRIuPTR ", %" PRIuPTR ", %" PRIuPTR "], \"pitch\": [%zu, %zu], \"rect\": [%d, %d, %d, %d], \"cw\": %d, \"format\": %d", (uintptr_t)d.p0,
                   (uintptr_t)d.p1, (uintptr_t)d.p2, d.pitch0, d.pitch1, d.sx, d.sy, d.sw, d.sh, d.cw, d.format);
            printf(", \"ratio_bits\": [%" PRIu64 ", %" PRIu64 "], \"kc\": [%d, %d, %d, %d, %d, %d]", bits(d.rx), bits(d.ry), d.kc.yoff, d.kc.cy, d.kc.crv, d.kc.cgu, d.kc.cgv,
                   d.kc.cbu);
            printf(", \"base\": [%" PRIuPTR ", %" PRIuPTR ", %" PRIuPTR "], \"bytes\": [%zu, %zu, %zu]", (uintptr_t)e.base[0], (uintptr_t)e.base[1], (uintptr_t)e.base[2],
                   e.bytes[0], e.bytes[1], e.bytes[2]);
        }
        printf("}\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "plan")) return run_plan(argv[2]);
    if (argc >= 3 && !strcmp(argv[1], "entry")) return run_entry(argv[2]);
    return 2;
}

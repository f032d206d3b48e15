// Host-only harness around headtrackr_amd/csrc/ht_orient_plan.h (the orientation of an ingested source, bits 8..10 of a format), built by
// tests/test_orient_cpu.py twice: plain, and with g++ -fsanitize=address,undefined (run directly, a program of its own).  Plane pointers are
// numbers here: the plans never dereference them.
//
//   orient_plan_harness entry <cases>   one case per line: p0 p1 p2 pitch0 pitch1 width height format matrix rx ry rw rh W H; one JSON object
//                                       per line out: {"status": s} and, for status 0, the oriented descriptor's fields, the extents and
//                                       "plain": whether ht_orient_as_plain of it equals ht_draw_list_plan_entry's descriptor of the same
//                                       entry with the orientation bits cleared, byte for byte (null where that plan refuses the entry)
//   orient_plan_harness map <cases>     one case per line: k w h; out: {"size": [ow, oh], "uv": [[u, v] for y < oh for x < ow]}
//   orient_plan_harness whole <cases>   the entry line; out: ht_orient_whole of the planned descriptor and ht_orient_upright of the entry
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "ht_orient_plan.h"

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, sizeof(b));
    return b;
}

static bool read_entry(std::istringstream &ls, ht_draw_source *s, int32_t *W, int32_t *H) {
    unsigned long long p0, p1, p2, pitch0, pitch1;
    long long w, h, fmt, mat, rx, ry, rw, rh, cw, ch;
    if (!(ls >> p0 >> p1 >> p2 >> pitch0 >> pitch1 >> w >> h >> fmt >> mat >> rx >> ry >> rw >> rh >> cw >> ch)) return false;
    std::memset(s, 0, sizeof(*s));
    s->p0 = (const void *)(uintptr_t)p0, s->p1 = (const void *)(uintptr_t)p1, s->p2 = (const void *)(uintptr_t)p2;
    s->pitch0 = (size_t)pitch0, s->pitch1 = (size_t)pitch1, s->width = (int32_t)w, s->height = (int32_t)h, s->format = (int32_t)fmt, s->matrix = (int32_t)mat;
    s->rect.x = (int32_t)rx, s->rect.y = (int32_t)ry, s->rect.width = (int32_t)rw, s->rect.height = (int32_t)rh;
    *W = (int32_t)cw, *H = (int32_t)ch;
    return true;
}

static void print_desc(const HtOrientDesc &o) {
    const HtDrawDesc &d = o.d;
    printf("\"p\": [%" PRIuPTR ", %" PRIuPTR ", %" PRIuPTR "], \"pitch\": [%zu, %zu], \"stored\": [%d, %d, %d, %d], \"cw\": %d, \"format\": %d", (uintptr_t)d.p0, (uintptr_t)d.p1,
           (uintptr_t)d.p2, d.pitch0, d.pitch1, d.sx, d.sy, d.sw, d.sh, d.cw, d.format);
    printf(", \"ratio_bits\": [%" PRIu64 ", %" PRIu64 "], \"kc\": [%d, %d, %d, %d, %d, %d]", bits(d.rx), bits(d.ry), d.kc.yoff, d.kc.cy, d.kc.crv, d.kc.cgu, d.kc.cgv, d.kc.cbu);
    printf(", \"orient\": %d, \"frame\": %d, \"rect\": [%d, %d, %d, %d]", o.orient, o.frame, o.ox, o.oy, o.orw, o.orh);
}

static int run_entry(const char *path, bool whole) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        ht_draw_source s;
        int32_t W, H;
        if (!read_entry(ls, &s, &W, &H)) return 2;
        HtOrientDesc o;
        HtDrawExtent e;
        std::memset(&o, 0xEE, sizeof(o));
        std::memset(&e, 0xEE, sizeof(e));
        const int st = ht_orient_plan_entry(s, W, H, &o, &e);
        printf("{\"status\": %d", st);
        if (st == HT_DRAW_LIST_OK && !whole) {
            printf(", ");
            print_desc(o);
            printf(", \"base\": [%" PRIuPTR ", %" PRIuPTR ", %" PRIuPTR "], \"bytes\": [%zu, %zu, %zu]", (uintptr_t)e.base[0], (uintptr_t)e.base[1], (uintptr_t)e.base[2],
                   e.bytes[0], e.bytes[1], e.bytes[2]);
            int32_t ow, oh;
            ht_orient_size(o.orient, s.width, s.height, &ow, &oh);
            printf(", \"size\": [%d, %d], \"present\": %s", ow, oh, ht_orient_present(s.format) ? "true" : "false");
            // the same entry without its orientation, through the draw list's own plan
            ht_draw_source plain = s;
            plain.format = HT_FORMAT_OF(s.format);
            HtDrawDesc d, mine = ht_orient_as_plain(o);
            HtDrawExtent pe;
            std::memset(&d, 0, sizeof(d));  // (compared as bytes: the padding of both is written)
            const int ps = ht_draw_list_plan_entry(plain, W, H, &d, &pe);
            if (ps != HT_DRAW_LIST_OK) printf(", \"plain\": null");
            else printf(", \"plain\": %s", !std::memcmp(&d, &mine, sizeof(d)) && !std::memcmp(&pe, &e, sizeof(e)) ? "true" : "false");
        }
        if (st == HT_DRAW_LIST_OK && whole) {
            const HtOrientDesc j = ht_orient_whole(o);
            printf(", ");
            print_desc(j);
            const ht_draw_source u = ht_orient_upright(s, o.orient, (const void *)(uintptr_t)0x7000);
            printf(", \"upright\": {\"p\": [%" PRIuPTR ", %" PRIuPTR ", %" PRIuPTR "], \"pitch\": [%zu, %zu], \"size\": [%d, %d], \"format\": %d, \"matrix\": %d, \"rect\": [%d, %d, %d, %d]}",
                   (uintptr_t)u.p0, (uintptr_t)u.p1, (uintptr_t)u.p2, u.pitch0, u.pitch1, u.width, u.height, u.format, u.matrix, u.rect.x, u.rect.y, u.rect.width, u.rect.height);
        }
        printf("}\n");
    }
    return 0;
}

static int run_map(const char *path) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        long long k, w, h;
        if (!(ls >> k >> w >> h)) return 2;
        int32_t ow, oh;
        ht_orient_size((int32_t)k, (int32_t)w, (int32_t)h, &ow, &oh);
        printf("{\"size\": [%d, %d], \"uv\": [", ow, oh);
        for (int32_t y = 0; y < oh; y++)
            for (int32_t x = 0; x < ow; x++) {
                int32_t u = -1, v = -1;
                ht_orient_map((int32_t)k, (int32_t)w, (int32_t)h, x, y, &u, &v);
                printf("%s[%d, %d]", x || y ? ", " : "", u, v);
            }
        printf("]}\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && !strcmp(argv[1], "entry")) return run_entry(argv[2], false);
    if (argc >= 3 && !strcmp(argv[1], "whole")) return run_entry(argv[2], true);
    if (argc >= 3 && !strcmp(argv[1], "map")) return run_map(argv[2]);
    return 2;
}

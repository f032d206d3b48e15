// Host-only harness around headtrackr_amd/csrc/ht_draw_list_plan.h (the validated plan of ht_draw_list_device: the descriptors k_draw_list
// reads and the plane extents of the overlap refusals), built by tests/test_draw_list_cpu.py twice: plain, and with
// g++ -fsanitize=address,undefined (run directly, a program of its own).  Plane pointers are numbers here: the plan never dereferences them.
//
//   draw_list_plan_harness <cases>   the file holds calls, one line each item:
//       call W H n                     begins a call that claims n entries (the lines that follow may be fewer: a refused count)
//       entry count p0 p1 p2 pitch0 pitch1 width height format matrix rx ry rw rh      `count` copies of one ht_draw_source
//       null                           the call passes no list at all
//       dst address bytes              after the plan: the first entry that overlaps [address, address + bytes)
//       end
//   one JSON object per call: {"status", "message", "bad"} and, for status 0, "desc" (rx / ry as the 16 hex digits of their binary64 bits),
//   "ext" (of a list longer than 64 only the first and the last entry) and, when asked, "overlap".  The descriptor and extent arrays hold exactly the entries given, so a write past them is a
//   sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ht_draw_list_plan.h"

static const void *ptr_of(unsigned long long v) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(v)); }
static unsigned long long num_of(const void *p) { return static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(p)); }
static unsigned long long bits_of(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int W = 0, H = 0;
    long long n = 0;
    bool null_list = false, have_dst = false;
    unsigned long long dst = 0, dst_bytes = 0;
    std::vector<ht_draw_source> srcs;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string what;
        if (!(ls >> what)) continue;
        if (what == "call") {
            if (!(ls >> W >> H >> n)) return 2;
            srcs.clear(), null_list = have_dst = false;
        } else if (what == "entry") {
            long long count, w, h, fmt, mat, rx, ry, rw, rh;
            unsigned long long p0, p1, p2, pitch0, pitch1;
            if (!(ls >> count >> p0 >> p1 >> p2 >> pitch0 >> pitch1 >> w >> h >> fmt >> mat >> rx >> ry >> rw >> rh)) return 2;
            ht_draw_source s;
            std::memset(&s, 0, sizeof(s));
            s.p0 = ptr_of(p0), s.p1 = ptr_of(p1), s.p2 = ptr_of(p2), s.pitch0 = (size_t)pitch0, s.pitch1 = (size_t)pitch1;
            s.width = (int32_t)w, s.height = (int32_t)h, s.format = (int32_t)fmt, s.matrix = (int32_t)mat;
            s.rect = ht_cs_rect{(int32_t)rx, (int32_t)ry, (int32_t)rw, (int32_t)rh};
            srcs.insert(srcs.end(), (size_t)count, s);
        } else if (what == "null") {
            null_list = true;
        } else if (what == "dst") {
            if (!(ls >> dst >> dst_bytes)) return 2;
            have_dst = true;
        } else if (what == "end") {
            std::vector<HtDrawDesc> desc(srcs.size());
            std::vector<HtDrawExtent> ext(srcs.size());
            if (!srcs.empty()) std::memset(desc.data(), 0xEE, desc.size() * sizeof(HtDrawDesc)), std::memset(ext.data(), 0xEE, ext.size() * sizeof(HtDrawExtent));
            int32_t bad = -7;
            // a call may claim more entries than it gives only where the plan refuses the count before it reads one
            if (n > (long long)srcs.size() && n >= 1 && n <= HT_DRAW_LIST_MAX && !null_list) return 3;
            const int st = ht_draw_list_plan(null_list ? nullptr : srcs.data(), (int32_t)n, W, H, desc.data(), ext.data(), &bad);
            printf("{\"status\": %d, \"message\": \"%s\", \"bad\": %d", st, ht_draw_list_message(st), bad);
            if (st == HT_DRAW_LIST_OK) {
                std::vector<long long> shown;  // every entry of a list of <= 64, the first and the last of a longer one
                for (long long i = 0; i < n; i++)
                    if (n <= 64 || i == 0 || i == n - 1) shown.push_back(i);
                printf(", \"desc\": [");
                for (long long i : shown) {
                    const HtDrawDesc &d = desc[(size_t)i];
                    printf("%s{\"p\": [%llu, %llu, %llu], \"pitch\": [%zu, %zu], \"rx\": \"%016llx\", \"ry\": \"%016llx\", \"rect\": [%d, %d, %d, %d], \"cw\": %d, \"format\": %d, "
                           "\"kc\": [%d, %d, %d, %d, %d, %d]}",
                           i ? ", " : "", num_of(d.p0), num_of(d.p1), num_of(d.p2), d.pitch0, d.pitch1, bits_of(d.rx), bits_of(d.ry), d.sx, d.sy, d.sw, d.sh, d.cw, d.format,
                           d.kc.yoff, d.kc.cy, d.kc.crv, d.kc.cgu, d.kc.cgv, d.kc.cbu);
                }
                printf("], \"ext\": [");
                for (long long i : shown) {
                    const HtDrawExtent &e = ext[(size_t)i];
                    printf("%s[[%llu, %zu], [%llu, %zu], [%llu, %zu]]", i ? ", " : "", num_of(e.base[0]), e.bytes[0], num_of(e.base[1]), e.bytes[1], num_of(e.base[2]), e.bytes[2]);
                }
                printf("]");
                if (have_dst) printf(", \"overlap\": %d", ht_draw_list_overlap(ext.data(), (int32_t)n, ptr_of(dst), (size_t)dst_bytes));
            }
            printf("}\n");
        } else {
            return 2;
        }
    }
    return 0;
}

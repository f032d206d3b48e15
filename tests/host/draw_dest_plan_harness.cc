// Host-only harness around headtrackr_amd/csrc/ht_draw_dest_plan.h (where a canvas-draw call writes: the bind or caller's-buffer form, the
// effective stride, the range the call will write, and each call kind's order of refusals), built by tests/test_draw_dest_plan_cpu.py twice:
// plain, and with g++ -fsanitize=address,undefined (run directly, a program of its own).  Pointers are numbers here: the plan never
// dereferences them.
//
//   draw_dest_plan_harness <cases>   one call per line:
//       kind W H n dst stride max_batch own_base own_bytes source_fault src src_bytes
//   (src, src_bytes: a one-plane source extent asked about the planned range, 0 0 for none)
//   one JSON object per line: {"status", "message", "behind_device"} and, for status 0, "bind", "fbytes", "stride", "base", "bytes",
//   "overlap" (ht_draw_list_overlap's answer for the source) and "overlap_message".
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>

#include "ht_draw_dest_plan.h"

static const void *ptr_of(unsigned long long v) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(v)); }
static unsigned long long num_of(const void *p) { return static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(p)); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        long long kind, W, H, n, max_batch, fault;
        unsigned long long dst, stride, own, own_bytes, src, src_bytes;
        if (!(ls >> kind >> W >> H >> n >> dst >> stride >> max_batch >> own >> own_bytes >> fault >> src >> src_bytes)) return 2;
        HtDrawDest d = {};
        const int st = ht_draw_dest_plan((int)kind, (int32_t)W, (int32_t)H, (int32_t)n, ptr_of(dst), (size_t)stride, (int32_t)max_batch, ptr_of(own), (size_t)own_bytes,
                                         fault != 0, &d);
        std::printf("{\"status\": %d, \"message\": \"%s\", \"behind_device\": %d", st, ht_draw_dest_message((int)kind, st), (int)ht_draw_dest_behind_device((int)kind, st));
        if (st == HT_DRAW_DEST_OK) {
            const HtDrawExtent x = {{ptr_of(src)}, {(size_t)src_bytes}};
            std::printf(", \"bind\": %d, \"fbytes\": %zu, \"stride\": %zu, \"base\": %llu, \"bytes\": %zu, \"overlap\": %d, \"overlap_message\": \"%s\"", (int)d.bind, d.fbytes,
                        d.stride, num_of(d.base), d.bytes, (int)ht_draw_list_overlap(&x, 1, d.base, d.bytes), ht_draw_dest_overlap_message((int)kind, d.bind));
        }
        std::printf("}\n");
    }
    return 0;
}

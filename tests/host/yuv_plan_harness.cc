// Host-only harness around headtrackr_amd/csrc/ht_yuv_plan.h (the declared YUV -> RGBA conversion and the call plan of the YUV ingest),
// built by tests/test_ingest_yuv_cpu.py twice: plain, and with g++ -fsanitize=address,undefined (run directly, a program of its own).
//
//   yuv_plan_harness crc            one line per matrix: the CRC-32 (zlib's polynomial) of yuv_to_rgba over all 2^24 triples, Y slowest,
//                                   V fastest, every pixel as 4 bytes R G B A; then the line for an out-of-range matrix (must be 0)
//   yuv_plan_harness plan <cases>   one case per line: width height format matrix y_pitch c_pitch frame_stride n; one JSON object per line
//                                   out: {"status": s, "message": ".."} and, for status 0, the plan's fields
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "ht_yuv_plan.h"

static uint32_t g_crc_table[256];
static void crc_init() {
    for (uint32_t n = 0; n < 256; n++) {
        uint32_t c = n;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
        g_crc_table[n] = c;
    }
}
static uint32_t crc_update(uint32_t c, const uint8_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) c = g_crc_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c;
}

static int run_crc() {
    crc_init();
    std::vector<uint8_t> row(256 * 4);  // exactly one V sweep: a write past it is a sanitizer report
    for (int m = 0; m < HT_YUV_NMATRICES; m++) {
        uint32_t c = 0xffffffffu;
        for (int y = 0; y < 256; y++)
            for (int u = 0; u < 256; u++) {
                for (int v = 0; v < 256; v++) {
                    const uint32_t px = yuv_to_rgba(y, u, v, m);
                    if (px != ht_yuv_to_rgba(y, u, v, HT_YUV_COEF[m])) return 3;  // the two forms of the scalar agree
                    row[4 * v] = (uint8_t)px, row[4 * v + 1] = (uint8_t)(px >> 8), row[4 * v + 2] = (uint8_t)(px >> 16), row[4 * v + 3] = (uint8_t)(px >> 24);
                }
                c = crc_update(c, row.data(), row.size());
            }
        printf("%d %u\n", m, c ^ 0xffffffffu);
    }
    printf("out-of-range %u %u\n", yuv_to_rgba(128, 128, 128, -1), yuv_to_rgba(128, 128, 128, HT_YUV_NMATRICES));
    return 0;
}

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
        printf("{\"status\": %d, \"message\": \"%s\"", s, ht_yuv_plan_message(s));
        if (s == HT_YUV_PLAN_OK)
            printf(", \"cw\": %d, \"ch\": %d, \"c_row\": %zu, \"y_pitch\": %zu, \"c_pitch\": %zu, \"stride\": %zu, \"y_extent\": %zu, \"c_extent\": %zu, \"packed_frame\": %zu",
                   p.cw, p.ch, p.c_row, p.y_pitch, p.c_pitch, p.stride, p.y_extent, p.c_extent, p.packed_frame);
        printf("}\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "crc")) return run_crc();
    if (argc >= 3 && !strcmp(argv[1], "plan")) return run_plan(argv[2]);
    return 2;
}

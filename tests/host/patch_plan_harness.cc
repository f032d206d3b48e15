// patch_plan_harness.cc — headtrackr_amd/csrc/ht_patch_plan.h (and ht_gray.h) as a program of its own: the lines k_cut_tensor and
// k_upright_tensor compile for the device, compiled by g++ -ffp-contract=off, plain and with -fsanitize=address,undefined
// (tests/test_patch_tensor_cpu.py builds and runs both and compares every answer with the Python restatement).
//
//   patch_plan_harness --values  in out   in: (float scale, float bias) pairs; out: per pair, per byte 0 .. 255, the f32 / f16 / bf16 bits (uint32 x 3)
//   patch_plan_harness --gray    out      the gray byte of all 2^24 (R, G, B), index R | G << 8 | B << 16
//   patch_plan_harness --formats in out   in: ht_patch_format structs; out: ht_patch_check_format's code (int32) for each
//   patch_plan_harness --sizes   in out   in: (w, h, dtype, layout, channels) int32 x 5; out: bytes, default stride, then the byte offsets of
//                                         elements (c, 0, 0) and (c, w - 1, h - 1) for c = 0 .. C - 1 (absent channels: 0), uint64 x 8
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ht_patch_plan.h"

static std::vector<unsigned char> slurp(const char *path) {
    std::vector<unsigned char> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}

static void spill(const char *path, const void *p, size_t n) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) {
        std::fprintf(stderr, "cannot write %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

int main(int argc, char **argv) {
    static_assert(sizeof(ht_patch_format) == 40, "ht_patch_format");
    if (argc == 3 && !std::strcmp(argv[1], "--gray")) {
        std::vector<unsigned char> out((size_t)1 << 24);
        for (uint32_t px = 0; px < (1u << 24); px++) out[px] = (unsigned char)ht_patch_byte(px | 0xff000000u, HT_PATCH_GRAY, 0);
        spill(argv[2], out.data(), out.size());
        return 0;
    }
    if (argc != 4) {
        std::fprintf(stderr, "usage: patch_plan_harness --values|--formats|--sizes in out | --gray out\n");
        return 2;
    }
    const std::vector<unsigned char> in = slurp(argv[2]);
    if (!std::strcmp(argv[1], "--values")) {
        const size_t n = in.size() / 8;
        std::vector<uint32_t> out(n * 256 * 3);
        for (size_t i = 0; i < n; i++) {
            float sb[2];
            std::memcpy(sb, in.data() + 8 * i, 8);
            for (uint32_t b = 0; b < 256; b++) {
                // through the byte selector too: b sits in the B byte and is read as channel 0 of BGR and as channel 2 of RGB
                const uint32_t px = b << 16, b0 = ht_patch_byte(px, HT_PATCH_BGR, 0), b2 = ht_patch_byte(px, HT_PATCH_RGB, 2);
                if (b0 != b || b2 != b || ht_patch_byte(px, HT_PATCH_RGB, 0) != 0) return 3;
                const float v = ht_patch_value(b0, sb[0], sb[1]);
                for (int dt = 0; dt < 3; dt++) out[(i * 256 + b) * 3 + dt] = ht_patch_element(v, dt);
            }
        }
        spill(argv[3], out.data(), out.size() * 4);
    } else if (!std::strcmp(argv[1], "--formats")) {
        const size_t n = in.size() / sizeof(ht_patch_format);
        std::vector<int32_t> out(n);
        for (size_t i = 0; i < n; i++) {
            ht_patch_format f;
            std::memcpy(&f, in.data() + i * sizeof f, sizeof f);
            out[i] = ht_patch_check_format(&f);
            if (!*ht_patch_format_message(out[i])) return 3;
        }
        spill(argv[3], out.data(), out.size() * 4);
    } else if (!std::strcmp(argv[1], "--sizes")) {
        const size_t n = in.size() / 20;
        std::vector<uint64_t> out(n * 8, 0);
        for (size_t i = 0; i < n; i++) {
            int32_t q[5];
            std::memcpy(q, in.data() + 20 * i, 20);
            uint64_t *o = &out[8 * i];
            o[0] = ht_patch_bytes(q[0], q[1], q[2], q[4]);
            o[1] = ht_patch_default_stride((size_t)o[0]);
            for (int c = 0; c < ht_patch_nchannels(q[4]); c++) {
                o[2 + c] = ht_patch_offset(q[0], q[1], q[2], q[3], q[4], c, 0, 0);
                o[5 + c] = ht_patch_offset(q[0], q[1], q[2], q[3], q[4], c, q[0] - 1, q[1] - 1);
            }
        }
        spill(argv[3], out.data(), out.size() * 8);
    } else {
        return 2;
    }
    return 0;
}

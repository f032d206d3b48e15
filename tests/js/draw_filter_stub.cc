// draw_filter_stub.cc — the two C-ABI functions of the prefiltered draw list, recording: ht_draw_list_filtered_device and
// ht_draw_filter_factors, linked together with tests/js/abi_stub.cc, tests/js/draw_list_stub.cc (both left as they are) and
// csrc/ht_napi.cc into a temporary .node by tests/test_draw_filter_cpu.py, so that the shim's drawListFilteredDevice and drawFilterFactors
// run on the CPU.  Never linked into the product addon.  Every call of the first appends one JSON line to the file named by
// HT_DF_STUB_LOG: n, max_factor, the destination (relative to entry 0's p0; null for the bind form), its stride, and per entry what
// draw_list_stub.cc logs.  n == 3 fails with HT_ERR_INVALID, to pin the shim's error path.  The factor function answers
// (src_width + canvas_width, src_height + 10 * max_factor + canvas_height) — every argument arrived — and refuses a source width of 16385.
#include <cstdio>
#include <cstdlib>

#include "headtrackr_hip.h"

static void rel(FILE *f, const void *p, const void *base) {
    if (!p) fprintf(f, "null");
    else fprintf(f, "%lld", (long long)((const char *)p - (const char *)base));
}

extern "C" ht_status ht_draw_list_filtered_device(ht_ctx *ctx, const ht_draw_source *srcs, int32_t n, int32_t max_factor, void *dst_dev, size_t dst_frame_stride) {
    const char *fn = getenv("HT_DF_STUB_LOG");
    FILE *f = fn ? fopen(fn, "a") : nullptr;
    if (f) {
        fprintf(f, "{\"ctx\": %s, \"n\": %d, \"max_factor\": %d, \"dst\": ", ctx ? "true" : "false", n, max_factor);
        rel(f, dst_dev, srcs[0].p0);
        fprintf(f, ", \"dst_stride\": %zu, \"entries\": [", dst_frame_stride);
        for (int32_t i = 0; i < n; i++) {
            const ht_draw_source &s = srcs[i];
            fprintf(f, "%s{\"p0\": ", i ? ", " : "");
            rel(f, s.p0, srcs[0].p0);
            fprintf(f, ", \"p1\": ");
            rel(f, s.p1, s.p0);
            fprintf(f, ", \"p2\": ");
            rel(f, s.p2, s.p0);
            fprintf(f, ", \"pitch\": [%zu, %zu], \"size\": [%d, %d], \"format\": %d, \"matrix\": %d, \"rect\": [%d, %d, %d, %d]}", s.pitch0, s.pitch1, s.width, s.height, s.format,
                    s.matrix, s.rect.x, s.rect.y, s.rect.width, s.rect.height);
        }
        fprintf(f, "]}\n");
        fclose(f);
    }
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}

extern "C" ht_status ht_draw_filter_factors(int32_t src_width, int32_t src_height, int32_t canvas_width, int32_t canvas_height, int32_t max_factor, int32_t *nx,
                                            int32_t *ny) {
    if (src_width == 16385) return HT_ERR_INVALID;
    *nx = src_width + canvas_width, *ny = src_height + 10 * max_factor + canvas_height;
    return HT_OK;
}

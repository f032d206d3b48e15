// draw_list_stub.cc — the one C-ABI function tests/js/abi_stub.cc (left as it is) does not have: a recording ht_draw_list_device, linked
// together with that stub and csrc/ht_napi.cc into a temporary .node by tests/test_draw_list_cpu.py, so that the shim's drawListDevice —
// the entry reader, the per-entry plane layout, the range checks, the destination offset and stride — runs on the CPU.  Never linked
// into the product addon.  Every call appends one JSON line to the file named by HT_DL_STUB_LOG: n, the destination (relative to entry
// 0's p0; null for the bind form), its stride, and per entry p0 relative to entry 0's p0, p1 and p2 relative to the entry's own p0 (null
// for a NULL pointer) and the scalars.  n == 3 fails with HT_ERR_INVALID, to pin the shim's error path.
#include <cstdio>
#include <cstdlib>

#include "headtrackr_hip.h"

static void rel(FILE *f, const void *p, const void *base) {
    if (!p) fprintf(f, "null");
    else fprintf(f, "%lld", (long long)((const char *)p - (const char *)base));
}

extern "C" ht_status ht_draw_list_device(ht_ctx *ctx, const ht_draw_source *srcs, int32_t n, void *dst_dev, size_t dst_frame_stride) {
    const char *fn = getenv("HT_DL_STUB_LOG");
    FILE *f = fn ? fopen(fn, "a") : nullptr;
    if (f) {
        fprintf(f, "{\"ctx\": %s, \"n\": %d, \"dst\": ", ctx ? "true" : "false", n);
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

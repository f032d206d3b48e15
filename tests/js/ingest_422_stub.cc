// ingest_422_stub.cc — the two C-ABI functions tests/js/abi_stub.cc (left as it is) does not have: recording ht_draw_frames_yuv and
// ht_draw_frames_yuv_device, linked together with that stub, tests/js/draw_list_stub.cc and csrc/ht_napi.cc into a temporary .node by
// tests/test_ingest_422_addon_cpu.py, so that the shim's drawFramesYuv / drawFramesYuvDevice — the format-aware frame size, the plane
// pointers of a packed 4:2:2 frame, the length checks — run on the CPU.  Never linked into the product addon.  Every call appends one JSON
// line to the file named by HT_422_STUB_LOG.  The host form sums the bytes of the n frames it was promised (4 cw h each for YUYV / UYVY), so
// that a shim that let a short buffer through reads past it; the device form logs u and v relative to y (null for a NULL pointer).
#include <cstdio>
#include <cstdlib>

#include "headtrackr_hip.h"

static FILE *open_log() {
    const char *fn = getenv("HT_422_STUB_LOG");
    return fn ? fopen(fn, "a") : nullptr;
}

static void rel(FILE *f, const void *p, const void *base) {
    if (!p) fprintf(f, "null");
    else fprintf(f, "%lld", (long long)((const char *)p - (const char *)base));
}

static void rect(FILE *f, const ht_cs_rect *r) {
    if (!r) fprintf(f, "null");
    else fprintf(f, "[%d, %d, %d, %d]", r->x, r->y, r->width, r->height);
}

extern "C" ht_status ht_draw_frames_yuv(ht_ctx *ctx, const uint8_t *host, int32_t n, int32_t width, int32_t height, int32_t format, int32_t matrix, size_t frame_stride,
                                        const ht_cs_rect *src_rect) {
    const bool packed = format == HT_YUV_YUYV || format == HT_YUV_UYVY;
    const size_t cw = (size_t)(width + 1) / 2, ch = (size_t)(height + 1) / 2;
    const size_t fsz = packed ? 4 * cw * (size_t)height : (size_t)width * height + 2 * cw * ch;
    unsigned long long sum = 0;
    for (size_t i = 0; i < fsz * (size_t)n; i++) sum += host[i];
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"ht_draw_frames_yuv\", \"ctx\": %s, \"n\": %d, \"size\": [%d, %d], \"format\": %d, \"matrix\": %d, \"stride\": %zu, \"bytes\": %zu, \"sum\": %llu, \"rect\": ",
                ctx ? "true" : "false", n, width, height, format, matrix, frame_stride, fsz * (size_t)n, sum);
        rect(f, src_rect);
        fprintf(f, "}\n");
        fclose(f);
    }
    return HT_OK;
}

extern "C" ht_status ht_draw_frames_yuv_device(ht_ctx *ctx, const ht_yuv_frames *s, int32_t n, const ht_cs_rect *src_rect, void *dst_dev, size_t dst_frame_stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"ht_draw_frames_yuv_device\", \"ctx\": %s, \"n\": %d, \"u\": ", ctx ? "true" : "false", n);
        rel(f, s->u, s->y);
        fprintf(f, ", \"v\": ");
        rel(f, s->v, s->y);
        fprintf(f, ", \"y_set\": %s, \"pitch\": [%zu, %zu], \"stride\": %zu, \"size\": [%d, %d], \"format\": %d, \"matrix\": %d, \"dst\": %s, \"dst_stride\": %zu, \"rect\": ",
                s->y ? "true" : "false", s->y_pitch, s->c_pitch, s->frame_stride, s->width, s->height, s->format, s->matrix, dst_dev ? "true" : "false", dst_frame_stride);
        rect(f, src_rect);
        fprintf(f, "}\n");
        fclose(f);
    }
    return HT_OK;
}

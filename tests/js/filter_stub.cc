// filter_stub.cc — the C-ABI functions of the prefiltered face crops that tests/js/abi_stub.cc, crop_stub.cc, align_stub.cc and patch_stub.cc
// (all left as they are) do not have: recording ht_camshift_{crop,align}_{pairs,sources}_filtered_device and the two factor functions,
// linked together with those stubs and csrc/ht_napi.cc into a temporary .node by tests/test_filter_cpu.py, so that the shim's
// cropPairsFilteredDevice, cropSourcesFilteredDevice, alignPairsFilteredDevice, alignSourcesFilteredDevice, cropFilterFactors and
// alignFilterFactors — the argument readers, maxFactor, the NULL or non-NULL format, the range check on the patch's or the tensor's bytes —
// run on the CPU.  Never linked into the product addon.  Every call appends one JSON line to the file named by HT_FILTER_STUB_LOG; the
// output pointer is logged relative to the first entry's p0 (sources form).  n == 3 fails with HT_ERR_INVALID.  The factor functions answer
// (width of the rect or ux >> 16) + out_width, (height or vy >> 16) + max_factor: a way to see every argument arrive.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "headtrackr_hip.h"

static FILE *open_log() {
    const char *fn = getenv("HT_FILTER_STUB_LOG");
    return fn ? fopen(fn, "a") : nullptr;
}
static void tail(FILE *f, int32_t w, int32_t h, int32_t m, uint32_t fl, int32_t max_factor, const ht_patch_format *t, size_t stride) {
    fprintf(f, ", \"params\": [%d, %d, %d, %u], \"max_factor\": %d, ", w, h, m, fl, max_factor);
    if (t) {
        uint32_t u[6];
        memcpy(u, t->scale, 12), memcpy(u + 3, t->bias, 12);
        fprintf(f, "\"format\": [%d, %d, %d, %d], \"coef\": [%u, %u, %u, %u, %u, %u]", t->dtype, t->layout, t->channels, t->pad, u[0], u[1], u[2], u[3], u[4], u[5]);
    } else {
        fprintf(f, "\"format\": null");
    }
    fprintf(f, ", \"stride\": %zu}\n", stride);
    fclose(f);
}
static void pairs_line(const char *fn, ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t w, int32_t h, int32_t m, uint32_t fl, int32_t max_factor,
                       const ht_patch_format *t, void *out, size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"%s\", \"ctx\": %s, \"n\": %d, \"out\": %d, \"pairs\": [", fn, ctx ? "true" : "false", n, out ? 1 : 0);
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s[%d, %d]", i ? ", " : "", pairs[i].stream, pairs[i].frame);
        fprintf(f, "]");
        tail(f, w, h, m, fl, max_factor, t, stride);
    }
}
static void sources_line(const char *fn, ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, int32_t w, int32_t h, int32_t m, uint32_t fl,
                         int32_t max_factor, const ht_patch_format *t, void *out, size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"%s\", \"ctx\": %s, \"n\": %d, \"out\": %lld, \"streams\": [", fn, ctx ? "true" : "false", n, (long long)((const char *)out - (const char *)srcs[0].p0));
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s%d", i ? ", " : "", streams[i]);
        fprintf(f, "], \"sizes\": [");
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s[%d, %d, %d]", i ? ", " : "", srcs[i].width, srcs[i].height, srcs[i].format);
        fprintf(f, "]");
        tail(f, w, h, m, fl, max_factor, t, stride);
    }
}

extern "C" ht_status ht_camshift_crop_pairs_filtered_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *p, int32_t max_factor,
                                                            const ht_patch_format *t, void *out, size_t stride) {
    pairs_line("crop_pairs", ctx, pairs, n, p->out_width, p->out_height, p->margin_q8, p->flags, max_factor, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_crop_sources_filtered_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *p,
                                                              int32_t max_factor, const ht_patch_format *t, void *out, size_t stride) {
    sources_line("crop_sources", ctx, streams, srcs, n, p->out_width, p->out_height, p->margin_q8, p->flags, max_factor, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_align_pairs_filtered_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *p, int32_t max_factor,
                                                             const ht_patch_format *t, void *out, size_t stride) {
    pairs_line("align_pairs", ctx, pairs, n, p->out_width, p->out_height, p->margin_q8, p->flags, max_factor, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_align_sources_filtered_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *p,
                                                               int32_t max_factor, const ht_patch_format *t, void *out, size_t stride) {
    sources_line("align_sources", ctx, streams, srcs, n, p->out_width, p->out_height, p->margin_q8, p->flags, max_factor, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_crop_filter_factors(const ht_crop_record *r, int32_t w, int32_t h, int32_t max_factor, int32_t *nx, int32_t *ny) {
    if (!r || !nx || !ny) return HT_ERR_INVALID;
    *nx = r->code ? r->rect.width + w : 0, *ny = r->code ? r->rect.height + max_factor : 0;
    (void)h;
    return HT_OK;
}
extern "C" ht_status ht_camshift_align_filter_factors(const ht_align_record *r, int32_t w, int32_t h, int32_t max_factor, int32_t *nx, int32_t *ny) {
    if (!r || !nx || !ny) return HT_ERR_INVALID;
    *nx = r->code ? (int32_t)(r->ux >> 16) + w : 0, *ny = r->code ? (int32_t)(r->vy >> 16) + max_factor : 0;
    (void)h;
    return HT_OK;
}

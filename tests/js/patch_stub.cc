// patch_stub.cc — the C-ABI functions of the model-input tensors that tests/js/abi_stub.cc, crop_stub.cc and align_stub.cc (all left as they
// are) do not have: recording ht_camshift_{crop,align}_{pairs,sources}_tensor_device, linked together with those stubs and csrc/ht_napi.cc
// into a temporary .node by tests/test_patch_tensor_cpu.py, so that the shim's cropPairsTensorDevice, cropSourcesTensorDevice,
// alignPairsTensorDevice and alignSourcesTensorDevice — the argument readers, the format object, the range check on the TENSOR's bytes, the
// output offset and stride — run on the CPU.  Never linked into the product addon.  Every call appends one JSON line to the file named by
// HT_PATCH_STUB_LOG; the output pointer is logged relative to the first entry's p0 (sources form).  n == 3 fails with HT_ERR_INVALID.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "headtrackr_hip.h"

static FILE *open_log() {
    const char *fn = getenv("HT_PATCH_STUB_LOG");
    return fn ? fopen(fn, "a") : nullptr;
}
static void tail(FILE *f, int32_t w, int32_t h, int32_t m, uint32_t fl, const ht_patch_format *t, size_t stride) {
    uint32_t u[6];
    memcpy(u, t->scale, 12), memcpy(u + 3, t->bias, 12);
    fprintf(f, ", \"params\": [%d, %d, %d, %u], \"format\": [%d, %d, %d, %d], \"coef\": [%u, %u, %u, %u, %u, %u], \"stride\": %zu}\n", w, h, m, fl, t->dtype, t->layout,
            t->channels, t->pad, u[0], u[1], u[2], u[3], u[4], u[5], stride);
    fclose(f);
}
static void pairs_line(const char *fn, ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t w, int32_t h, int32_t m, uint32_t fl, const ht_patch_format *t, void *out,
                       size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"%s\", \"ctx\": %s, \"n\": %d, \"out\": %d, \"pairs\": [", fn, ctx ? "true" : "false", n, out ? 1 : 0);
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s[%d, %d]", i ? ", " : "", pairs[i].stream, pairs[i].frame);
        fprintf(f, "]");
        tail(f, w, h, m, fl, t, stride);
    }
}
static void sources_line(const char *fn, ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, int32_t w, int32_t h, int32_t m, uint32_t fl,
                         const ht_patch_format *t, void *out, size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"%s\", \"ctx\": %s, \"n\": %d, \"out\": %lld, \"streams\": [", fn, ctx ? "true" : "false", n, (long long)((const char *)out - (const char *)srcs[0].p0));
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s%d", i ? ", " : "", streams[i]);
        fprintf(f, "], \"sizes\": [");
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s[%d, %d, %d]", i ? ", " : "", srcs[i].width, srcs[i].height, srcs[i].format);
        fprintf(f, "]");
        tail(f, w, h, m, fl, t, stride);
    }
}

extern "C" ht_status ht_camshift_crop_pairs_tensor_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *p, const ht_patch_format *t, void *out,
                                                          size_t stride) {
    pairs_line("crop_pairs", ctx, pairs, n, p->out_width, p->out_height, p->margin_q8, p->flags, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_crop_sources_tensor_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *p,
                                                            const ht_patch_format *t, void *out, size_t stride) {
    sources_line("crop_sources", ctx, streams, srcs, n, p->out_width, p->out_height, p->margin_q8, p->flags, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_align_pairs_tensor_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *p, const ht_patch_format *t, void *out,
                                                           size_t stride) {
    pairs_line("align_pairs", ctx, pairs, n, p->out_width, p->out_height, p->margin_q8, p->flags, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}
extern "C" ht_status ht_camshift_align_sources_tensor_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *p,
                                                             const ht_patch_format *t, void *out, size_t stride) {
    sources_line("align_sources", ctx, streams, srcs, n, p->out_width, p->out_height, p->margin_q8, p->flags, t, out, stride);
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}

// align_stub.cc — the C-ABI functions of the aligned crops that tests/js/abi_stub.cc and tests/js/crop_stub.cc (both left as they are) do not
// have: recording ht_camshift_align_pairs_device / ht_camshift_align_sources_device and an ht_camshift_align_result with fixed records,
// linked together with those stubs and csrc/ht_napi.cc into a temporary .node by tests/test_align_cpu.py, so that the shim's
// alignPairsDevice, alignSourcesDevice and alignResult — the argument readers, the range checks, the output offset and stride — run on the
// CPU.  Never linked into the product addon.  Every align call appends one JSON line to the file named by HT_ALIGN_STUB_LOG; pointers are
// logged relative to `out` (sources form: p0 of an entry relative to out, p1 / p2 relative to the entry's p0).  n == 3 fails with
// HT_ERR_INVALID, to pin the error path.
#include <cstdio>
#include <cstdlib>

#include "headtrackr_hip.h"

static FILE *open_log() {
    const char *fn = getenv("HT_ALIGN_STUB_LOG");
    return fn ? fopen(fn, "a") : nullptr;
}
static void rel(FILE *f, const void *p, const void *base) {
    if (!p) fprintf(f, "null");
    else fprintf(f, "%lld", (long long)((const char *)p - (const char *)base));
}
static void tail(FILE *f, const ht_align_params *p, size_t stride) {
    fprintf(f, ", \"params\": [%d, %d, %d, %u], \"stride\": %zu}\n", p->out_width, p->out_height, p->margin_q8, p->flags, stride);
    fclose(f);
}

extern "C" ht_status ht_camshift_align_pairs_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *p, void *out, size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"pairs\", \"ctx\": %s, \"n\": %d, \"out\": %d, \"pairs\": [", ctx ? "true" : "false", n, out ? 1 : 0);
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s[%d, %d]", i ? ", " : "", pairs[i].stream, pairs[i].frame);
        fprintf(f, "]");
        tail(f, p, stride);
    }
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}

extern "C" ht_status ht_camshift_align_sources_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *p, void *out,
                                                     size_t stride) {
    if (FILE *f = open_log()) {
        fprintf(f, "{\"fn\": \"sources\", \"ctx\": %s, \"n\": %d, \"streams\": [", ctx ? "true" : "false", n);
        for (int32_t i = 0; i < n; i++) fprintf(f, "%s%d", i ? ", " : "", streams[i]);
        fprintf(f, "], \"entries\": [");
        for (int32_t i = 0; i < n; i++) {
            const ht_draw_source &s = srcs[i];
            fprintf(f, "%s{\"p0\": ", i ? ", " : "");
            rel(f, s.p0, out);
            fprintf(f, ", \"p1\": ");
            rel(f, s.p1, s.p0);
            fprintf(f, ", \"p2\": ");
            rel(f, s.p2, s.p0);
            fprintf(f, ", \"size\": [%d, %d], \"format\": %d, \"matrix\": %d, \"rect\": [%d, %d, %d, %d]}", s.width, s.height, s.format, s.matrix, s.rect.x, s.rect.y,
                    s.rect.width, s.rect.height);
        }
        fprintf(f, "]");
        tail(f, p, stride);
    }
    return n == 3 ? HT_ERR_INVALID : HT_OK;
}

// record i: code i & 1, stream 10 + i, a12 100 i, pad 0, cx .. vy = +-(2^40 + 7 i + k) (negative for odd k); n == 5 is refused
extern "C" ht_status ht_camshift_align_result(ht_ctx *, int32_t n, ht_align_record *out) {
    if (n == 5) return HT_ERR_STATE;
    for (int32_t i = 0; i < n; i++) {
        out[i].code = i & 1, out[i].stream = 10 + i, out[i].a12 = 100 * i, out[i].pad = 0;
        int64_t *q[6] = {&out[i].cx, &out[i].cy, &out[i].ux, &out[i].uy, &out[i].vx, &out[i].vy};
        for (int k = 0; k < 6; k++) *q[k] = ((int64_t)1 << 40) + 7 * i + k, *q[k] = (k & 1) ? -*q[k] : *q[k];
    }
    return HT_OK;
}

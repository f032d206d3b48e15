// abi_stub.cc — a recording stand-in for the 47 C-ABI functions the N-API shim (headtrackr_amd/csrc/ht_napi.cc) references, so that the
// shim's own behaviour — argument validation, range checks, optional arguments, result shapes, error messages — can be pinned without a
// GPU (tests/js/addon_calls.js, tests/test_addon_calls_cpu.py).  No HIP, no GPU code, no algorithm: it is linked in place of
// libheadtrackr_hip.so into a temporary .node and never into the product addon.
//
//  * Every function appends one line to the file named by the environment variable HT_STUB_LOG: its name and scalar arguments.
//  * Contexts are logged as ctx#<index>; device pointers as dev#<allocation index>+<byte offset> (ht_device_alloc hands out plain host
//    memory, which the stub never reads or writes through a "device" pointer, so a range the shim let through by mistake is logged, not
//    dereferenced); host input buffers by length and FNV-1a hash; small input tables (rects, pairs, level dims, the per-call pointers
//    of a sequence) by content.
//  * Every HOST output buffer is filled over its whole stated size: byte i = 7 i + 3 (mod 256), double i = i / 2 + 1, hit and track
//    object fields counted up from their index.  An undersized buffer shows up as a size in the log (and under a memory checker).
//  * State the shim reads back: ht_plane reports the last ht_set_geometry size (HT_ERR_STATE before one); ht_frames_bound and
//    ht_frames_enqueued the n bound last; the first ht_detect_batch of a context reports HT_ERR_CAPACITY with 5000 hits (above the
//    shim's first buffer of 4096), later ones succeed with `cap` hits when cap > 4096, else 3.
//  * Forced failures, to pin every error message of the shim.  The magic value is 7777:
//      ht_camshift_reserve(ctx, 7777)      fails itself
//      ht_camshift_reserve(ctx, 7777 + k)  1 <= k <= 9: succeeds, and the k-th following status-returning call that takes this context
//                                          (ht_plane not counted) fails with HT_ERR_INVALID; ht_last_error names the function
//      ht_create with device 7777, ht_host_alloc(7777)   fail
//      ht_detect_enqueue(ctx, 7777)        succeeds; the following ht_detect_collect reports HT_ERR_CAPACITY with 70000 hits
//    ht_device_free on another context than the allocating one fails with HT_ERR_STATE, as the library's does.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "headtrackr_hip.h"

struct ht_ctx {
    int index = 0;
    int w = 0, h = 0, bound = 0, arm = 0;
    bool detected = false, big_collect = false;
    std::string err;
};

namespace {

constexpr int MAGIC = 7777;

struct Alloc {
    char *p;
    size_t bytes;
    const ht_ctx *owner;
    bool live;
};
std::mutex g_mu;
std::vector<ht_ctx *> g_ctxs;  // never freed: a stale pointer from the shim would be logged, not chased into freed memory
std::vector<Alloc> g_allocs;
std::string g_err = "no error";

void logf(const char *fmt, ...) {
    const char *fn = getenv("HT_STUB_LOG");
    if (!fn) return;
    std::lock_guard<std::mutex> lk(g_mu);
    FILE *f = fopen(fn, "a");
    if (!f) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(f, fmt, ap);
    va_end(ap);
    fputc('\n', f);
    fclose(f);
}

std::string cx(const ht_ctx *c) { return c ? "ctx#" + std::to_string(c->index) : std::string("null"); }

std::string dev(const void *p) {
    if (!p) return "null";
    const char *q = static_cast<const char *>(p);
    for (size_t i = 0; i < g_allocs.size(); i++)
        if (q >= g_allocs[i].p && (size_t)(q - g_allocs[i].p) <= g_allocs[i].bytes) return "dev#" + std::to_string(i) + "+" + std::to_string(q - g_allocs[i].p);
    for (size_t i = 0; i < g_allocs.size(); i++)  // outside every allocation: relative to the nearest one below, so the line stays deterministic
        if (q >= g_allocs[i].p) return "dev#" + std::to_string(i) + "+" + std::to_string(q - g_allocs[i].p) + "(outside)";
    return "dev?";
}

std::string host_in(const void *p, size_t n) {
    if (!p) return "null";
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const uint8_t *>(p)[i]) * 16777619u;
    char b[48];
    snprintf(b, sizeof b, "host[%zu]:%08x", n, h);
    return b;
}

std::string ints(const int32_t *p, size_t n) {
    if (!p) return "null";
    std::string s = "[";
    for (size_t i = 0; i < n; i++) s += (i ? "," : "") + std::to_string(p[i]);
    return s + "]";
}

std::string rect(const ht_cs_rect *r) { return r ? ints(&r->x, 4) : std::string("null"); }

void fill_bytes(void *p, size_t n) {
    for (size_t i = 0; i < n; i++) static_cast<uint8_t *>(p)[i] = (uint8_t)(7 * i + 3);
}
void fill_f64(double *p, size_t n) {
    for (size_t i = 0; i < n; i++) p[i] = 0.5 * (double)i + 1;
}
void fill_objs(ht_cs_trackobj *o, size_t n) {
    for (size_t i = 0; i < n; i++) {
        const double b = 10.0 * (double)i;
        o[i] = {b + 1, b + 2, b + 3, b + 4, b + 0.5, (int32_t)i + 5, (int32_t)i + 6, (int32_t)i + 7, (int32_t)i + 8};
    }
}
void fill_hits(ht_hit *h, size_t n) {
    for (size_t i = 0; i < n; i++) h[i] = {(uint32_t)(i / 3), (uint16_t)(i + 1), (uint16_t)(2 * i + 1), (uint8_t)(i % 7), (uint8_t)(i & 3), 0, 0, 0.25 * (double)i - 1};
}
void fill_rects(ht_rect *r, size_t n) {
    for (size_t i = 0; i < n; i++) r[i] = {(double)i + 0.5, (double)i + 1.5, (double)i + 20, (double)i + 30, 0.125 * (double)i, (int32_t)i + 2, 0};
}
void fill_u32(uint32_t *p, size_t n) {
    for (size_t i = 0; i < n; i++) p[i] = (uint32_t)i + 1;
}

// the k-th call after ht_camshift_reserve(ctx, MAGIC + k) fails
bool forced(ht_ctx *c, const char *name) {
    if (c->arm <= 0 || --c->arm > 0) return false;
    c->err = std::string("stub: forced failure of ") + name;
    logf("%s FAILS", name);
    return true;
}
#define ENTER(ctx, name) \
    if (forced(ctx, name)) return HT_ERR_INVALID

}  // namespace

extern "C" {

ht_status ht_create(const ht_config *cfg, const void *blob, size_t len, ht_ctx **out) {
    logf("ht_create struct_size=%u device=%d interval=%d hit_capacity=%u stream=%s queue_capacity=%u flags=%u options=%s blob=%s", cfg->struct_size, cfg->device,
         cfg->interval, cfg->hit_capacity, cfg->stream ? "set" : "null", cfg->queue_capacity, cfg->flags, cfg->options ? cfg->options : "null", host_in(blob, len).c_str());
    if (cfg->device == MAGIC) {
        g_err = "stub: forced failure of ht_create";
        return HT_ERR_NO_DEVICE;
    }
    ht_ctx *c = new ht_ctx();
    std::lock_guard<std::mutex> lk(g_mu);
    c->index = (int)g_ctxs.size();
    g_ctxs.push_back(c);
    *out = c;
    return HT_OK;
}
void ht_destroy(ht_ctx *ctx) { logf("ht_destroy %s", cx(ctx).c_str()); }
const char *ht_last_error(const ht_ctx *ctx) {
    logf("ht_last_error %s", cx(ctx).c_str());
    return ctx ? ctx->err.c_str() : g_err.c_str();
}
int32_t ht_abi_version(void) {
    logf("ht_abi_version");
    return HT_ABI_VERSION;
}

ht_status ht_set_geometry(ht_ctx *ctx, int32_t w, int32_t h, int32_t max_batch, const int32_t *dims, int32_t nlevels) {
    logf("ht_set_geometry %s w=%d h=%d max_batch=%d dims=%s nlevels=%d", cx(ctx).c_str(), w, h, max_batch, ints(dims, 2 * (size_t)(nlevels > 0 ? nlevels : 0)).c_str(), nlevels);
    ENTER(ctx, "ht_set_geometry");
    ctx->w = w, ctx->h = h;
    return HT_OK;
}
int32_t ht_num_levels(const ht_ctx *ctx) {
    logf("ht_num_levels %s", cx(ctx).c_str());
    return 31;
}
ht_status ht_plane(const ht_ctx *ctx, int32_t level, int32_t slot, ht_plane_info *out) {
    logf("ht_plane %s level=%d slot=%d", cx(ctx).c_str(), level, slot);
    if (ctx->w <= 0) return HT_ERR_STATE;
    *out = {ctx->w, ctx->h, ctx->w, 1, 0};
    return HT_OK;
}
uint64_t ht_windows_per_frame(const ht_ctx *ctx) {
    logf("ht_windows_per_frame %s", cx(ctx).c_str());
    return 123456789012ull;
}
uint64_t ht_pyramid_bytes_per_frame(const ht_ctx *ctx) {
    logf("ht_pyramid_bytes_per_frame %s", cx(ctx).c_str());
    return 9876543210ull;
}

ht_status ht_upload_frames(ht_ctx *ctx, const uint8_t *rgba, int32_t n, size_t stride) {
    logf("ht_upload_frames %s rgba=%s n=%d stride=%zu", cx(ctx).c_str(), host_in(rgba, (size_t)n * stride).c_str(), n, stride);
    ENTER(ctx, "ht_upload_frames");
    ctx->bound = n;
    return HT_OK;
}
ht_status ht_upload_frames_async(ht_ctx *ctx, const uint8_t *rgba, int32_t n, size_t stride) {
    logf("ht_upload_frames_async %s rgba=%s n=%d stride=%zu", cx(ctx).c_str(), host_in(rgba, (size_t)n * stride).c_str(), n, stride);
    ENTER(ctx, "ht_upload_frames_async");
    ctx->bound = n;
    return HT_OK;
}
ht_status ht_swap_frames(ht_ctx *ctx) {
    logf("ht_swap_frames %s", cx(ctx).c_str());
    ENTER(ctx, "ht_swap_frames");
    return HT_OK;
}
ht_status ht_bind_frames_device(ht_ctx *ctx, const void *d, int32_t n, size_t stride) {
    logf("ht_bind_frames_device %s frames=%s n=%d stride=%zu", cx(ctx).c_str(), dev(d).c_str(), n, stride);
    ENTER(ctx, "ht_bind_frames_device");
    ctx->bound = n;
    return HT_OK;
}
int32_t ht_frames_bound(const ht_ctx *ctx) {
    logf("ht_frames_bound %s", cx(ctx).c_str());
    return ctx->bound;
}
int32_t ht_frames_enqueued(const ht_ctx *ctx) {
    logf("ht_frames_enqueued %s", cx(ctx).c_str());
    return ctx->bound;
}

ht_status ht_host_alloc(size_t bytes, void **out) {
    logf("ht_host_alloc bytes=%zu", bytes);
    if (bytes == (size_t)MAGIC || !(*out = calloc(1, bytes))) {
        g_err = "stub: forced failure of ht_host_alloc";
        return HT_ERR_NOMEM;
    }
    return HT_OK;
}
void ht_host_free(void *p) {
    logf("ht_host_free");
    free(p);
}
ht_status ht_device_alloc(ht_ctx *ctx, size_t bytes, void **out) {
    logf("ht_device_alloc %s bytes=%zu", cx(ctx).c_str(), bytes);
    ENTER(ctx, "ht_device_alloc");
    char *p = static_cast<char *>(calloc(1, bytes));
    if (!p) {
        ctx->err = "stub: out of memory";
        return HT_ERR_NOMEM;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    g_allocs.push_back({p, bytes, ctx, true});
    *out = p;
    return HT_OK;
}
ht_status ht_device_free(ht_ctx *ctx, void *p) {
    logf("ht_device_free %s buf=%s", cx(ctx).c_str(), dev(p).c_str());
    ENTER(ctx, "ht_device_free");
    for (Alloc &a : g_allocs)
        if (a.p == p && a.live) {
            if (a.owner != ctx) {
                ctx->err = "stub: the buffer belongs to another context";
                return HT_ERR_STATE;
            }
            a.live = false;  // the memory stays: later lines can still name it
            return HT_OK;
        }
    ctx->err = "stub: not a live device buffer";
    return HT_ERR_INVALID;
}
ht_status ht_device_upload(ht_ctx *ctx, void *dst, const void *src, size_t bytes) {
    logf("ht_device_upload %s dst=%s src=%s bytes=%zu", cx(ctx).c_str(), dev(dst).c_str(), host_in(src, bytes).c_str(), bytes);
    ENTER(ctx, "ht_device_upload");
    return HT_OK;
}
ht_status ht_device_download(ht_ctx *ctx, void *dst, const void *src, size_t bytes) {
    logf("ht_device_download %s src=%s bytes=%zu", cx(ctx).c_str(), dev(src).c_str(), bytes);
    ENTER(ctx, "ht_device_download");
    fill_bytes(dst, bytes);
    return HT_OK;
}

ht_status ht_draw_frames_device(ht_ctx *ctx, const void *src, int32_t n, int32_t sw, int32_t sh, size_t pitch, size_t stride, const ht_cs_rect *r, void *dst, size_t dstride) {
    logf("ht_draw_frames_device %s src=%s n=%d sw=%d sh=%d pitch=%zu stride=%zu rect=%s dst=%s dst_stride=%zu", cx(ctx).c_str(), dev(src).c_str(), n, sw, sh, pitch, stride,
         rect(r).c_str(), dev(dst).c_str(), dstride);
    ENTER(ctx, "ht_draw_frames_device");
    if (!dst) ctx->bound = n;
    return HT_OK;
}
ht_status ht_draw_frames(ht_ctx *ctx, const uint8_t *rgba, int32_t n, int32_t sw, int32_t sh, size_t stride, const ht_cs_rect *r) {
    logf("ht_draw_frames %s rgba=%s n=%d sw=%d sh=%d stride=%zu rect=%s", cx(ctx).c_str(), host_in(rgba, (size_t)n * sw * sh * 4).c_str(), n, sw, sh, stride,
         rect(r).c_str());
    ENTER(ctx, "ht_draw_frames");
    ctx->bound = n;
    return HT_OK;
}

ht_status ht_detect_enqueue(ht_ctx *ctx, uint32_t flags) {
    logf("ht_detect_enqueue %s flags=%u", cx(ctx).c_str(), flags);
    ENTER(ctx, "ht_detect_enqueue");
    ctx->big_collect = flags == (uint32_t)MAGIC;
    return HT_OK;
}
ht_status ht_detect_collect(ht_ctx *ctx, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total) {
    logf("ht_detect_collect %s cap=%u counts=%s", cx(ctx).c_str(), cap, counts ? "set" : "null");
    ENTER(ctx, "ht_detect_collect");
    fill_hits(hits, cap);
    if (counts) fill_u32(counts, (size_t)ctx->bound);
    *total = ctx->big_collect ? 70000 : 4;
    if (ctx->big_collect) ctx->err = "stub: 70000 hits";
    return ctx->big_collect ? HT_ERR_CAPACITY : HT_OK;
}
ht_status ht_detect_batch(ht_ctx *ctx, const uint8_t *rgba, int32_t n, int32_t w, int32_t h, size_t stride, uint32_t flags, ht_hit *hits, uint32_t cap, uint32_t *counts,
                          uint32_t *total) {
    logf("ht_detect_batch %s rgba=%s n=%d w=%d h=%d stride=%zu flags=%u cap=%u", cx(ctx).c_str(), host_in(rgba, (size_t)n * stride).c_str(), n, w, h, stride, flags, cap);
    ENTER(ctx, "ht_detect_batch");
    fill_hits(hits, cap);
    fill_u32(counts, (size_t)n);
    ctx->w = w, ctx->h = h, ctx->bound = n;
    if (!ctx->detected) {
        ctx->detected = true;
        *total = 5000;
        ctx->err = "stub: 5000 hits";
        return HT_ERR_CAPACITY;
    }
    *total = cap > 4096 ? cap : 3;
    return HT_OK;
}
ht_status ht_grayscale_batch(ht_ctx *ctx, uint8_t *rgba, int32_t n, int32_t w, int32_t h, size_t stride) {
    logf("ht_grayscale_batch %s rgba=%s n=%d w=%d h=%d stride=%zu", cx(ctx).c_str(), host_in(rgba, (size_t)n * stride).c_str(), n, w, h, stride);
    ENTER(ctx, "ht_grayscale_batch");
    fill_bytes(rgba, (size_t)n * stride);
    return HT_OK;
}
ht_status ht_whitebalance_batch(ht_ctx *ctx, double *out, int32_t n) {
    logf("ht_whitebalance_batch %s n=%d", cx(ctx).c_str(), n);
    ENTER(ctx, "ht_whitebalance_batch");
    fill_f64(out, (size_t)n);
    return HT_OK;
}
ht_status ht_detect_whitebalance(ht_ctx *ctx, double *out, int32_t n) {
    logf("ht_detect_whitebalance %s n=%d", cx(ctx).c_str(), n);
    ENTER(ctx, "ht_detect_whitebalance");
    fill_f64(out, (size_t)n);
    return HT_OK;
}
ht_status ht_detect_collect_best(ht_ctx *ctx, int32_t mn, ht_rect *best, uint32_t *total) {
    logf("ht_detect_collect_best %s min_neighbors=%d", cx(ctx).c_str(), mn);
    ENTER(ctx, "ht_detect_collect_best");
    fill_rects(best, (size_t)ctx->bound);
    *total = 11;
    return HT_OK;
}
ht_status ht_detect_collect_best_requeue(ht_ctx *ctx, int32_t mn, ht_rect *best, uint32_t *total, uint32_t next_flags) {
    logf("ht_detect_collect_best_requeue %s min_neighbors=%d next_flags=%u", cx(ctx).c_str(), mn, next_flags);
    ENTER(ctx, "ht_detect_collect_best_requeue");
    fill_rects(best, (size_t)ctx->bound);
    *total = 12;
    return HT_OK;
}

ht_status ht_camshift_reserve(ht_ctx *ctx, int32_t n) {
    logf("ht_camshift_reserve %s nstreams=%d", cx(ctx).c_str(), n);
    if (n == MAGIC) {
        ctx->err = "stub: forced failure of ht_camshift_reserve";
        return HT_ERR_INVALID;
    }
    if (n > MAGIC && n <= MAGIC + 9) ctx->arm = n - MAGIC;
    return HT_OK;
}
ht_status ht_camshift_init_batch(ht_ctx *ctx, int32_t first, int32_t n, const ht_cs_rect *rects) {
    logf("ht_camshift_init_batch %s first=%d n=%d rects=%s", cx(ctx).c_str(), first, n, ints(&rects->x, 4 * (size_t)n).c_str());
    ENTER(ctx, "ht_camshift_init_batch");
    return HT_OK;
}
ht_status ht_camshift_track_batch(ht_ctx *ctx, int32_t first, int32_t n, int32_t calc, ht_cs_trackobj *out) {
    logf("ht_camshift_track_batch %s first=%d n=%d calc_angles=%d out=%s", cx(ctx).c_str(), first, n, calc, out ? "set" : "null");
    ENTER(ctx, "ht_camshift_track_batch");
    if (out) fill_objs(out, (size_t)n);
    return HT_OK;
}
ht_status ht_camshift_track_collect(ht_ctx *ctx, int32_t n, ht_cs_trackobj *out) {
    logf("ht_camshift_track_collect %s n=%d", cx(ctx).c_str(), n);
    ENTER(ctx, "ht_camshift_track_collect");
    fill_objs(out, (size_t)n);
    return HT_OK;
}
ht_status ht_camshift_init_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_cs_rect *rects) {
    logf("ht_camshift_init_pairs %s pairs=%s n=%d rects=%s", cx(ctx).c_str(), ints(&pairs->stream, 2 * (size_t)n).c_str(), n, ints(&rects->x, 4 * (size_t)n).c_str());
    ENTER(ctx, "ht_camshift_init_pairs");
    return HT_OK;
}
ht_status ht_camshift_track_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t calc, ht_cs_trackobj *out) {
    logf("ht_camshift_track_pairs %s pairs=%s n=%d calc_angles=%d out=%s", cx(ctx).c_str(), ints(&pairs->stream, 2 * (size_t)n).c_str(), n, calc, out ? "set" : "null");
    ENTER(ctx, "ht_camshift_track_pairs");
    if (out) fill_objs(out, (size_t)n);
    return HT_OK;
}
ht_status ht_camshift_track_sequence(ht_ctx *ctx, int32_t first, int32_t n, int32_t calc, const void *const *frames, int32_t ncalls, size_t stride, ht_cs_trackobj *out,
                                     int32_t out_all) {
    std::string f;
    for (int32_t k = 0; k < ncalls; k++) f += (k ? "," : "") + dev(frames[k]);
    logf("ht_camshift_track_sequence %s first=%d n=%d calc_angles=%d frames=[%s] ncalls=%d stride=%zu out=%s out_all=%d", cx(ctx).c_str(), first, n, calc, f.c_str(), ncalls,
         stride, out ? "set" : "null", out_all);
    ENTER(ctx, "ht_camshift_track_sequence");
    if (out) fill_objs(out, (size_t)n * (out_all ? (size_t)ncalls : 1));
    return HT_OK;
}
ht_status ht_camshift_sequence_collect(ht_ctx *ctx, int32_t n, int32_t ncalls, int32_t out_all, ht_cs_trackobj *out) {
    logf("ht_camshift_sequence_collect %s n=%d ncalls=%d out_all=%d", cx(ctx).c_str(), n, ncalls, out_all);
    ENTER(ctx, "ht_camshift_sequence_collect");
    fill_objs(out, (size_t)n * (out_all ? (size_t)ncalls : 1));
    return HT_OK;
}

ht_status ht_camshift_backproject(ht_ctx *ctx, int32_t first, int32_t n, int32_t kind, void *out, size_t stride) {
    logf("ht_camshift_backproject %s first=%d n=%d kind=%d stride=%zu", cx(ctx).c_str(), first, n, kind, stride);
    ENTER(ctx, "ht_camshift_backproject");
    if (kind == HT_BP_F64) fill_f64(static_cast<double *>(out), (size_t)n * stride / 8);
    else fill_bytes(out, (size_t)n * stride);
    return HT_OK;
}
ht_status ht_camshift_backproject_device(ht_ctx *ctx, int32_t first, int32_t n, int32_t kind, void *out, size_t stride) {
    logf("ht_camshift_backproject_device %s first=%d n=%d kind=%d out=%s stride=%zu", cx(ctx).c_str(), first, n, kind, dev(out).c_str(), stride);
    ENTER(ctx, "ht_camshift_backproject_device");
    return HT_OK;
}
ht_status ht_camshift_backproject_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out, size_t stride) {
    logf("ht_camshift_backproject_pairs %s pairs=%s n=%d kind=%d stride=%zu", cx(ctx).c_str(), ints(&pairs->stream, 2 * (size_t)n).c_str(), n, kind, stride);
    ENTER(ctx, "ht_camshift_backproject_pairs");
    if (kind == HT_BP_F64) fill_f64(static_cast<double *>(out), (size_t)n * stride / 8);
    else fill_bytes(out, (size_t)n * stride);
    return HT_OK;
}
ht_status ht_camshift_backproject_pairs_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out, size_t stride) {
    // a pair count the shim let through by overflow would make the table too long to print: its length is enough then
    logf("ht_camshift_backproject_pairs_device %s pairs=%s n=%d kind=%d out=%s stride=%zu", cx(ctx).c_str(), n <= 64 ? ints(&pairs->stream, 2 * (size_t)n).c_str() : "(long)", n,
         kind, dev(out).c_str(), stride);
    ENTER(ctx, "ht_camshift_backproject_pairs_device");
    return HT_OK;
}

ht_status ht_allgather_best_faces(ht_ctx *const *ctxs, int32_t nranks, const ht_rect *const *best, int32_t per, ht_rect *gathered) {
    std::string s;
    for (int32_t i = 0; i < nranks; i++) {
        s += " " + cx(ctxs[i]) + ":";
        for (int32_t f = 0; f < per; f++) {
            const ht_rect &r = best[i][f];
            char b[200];
            snprintf(b, sizeof b, "(%.17g,%.17g,%.17g,%.17g,%.17g,%d,%d)", r.x, r.y, r.width, r.height, r.confidence, r.neighbors, r.reserved);
            s += b;
        }
    }
    logf("ht_allgather_best_faces nranks=%d frames_per_rank=%d%s", nranks, per, s.c_str());
    ENTER(ctxs[0], "ht_allgather_best_faces");
    fill_rects(gathered, (size_t)nranks * (size_t)per);
    return HT_OK;
}
int32_t ht_device_count(void) {
    logf("ht_device_count");
    return 3;
}
uint64_t ht_graph_launches(const ht_ctx *ctx) {
    logf("ht_graph_launches %s", cx(ctx).c_str());
    return 41;
}
ht_status ht_synchronize(ht_ctx *ctx) {
    logf("ht_synchronize %s", cx(ctx).c_str());
    ENTER(ctx, "ht_synchronize");
    return HT_OK;
}

}  // extern "C"

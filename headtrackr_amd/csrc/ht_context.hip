// ht_context.hip — context lifetime, the cascade's and the geometry's plans on the device (ht_cascade_plan.h, ht_geometry_plan.h),
// the host-side post-processing (rect conversion + grouping) and the measurement calls of libheadtrackr_hip.so.  Two more files are
// compiled as part of this one, included at its end: ht_detect_step.hip (a detect batch: enqueue, graph cache, the collect calls,
// whitebalance) and ht_frames.hip (frame buffers and their binding).
//
// Reference behaviour restated here (paths under /root/reference/src/):
//   geometry            ccv.js:110-147      (scale, scale_upto, level sizes, variant planes)
//   hits -> seq rects   ccv.js:227-234,244-245
//   grouping            ccv.js:34-107 (array_group), 249-332 (averaging, nested-rect filter)
#include <sched.h>
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ht_internal.h"
#include "ht_hostpost.h"
#include "ht_geometry_plan.h"
#include "ht_cascade_plan.h"

static thread_local std::string g_create_err;

// roctx (see ht_internal.h)
#include <dlfcn.h>
namespace {
struct Roctx {
    int (*push)(const char *) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            push = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
            pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
            if (!push || !pop) push = nullptr, pop = nullptr;
        }
    }
};
Roctx &roctx() {
    static Roctx r;
    return r;
}
}  // namespace
HtRange::HtRange(const char *name) : on(roctx().push != nullptr) {
    if (on) roctx().push(name);
}
HtRange::~HtRange() {
    if (on) roctx().pop();
}

// Every live context's published frame binding and the ht_device_alloc buffers that outlived their owner (ht_frame_registry.h): the
// registry says what may go, release_buffers frees it — for ht_destroy and for the sweep behind every move of a context's frames
// (ht_frames.hip) alike.
static HtFrameRegistry g_frames;
static void release_buffers(const std::vector<HtFrameBuffer> &list) {
    for (const HtFrameBuffer &a : list) {
        if (a.orphan) {  // whatever a context that has meanwhile re-bound elsewhere still had enqueued against it has to be through
            (void)hipSetDevice(a.device);
            (void)hipDeviceSynchronize();
        }
        (void)hipFree(a.p);
    }
}

static inline HtPostCfg post_cfg(const ht_ctx *c) { return HtPostCfg{c->interval, c->cascade.cw, c->cascade.ch}; }

ht_status ht_fail(ht_ctx *ctx, ht_status st, const std::string &msg) {
    if (ctx)
        ctx->err = msg;
    else
        g_create_err = msg;
    return st;
}

HtProfScope::HtProfScope(ht_ctx *c, const char *name, hipStream_t on) : ctx(c), stream(on ? on : c->stream) {
    if (!ctx->profiling) return;
    for (size_t i = 0; i < ctx->timers.size(); i++)
        if (ctx->timers[i].name == name) idx = (int)i;
    if (idx < 0) {
        ctx->timers.emplace_back();
        ctx->timers.back().name = name;
        idx = (int)ctx->timers.size() - 1;
    }
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
        idx = -1;
        return;
    }
    (void)hipEventRecord(a, stream);
}
HtProfScope::~HtProfScope() {
    if (idx < 0) return;
    (void)hipEventRecord(b, stream);
    ctx->timers[idx].pending.emplace_back(a, b);
    ctx->timers[idx].launches++;
}

extern "C" int32_t ht_abi_version(void) { return HT_ABI_VERSION; }

extern "C" const char *ht_last_error(const ht_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// ---------------------------------------------------------------------------------------------------------
// ht_config.options: "key=value,key=value".  Every key selects among schedules with identical results; the three that do not
// (results incomplete by design: timing experiments) exist only with -DHT_DEBUG_KNOBS.
static bool apply_options(ht_ctx *c, const std::string &opts, std::string &why) {
    size_t pos = 0;
    while (pos < opts.size()) {
        size_t end = opts.find(',', pos);
        if (end == std::string::npos) end = opts.size();
        std::string kv = opts.substr(pos, end - pos);
        pos = end + 1;
        while (!kv.empty() && (kv.front() == ' ')) kv.erase(kv.begin());
        while (!kv.empty() && (kv.back() == ' ')) kv.pop_back();
        if (kv.empty()) continue;
        const size_t eq = kv.find('=');
        const std::string key = kv.substr(0, eq), val = eq == std::string::npos ? "1" : kv.substr(eq + 1);
        char *endp = nullptr;
        const long long v = std::strtoll(val.c_str(), &endp, 10);
        if (val.empty() || (endp && *endp)) {
            why = "option '" + key + "': value is not an integer";
            return false;
        }
        const int iv = (int)std::max<long long>(std::min<long long>(v, 1ll << 30), -(1ll << 30));
        if (key == "rs_rpt") { if (iv >= 1 && iv <= HT_RS_MAX_PASSES) c->rs_rpt = iv; }
        else if (key == "rs_tailtable") c->tail_table = iv < 0 ? 0 : (iv > 2 ? 2 : (int)iv), c->tail_table_forced = true;
        else if (key == "rs_tailcap") c->rs_tailcap = (uint64_t)std::max<long long>(v, 0), c->rs_tailcap_forced = true;
        else if (key == "rs_notail") c->rs_notail = iv != 0;
        else if (key == "rs_nofast") c->rs_nofast = iv != 0;
        else if (key == "rs_nosort") c->rs_nosort = iv != 0;
        else if (key == "rs_bands") c->rs_bands = iv != 0;
        else if (key == "rs_gennames") c->rs_gennames = iv != 0;
        else if (key == "rs_minwg") c->rs_min_wgs = std::max(1, iv);
        else if (key == "rs_k") c->dbg_rs_k = iv;
        else if (key == "rs_group") { if (iv >= 1 && iv <= 64) c->rs_group = iv, c->rs_group_forced = true; }
        else if (key == "early_scan") c->early_scan = iv != 0;
        else if (key == "force_exact") c->dbg_force_exact = iv;
        else if (key == "deep_bias") c->deep_bias = (uint32_t)std::max(0, iv);
        else if (key == "deep_v") c->dbg_deep_v = iv;
        else if (key == "cs_flags") c->cs_flags = iv != 0;
        else if (key == "cs_sync_ring") c->cs_sync_ring = iv != 0;
        else if (key == "cs_pairs_force") c->cs_pairs_force = iv != 0;
        else if (key == "cs_pairs_cluster") c->cs_pairs_cluster = iv != 0;
        else if (key == "fp_sparse") c->fp_sparse = iv != 0;
        else if (key == "deep_grid") c->deep_grid = std::max(1, iv);
        else if (key == "split") c->opt_split = std::max(1, iv);
        else if (key == "cs_fused_min") c->cs_fused_min_streams = std::max(1, iv);
        else if (key == "cs_fused_nt") c->cs_fused_nt = iv;
        else if (key == "cs_keep_hist") c->cs_keep_hist = iv != 0;
        else if (key == "cs_seq_fused") c->cs_seq_fused = iv != 0;
        else if (key == "cs_cluster") c->cs_cluster = iv != 0;
        else if (key == "cs_cluster_min_px") c->cs_cluster_min_px = (uint32_t)std::max(0, iv);
        else if (key == "cs_region") c->cs_region_cap = std::min(40960, std::max(0, iv));
        else if (key == "cs_barrier_budget") c->cs_barrier_budget = std::max(1ll, v);
        else if (key == "graph_max_frames") c->graph_max_frames = std::max(0, iv);
        else if (key == "host_threads") c->host_threads = std::min(64, std::max(0, iv));
        else if (key == "force_rccl") c->force_rccl = iv != 0;
        else if (key == "group_cap") c->grp_cap_opt = std::max(1, iv);
        else if (key == "draw_filter_rows") { if (iv == 0 || iv == 4 || iv == 16) c->draw_filter_rows = iv; }  // k_draw_list_mean_tile's tile rows (0: the shipped 4)
        else if (key == "orient_lanes") { if (iv >= 0 && iv <= 2) c->orient_lanes = iv; }  // the oriented draw's lane mapping for odd rot (0: the shipped one)
#ifdef HT_DEBUG_KNOBS
        else if (key == "stop_stage") c->dbg_stop_stage = iv;                        // the tile kernel stops before this stage
        else if (key == "cs_iters") c->dbg_cs_iters = std::min(10, std::max(0, iv));   // mean-shift iterations (camshift.js:284 has 10)
        else if (key == "rs_maxgen") c->rs_maxgen = iv;                                // pyramid generations built
#endif
        else {
            why = "unknown option '" + key + "'";
            return false;
        }
    }
    return true;
}

// one table of a plan (cascade, geometry) on the device
template <typename T>
static ht_status upload_table(ht_ctx *c, T *&dst, const std::vector<T> &src) {
    if (src.empty()) return HT_OK;
    HT_HIP(c, hipMalloc(&dst, src.size() * sizeof(T)));
    HT_HIP(c, hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return HT_OK;
}

extern "C" ht_status ht_create(const ht_config *cfg, const void *cascade_blob, size_t cascade_len, ht_ctx **out) {
    // ABI 1 callers pass the struct without its last member (options)
    if (!cfg || !out || (cfg->struct_size != sizeof(ht_config) && cfg->struct_size != offsetof(ht_config, options)))
        return ht_fail(nullptr, HT_ERR_INVALID, "ht_create: bad config");
    *out = nullptr;
    if (cfg->interval < 1 || cfg->interval > 12) return ht_fail(nullptr, HT_ERR_INVALID, "ht_create: interval must be 1..12");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return ht_fail(nullptr, HT_ERR_NO_DEVICE, "ht_create: no HIP device visible (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return ht_fail(nullptr, HT_ERR_INVALID, "ht_create: device ordinal out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return ht_fail(nullptr, HT_ERR_HIP, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return ht_fail(nullptr, HT_ERR_NO_DEVICE, std::string("ht_create: device is ") + prop.gcnArchName + ", this build is gfx950-only");
    ht_ctx *c = new (std::nothrow) ht_ctx();
    if (!c) return ht_fail(nullptr, HT_ERR_NOMEM, "ht_create: out of host memory");
    c->device = cfg->device;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    c->interval = cfg->interval;
    c->next = cfg->interval + 1;
    if (cfg->hit_capacity) c->hit_capacity = cfg->hit_capacity;
    c->queue_capacity_cfg = cfg->queue_capacity;
    std::string why;
    if (!ht_plan_cascade((const uint8_t *)cascade_blob, cascade_len, &c->cascade, &why)) {
        delete c;
        return ht_fail(nullptr, HT_ERR_INVALID, "ht_create: " + why);
    }
    ht_status st = HT_OK;
    auto bail = [&](ht_status s) {
        g_create_err = c->err;
        ht_destroy(c);
        return s;
    };
    if (hipSetDevice(c->device) != hipSuccess) {
        c->err = "hipSetDevice failed";
        return bail(HT_ERR_HIP);
    }
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            c->err = "hipStreamCreate failed";
            return bail(HT_ERR_HIP);
        }
        c->own_stream = true;
    }
    // per-context options (schedule selectors for tests / A-B runs): from the config string only — this library reads no environment
    {
        std::string opts = (cfg->struct_size >= offsetof(ht_config, options) + sizeof(const char *) && cfg->options) ? cfg->options : "";
#ifdef HT_DEBUG_KNOBS  // instrumented builds (tools/build_alt.py) may also be steered from the shell
        if (const char *e = std::getenv("HT_OPTIONS")) opts += std::string(opts.empty() ? "" : ",") + e;
#endif
        std::string why;
        if (!apply_options(c, opts, why)) {
            c->err = "ht_create: " + why;
            return bail(HT_ERR_INVALID);
        }
    }
    if (c->early_scan) {
        if (hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ev_early_ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_early_done, hipEventDisableTiming) != hipSuccess) {
            c->err = "hipStreamCreate (aux) failed";
            return bail(HT_ERR_HIP);
        }
    }
    c->builtin_cascade = ht_scan_is_builtin_cascade((const uint8_t *)cascade_blob, cascade_len) && c->interval >= 1;
    ht_plan_cascade_split(&c->cascade, c->builtin_cascade, c->opt_split);
    const HtCascadePlan &P = c->cascade;
    if ((st = upload_table(c, c->d_deep_feats, P.deep)) != HT_OK || (st = upload_table(c, c->d_stages, P.dev_stages)) != HT_OK ||
        (st = upload_table(c, c->d_tile_feats, P.tile)) != HT_OK || (st = upload_table(c, c->d_fp_feats, P.fp)) != HT_OK ||
        (st = upload_table(c, c->d_patch_feats, P.patch)) != HT_OK || (st = upload_table(c, c->d_packed_feats, P.packed)) != HT_OK)
        return bail(st);
    if (hipHostMalloc(reinterpret_cast<void **>(&c->h_pinned), sizeof(HtCounters) + (size_t)HT_PINNED_HITS * sizeof(ht_hit), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&c->d_stats, sizeof(unsigned long long) * 64 * HT_STAT_SHARDS) != hipSuccess ||
        // counters and hits in ONE allocation, counters first: ht_detect_collect fetches both with a single copy
        hipMalloc(reinterpret_cast<void **>(&c->d_counters), sizeof(HtCounters) + (size_t)c->hit_capacity * sizeof(ht_hit)) != hipSuccess) {
        c->err = "hipMalloc(hits) failed";
        return bail(HT_ERR_NOMEM);
    }
    c->frame_slot.device = c->device;
    g_frames.add(&c->frame_slot);
    c->d_hits = reinterpret_cast<ht_hit *>(reinterpret_cast<uint8_t *>(c->d_counters) + sizeof(HtCounters));
    *out = c;
    return HT_OK;
}

static void destroy_graphs(ht_ctx *c);
static void free_geometry(ht_ctx *c) {
    destroy_graphs(c);  // captured launch sequences hold this geometry's pointers
    if (c->d_levels) (void)hipFree(c->d_levels), c->d_levels = nullptr;
    if (c->d_arena) (void)hipFree(c->d_arena), c->d_arena = nullptr;
    if (c->d_scales) (void)hipFree(c->d_scales), c->d_scales = nullptr;
    if (c->d_queue) (void)hipFree(c->d_queue), c->d_queue = nullptr;
    for (auto p : c->d_gen_blocks)
        if (p) (void)hipFree(p);
    c->d_gen_blocks.clear();
    if (c->d_tile_recs) (void)hipFree(c->d_tile_recs), c->d_tile_recs = nullptr;
    if (c->d_tail_jobs) (void)hipFree(c->d_tail_jobs), c->d_tail_jobs = nullptr;
    if (c->d_tail_prefix) (void)hipFree(c->d_tail_prefix), c->d_tail_prefix = nullptr;
    if (c->d_tail_taps) (void)hipFree(c->d_tail_taps), c->d_tail_taps = nullptr;
    if (c->d_tail_taps_fast) (void)hipFree(c->d_tail_taps_fast), c->d_tail_taps_fast = nullptr;
    if (c->d_tail_tapref) (void)hipFree(c->d_tail_tapref), c->d_tail_tapref = nullptr;
    c->plan.tail_first_gen = 0;
    c->plan.gens.clear();
    c->plan.gen_blocks.clear();
    c->plan.scales.clear();
}

extern "C" void ht_destroy(ht_ctx *c) {
    if (!c) return;
    // same rule as ht_device_free: never free HBM under a live context that has frames bound inside it — such a buffer outlives its owner
    // as an orphan instead.  release: the buffers nobody is bound to any more, this context's own and orphans of earlier destroys
    g_frames.remove(&c->frame_slot);
    const std::vector<HtFrameBuffer> release = g_frames.retire(c->device, c->user_allocs);
    c->user_allocs.clear();
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream), (void)hipStreamDestroy(c->aux_stream);
    if (c->ev_early_ready) (void)hipEventDestroy(c->ev_early_ready);
    if (c->ev_early_done) (void)hipEventDestroy(c->ev_early_done);
    free_geometry(c);
    if (c->d_tile_feats) (void)hipFree(c->d_tile_feats);
    if (c->d_deep_feats) (void)hipFree(c->d_deep_feats);
    if (c->d_patch_feats) (void)hipFree(c->d_patch_feats);
    if (c->d_packed_feats) (void)hipFree(c->d_packed_feats);
    if (c->d_fp_feats) (void)hipFree(c->d_fp_feats);
    if (c->d_stages) (void)hipFree(c->d_stages);
    if (c->d_frames_own) (void)hipFree(c->d_frames_own);
    if (c->d_frames_back) (void)hipFree(c->d_frames_back);
    if (c->ev_copy_done) (void)hipEventDestroy(c->ev_copy_done);
    if (c->ev_front_free) (void)hipEventDestroy(c->ev_front_free);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->d_counters) (void)hipFree(c->d_counters);  // (d_hits lives in the same allocation)
    if (c->d_stats) (void)hipFree(c->d_stats);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    if (c->h_wb_pinned) (void)hipHostFree(c->h_wb_pinned);
    ht_camshift_free(c);
    ht_backproject_free(c);
    ht_ingest_free(c);
    ht_cs_pairs_free(c);
    ht_cs_best_free(c);
    ht_cs_faces_free(c);
    ht_group_free(c);
    if (c->d_gather) (void)hipFree(c->d_gather);
    release_buffers(release);
    (void)hipSetDevice(c->device);
    for (auto &t : c->timers)
        for (auto &p : t.pending) (void)hipEventDestroy(p.first), (void)hipEventDestroy(p.second);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ---------------------------------------------------------------------------------------------------------
// geometry, ccv.js:110-147: planned on the host by ht_plan_geometry (ht_geometry_plan.h), uploaded here

// Builds every table / allocation of one geometry.  On any failure the caller (ht_set_geometry) frees what was built and
// leaves the context without a geometry, so a retry (e.g. with a smaller max_batch after HT_ERR_NOMEM) starts clean.
static ht_status set_geometry_impl(ht_ctx *c, int32_t width, int32_t height, int32_t max_batch, const int32_t *level_dims, int n, int upto) {
    c->W = width;
    c->H = height;
    c->max_batch = max_batch;
    c->nlevels = n;
    c->upto = upto;

    HtPlanInputs in;
    in.interval = c->interval, in.next = c->next, in.cw = c->cascade.cw, in.ch = c->cascade.ch;
    in.rs_rpt = c->rs_rpt, in.rs_nofast = c->rs_nofast, in.rs_nosort = c->rs_nosort, in.rs_notail = c->rs_notail;
    in.rs_tailcap = c->rs_tailcap, in.rs_tailcap_forced = c->rs_tailcap_forced;
    in.tail_table = c->tail_table, in.tail_table_forced = c->tail_table_forced;
    in.early_scan = c->early_scan, in.aux_stream = c->aux_stream != nullptr;
    in.queue_capacity_cfg = c->queue_capacity_cfg;
    HtGeometryPlan &P = c->plan;
    std::string why;
    ht_status st = ht_plan_geometry(in, width, height, max_batch, level_dims, n, upto, &P, &why);
    if (st != HT_OK) return ht_fail(c, st, why);

    c->d_gen_blocks.assign(P.gens.size(), nullptr);
    for (size_t g = 1; g < P.gens.size(); g++)
        if ((st = upload_table(c, c->d_gen_blocks[g], P.gen_tiles[g])) != HT_OK) return st;
    HT_HIP(c, hipMalloc(&c->d_levels, sizeof(HtDevLevel) * HT_MAX_LEVELS));
    HT_HIP(c, hipMemcpy(c->d_levels, P.levels, sizeof(HtDevLevel) * n, hipMemcpyHostToDevice));
    if (hipMalloc(&c->d_arena, P.arena_stride * (uint64_t)max_batch) != hipSuccess)
        return ht_fail(c, HT_ERR_NOMEM, "ht_set_geometry: hipMalloc(pyramid arena) failed");
    HT_HIP(c, hipMemset(c->d_arena, 0, P.arena_stride * (uint64_t)max_batch));
    if ((st = upload_table(c, c->d_tail_jobs, P.tail_jobs)) != HT_OK || (st = upload_table(c, c->d_tail_prefix, P.tail_prefix)) != HT_OK ||
        (st = upload_table(c, c->d_tail_taps, P.tail_taps)) != HT_OK || (st = upload_table(c, c->d_tail_taps_fast, P.tail_taps_fast)) != HT_OK ||
        (st = upload_table(c, c->d_tail_tapref, P.tail_tapref)) != HT_OK || (st = upload_table(c, c->d_tile_recs, P.tile_recs)) != HT_OK ||
        (st = upload_table(c, c->d_scales, P.scales)) != HT_OK)
        return st;
    if (hipMalloc(&c->d_queue, (size_t)P.queue_capacity * sizeof(HtQueueEntry) + HT_DEEP_CTR_BYTES) != hipSuccess)  // + the deep kernel's work counters
        return ht_fail(c, HT_ERR_NOMEM, "ht_set_geometry: hipMalloc(survivor queue) failed");
    return HT_OK;
}

extern "C" ht_status ht_set_geometry(ht_ctx *c, int32_t width, int32_t height, int32_t max_batch, const int32_t *level_dims,
                                     int32_t nlevels_in) {
    if (!c) return HT_ERR_INVALID;
    if (width <= 0 || height <= 0 || width > 16384 || height > 16384 || max_batch <= 0)
        return ht_fail(c, HT_ERR_INVALID, "ht_set_geometry: width/height must be 1..16384 and max_batch > 0");
    HT_HIP(c, hipSetDevice(c->device));
    const int upto = (int)std::floor(std::log((double)std::min(c->cascade.cw, c->cascade.ch)) / std::log(ht_scale_of(c->interval)));  // ccv.js:112
    const int n = upto + c->next * 2;  // ccv.js:113
    if (n > HT_MAX_LEVELS) return ht_fail(c, HT_ERR_INVALID, "ht_set_geometry: too many pyramid levels");
    if (level_dims && nlevels_in != n) return ht_fail(c, HT_ERR_INVALID, "ht_set_geometry: level_dims has the wrong number of levels");
    if (level_dims) {  // everything that can be rejected is rejected before the current geometry is torn down
        std::string why;
        const ht_status st = ht_check_level_dims(c->next, width, height, level_dims, n, &why);
        if (st != HT_OK) return ht_fail(c, st, why);
    }
    if (c->W == width && c->H == height && c->max_batch >= max_batch && c->nlevels == n && !level_dims) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->copy_stream) HT_HIP(c, hipStreamSynchronize(c->copy_stream));
    free_geometry(c);
    // frames bound / uploaded for the old geometry (incl. a pending ht_upload_frames_async) do not survive a size change
    ht_frames_set(c, nullptr, 0, 0);
    c->enq_nframes = 0;
    c->wb_collected_n = -1;
    c->back_n = 0;
    c->enqueued = false;
    const ht_status st = set_geometry_impl(c, width, height, max_batch, level_dims, n, upto);
    if (st != HT_OK) {  // no half-built geometry: the early-out above must not fire on a retry
        (void)hipGetLastError();  // a failed hipMalloc leaves a sticky error that the next launch check would report
        free_geometry(c);
        c->W = c->H = c->max_batch = c->nlevels = c->upto = 0;
    }
    return st;
}

extern "C" int32_t ht_num_levels(const ht_ctx *c) { return c ? c->nlevels : 0; }
extern "C" uint64_t ht_windows_per_frame(const ht_ctx *c) { return c ? c->plan.windows_per_frame : 0; }
extern "C" uint64_t ht_pyramid_bytes_per_frame(const ht_ctx *c) { return c ? c->plan.pyr_bytes : 0; }

extern "C" ht_status ht_plane(const ht_ctx *c, int32_t level, int32_t slot, ht_plane_info *out) {
    if (!c || !out || level < 0 || level >= c->nlevels || slot < 0 || slot > 3) return HT_ERR_INVALID;
    const HtDevLevel &L = c->plan.levels[level];
    out->width = L.w;
    out->height = L.h;
    out->stride = L.stride;
    out->present = L.off[slot] != 0xffffffffu;
    out->offset = out->present ? L.off[slot] : 0;
    return HT_OK;
}

extern "C" ht_status ht_pyramid_readback(ht_ctx *c, int32_t frame, int32_t level, int32_t slot, uint8_t *out, size_t cap) {
    if (!c || !out) return HT_ERR_INVALID;
    if (frame < 0 || frame >= c->max_batch || level < 0 || level >= c->nlevels || slot < 0 || slot > 3)
        return ht_fail(c, HT_ERR_INVALID, "ht_pyramid_readback: index out of range");
    const HtDevLevel &L = c->plan.levels[level];
    if (L.off[slot] == 0xffffffffu) return ht_fail(c, HT_ERR_INVALID, "ht_pyramid_readback: plane does not exist");
    if (cap < (size_t)L.w * L.h) return ht_fail(c, HT_ERR_CAPACITY, "ht_pyramid_readback: buffer too small");
    if (L.w == 0 || L.h == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    HT_HIP(c, hipMemcpy2D(out, L.w, c->d_arena + (uint64_t)frame * c->plan.arena_stride + L.off[slot], L.stride, L.w, L.h, hipMemcpyDeviceToHost));
    return HT_OK;
}

extern "C" ht_status ht_stage_counts(ht_ctx *c, uint64_t *counts, int32_t n) {
    if (!c || !counts || n < (int32_t)c->cascade.nstages + 1) return HT_ERR_INVALID;
    for (uint32_t j = 0; j <= c->cascade.nstages; j++) counts[j] = c->h_stage_in[j];
    for (int32_t j = (int32_t)c->cascade.nstages + 1; j < std::min<int32_t>(n, 64); j++) counts[j] = c->h_stage_in[j];  // raw counter row (timeline builds)
    return HT_OK;
}

extern "C" ht_status ht_grayscale_batch(ht_ctx *c, uint8_t *host_rgba, int32_t n, int32_t width, int32_t height, size_t frame_stride) {
    if (!c || !host_rgba || n <= 0 || width <= 0 || height <= 0 || frame_stride < (size_t)width * height * 4) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    const size_t fbytes = (size_t)width * height * 4;
    uint8_t *d = nullptr;
    if (hipMalloc(&d, fbytes * n) != hipSuccess) return ht_fail(c, HT_ERR_NOMEM, "ht_grayscale_batch: hipMalloc failed");
    ht_status st = HT_OK;
    hipError_t e = hipMemcpy2DAsync(d, fbytes, host_rgba, frame_stride, fbytes, n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        const int W0 = c->W, H0 = c->H;
        c->W = width, c->H = height;  // the in-place kernel only needs the pixel count
        st = ht_launch_gray_inplace(c, d, n, fbytes);
        c->W = W0, c->H = H0;
    }
    if (e == hipSuccess && st == HT_OK) e = hipMemcpy2DAsync(host_rgba, frame_stride, d, fbytes, fbytes, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return ht_fail(c, HT_ERR_HIP, std::string("ht_grayscale_batch: ") + hipGetErrorString(e));
    return st;
}

// ---------------------------------------------------------------------------------------------------------
// host post-processing

extern "C" ht_status ht_hits_to_rects(const ht_ctx *c, const ht_hit *hits, uint32_t n, ht_rect *out) {
    if (!c || (n && (!hits || !out))) return HT_ERR_INVALID;
    const HtPostCfg cfg = post_cfg(c);
    double sx[HT_MAX_LEVELS];
    ht_post_level_scales(cfg, sx);
    return ht_post_hits_to_rects(cfg, sx, hits, n, out);
}

extern "C" ht_status ht_group_rects(const ht_rect *seq, uint32_t n, int32_t min_neighbors, ht_rect *out, uint32_t *nout) {
    return ht_post_group_rects(seq, n, min_neighbors, out, nout);
}

extern "C" ht_status ht_best_faces(const ht_ctx *c, const ht_hit *hits, const uint32_t *counts, int32_t nframes, int32_t min_neighbors,
                                   ht_rect *best) {
    if (!c || !counts || !best || nframes < 0) return HT_ERR_INVALID;
    const HtPostCfg cfg = post_cfg(c);
    double sx[HT_MAX_LEVELS];
    ht_post_level_scales(cfg, sx);  // once per batch, not once per frame
    size_t k = 0;
    for (int f = 0; f < nframes; f++) {
        const ht_status st = ht_post_best_face(cfg, sx, hits ? hits + k : nullptr, counts[f], min_neighbors, &best[f]);
        if (st != HT_OK) return st;
        k += counts[f];
    }
    return HT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// measurement

extern "C" ht_status ht_profile(ht_ctx *c, int32_t on) {
    if (!c) return HT_ERR_INVALID;
    c->profiling = on != 0;
    return HT_OK;
}

extern "C" ht_status ht_kernel_times(ht_ctx *c, ht_kernel_time *out, int32_t *n, int32_t reset) {
    if (!c || !n) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    for (auto &t : c->timers) {
        for (auto &p : t.pending) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) t.ms += ms;
            (void)hipEventDestroy(p.first);
            (void)hipEventDestroy(p.second);
        }
        t.pending.clear();
    }
    const int cap = *n;
    int k = 0;
    for (auto &t : c->timers) {
        if (out && k < cap) {
            std::memset(&out[k], 0, sizeof(ht_kernel_time));
            std::strncpy(out[k].name, t.name.c_str(), sizeof(out[k].name) - 1);
            out[k].ms = t.ms;
            out[k].launches = t.launches;
        }
        k++;
    }
    // which form of k_cs_track_fused the launches took (chosen per launch, ht_camshift.hip): counted with profiling on or off
    static const char *const form_names[2] = {"cs_fused_launches_1024", "cs_fused_launches_512"};
    for (int f = 0; f < 2; f++) {
        if (!c->cs_fused_launches[f]) continue;
        if (out && k < cap) {
            std::memset(&out[k], 0, sizeof(ht_kernel_time));
            std::strncpy(out[k].name, form_names[f], sizeof(out[k].name) - 1);
            out[k].launches = c->cs_fused_launches[f];
        }
        k++;
    }
    // frames of device-grouped batches (ht_group.hip) whose status word said "over the cap" and that the host finished: counted like the
    // forms above, profiling on or off
    if (c->grp_over_cap_frames) {
        if (out && k < cap) {
            std::memset(&out[k], 0, sizeof(ht_kernel_time));
            std::strncpy(out[k].name, "grp_over_cap_frames", sizeof(out[k].name) - 1);
            out[k].launches = c->grp_over_cap_frames;
        }
        k++;
    }
    *n = k;
    if (reset) c->timers.clear(), c->cs_fused_launches[0] = c->cs_fused_launches[1] = 0, c->grp_over_cap_frames = 0;
    return HT_OK;
}

extern "C" void *ht_stream(const ht_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" ht_status ht_synchronize(ht_ctx *c) {
    if (!c) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the detect step and the frames: compiled here, written in files of their own
#include "ht_detect_step.hip"
#include "ht_frames.hip"

// ht_context.hip — context lifetime, the cascade's and the geometry's plans on the device (ht_cascade_plan.h, ht_geometry_plan.h),
// frame binding, result collection and the host-side post-processing (rect conversion + grouping) of libheadtrackr_hip.so.
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

// every live context of the process: ht_device_free looks for OTHER contexts that still have frames bound inside the buffer
#include <atomic>
#include <mutex>
static std::mutex g_live_mu;
static std::vector<ht_ctx *> g_live;
// ht_device_alloc buffers whose owning context was destroyed while ANOTHER live context still had frames bound inside them (a batch
// host shares one frame buffer between its pipelined contexts): kept alive here and freed by the ht_destroy after which no live
// context is bound inside them any more — never under a context that would read freed HBM on its next enqueue.
struct HtOrphan {
    void *p;
    size_t bytes;
    int device;
    bool orphan;  // false: released by its own context's ht_destroy
};
static std::vector<HtOrphan> g_orphans;
static std::atomic<int> g_orphan_count{0};  // g_orphans.size(), readable without the lock: the frame-binding calls look at it first

// g_live_mu held.  Reads the other contexts' d_frames without their lock: a context being re-bound concurrently with the destruction
// or ht_device_free of the buffer it is bound to is a caller error (include/headtrackr_hip.h, "Lifetime of shared frame buffers").
static bool bound_by_live_context(const ht_ctx *except, int device, const void *p, size_t bytes) {
    const uint8_t *pb = static_cast<const uint8_t *>(p);
    for (const ht_ctx *o : g_live)
        if (o != except && o->device == device && o->d_frames && o->d_frames >= pb && o->d_frames < pb + bytes) return true;
    return false;
}

// A context's frames moved (bind / upload / swap / free): orphans that no live context is bound inside any more are released here as
// well, not only by some later ht_destroy — a host that re-binds its last binder elsewhere and never destroys anything would keep
// the HBM for the life of the process.  One relaxed load when there are no orphans (the streaming hosts bind per step).
static void sweep_orphans(ht_ctx *c) {
    if (g_orphan_count.load(std::memory_order_relaxed) == 0) return;
    std::vector<HtOrphan> release;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        for (size_t i = 0; i < g_orphans.size();) {
            if (!bound_by_live_context(nullptr, g_orphans[i].device, g_orphans[i].p, g_orphans[i].bytes)) {
                release.push_back(g_orphans[i]);
                g_orphans.erase(g_orphans.begin() + (long)i);
            } else {
                i++;
            }
        }
        g_orphan_count.store((int)g_orphans.size(), std::memory_order_relaxed);
    }
    for (auto &a : release) {  // whatever the context that just moved away (or anybody else) still had enqueued against it has to be through
        (void)hipSetDevice(a.device);
        (void)hipDeviceSynchronize();
        (void)hipFree(a.p);
    }
    if (!release.empty() && c) (void)hipSetDevice(c->device);
}

static inline HtPostCfg post_cfg(const ht_ctx *c) { return HtPostCfg{c->interval, c->cascade.cw, c->cascade.ch}; }

// workers for a batch of `frames` frames holding `hits` raw hits: option host_threads, or (auto) up to 7 when the batch is worth it
static int ht_host_workers(const ht_ctx *c, int frames, uint32_t hits) {
    if (c->host_threads == 0) return 0;
    if (c->host_threads > 0) return c->host_threads;
    if (frames < 32 || hits < 256) return 0;  // a live feed's frame or two: the hand-off would cost more than the work
    // auto: half of this process's share of the host cores — the cores its affinity mask allows, divided by the GPUs of the node (a
    // one-process-per-GPU job runs one such pool per GPU: 8 ranks x 7 spinning workers must not pin 64 cores of a small host)
    static const int share = [] {
        cpu_set_t set;
        CPU_ZERO(&set);
        int cpus = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
        int ngpu = 1;
        if (hipGetDeviceCount(&ngpu) != hipSuccess || ngpu < 1) ngpu = 1;
        return std::max(0, std::min(7, cpus / (2 * ngpu) - 1));
    }();
    return share;
}


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
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.push_back(c);
    }
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
    std::vector<HtOrphan> release;  // buffers nobody is bound to any more: this context's own and orphans of earlier destroys
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), c), g_live.end());
        for (auto &a : c->user_allocs) {
            // same rule as ht_device_free: never free HBM under a live context that has frames bound inside it — the buffer outlives
            // its owner as an orphan instead
            if (bound_by_live_context(c, c->device, a.first, a.second)) g_orphans.push_back(HtOrphan{a.first, a.second, c->device, true});
            else release.push_back(HtOrphan{a.first, a.second, c->device, false});
        }
        c->user_allocs.clear();
        for (size_t i = 0; i < g_orphans.size();) {
            if (!bound_by_live_context(nullptr, g_orphans[i].device, g_orphans[i].p, g_orphans[i].bytes)) {
                release.push_back(g_orphans[i]);
                g_orphans.erase(g_orphans.begin() + (long)i);
            } else {
                i++;
            }
        }
        g_orphan_count.store((int)g_orphans.size(), std::memory_order_relaxed);
    }
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
    for (auto &a : release) {
        if (a.orphan) {  // whatever a context that has meanwhile re-bound elsewhere still had enqueued against it has to be through
            (void)hipSetDevice(a.device);
            (void)hipDeviceSynchronize();
        }
        (void)hipFree(a.p);
    }
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
    c->nframes = c->enq_nframes = 0;
    c->wb_collected_n = -1;
    c->back_n = 0;
    c->d_frames = nullptr;
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

// ---------------------------------------------------------------------------------------------------------
// frames

extern "C" ht_status ht_upload_frames(ht_ctx *c, const uint8_t *host_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_upload_frames");
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, "ht_upload_frames: call ht_set_geometry first");
    const size_t fbytes = (size_t)c->W * c->H * 4;
    if (!host_rgba || n <= 0 || n > c->max_batch || frame_stride < fbytes)
        return ht_fail(c, HT_ERR_INVALID, "ht_upload_frames: bad frame count or stride");
    HT_HIP(c, hipSetDevice(c->device));
    const size_t need = fbytes * (size_t)n;
    const ht_status st = ht_frames_own_reserve(c, need, "ht_upload_frames");
    if (st != HT_OK) return st;
    if (frame_stride == fbytes) {
        HT_HIP(c, hipMemcpyAsync(c->d_frames_own, host_rgba, need, hipMemcpyHostToDevice, c->stream));
    } else {
        HT_HIP(c, hipMemcpy2DAsync(c->d_frames_own, fbytes, host_rgba, frame_stride, fbytes, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    ht_frames_bind_own(c, n);
    return HT_OK;
}

// The context's own frame buffer, grown on demand (what ht_upload_frames and the bind form of ht_draw_frames_device write), and the
// binding of its first n frames.
ht_status ht_frames_own_reserve(ht_ctx *c, size_t need, const char *fn) {
    if (c->d_frames_own_bytes >= need) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_frames == c->d_frames_own) c->d_frames = nullptr, c->nframes = 0;  // bound inside the buffer that goes away (the caller binds the new one)
    if (c->d_frames_own) (void)hipFree(c->d_frames_own);
    c->d_frames_own = nullptr;
    c->d_frames_own_bytes = 0;
    if (hipMalloc(&c->d_frames_own, need) != hipSuccess) return (void)hipGetLastError(), ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": hipMalloc failed");
    c->d_frames_own_bytes = need;
    return HT_OK;
}
void ht_frames_bind_own(ht_ctx *c, int n) {
    c->d_frames = c->d_frames_own;
    c->frame_stride = (size_t)c->W * c->H * 4;
    c->nframes = n;
    sweep_orphans(c);
}

extern "C" ht_status ht_upload_frames_async(ht_ctx *c, const uint8_t *host_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, "ht_upload_frames_async: call ht_set_geometry first");
    const size_t fbytes = (size_t)c->W * c->H * 4;
    if (!host_rgba || n <= 0 || n > c->max_batch || frame_stride < fbytes)
        return ht_fail(c, HT_ERR_INVALID, "ht_upload_frames_async: bad frame count or stride");
    HT_HIP(c, hipSetDevice(c->device));
    if (!c->copy_stream) {
        HT_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HT_HIP(c, hipEventCreateWithFlags(&c->ev_copy_done, hipEventDisableTiming));
        HT_HIP(c, hipEventCreateWithFlags(&c->ev_front_free, hipEventDisableTiming));
    }
    const size_t need = fbytes * (size_t)n;
    if (c->d_frames_back_bytes < need) {
        HT_HIP(c, hipStreamSynchronize(c->copy_stream));
        if (c->d_frames_back) (void)hipFree(c->d_frames_back);
        c->d_frames_back = nullptr;
        c->d_frames_back_bytes = 0;
        if (hipMalloc(&c->d_frames_back, need) != hipSuccess) return ht_fail(c, HT_ERR_NOMEM, "ht_upload_frames_async: hipMalloc failed");
        c->d_frames_back_bytes = need;
    }
    // the back buffer was the front buffer until the last swap: kernels enqueued before that swap may still read it
    HT_HIP(c, hipStreamWaitEvent(c->copy_stream, c->ev_front_free, 0));
    if (frame_stride == fbytes) {
        HT_HIP(c, hipMemcpyAsync(c->d_frames_back, host_rgba, need, hipMemcpyHostToDevice, c->copy_stream));
    } else {
        HT_HIP(c, hipMemcpy2DAsync(c->d_frames_back, fbytes, host_rgba, frame_stride, fbytes, (size_t)n, hipMemcpyHostToDevice, c->copy_stream));
    }
    HT_HIP(c, hipEventRecord(c->ev_copy_done, c->copy_stream));
    c->back_n = n;
    return HT_OK;
}

extern "C" ht_status ht_swap_frames(ht_ctx *c) {
    if (!c) return HT_ERR_INVALID;
    if (c->back_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_swap_frames: no ht_upload_frames_async pending");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventRecord(c->ev_front_free, c->stream));            // everything enqueued so far used the old front buffer
    HT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_copy_done, 0));      // later kernels wait for the copy, the host does not
    std::swap(c->d_frames_own, c->d_frames_back);
    std::swap(c->d_frames_own_bytes, c->d_frames_back_bytes);
    c->d_frames = c->d_frames_own;
    c->frame_stride = (size_t)c->W * c->H * 4;
    c->nframes = c->back_n;
    c->back_n = 0;
    sweep_orphans(c);
    return HT_OK;
}

extern "C" ht_status ht_bind_frames_device(ht_ctx *c, const void *dev_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, "ht_bind_frames_device: call ht_set_geometry first");
    if (!dev_rgba || n <= 0 || n > c->max_batch || frame_stride < (size_t)c->W * c->H * 4 || (frame_stride & 3) ||
        ((uintptr_t)dev_rgba & 3))
        return ht_fail(c, HT_ERR_INVALID, "ht_bind_frames_device: bad pointer, frame count or stride (4-byte alignment required)");
    c->d_frames = (const uint8_t *)dev_rgba;
    c->frame_stride = frame_stride;
    c->nframes = n;
    sweep_orphans(c);
    return HT_OK;
}

extern "C" int32_t ht_frames_bound(const ht_ctx *c) { return c ? c->nframes : 0; }
extern "C" int32_t ht_frames_enqueued(const ht_ctx *c) { return (c && c->enqueued) ? c->enq_nframes : 0; }

extern "C" ht_status ht_host_alloc(size_t bytes, void **out) {
    if (!out || bytes == 0) return HT_ERR_INVALID;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(nullptr, HT_ERR_NOMEM, "ht_host_alloc: hipHostMalloc failed");
    }
    return HT_OK;
}
extern "C" void ht_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
extern "C" ht_status ht_device_alloc(ht_ctx *c, size_t bytes, void **out) {
    if (!c || !out || bytes == 0) return HT_ERR_INVALID;
    *out = nullptr;
    HT_HIP(c, hipSetDevice(c->device));
    if (hipMalloc(out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, "ht_device_alloc: hipMalloc failed");
    }
    c->user_allocs.emplace_back(*out, bytes);
    return HT_OK;
}
extern "C" ht_status ht_device_free(ht_ctx *c, void *p) {
    if (!c) return HT_ERR_INVALID;
    if (!p) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));  // nothing enqueued on this context may still read it
    auto it = std::find_if(c->user_allocs.begin(), c->user_allocs.end(), [p](const std::pair<void *, size_t> &a) { return a.first == p; });
    if (it == c->user_allocs.end()) return ht_fail(c, HT_ERR_INVALID, "ht_device_free: not a live ht_device_alloc buffer of this context");
    const uint8_t *pb = static_cast<const uint8_t *>(p);
    {   // a buffer that other contexts of this device have bound (ht_bind_frames_device: a batch host shares one frame buffer between
        // its pipelined contexts) is NOT freed under them: their next enqueue would read freed HBM.  Rebind or destroy them first.
        std::lock_guard<std::mutex> lk(g_live_mu);
        if (bound_by_live_context(c, c->device, pb, it->second))
            return ht_fail(c, HT_ERR_STATE, "ht_device_free: another live context still has frames bound inside this buffer (rebind or destroy it first)");
    }
    if (c->d_frames && c->d_frames >= pb && c->d_frames < pb + it->second) {  // frames bound inside it
        c->d_frames = nullptr, c->nframes = 0;
        destroy_graphs(c);  // their keys hold the freed pointer: an allocation that reuses the address must not replay them
    }
    c->user_allocs.erase(it);
    HT_HIP(c, hipFree(p));
    sweep_orphans(c);
    return HT_OK;
}
extern "C" ht_status ht_device_upload(ht_ctx *c, void *dst_dev, const void *src_host, size_t bytes) {
    if (!c || !dst_dev || !src_host) return HT_ERR_INVALID;
    if (bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

extern "C" ht_status ht_device_download(ht_ctx *c, void *dst_host, const void *src_dev, size_t bytes) {
    if (!c || !dst_host || !src_dev) return HT_ERR_INVALID;
    if (bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

// ---------------------------------------------------------------------------------------------------------
// detect

// 4 u64 per frame (R, G, B channel sums + pad), two regions of max_batch frames: the batch in flight (fused into its gray pass) and the
// stand-alone ht_whitebalance_batch; plus the pinned staging the in-flight batch's sums are copied to by ht_detect_collect
static ht_status wb_scratch(ht_ctx *c) {
    const size_t region = sizeof(unsigned long long) * 4 * (size_t)std::max(c->max_batch, 1), need = 2 * region;
    if (c->d_scratch_bytes < need) {
        HT_HIP(c, hipStreamSynchronize(c->stream));
        destroy_graphs(c);  // captured detect sequences bake the d_scratch pointer into their gray / whitebalance nodes
        if (c->d_scratch) (void)hipFree(c->d_scratch);
        c->d_scratch = nullptr;
        c->d_scratch_bytes = 0;
        if (hipMalloc(&c->d_scratch, need) != hipSuccess) return ht_fail(c, HT_ERR_NOMEM, "whitebalance scratch: hipMalloc failed");
        c->d_scratch_bytes = need;
    }
    if (c->h_wb_pinned_bytes < region) {
        HT_HIP(c, hipStreamSynchronize(c->stream));
        if (c->h_wb_pinned) (void)hipHostFree(c->h_wb_pinned);
        c->h_wb_pinned = nullptr;
        c->h_wb_pinned_bytes = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_wb_pinned), region, hipHostMallocDefault) != hipSuccess)
            return ht_fail(c, HT_ERR_NOMEM, "whitebalance staging: hipHostMalloc failed");
        c->h_wb_pinned_bytes = region;
    }
    return HT_OK;
}
static unsigned long long *wb_standalone_region(ht_ctx *c) {
    return reinterpret_cast<unsigned long long *>(c->d_scratch) + 4 * (size_t)std::max(c->max_batch, 1);
}

// What a detect batch counts in, zeroed on the stream in front of its kernels: counters, (stage statistics, whitebalance sums).  Always
// enqueued plainly, NEVER captured: a memset node of a captured sequence was replayed with a garbage fill value once other work had gone
// through the process — a context's replay returned nhits = 0x682aa5da for 1517 hits after another context had merely been created, while
// its plain launches counted right (LABLOG 2026-10-20).  The kernels' arguments belong to the graph; the fill pattern of a memset node does not.
static ht_status detect_enqueue_zero(ht_ctx *c, uint32_t flags) {
    HT_HIP(c, hipMemsetAsync(c->d_counters, 0, sizeof(HtCounters), c->stream));
    if (flags & HT_SCAN_STATS) HT_HIP(c, hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * 64 * HT_STAT_SHARDS, c->stream));
    if (flags & HT_DETECT_WHITEBALANCE) HT_HIP(c, hipMemsetAsync(c->d_scratch, 0, sizeof(unsigned long long) * 4 * (size_t)c->nframes, c->stream));
    return HT_OK;
}

// the kernels of one detect batch behind detect_enqueue_zero: gray (with the whitebalance sums), pyramid generations, cascade scan
static ht_status detect_enqueue_body(ht_ctx *c, uint32_t flags) {
    c->early_launched = false;
    ht_status st;
    c->wb_fused = false;
    const bool wb = (flags & HT_DETECT_WHITEBALANCE) != 0;
    if (wb) c->wb_fused = (c->W & 3) == 0;  // the linear gray kernel carries the channel sums (no second read of the frames); odd widths take the separate pass below
    st = ht_launch_pyramid(c, flags);
    c->wb_fused = false;
    if (st != HT_OK) return st;
    if (wb && (c->W & 3) != 0 && (st = ht_launch_whitebalance(c, c->d_scratch, false)) != HT_OK) return st;
    return ht_launch_scan(c, flags);
}

static void destroy_graphs(ht_ctx *c) {
    for (auto &g : c->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    c->graphs.clear();
}

extern "C" uint64_t ht_graph_launches(const ht_ctx *c) { return c ? c->graph_launches : 0; }

extern "C" ht_status ht_detect_enqueue(ht_ctx *c, uint32_t flags) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_detect_enqueue");
    if (!c->d_frames || c->nframes <= 0) return ht_fail(c, HT_ERR_STATE, "ht_detect_enqueue: no frames bound");
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st;
    if ((flags & HT_DETECT_WHITEBALANCE) && (st = wb_scratch(c)) != HT_OK) return st;  // may allocate and synchronise: never inside a capture
    // Small batches are launch-bound (one 1080p frame: ~0.13 ms of kernels inside a ~0.38 ms sequence of ~10 dependent launches):
    // the second enqueue of the same (frames, count, flags) captures the sequence into a hipGraph, later ones replay it.  The first
    // one always runs plainly (it also sets the function attributes a capture must not).
    const bool graph_ok = c->graph_max_frames > 0 && c->nframes <= c->graph_max_frames && c->own_stream && !c->profiling && !c->early_scan &&
                          !(flags & HT_SCAN_STATS);
    if ((st = detect_enqueue_zero(c, flags)) != HT_OK) return st;  // in front of the capture, the replay and the plain launches alike
    bool done = false;
    if (graph_ok) {
        HtDetectGraph *g = nullptr;
        for (auto &e : c->graphs)
            if (e.frames == c->d_frames && e.frame_stride == c->frame_stride && e.nframes == c->nframes && e.flags == flags) g = &e;
        if (!g) {
            if (c->graphs.size() >= 8) {  // a streaming host alternates between two frame buffers; 8 keys are plenty
                HtDetectGraph &old = c->graphs.front();
                if (old.exec) (void)hipGraphExecDestroy(old.exec);
                if (old.graph) (void)hipGraphDestroy(old.graph);
                c->graphs.erase(c->graphs.begin());
            }
            c->graphs.emplace_back();
            g = &c->graphs.back();
            g->frames = c->d_frames, g->frame_stride = c->frame_stride, g->nframes = c->nframes, g->flags = flags;
        }
        if (!g->exec && g->seen == 1) {
            ht_capture_mark(c, true);
            if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                st = detect_enqueue_body(c, flags);
                hipGraph_t graph = nullptr;
                const hipError_t e = hipStreamEndCapture(c->stream, &graph);
                ht_capture_mark(c, false);
                if (st == HT_OK && e == hipSuccess && graph && hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                    g->graph = graph;
                } else {  // not capturable here: keep launching plainly
                    if (graph) (void)hipGraphDestroy(graph);
                    g->exec = nullptr;
                    g->seen = 1 << 30;
                    (void)hipGetLastError();
                }
            } else {
                ht_capture_mark(c, false);
                (void)hipGetLastError();
                g->seen = 1 << 30;
            }
        }
        if (g->exec) {
            HT_HIP(c, hipGraphLaunch(g->exec, c->stream));
            c->graph_launches++;
            c->early_launched = false;
            done = true;
        } else if (g->seen < (1 << 30)) {
            g->seen++;
        }
    }
    if (!done && (st = detect_enqueue_body(c, flags)) != HT_OK) return st;
    c->stats_enqueued = (flags & HT_SCAN_STATS) != 0;
    c->wb_enqueued = (flags & HT_DETECT_WHITEBALANCE) != 0;
    c->enqueued = true;
    c->grp_enqueued = false;      // a device grouping belongs to the batch it was enqueued behind (ht_detect_best_enqueue), not to this one
    c->enq_nframes = c->nframes;  // ht_detect_collect reports THIS batch even if other frames were bound / swapped in meanwhile
    return HT_OK;
}

// What every collect call leaves behind once the stream has been synchronised: the batch counts as collected, the whitebalance sums that
// travelled to h_wb_pinned become the snapshot ht_detect_whitebalance reports (wb_snap), the stage counts are fetched.  Shared with the
// device-grouped collect (ht_group.hip).
ht_status ht_detect_mark_collected(ht_ctx *c, bool wb_snap) {
    c->enqueued = false;
    if (wb_snap) {
        c->h_wb_sums.assign(c->h_wb_pinned, c->h_wb_pinned + 4 * (size_t)c->enq_nframes);
        c->wb_collected_n = c->enq_nframes;
    } else {
        c->wb_collected_n = -1;
    }
    std::memset(c->h_stage_in, 0, sizeof(c->h_stage_in));
    if (c->stats_enqueued) {
        std::vector<unsigned long long> sh((size_t)64 * HT_STAT_SHARDS);
        HT_HIP(c, hipMemcpy(sh.data(), c->d_stats, sh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (int r = 0; r < HT_STAT_SHARDS; r++)
            for (int j = 0; j < 64; j++) c->h_stage_in[j] += sh[(size_t)r * 64 + j];
    }
    return HT_OK;
}

static inline bool hit_less(const ht_hit &a, const ht_hit &b) {  // emission order, ccv.js:154,178,181-182
    if (a.frame != b.frame) return a.frame < b.frame;
    if (a.scale != b.scale) return a.scale < b.scale;
    if (a.q != b.q) return a.q < b.q;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
}

extern "C" ht_status ht_detect_collect(ht_ctx *c, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_detect_collect");
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect: nothing enqueued");
    HT_HIP(c, hipSetDevice(c->device));
    // counters + the first HT_PINNED_HITS hits in one go (pinned host memory), one synchronisation per batch
    // (speculative: as many hits as a batch of this size usually has — 64 per frame, at least 256 —, not the whole staging buffer:
    // a live feed's single frame would otherwise wait for a 196 KB copy it almost never needs; the rare excess is fetched below)
    // ... and, once a batch of this context has been collected, 1.5 x what that one had: a 256-frame C2 batch has ~1.4 k hits, not 16 k)
    uint32_t spec = std::max<uint32_t>(256u, 64u * (uint32_t)std::max(c->enq_nframes, 1));
    if (c->spec_hint) spec = std::min(spec, std::max<uint32_t>(256u, c->spec_hint + c->spec_hint / 2 + 64u));
    spec = std::min<uint32_t>(spec, std::min<uint32_t>(HT_PINNED_HITS, c->hit_capacity));
    HT_HIP(c, hipMemcpyAsync(c->h_pinned, c->d_counters, sizeof(HtCounters) + (size_t)spec * sizeof(ht_hit), hipMemcpyDeviceToHost, c->stream));  // one copy: they are contiguous
    // the whitebalance sums of THIS batch travel with its counters: a re-enqueue below (or any later enqueue) zeroes and refills the
    // device sums, ht_detect_whitebalance reports the snapshot of the batch collected last
    const bool wb_snap = c->wb_enqueued && c->h_wb_pinned;
    if (wb_snap)
        HT_HIP(c, hipMemcpyAsync(c->h_wb_pinned, c->d_scratch, sizeof(unsigned long long) * 4 * (size_t)c->enq_nframes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(&c->h_counters, c->h_pinned, sizeof(HtCounters));
    c->grp_enqueued = false;  // a device grouping enqueued behind this batch (ht_detect_best_enqueue) is dropped with it
    const ht_status cst = ht_detect_mark_collected(c, wb_snap);
    if (cst != HT_OK) return cst;
    const uint32_t found = c->h_counters.nhits;
    c->spec_hint = found;
    if (total) *total = found;
    const uint32_t nfr = (uint32_t)c->enq_nframes;
    if (counts) std::memset(counts, 0, sizeof(uint32_t) * (size_t)nfr);
    if (found > c->hit_capacity)
        return ht_fail(c, HT_ERR_CAPACITY, "ht_detect_collect: more raw hits than ht_config.hit_capacity; results incomplete");
    std::vector<ht_hit> &tmp = c->h_raw_hits;  // context scratch: no allocation, no zero-fill per batch
    tmp.resize(found);
    if (found) {
        const uint32_t have = std::min(found, spec);
        std::memcpy(tmp.data(), c->h_pinned + sizeof(HtCounters), (size_t)have * sizeof(ht_hit));
        if (found > have)
            HT_HIP(c, hipMemcpy(tmp.data() + have, c->d_hits + have, (size_t)(found - have) * sizeof(ht_hit), hipMemcpyDeviceToHost));
    }
    // every raw hit of this batch is in host memory: the next batch of the same frames buffer may start while the host sorts and
    // groups this one (ht_detect_collect_best_requeue) — the GPU never runs one batch short during the host's post-processing
    if (c->requeue_flags >= 0) {
        const uint32_t fl = (uint32_t)c->requeue_flags;
        c->requeue_flags = -1;
        ht_status rq = ht_detect_enqueue(c, fl);
        if (rq != HT_OK) return rq;
    }
    // emission order (frame, scale, q, y, x).  The frame is the major key and a frame has few hits: a counting sort by frame
    // straight into the destination, then each frame's handful ordered by one packed 48-bit key — a 256-frame batch's 1.4 k hits
    // took ~0.1 ms of the host's 0.25 ms per batch in one std::sort with the five-field comparator (profiles/r03_host_post.txt)
    const uint32_t ncopy = std::min(found, cap);
    ht_hit *dst = hits;
    if (found && (!hits || cap < found)) {
        c->h_ordered_hits.resize(found);
        dst = c->h_ordered_hits.data();
    }
    bool bucketed = found > 0 && nfr > 0;
    if (bucketed) {
        // emission order (frame, scale, q, y, x).  The frame is the major key and a frame has few hits: a counting sort by frame straight
        // into the destination, then each frame's handful ordered by one packed 48-bit key (ht_hostpost.h) — a 256-frame batch's 1.4 k
        // hits took ~0.1 ms of the host's 0.25 ms per batch in one std::sort with the five-field comparator (profiles/r03_host_post.txt)
        bucketed = ht_post_bucket_by_frame(tmp.data(), found, nfr, dst, c->h_frame_start, counts);
        if (bucketed) {
            const uint32_t *se = c->h_frame_start.data();
            if (c->collect_best_follows) {
                c->h_sort_deferred = true;  // ht_detect_collect_best orders every frame inside its own per-frame pass
            } else {
                auto sort_frames = [&](int f0, int f1) {
                    for (int f = f0; f < f1; f++) ht_post_sort_frame(dst, f ? se[f - 1] : 0u, se[f]);
                };
                const int nw = ht_host_workers(c, (int)nfr, found);
                if (nw > 0) HtPool::get().run((int)nfr, 16, nw, sort_frames);
                else sort_frames(0, (int)nfr);
            }
        }
    }
    if (found && !bucketed) {
        std::sort(tmp.begin(), tmp.end(), hit_less);
        if (counts) {
            std::memset(counts, 0, sizeof(uint32_t) * (size_t)nfr);
            for (uint32_t i = 0; i < found; i++)
                if (tmp[i].frame < nfr) counts[tmp[i].frame]++;
        }
        std::memcpy(dst, tmp.data(), (size_t)found * sizeof(ht_hit));
    }
    if (found && dst != hits && hits && ncopy) std::memcpy(hits, dst, (size_t)ncopy * sizeof(ht_hit));
    if (found > cap) return ht_fail(c, HT_ERR_CAPACITY, "ht_detect_collect: caller buffer too small for all hits");
    return HT_OK;
}

extern "C" ht_status ht_detect_batch(ht_ctx *c, const uint8_t *host_rgba, int32_t n, int32_t width, int32_t height, size_t frame_stride,
                                     uint32_t flags, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total) {
    if (!c) return HT_ERR_INVALID;
    ht_status st;
    if (c->W != width || c->H != height || c->max_batch < n)
        if ((st = ht_set_geometry(c, width, height, n, nullptr, 0)) != HT_OK) return st;
    if ((st = ht_upload_frames(c, host_rgba, n, frame_stride)) != HT_OK) return st;
    if ((st = ht_detect_enqueue(c, flags)) != HT_OK) return st;
    return ht_detect_collect(c, hits, cap, counts, total);
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

// per-frame channel sums -> getWhitebalance values (whitebalance.js:14-26)
static void wb_values(const ht_ctx *c, const unsigned long long *sums, double *out, int32_t n) {
    const double imagesize = (double)c->W * (double)c->H;  // whitebalance.js:14
    for (int i = 0; i < n; i++) {
        // r, g, b are sums of integers < 2^53: exactly what the reference's double accumulation holds (whitebalance.js:17-21)
        const double avgr = (double)sums[4 * i] / imagesize, avgg = (double)sums[4 * i + 1] / imagesize, avgb = (double)sums[4 * i + 2] / imagesize;
        out[i] = (avgr + avgg + avgb) / 3;  // whitebalance.js:23-26
    }
}

extern "C" ht_status ht_whitebalance_batch(ht_ctx *c, double *out, int32_t n) {
    if (!c || !out) return HT_ERR_INVALID;
    if (!c->d_frames || n <= 0 || n > c->nframes) return ht_fail(c, HT_ERR_STATE, "ht_whitebalance_batch: no frames bound");
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st = wb_scratch(c);
    if (st != HT_OK) return st;
    unsigned long long *d_sums = wb_standalone_region(c);  // never the region a batch in flight accumulates into
    if ((st = ht_launch_whitebalance(c, reinterpret_cast<double *>(d_sums), true)) != HT_OK) return st;
    std::vector<unsigned long long> sums((size_t)n * 4);
    HT_HIP(c, hipMemcpyAsync(sums.data(), d_sums, sizeof(unsigned long long) * 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    wb_values(c, sums.data(), out, n);
    return HT_OK;
}

extern "C" ht_status ht_detect_whitebalance(ht_ctx *c, double *out, int32_t n) {
    if (!c || !out) return HT_ERR_INVALID;
    if (c->wb_collected_n < 0)
        return ht_fail(c, HT_ERR_STATE, "ht_detect_whitebalance: the batch collected last was not enqueued with HT_DETECT_WHITEBALANCE (call after ht_detect_collect)");
    if (n <= 0 || n > c->wb_collected_n) return ht_fail(c, HT_ERR_INVALID, "ht_detect_whitebalance: n exceeds the collected batch");
    wb_values(c, c->h_wb_sums.data(), out, n);  // host snapshot: no device work, no wait for a batch that was re-enqueued meanwhile
    return HT_OK;
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

extern "C" ht_status ht_detect_collect_best(ht_ctx *c, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits) {
    if (!c || !best) return HT_ERR_INVALID;
    HtRange range("ht_detect_collect_best");
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect_best: nothing enqueued");
    const int nfr = c->enq_nframes;
    // the context's own buffers: nothing but the per-frame rects crosses the ABI (a batch server calls this once per batch)
    if (c->h_collect_hits.size() < (size_t)c->hit_capacity) c->h_collect_hits.resize(c->hit_capacity);
    c->h_collect_counts.resize((size_t)std::max(nfr, 1));
    uint32_t total = 0;
    c->collect_best_follows = true;  // the hits arrive bucketed by frame; each frame's ordering happens in the per-frame pass below
    c->h_sort_deferred = false;
    ht_status st = ht_detect_collect(c, c->h_collect_hits.data(), c->hit_capacity, c->h_collect_counts.data(), &total);
    c->collect_best_follows = false;
    if (total_hits) *total_hits = total;
    if (st != HT_OK) return st;
    if (!c->h_sort_deferred) return ht_best_faces(c, c->h_collect_hits.data(), c->h_collect_counts.data(), nfr, min_neighbors, best);
    // One pass per frame — order its hits (emission order: scale, q, y, x), seq rects, grouping, best face — dealt out to the host pool
    // (ht_hostpost.h): frames are independent and write their own slots, byte-identical to the single-threaded order
    // (tests/test_host_post.py runs the same code under ASan with 0 and 7 workers).  A C2 batch took 0.144 ms of one core here, more
    // than half of the 0.25 ms the GPU needs for it (profiles/r03_host_post.txt).
    return ht_post_frames(post_cfg(c), c->h_collect_hits.data(), c->h_frame_start.data(), nfr, min_neighbors, ht_host_workers(c, nfr, total), best);
}

extern "C" ht_status ht_detect_collect_best_requeue(ht_ctx *c, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits, uint32_t next_flags) {
    if (!c || !best) return HT_ERR_INVALID;
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect_best_requeue: nothing enqueued");
    c->requeue_flags = (int64_t)next_flags;
    const ht_status st = ht_detect_collect_best(c, min_neighbors, best, total_hits);
    c->requeue_flags = -1;
    return st;
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

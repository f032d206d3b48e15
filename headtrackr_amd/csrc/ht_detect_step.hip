// ht_detect_step.hip — one detect batch on the host side: what it counts in, its launch sequence and the cache of captured sequences,
// the collect calls and the whitebalance values that travel with a batch.  Included by ht_context.hip (no device code).
//
// Reference behaviour restated here:
//   emission order      ccv.js:154,178,181-182
//   whitebalance        whitebalance.js:14-26

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

// 4 u64 per frame (R, G, B channel sums + pad), two regions of max_batch frames: the batch in flight (fused into its gray pass) and the
// stand-alone ht_whitebalance_batch; plus the pinned staging the in-flight batch's sums are copied to by ht_detect_fetch
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

// ---------------------------------------------------------------------------------------------------------
// The cache of captured sequences (HtDetectGraph, ht_internal.h).  Small batches are launch-bound (one 1080p frame: ~0.13 ms of kernels
// inside a ~0.38 ms sequence of ~10 dependent launches): the second enqueue of the same (frames, stride, count, flags) captures the
// sequence into a hipGraph, later ones replay it.  The first one always runs plainly (it also sets the function attributes a capture
// must not).  `seen` counts a key's plain enqueues; 1 << 30 says "not capturable here: keep launching plainly".

static void graph_drop(HtDetectGraph &g) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    if (g.graph) (void)hipGraphDestroy(g.graph);
}

static void destroy_graphs(ht_ctx *c) {
    for (auto &g : c->graphs) graph_drop(g);
    c->graphs.clear();
}

// the entry of the bound frames and these flags; a new key takes the place of the oldest once there are 8
static HtDetectGraph *graph_find_or_add(ht_ctx *c, uint32_t flags) {
    for (auto &e : c->graphs)
        if (e.frames == c->d_frames && e.frame_stride == c->frame_stride && e.nframes == c->nframes && e.flags == flags) return &e;
    if (c->graphs.size() >= 8) {  // a streaming host alternates between two frame buffers; 8 keys are plenty
        graph_drop(c->graphs.front());
        c->graphs.erase(c->graphs.begin());
    }
    c->graphs.emplace_back();
    HtDetectGraph *g = &c->graphs.back();
    g->frames = c->d_frames, g->frame_stride = c->frame_stride, g->nframes = c->nframes, g->flags = flags;
    return g;
}

// captures the batch's kernels into g->exec; where that is not possible g stays without one and is never tried again
static void graph_capture(ht_ctx *c, HtDetectGraph *g, uint32_t flags) {
    ht_capture_mark(c, true);
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        ht_capture_mark(c, false);
        (void)hipGetLastError();
        g->seen = 1 << 30;
        return;
    }
    const ht_status st = detect_enqueue_body(c, flags);
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
}

extern "C" uint64_t ht_graph_launches(const ht_ctx *c) { return c ? c->graph_launches : 0; }

extern "C" ht_status ht_detect_enqueue(ht_ctx *c, uint32_t flags) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_detect_enqueue");
    if (!c->d_frames || c->nframes <= 0) return ht_fail(c, HT_ERR_STATE, "ht_detect_enqueue: no frames bound");
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st;
    if ((flags & HT_DETECT_WHITEBALANCE) && (st = wb_scratch(c)) != HT_OK) return st;  // may allocate and synchronise: never inside a capture
    const bool graph_ok = c->graph_max_frames > 0 && c->nframes <= c->graph_max_frames && c->own_stream && !c->profiling && !c->early_scan &&
                          !(flags & HT_SCAN_STATS);
    if ((st = detect_enqueue_zero(c, flags)) != HT_OK) return st;  // in front of the capture, the replay and the plain launches alike
    bool done = false;
    if (graph_ok) {
        HtDetectGraph *g = graph_find_or_add(c, flags);
        if (!g->exec && g->seen == 1) graph_capture(c, g, flags);
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
// travelled to h_wb_pinned become the snapshot ht_detect_whitebalance reports (wb_snap), the stage counts are fetched.
static ht_status ht_detect_mark_collected(ht_ctx *c, bool wb_snap) {
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

// The head of every collect call, the device-grouped one (ht_group.hip) included: `bytes` of the batch's results from the device into
// pinned memory, one synchronisation per batch, ht_detect_mark_collected.  The whitebalance sums of THIS batch travel with them: a
// re-enqueue (or any later enqueue) zeroes and refills the device sums, ht_detect_whitebalance reports the snapshot of the batch
// collected last.
ht_status ht_detect_fetch(ht_ctx *c, void *pinned_dst, const void *dev_src, size_t bytes) {
    HT_HIP(c, hipMemcpyAsync(pinned_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
    const bool wb_snap = c->wb_enqueued && c->h_wb_pinned;
    if (wb_snap)
        HT_HIP(c, hipMemcpyAsync(c->h_wb_pinned, c->d_scratch, sizeof(unsigned long long) * 4 * (size_t)c->enq_nframes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return ht_detect_mark_collected(c, wb_snap);
}

static inline bool hit_less(const ht_hit &a, const ht_hit &b) {  // emission order, ccv.js:154,178,181-182
    if (a.frame != b.frame) return a.frame < b.frame;
    if (a.scale != b.scale) return a.scale < b.scale;
    if (a.q != b.q) return a.q < b.q;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
}

// The collect calls' one body.  next_flags >= 0: the next batch of the bound frames is enqueued with these flags as soon as every raw
// hit is on the host.  sort_deferred != nullptr: the caller orders each frame's hits itself (ht_post_frames); *sort_deferred says whether
// they were left bucketed by frame (c->h_frame_start) and unordered inside a frame, or arrive in full emission order after all.
static ht_status detect_collect(ht_ctx *c, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total, int64_t next_flags, bool *sort_deferred) {
    HtRange range("ht_detect_collect");
    if (sort_deferred) *sort_deferred = false;
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect: nothing enqueued");
    HT_HIP(c, hipSetDevice(c->device));
    // counters + the first HT_PINNED_HITS hits in one go (pinned host memory: they are contiguous on the device)
    // (speculative: as many hits as a batch of this size usually has — 64 per frame, at least 256 —, not the whole staging buffer:
    // a live feed's single frame would otherwise wait for a 196 KB copy it almost never needs; the rare excess is fetched below)
    // ... and, once a batch of this context has been collected, 1.5 x what that one had: a 256-frame C2 batch has ~1.4 k hits, not 16 k)
    uint32_t spec = std::max<uint32_t>(256u, 64u * (uint32_t)std::max(c->enq_nframes, 1));
    if (c->spec_hint) spec = std::min(spec, std::max<uint32_t>(256u, c->spec_hint + c->spec_hint / 2 + 64u));
    spec = std::min<uint32_t>(spec, std::min<uint32_t>(HT_PINNED_HITS, c->hit_capacity));
    const ht_status fst = ht_detect_fetch(c, c->h_pinned, c->d_counters, sizeof(HtCounters) + (size_t)spec * sizeof(ht_hit));
    if (fst != HT_OK) return fst;
    std::memcpy(&c->h_counters, c->h_pinned, sizeof(HtCounters));
    c->grp_enqueued = false;  // a device grouping enqueued behind this batch (ht_detect_best_enqueue) is dropped with it
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
    if (next_flags >= 0) {
        const ht_status rq = ht_detect_enqueue(c, (uint32_t)next_flags);
        if (rq != HT_OK) return rq;
    }
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
            if (sort_deferred) {
                *sort_deferred = true;
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

extern "C" ht_status ht_detect_collect(ht_ctx *c, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total) {
    if (!c) return HT_ERR_INVALID;
    return detect_collect(c, hits, cap, counts, total, -1, nullptr);
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

// the batch in flight collected into the context's own buffers and reduced to one rect per frame (next_flags: as in detect_collect)
static ht_status detect_collect_best(ht_ctx *c, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits, int64_t next_flags) {
    HtRange range("ht_detect_collect_best");
    const int nfr = c->enq_nframes;
    // the context's own buffers: nothing but the per-frame rects crosses the ABI (a batch server calls this once per batch)
    if (c->h_collect_hits.size() < (size_t)c->hit_capacity) c->h_collect_hits.resize(c->hit_capacity);
    c->h_collect_counts.resize((size_t)std::max(nfr, 1));
    uint32_t total = 0;
    bool deferred = false;  // the hits arrive bucketed by frame; each frame's ordering happens in the per-frame pass below
    const ht_status st = detect_collect(c, c->h_collect_hits.data(), c->hit_capacity, c->h_collect_counts.data(), &total, next_flags, &deferred);
    if (total_hits) *total_hits = total;
    if (st != HT_OK) return st;
    if (!deferred) return ht_best_faces(c, c->h_collect_hits.data(), c->h_collect_counts.data(), nfr, min_neighbors, best);
    // One pass per frame — order its hits (emission order: scale, q, y, x), seq rects, grouping, best face — dealt out to the host pool
    // (ht_hostpost.h): frames are independent and write their own slots, byte-identical to the single-threaded order
    // (tests/test_host_post.py runs the same code under ASan with 0 and 7 workers).  A C2 batch took 0.144 ms of one core here, more
    // than half of the 0.25 ms the GPU needs for it (profiles/r03_host_post.txt).
    return ht_post_frames(post_cfg(c), c->h_collect_hits.data(), c->h_frame_start.data(), nfr, min_neighbors, ht_host_workers(c, nfr, total), best);
}

extern "C" ht_status ht_detect_collect_best(ht_ctx *c, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits) {
    if (!c || !best) return HT_ERR_INVALID;
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect_best: nothing enqueued");
    return detect_collect_best(c, min_neighbors, best, total_hits, -1);
}

extern "C" ht_status ht_detect_collect_best_requeue(ht_ctx *c, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits, uint32_t next_flags) {
    if (!c || !best) return HT_ERR_INVALID;
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_collect_best_requeue: nothing enqueued");
    return detect_collect_best(c, min_neighbors, best, total_hits, (int64_t)next_flags);
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

// ht_cs_pairs.hip — camshift on an arbitrary list of (stream, frame) pairs (ht_camshift_init_pairs / ht_camshift_track_pairs).
//
// ht_camshift_track_batch pairs stream first + i with bound frame i.  Here any reserved stream meets any bound frame, and a frame may
// serve several streams: every face of one canvas gets a tracker of its own (the reference creates one camshift.Tracker per face), and a
// host whose feeds are in different states (main.js:229-244: one re-detects, the others track) tracks exactly the feeds that track.
// The full-frame histogram (camshift.js:268) depends on the frame alone, so it is computed once per DISTINCT frame of the call:
//
//   k_csp_hist       grid (chunks, distinct frames): k_cs_hist's pass over the frames a device list names
//   k_csp_meanshift  one CS_NT-thread workgroup per pair: k_cs_meanshift with three look-ups (state, pixels, histogram slot)
//   k_csp_init       one workgroup per pair: k_cs_init with the same look-ups
//
// Everything below the look-ups is ht_cs_device.h, i.e. the code k_cs_meanshift runs: same wavefront count, same summation order, same
// bits as the few-stream schedule of ht_camshift_track_batch (options cs_fused_min=large, cs_cluster=0).
//
// Compiled as part of ht_backproject.hip (included at its end, like ht_ingest.hip): the library keeps ONE code object besides the three
// that profiles/traffic.json fingerprints.  No kernel name here carries one of the fingerprint's markers.
#include <cstring>
#include <vector>

namespace {

#include "ht_cs_device.h"  // after ht_backproject.hip's cs_bin

constexpr int CSP_INIT_NT = 1024;  // k_cs_init's workgroup

struct CspEntry {
    int32_t stream, frame;  // the pair
    int32_t slot;           // index of `frame` among the call's distinct frames = its chunk histograms in the scratch
    int32_t pad;
    ht_cs_rect rect;        // k_csp_init only
};
static_assert(sizeof(CspEntry) == 32, "CspEntry");

// k_cs_hist over the frames frame_list[0 .. gridDim.y) names: four 16-byte loads per thread in flight, counts merged per thread and per
// wavefront before they reach LDS, the chunk's histogram written whole into hist[blockIdx.y][blockIdx.x][4096]
__global__ __launch_bounds__(HIST_NT) void k_csp_hist(const uint8_t *__restrict__ frames, size_t frame_stride, uint32_t npix, uint32_t chunk_px,
                                                      const int32_t *__restrict__ frame_list, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[4096];
    for (int i = threadIdx.x; i < 4096; i += HIST_NT) h[i] = 0;
    __syncthreads();
    const uint8_t *frame = frames + (size_t)frame_list[blockIdx.y] * frame_stride;
    const uint32_t beg = blockIdx.x * chunk_px, end = min(beg + chunk_px, npix);  // chunk_px is a multiple of 4 * HIST_NT; beg < npix
    const uint32_t nquad = (end - beg) / 4;
    const uint4 *img4 = reinterpret_cast<const uint4 *>(frame + (size_t)beg * 4);
    const uint32_t iters = chunk_px / (4 * HIST_NT);
    for (uint32_t it0 = 0; it0 < iters; it0 += HIST_UNROLL) {
        uint4 pv[HIST_UNROLL];
        bool onv[HIST_UNROLL];
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            const uint32_t i = (it0 + (uint32_t)u) * HIST_NT + threadIdx.x;
            onv[u] = it0 + (uint32_t)u < iters && i < nquad;
            pv[u] = make_uint4(0u, 0u, 0u, 0u);
            if (onv[u]) pv[u] = img4[i];
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            CS_BATCH_LOADED(pv[u].x);
            CS_BATCH_LOADED(pv[u].y);
            CS_BATCH_LOADED(pv[u].z);
            CS_BATCH_LOADED(pv[u].w);
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            if (it0 + (uint32_t)u >= iters) break;  // workgroup-uniform
            const uint4 p = pv[u];
            const bool on = onv[u];
            const uint32_t b0 = cs_bin(p.x), b1 = cs_bin(p.y), b2 = cs_bin(p.z), b3 = cs_bin(p.w);
            const bool flat = (b0 == b1) && (b2 == b3) && (b0 == b2);
            hist_add_wave(h, b0, flat ? 4u : 1u, on);
            if (on && !flat) {
                atomicAdd(&h[b1], 1u);
                atomicAdd(&h[b2], 1u);
                atomicAdd(&h[b3], 1u);
            }
        }
    }
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frame);
    for (uint32_t i = beg + nquad * 4 + threadIdx.x; i < end; i += HIST_NT) atomicAdd(&h[cs_bin(img[i])], 1u);  // < 4 pixels
    __syncthreads();
    uint32_t *out = hist + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
    for (int i = threadIdx.x; i < 4096; i += HIST_NT) out[i] = h[i];
}

// track() of pair blockIdx.x: the state is states[pair.stream], the pixels are frame pair.frame, the frame's histogram is the sum of the
// chunk histograms of slot pair.slot; the track object goes to out[blockIdx.x] (pair order)
__global__ __launch_bounds__(CS_NT) void k_csp_meanshift(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H,
                                                         const uint32_t *__restrict__ hist, int nchunks, HtCsState *__restrict__ states,
                                                         const CspEntry *__restrict__ entries, int calc_angles, int max_it, int region_cap,
                                                         ht_cs_trackobj *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cs_dyn[];  // [region_cap] u16 bins of the cached search region
    __shared__ double lut[4096];
    __shared__ double red[6][CS_NT / 64];
    __shared__ int s_sw[4];
    const int s = blockIdx.x;
    const int e_stream = entries[s].stream, e_frame = entries[s].frame, e_slot = entries[s].slot;
    HtCsState &st = states[e_stream];
    const uint32_t *cur = hist + (size_t)e_slot * nchunks * 4096;
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)e_frame * frame_stride);
    {  // getWeights, camshift.js:314-330; the frame's histogram = sum of its chunk histograms (4 bins per 16-byte load)
        const uint4 *cur4 = reinterpret_cast<const uint4 *>(cur);
        const uint4 *model4 = reinterpret_cast<const uint4 *>(st.model);
        for (int i4 = threadIdx.x; i4 < 1024; i4 += CS_NT) {
            uint4 acc = make_uint4(0u, 0u, 0u, 0u);
            for (int k = 0; k < nchunks; k++) {
                const uint4 v = cur4[(size_t)k * 1024 + i4];
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
            const uint4 m = model4[i4];
            const uint32_t chv[4] = {acc.x, acc.y, acc.z, acc.w}, mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double p = 0.0;
                if (chv[q] != 0) {
                    p = (double)mv[q] / (double)chv[q];
                    p = p < 1.0 ? p : 1.0;
                }
                lut[i4 * 4 + q] = p;
            }
        }
    }
    if (threadIdx.x < 4) s_sw[threadIdx.x] = st.sw[threadIdx.x];
    __syncthreads();
    const CsRegion R = cs_cache_region<CS_NT>(img, W, H, s_sw, reinterpret_cast<uint16_t *>(cs_dyn), region_cap);
    __syncthreads();
    meanshift_body(W, H, s_sw, st, calc_angles, max_it, out ? out + s : nullptr, nullptr, true,
                   [&](int x, int y, int w, int h) { return window_moments_any<true, CS_NT / 64>(img, W, lut, R, x, y, w, h, red); });
}

// initTracker of pair blockIdx.x (k_cs_init: rows of the rect by wavefront, columns by lane, 8 independent loads per lane in flight)
__global__ __launch_bounds__(CSP_INIT_NT) void k_csp_init(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H,
                                                          const CspEntry *__restrict__ entries, HtCsState *__restrict__ states) {
    __shared__ uint32_t h[4096];
    const int s = blockIdx.x;
    for (int i = threadIdx.x; i < 4096; i += CSP_INIT_NT) h[i] = 0;
    __syncthreads();
    const ht_cs_rect r = entries[s].rect;
    const int e_stream = entries[s].stream, e_frame = entries[s].frame;
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)e_frame * frame_stride);
    const int rw = max(r.width, 0), rh = max(r.height, 0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NWV = CSP_INIT_NT / 64;
    for (int j0 = wave; j0 - wave < rh; j0 += 8 * NWV) {  // same trip count for every wavefront's lanes (ballots inside)
        for (int cb = 0; cb < rw; cb += 64) {
            const int c = cb + lane;
            uint32_t px[8];
            bool in[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int y = r.y + j0 + u * NWV, x = r.x + c;
                in[u] = c < rw && j0 + u * NWV < rh;                               // inside the rect
                const bool img_ok = in[u] && x >= 0 && x < W && y >= 0 && y < H;  // inside the canvas
                px[u] = img_ok ? img[(size_t)y * W + x] : 0u;  // getImageData outside the canvas: transparent black -> bin 0 (camshift.js:206)
            }
#pragma unroll
            for (int u = 0; u < 8; u++) CS_BATCH_LOADED(px[u]);
#pragma unroll
            for (int u = 0; u < 8; u++) hist_add_wave(h, cs_bin(px[u]), 1u, in[u]);
        }
    }
    __syncthreads();
    HtCsState &st = states[e_stream];
    for (int i = threadIdx.x; i < 4096; i += CSP_INIT_NT) st.model[i] = h[i];
    if (threadIdx.x == 0) {
        st.sw[0] = r.x, st.sw[1] = r.y, st.sw[2] = r.width, st.sw[3] = r.height;  // camshift.js:209
        st.x = st.y = st.width = st.height = st.angle = 0.0;                         // camshift.js:210
        st.win_px = st.calls = 0;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

struct CspPlan {
    std::vector<CspEntry> entries;
    std::vector<int32_t> frames;  // the distinct frames, in order of first appearance
    bool identity = false;        // pairs[i] == (first + i, i): the layout of ht_camshift_track_batch
    int32_t first = 0;
};

// every argument check of both entry points, before anything is enqueued or any state changes
ht_status csp_plan(ht_ctx *c, const char *fn, const ht_cs_pair *pairs, int32_t n, const ht_cs_rect *rects, CspPlan *plan) {
    if (n <= 0 || n > c->cs_streams) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": n must be 1 .. the number of reserved streams");
    if (!c->d_frames || c->nframes <= 0) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": bind frames first");
    std::vector<int32_t> slot_of((size_t)c->nframes, -1);
    std::vector<uint8_t> seen((size_t)c->cs_streams, 0);
    plan->entries.resize((size_t)n);
    plan->identity = true, plan->first = pairs[0].stream;
    for (int32_t i = 0; i < n; i++) {
        const int32_t s = pairs[i].stream, f = pairs[i].frame;
        if (s < 0 || s >= c->cs_streams) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": stream " + std::to_string(s) + " is not reserved");
        if (f < 0 || f >= c->nframes) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": frame " + std::to_string(f) + " is not bound");
        if (seen[(size_t)s]) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": stream " + std::to_string(s) + " appears twice");
        seen[(size_t)s] = 1;
        if (slot_of[(size_t)f] < 0) {
            slot_of[(size_t)f] = (int32_t)plan->frames.size();
            plan->frames.push_back(f);
        }
        if (s != plan->first + i || f != i) plan->identity = false;
        CspEntry &e = plan->entries[(size_t)i];
        e.stream = s, e.frame = f, e.slot = slot_of[(size_t)f], e.pad = 0;
        e.rect = rects ? rects[i] : ht_cs_rect{0, 0, 0, 0};
    }
    return HT_OK;
}

// the call's table -> device (entries, then the distinct frames): staged in a pinned buffer, copied on the context's stream in front of
// the kernels that read it.  HT_CSP_STAGE staging buffers take turns, so a call practically never waits for an earlier call's copy.
ht_status csp_upload(ht_ctx *c, const char *fn, const CspPlan &plan, const CspEntry **d_entries, const int32_t **d_frames) {
    const size_t n = plan.entries.size(), words = n * (sizeof(CspEntry) / 4) + plan.frames.size();
    if (c->csp_tab_cap < words || c->h_csp_tab_cap < words) {
        HT_HIP(c, hipStreamSynchronize(c->stream));
        const size_t cap = std::max(words, (size_t)c->cs_streams * (sizeof(CspEntry) / 4 + 1));
        if (c->d_csp_tab) (void)hipFree(c->d_csp_tab);
        c->d_csp_tab = nullptr, c->csp_tab_cap = 0;
        for (auto &h : c->h_csp_tab) {
            if (h) (void)hipHostFree(h);
            h = nullptr;
        }
        c->h_csp_tab_cap = 0;
        bool ok = hipMalloc(reinterpret_cast<void **>(&c->d_csp_tab), cap * 4) == hipSuccess;
        for (int k = 0; ok && k < ht_ctx::HT_CSP_STAGE; k++) {
            ok = hipHostMalloc(reinterpret_cast<void **>(&c->h_csp_tab[k]), cap * 4, hipHostMallocDefault) == hipSuccess;
            if (ok && !c->ev_csp_tab[k]) ok = hipEventCreateWithFlags(&c->ev_csp_tab[k], hipEventDisableTiming) == hipSuccess;
        }
        if (!ok) {
            (void)hipGetLastError();
            return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": allocation of the pair table failed");
        }
        c->csp_tab_cap = c->h_csp_tab_cap = cap;
    }
    const int k = c->csp_stage_next;
    c->csp_stage_next = (k + 1) % ht_ctx::HT_CSP_STAGE;
    HT_HIP(c, hipEventSynchronize(c->ev_csp_tab[k]));  // never recorded: returns at once
    std::memcpy(c->h_csp_tab[k], plan.entries.data(), n * sizeof(CspEntry));
    std::memcpy(c->h_csp_tab[k] + n * (sizeof(CspEntry) / 4), plan.frames.data(), plan.frames.size() * 4);
    HT_HIP(c, hipMemcpyAsync(c->d_csp_tab, c->h_csp_tab[k], words * 4, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_csp_tab[k], c->stream));
    *d_entries = reinterpret_cast<const CspEntry *>(c->d_csp_tab);
    *d_frames = c->d_csp_tab + n * (sizeof(CspEntry) / 4);
    return HT_OK;
}

// one track() of every pair: table, histograms of the distinct frames, one mean-shift workgroup per pair; results to d_out[0 .. n)
ht_status csp_launch_track(ht_ctx *c, const CspPlan &plan, int32_t calc_angles, ht_cs_trackobj *d_out) {
    const char *fn = "ht_camshift_track_pairs";
    const int n = (int)plan.entries.size(), nd = (int)plan.frames.size();
    const uint32_t npix = (uint32_t)((size_t)c->W * c->H);
    if (!c->csp_attr_set) {  // the cached search region needs more than the default 64 KB of LDS per workgroup
        HT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_csp_meanshift), hipFuncAttributeMaxDynamicSharedMemorySize, CS_REGION_CAP * 2));
        c->csp_attr_set = true;
    }
    uint32_t chunk_px = 0, nchunks = 0;
    ht_cs_hist_plan(npix, nd, &chunk_px, &nchunks);
    const size_t need = (size_t)nd * nchunks * 4096;
    if (c->csp_hist_cap < need) {
        HT_HIP(c, hipStreamSynchronize(c->stream));
        if (c->d_csp_hist) (void)hipFree(c->d_csp_hist);
        c->d_csp_hist = nullptr, c->csp_hist_cap = 0;
        if (c->cs_last_hist && c->cs_last_hist != c->d_cs_hist) c->cs_last_hist = nullptr, c->cs_last_n = 0;  // pointed into the old scratch
        if (hipMalloc(reinterpret_cast<void **>(&c->d_csp_hist), need * sizeof(uint32_t)) != hipSuccess) {
            (void)hipGetLastError();
            return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": hipMalloc failed (chunk histograms)");
        }
        c->csp_hist_cap = need;
    }
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr;
    ht_status st = csp_upload(c, fn, plan, &d_entries, &d_flist);
    if (st != HT_OK) return st;
    {
        HtProfScope ps(c, "csp_hist");
        hipLaunchKernelGGL(k_csp_hist, dim3(nchunks, nd), dim3(HIST_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px, d_flist, c->d_csp_hist);
        HT_HIP(c, hipGetLastError());
    }
    {
        HtProfScope ps(c, "csp_meanshift");
        hipLaunchKernelGGL(k_csp_meanshift, dim3(n), dim3(CS_NT), (size_t)CS_REGION_CAP * 2, c->stream, c->d_frames, c->frame_stride, c->W, c->H, c->d_csp_hist,
                           (int)nchunks, c->d_cs, d_entries, calc_angles, c->dbg_cs_iters, c->cs_region_cap, d_out);
        HT_HIP(c, hipGetLastError());
    }
    // what ht_camshift_debug_hist(current) reads: the slot of every paired stream's frame (the map stays on the host)
    c->cs_pair_slot.assign((size_t)c->cs_streams, -1);
    for (const CspEntry &e : plan.entries) c->cs_pair_slot[(size_t)e.stream] = e.slot;
    c->cs_pair_chunks = (int)nchunks;
    c->cs_last_hist = c->d_csp_hist, c->cs_last_first = 0, c->cs_last_n = 0, c->cs_last_chunks = 0;
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_init_pairs(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_cs_rect *rects) {
    HtRange range("ht_camshift_init_pairs");
    if (!c || !pairs || !rects) return HT_ERR_INVALID;
    CspPlan plan;
    ht_status st = csp_plan(c, "ht_camshift_init_pairs", pairs, n, rects, &plan);
    if (st != HT_OK) return st;
    if (plan.identity && !c->cs_pairs_force) return ht_camshift_init_batch(c, plan.first, n, rects);
    HT_HIP(c, hipSetDevice(c->device));
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr;
    st = csp_upload(c, "ht_camshift_init_pairs", plan, &d_entries, &d_flist);
    if (st != HT_OK) return st;
    HtProfScope ps(c, "csp_init");
    hipLaunchKernelGGL(k_csp_init, dim3(n), dim3(CSP_INIT_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_entries, c->d_cs);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

extern "C" ht_status ht_camshift_track_pairs(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, int32_t calc_angles, ht_cs_trackobj *out) {
    HtRange range("ht_camshift_track_pairs");
    if (!c || !pairs) return HT_ERR_INVALID;
    CspPlan plan;
    ht_status st = csp_plan(c, "ht_camshift_track_pairs", pairs, n, nullptr, &plan);
    if (st != HT_OK) return st;
    if (plan.identity && !c->cs_pairs_force) return ht_camshift_track_batch(c, plan.first, n, calc_angles, out);  // all three schedules, unchanged
    if (c->W == 0 || c->H == 0) return HT_OK;  // camshift.js:219
    HT_HIP(c, hipSetDevice(c->device));
    // like ht_camshift_track_batch: a synchronous call with nothing outstanding takes the enqueue-only route and collects at once
    const bool via_ring = out && c->cs_sync_ring && c->cs_ring_count == 0 && n <= c->cs_ring_streams;
    if (!out || via_ring) {
        if (n > c->cs_ring_streams) return ht_fail(c, HT_ERR_STATE, "ht_camshift_track_pairs: no result ring for this many streams (ht_camshift_reserve failed to allocate it)");
        if (c->cs_ring_count == ht_ctx::HT_CS_RING)
            return ht_fail(c, HT_ERR_STATE, "ht_camshift_track_pairs: too many enqueue-only calls outstanding (collect with ht_camshift_track_collect)");
        ht_ctx::HtCsSlot &sl = c->cs_ring[(c->cs_ring_head + c->cs_ring_count) % ht_ctx::HT_CS_RING];
        st = csp_launch_track(c, plan, calc_angles, sl.h_out);
        if (st != HT_OK) return st;
        sl.seq = 0u;  // completed by the event
        HT_HIP(c, hipEventRecord(sl.ev, c->stream));
        sl.n = n;
        c->cs_ring_count++;
        return via_ring ? ht_camshift_track_collect(c, n, out) : HT_OK;
    }
    st = csp_launch_track(c, plan, calc_angles, c->d_cs_out);
    if (st != HT_OK) return st;
    HT_HIP(c, hipMemcpyAsync(out, c->d_cs_out, sizeof(ht_cs_trackobj) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

void ht_cs_pairs_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_csp_tab) (void)hipFree(c->d_csp_tab);
    if (c->d_csp_hist) (void)hipFree(c->d_csp_hist);
    for (auto &h : c->h_csp_tab)
        if (h) (void)hipHostFree(h);
    for (auto &e : c->ev_csp_tab)
        if (e) (void)hipEventDestroy(e);
    c->d_csp_tab = nullptr, c->d_csp_hist = nullptr, c->csp_tab_cap = c->h_csp_tab_cap = c->csp_hist_cap = 0;
    for (auto &h : c->h_csp_tab) h = nullptr;
    for (auto &e : c->ev_csp_tab) e = nullptr;
}

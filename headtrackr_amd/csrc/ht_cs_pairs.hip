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
// and, under option cs_pairs_cluster=1, for a few pairs on large frames (ht_cs_plan_track_pairs / ht_cs_plan_init_pairs decide):
//
//   k_csp_lut                grid (64, pairs): k_cs_lut — the pair's weight LUT from its frame's chunk histograms, its exchange slots marked
//   k_csp_meanshift_cluster  G workgroups per pair: k_cs_meanshift_cluster, behind the cluster gate (ht_cs_cluster_gate_begin / _end)
//   k_csp_zero_models        one workgroup per pair zeroes the pair's model (the paired streams are not contiguous: no 2-D memset), for
//   k_csp_init_rows          grid (G, pairs): k_cs_init_rows, which adds into the model with integer atomics
//   LUT, exchange slots and `out` are indexed by the pair's position in the call; state, pixels and histogram slot come from the table.
//
// The kernels are ht_cs_kernels.inc, the text ht_camshift.hip compiles its k_cs_* from; this unit supplies the look-ups through
// the call's device table (CspEntry).  Same wavefront count, same summation order, same bits as the few-stream schedule of
// ht_camshift_track_batch (options cs_fused_min=large, cs_cluster=0).
//
// Compiled as part of ht_backproject.hip (included at its end, like ht_ingest.hip): the library keeps ONE code object besides the three
// that profiles/traffic.json fingerprints.  No kernel name here carries one of the fingerprint's markers.  ht_backproject.hip has
// included ht_cs_device.h (cs_bin, the workgroup sizes, the device helpers) in front of its own kernels: this file sees it from there.
#include <cstring>
#include <vector>

#define HT_CSB_FN __host__ __device__ inline  // k_csb_resolve (ht_cs_best.hip, behind this file) calls the header's functions on the device
#include "ht_cs_best_plan.h"                 // the flag word of CspEntry.pad

namespace {

struct CspEntry {
    int32_t stream, frame;  // the pair
    int32_t slot;           // index of `frame` among the call's distinct frames = its chunk histograms in the scratch
    int32_t pad;            // flag word (ht_cs_best_plan.h): 0 for every call but ht_camshift_init_best
    ht_cs_rect rect;        // k_csp_init only
};
static_assert(sizeof(CspEntry) == 32, "CspEntry");

#define CS_K(name) k_csp_##name
typedef const CspEntry *__restrict__ CsLookup;  // the call's table: workgroup s is pair s
__device__ __forceinline__ int cs_stream_of(const CspEntry *e, int s) { return e[s].stream; }
__device__ __forceinline__ int cs_frame_of(const CspEntry *e, int s) { return e[s].frame; }
__device__ __forceinline__ int cs_slot_of(const CspEntry *e, int s) { return e[s].slot; }
#define CS_INIT_PARAMS CsLookup lk, HtCsState *__restrict__ states
#define CS_INIT_RECT(s_) lk[s_].rect
#define CS_INIT_SKIP(s_) if (lk[s_].pad & HT_CSB_F_SKIP) return;  // ht_camshift_init_best resolved the pair to "leave the stream alone"
#define CS_HIST_FRAMES_PARAM const int32_t *__restrict__ frame_list,  // the call's distinct frames, one per grid row
#define CS_HIST_FRAME(y_) frame_list[y_]
#include "ht_cs_kernels.inc"

// the models of the call's pairs = 0, in front of k_csp_init_rows: workgroup s clears the 16 KB of pair s's stream, 16 bytes per thread
__global__ __launch_bounds__(1024) void k_csp_zero_models(CsLookup lk, HtCsState *__restrict__ states) {
    CS_INIT_SKIP(blockIdx.x)
    reinterpret_cast<uint4 *>(states[cs_stream_of(lk, blockIdx.x)].model)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}
static_assert(sizeof(HtCsState::model) == 1024 * sizeof(uint4), "k_csp_zero_models: one uint4 per thread");

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

// the call's table -> device (entries, then the distinct frames): through the context's staged pair table (HtStagedTable, ht_internal.h),
// copied on the context's stream in front of the kernels that read it.
// ht_bp_pairs.hip sends its group records along (`extra`, extra_words 32-bit words behind the frame list; at most 8 per pair).
ht_status csp_upload(ht_ctx *c, const char *fn, const CspPlan &plan, const CspEntry **d_entries, const int32_t **d_frames, const void *extra = nullptr,
                     size_t extra_words = 0, const int32_t **d_extra = nullptr) {
    const size_t n = plan.entries.size(), base_words = n * (sizeof(CspEntry) / 4) + plan.frames.size(), words = base_words + extra_words;
    const size_t minimum = (size_t)c->cs_streams * (2 * sizeof(CspEntry) / 4 + 1);  // entry + frame + group record per stream
    ht_status st = ht_stage_reserve(c, &c->csp_tab, words * 4, minimum * 4, std::string(fn) + ": allocation of the pair table failed");
    if (st != HT_OK) return st;
    uint8_t *slot = nullptr;
    if ((st = ht_stage_take(c, &c->csp_tab, &slot)) != HT_OK) return st;
    std::memcpy(slot, plan.entries.data(), n * sizeof(CspEntry));
    std::memcpy(slot + n * sizeof(CspEntry), plan.frames.data(), plan.frames.size() * 4);
    if (extra_words) std::memcpy(slot + base_words * 4, extra, extra_words * 4);
    if ((st = ht_stage_commit(c, &c->csp_tab, words * 4)) != HT_OK) return st;
    const int32_t *d_tab = reinterpret_cast<const int32_t *>(c->csp_tab.d);
    *d_entries = reinterpret_cast<const CspEntry *>(d_tab);
    *d_frames = d_tab + n * (sizeof(CspEntry) / 4);
    if (d_extra) *d_extra = d_tab + base_words;
    return HT_OK;
}

// the schedule of a pair call of n pairs on nd distinct frames with this context's geometry and options (ht_cs_schedule.h)
HtCspTrackPlan csp_plan_track(ht_ctx *c, int n, int nd) {
    HtCspTrackIn in;
    in.n = n, in.nd = nd, in.W = c->W, in.H = c->H, in.num_cus = c->num_cus;
    in.cs_pairs_cluster = c->cs_pairs_cluster, in.cs_cluster = c->cs_cluster, in.cs_cluster_min_px = c->cs_cluster_min_px;
    in.dbg_cs_iters = c->dbg_cs_iters, in.cs_region_cap = c->cs_region_cap;
    return ht_cs_plan_track_pairs(in);
}

// one track() of every pair: table, histograms of the distinct frames, then what the plan says — one mean-shift workgroup per pair, or
// the pair's LUT and a cluster of G workgroups per pair; results to d_out[0 .. n).  *cluster: the call took the cluster form (its
// read-back fetches the error word)
ht_status csp_launch_track(ht_ctx *c, const CspPlan &plan, int32_t calc_angles, ht_cs_trackobj *d_out, bool *cluster) {
    const char *fn = "ht_camshift_track_pairs";
    const int n = (int)plan.entries.size(), nd = (int)plan.frames.size();
    const HtCspTrackPlan p = csp_plan_track(c, n, nd);
    *cluster = p.form == HT_CSP_CLUSTER;
    if (!c->csp_attr_set) {  // the cached search region needs more than the default 64 KB of LDS per workgroup
        HT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_csp_meanshift), hipFuncAttributeMaxDynamicSharedMemorySize, CS_REGION_CAP * 2));
        c->csp_attr_set = true;
    }
    const uint32_t nchunks = p.nchunks;
    const size_t need = (size_t)nd * nchunks * 4096;
    // the scratch is about to be replaced: what ht_camshift_debug_hist would read must not point into the old one, also when the allocation fails
    if (c->csp_hist_cap < need && c->cs_last_hist && c->cs_last_hist != c->d_cs_hist) c->cs_last_hist = nullptr, c->cs_last_n = 0;
    ht_status gs = ht_grow_device(c, &c->d_csp_hist, &c->csp_hist_cap, need, "ht_camshift_track_pairs: hipMalloc failed (chunk histograms)");
    if (gs != HT_OK) return gs;
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr;
    ht_status st = csp_upload(c, fn, plan, &d_entries, &d_flist);
    if (st != HT_OK) return st;
    {
        HtProfScope ps(c, p.hist.timer);
        hipLaunchKernelGGL(k_csp_hist, dim3(p.hist.grid_x, p.hist.grid_y), dim3(p.hist.block), 0, c->stream, c->d_frames, c->frame_stride, p.npix, p.chunk_px, d_flist,
                           c->d_csp_hist);
        HT_HIP(c, hipGetLastError());
    }
    if (p.form == HT_CSP_CLUSTER) {
        // d_cs_lut / d_cs_parts hold min(reserved, CL_MAX_STREAMS) streams (ht_cs_reserve_sizes) >= n here; the context's one stream orders
        // them against the batch cluster calls
        {
            HtProfScope ps(c, p.lut.timer);
            hipLaunchKernelGGL(k_csp_lut, dim3(p.lut.grid_x, p.lut.grid_y), dim3(p.lut.block), 0, c->stream, c->d_csp_hist, (int)nchunks, c->d_cs, d_entries, c->d_cs_lut,
                               reinterpret_cast<unsigned long long *>(c->d_cs_parts));
            HT_HIP(c, hipGetLastError());
        }
        HtProfScope ps(c, p.meanshift.timer);
        st = ht_cs_cluster_gate_begin(c);
        if (st != HT_OK) return st;
        hipLaunchKernelGGL(k_csp_meanshift_cluster, dim3(p.meanshift.grid_x), dim3(p.meanshift.block), p.meanshift.lds, c->stream, c->d_frames, c->frame_stride, c->W,
                           c->H, c->d_cs_lut, c->d_cs, d_entries, calc_angles, c->dbg_cs_iters, p.G, c->d_cs_parts, c->d_cs_err, c->h_cs_err_direct,
                           (long long)c->cs_barrier_budget, d_out, static_cast<uint32_t *>(nullptr), 0u);  // completed by the slot's event
        const hipError_t le = hipGetLastError();
        st = ht_cs_cluster_gate_end(c);
        HT_HIP(c, le);
        if (st != HT_OK) return st;
    } else {
        HtProfScope ps(c, p.meanshift.timer);
        hipLaunchKernelGGL(k_csp_meanshift, dim3(p.meanshift.grid_x), dim3(p.meanshift.block), p.meanshift.lds, c->stream, c->d_frames, c->frame_stride, c->W, c->H,
                           c->d_csp_hist, (int)nchunks, c->d_cs, d_entries, calc_angles, c->dbg_cs_iters, p.region_cap, d_out);
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
    int max_rh = 0;
    for (int32_t i = 0; i < n; i++) max_rh = std::max(max_rh, rects[i].height);
    const HtCsInitPlan ip = ht_cs_plan_init_pairs(c->cs_pairs_cluster, n, max_rh, c->num_cus);
    if (ip.rows) {
        HtProfScope ps(c, "csp_init_rows");
        hipLaunchKernelGGL(k_csp_zero_models, dim3(n), dim3(1024), 0, c->stream, d_entries, c->d_cs);
        hipLaunchKernelGGL(k_csp_init_rows, dim3(ip.G, n), dim3(CS_INIT_ROWS_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_entries, c->d_cs);
        HT_HIP(c, hipGetLastError());
    } else {
        HtProfScope ps(c, "csp_init");
        hipLaunchKernelGGL(k_csp_init, dim3(n), dim3(INIT_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_entries, c->d_cs);
        HT_HIP(c, hipGetLastError());
    }
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
    bool via_ring = false;
    ht_ctx::HtCsSlot *slot = nullptr;
    st = ht_cs_ring_begin(c, "ht_camshift_track_pairs", n, out, &via_ring, &slot);
    if (st != HT_OK) return st;
    bool cluster = false;
    if (slot) {
        st = csp_launch_track(c, plan, calc_angles, slot->h_out, &cluster);
        if (st != HT_OK) return st;
        slot->seq = 0u;  // completed by the event
        HT_HIP(c, hipEventRecord(slot->ev, c->stream));
        ht_cs_ring_commit(c, slot, n);
        return via_ring ? ht_camshift_track_collect(c, n, out) : HT_OK;
    }
    st = csp_launch_track(c, plan, calc_angles, c->d_cs_out, &cluster);
    if (st != HT_OK) return st;
    if (cluster) return ht_cs_read_back(c, "ht_camshift_track_pairs", out, c->d_cs_out, (size_t)n);  // the track objects and the cluster error word
    HT_HIP(c, hipMemcpyAsync(out, c->d_cs_out, sizeof(ht_cs_trackobj) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

void ht_cs_pairs_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    ht_stage_free(&c->csp_tab);
    if (c->d_csp_hist) (void)hipFree(c->d_csp_hist);
    c->d_csp_hist = nullptr, c->csp_hist_cap = 0;
}

// The record-driven initTracker (ht_camshift_init_best, k_csb_resolve) is compiled right behind this file, whose plan, table upload and
// init kernels it uses; ht_group.hip, whose records it reads, comes in front of both in ht_backproject.hip.
#include "ht_cs_best.hip"
// ... and behind it the same hand-off for every grouped face of a frame (ht_camshift_init_faces, k_csf_resolve).
#include "ht_cs_faces.hip"

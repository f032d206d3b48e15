// ht_camshift.hip — camshift.Tracker on the device (reference: /root/reference/src/camshift.js).
//
//   Histogram            camshift.js:49-72     bins[256*(R>>4) + 16*(G>>4) + (B>>4)]++ over RGBA pixels
//   initTracker          camshift.js:198-211   model histogram of the tracked rect (outside the canvas = transparent
//                                              black = bin 0), search window = rect
//   track -> camShift    camshift.js:213-259   size / angle from second moments, new window = 1.1 x object size
//   meanShift            camshift.js:261-312   full-frame histogram, weights, <= 10 window iterations
//   getWeights           camshift.js:314-330   w = ch ? min(mh/ch, 1) : 0
//   Moments              camshift.js:79-120
//
// Device mapping: one tracker ("stream") per frame of the bound batch; state (model histogram, search window, track
// object) stays in HBM between calls.  track = (1) k_cs_hist: LDS-privatised 4096-bin histogram per frame chunk,
// written as partial histograms (<= 8 per stream, no global atomics); (2) k_cs_meanshift: ONE workgroup per stream keeps the 4096-entry weight LUT in LDS
// (binary64, 32 KB) and runs the whole <=10-iteration mean-shift loop: each iteration is a window moment reduction
// straight from the RGBA pixels through the LUT — the back-projection image of the reference (camshift.js:332-353) is
// never materialised, it is only observable through debug getters.  Moment sums are binary64 with a fixed
// thread-to-pixel assignment and a fixed reduction tree (deterministic); the summation ORDER differs from the
// reference's column-major scalar loop, so results are equal up to rounding in the last bits of xc/yc — the
// acceptance bound of BASELINE.json (+-1 px, +-0.5 deg) covers the rare truncation flips this can cause.
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "ht_internal.h"

namespace {

// the device helpers this unit shares with the pair kernels (ht_cs_pairs.hip) and the back-projection: cs_bin, CS_STAMP, CS_NT / HIST_NT /
// HIST_UNROLL / INIT_NT / CS_REGION_CAP, CS_BATCH_LOADED, toint32, hist_add_wave, Mom, the DPP wave sum, CsRegion, cs_cache_region,
// window_moments*, meanshift_body
#include "ht_cs_device.h"

// k_cs_init, k_cs_init_rows, k_cs_hist, k_cs_meanshift, k_cs_lut and k_cs_meanshift_cluster are ht_cs_kernels.inc with the look-ups of a batch: stream first + s works on bound frame s,
// whose chunk histograms are slot s, and its rect is rects[s]
#define CS_K(name) k_cs_##name
typedef int CsLookup;  // `first`
__device__ __forceinline__ int cs_stream_of(int first, int s) { return first + s; }
__device__ __forceinline__ int cs_frame_of(int, int s) { return s; }
__device__ __forceinline__ int cs_slot_of(int, int s) { return s; }
#define CS_INIT_PARAMS const ht_cs_rect *__restrict__ rects, HtCsState *__restrict__ states, CsLookup lk
#define CS_INIT_RECT(s_) rects[s_]
#define CS_HIST_FRAMES_PARAM
#define CS_HIST_FRAME(y_) (y_)

// (the chunk plan of the histogram pass — HIST_MAXCHUNKS, hist_max_chunks, hist_chunks — and every workgroup size: ht_cs_schedule.h)

#define CS_KERNELS_PART 1  // k_cs_init
#include "ht_cs_kernels.inc"

#define CS_KERNELS_PART 3  // k_cs_init_rows
#include "ht_cs_kernels.inc"

#define CS_KERNELS_PART 2  // k_cs_hist, k_cs_meanshift: behind k_cs_init_rows, the order the recorded code object has
#include "ht_cs_kernels.inc"

// One launch per track() call when there are enough streams to fill the chip by themselves: ONE 1024-thread workgroup per stream
// does the full-frame histogram in LDS, turns it into the weight LUT in place (no partial histograms through HBM, no second
// launch) and runs the mean-shift loop.  Per stream and call the only memory traffic left is the frame itself (4*W*H, then the
// window passes from L2), the model histogram (16 KB) and the state.
// FUSED_NT threads, or FUSED_NT_SMALL with a CS_REGION_CAP_SMALL region: two forms with the same bits, chosen per launch (ht_cs_schedule.h).

// Up to CS_SEQ_MAX successive track() calls of every stream in ONE launch (ht_camshift_track_sequence): the frame batches of the calls
// travel as kernel arguments, a workgroup walks its stream's calls in order.  The calls of a stream depend on each other through its
// search window, the streams do not: with one launch per call every call waited for its slowest stream (and paid a launch); now a
// workgroup that converges quickly on one frame is already working on the next one.
constexpr int CS_SEQ_MAX = 64;
struct CsFrameList {
    const uint8_t *p[CS_SEQ_MAX];
};
// Everything the kernel needs travels in ONE struct = the whole kernarg segment.  The kernel reads it through the kernarg pointer,
// made opaque at the top of every call of the sequence: the ~20 scalars are then re-loaded (scalar loads from the constant cache) per
// call instead of being kept alive across the whole call body — as loop invariants they cost the 128-VGPR kernel 52 spilled VGPRs and
// 24 spilled SGPRs (212 B of scratch per lane).
struct CsFusedArgs {
    CsFrameList flist;
    int ncalls;
    int W, H;
    uint32_t npix;
    size_t frame_stride;
    HtCsState *states;
    int first, calc_angles, max_it, region_cap;
    ht_cs_trackobj *out;
    uint32_t *dbg_hist;
    uint32_t out_call_stride;
};
typedef const CsFusedArgs __attribute__((address_space(4))) *CsFusedArgsPtr;

template <bool SEQ, int NT>
__global__ __launch_bounds__(NT, 4) void k_cs_track_fused(const CsFusedArgs args_by_value) {
    constexpr int NWV = FUSED_NT / 64;  // wavefronts the moment passes are laid out for (window_moments), whatever NT is
    extern __shared__ __attribute__((aligned(16))) uint8_t cs_dyn[];  // [region_cap] u16 bins of the cached search region
    __shared__ double lut[4096];
    // the frame's histogram overlays the upper half of the LUT it is turned into (every bin is read into registers, then a barrier,
    // then the weights are written): 16 KB of LDS that the cached search region of the 512-thread form gets instead
    uint32_t *const h = reinterpret_cast<uint32_t *>(lut + 2048);
    __shared__ double red[6][NWV];
    __shared__ int s_sw[4];
    (void)args_by_value;
    CsFusedArgsPtr ka = (CsFusedArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    const int s = blockIdx.x;
    const int ncalls = SEQ ? ka->ncalls : 1;
    for (int call = 0; call < ncalls; call++) {
    if (SEQ) asm volatile("" : "+s"(ka));  // opaque: nothing loaded through ka before this point stays live across the call
    if (call) __syncthreads();  // thread 0 stored the new search window; every wavefront is done with h / lut / the cached region
    const int W = ka->W, H = ka->H, region_cap = ka->region_cap;
    const uint32_t npix = ka->npix;
    HtCsState &st = ka->states[ka->first + s];
    const uint8_t *frame = ka->flist.p[call] + (size_t)s * ka->frame_stride;
    uint32_t *const dbg_hist = ka->dbg_hist;
#ifdef HT_CS_TIMELINE
    __shared__ unsigned long long s_stamps[32];
    if (threadIdx.x < 32) s_stamps[threadIdx.x] = 0;
    unsigned long long *stamps = s_stamps;
    __syncthreads();
#else
    unsigned long long *stamps = nullptr;
#endif
    CS_STAMP(stamps, 0);
    for (int i = threadIdx.x; i < 4096; i += NT) h[i] = 0;
    if (threadIdx.x < 4) s_sw[threadIdx.x] = st.sw[threadIdx.x];
    __syncthreads();
    // the search region (search window + margin) is cached in LDS as histogram bins for the moment passes; when rows are whole
    // 16-byte groups the histogram pass below stashes it on the way (the frame is read exactly once), otherwise a separate copy
    // pass after the LUT does (cs_cache_region)
    uint16_t *const rbins = reinterpret_cast<uint16_t *>(cs_dyn);
    const int qpr = W >> 2, rpi = qpr > 0 ? NT / qpr : 0;  // 16-byte groups per row, rows per sweep of the workgroup
    const bool rows2d = (W & 3) == 0 && rpi >= 1;
    CsRegion R = {rbins, 0, 0, 0, 0};
    if (rows2d) R = cs_region_rect(W, H, s_sw, rbins, region_cap);
    {  // camshift.Histogram of the whole frame (camshift.js:268), counts merged per thread and per wavefront like k_cs_hist
        const uint4 *img4 = reinterpret_cast<const uint4 *>(frame);
        if (rows2d) {
            // thread = (row within the sweep, 16-byte group of the row): its column never changes, so the region test is two row
            // compares per load; 8 independent loads per thread in flight
            const int trow = (int)threadIdx.x / qpr, tq = (int)threadIdx.x - trow * qpr;
            const bool tact = trow < rpi;
            const int colx = 4 * tq - R.x0;  // column of the group's first pixel inside the region
            const bool colhit = R.rw > 0 && colx + 3 >= 0 && colx < R.rw;
            for (int row0 = trow; row0 - trow < H; row0 += 8 * rpi) {  // same trip count for every thread (ballots inside)
                uint4 p[8];
#pragma unroll
                for (int u = 0; u < 8; u++) p[u] = img4[(size_t)min(row0 + u * rpi, H - 1) * qpr + tq];  // clamped address, masked below
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int row = row0 + u * rpi;
                    const bool on = tact && row < H;
                    const uint32_t b0 = cs_bin(p[u].x), b1 = cs_bin(p[u].y), b2 = cs_bin(p[u].z), b3 = cs_bin(p[u].w);
                    const bool flat = (b0 == b1) && (b2 == b3) && (b0 == b2);
                    hist_add_wave(h, b0, flat ? 4u : 1u, on);
                    if (on && !flat) {
                        atomicAdd(&h[b1], 1u);
                        atomicAdd(&h[b2], 1u);
                        atomicAdd(&h[b3], 1u);
                    }
                    const int ry = row - R.y0;
                    if (on && colhit && ry >= 0 && ry < R.rh) {
                        uint16_t *d = rbins + ry * R.rw + colx;
                        if (colx >= 0) d[0] = (uint16_t)b0;
                        if (colx + 1 >= 0 && colx + 1 < R.rw) d[1] = (uint16_t)b1;
                        if (colx + 2 >= 0 && colx + 2 < R.rw) d[2] = (uint16_t)b2;
                        if (colx + 3 < R.rw) d[3] = (uint16_t)b3;
                    }
                }
            }
        } else {
            const uint32_t nquad = npix / 4;
            // 8 independent 16-byte loads per thread in flight (128 KB per workgroup): one workgroup has a whole frame to pull
            for (uint32_t i0 = threadIdx.x; i0 < nquad; i0 += 8 * NT) {
                uint4 p[8];
#pragma unroll
                for (int u = 0; u < 8; u++) p[u] = img4[min(i0 + u * NT, nquad - 1)];  // clamped address, masked below
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const bool on = i0 + u * NT < nquad;
                    const uint32_t b0 = cs_bin(p[u].x), b1 = cs_bin(p[u].y), b2 = cs_bin(p[u].z), b3 = cs_bin(p[u].w);
                    const bool flat = (b0 == b1) && (b2 == b3) && (b0 == b2);
                    hist_add_wave(h, b0, flat ? 4u : 1u, on);
                    if (on && !flat) {
                        atomicAdd(&h[b1], 1u);
                        atomicAdd(&h[b2], 1u);
                        atomicAdd(&h[b3], 1u);
                    }
                }
            }
            const uint32_t *img1 = reinterpret_cast<const uint32_t *>(frame);
            for (uint32_t i = nquad * 4 + threadIdx.x; i < npix; i += NT) atomicAdd(&h[cs_bin(img1[i])], 1u);  // < 4 pixels
        }
    }
    __syncthreads();
    CS_STAMP(stamps, 1);
    {  // getWeights, camshift.js:314-330
        const uint4 *model4 = reinterpret_cast<const uint4 *>(st.model);
        constexpr int RND = 1024 / NT;  // 4 bins per thread and round
        uint4 mq[RND], cq[RND];
#pragma unroll
        for (int rd = 0; rd < RND; rd++) {
            const int i4 = (int)threadIdx.x + rd * NT;
            mq[rd] = model4[i4];
            cq[rd] = reinterpret_cast<const uint4 *>(h)[i4];
            if (dbg_hist) reinterpret_cast<uint4 *>(dbg_hist + (size_t)s * 4096)[i4] = cq[rd];
        }
        __syncthreads();  // every bin of h is in a register: the weights may overwrite it
#pragma unroll
        for (int rd = 0; rd < RND; rd++) {
            const int i4 = (int)threadIdx.x + rd * NT;
            const uint32_t chv[4] = {cq[rd].x, cq[rd].y, cq[rd].z, cq[rd].w}, mv[4] = {mq[rd].x, mq[rd].y, mq[rd].z, mq[rd].w};
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
    CS_STAMP(stamps, 2);
    // the search region: the frame went through this CU a moment ago, but not into any cache that would still hold it
    if (!rows2d) R = cs_cache_region<NT>(reinterpret_cast<const uint32_t *>(frame), W, H, s_sw, rbins, region_cap);
    __syncthreads();  // LUT and region complete
    CS_STAMP(stamps, 3);
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frame);
    ht_cs_trackobj *const out = ka->out;
    meanshift_body(W, H, s_sw, st, ka->calc_angles, ka->max_it, out ? out + (size_t)call * ka->out_call_stride + s : nullptr, stamps, true,
                   [&](int x, int y, int w, int h) { return window_moments_any<true, NWV, NT / 64>(img, W, lut, R, x, y, w, h, red); });
#ifdef HT_CS_TIMELINE
    if (threadIdx.x == 0 && dbg_hist)
        for (int i = 0; i < 30; i++) reinterpret_cast<unsigned long long *>(dbg_hist + (size_t)s * 4096 + 4032)[i] = s_stamps[i];
#endif
    }  // next call of this stream
}

// ---- few large streams: a CLUSTER of workgroups per stream ---------------------------------------------------------------
// One workgroup streams a window at one CU's memory rate: a 360 x 360 search window of a 1080p feed (130 k pixels, 0.5 MB per
// pass) took ~30 us per pass, 146 us per track() call.  Here G workgroups share every pass (rows interleaved over all their
// wavefronts) and publish their six partial sums with agent-scope stores into the pass's exchange slot, whose entries k_cs_lut
// marked "not written yet" (a NaN no sum can be): every workgroup polls the G x 6 entries, one thread per entry, until the mark is
// gone — the value that ends the wait is the partial sum itself (round 5; until then: store, drain, arrive on a counter, poll the
// counter, read the partials = three dependent L2 round trips, ~3 us per pass).  No agent-scope fences: every payload word is an
// sc1 store on one side and an sc1 load on the other.  Every workgroup sums the G partials in the same order, so all of them take
// identical mean-shift decisions; workgroup 0 writes the state.  The grid (streams x G <= 256 workgroups) is always co-resident: the spin cannot starve a workgroup that has not started.
// (CL_NT threads, <= CL_MAXG workgroups per stream, CL_SLOTS exchange slots: ht_cs_schedule.h)
// (CL_UNWRITTEN, ClusterSync, cluster_moments: ht_cs_device.h)
#define CS_KERNELS_PART 4  // k_cs_lut, k_cs_meanshift_cluster
#include "ht_cs_kernels.inc"

}  // namespace

// One cluster launch (k_cs_meanshift_cluster) in flight per device and process: its workgroups spin on each other, so two such grids
// from different contexts must not share the chip's workgroup slots (each could hold the slots the other's missing workgroups need).
// The serialisation is device-side — the launching stream waits for the event recorded after the previous cluster launch on that
// device — so no host thread blocks.
namespace {
struct ClusterGate {
    std::mutex mu;
    struct Dev {
        hipEvent_t last = nullptr;            // recorded after the most recent cluster launch (only while `multi`)
        std::vector<const ht_ctx *> users;    // contexts that have launched a cluster grid on this device
        std::vector<const ht_ctx *> fused;    // contexts that have launched k_cs_track_fused on this device (fused_threads)
        bool multi = false;                   // more than one user: every launch waits for `last` and records it
    };
    std::map<int, Dev> dev;
};
ClusterGate &cluster_gate() {
    static ClusterGate g;
    return g;
}

// ht_camshift_free: the context stops counting as a user of its device's cluster gate (its stream has been synchronised)
void cluster_gate_forget(const ht_ctx *c) {
    ClusterGate &gate = cluster_gate();
    std::lock_guard<std::mutex> lk(gate.mu);
    auto it = gate.dev.find(c->device);
    if (it == gate.dev.end()) return;
    auto &u = it->second.users;
    u.erase(std::remove(u.begin(), u.end(), c), u.end());
    auto &fu = it->second.fused;
    fu.erase(std::remove(fu.begin(), fu.end(), c), fu.end());
    if (u.size() <= 1 && it->second.multi) {
        // back to one user: its recorded grids are ordered by its own stream from here on
        it->second.multi = false;
    }
}
}  // namespace
// ht_detect_enqueue around its graph capture.  Setting the flag takes the gate's lock, and fused_threads() holds that lock across its
// queries: a query of this context's stream either completed before the capture began or sees the flag and is skipped.
void ht_capture_mark(ht_ctx *c, bool on) {
    if (on) {
        std::lock_guard<std::mutex> lk(cluster_gate().mu);
        c->capturing.store(true);
    } else {
        c->capturing.store(false);
    }
}
// fetched with every result read-back: a cluster barrier that ran out of its cycle budget surfaces as a status code
ht_status ht_cs_check_err(ht_ctx *c, const char *where) {
    const bool direct = c->h_cs_err_direct && __atomic_load_n(c->h_cs_err_direct, __ATOMIC_ACQUIRE) != 0;
    if (!direct && (!c->h_cs_err || *c->h_cs_err == 0)) return HT_OK;
    if (c->h_cs_err) *c->h_cs_err = 0;
    if (c->h_cs_err_direct) __atomic_store_n(c->h_cs_err_direct, 0u, __ATOMIC_RELEASE);
    (void)hipMemsetAsync(c->d_cs_err, 0, sizeof(uint32_t), c->stream);
    return ht_fail(c, HT_ERR_STATE, std::string(where) + ": a camshift cluster barrier timed out (workgroups of one stream were not co-resident); the affected streams' state is undefined — re-initialise them");
}

// The cluster gate around one launch of a grid that spins on its own workgroups (launch_track here, csp_launch_track in ht_cs_pairs.hip).
// begin takes the gate's lock and, on success, keeps it until end; a failed begin has released it.
ht_status ht_cs_cluster_gate_begin(ht_ctx *c) {
    ClusterGate &gate = cluster_gate();
    std::unique_lock<std::mutex> lk(gate.mu);
    ClusterGate::Dev &gd = gate.dev[c->device];
    if (std::find(gd.users.begin(), gd.users.end(), c) == gd.users.end()) {
        // A single context's cluster grids are ordered by its own stream: no event traffic (a record is a barrier packet of its own
        // between this step's last and the next step's first kernel).  When a second context of the device starts using the
        // cluster path, the unrecorded grids of the first are drained once, and from then on every launch waits and records.
        if (!gd.users.empty() && !gd.multi) {
            HT_HIP(c, hipDeviceSynchronize());
            gd.multi = true;
        }
        gd.users.push_back(c);
    }
    if (gd.multi) {
        if (!gd.last) HT_HIP(c, hipEventCreateWithFlags(&gd.last, hipEventDisableTiming));
        else HT_HIP(c, hipStreamWaitEvent(c->stream, gd.last, 0));  // the previous cluster grid on this device (any context) has drained
    }
    lk.release();  // held until ht_cs_cluster_gate_end
    return HT_OK;
}
ht_status ht_cs_cluster_gate_end(ht_ctx *c) {
    ClusterGate &gate = cluster_gate();
    std::unique_lock<std::mutex> lk(gate.mu, std::adopt_lock);
    ClusterGate::Dev &gd = gate.dev[c->device];
    if (gd.multi && gd.last) HT_HIP(c, hipEventRecord(gd.last, c->stream));
    return HT_OK;
}

// the histogram pass, also for callers outside this unit (ht_backproject.hip): host code only, the kernel stays here
ht_status ht_cs_hist_launch(ht_ctx *c, const uint8_t *frames, size_t frame_stride, int n, uint32_t npix, uint32_t chunk_px, uint32_t nchunks, uint32_t *hist) {
    hipLaunchKernelGGL(k_cs_hist, dim3(nchunks, n), dim3(HIST_NT), 0, c->stream, frames, frame_stride, npix, chunk_px, hist);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

extern "C" ht_status ht_camshift_reserve(ht_ctx *c, int32_t nstreams) {
    if (!c || nstreams <= 0) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    if (c->cs_streams >= nstreams) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    // every new buffer first; the context only changes once all of them exist (a failed reservation keeps the old trackers usable)
    const HtCsReserveSizes sz = ht_cs_reserve_sizes(nstreams);
    HtCsState *ns = nullptr;
    uint32_t *nhist = nullptr, *nerr = c->d_cs_err, *herr = c->h_cs_err;
    ht_cs_trackobj *nout = nullptr;
    double *nlut = nullptr, *nparts = nullptr;
    bool ok = hipMalloc(&ns, sz.states) == hipSuccess && hipMalloc(&nhist, sz.hist) == hipSuccess && hipMalloc(&nout, sz.out) == hipSuccess &&
              hipMalloc(&nlut, sz.lut) == hipSuccess && hipMalloc(&nparts, sz.parts) == hipSuccess;
    if (ok && !nerr) ok = hipMalloc(&nerr, sz.err_word) == hipSuccess && hipMemset(nerr, 0, sz.err_word) == hipSuccess;
    if (ok && !herr) {
        ok = hipHostMalloc(reinterpret_cast<void **>(&herr), sz.err_word, hipHostMallocDefault) == hipSuccess;
        if (ok) *herr = 0;
    }
    if (ok) ok = hipMemset(ns, 0, sz.states) == hipSuccess;
    if (ok && c->d_cs)  // keep existing trackers
        ok = hipMemcpy(ns, c->d_cs, sizeof(HtCsState) * (size_t)c->cs_streams, hipMemcpyDeviceToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (ns) (void)hipFree(ns);
        if (nhist) (void)hipFree(nhist);
        if (nout) (void)hipFree(nout);
        if (nlut) (void)hipFree(nlut);
        if (nparts) (void)hipFree(nparts);
        if (nerr && nerr != c->d_cs_err) (void)hipFree(nerr);
        if (herr && herr != c->h_cs_err) (void)hipHostFree(herr);
        return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_reserve: allocation failed (the previous reservation is unchanged)");
    }
    if (c->d_cs) (void)hipFree(c->d_cs);
    if (c->d_cs_hist) (void)hipFree(c->d_cs_hist);
    if (c->d_cs_out) (void)hipFree(c->d_cs_out);
    if (c->d_cs_lut) (void)hipFree(c->d_cs_lut);
    if (c->d_cs_parts) (void)hipFree(c->d_cs_parts);
    c->d_cs = ns, c->d_cs_hist = nhist, c->d_cs_out = nout, c->d_cs_lut = nlut, c->d_cs_parts = nparts;
    c->d_cs_err = nerr, c->h_cs_err = herr;
    c->cs_last_n = c->cs_last_chunks = 0;  // the debug histogram buffer is new
    c->cs_last_hist = nullptr;
    c->cs_streams = nstreams;
    // result ring of the enqueue-only track calls (the stream was synchronised above: no slot is in use; uncollected results are dropped)
    c->cs_ring_head = c->cs_ring_count = 0;
    if (!c->h_cs_err_direct) {
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_cs_err_direct), sz.err_word, hipHostMallocDefault) != hipSuccess)
            return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_reserve: hipHostMalloc failed");
        *c->h_cs_err_direct = 0;
    }
    for (auto &sl : c->cs_ring) {
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        sl.h_out = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&sl.h_out), sz.ring_out, hipHostMallocDefault) != hipSuccess) {
            c->cs_ring_streams = 0;
            return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_reserve: hipHostMalloc failed");
        }
        if (!sl.ev && hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) return ht_fail(c, HT_ERR_HIP, "ht_camshift_reserve: hipEventCreate failed");
        if (sl.h_flag) (void)hipHostFree(sl.h_flag);
        sl.h_flag = nullptr, sl.seq = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&sl.h_flag), sz.ring_flags, hipHostMallocDefault) != hipSuccess) {
            c->cs_ring_streams = 0;
            return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_reserve: hipHostMalloc failed");
        }
        std::memset(sl.h_flag, 0, sz.ring_flags);
    }
    c->cs_ring_streams = nstreams;
    return HT_OK;
}

void ht_camshift_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_cs_err) (void)hipFree(c->d_cs_err);
    if (c->h_cs_err) (void)hipHostFree(c->h_cs_err);
    if (c->h_cs_err_direct) (void)hipHostFree(c->h_cs_err_direct);
    for (auto &sl : c->cs_ring) {
        if (sl.h_out) (void)hipHostFree(sl.h_out);
        if (sl.h_flag) (void)hipHostFree(sl.h_flag);
        if (sl.ev) (void)hipEventDestroy(sl.ev);
    }
    cluster_gate_forget(c);
    if (c->h_cs_rects) (void)hipHostFree(c->h_cs_rects);
    if (c->ev_cs_rects) (void)hipEventDestroy(c->ev_cs_rects);
    if (c->d_cs) (void)hipFree(c->d_cs);
    if (c->d_cs_hist) (void)hipFree(c->d_cs_hist);
    if (c->d_cs_out) (void)hipFree(c->d_cs_out);
    if (c->d_cs_seq_out) (void)hipFree(c->d_cs_seq_out);
    if (c->d_cs_lut) (void)hipFree(c->d_cs_lut);
    if (c->d_cs_parts) (void)hipFree(c->d_cs_parts);
}

extern "C" ht_status ht_camshift_init_batch(ht_ctx *c, int32_t first, int32_t n, const ht_cs_rect *rects) {
    HtRange range("ht_camshift_init_batch");
    if (!c || !rects) return HT_ERR_INVALID;
    if (!c->d_frames || n <= 0 || n > c->nframes) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_batch: bind n frames first");
    if (first < 0 || first + n > c->cs_streams) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_init_batch: stream range not reserved");
    HT_HIP(c, hipSetDevice(c->device));
    ht_cs_rect *d_rects = reinterpret_cast<ht_cs_rect *>(c->d_cs_out);  // scratch: sizeof(ht_cs_trackobj) >= sizeof(ht_cs_rect); enqueue-only track calls keep their results in the pinned ring
    // rects[] is the caller's (pageable) memory: staged in a pinned buffer of the context, so the copy is asynchronous and the call
    // does not wait for the stream — a streaming host enqueues the next track step right behind initTracker (the stream synchronisation
    // that used to end this call was 15-20 us of idle GPU per detect step of the C5 loop)
    if (c->h_cs_rects_cap < n) {
        if (c->h_cs_rects) {
            HT_HIP(c, hipStreamSynchronize(c->stream));
            (void)hipHostFree(c->h_cs_rects);
        }
        c->h_cs_rects = nullptr, c->h_cs_rects_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_cs_rects), sizeof(ht_cs_rect) * (size_t)c->cs_streams, hipHostMallocDefault) != hipSuccess)
            return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_init_batch: hipHostMalloc failed");
        c->h_cs_rects_cap = c->cs_streams;
        if (!c->ev_cs_rects) HT_HIP(c, hipEventCreateWithFlags(&c->ev_cs_rects, hipEventDisableTiming));
    } else {
        HT_HIP(c, hipEventSynchronize(c->ev_cs_rects));  // the previous call's copy has left the staging buffer (long ago, normally)
    }
    std::memcpy(c->h_cs_rects, rects, sizeof(ht_cs_rect) * (size_t)n);
    HT_HIP(c, hipMemcpyAsync(d_rects, c->h_cs_rects, sizeof(ht_cs_rect) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_cs_rects, c->stream));
    {
        HtProfScope ps(c, "cs_init");
        int max_rh = 0;
        for (int i = 0; i < n; i++) max_rh = std::max(max_rh, rects[i].height);
        const HtCsInitPlan ip = ht_cs_plan_init(n, max_rh, c->num_cus);
        if (ip.rows) {
            HT_HIP(c, hipMemset2DAsync(c->d_cs[first].model, sizeof(HtCsState), 0, sizeof(uint32_t) * 4096, (size_t)n, c->stream));
            hipLaunchKernelGGL(k_cs_init_rows, dim3(ip.G, n), dim3(CS_INIT_ROWS_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_rects, c->d_cs, first);
        } else {
            hipLaunchKernelGGL(k_cs_init, dim3(n), dim3(INIT_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_rects, c->d_cs, first);
        }
        HT_HIP(c, hipGetLastError());
    }
    return HT_OK;
}

// Threads per workgroup of k_cs_track_fused for a launch of n streams (ht_cs_fused_form): this is the part of the choice that needs the
// device — does ANOTHER live context of the device that uses this path have work in flight right now (hipStreamQuery on its stream: no
// packet, ~1 us)?
static int fused_threads(ht_ctx *c, int n) {
    if (ht_cs_fused_form_forced(c->cs_fused_nt)) return c->cs_fused_nt;
    bool other_busy = false;
    {
        ClusterGate &gate = cluster_gate();
        std::lock_guard<std::mutex> lk(gate.mu);  // ht_destroy forgets a context under this lock before it destroys its stream
        auto &fu = gate.dev[c->device].fused;
        if (std::find(fu.begin(), fu.end(), c) == fu.end()) fu.push_back(c);
        for (const ht_ctx *o : fu) {
            if (o == c || !o->stream) continue;
            // a context that is capturing its detect sequence is about to have work in flight; its stream must not be queried
            // (hipErrorStreamCaptureUnsupported, and the capture may be invalidated: ADVICE round 5)
            if (o->capturing.load() || hipStreamQuery(o->stream) == hipErrorNotReady) {
                other_busy = true;
                break;
            }
        }
        (void)hipGetLastError();  // hipErrorNotReady is an answer, not an error: keep it out of the launch checks that follow
    }
    return ht_cs_fused_form(c->cs_fused_nt, n, c->num_cus, other_busy);
}

// the schedule of a track() call of n streams with this context's geometry, reservation and options (ht_cs_schedule.h)
static HtCsTrackPlan plan_track(ht_ctx *c, int n) {
    HtCsTrackIn in;
    in.n = n, in.cs_streams = c->cs_streams, in.W = c->W, in.H = c->H, in.num_cus = c->num_cus;
    in.cs_fused_min_streams = c->cs_fused_min_streams, in.cs_cluster = c->cs_cluster, in.cs_cluster_min_px = c->cs_cluster_min_px;
    in.dbg_cs_iters = c->dbg_cs_iters, in.cs_region_cap = c->cs_region_cap;
    if (ht_cs_takes_fused(n, c->cs_fused_min_streams)) in.fused_nt = fused_threads(c, n);
    return ht_cs_plan_track(in);
}

// k_cs_track_fused as the plan says: ncalls successive track() calls of streams [first, first + n), call k on frames[k]; the track
// objects of call k go to d_out + k * out_call_stride (stride 0: the last call's remain).  `seq`: the instantiation whose workgroups walk
// a list of calls (ht_camshift_track_sequence); a single track() call launches the other one, which ignores everything but frames[0].
static ht_status launch_fused(ht_ctx *c, const HtCsTrackPlan &p, bool seq, const void *const *frames, int ncalls, size_t frame_stride, int32_t first,
                              int32_t n, int32_t calc_angles, ht_cs_trackobj *d_out, uint32_t out_call_stride) {
    const bool small = p.form == HT_CS_FUSED_512;
    const dim3 grid(p.fused.grid_x), block(p.fused.block);
    HtProfScope ps(c, p.fused.timer);
    c->cs_fused_launches[small ? 1 : 0]++;
    CsFusedArgs ka;
    std::memset(&ka, 0, sizeof(ka));
    for (int k = 0; k < ncalls; k++) ka.flist.p[k] = static_cast<const uint8_t *>(frames[k]);
    ka.ncalls = ncalls, ka.W = c->W, ka.H = c->H, ka.npix = p.npix, ka.frame_stride = frame_stride, ka.states = c->d_cs, ka.first = first;
    ka.calc_angles = calc_angles, ka.max_it = c->dbg_cs_iters, ka.region_cap = p.region_cap, ka.out = d_out, ka.out_call_stride = out_call_stride;
    ka.dbg_hist = c->cs_keep_hist ? c->d_cs_hist : nullptr;
    // (the instantiations are emitted in the order they are named here: the recorded camshift code object has this one)
    if (!seq && !small) hipLaunchKernelGGL((k_cs_track_fused<false, FUSED_NT>), grid, block, p.fused.lds, c->stream, ka);
    else if (!seq) hipLaunchKernelGGL((k_cs_track_fused<false, FUSED_NT_SMALL>), grid, block, p.fused.lds, c->stream, ka);
    else if (!small) hipLaunchKernelGGL((k_cs_track_fused<true, FUSED_NT>), grid, block, p.fused.lds, c->stream, ka);
    else hipLaunchKernelGGL((k_cs_track_fused<true, FUSED_NT_SMALL>), grid, block, p.fused.lds, c->stream, ka);
    HT_HIP(c, hipGetLastError());
    c->cs_last_first = first, c->cs_last_n = n, c->cs_last_chunks = c->cs_keep_hist ? 1 : 0;
    c->cs_last_hist = c->d_cs_hist;
    return HT_OK;
}

// one track() call of streams [first, first + n) on frames[0..n): plan, then launch what the plan says; results to d_out[0..n)
// done_flags (pinned, n words) / done_seq: completion marks for an enqueue-only call — written by the cluster kernel if that path is
// taken (*flags_used = true), otherwise the caller records its event.
static ht_status launch_track(ht_ctx *c, const uint8_t *frames, size_t frame_stride, int32_t first, int32_t n, int32_t calc_angles,
                              ht_cs_trackobj *d_out, uint32_t *done_flags = nullptr, uint32_t done_seq = 0u, bool *flags_used = nullptr) {
    if (!c->cs_attr_set) {  // the cached search region needs more than the default 64 KB of LDS per workgroup (per context = per device)
        HT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_cs_track_fused<false, FUSED_NT>), hipFuncAttributeMaxDynamicSharedMemorySize, CS_REGION_CAP * 2));
        HT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_cs_meanshift), hipFuncAttributeMaxDynamicSharedMemorySize, CS_REGION_CAP * 2));
        c->cs_attr_set = true;
    }
    const HtCsTrackPlan p = plan_track(c, n);
    if (p.form == HT_CS_FUSED_1024 || p.form == HT_CS_FUSED_512) {
        const void *frame_list[1] = {frames};
        return launch_fused(c, p, false, frame_list, 1, frame_stride, first, n, calc_angles, d_out, 0u);
    }
    uint32_t *hist = c->d_cs_hist;
    double *lut = c->d_cs_lut;
    {
        HtProfScope ps(c, p.hist.timer);
        ht_status st = ht_cs_hist_launch(c, frames, frame_stride, n, p.npix, p.chunk_px, p.nchunks, hist);
        if (st != HT_OK) return st;
    }
    if (p.form == HT_CS_CLUSTER) {
        {
            HtProfScope ps(c, p.lut.timer);
            hipLaunchKernelGGL(k_cs_lut, dim3(p.lut.grid_x, p.lut.grid_y), dim3(p.lut.block), 0, c->stream, hist, (int)p.nchunks, c->d_cs, first, lut,
                               reinterpret_cast<unsigned long long *>(c->d_cs_parts));
            HT_HIP(c, hipGetLastError());
        }
        HtProfScope ps(c, p.meanshift.timer);
        if (flags_used) *flags_used = done_flags != nullptr;
        ht_status gs = ht_cs_cluster_gate_begin(c);
        if (gs != HT_OK) return gs;
        hipLaunchKernelGGL(k_cs_meanshift_cluster, dim3(p.meanshift.grid_x), dim3(p.meanshift.block), p.meanshift.lds, c->stream, frames, frame_stride, c->W,
                           c->H, lut, c->d_cs, first, calc_angles, c->dbg_cs_iters, p.G, c->d_cs_parts, c->d_cs_err, c->h_cs_err_direct,
                           (long long)c->cs_barrier_budget, d_out, done_flags, done_seq);
        const hipError_t le = hipGetLastError();
        gs = ht_cs_cluster_gate_end(c);
        HT_HIP(c, le);
        if (gs != HT_OK) return gs;
    } else {
        HtProfScope ps(c, p.meanshift.timer);
        hipLaunchKernelGGL(k_cs_meanshift, dim3(p.meanshift.grid_x), dim3(p.meanshift.block), p.meanshift.lds, c->stream, frames, frame_stride, c->W, c->H, hist,
                           (int)p.nchunks, c->d_cs, first, calc_angles, c->dbg_cs_iters, p.region_cap, d_out);
        HT_HIP(c, hipGetLastError());
    }
    c->cs_last_hist = hist;
    c->cs_last_first = first, c->cs_last_n = n, c->cs_last_chunks = (int)p.nchunks;
    return HT_OK;
}

// The result ring of the enqueue-only track calls, for ht_camshift_track_batch and ht_camshift_track_pairs (`fn`, for the message).
// A call without `out` is enqueue-only; a synchronous call with nothing outstanding goes the same way and collects at once (*via_ring).
// *slot = the next free pinned slot on that route — refused when the ring does not hold n streams or is full —, nullptr on the copy-back
// route.  ht_cs_ring_commit counts the slot as outstanding once its completion (a mark or an event) has been enqueued.
ht_status ht_cs_ring_begin(ht_ctx *c, const char *fn, int32_t n, const ht_cs_trackobj *out, bool *via_ring, ht_ctx::HtCsSlot **slot) {
    *slot = nullptr;
    *via_ring = out && c->cs_sync_ring && c->cs_ring_count == 0 && n <= c->cs_ring_streams;
    if (out && !*via_ring) return HT_OK;
    if (n > c->cs_ring_streams) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": no result ring for this many streams (ht_camshift_reserve failed to allocate it)");
    if (c->cs_ring_count == ht_ctx::HT_CS_RING)
        return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": too many enqueue-only calls outstanding (collect with ht_camshift_track_collect)");
    *slot = &c->cs_ring[(c->cs_ring_head + c->cs_ring_count) % ht_ctx::HT_CS_RING];
    return HT_OK;
}
void ht_cs_ring_commit(ht_ctx *c, ht_ctx::HtCsSlot *slot, int32_t n) {
    slot->n = n;
    c->cs_ring_count++;
}

// the oldest outstanding call leaves the ring
static void cs_ring_pop(ht_ctx *c) {
    c->cs_ring_head = (c->cs_ring_head + 1) % ht_ctx::HT_CS_RING;
    c->cs_ring_count--;
}

// the copy-back route of a result read-back: `count` track objects and the error word, then the stream is synchronised and the word checked
ht_status ht_cs_read_back(ht_ctx *c, const char *fn, ht_cs_trackobj *out, const ht_cs_trackobj *d_src, size_t count) {
    HT_HIP(c, hipMemcpyAsync(out, d_src, sizeof(ht_cs_trackobj) * count, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipMemcpyAsync(c->h_cs_err, c->d_cs_err, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return ht_cs_check_err(c, fn);
}

extern "C" ht_status ht_camshift_track_batch(ht_ctx *c, int32_t first, int32_t n, int32_t calc_angles, ht_cs_trackobj *out) {
    HtRange range("ht_camshift_track_batch");
    if (!c) return HT_ERR_INVALID;
    if (!c->d_frames || n <= 0 || n > c->nframes) return ht_fail(c, HT_ERR_STATE, "ht_camshift_track_batch: bind n frames first");
    if (first < 0 || first + n > c->cs_streams) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_track_batch: stream range not reserved");
    if (c->W == 0 || c->H == 0) return HT_OK;  // camshift.js:219
    HT_HIP(c, hipSetDevice(c->device));
    // A synchronous call with nothing outstanding goes the same way as an enqueue-only call that is collected at once: the kernels write
    // the track objects into a pinned slot and mark it, the host polls the marks — no device-to-host copies (two copy kernels: objects and
    // the error word) and no stream synchronisation.  Wall clock of a single-stream track() call, round 6 (tools/gpu_cs_wall.py):
    // 41.4 -> 28.9 us at 320x240 (event-marked slot), 38.7 -> 20.7 us at 640x480 and 41.0 -> 22.6 us at 1920x1080 (kernel-marked slot).
    bool via_ring = false;
    ht_ctx::HtCsSlot *slot = nullptr;
    ht_status rs = ht_cs_ring_begin(c, "ht_camshift_track_batch", n, out, &via_ring, &slot);
    if (rs != HT_OK) return rs;
    if (slot) {  // enqueue only: results go straight to the next pinned slot, a mark or an event says they are complete
        ht_ctx::HtCsSlot &sl = *slot;
        bool flagged = false;
        uint32_t seq = 0;
        if (c->cs_flags && sl.h_flag) {
            seq = ++c->cs_flag_seq ? c->cs_flag_seq : ++c->cs_flag_seq;  // never 0
            for (int i = 0; i < n; i++) __atomic_store_n(&sl.h_flag[i], 0u, __ATOMIC_RELAXED);
        }
        ht_status st = launch_track(c, c->d_frames, c->frame_stride, first, n, calc_angles, sl.h_out, seq ? sl.h_flag : nullptr, seq, &flagged);
        if (st != HT_OK) return st;
        sl.seq = flagged ? seq : 0u;
        if (!flagged) HT_HIP(c, hipEventRecord(sl.ev, c->stream));
        ht_cs_ring_commit(c, slot, n);
        return via_ring ? ht_camshift_track_collect(c, n, out) : HT_OK;
    }
    ht_status st = launch_track(c, c->d_frames, c->frame_stride, first, n, calc_angles, c->d_cs_out);
    if (st != HT_OK) return st;
    return out ? ht_cs_read_back(c, "ht_camshift_track_batch", out, c->d_cs_out, (size_t)n) : HT_OK;
}

extern "C" ht_status ht_camshift_track_collect(ht_ctx *c, int32_t n, ht_cs_trackobj *out) {
    HtRange range("ht_camshift_track_collect");
    if (!c || !out || n <= 0) return HT_ERR_INVALID;
    if (c->cs_ring_count == 0 || c->cs_ring[c->cs_ring_head].n != n)
        return ht_fail(c, HT_ERR_STATE, "ht_camshift_track_collect: no enqueue-only ht_camshift_track_batch of n streams is pending");
    HT_HIP(c, hipSetDevice(c->device));
    ht_ctx::HtCsSlot &sl = c->cs_ring[c->cs_ring_head];
    if (sl.seq) {  // the kernel marks every stream's slot word; poll them (the OLDEST outstanding call; later ones keep running)
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; i++) {
            uint64_t spins = 0;
            while (__atomic_load_n(&sl.h_flag[i], __ATOMIC_ACQUIRE) != sl.seq) {
                if ((++spins & 0xfff) == 0) {  // not there after a while: is the stream still running at all?
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                        const hipError_t q = hipStreamQuery(c->stream);
                        if (q == hipSuccess) {
                            if (__atomic_load_n(&sl.h_flag[i], __ATOMIC_ACQUIRE) == sl.seq) break;
                            return ht_fail(c, HT_ERR_HIP, "ht_camshift_track_collect: the stream drained without the call's completion mark");
                        }
                        if (q != hipErrorNotReady) return ht_fail(c, HT_ERR_HIP, std::string("ht_camshift_track_collect: ") + hipGetErrorString(q));
                        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30))
                            return ht_fail(c, HT_ERR_HIP, "ht_camshift_track_collect: timed out waiting for the call's completion mark");
                    }
                }
            }
        }
    } else {
        HT_HIP(c, hipEventSynchronize(sl.ev));  // the OLDEST outstanding call; later ones keep running
    }
    std::memcpy(out, sl.h_out, sizeof(ht_cs_trackobj) * (size_t)n);
    cs_ring_pop(c);
    return ht_cs_check_err(c, "ht_camshift_track_collect");
}

extern "C" ht_status ht_camshift_track_sequence(ht_ctx *c, int32_t first, int32_t n, int32_t calc_angles, const void *const *dev_frames,
                                                int32_t ncalls, size_t frame_stride, ht_cs_trackobj *out, int32_t out_all) {
    HtRange range("ht_camshift_track_sequence");
    if (!c || !dev_frames) return HT_ERR_INVALID;
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_track_sequence: call ht_set_geometry first");
    if (n <= 0 || ncalls <= 0 || frame_stride < (size_t)c->W * c->H * 4 || (frame_stride & 3))
        return ht_fail(c, HT_ERR_INVALID, "ht_camshift_track_sequence: bad stream count, call count or frame stride");
    if (first < 0 || first + n > c->cs_streams) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_track_sequence: stream range not reserved");
    for (int k = 0; k < ncalls; k++)
        if (!dev_frames[k] || ((uintptr_t)dev_frames[k] & 3)) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_track_sequence: bad frame pointer");
    HT_HIP(c, hipSetDevice(c->device));
    const size_t need = (size_t)n * (size_t)(out_all ? ncalls : 1);
    ht_status gs = ht_grow_device(c, &c->d_cs_seq_out, &c->cs_seq_cap, need, "ht_camshift_track_sequence: hipMalloc failed");
    if (gs != HT_OK) return gs;
    // the calls of one stream are sequentially dependent (search window, camshift.js:257-258), the streams are not: 2 launches
    // per call on the context's stream, no host round trip in between
    if (ht_cs_takes_fused(n, c->cs_fused_min_streams) && c->cs_seq_fused) {
        // one launch per CS_SEQ_MAX calls: every workgroup walks its stream's calls on its own (see k_cs_track_fused)
        if (!c->cs_seq_attr_set) {
            HT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_cs_track_fused<true, FUSED_NT>), hipFuncAttributeMaxDynamicSharedMemorySize, CS_REGION_CAP * 2));
            c->cs_seq_attr_set = true;
        }
        const HtCsTrackPlan p = plan_track(c, n);  // the form is chosen once for the whole sequence
        for (int k0 = 0; k0 < ncalls; k0 += CS_SEQ_MAX) {
            ht_status st = launch_fused(c, p, true, dev_frames + k0, std::min(CS_SEQ_MAX, ncalls - k0), frame_stride, first, n, calc_angles,
                                        c->d_cs_seq_out + (out_all ? (size_t)k0 * n : 0), out_all ? (uint32_t)n : 0u);
            if (st != HT_OK) return st;
        }
    } else {
        for (int k = 0; k < ncalls; k++) {
            ht_cs_trackobj *d_out = c->d_cs_seq_out + (out_all ? (size_t)k * n : 0);
            ht_status st = launch_track(c, static_cast<const uint8_t *>(dev_frames[k]), frame_stride, first, n, calc_angles, d_out);
            if (st != HT_OK) return st;
        }
    }
    c->cs_seq_pending_n = 0;
    if (out) return ht_cs_read_back(c, "ht_camshift_track_sequence", out, c->d_cs_seq_out, need);
    c->cs_seq_pending_n = n, c->cs_seq_pending_calls = ncalls, c->cs_seq_pending_all = out_all ? 1 : 0;  // what ht_camshift_sequence_collect may fetch
    return HT_OK;
}

extern "C" ht_status ht_camshift_sequence_collect(ht_ctx *c, int32_t n, int32_t ncalls, int32_t out_all, ht_cs_trackobj *out) {
    if (!c || !out || n <= 0 || ncalls <= 0) return HT_ERR_INVALID;
    const size_t need = (size_t)n * (size_t)(out_all ? ncalls : 1);
    // only the sequence that was enqueued with out == NULL, with the layout it was enqueued with: anything else would read stale or
    // differently strided track objects
    if (!c->d_cs_seq_out || c->cs_seq_cap < need || c->cs_seq_pending_n != n || c->cs_seq_pending_calls != ncalls || c->cs_seq_pending_all != (out_all ? 1 : 0))
        return ht_fail(c, HT_ERR_STATE, "ht_camshift_sequence_collect: no enqueue-only sequence with this n / ncalls / out_all is pending");
    HT_HIP(c, hipSetDevice(c->device));
    const ht_status st = ht_cs_read_back(c, "ht_camshift_sequence_collect", out, c->d_cs_seq_out, need);
    if (st != HT_ERR_HIP) c->cs_seq_pending_n = 0;  // fetched, whatever the error word says; a failed copy leaves the sequence pending
    return st;
}

extern "C" ht_status ht_camshift_stats(ht_ctx *c, int32_t first, int32_t n, uint64_t *window_pixels, uint64_t *calls, int32_t reset) {
    if (!c || n <= 0 || first < 0 || first + n > c->cs_streams) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> v((size_t)n * 2);  // {win_px, calls} of every stream: one strided copy
    HT_HIP(c, hipMemcpy2D(v.data(), 16, &c->d_cs[first].win_px, sizeof(HtCsState), 16, (size_t)n, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        if (window_pixels) window_pixels[i] = v[2 * (size_t)i];
        if (calls) calls[i] = v[2 * (size_t)i + 1];
    }
    if (reset) HT_HIP(c, hipMemset2D(&c->d_cs[first].win_px, sizeof(HtCsState), 0, 16, (size_t)n));
    return HT_OK;
}

// current[4096] = the sum of the nchunks chunk histograms at d_hist (either layout: a stream's slot of d_cs_hist or a frame's of d_csp_hist)
static ht_status cs_sum_chunks(ht_ctx *c, const uint32_t *d_hist, int nchunks, uint32_t *current) {
    std::vector<uint32_t> part((size_t)nchunks * 4096);
    HT_HIP(c, hipMemcpy(part.data(), d_hist, part.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < 4096; b++) {
        uint32_t v = 0;
        for (int k = 0; k < nchunks; k++) v += part[(size_t)k * 4096 + b];
        current[b] = v;
    }
    return HT_OK;
}

extern "C" ht_status ht_camshift_debug_hist(ht_ctx *c, int32_t stream, uint32_t *model, uint32_t *current) {
    if (!c || stream < 0 || stream >= c->cs_streams) return HT_ERR_INVALID;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (model) HT_HIP(c, hipMemcpy(model, c->d_cs[stream].model, sizeof(uint32_t) * 4096, hipMemcpyDeviceToHost));
    if (current) {
        if (c->d_csp_hist && c->cs_last_hist == c->d_csp_hist) {  // the last track call was a pair call: the stream's frame has a slot of its own
            const int slot = stream < (int)c->cs_pair_slot.size() ? c->cs_pair_slot[stream] : -1;
            if (slot < 0 || c->cs_pair_chunks <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_debug_hist: the stream was not part of the last track call");
            return cs_sum_chunks(c, c->d_csp_hist + (size_t)slot * c->cs_pair_chunks * 4096, c->cs_pair_chunks, current);
        }
        if (stream < c->cs_last_first || stream >= c->cs_last_first + c->cs_last_n || c->cs_last_chunks <= 0 || !c->cs_last_hist)
            return ht_fail(c, HT_ERR_STATE, "ht_camshift_debug_hist: the stream was not part of the last track call");
        return cs_sum_chunks(c, c->cs_last_hist + (size_t)(stream - c->cs_last_first) * c->cs_last_chunks * 4096, c->cs_last_chunks, current);
    }
    return HT_OK;
}

// ht_cs_schedule.h — the host-side decisions of the camshift calls, without HIP: which schedule a track() call takes, the grid, block and
// dynamic LDS of each of its launches, the chunk plan of the full-frame histogram pass, the row split of initTracker, and the sizes of
// the buffers ht_camshift_reserve allocates.  ht_camshift.hip plans with these functions and launches what the plan says; the workgroup
// sizes and capacities the kernels are compiled with are defined here too, so plan and kernels cannot disagree.  Plain C++17: the CPU
// suite compiles this header alone (tests/host/cs_schedule_harness.cc) with AddressSanitizer + UBSan and checks the decision table.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "headtrackr_hip.h"

// ---- what the kernels are compiled with ---------------------------------------------------------------------------------------------------
constexpr int CS_NT = 512;          // threads of the mean-shift workgroup
constexpr int HIST_NT = 1024;
constexpr int INIT_NT = 1024;   // threads of the one-workgroup-per-stream initTracker (k_cs_init)
constexpr int CS_INIT_ROWS_NT = 256, CS_LUT_NT = 512;  // k_cs_init_rows, k_cs_lut

constexpr int CS_REGION_CAP = 40960;  // pixels of the cached search region: 80 KB of LDS next to the 32 KB LUT (which the 16 KB histogram overlays)

// One launch per track() call when there are enough streams to fill the chip by themselves (k_cs_track_fused): ONE 1024-thread workgroup
// per stream.
constexpr int FUSED_NT = 1024;
// The 1024-thread form owns its CU: 112 KB of LDS and 16 wavefronts x 122 VGPRs leave no room for anything else, so the track launches
// of several contexts (and the detect kernels of their next batches) run strictly one after the other although a call is a bandwidth
// phase (the frame streams through the histogram) followed by a latency phase (<= 10 dependent moment passes from LDS).  The
// 512-thread form (round 5) is half of it — 8 wavefronts, <= 128 VGPRs, a 44 KB region: 77 KB of LDS — so TWO workgroups share a CU,
// normally at different phases of their calls, or a workgroup shares it with another batch's detect kernels.  Its wavefronts play the
// 16 of the large form in window_moments, so both forms return the same bits.  Chosen per launch (ht_cs_fused_form below): more streams
// than CUs, or more than one context of the device on this path.
constexpr int FUSED_NT_SMALL = 512;
constexpr int CS_REGION_CAP_SMALL = 22528;  // 44 KB: a 118 x 118 search window + 16 px of margin, or 150 x 150 without

// the cluster mean-shift (k_cs_meanshift_cluster): threads, workgroups per stream at most, exchange slots per stream
constexpr int CL_NT = 512, CL_MAXG = 32, CL_SLOTS = 12;  // <= 11 moment passes per call (camshift.js:284-306)
constexpr int CL_MAX_STREAMS = 64;                       // the cluster path is only taken for <= 64 streams per call

// camshift per-stream device state (camshift.js:153-160)
struct alignas(16) HtCsState {
    uint32_t model[4096];  // _modelHist
    int32_t sw[4];         // _searchWindow
    double x, y, width, height, angle;  // _trackObj
    unsigned long long win_px;          // measurement: pixels visited by the window moment passes since the last reset
    unsigned long long calls;           // measurement: track() calls since the last reset
};

// ---- the chunk plan of the full-frame histogram pass (k_cs_hist, k_csp_hist) ----------------------------------------------------------------
// Partial histograms per stream: enough chunks to put ~256 workgroups of 1024 threads on the chip (a single 1080p stream gets 127,
// eight of them 32 each, a batch of >= 32 streams 8 each), each chunk >= 16384 pixels and a multiple of 4 * HIST_NT.  Round 5, same box,
// the C5 track step of 8 / 1 feeds (tools/gpu_cs_step.py): 256 threads x ~1024 workgroups 39.1 / 27.8 us, 512 x 512: 36.5 / 24.6,
// 1024 x 512: 36.4 / 24.2, 1024 x 256: 35.8 / 24.0 (a quarter of the chunk histograms to write and to sum), 8 loads in flight per
// thread instead of 4: 39.4 / 26.8.
constexpr int HIST_MAXCHUNKS = 128;
constexpr int HIST_TARGET_WGS = 256;  // workgroups of a k_cs_hist launch, all streams together
inline uint32_t hist_max_chunks(int nstreams) { return (uint32_t)std::min(HIST_MAXCHUNKS, std::max(8, HIST_TARGET_WGS / std::max(nstreams, 1))); }
inline void hist_chunks(uint32_t npix, uint32_t max_chunks, uint32_t *chunk_px, uint32_t *nchunks) {
    uint32_t n = std::min<uint32_t>((npix + 16383u) / 16384u, max_chunks);
    n = std::max<uint32_t>(n, 1u);
    const uint32_t q = 4u * HIST_NT;
    *chunk_px = std::max<uint32_t>(((npix + n - 1) / n + q - 1) / q * q, q);
    *nchunks = std::max<uint32_t>((npix + *chunk_px - 1) / *chunk_px, 1u);
}
// the plan for a call (or a reservation) of nstreams frames
inline void ht_cs_hist_plan(uint32_t npix, int nstreams, uint32_t *chunk_px, uint32_t *nchunks) { hist_chunks(npix, hist_max_chunks(nstreams), chunk_px, nchunks); }

// ---- track(): one of three schedules ------------------------------------------------------------------------------------------------------
enum HtCsForm {
    HT_CS_FUSED_1024,  // k_cs_track_fused, one 1024-thread workgroup per stream
    HT_CS_FUSED_512,   // ... its 512-thread form
    HT_CS_CLUSTER,     // k_cs_hist + k_cs_lut + k_cs_meanshift_cluster: G workgroups per stream
    HT_CS_PER_STREAM   // k_cs_hist + k_cs_meanshift: one workgroup per stream
};
struct HtCsLaunch {
    uint32_t grid_x = 0, grid_y = 1, block = 0;  // block == 0: the form does not launch this kernel
    size_t lds = 0;                              // dynamic LDS bytes
    const char *timer = nullptr;                 // name of the profiling timer
};
struct HtCsTrackIn {
    int n = 0;           // streams of the call
    int cs_streams = 0;  // streams reserved (sizes the chunk histograms)
    int W = 0, H = 0, num_cus = 256;
    int cs_fused_min_streams = 192;
    bool cs_cluster = true;
    uint32_t cs_cluster_min_px = 10000;
    int dbg_cs_iters = 10, cs_region_cap = CS_REGION_CAP;
    int fused_nt = 0;  // FUSED_NT / FUSED_NT_SMALL from ht_cs_fused_form when ht_cs_takes_fused(n, cs_fused_min_streams); otherwise unused
};
struct HtCsTrackPlan {
    HtCsForm form = HT_CS_PER_STREAM;
    HtCsLaunch fused, hist, lut, meanshift;
    uint32_t npix = 0, chunk_px = 0, nchunks = 0;
    int G = 0;           // workgroups per stream of the cluster form
    int region_cap = 0;  // pixels of the LDS-cached search region the mean-shift launch is given
};

// enough streams to keep (most of) the 256 CUs busy with one workgroup each: the fused single-launch kernel; fewer streams (a handful of
// large feeds): chunk histograms from every CU, then the mean-shift launch
inline bool ht_cs_takes_fused(int n, int cs_fused_min_streams) { return n >= cs_fused_min_streams; }

// Threads per workgroup of k_cs_track_fused for a launch of n streams: option cs_fused_nt (`forced_nt`), else the small form when the
// launch has more workgroups than the device has CUs (all of them resident at once, two per CU) or when ANOTHER live context of the
// device that uses this path has work in flight right now (`other_busy`, found by ht_camshift.hip's fused_threads) — its track launch, or
// the detect kernels of its next batch, then share the CUs with this launch instead of queueing behind it —, else the large form (one
// stream per CU with the whole CU to itself: the lowest latency, and the right choice whenever nothing else wants the chip: measured on
// C3 with TWO steps in flight, where a context's track launch never meets the other's, the small form costs 18 %).  Both forms return the
// same bits.
inline bool ht_cs_fused_form_forced(int forced_nt) { return forced_nt == FUSED_NT || forced_nt == FUSED_NT_SMALL; }
inline int ht_cs_fused_form(int forced_nt, int n, int num_cus, bool other_busy) {
    if (ht_cs_fused_form_forced(forced_nt)) return forced_nt;
    return (n > num_cus || other_busy) ? FUSED_NT_SMALL : FUSED_NT;
}

inline HtCsTrackPlan ht_cs_plan_track(const HtCsTrackIn &in) {
    HtCsTrackPlan p;
    const int n = in.n;
    p.npix = (uint32_t)((size_t)in.W * in.H);
    if (ht_cs_takes_fused(n, in.cs_fused_min_streams)) {
        const bool small = in.fused_nt == FUSED_NT_SMALL;
        p.form = small ? HT_CS_FUSED_512 : HT_CS_FUSED_1024;
        p.fused.grid_x = (uint32_t)n, p.fused.block = small ? FUSED_NT_SMALL : FUSED_NT;
        p.fused.lds = (size_t)(small ? CS_REGION_CAP_SMALL : CS_REGION_CAP) * 2;
        p.fused.timer = small ? "cs_track_512" : "cs_track";  // the timer's name tells the form
        p.region_cap = small ? std::min(in.cs_region_cap, CS_REGION_CAP_SMALL) : in.cs_region_cap;
        return p;
    }
    hist_chunks(p.npix, hist_max_chunks(in.cs_streams), &p.chunk_px, &p.nchunks);  // buffer sized for cs_streams x that many chunks
    // a few large frames: G workgroups per stream share every moment pass (k_cs_meanshift_cluster); otherwise one workgroup per stream
    // cluster size: the grid never exceeds one workgroup per CU of THIS device, so it is co-resident whatever else is resident
    // (a CU has room for four of these workgroups); fewer than 4 workgroups per stream are not worth the barriers
    p.G = std::min(CL_MAXG, in.num_cus / std::max(n, 1));
    const bool cluster = in.cs_cluster && n <= CL_MAX_STREAMS && p.G >= 4 && p.npix >= in.cs_cluster_min_px && in.dbg_cs_iters > 0;
    p.form = cluster ? HT_CS_CLUSTER : HT_CS_PER_STREAM;
    p.hist.grid_x = p.nchunks, p.hist.grid_y = (uint32_t)n, p.hist.block = HIST_NT, p.hist.timer = "cs_hist";
    p.meanshift.timer = "cs_meanshift";
    if (cluster) {
        p.lut.grid_x = 64, p.lut.grid_y = (uint32_t)n, p.lut.block = CS_LUT_NT, p.lut.timer = "cs_lut";
        p.meanshift.grid_x = (uint32_t)(n * p.G), p.meanshift.block = CL_NT;
    } else {
        p.meanshift.grid_x = (uint32_t)n, p.meanshift.block = CS_NT, p.meanshift.lds = (size_t)CS_REGION_CAP * 2;
        p.region_cap = in.cs_region_cap;
    }
    return p;
}

// ---- track() of (stream, frame) pairs (ht_camshift_track_pairs): one of two schedules --------------------------------------------------------
// n pairs on nd distinct bound frames.  The chunk histograms are per DISTINCT frame (k_csp_hist), so the chunk plan follows nd; the
// mean-shift is per pair.  The cluster form (option cs_pairs_cluster) is ht_cs_plan_track's cluster rule with n = pairs.
enum HtCspForm {
    HT_CSP_PER_PAIR,  // k_csp_hist + k_csp_meanshift: one workgroup per pair
    HT_CSP_CLUSTER    // k_csp_hist + k_csp_lut + k_csp_meanshift_cluster: G workgroups per pair
};
struct HtCspTrackIn {
    int n = 0, nd = 0;  // pairs, distinct frames
    int W = 0, H = 0, num_cus = 256;
    bool cs_pairs_cluster = false, cs_cluster = true;
    uint32_t cs_cluster_min_px = 10000;
    int dbg_cs_iters = 10, cs_region_cap = CS_REGION_CAP;
};
struct HtCspTrackPlan {
    HtCspForm form = HT_CSP_PER_PAIR;
    HtCsLaunch hist, lut, meanshift;
    uint32_t npix = 0, chunk_px = 0, nchunks = 0;
    int G = 0;           // workgroups per pair of the cluster form
    int region_cap = 0;  // pixels of the LDS-cached search region (one-workgroup form)
};
inline HtCspTrackPlan ht_cs_plan_track_pairs(const HtCspTrackIn &in) {
    HtCspTrackPlan p;
    const int n = in.n;
    p.npix = (uint32_t)((size_t)in.W * in.H);
    ht_cs_hist_plan(p.npix, in.nd, &p.chunk_px, &p.nchunks);
    p.hist.grid_x = p.nchunks, p.hist.grid_y = (uint32_t)in.nd, p.hist.block = HIST_NT, p.hist.timer = "csp_hist";
    // the grid n * G never exceeds one workgroup per CU: co-resident whatever else is resident (see ht_cs_plan_track)
    p.G = std::min(CL_MAXG, in.num_cus / std::max(n, 1));
    const bool cluster = in.cs_pairs_cluster && in.cs_cluster && n <= CL_MAX_STREAMS && p.G >= 4 && p.npix >= in.cs_cluster_min_px && in.dbg_cs_iters > 0;
    if (cluster) {
        p.form = HT_CSP_CLUSTER;
        p.lut.grid_x = 64, p.lut.grid_y = (uint32_t)n, p.lut.block = CS_LUT_NT, p.lut.timer = "csp_lut";
        p.meanshift.grid_x = (uint32_t)(n * p.G), p.meanshift.block = CL_NT, p.meanshift.timer = "csp_meanshift_cluster";
    } else {
        p.meanshift.grid_x = (uint32_t)n, p.meanshift.block = CS_NT, p.meanshift.lds = (size_t)CS_REGION_CAP * 2, p.meanshift.timer = "csp_meanshift";
        p.region_cap = in.cs_region_cap;
    }
    return p;
}

// ---- initTracker --------------------------------------------------------------------------------------------------------------------------
// few streams with tall rects: rows spread over G workgroups per stream (k_cs_init_rows; one workgroup per stream would leave the chip
// idle), otherwise one workgroup per stream (k_cs_init)
struct HtCsInitPlan {
    bool rows = false;
    int G = 1;
};
inline HtCsInitPlan ht_cs_plan_init(int n, int max_rect_height, int num_cus) {
    HtCsInitPlan p;
    p.G = std::min(std::min(32, std::max(1, num_cus * 2 / std::max(n, 1))), (max_rect_height + 15) / 16);
    p.rows = n < 64 && p.G >= 2;
    return p;
}
// ht_camshift_init_pairs: the row form only under option cs_pairs_cluster (k_csp_init_rows), otherwise one workgroup per pair (k_csp_init)
inline HtCsInitPlan ht_cs_plan_init_pairs(bool cs_pairs_cluster, int n, int max_rect_height, int num_cus) {
    HtCsInitPlan p = ht_cs_plan_init(n, max_rect_height, num_cus);
    if (!cs_pairs_cluster) p.rows = false;
    if (!p.rows) p.G = 1;
    return p;
}

// ---- ht_camshift_reserve: bytes of every buffer it allocates --------------------------------------------------------------------------------
struct HtCsReserveSizes {
    size_t states;      // d_cs: tracker state per stream
    size_t hist;        // d_cs_hist: hist_max_chunks(nstreams) chunk histograms per stream
    size_t out;         // d_cs_out: a track object per stream
    size_t lut, parts;  // cluster mean-shift (few large streams): per stream a LUT and CL_SLOTS x CL_MAXG partial-sum slots
    size_t err_word;    // d_cs_err, h_cs_err, h_cs_err_direct
    size_t ring_out, ring_flags;  // per slot of the result ring (pinned): a track object and a completion word per stream
};
inline HtCsReserveSizes ht_cs_reserve_sizes(int nstreams) {
    const size_t ns = (size_t)nstreams, ncl = (size_t)std::min(nstreams, CL_MAX_STREAMS);
    HtCsReserveSizes s;
    s.states = sizeof(HtCsState) * ns;
    s.hist = sizeof(uint32_t) * 4096 * hist_max_chunks(nstreams) * ns;
    s.out = sizeof(ht_cs_trackobj) * ns;
    s.lut = sizeof(double) * 4096 * ncl;
    s.parts = sizeof(double) * CL_SLOTS * CL_MAXG * 6 * ncl;
    s.err_word = sizeof(uint32_t);
    s.ring_out = sizeof(ht_cs_trackobj) * ns;
    s.ring_flags = sizeof(uint32_t) * ns;
    return s;
}

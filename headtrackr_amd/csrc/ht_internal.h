// ht_internal.h — shared host/device definitions of libheadtrackr_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <vector>

#include "headtrackr_hip.h"

// ---------------------------------------------------------------------------------------------------------
// The cascade's records (the "HTCB" blob's rows, the device-side feature and stage tables), the LDS layout constants their offsets address
// and the plan that holds them live in a header without HIP, shared with the host-only planner (ht_cascade_plan.h).
#include "ht_cascade_types.h"

// ---------------------------------------------------------------------------------------------------------
// The plain records of a geometry's plan (levels, resample jobs / tile records, taps, tail generations, scan scales and tile records)
// live in a header without HIP, shared with the host-only planner (ht_geometry_plan.h).
#include "ht_plan_types.h"

constexpr int HT_TAIL_LDS_TAPS = 4096;  // compact taps of one generation kept in LDS by k_resample_tail (32 KB)

// Direct block -> work lookup (one 8-byte load per workgroup instead of a serial scan over a prefix table).
struct HtBlockRef {
    uint16_t item;  // resample: job index in the generation; scan: index into the scale table
    uint16_t bx, by;  // tile column / row (resample: by = first 16-row pass of the tile)
    uint16_t pad;     // resample: number of 16-row passes in this tile; scan: unused
};

// Survivor handed from the tile kernel to the deep kernel.  The tile kernel holds the scale's plane offsets and strides in scalar
// registers (its tile record), so the entry carries the window's three plane origins ready-made: the deep kernel used to look the
// scale's three level records up behind the entry — a third dependent memory round trip in front of every window's patch load.
struct alignas(16) HtQueueEntry {
    uint32_t frame;
    uint16_t x, y;
    uint8_t scale, q;
    uint16_t stage;        // first stage the deep kernel has to run
    uint32_t o0, o1, o2;   // byte offsets of the window origin inside the frame's arena: level i (ccv.js:180,235), i + 6 (236), variant q of i + 12 (237)
    uint16_t s0, s1, s2;   // row strides of the three planes
    uint16_t pad;
};
static_assert(sizeof(HtQueueEntry) == 32, "HtQueueEntry");

// k_scan_deep_lds hands its queue entries out through HT_DEEP_CTRS counters, one per 256-byte line, in the 4 KB behind the queue's
// last entry (zeroed by the first workgroup of every k_scan_tiles launch): same-address atomics retire at ~90 per us, one counter for
// the 6 103 windows of a C2 batch made the launch 0.10 ms long whatever the grid.
#define HT_DEEP_CTRS 16
#define HT_DEEP_CTR_BYTES (HT_DEEP_CTRS * 256)
#define HT_PINNED_HITS 8192
#define HT_STAT_SHARDS 256  // rows of 64 u64 counters; a workgroup adds to row (blockIdx & 255)

// Device counters block (zeroed before each batch).
struct HtCounters {
    uint32_t nhits;        // hits appended (may exceed capacity)
    uint32_t nqueue;       // survivors appended to the deep queue (may exceed capacity)
    uint32_t queue_inline; // survivors that did not fit the queue and were finished inside the tile kernel
    uint32_t pad;
};

// The camshift launch constants, the per-stream device state (HtCsState) and the host-side schedule of the camshift calls live in a header
// without HIP as well, shared with the CPU suite's harness.
#include "ht_cs_schedule.h"

// A context's published frame binding (HtFrameSlot) and the process-wide registry of them: plain C++ too, shared with the CPU suite's harness.
#include "ht_frame_registry.h"

// A captured detect sequence (memsets + gray + pyramid generations + scan kernels: ~10 dependent launches) replayed with one
// hipGraphLaunch.  Keyed by everything the kernels' arguments depend on besides the geometry (which owns the cache).
// INVARIANT: a captured graph bakes in d_arena, d_counters, d_hits, d_queue, d_stats, the tile / job tables and d_scratch.  The first
// four live as long as the context; the geometry's allocations are only freed by free_geometry(), d_scratch only by wb_scratch() — both
// call destroy_graphs() first.  Anything else that reallocates a buffer a detect kernel reads must do the same.
struct HtDetectGraph {
    const uint8_t *frames = nullptr;
    size_t frame_stride = 0;
    int nframes = 0;
    uint32_t flags = 0;
    int seen = 0;                  // plain enqueues of this key so far (the sequence is captured on the second one)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

// ---------------------------------------------------------------------------------------------------------
// A call's table on its way to the device: ONE device table and a ring of HT_STAGE_SLOTS pinned slots, each with an event.  A call takes
// the next slot (waiting for the event behind that slot's previous copy), fills it, and commits: one hipMemcpyAsync on the context's stream
// and the event behind it.  Copy and kernel are ordered on the stream, so a later call's table cannot reach the device before an earlier
// call's kernel has read its own.  The draw list, the crop calls, the align calls and the camshift pair calls each have one
// (ht_stage_reserve / _take / _commit / _free below; the arithmetic is ht_stage_plan.h).
#include "ht_stage_plan.h"
struct HtStagedTable {
    uint8_t *d = nullptr;                  // the device table
    uint8_t *h[HT_STAGE_SLOTS] = {};       // the pinned slots
    hipEvent_t ev[HT_STAGE_SLOTS] = {};    // a slot's copy has left it
    size_t cap = 0;                        // bytes the table and every slot hold
    int next = 0, taken = 0;               // the slot the next call takes; the slot taken last (what commit copies)
};

// The buffers of one family of face-patch calls (crop, align): the descriptor table, the records of the last call on the device and in
// a pinned twin the call copies them to; the event behind that copy is what ht_camshift_*_result waits for
struct HtFaceCalls {
    HtStagedTable tab;
    uint8_t *d_rec = nullptr, *h_rec = nullptr;
    size_t rec_cap = 0;       // records both hold
    hipEvent_t ev = nullptr;
    int n = 0;                // entries of the last call (0: none, or its record copy is not enqueued yet)
};

struct HtKernelTimer {
    std::string name;
    double ms = 0;
    uint32_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct ht_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // early scan (opt-in, option early_scan=1): the scales whose three planes exist after pyramid generation `early_gen` are
    // scanned on a second stream while the main stream builds the remaining (small, latency-bound) generations.  Measured with
    // 3 batches in flight: +2.5 % at 128 x 720p, -12 % at 256 x 320x240 (the other batches already fill those gaps; the extra
    // concurrency only adds contention), so it is off by default; it shortens the latency of a single batch in flight.
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_early_ready = nullptr, ev_early_done = nullptr;
    bool early_scan = false;
    bool early_launched = false;   // this batch's early part was launched (ht_launch_scan then only does the rest)
    std::string err;

    // cascade
    int interval = 5, next = 6;
    HtCascadePlan cascade;  // the host side of the cascade (ht_cascade_types.h), planned by ht_plan_cascade / ht_plan_cascade_split; below: its tables on the device
    HtTileFeature *d_tile_feats = nullptr;
    HtDeepFeature *d_deep_feats = nullptr;
    HtPatchFeature *d_patch_feats = nullptr;
    HtPackedFeature *d_packed_feats = nullptr;  // cascade.packed (nullptr: empty)
    HtPackedFeature *d_fp_feats = nullptr;      // cascade.fp (nullptr: empty)
    bool fp_sparse = true;  // option fp_sparse=0: the sparse stages always run as four feature slices (A/B)
    bool builtin_cascade = false;  // blob == the cascade ht_cascade_gen.inc was generated from
    uint32_t deep_bias = 1;        // tile kernel hands survivors to the deep kernel when n*bias*ceil(count/64) <= count
                                   // (measured on C2/C4: split 8 + bias 0..1 is the optimum, profiles/r01_sweeps.txt)
    int dbg_stop_stage = -1, dbg_force_exact = 0, dbg_deep_v = 4, deep_grid = 192;  // ht_config.options, parsed once in ht_create
    HtDevStage *d_stages = nullptr;
    int opt_split = 0;         // option split (0 = default)

    // geometry
    int W = 0, H = 0, max_batch = 0, nlevels = 0, upto = 0;
    HtGeometryPlan plan;  // the host side of the geometry (ht_plan_types.h), planned by ht_plan_geometry; below: its tables on the device
    HtDevLevel *d_levels = nullptr;
    uint8_t *d_arena = nullptr;
    std::vector<HtResampleJob *> d_gen_blocks;  // plan.gen_tiles
    HtTileRec *d_tile_recs = nullptr;
    HtScanScale *d_scales = nullptr;
    HtResampleJob *d_tail_jobs = nullptr;
    uint32_t *d_tail_prefix = nullptr;
    HtTap *d_tail_taps = nullptr;
    HtTapFast *d_tail_taps_fast = nullptr;
    HtTailTapRef *d_tail_tapref = nullptr;
    bool deep_attr_set = false;              // k_scan_deep_lds: > 64 KB dynamic LDS enabled on this context's device
    int tail_table = 1;  // option rs_tailtable: the tail form (plan.tail_table) ...
    bool tail_table_forced = false;  // ... when the option was given: the plan keeps it instead of choosing by batch size
    bool rs_nofast = false, rs_nosort = false, rs_notail = false, rs_gennames = false;  // options of the same names (A/B, cross-checks)
    uint64_t rs_tailcap = 32768;     // destination pixels per frame the tail kernel takes at most (option rs_tailcap; batches <= 48 frames: 4 000 unless the option is given)
    bool rs_tailcap_forced = false;
    int rs_maxgen = 1 << 30;         // HT_DEBUG_KNOBS builds only (results stale): pyramid generations built
    bool force_rccl = false;         // option force_rccl: ht_allgather_* runs RCCL even with one rank
    int host_threads = -1;           // option host_threads: workers of the host post-processing (-1 = auto, 0 = none)
    int rs_min_wgs = 1536;  // ... but never fewer workgroups per launch than this (option rs_minwg; round 4, three batches in flight at C2: 1024 / 1536 / 2048 / 4096 -> 0.2288 / 0.2283 / 0.2303 / 0.2365 ms per step)
    int dbg_rs_k = 0;  // option rs_k: frames per k_resample workgroup, forced (any value)
    int rs_group = 8;  // pyramid generation kernels: frames per workgroup at most (option rs_group).  Frames of >= 400 k pixels take 4 unless the option is
                       // given: with k_resample_bands at 128 x 720p, K = 8 / 4 / 3 / 2 / 1 -> resample 0.480 / 0.456 / 0.455 / 0.465 / 0.529 ms per step,
                       // wall (two in flight) 1.1114 / 1.1040 / 1.1103 / 1.1295 / 1.2585; at 256 x 320x240 8 stays best (wall 0.2184 vs 0.2218)
    bool rs_group_forced = false;
    int rs_rpt = 4;  // k_resample: destination rows per thread (tile = 64 x 16*rs_rpt)
    bool rs_bands = true;  // option rs_bands=0: the pyramid generations run k_resample (register-staged tile, two barriers per frame) instead of k_resample_bands (A/B)

    // frames
    uint8_t *d_frames_own = nullptr;
    size_t d_frames_own_bytes = 0;
    uint8_t *d_frames_back = nullptr;  // ht_upload_frames_async target; ht_swap_frames exchanges it with d_frames_own
    size_t d_frames_back_bytes = 0;
    int back_n = 0;                    // frames in the back buffer (0 = nothing pending)
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copy_done = nullptr, ev_front_free = nullptr;
    // the binding: written by ht_frames_set (ht_frames.hip) and by nothing else, read by this context's own calls.  What OTHER contexts'
    // threads may see of it is the copy ht_frames_set publishes in frame_slot (ht_frame_registry.h)
    const uint8_t *d_frames = nullptr;
    size_t frame_stride = 0;
    int nframes = 0;
    HtFrameSlot frame_slot;
    // small batches (a live feed = 1 frame) are launch-bound: ~10 dependent launches cost more than their kernels.  Their sequence is
    // captured into a hipGraph per (frames pointer, count, flags) and replayed.  0 disables (option graph_max_frames)
    // set (under the cluster gate's lock: ht_capture_mark) while this context's stream is between hipStreamBeginCapture and EndCapture:
    // another context's fused_threads() must not hipStreamQuery a capturing stream (the query fails and may invalidate the capture)
    std::atomic<bool> capturing{false};
    int graph_max_frames = 256;  // round 4: replaying a 256-frame C2 batch instead of launching its 9 kernels: 0.2253 -> 0.2239 ms per step at three in flight (16 until then: only launch-bound small batches)
    std::vector<HtDetectGraph> graphs;
    uint64_t graph_launches = 0;  // measurement: enqueues served by a graph replay
    int enq_nframes = 0;  // frames of the batch enqueued last (what ht_detect_collect reports on)

    // scan outputs
    uint32_t hit_capacity = 1u << 20, queue_capacity_cfg = 0;
    ht_hit *d_hits = nullptr;
    HtQueueEntry *d_queue = nullptr;
    HtCounters *d_counters = nullptr;   // device block [HtCounters][hit_capacity x ht_hit]: d_hits points behind the counters
    uint32_t spec_hint = 0;             // raw hits of the batch collected last (sizes the next speculative read-back)
    HtCounters h_counters;
    uint8_t *h_pinned = nullptr;  // pinned staging: [HtCounters][HT_PINNED_HITS x ht_hit], one D2H + one sync per batch
    unsigned long long *d_stats = nullptr;      // [HT_STAT_SHARDS][64], only touched with HT_SCAN_STATS
    unsigned long long h_stage_in[64] = {0};   // windows that entered stage j ([nstages] = full survivors), last collected batch
    std::vector<ht_hit> h_collect_hits;        // ht_detect_collect_best: sorted raw hits of the last batch
    std::vector<uint32_t> h_collect_counts;    // ... and their per-frame counts
    std::vector<ht_hit> h_raw_hits;            // ht_detect_collect: the batch's raw hits in arrival order (scratch, kept between calls)
    std::vector<ht_hit> h_ordered_hits;        // ... and in emission order when the caller's buffer cannot take them directly
    std::vector<uint32_t> h_frame_start;       // ... bucket offsets of the counting sort by frame
    bool stats_enqueued = false;
    bool enqueued = false;

    // whitebalance / grayscale scratch
    double *d_scratch = nullptr;
    size_t d_scratch_bytes = 0;
    bool wb_fused = false;     // set around ht_launch_pyramid: the gray kernel also accumulates the channel sums into d_scratch
    bool wb_enqueued = false;  // the batch enqueued last carried HT_DETECT_WHITEBALANCE: ht_detect_collect snapshots its sums
    // d_scratch holds two regions of 4 u64 per frame: [0, max_batch) the sums of the batch in flight (fused gray pass),
    // [max_batch, 2 max_batch) the stand-alone ht_whitebalance_batch — so neither can zero the other's sums
    unsigned long long *h_wb_pinned = nullptr;       // pinned staging of the in-flight batch's sums (copied with the counters)
    size_t h_wb_pinned_bytes = 0;
    std::vector<unsigned long long> h_wb_sums;       // channel sums of the batch COLLECTED last (what ht_detect_whitebalance reports)
    int wb_collected_n = -1;                         // frames in h_wb_sums; -1: the collected batch carried no HT_DETECT_WHITEBALANCE

    // camshift
    int cs_streams = 0;
    HtCsState *d_cs = nullptr;
    uint32_t *d_cs_hist = nullptr;  // per-stream current-frame histogram (4096 bins)
    ht_cs_trackobj *d_cs_out = nullptr;
    double *d_cs_lut = nullptr, *d_cs_parts = nullptr;  // cluster mean-shift: per-stream weight LUT, partial-sum exchange slots
    bool cs_cluster = true;                              // option cs_cluster=0 disables the cluster path
    uint32_t cs_cluster_min_px = 10000;                  // frames at least this large take it (option cs_cluster_min_px).  Round 6, rocprofv3 kernel trace of
                                                         // track() calls in turn (tools/gpu_cs_one_stream_trace.sh), device us per call, cluster / one workgroup per
                                                         // stream: 320x240 x 1: 19.1 / 19.1, x 8: 20.0 / 20.6; 480x360 x 1: 18.6 / 24.7, x 16: 20.5 / 29.8; 640x480 x 1:
                                                         // 20.8 / 31.2, x 8: 20.5 / 35.1; 1280x720 x 8: 22.4 / 40.9 — and its calls are completed by marks in the pinned
                                                         // slot instead of an event: wall per synchronous call at 320x240 21.5 / 30.2 us (tools/gpu_cs_wall.py).  The
                                                         // threshold was 400 k pixels until then: VGA and the reference's own 320x240 canvas took the slower path
    ht_cs_trackobj *d_cs_seq_out = nullptr;  // ht_camshift_track_sequence: [calls][streams] results, one D2H at the end
    size_t cs_seq_cap = 0;
    // the sequence enqueued with out == NULL that ht_camshift_sequence_collect may fetch (n == 0: none pending)
    int cs_seq_pending_n = 0, cs_seq_pending_calls = 0, cs_seq_pending_all = 0;
    // enqueue-only track calls (ht_camshift_track_batch with out == NULL): the kernels write their track objects straight into a pinned
    // host slot of this ring, an event marks the slot complete; ht_camshift_track_collect takes the oldest.  Up to HT_CS_RING calls may be
    // outstanding, so a streaming host enqueues step i + 1 before it waits for step i.
    static constexpr int HT_CS_RING = 4;
    struct HtCsSlot {
        ht_cs_trackobj *h_out = nullptr;  // pinned, cs_ring_streams objects
        hipEvent_t ev = nullptr;
        int n = 0;
        // completion without an event (option cs_flags, cluster path): the kernel stores `seq` into h_flag[stream] (pinned, system scope,
        // after the stream's track object); the collect call polls the n words.  An event record is a barrier packet of its own on the
        // stream — two of them per step (this one and the cluster gate's) were the 10 us between a step's last and the next step's
        // first kernel (rocprofv3 kernel trace, LABLOG.md round 5).
        uint32_t *h_flag = nullptr;
        uint32_t seq = 0;  // 0: this slot's call is marked by the event
    };
    ht_cs_rect *h_cs_rects = nullptr;  // pinned staging of ht_camshift_init_batch's rects
    int h_cs_rects_cap = 0;
    hipEvent_t ev_cs_rects = nullptr;  // its copy to the device has been issued and completed
    uint32_t cs_flag_seq = 0;
    bool cs_flags = true;
    bool cs_sync_ring = true;  // option cs_sync_ring=0: a synchronous track call copies its results back and synchronises the stream (A/B)
    HtCsSlot cs_ring[HT_CS_RING];
    int cs_ring_head = 0, cs_ring_count = 0, cs_ring_streams = 0;
    uint32_t *h_cs_err_direct = nullptr;  // pinned word the cluster kernel itself sets when a barrier times out (read with a ring slot: no copy)
    uint32_t *d_cs_err = nullptr;      // device word: a cluster barrier ran out of its cycle budget (k_cs_meanshift_cluster)
    uint32_t *h_cs_err = nullptr;      // pinned copy, fetched with every result read-back
    long long cs_barrier_budget = 1ll << 28;  // shader-clock cycles a workgroup waits at one cluster barrier (option cs_barrier_budget)
    int num_cus = 256;                 // hipDeviceProp_t::multiProcessorCount: sizes the cluster of k_cs_meanshift_cluster
    uint32_t cs_fused_launches[2] = {0, 0};  // k_cs_track_fused launches in the 1024- / 512-thread form since the last ht_kernel_times(reset): reported there as
                                            // the pseudo-timers cs_fused_launches_1024 / _512 (ms = 0), profiling on or off
    int cs_fused_nt = 0;             // option cs_fused_nt=512|1024: threads per workgroup of k_cs_track_fused (0: chosen per launch, ht_cs_fused_form)
    int cs_fused_min_streams = 192;  // >= this many streams per call: k_cs_track_fused (option cs_fused_min)
    bool cs_seq_attr_set = false;
    bool cs_seq_fused = true;      // option cs_seq_fused=0: ht_camshift_track_sequence launches one kernel per call (A/B)
    int dbg_cs_iters = 10;            // option cs_iters: mean-shift iterations at most (camshift.js:284 has 10; anything else = wrong results)
    bool cs_keep_hist = false;
    bool cs_attr_set = false;         // > 64 KB dynamic LDS enabled for the camshift kernels on this context's device
    int cs_region_cap = 40960;        // pixels of the LDS-cached search region (option cs_region=0 disables it)        // option cs_keep_hist: the fused kernel also writes its histogram for ht_camshift_debug_hist
    int cs_last_first = 0, cs_last_n = 0, cs_last_chunks = 0;  // layout of d_cs_hist after the last track call (debug read-back)
    const uint32_t *cs_last_hist = nullptr;                    // ... and which half of d_cs_hist it used

    // back-projection (ht_backproject.hip): scratch of its own, grown on demand, so that a call between two track steps leaves d_cs_hist,
    // d_cs_lut and the exchange slots alone.  Capacities in elements.
    uint32_t *d_bp_hist = nullptr;    // [frames][chunks][4096] chunk histograms of the bound frames
    double *d_bp_lut_w = nullptr;     // [frames][4096] weights (HT_BP_F64)
    uint32_t *d_bp_lut_px = nullptr;  // [frames][4096] expanded pixels v, v, v, 255 (HT_BP_RGBA8)
    uint8_t *d_bp_out = nullptr;      // staging of the host form's result
    size_t bp_hist_cap = 0, bp_lut_w_cap = 0, bp_lut_px_cap = 0, bp_out_cap = 0;

    // camshift on (stream, frame) pairs (ht_cs_pairs.hip): the call's pair table {stream, frame, histogram slot, rect} + list of distinct
    // frames goes through a staged table (HtStagedTable: copies and kernels are ordered by the stream);
    // the chunk histograms of the distinct frames have scratch of their own, grown on demand.  Capacities in elements.
    HtStagedTable csp_tab;
    uint32_t *d_csp_hist = nullptr;  // [distinct frames][chunks][4096]
    size_t csp_hist_cap = 0;
    bool csp_attr_set = false;       // > 64 KB dynamic LDS enabled for k_csp_meanshift on this context's device
    bool cs_pairs_force = false;     // option cs_pairs_force=1: identity layouts (first + i, i) go through the pair kernels too (tests, A/B)
    bool cs_pairs_cluster = false;   // option cs_pairs_cluster=1: pair calls on a few large frames take the cluster schedule (k_csp_lut + k_csp_meanshift_cluster),
                                     // tall rects of a few pairs the row-split initTracker (k_csp_init_rows); ht_cs_plan_track_pairs / ht_cs_plan_init_pairs
    std::vector<int32_t> cs_pair_slot;  // after a pair call: histogram slot of every stream it paired (-1: not part of it), for ht_camshift_debug_hist
    int cs_pair_chunks = 0;

    // ht_camshift_init_best (ht_cs_best.hip): what its resolve kernel decided — [pairs codes][pairs rects of 4 int32] on the device, copied
    // to the pinned twin by the call itself; the event behind the call's kernels is what ht_camshift_init_best_result waits for
    int32_t *d_csb_res = nullptr, *h_csb_res = nullptr;
    size_t csb_cap = 0;                // pairs both hold
    hipEvent_t ev_csb = nullptr;
    int csb_n = 0;                     // pairs of the last call (0: none)
    const void *csb_states = nullptr;  // d_cs at that call: a later ht_camshift_reserve that reallocated the trackers ends the result's life
    // ht_camshift_init_faces (ht_cs_faces.hip): the same for its 32-byte records (ht_csf_record), one per pair
    uint8_t *d_csf_res = nullptr, *h_csf_res = nullptr;
    size_t csf_cap = 0;                // records both hold
    hipEvent_t ev_csf = nullptr;
    int csf_n = 0;                     // pairs of the last call (0: none)
    const void *csf_states = nullptr;  // d_cs at that call

    // ingest (ht_ingest.hip): device staging of ht_draw_frames' host-resident source frames, grown on demand
    uint8_t *d_ingest_src = nullptr;
    size_t ingest_src_cap = 0;
    // ht_draw_list_device (ht_draw_list.hip): the call's descriptor table
    // (ht_draw_list_filtered_device, ht_draw_filter.hip, stages its wider descriptors through the same table: both are the draw list)
    HtStagedTable dl_tab;
    int draw_filter_rows = 0;  // option draw_filter_rows: the filtered draw's tile rows, 4 or 16 (0: the shipped 4) — for A-B measurements
    int orient_lanes = 0;  // option orient_lanes: the oriented draw's kernel for entries of odd rot, 1 = k_draw_list_oriented, 2 = .._turn (0: the shipped one) — for A-B measurements
    // the face crops (ht_crop.hip) and the aligned crops (ht_align.hip), one host path for both (ht_face_calls.hip): each family has a
    // descriptor table and the records of its last call of its OWN — a draw call, a crop call and an align call of one step share nothing
    HtFaceCalls crop, align;

    std::vector<std::pair<void *, size_t>> user_allocs;  // ht_device_alloc buffers still alive (pointer, bytes): freed by ht_destroy at the latest

    // device grouping (ht_group.hip): a batch's raw hits bucketed by frame, grouped and reduced to one 64-byte record per frame on the
    // device.  hits2 / rects hold hit_capacity entries and are allocated on first use; the result block (ht_group_plan.h: head, records,
    // status, ngrouped, count, start) and the scatter cursors grow with the frame count; konst = [HT_MAX_LEVELS level scales][u32 n].
    int grp_cap_opt = 1 << 30;           // option group_cap: hits of a frame one workgroup takes at most (ht_grp_cap clamps it)
    ht_hit *d_grp_hits2 = nullptr;
    ht_rect *d_grp_rects = nullptr;
    uint8_t *d_grp_out = nullptr, *h_grp_out = nullptr;  // device block and its pinned copy
    size_t grp_out_cap = 0, h_grp_out_cap = 0;           // bytes
    uint32_t *d_grp_cursor = nullptr;
    size_t grp_cursor_cap = 0;
    double *d_grp_konst = nullptr;
    ht_hit *d_grp_in = nullptr;          // ht_group_hits: the uploaded hit list
    size_t grp_in_cap = 0;
    bool grp_enqueued = false;           // ht_detect_best_enqueue was issued behind the batch in flight
    bool grp_valid = false;              // the device buffers hold the batch collected last (until the next enqueue of this kind)
    int grp_nframes = 0;                 // frames of the batch enqueued / collected last on this route
    int32_t grp_min_neighbors = 1, grp_frame_base = 0;
    std::vector<uint32_t> h_grp_ngrouped, h_grp_start, h_grp_status;   // per frame of the collected batch
    std::vector<std::vector<ht_rect>> h_grp_over;                      // grouped lists of the frames the host finished (over the cap)
    uint32_t grp_over_cap_frames = 0;    // such frames since the last ht_kernel_times(reset): reported there as grp_over_cap_frames

    // multi-GPU exchange buffer (ht_allgather.hip: ht_allgather_best_faces)
    void *d_gather = nullptr;
    size_t d_gather_bytes = 0;

    // profiling
    bool profiling = false;
    std::vector<HtKernelTimer> timers;
};

// roctx ranges around the host-side phases of a batch: libroctx64 is looked up once with dlopen; without it (or without a
// profiler attached) a range costs one predictable branch.  rocprofv3 --marker-trace shows "ht_detect_enqueue", "ht_detect_collect", ...
struct HtRange {
    explicit HtRange(const char *name);
    ~HtRange();
    bool on;
};

// error helpers -------------------------------------------------------------------------------------------
ht_status ht_fail(ht_ctx *ctx, ht_status st, const std::string &msg);
#define HT_HIP(ctx, call)                                                                                   \
    do {                                                                                                    \
        hipError_t e_ = (call);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return ht_fail((ctx), HT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)

// Device scratch grown on demand: *p holds >= need elements afterwards.  A reallocation waits for the work in flight first, like every
// reallocation of the library: synchronise, free, zero the capacity, allocate.  `message`: the HT_ERR_NOMEM text of a failed allocation
// (the buffer is then gone: *p == nullptr, *cap == 0).
template <typename T>
ht_status ht_grow_device(ht_ctx *c, T **p, size_t *cap, size_t need, const char *message) {
    if (*cap >= need) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (*p) (void)hipFree(*p);
    *p = nullptr, *cap = 0;
    if (hipMalloc(reinterpret_cast<void **>(p), need * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, message);
    }
    *cap = need;
    return HT_OK;
}

// The staged table's four steps.  reserve: the table and its slots hold >= need bytes afterwards (>= minimum when they have to be
// allocated); a reallocation waits for the work in flight first.  `message`: the HT_ERR_NOMEM text (the table is then empty: cap == 0).
inline ht_status ht_stage_reserve(ht_ctx *c, HtStagedTable *t, size_t need, size_t minimum, const std::string &message) {
    const size_t cap = ht_stage_capacity(t->cap, need, minimum);
    if (cap == t->cap) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (t->d) (void)hipFree(t->d);
    t->d = nullptr, t->cap = 0;
    for (auto &h : t->h) {
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
    bool ok = hipMalloc(reinterpret_cast<void **>(&t->d), cap) == hipSuccess;
    for (int k = 0; ok && k < HT_STAGE_SLOTS; k++) {
        ok = hipHostMalloc(reinterpret_cast<void **>(&t->h[k]), cap, hipHostMallocDefault) == hipSuccess;
        if (ok && !t->ev[k]) ok = hipEventCreateWithFlags(&t->ev[k], hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, message);
    }
    t->cap = cap;
    return HT_OK;
}

// take: the next pinned slot, for the caller to fill (csp_upload fills it from three pieces); waits until that slot's previous copy has left it
inline ht_status ht_stage_take(ht_ctx *c, HtStagedTable *t, uint8_t **slot) {
    t->taken = t->next;
    t->next = ht_stage_next_slot(t->next);
    HT_HIP(c, hipEventSynchronize(t->ev[t->taken]));  // never recorded: returns at once
    *slot = t->h[t->taken];
    return HT_OK;
}

// commit: the first `bytes` of the slot taken last go to the device table, behind everything enqueued so far
inline ht_status ht_stage_commit(ht_ctx *c, HtStagedTable *t, size_t bytes) {
    HT_HIP(c, hipMemcpyAsync(t->d, t->h[t->taken], bytes, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipEventRecord(t->ev[t->taken], c->stream));
    return HT_OK;
}

inline void ht_stage_free(HtStagedTable *t) {  // the stream has been synchronised
    if (t->d) (void)hipFree(t->d);
    for (int k = 0; k < HT_STAGE_SLOTS; k++) {
        if (t->h[k]) (void)hipHostFree(t->h[k]);
        if (t->ev[k]) (void)hipEventDestroy(t->ev[k]);
    }
    *t = HtStagedTable();
}

// profiling scope: records a start/stop event pair around kernel launches when ctx->profiling
struct HtProfScope {
    ht_ctx *ctx;
    hipStream_t stream;
    int idx = -1;
    hipEvent_t a = nullptr, b = nullptr;
    HtProfScope(ht_ctx *c, const char *name, hipStream_t on = nullptr);  // on == nullptr: the context's main stream
    ~HtProfScope();
};

// implemented in the .hip files ---------------------------------------------------------------------------
void ht_capture_mark(ht_ctx *ctx, bool on);                 // ht_camshift.hip: ctx->capturing, ordered against fused_threads' stream queries
// ht_camshift.hip: k_cs_hist on n frames into hist[n][nchunks][4096], chunk plan from ht_cs_hist_plan (ht_cs_schedule.h) — for
// ht_backproject.hip, which must not carry a copy of the kernel
ht_status ht_cs_hist_launch(ht_ctx *ctx, const uint8_t *frames, size_t frame_stride, int n, uint32_t npix, uint32_t chunk_px, uint32_t nchunks, uint32_t *hist);
// ht_camshift.hip: the result ring of the enqueue-only track calls (batch and pair form).  begin: *slot = the next free pinned slot when
// the call is enqueue-only or a synchronous call that goes through the ring (*via_ring), nullptr when it copies back; commit: the slot
// is outstanding
ht_status ht_cs_ring_begin(ht_ctx *ctx, const char *fn, int32_t n, const ht_cs_trackobj *out, bool *via_ring, ht_ctx::HtCsSlot **slot);
void ht_cs_ring_commit(ht_ctx *ctx, ht_ctx::HtCsSlot *slot, int32_t n);
// ht_camshift.hip: the cluster gate — one grid whose workgroups spin on each other (k_cs_meanshift_cluster, k_csp_meanshift_cluster) in
// flight per device and process once more than one context uses such grids.  begin: in front of the launch (takes the gate's lock; the
// context's stream waits for the previous cluster grid of the device when several contexts use the path); end: behind the launch (records
// it, releases the lock).  end must follow every begin, also a failed one and a failed launch.
ht_status ht_cs_cluster_gate_begin(ht_ctx *ctx);
ht_status ht_cs_cluster_gate_end(ht_ctx *ctx);
// ht_camshift.hip: the cluster error word (d_cs_err / h_cs_err / h_cs_err_direct) as a status: HT_ERR_STATE with the barrier message when set
ht_status ht_cs_check_err(ht_ctx *ctx, const char *where);
// ht_camshift.hip: copy-back route of a result read-back: `count` track objects and the error word, stream synchronised, word checked
ht_status ht_cs_read_back(ht_ctx *ctx, const char *fn, ht_cs_trackobj *out, const ht_cs_trackobj *d_src, size_t count);
void ht_camshift_free(ht_ctx *ctx);                         // ht_camshift.hip: tracker state, scratch, result ring, the cluster gate's entry (ht_destroy)
void ht_backproject_free(ht_ctx *ctx);                      // ht_backproject.hip: its scratch (ht_destroy)
void ht_cs_pairs_free(ht_ctx *ctx);                         // ht_cs_pairs.hip: pair table, staging and histogram scratch (ht_destroy)
void ht_cs_best_free(ht_ctx *ctx);                          // ht_cs_best.hip: the result buffers of ht_camshift_init_best (ht_destroy)
void ht_cs_faces_free(ht_ctx *ctx);                         // ht_cs_faces.hip: the result buffers of ht_camshift_init_faces (ht_destroy)
void ht_ingest_free(ht_ctx *ctx);                           // ht_ingest.hip: the host form's source staging, the draw list's table (ht_destroy)
void ht_align_free(ht_ctx *ctx);                            // ht_face_calls.hip: the aligned crops' table, records and events (called by ht_ingest_free)
void ht_crop_free(ht_ctx *ctx);                             // ht_face_calls.hip: the face crops' table, records and events (called by ht_ingest_free)
void ht_group_free(ht_ctx *ctx);                            // ht_group.hip: the device grouping's buffers (ht_destroy)
// ht_detect_step.hip: the head of every collect call — `bytes` from the device into pinned memory and the batch's whitebalance sums behind
// them, one synchronisation, the state every collect call leaves behind
ht_status ht_detect_fetch(ht_ctx *ctx, void *pinned_dst, const void *dev_src, size_t bytes);
void ht_frames_set(ht_ctx *ctx, const uint8_t *frames, size_t frame_stride, int n);  // ht_frames.hip: THE binding setter (frames == nullptr: unbound)
ht_status ht_frames_own_reserve(ht_ctx *ctx, size_t need, const char *fn);  // ht_frames.hip: the context's own frame buffer holds >= need bytes
void ht_frames_bind_own(ht_ctx *ctx, int n);                // ht_frames.hip: binds its first n frames (packed), as after ht_upload_frames
ht_status ht_launch_pyramid(ht_ctx *ctx, uint32_t flags);   // ht_pyramid.hip
ht_status ht_launch_scan(ht_ctx *ctx, uint32_t flags);      // ht_scan.hip
ht_status ht_launch_scan_early(ht_ctx *ctx, uint32_t flags); // ht_scan.hip: called by ht_launch_pyramid after generation early_gen
bool ht_scan_is_builtin_cascade(const uint8_t *blob, size_t len);  // ht_scan.hip: an input of ht_plan_cascade_split
ht_status ht_launch_gray_inplace(ht_ctx *ctx, uint8_t *d_rgba, int n, size_t stride);  // ht_pyramid.hip
ht_status ht_launch_whitebalance(ht_ctx *ctx, double *d_out, bool zero);                 // ht_pyramid.hip

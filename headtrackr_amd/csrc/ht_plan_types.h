// ht_plan_types.h — the plain records of a geometry's plan: what the host planner (ht_geometry_plan.h) fills in and the pyramid and scan
// kernels read.  No HIP: ht_internal.h includes it for the library, tests/host/geometry_plan_harness.cc compiles it with g++.
#pragma once

#include <stdint.h>

#include <vector>

#include "headtrackr_hip.h"  // HT_MAX_LEVELS

// ---------------------------------------------------------------------------------------------------------
// Pyramid geometry (ccv.js:110-147), device copy.
struct HtDevLevel {
    int32_t w, h, stride;
    uint32_t off[4];  // byte offset of slot 0..3 inside one frame's arena (0xffffffff = absent)
};

// One resample job = one canvas of the pyramid (ccv.js:121,128,135,140,145).
// k_resample_tail argument: generations [first, first + ngen) as ranges into the tail job table
constexpr int HT_TAIL_MAX_GENS = 8;
constexpr int HT_TAIL_MAX_JOBS = 32;  // per generation (6 levels x 4 variants = 24 in the reference's pyramid)
struct HtTailGens {
    int32_t ngen;
    int32_t job_begin[HT_TAIL_MAX_GENS + 1];
    uint32_t groups[HT_TAIL_MAX_GENS];  // 4-pixel groups (canvas width rounded up to 4, times canvas height) per generation
    uint32_t tap_begin[HT_TAIL_MAX_GENS + 1];  // range of the generation's entries in the tap tables (its jobs' taps are contiguous)
};

// One tap of the declared resampler (oracle/canvas_shim.js): destination coordinate i of a drawImage call reads source samples a
// and b = min(a + 1, s - 1) (absolute, incl. the source rect origin) with weights u = 1 - t and t.  Computed on the device by
// rs_tap (ht_resample_tap.h) and, for the tile records and the tail kernel's jobs, once on the host by ht_host_tap
// (ht_geometry_plan.h) — the same binary64 operations.
struct HtTap {
    double t, u;
    int32_t a, b;
};
// k_resample_tail reads its taps from tables built by the host: the compact form {a, (float)t} for the binary32 estimate (column
// tables are padded by 3 entries so that 4 consecutive ones can always be loaded), the full form for the rare binary64 fallback
struct HtTapFast {
    int32_t a;
    float tf;
};
struct HtTailTapRef {
    uint32_t col, row;  // first column / row tap of the job in both tables
    uint32_t mode;      // bit 0: exact 2:1 in both directions (integer 2x2 box mean), bit 1: binary64 everywhere (option rs_nofast)
    uint32_t pad;
};

// One drawImage call (host job list) and, with the tile fields filled in, one k_resample workgroup (device tile table).
constexpr int HT_RS_SRC_ROWS = 75;   // k_resample LDS window: source rows per tile (3 staging passes of 25 rows; 16 * 4 * 1.1225 + 3 = 74.8 still fits)
constexpr int HT_RS_MAX_PASSES = 4;  // k_resample: 16-row passes per tile at most
struct HtResampleJob {
    uint32_t src_off, dst_off;
    int32_t src_stride, dst_stride;
    int32_t sx, sy, sw, sh;  // source rect
    int32_t dw, dh;          // destination rect (at 0,0)
    int32_t cw, ch;          // destination canvas size (pixels outside dw x dh are written 0)
    uint16_t bx, pass0;      // tile record only: tile column (64 px), first 16-row pass
    uint16_t np, pad;        // tile record only: number of 16-row passes (<= HT_RS_MAX_PASSES)
    double rx, ry;           // sw/dw, sh/dh computed on the host (binary64 division)
    // tile record only: the source rectangle the tile's taps touch, from the host (ht_host_tap: the same binary64 operations as
    // rs_tap).  ex_sw16 == 0: not filled in, the kernel derives it (four rs_tap evaluations, ~1 400 cycles at the top of every
    // workgroup before its first load can be issued)
    int32_t ex_xa, ex_ya;    // first source column (rounded down to 16) / row
    int32_t ex_sw16, ex_sh;  // 16-byte chunks per source row, source rows
    // k_resample_bands: wavefront w of the tile owns destination rows [4 np w, 4 np (w + 1)) and the source rows they touch — byte w of
    // band_ya4 = first row relative to ex_ya, byte w of band_sh4 = rows; pad bit 2 says that all four fit a band (<= HT_RSB_ROWS rows)
    uint32_t band_ya4, band_sh4;
};
constexpr int HT_RSB_ROWS = 24;  // k_resample_bands: source rows per wavefront band (4 KB of the 160-byte LDS pitch, one spare row)

// One scan scale (ccv.js:154-160) and its tiling.
constexpr int HT_SCAN_TXH = 64;  // k_scan_tiles tile width  in half-window steps X'
constexpr int HT_SCAN_TYH = 32;  // k_scan_tiles tile height in half-window steps Y'
struct HtScanScale {
    int32_t l0, l1, l2;   // levels i, i+next, i+2*next
    int32_t qw, qh;       // windows per row / column on the quarter-resolution plane (ccv.js:155-156)
    int32_t tw2, th2;     // tile size in half-window steps X', Y' (X' = 2x+dx, Y' = 2y+dy)
    int32_t ntx, nty;     // tiles per row / column
    uint32_t tile_begin;  // first tile of this scale in the per-frame tile list
    uint32_t div_magic;   // ceil(2^20 / tw2): id / tw2 == (id * magic) >> 20 for id < 4096
    uint32_t win_begin;   // first window of this scale in the flat per-frame window index (simple kernel)
};

// Everything a k_scan_tiles workgroup needs to know about its tile in one 64-byte record = ONE scalar load after the tile index is
// known (it used to be a chain of three dependent lookups — tile -> scale -> three level records — in front of the tile's first
// HBM load; a workgroup holds its 26 KB of LDS while it waits).
struct alignas(64) HtTileRec {
    uint32_t off0, off1, off2[4];  // byte offsets inside a frame's arena: level i, level i+6, the four variants of level i+12
    uint32_t sh0, sh1, sh2;        // stride | height << 16 of the three levels
    uint32_t origin;               // X0 | Y0 << 16: tile origin in half-window steps
    uint32_t size;                 // tw | th << 16: half-window steps of the tile that hold windows (clipped to the scale)
    uint32_t tw2_l0;               // tile pitch tw2 (window id = Y' * tw2 + X') | the scale's level index << 16
    uint32_t div_magic;            // ceil(2^20 / tw2)
    uint32_t strip_magic;          // ceil(2^24 / (4 * th)): stage 0 walks the tile in strips of 4 window pairs (see k_scan_tiles)
    uint32_t pad[2];
};
static_assert(sizeof(HtTileRec) == 64, "HtTileRec");

// ---------------------------------------------------------------------------------------------------------
// The planner's interface (ht_geometry_plan.h: ht_plan_geometry).  Inputs: everything besides the frame size, the batch size and the
// level sizes that a plan depends on — the cascade's window, ccv's interval and the options that select among schedules.
struct HtPlanInputs {
    int interval, next;
    uint32_t cw, ch;
    int rs_rpt;
    bool rs_nofast, rs_nosort, rs_notail;
    uint64_t rs_tailcap;
    bool rs_tailcap_forced;
    int tail_table;
    bool tail_table_forced;
    bool early_scan, aux_stream;  // option early_scan / the context has its second stream
    uint32_t queue_capacity_cfg;
};

// One geometry's plan: the host tables the launch code reads and the ones ht_set_geometry uploads as they are.
struct HtGeometryPlan {
    HtDevLevel levels[HT_MAX_LEVELS] = {};
    uint64_t arena_stride = 0;  // bytes per frame
    uint64_t pyr_bytes = 0, windows_per_frame = 0;
    std::vector<std::vector<HtResampleJob>> gens;       // generation g: jobs that only depend on generations < g
    std::vector<std::vector<HtResampleJob>> gen_tiles;  // per generation: k_resample tile records (job + tile position) in launch order
    std::vector<uint32_t> gen_blocks;                   // ... and how many
    // k_resample_tail: the last generations (tiny levels) in ONE launch, one workgroup per frame
    int tail_first_gen = 0;                  // first generation handled by the tail kernel (0 = none)
    int tail_table = 0;  // k_resample_tail with host tap tables: 1 = compact taps in LDS, 2 = taps from L2 / small footprint; 0: the round-1 binary64 tail (option rs_tailtable)
    std::vector<HtResampleJob> tail_jobs;    // jobs of generations >= tail_first_gen, generation by generation
    std::vector<uint32_t> tail_prefix;       // per job: 4-pixel groups of the jobs before it in its generation
    std::vector<HtTap> tail_taps;            // tap tables of the tail jobs (full form) ...
    std::vector<HtTapFast> tail_taps_fast;   // ... and compact form
    std::vector<HtTailTapRef> tail_tapref;   // per tail job: where its taps start
    HtTailGens tail = {};                    // per generation: job range and group count (kernel argument)
    std::vector<HtScanScale> scales;
    std::vector<HtTileRec> tile_recs;        // per-frame tile list (same for every frame of a batch)
    uint32_t tiles_per_frame = 0;
    int early_gen = 0;             // generation after which the early tiles may start (0 = none for this geometry)
    uint32_t early_tiles = 0;      // tiles per frame of the early scales (a prefix of the tile list)
    uint32_t queue_capacity = 0;   // survivor queue entries
};

// ht_cascade_types.h — the plain records of a cascade's plan: what the host planner (ht_cascade_plan.h) fills in and the scan kernels read,
// with the LDS layout constants both sides address by.  No HIP: ht_internal.h includes it for the library,
// tests/host/cascade_plan_harness.cc compiles it with g++.
#pragma once

#include <stdint.h>

#include <vector>

#include "ht_plan_types.h"  // HT_SCAN_TXH, HT_SCAN_TYH

#define HT_MAXPTS 8

// ---------------------------------------------------------------------------------------------------------
// Cascade, host view of the "HTCB" blob (headtrackr_amd/js/cascade_pack.js) == headtrackr.cascade (cascade.js:19)
struct HtBlobFeature {
    uint8_t size, pad[7];
    int8_t px[HT_MAXPTS], py[HT_MAXPTS], pz[HT_MAXPTS];
    int8_t nx[HT_MAXPTS], ny[HT_MAXPTS], nz[HT_MAXPTS];
    double alpha[2];
};
struct HtBlobStage {
    uint32_t count, first;
    double threshold;
};
static_assert(sizeof(HtBlobFeature) == 72 && sizeof(HtBlobStage) == 16, "HTCB layout");

// ---------------------------------------------------------------------------------------------------------
// The LDS layouts the offset tables address (ht_scan.hip keeps its short names for them, with the measurements behind the values).
// k_scan_tiles, "unified-base" tile: plane 0 in HT_SCAN_ROWS0 rows of HT_SCAN_PITCH0 bytes, behind it the half-step grid of planes 1 / 2.
constexpr int HT_SCAN_PITCH0 = 152;
constexpr int HT_SCAN_ROWS0 = 2 * HT_SCAN_TYH + 22;                  // 86
constexpr int HT_SCAN_P12_BASE = HT_SCAN_PITCH0 * HT_SCAN_ROWS0;     // 13072
constexpr int HT_SCAN_GH = HT_SCAN_TYH + 11;                         // 43 grid rows ...
constexpr int HT_SCAN_G_PITCH = 2 * HT_SCAN_PITCH0;                  // ... of 304 bytes
constexpr int HT_SCAN_LDS_TILE_BYTES = HT_SCAN_P12_BASE + HT_SCAN_GH * HT_SCAN_G_PITCH;  // 26144
// unified-base LDS offsets of a feature point (x, y) on plane 0 / 1 / 2, relative to the window base B: the generated stages
// (ht_cascade_gen.inc) and the planner's tables (ht_tile_off) both come from these three
#define HT_O0(x, y) ((y) * HT_SCAN_PITCH0 + (x))                             // level i:        1 B/px, row pitch P
#define HT_O1(x, y) (HT_SCAN_P12_BASE + (y) * HT_SCAN_G_PITCH + 2 * (x))     // level i+6:      2 B/px, row pitch 2P
#define HT_O2(x, y) (HT_SCAN_P12_BASE + 1 + 4 * (y) * HT_SCAN_PITCH0 + 4 * (x))  // level i+12 q: odd bytes, 4 B/px, row pitch 4P
// k_scan_deep / k_scan_deep_lds, per-wavefront window patch: the cw x ch window of level i at 0, its half-resolution counterpart at
// HT_PATCH1, the quarter-resolution one at HT_PATCH2 (24x24 + 12x12 + 6x6 = 756 bytes)
constexpr int HT_PATCH1 = 576, HT_PATCH2 = 720, HT_PATCH_BYTES = 768;
constexpr uint32_t HT_DEEP_LDS_TABLE_BYTES = 64 * 1024;  // k_scan_deep_lds: the packed tail of the cascade it keeps in LDS, at most

// ---------------------------------------------------------------------------------------------------------
// Device-side cascade tables.
//
// Tile kernel: every point of every feature as a byte offset into the workgroup's LDS tile, relative to the
// window base (see ht_scan.hip "unified-base layout"); read with uniform (scalar) loads, one feature at a time.
struct alignas(64) HtTileFeature {
    uint32_t po[HT_MAXPTS / 2];  // positive-point offsets, two u16 per word (low half first); valid ones first, count = np
    uint32_t no[HT_MAXPTS / 2];  // negative-point offsets, count = nn
    uint32_t a[4];               // alpha[2k] (lo,hi words), alpha[2k+1] (lo,hi)  (ccv.js:194,219)
    uint32_t np, nn;
    uint32_t pad[2];
};
static_assert(sizeof(HtTileFeature) == 64, "HtTileFeature");

// Deep kernel: coordinate form, one feature per lane.  Slots >= np / nn repeat slot 0 (min/max are idempotent).
struct alignas(16) HtDeepFeature {
    uint8_t px[HT_MAXPTS], py[HT_MAXPTS], pz[HT_MAXPTS];  // each array is read as one 64-bit word on the device
    uint8_t nx[HT_MAXPTS], ny[HT_MAXPTS], nz[HT_MAXPTS];
    int64_t a0i, a1i;  // alpha * 1e8 as exact integers (valid when the cascade is "decimal", see ht_cascade_plan.h)
    double a0, a1;
};
static_assert(sizeof(HtDeepFeature) == 80, "HtDeepFeature");

// Deep kernel: offsets into the per-wavefront window patch in LDS (24x24 + 12x12 + 6x6 bytes, see ht_scan.hip).
struct alignas(16) HtPatchFeature {
    uint16_t poff[HT_MAXPTS];  // slots >= np repeat slot 0
    uint16_t noff[HT_MAXPTS];
    int64_t a0i, a1i;          // alpha * 1e8 as exact integers
    double a0, a1;
};
static_assert(sizeof(HtPatchFeature) == 64, "HtPatchFeature");

// Deep kernel, LDS-resident form: 32-byte record, the whole tail of the cascade (stages >= split) is copied into LDS once
// per workgroup.  Usable when every feature has <= 5 points per polarity and |alpha * 1e8| < 2^31 (decimal cascade).
struct alignas(16) HtPackedFeature {
    uint16_t off[10];  // p0..p4, n0..n4 patch offsets (unused slots repeat slot 0 of their polarity)
    int32_t a0i, a1i;  // alpha * 1e8; the binary64 alpha is recovered exactly as (double)a / 1e8
    uint32_t pad;
};
static_assert(sizeof(HtPackedFeature) == 32, "HtPackedFeature");

struct HtDevStage {
    uint32_t first, count;
    uint32_t maxpts;  // max(np, nn) over the stage's features
    uint32_t pad;
    double threshold;
    int64_t thri;  // threshold * 1e8
};

// ---------------------------------------------------------------------------------------------------------
// One cascade's plan (ht_cascade_plan.h: ht_plan_cascade, then ht_plan_cascade_split): the blob's rows, what the launch code asks about
// them, and the tables ht_create uploads as they are.
struct HtCascadePlan {
    uint32_t cw = 24, ch = 24, nstages = 0, nfeat = 0;
    std::vector<HtBlobStage> stages;  // the blob's rows
    std::vector<HtBlobFeature> feats;
    bool decimal_alphas = false;  // all alphas / thresholds are k * 1e-8 exactly -> integer decisions allowed
    uint32_t split_stage = 4;     // stages [0, split) in the tile kernel, [split, nstages) in the deep kernel
    uint32_t packed_first = 0;    // global index of packed[0]: the first feature of split_stage
    std::vector<HtDevStage> dev_stages;
    std::vector<HtDeepFeature> deep;
    std::vector<HtTileFeature> tile;
    // every feature in the packed 32-byte form with TILE offsets (off[] relative to a window's LDS base, a1i = alpha[2k+1] * 1e8): the tile
    // kernel's feature-parallel sparse phase reads one record per lane (empty: cascade not decimal / more than 5 points / a0 != -a1)
    std::vector<HtPackedFeature> fp;
    std::vector<HtPatchFeature> patch;
    std::vector<HtPackedFeature> packed;  // features of stages >= split_stage with PATCH offsets (empty: k_scan_deep runs instead of k_scan_deep_lds)
};

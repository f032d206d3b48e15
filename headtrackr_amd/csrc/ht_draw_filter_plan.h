// ht_draw_filter_plan.h — the host side of ht_draw_list_filtered_device (the draw list with a prefilter for strong downscales): a list is
// validated by ht_draw_list_plan.h's rules and turned into the descriptors k_draw_list_mean_tile reads, without HIP.
//
// The draw list samples one bilinear tap pair per canvas pixel: 1920 x 1080 drawn onto 320 x 240 reads 2 of every 6 columns and 2 of every
// 4.5 rows, the rest alias.  The filtered call writes each canvas pixel as the mean of an Nx x Ny block of the UNFILTERED rule's samples
// instead.  For an entry whose source rect is sw x sh, drawn onto a W x H canvas with max_factor 1 .. 8:
//
//   Nx = ht_filter_factor(sw, W, max_factor) = min(max_factor, max(1, ceil(sw / W))),  Ny likewise from sh and H      (ht_filter_plan.h)
//
// The fine frame F is, by definition, what ht_draw_list_device gives for the same entry on a canvas of Nx W x Ny H: the same rect,
// rx' = sw / (Nx W) and ry' = sh / (Ny H) as ONE binary64 division each, the same edge clamps, YUV taps converted first.  Per channel, alpha
// included, with n = Nx Ny:
//
//   out(x, y) = (sum of F(Nx x + a, Ny y + b) over a < Nx, b < Ny  +  (n >> 1)) / n            (integer division: ht_filter_pixel)
//
// Consequences: factors (1, 1) — max_factor 1, any source rect not larger than the canvas, upscales — give ht_draw_list_device's bytes;
// where sw == Nx W and sh == Ny H exactly, the fine frame of an RGBA entry is the source block itself and the output its exact integer box
// mean; a ratio above max_factor is clamped to it: the fine frame is then itself a decimating draw, and the result is defined all the same.
//
// The factors are known on the host (unlike the face crops', which follow a tracked box): the plan writes them, with the FINE ratios in the
// place of rx and ry, into a descriptor of 112 bytes — HtDrawDesc (104 bytes, unchanged) and the two factors.  Bounds: sw, sh <= 2^14, so
// Nx W < sw + W: a fine canvas is less than 2^14 wider than the canvas and stays inside int32 for every canvas the geometry admits.
//
// Plain C++17: ht_draw_filter.hip plans every call with ht_draw_filter_plan; the CPU suite compiles this header alone
// (tests/host/draw_filter_plan_harness.cc) with AddressSanitizer + UBSan.
#pragma once

#include "ht_draw_list_plan.h"
#include "ht_filter_plan.h"

// what a workgroup of k_draw_list_mean_tile reads for its entry: the draw list's descriptor with rx, ry the FINE ratios, and the factors
template <class PLANE>
struct HtDrawMeanDescT {
    HtDrawDescT<PLANE> d;
    int32_t nx, ny;
};
typedef HtDrawMeanDescT<const uint8_t *> HtDrawMeanDesc;
static_assert(sizeof(HtDrawMeanDesc) == 112 && alignof(HtDrawMeanDesc) == 8, "descriptor layout");

// the call's own status, behind ht_draw_list_plan.h's
constexpr int HT_DRAW_FILTER_BAD_FACTOR = 100;

inline const char *ht_draw_filter_message(int st) { return st == HT_DRAW_FILTER_BAD_FACTOR ? "max_factor must be 1..8" : ht_draw_list_message(st); }

inline bool ht_draw_filter_factor_ok(int32_t max_factor) { return max_factor >= HT_FILTER_MIN_FACTOR && max_factor <= HT_FILTER_MAX_FACTOR; }

// the factors of a sw x sh rect on a W x H canvas; every argument positive, max_factor 1 .. 8
inline void ht_draw_filter_factors_of(int32_t sw, int32_t sh, int32_t W, int32_t H, int32_t max_factor, int32_t *nx, int32_t *ny) {
    *nx = ht_filter_factor(sw, W, max_factor), *ny = ht_filter_factor(sh, H, max_factor);
}

// one entry: *d and *e are written only on success
inline int ht_draw_filter_plan_entry(const ht_draw_source &s, int32_t W, int32_t H, int32_t max_factor, HtDrawMeanDesc *d, HtDrawExtent *e) {
    HtDrawMeanDesc o = {};
    HtDrawExtent x = {};
    const int st = ht_draw_list_plan_entry(s, W, H, &o.d, &x);
    if (st != HT_DRAW_LIST_OK) return st;
    ht_draw_filter_factors_of(o.d.sw, o.d.sh, W, H, max_factor, &o.nx, &o.ny);
    // the fine frame's ratios: one binary64 division each (at factor 1 the bits of the unfiltered plan's)
    o.d.rx = (double)o.d.sw / (double)((int64_t)o.nx * W), o.d.ry = (double)o.d.sh / (double)((int64_t)o.ny * H);
    *d = o, *e = x;
    return HT_DRAW_LIST_OK;
}

// the whole list: ht_draw_list_plan's contract, with max_factor checked between the call's own arguments and the first entry
inline int ht_draw_filter_plan(const ht_draw_source *srcs, int32_t n, int32_t W, int32_t H, int32_t max_factor, HtDrawMeanDesc *desc, HtDrawExtent *ext,
                               int32_t *bad) {
    *bad = -1;
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return HT_DRAW_LIST_BAD_COUNT;
    if (W <= 0 || H <= 0) return HT_DRAW_LIST_BAD_CANVAS;
    if (!ht_draw_filter_factor_ok(max_factor)) return HT_DRAW_FILTER_BAD_FACTOR;
    for (int32_t i = 0; i < n; i++) {
        const int st = ht_draw_filter_plan_entry(srcs[i], W, H, max_factor, desc + i, ext + i);
        if (st != HT_DRAW_LIST_OK) {
            *bad = i;
            return st;
        }
    }
    return HT_DRAW_LIST_OK;
}

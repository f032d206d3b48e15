// ht_cs_best_plan.h — the decision of ht_camshift_init_best, without HIP: does a frame's best-face record (ht_group.hip: 8 binary64
// [x, y, width, height, confidence, neighbors, frame, 1.0]) initialise a tracker, with which rect, or is the pair left alone?
// facetrackr.js:97-107: `confidence > threshold`, the rect floored, initTracker.  Host AND device text: k_csb_resolve (ht_cs_best.hip)
// compiles these lines as device functions (it defines HT_CSB_FN in front of the #include), tests/host/init_best_harness.cc compiles the
// SAME lines with g++ -fsanitize=address,undefined.  No library call and no HIP type: floor is written out in integer conversions.
#pragma once

#include <stdint.h>

#include "headtrackr_hip.h"  // HT_CSB_* result codes, ht_cs_rect

#ifndef HT_CSB_FN
#define HT_CSB_FN inline
#endif

// the flag word of a pair (CspEntry.pad of the call's device table) and of the call
enum : int32_t {
    HT_CSB_F_SKIP = 1,          // written by k_csb_resolve: the init kernels' workgroups of this pair return at once
    HT_CSB_F_HAS_FALLBACK = 2,  // set by the host: the entry's rect is the pair's fallback rect
};
constexpr uint32_t HT_CSB_ST_OVER_CAP = 1u;  // == HT_GRP_ST_OVER_CAP (ht_group_plan.h; ht_cs_best.hip asserts it)

// floor(v) as int32, saturated; NaN -> 0.  (int32_t)v truncates towards zero and is only evaluated inside the int32 range.
HT_CSB_FN int32_t ht_csb_floor_i32(double v) {
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return INT32_MAX;
    if (v <= -2147483648.0) return INT32_MIN;
    const int32_t t = (int32_t)v;
    return (double)t > v ? t - 1 : t;  // t >= -2147483647 here
}

// One pair.  rec: the frame's record; status: its status word; head_nhits / head_bad: the batch head; collected: the batch has been
// collected (grp_take_results completed the over-cap records on the device: the status word no longer says "not final").
// Returns the HT_CSB_* code and writes the rect the init kernels use (zeros for HT_CSB_UNTOUCHED / HT_CSB_DEFERRED).
HT_CSB_FN int32_t ht_csb_decide(const double *rec, uint32_t status, uint32_t head_nhits, uint32_t head_bad, uint32_t hit_capacity, bool collected,
                                double min_confidence, bool has_fallback, const ht_cs_rect &fallback, ht_cs_rect *rect) {
    rect->x = rect->y = rect->width = rect->height = 0;
    if (head_nhits > hit_capacity || head_bad != 0u || (!collected && (status & HT_CSB_ST_OVER_CAP))) return HT_CSB_DEFERRED;
    if (rec[5] > 0.0 && rec[4] > min_confidence) {  // neighbors > 0 && confidence > threshold (strict: facetrackr.js:97)
        rect->x = ht_csb_floor_i32(rec[0]), rect->y = ht_csb_floor_i32(rec[1]);
        rect->width = ht_csb_floor_i32(rec[2]), rect->height = ht_csb_floor_i32(rec[3]);
        return HT_CSB_FACE;
    }
    if (has_fallback) {
        *rect = fallback;
        return HT_CSB_FALLBACK;
    }
    return HT_CSB_UNTOUCHED;
}

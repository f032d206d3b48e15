// ht_crop_plan.h — the rule of the face crops (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device), without HIP and in
// integers only: which rect of a feed's source frame belongs to a stream's track object?  The track object (camshift.js:253-254: x, y is
// the CENTRE) lives in canvas coordinates; the canvas was drawn from the mapping rect (mx, my, mw, mh) of a source of SW x SH pixels.  The
// box, widened by margin_q8 / 256, is mapped back through that rect, rounded OUTWARDS to whole source pixels, optionally made square, and
// clamped to the source frame (not to the mapping rect: a face at the edge of the drawn region keeps its surroundings).
//
// Host AND device text, as ht_cs_best_plan.h is: k_crop_list (ht_crop.hip) compiles these lines as device functions (it defines HT_CROP_FN
// in front of the #include), tests/host/crop_plan_harness.cc compiles the SAME lines with g++ -fsanitize=address,undefined.  No library
// call and no HIP type.  Every product is formed in int64: |edge| <= 512 * 2^20 + 65536 * 1024 < 2^30, times a mapping extent < 2^31.
#pragma once

#include <stdint.h>

#include "headtrackr_hip.h"   // HT_CROP_* codes and flags, ht_cs_rect
#include "ht_cs_best_plan.h"  // ht_csb_floor_i32

#ifndef HT_CROP_FN
#define HT_CROP_FN inline
#endif

constexpr int32_t HT_CROP_MAX_BOX = 65536;        // a tracked box wider or taller than this is no box
constexpr int32_t HT_CROP_MAX_CENTRE = 1 << 20;   // ... and neither is one centred further out
constexpr int32_t HT_CROP_MIN_MARGIN = 64, HT_CROP_MAX_MARGIN = 1024, HT_CROP_MAX_OUT = 1024;

// a / b rounded towards -inf and towards +inf; b > 0
HT_CROP_FN int64_t ht_crop_floordiv(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}
HT_CROP_FN int64_t ht_crop_ceildiv(int64_t a, int64_t b) {
    const int64_t q = a / b;
    return (a % b != 0 && a > 0) ? q + 1 : q;
}

// (x, y, width, height): the track object.  W, H >= 1: the canvas.  SW, SH: the source.  (mx, my, mw, mh): the rect of the source that was
// drawn onto the canvas; mw == 0 && mh == 0: the whole source.  Returns HT_CROP_FACE and the rect in source pixels, or HT_CROP_EMPTY and zeros.
HT_CROP_FN int32_t ht_crop_rule(double x, double y, double width, double height, int32_t W, int32_t H, int32_t SW, int32_t SH, int32_t mx, int32_t my,
                                int32_t mw, int32_t mh, int32_t margin_q8, uint32_t flags, ht_cs_rect *rect) {
    rect->x = rect->y = rect->width = rect->height = 0;
    if (mw == 0 && mh == 0) mx = 0, my = 0, mw = SW, mh = SH;
    const int32_t cx = ht_csb_floor_i32(x), cy = ht_csb_floor_i32(y), w = ht_csb_floor_i32(width), h = ht_csb_floor_i32(height);
    if (w <= 0 || h <= 0 || w > HT_CROP_MAX_BOX || h > HT_CROP_MAX_BOX) return HT_CROP_EMPTY;
    if (cx > HT_CROP_MAX_CENTRE || cx < -HT_CROP_MAX_CENTRE || cy > HT_CROP_MAX_CENTRE || cy < -HT_CROP_MAX_CENTRE) return HT_CROP_EMPTY;
    // the edges in 1/512 canvas pixel
    const int64_t L = 512 * (int64_t)cx - (int64_t)w * margin_q8, R = 512 * (int64_t)cx + (int64_t)w * margin_q8;
    const int64_t T = 512 * (int64_t)cy - (int64_t)h * margin_q8, B = 512 * (int64_t)cy + (int64_t)h * margin_q8;
    // ... in source pixels, rounded outwards
    int64_t l = mx + ht_crop_floordiv(L * mw, 512 * (int64_t)W), r = mx + ht_crop_ceildiv(R * mw, 512 * (int64_t)W);
    int64_t t = my + ht_crop_floordiv(T * mh, 512 * (int64_t)H), b = my + ht_crop_ceildiv(B * mh, 512 * (int64_t)H);
    if (flags & HT_CROP_SQUARE) {  // the shorter side grows around its middle, before the clamp
        const int64_t dw = r - l, dh = b - t;
        if (dw < dh) l -= ht_crop_floordiv(dh - dw, 2), r = l + dh;
        else if (dh < dw) t -= ht_crop_floordiv(dw - dh, 2), b = t + dw;
    }
    l = l < 0 ? 0 : l, t = t < 0 ? 0 : t, r = r > SW ? SW : r, b = b > SH ? SH : b;
    if (r <= l || b <= t) return HT_CROP_EMPTY;
    rect->x = (int32_t)l, rect->y = (int32_t)t, rect->width = (int32_t)(r - l), rect->height = (int32_t)(b - t);
    return HT_CROP_FACE;
}

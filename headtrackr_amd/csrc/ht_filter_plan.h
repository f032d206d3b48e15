// ht_filter_plan.h — the rule of the prefiltered face crops (ht_camshift_crop_*_filtered_device / ht_camshift_align_*_filtered_device),
// without HIP and in integers only: by which factors is an entry's patch oversampled, and how is a block of fine samples averaged?
//
// The crop, align and tensor calls sample one bilinear tap pair per patch pixel.  A face 792 source pixels wide cut to 112 x 112 is a 7 : 1
// decimation: 2 of every 7 source rows and columns are read, the rest alias.  A filtered call writes each patch pixel as the mean of an
// Nx x Ny block of the UNFILTERED rule's samples instead.  With P x Q = out_width x out_height and max_factor 1 .. 8:
//
//   crop    (l, t, w, h) the crop rule's rect:            Nx = min(max_factor, max(1, ceil(w / P))),  Ny likewise with h and Q
//   align   (ux, uy), (vx, vy) the plan's Q16 vectors:    Nx = min(max_factor, max(1, ceil((|ux| + |uy|) / (P 65536)))),  Ny with v and Q
//           (the L1 norm never under-samples; upright, a12 == 1024, it is the crop's w / P)
//
// The fine patch F is, by definition, what the unfiltered rule of the same call gives for the same entry at Nx P x Ny Q: the crop's
// drawImage of the same rect with rx' = w / (Nx P), ry' = h / (Ny Q) (one binary64 division each); the align call's
// ht_align_term(i, Nx P, ..), ht_align_term(j, Ny Q, ..) with the same C, U, V, the range test and the four zero bytes of a sample outside
// the frame as they are.  Per channel, alpha included, with n = Nx Ny:
//
//   out(x, y) = (sum of F(Nx x + a, Ny y + b) over a < Nx, b < Ny  +  (n >> 1)) / n            (integer division)
//
// Consequences: Nx == Ny == 1 (max_factor 1, or a box that is not downscaled) is byte for byte the unfiltered call; where w == Nx P and
// h == Ny Q exactly the fine patch is the source block itself and the output its exact integer box mean; an empty entry is zeros; an
// aligned patch's edge fades where fine samples fall outside the frame.
//
// Host AND device text, as ht_crop_plan.h and ht_align_plan.h are: the kernels of ht_filter.hip compile these lines as device functions
// (HT_FILTER_FN is defined in front of the #include), tests/host/filter_plan_harness.cc compiles the SAME lines with
// g++ -fsanitize=address,undefined.  Bounds: w, h <= 2^14, P, Q <= 2^10; |ux| + |uy| <= 2^49 (ht_align_plan.h: each <= 2^48), P 65536 <= 2^26;
// a sum of n <= 64 bytes is < 2^14.  The fine patch is at most Nx P = 8192 wide, so the align term's product
// |(2i + 1 - P') UxS| < 2^13 2^48 = 2^61 stays inside int64 (ht_align_plan.h states 2^58 for P <= 2^10).
#pragma once

#include <stdint.h>

#include "headtrackr_hip.h"  // ht_crop_record, ht_align_record, HT_CROP_FACE, HT_ALIGN_FACE

#ifndef HT_FILTER_FN
#define HT_FILTER_FN inline
#endif

constexpr int32_t HT_FILTER_MIN_FACTOR = 1, HT_FILTER_MAX_FACTOR = 8;

// min(max_factor, max(1, ceil(num / den))); num >= 0, den > 0, max_factor >= 1
HT_FILTER_FN int32_t ht_filter_factor(int64_t num, int64_t den, int32_t max_factor) {
    const int64_t need = (num + den - 1) / den;
    return need < 1 ? 1 : need > max_factor ? max_factor : (int32_t)need;
}

// one axis of a crop entry: extent = the rect's width (height), out = P (Q)
HT_FILTER_FN int32_t ht_filter_crop_factor(int32_t extent, int32_t out, int32_t max_factor) { return ht_filter_factor(extent, out, max_factor); }

// one axis of an align entry: (a, b) = (ux, uy) with out = P, or (vx, vy) with out = Q
HT_FILTER_FN int32_t ht_filter_align_factor(int64_t a, int64_t b, int32_t out, int32_t max_factor) {
    const int64_t l1 = (a < 0 ? -a : a) + (b < 0 ? -b : b);
    return ht_filter_factor(l1, (int64_t)out * 65536, max_factor);
}

// one channel of one output pixel: the sum of its n fine samples, rounded half up
HT_FILTER_FN uint32_t ht_filter_mean(uint32_t sum, uint32_t n) { return (sum + (n >> 1)) / n; }

// four byte sums -> the pixel's RGBA8 dword
HT_FILTER_FN uint32_t ht_filter_pixel(const uint32_t sum[4], uint32_t n) {
    return ht_filter_mean(sum[0], n) | ht_filter_mean(sum[1], n) << 8 | ht_filter_mean(sum[2], n) << 16 | ht_filter_mean(sum[3], n) << 24;
}

// the arguments the two exported factor functions and the calls share
HT_FILTER_FN bool ht_filter_args_ok(int32_t out_width, int32_t out_height, int32_t max_factor) {
    return out_width >= 1 && out_width <= 1024 && out_height >= 1 && out_height <= 1024 && max_factor >= HT_FILTER_MIN_FACTOR && max_factor <= HT_FILTER_MAX_FACTOR;
}

// the factors of a record: 0, 0 for an empty one
HT_FILTER_FN void ht_filter_crop_record_factors(const ht_crop_record &r, int32_t P, int32_t Q, int32_t max_factor, int32_t *nx, int32_t *ny) {
    *nx = *ny = 0;
    if (r.code != HT_CROP_FACE) return;
    *nx = ht_filter_crop_factor(r.rect.width, P, max_factor), *ny = ht_filter_crop_factor(r.rect.height, Q, max_factor);
}
HT_FILTER_FN void ht_filter_align_record_factors(const ht_align_record &r, int32_t P, int32_t Q, int32_t max_factor, int32_t *nx, int32_t *ny) {
    *nx = *ny = 0;
    if (r.code != HT_ALIGN_FACE) return;
    *nx = ht_filter_align_factor(r.ux, r.uy, P, max_factor), *ny = ht_filter_align_factor(r.vx, r.vy, Q, max_factor);
}

// ht_gray.h — the project's ccv.grayscale byte of an RGBA8 dword (ccv.js:29), written once: g = R * 0.3 + G * 0.59 + B * 0.11 in binary64,
// three products and two sums each rounded on its own (never contracted into an FMA), round half to even, clamp (Uint8ClampedArray).
// The gray plane of the detector (ht_pyramid.hip) and the gray channel of the model-input patches (ht_patch_plan.h) compile THIS text.
//
// Host AND device text: a unit defines HT_GRAY_FN in front of the #include (ht_pyramid.hip: __device__ __forceinline__).  The device pass
// spells the operations __dmul_rn / __dadd_rn, as ht_pyramid.hip always did; a host compiler takes plain * and + and must be run with
// -ffp-contract=off (on x86-64 without -march flags it has no FMA to contract into anyway).
#pragma once

#include <stdint.h>

#ifndef HT_GRAY_FN
#define HT_GRAY_FN inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define HT_GRAY_MUL(a, b) __dmul_rn(a, b)
#define HT_GRAY_ADD(a, b) __dadd_rn(a, b)
#define HT_GRAY_CLAMP(q) min(max(q, 0), 255)
#else
#define HT_GRAY_MUL(a, b) ((a) * (b))
#define HT_GRAY_ADD(a, b) ((a) + (b))
#define HT_GRAY_CLAMP(q) ((q) < 0 ? 0 : (q) > 255 ? 255 : (q))
#endif

HT_GRAY_FN uint32_t ht_gray_of(uint32_t px) {  // ccv.js:29
    const double r = (double)(px & 0xffu), g = (double)((px >> 8) & 0xffu), b = (double)((px >> 16) & 0xffu);
    const double v = HT_GRAY_ADD(HT_GRAY_ADD(HT_GRAY_MUL(r, 0.3), HT_GRAY_MUL(g, 0.59)), HT_GRAY_MUL(b, 0.11));
    const int q = (int)__builtin_rint(v);  // round half to even (Uint8ClampedArray)
    return (uint32_t)HT_GRAY_CLAMP(q);
}

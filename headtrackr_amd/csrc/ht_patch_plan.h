// ht_patch_plan.h — the rule of the model-input patches (ht_camshift_crop_*_tensor_device / ht_camshift_align_*_tensor_device), without HIP:
// which element bits does a face patch become when a network reads it?
//
// DEFINITION.  A tensor call produces f(patch), where `patch` is, byte for byte, the RGBA8 patch the call of the same name without `_tensor`
// produces from the same arguments on the same tracker state (ht_crop_plan.h / ht_align_plan.h), and f works per pixel and per output
// channel c:
//   1. source byte b     HT_PATCH_RGB: bytes R, G, B of the pixel (c = 0, 1, 2); HT_PATCH_BGR: bytes B, G, R; HT_PATCH_GRAY: ONE channel, the
//                        ccv.grayscale byte of (R, G, B) (ccv.js:29, ht_gray.h: binary64 products and sums, round half to even, clamp).
//                        Alpha is dropped.
//   2. value             v = fl32(fl32((float)b * scale[c]) + bias[c]): two IEEE binary32 operations, each rounded to nearest even, never
//                        contracted into an FMA, subnormals kept.
//   3. element           HT_PATCH_F32: the bits of v.  HT_PATCH_F16: v rounded to binary16, nearest even, gradual underflow, overflow to
//                        infinity.  HT_PATCH_BF16: v rounded to bfloat16, nearest even: (u + 0x7fff + ((u >> 16) & 1)) >> 16 on v's bits u.
//   4. layout            HT_PATCH_CHW: C planes of out_height x out_width elements, packed.  HT_PATCH_HWC: C elements per pixel, packed.
// It FOLLOWS that an EMPTY entry (a lost or never tracked stream) is f of the zero byte in every element — bias[c] rounded to the dtype,
// not zero bytes —, and so is a pixel of an aligned patch whose sample centre lies outside the source (four zero bytes in RGBA).  Nothing in
// the tensor tells such an element from a black pixel: the record's `code` (ht_camshift_crop_result / ht_camshift_align_result) does.
//
// BOUNDS.  scale[c] and bias[c] are finite and each is 0 or has a magnitude in [2^-64, 2^64]; the slots of channels the mode does not
// have (gray: 1 and 2) are 0.  Then |b scale| is 0 or in [2^-64, 2^72) and the sum is 0 or at least one ulp of its larger operand, which is
// above 2^-88: no binary32 intermediate is subnormal, infinite or NaN, and step 2 is the same bits on every IEEE machine.
//
// Host AND device text, as ht_crop_plan.h and ht_align_plan.h are: k_cut_tensor / k_upright_tensor (ht_patch.hip) compile these lines as
// device functions (HT_PATCH_FN is defined in front of the #include), tests/host/patch_plan_harness.cc compiles the SAME lines with g++
// -ffp-contract=off, plain and under -fsanitize=address,undefined.  No library call and no HIP type.  One line differs by pass: the device
// takes binary16 from the hardware conversion (a _Float16 cast: v_cvt_f16_f32, round to nearest even, subnormals kept in hipcc's default
// kernel mode), a host compiler without _Float16 takes the integer text below; tests/test_gpu_patch_tensor.py holds the two together.
//
// Not part of this: an alpha or validity-mask channel, sub-pixel centres, a prefilter for strong downscales, per-entry formats,
// integer-quantised (int8) output.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "headtrackr_hip.h"  // ht_patch_format, HT_PATCH_*

#ifndef HT_PATCH_FN
#define HT_PATCH_FN inline
#endif
#ifndef HT_GRAY_FN
#define HT_GRAY_FN HT_PATCH_FN
#endif
#include "ht_gray.h"

enum {
    HT_PATCH_FMT_OK = 0,
    HT_PATCH_FMT_DTYPE,
    HT_PATCH_FMT_LAYOUT,
    HT_PATCH_FMT_CHANNELS,
    HT_PATCH_FMT_PAD,
    HT_PATCH_FMT_SCALE,
    HT_PATCH_FMT_BIAS,
    HT_PATCH_FMT_UNUSED,
};

inline const char *ht_patch_format_message(int code) {
    switch (code) {
    case HT_PATCH_FMT_DTYPE: return "unknown dtype";
    case HT_PATCH_FMT_LAYOUT: return "unknown layout";
    case HT_PATCH_FMT_CHANNELS: return "unknown channels value";
    case HT_PATCH_FMT_PAD: return "pad must be 0";
    case HT_PATCH_FMT_SCALE: return "scale must be finite and 0 or of a magnitude within 2^-64 .. 2^64";
    case HT_PATCH_FMT_BIAS: return "bias must be finite and 0 or of a magnitude within 2^-64 .. 2^64";
    case HT_PATCH_FMT_UNUSED: return "scale and bias of an unused channel must be 0";
    default: return "ok";
    }
}

HT_PATCH_FN uint32_t ht_patch_f32_bits(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

HT_PATCH_FN int ht_patch_nchannels(int channels) { return channels == HT_PATCH_GRAY ? 1 : 3; }
HT_PATCH_FN int ht_patch_esize(int dtype) { return dtype == HT_PATCH_F32 ? 4 : 2; }

// 0, or a magnitude within [2^-64, 2^64]: on the bits, so NaN and the infinities (exponent 255 > 191) fail without a comparison of floats
HT_PATCH_FN bool ht_patch_coef_ok(float v) {
    const uint32_t a = ht_patch_f32_bits(v) & 0x7fffffffu;
    return a == 0u || (a >= ((127u - 64u) << 23) && a <= ((127u + 64u) << 23));
}

HT_PATCH_FN int ht_patch_check_format(const ht_patch_format *f) {
    if (f->dtype != HT_PATCH_F32 && f->dtype != HT_PATCH_F16 && f->dtype != HT_PATCH_BF16) return HT_PATCH_FMT_DTYPE;
    if (f->layout != HT_PATCH_CHW && f->layout != HT_PATCH_HWC) return HT_PATCH_FMT_LAYOUT;
    if (f->channels != HT_PATCH_RGB && f->channels != HT_PATCH_BGR && f->channels != HT_PATCH_GRAY) return HT_PATCH_FMT_CHANNELS;
    if (f->pad != 0) return HT_PATCH_FMT_PAD;
    const int C = ht_patch_nchannels(f->channels);
    for (int c = 0; c < 3; c++) {
        if (c >= C) {
            if ((ht_patch_f32_bits(f->scale[c]) | ht_patch_f32_bits(f->bias[c])) & 0x7fffffffu) return HT_PATCH_FMT_UNUSED;
            continue;
        }
        if (!ht_patch_coef_ok(f->scale[c])) return HT_PATCH_FMT_SCALE;
        if (!ht_patch_coef_ok(f->bias[c])) return HT_PATCH_FMT_BIAS;
    }
    return HT_PATCH_FMT_OK;
}

// a patch's bytes, the default stride (the bytes rounded up to 4) and the byte offset of element (c, x, y) in a patch
HT_PATCH_FN size_t ht_patch_bytes(int w, int h, int dtype, int channels) { return (size_t)ht_patch_nchannels(channels) * (size_t)w * (size_t)h * (size_t)ht_patch_esize(dtype); }
HT_PATCH_FN size_t ht_patch_default_stride(size_t bytes) { return (bytes + 3) & ~(size_t)3; }
HT_PATCH_FN size_t ht_patch_offset(int w, int h, int dtype, int layout, int channels, int c, int x, int y) {
    const size_t C = (size_t)ht_patch_nchannels(channels), px = (size_t)y * (size_t)w + (size_t)x;
    return (layout == HT_PATCH_CHW ? (size_t)c * (size_t)w * (size_t)h + px : px * C + (size_t)c) * (size_t)ht_patch_esize(dtype);
}

// step 1: the source byte of output channel c of the RGBA8 dword px (R in the low byte)
HT_PATCH_FN uint32_t ht_patch_byte(uint32_t px, int channels, int c) {
    if (channels == HT_PATCH_GRAY) return ht_gray_of(px);
    return (px >> (8 * (channels == HT_PATCH_BGR ? 2 - c : c))) & 0xffu;
}

// step 2: two binary32 operations (the units that compile this are built with -ffp-contract=off)
HT_PATCH_FN float ht_patch_value(uint32_t b, float scale, float bias) {
    const float m = (float)b * scale;
    return m + bias;
}

// step 3, binary16: round to nearest even, gradual underflow, overflow to infinity
HT_PATCH_FN uint32_t ht_patch_f16_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 h = (_Float16)v;  // v_cvt_f16_f32
    uint16_t r;
    __builtin_memcpy(&r, &h, 2);
    return r;
#else
    const uint32_t u = ht_patch_f32_bits(v), sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return sign | 0x7e00u;  // NaN (the bounds exclude it)
    if (a >= 0x38800000u) {                      // 2^-14 and above: a normal binary16, or beyond its range
        const uint32_t r = a - 0x38000000u, q = a >= 0x47800000u ? 0x7c00u : (r + 0xfffu + ((r >> 13) & 1u)) >> 13;
        return sign | (q > 0x7c00u ? 0x7c00u : q);
    }
    const uint32_t e = a >> 23;
    if (e < 102u) return sign;  // below 2^-25: nearer to zero than to the smallest subnormal (2^-25 itself is the tie below, to even: zero)
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;  // 14 .. 24: units of 2^-24
    const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
#endif
}

// step 3, bfloat16 of a finite v: round to nearest even on the bits
HT_PATCH_FN uint32_t ht_patch_bf16_bits(float v) {
    const uint32_t u = ht_patch_f32_bits(v);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

HT_PATCH_FN uint32_t ht_patch_element(float v, int dtype) {
    return dtype == HT_PATCH_F32 ? ht_patch_f32_bits(v) : dtype == HT_PATCH_F16 ? ht_patch_f16_bits(v) : ht_patch_bf16_bits(v);
}

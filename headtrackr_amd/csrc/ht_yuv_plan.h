// ht_yuv_plan.h — the DECLARED YUV 4:2:0 -> RGBA conversion of the YUV ingest (ht_draw_frames_yuv / ht_draw_frames_yuv_device) and the
// validated plan of such a call, without HIP.  The reference has no YUV path (a browser's drawImage(video, ..) hides the conversion), so
// the conversion is declared here the way oracle/canvas_shim.js declares the resampler; it is integer-only and therefore the same bits
// on every machine.  With C = Y - yoff, D = U - 128, E = V - 128 (int32; >> is an arithmetic shift):
//
//     R = clamp((cy C         + crv E + 128) >> 8)     G = clamp((cy C + cgu D + cgv E + 128) >> 8)     B = clamp((cy C + cbu D + 128) >> 8)
//
// clamp to [0, 255], A = 255.  Chroma siting: the chroma sample of source pixel (x, y) is sample (x >> 1, y >> 1) of the FRAME (not of a
// source rect), replicated without interpolation; the chroma planes of a w x h frame are ceil(w / 2) x ceil(h / 2).
//
// Packed 4:2:2 (HT_YUV_FMT_YUYV = 4, HT_YUV_FMT_UYVY = 5: what an uncompressed webcam or a capture card delivers).  A frame is ONE plane;
// with cw = ceil(w / 2), row y holds cw macropixels of 4 bytes: YUYV Y(2m) U(m) Y(2m+1) V(m), UYVY U(m) Y(2m) V(m) Y(2m+1).  Pixel (x, y)
// takes its own Y byte and the U and V of macropixel (x >> 1) of ROW y of the frame: the 4:2:0 rule without the vertical halving, replicated
// and not interpolated.  The triple goes through the same ht_yuv_to_rgba and the same four matrices.  An odd width is legal: the last
// macropixel's second luma byte is in memory and never selected.  Layout: base and pitch multiples of 4 (a macropixel is one aligned
// dword), pitch >= 4 cw (0 = 4 cw), for n > 1 a frame stride that is a multiple of 4 and at least pitch (h - 1) + 4 cw; a tightly packed
// frame is 4 cw h bytes.  Formats 2, 3, 6 and everything else stay refused: the legal numbers are a predicate (ht_yuv_format_ok), not a range.
//
// Plain C++17: ht_ingest_yuv.hip compiles the scalar into its kernels and plans every call with ht_yuv_plan; the CPU suite compiles this
// header alone (tests/host/yuv_plan_harness.cc), also with AddressSanitizer + UBSan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HT_YUV_HD __host__ __device__
#else
#define HT_YUV_HD
#endif

constexpr int32_t HT_YUV_FMT_NV12 = 0, HT_YUV_FMT_I420 = 1;  // = HT_YUV_NV12 / HT_YUV_I420 of headtrackr_hip.h
constexpr int32_t HT_YUV_FMT_YUYV = 4, HT_YUV_FMT_UYVY = 5;  // = HT_YUV_YUYV / HT_YUV_UYVY: packed 4:2:2, one plane
HT_YUV_HD constexpr bool ht_yuv_is_422(int32_t format) { return format == HT_YUV_FMT_YUYV || format == HT_YUV_FMT_UYVY; }
HT_YUV_HD constexpr bool ht_yuv_format_ok(int32_t format) { return format == HT_YUV_FMT_NV12 || format == HT_YUV_FMT_I420 || ht_yuv_is_422(format); }
constexpr int32_t HT_YUV_NMATRICES = 4;
constexpr int32_t HT_YUV_MAX_DIM = 16384;  // as ht_draw_frames

struct HtYuvCoef {
    int32_t yoff, cy, crv, cgu, cgv, cbu;
};

// matrix 0 .. 3: BT.601 limited, BT.709 limited, BT.601 full, BT.709 full range.  Each is within 1 of the exact ITU matrix (binary64,
// rounded, clamped) over all 2^24 triples (tests/test_ingest_yuv_cpu.py re-derives that).
constexpr HtYuvCoef HT_YUV_COEF[HT_YUV_NMATRICES] = {
    {16, 298, 409, -100, -208, 516},
    {16, 298, 459, -55, -136, 541},
    {0, 256, 359, -88, -183, 454},
    {0, 256, 403, -48, -120, 475},
};

HT_YUV_HD inline uint32_t ht_yuv_clamp8(int32_t v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// one pixel as the RGBA8 dword the draw kernels read (R in the low byte).  No sum leaves int32: |cy C| < 2^17, |c E| < 2^17.
HT_YUV_HD inline uint32_t ht_yuv_to_rgba(int32_t y, int32_t u, int32_t v, const HtYuvCoef &k) {
    const int32_t c = k.cy * (y - k.yoff) + 128, d = u - 128, e = v - 128;
    const uint32_t r = ht_yuv_clamp8((c + k.crv * e) >> 8);
    const uint32_t g = ht_yuv_clamp8((c + k.cgu * d + k.cgv * e) >> 8);
    const uint32_t b = ht_yuv_clamp8((c + k.cbu * d) >> 8);
    return r | (g << 8) | (b << 16) | 0xff000000u;
}

// the same by matrix number; a matrix out of range gives 0 (no such pixel exists: A is 255 everywhere else)
inline uint32_t yuv_to_rgba(int32_t y, int32_t u, int32_t v, int32_t matrix) {
    if (matrix < 0 || matrix >= HT_YUV_NMATRICES) return 0u;
    return ht_yuv_to_rgba(y, u, v, HT_YUV_COEF[matrix]);
}

enum HtYuvPlanStatus {
    HT_YUV_PLAN_OK = 0,
    HT_YUV_PLAN_BAD_COUNT,    // n <= 0
    HT_YUV_PLAN_BAD_SIZE,     // width / height outside 1 .. 16384
    HT_YUV_PLAN_BAD_FORMAT,
    HT_YUV_PLAN_BAD_MATRIX,
    HT_YUV_PLAN_BAD_Y_PITCH,  // smaller than a row; 4:2:2: or not a multiple of 4
    HT_YUV_PLAN_BAD_C_PITCH,  // smaller than a chroma row, or odd for NV12
    HT_YUV_PLAN_BAD_STRIDE,   // n > 1 without a stride; smaller than a plane of one frame; odd for NV12; 4:2:2: not a multiple of 4
};

inline const char *ht_yuv_plan_message(int st) {
    switch (st) {
        case HT_YUV_PLAN_OK: return "ok";
        case HT_YUV_PLAN_BAD_COUNT: return "bad frame count";
        case HT_YUV_PLAN_BAD_SIZE: return "source width/height must be 1..16384";
        case HT_YUV_PLAN_BAD_FORMAT: return "format must be HT_YUV_NV12, HT_YUV_I420, HT_YUV_YUYV or HT_YUV_UYVY";
        case HT_YUV_PLAN_BAD_MATRIX: return "matrix must be 0..3 (HT_YUV_BT601_LIMITED .. HT_YUV_BT709_FULL)";
        case HT_YUV_PLAN_BAD_Y_PITCH: return "Y pitch smaller than a row (YUYV / UYVY: 4 ceil(w / 2) bytes, and a multiple of 4)";
        case HT_YUV_PLAN_BAD_C_PITCH: return "chroma pitch smaller than a chroma row, or odd for NV12";
        case HT_YUV_PLAN_BAD_STRIDE: return "frame stride missing for n > 1, smaller than a plane of one frame, odd for NV12, or not a multiple of 4 for YUYV / UYVY";
    }
    return "unknown";
}

struct HtYuvPlan {  // a validated source description
    int32_t cw, ch;                // chroma samples per row / chroma rows: ceil(w / 2), ceil(h / 2); 4:2:2: macropixels per row, h
    size_t c_row;                  // bytes of one chroma row of one chroma plane: 2 cw (NV12: U and V interleaved) or cw (I420); 4:2:2: 0
    size_t y_pitch, c_pitch;       // effective pitches
    size_t stride;                 // effective frame stride (0 only for n == 1)
    size_t y_extent, c_extent;     // bytes from a plane's base to the end of the last row of frame n - 1
    size_t packed_frame;           // bytes of one tightly packed frame: w h + 2 cw ch; 4:2:2: 4 cw h
};

// (frame_stride is added to EVERY plane pointer per frame, so it has to clear one frame of the Y plane and of a chroma plane; whether
// the planes of different frames interleave in one allocation is the caller's layout and needs no rule: the draw only reads them)
inline int ht_yuv_plan(int32_t width, int32_t height, int32_t format, int32_t matrix, size_t y_pitch, size_t c_pitch, size_t frame_stride, int32_t n,
                       HtYuvPlan *p) {
    if (n <= 0) return HT_YUV_PLAN_BAD_COUNT;
    if (width <= 0 || height <= 0 || width > HT_YUV_MAX_DIM || height > HT_YUV_MAX_DIM) return HT_YUV_PLAN_BAD_SIZE;
    if (!ht_yuv_format_ok(format)) return HT_YUV_PLAN_BAD_FORMAT;
    if (matrix < 0 || matrix >= HT_YUV_NMATRICES) return HT_YUV_PLAN_BAD_MATRIX;
    constexpr size_t LIM = (size_t)1 << 32;  // (n < 2^31 frames of < 2^32 bytes: every product below stays inside 64 bits)
    if (ht_yuv_is_422(format)) {  // one plane (y / y_pitch); c_pitch is not looked at and the chroma extent is 0: the overlap refusals see one plane
        p->cw = (width + 1) >> 1, p->ch = height;
        const size_t row = 4 * (size_t)p->cw;
        p->c_row = 0, p->c_pitch = 0, p->c_extent = 0;
        p->y_pitch = y_pitch ? y_pitch : row;
        if (p->y_pitch < row || (p->y_pitch & 3) || p->y_pitch > LIM) return HT_YUV_PLAN_BAD_Y_PITCH;
        if (frame_stride > LIM) return HT_YUV_PLAN_BAD_STRIDE;
        const size_t frame = p->y_pitch * (size_t)(height - 1) + row;
        p->stride = frame_stride;
        if (n > 1 && (frame_stride < frame || (frame_stride & 3))) return HT_YUV_PLAN_BAD_STRIDE;
        if (n == 1) p->stride = 0;  // never added
        p->y_extent = (size_t)(n - 1) * p->stride + frame;
        p->packed_frame = row * (size_t)height;
        return HT_YUV_PLAN_OK;
    }
    const bool nv12 = format == HT_YUV_FMT_NV12;
    p->cw = (width + 1) >> 1, p->ch = (height + 1) >> 1;
    p->c_row = nv12 ? 2 * (size_t)p->cw : (size_t)p->cw;
    p->y_pitch = y_pitch ? y_pitch : (size_t)width;
    if (p->y_pitch < (size_t)width) return HT_YUV_PLAN_BAD_Y_PITCH;
    p->c_pitch = c_pitch ? c_pitch : p->c_row;
    if (p->c_pitch < p->c_row || (nv12 && (p->c_pitch & 1))) return HT_YUV_PLAN_BAD_C_PITCH;
    // pitches are bounded only by size_t: refuse what would wrap the extents below (no plane of a real frame comes near)
    if (p->y_pitch > LIM || p->c_pitch > LIM || frame_stride > LIM) return p->y_pitch > LIM ? HT_YUV_PLAN_BAD_Y_PITCH : p->c_pitch > LIM ? HT_YUV_PLAN_BAD_C_PITCH : HT_YUV_PLAN_BAD_STRIDE;
    const size_t y_frame = p->y_pitch * (size_t)(height - 1) + (size_t)width, c_frame = p->c_pitch * (size_t)(p->ch - 1) + p->c_row;
    p->stride = frame_stride;
    if (n > 1 && (frame_stride < y_frame || frame_stride < c_frame || (nv12 && (frame_stride & 1)))) return HT_YUV_PLAN_BAD_STRIDE;
    if (n == 1) p->stride = 0;  // never added
    p->y_extent = (size_t)(n - 1) * p->stride + y_frame;
    p->c_extent = (size_t)(n - 1) * p->stride + c_frame;
    p->packed_frame = (size_t)width * (size_t)height + 2 * (size_t)p->cw * (size_t)p->ch;
    return HT_YUV_PLAN_OK;
}

// ht_draw_list_plan.h — the host side of ht_draw_list_device (one launch draws a list of per-feed sources, each with an allocation, size,
// format, matrix and rect of its own): a list is validated here and turned into the descriptors k_draw_list reads, without HIP.  The rules
// of an entry are those of ht_draw_frames_device (RGBA) and of ht_draw_frames_yuv_device (NV12 / I420 / YUYV / UYVY) with n = 1; the YUV rules are not
// restated: ht_yuv_plan (ht_yuv_plan.h) is asked.  The ratios rx = sw / W and ry = sh / H are ONE binary64 division each, done here, as
// oracle/canvas_shim.js divides them and as the single-source calls do on the host.
//
// Plain C++17: ht_draw_list.hip plans every call with ht_draw_list_plan; the CPU suite compiles this header alone
// (tests/host/draw_list_plan_harness.cc), also with AddressSanitizer + UBSan.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "headtrackr_hip.h"
#include "ht_yuv_plan.h"

constexpr int32_t HT_DRAW_LIST_MAX = 65535;  // entries of one call: the grid's z extent
static_assert(!ht_yuv_format_ok(HT_DRAW_RGBA), "the RGBA format number is no YUV format's");

// what a workgroup of k_draw_list reads for its entry (blockIdx.z): 104 bytes, pointers first.  PLANE: how a plane pointer is spelled — the
// host writes plain pointers, the kernel reads the same bytes as global-address-space pointers (ht_draw_list.hip)
template <class PLANE>
struct HtDrawDescT {
    PLANE p0, p1, p2;             // RGBA: p0.  NV12: Y, UV (p2 = p1).  I420: Y, U, V.  YUYV / UYVY: p0 (p1 = p2 = NULL)
    size_t pitch0, pitch1;        // effective pitches
    double rx, ry;                // sw / W, sh / H
    int32_t sx, sy, sw, sh;       // the source rect
    int32_t cw, format;           // chroma samples per row of the source (0 for RGBA; YUYV / UYVY: macropixels per row)
    HtYuvCoef kc;                 // the entry's matrix (zeros for RGBA)
};
typedef HtDrawDescT<const uint8_t *> HtDrawDesc;
static_assert(sizeof(HtDrawDesc) == 104, "descriptor layout");

// the bytes an entry's planes occupy, for the overlap refusals: base[k] == nullptr for a plane the format does not have.  A plane ends with
// its last ROW, not with a whole pitch.
struct HtDrawExtent {
    const void *base[3];
    size_t bytes[3];
};

enum HtDrawListStatus {
    HT_DRAW_LIST_OK = 0,
    HT_DRAW_LIST_BAD_COUNT,    // n outside 1 .. 65535, or no list
    HT_DRAW_LIST_BAD_CANVAS,   // W / H not positive
    HT_DRAW_LIST_BAD_FORMAT,
    HT_DRAW_LIST_BAD_SIZE,
    HT_DRAW_LIST_BAD_MATRIX,
    HT_DRAW_LIST_BAD_PITCH0,
    HT_DRAW_LIST_BAD_PITCH1,
    HT_DRAW_LIST_NULL_PLANE,
    HT_DRAW_LIST_MISALIGNED,   // RGBA / YUYV / UYVY base not a multiple of 4, NV12 chroma base odd
    HT_DRAW_LIST_BAD_RECT,
};

inline const char *ht_draw_list_message(int st) {
    switch (st) {
        case HT_DRAW_LIST_OK: return "ok";
        case HT_DRAW_LIST_BAD_COUNT: return "the list must hold 1..65535 entries";
        case HT_DRAW_LIST_BAD_CANVAS: return "no canvas geometry";
        case HT_DRAW_LIST_BAD_FORMAT: return "format must be HT_YUV_NV12, HT_YUV_I420, HT_YUV_YUYV, HT_YUV_UYVY or HT_DRAW_RGBA";
        case HT_DRAW_LIST_BAD_SIZE: return "source width/height must be 1..16384";
        case HT_DRAW_LIST_BAD_MATRIX: return "matrix must be 0..3 (HT_YUV_BT601_LIMITED .. HT_YUV_BT709_FULL)";
        case HT_DRAW_LIST_BAD_PITCH0: return "pitch0 smaller than a row (RGBA, YUYV, UYVY: or not a multiple of 4)";
        case HT_DRAW_LIST_BAD_PITCH1: return "chroma pitch smaller than a chroma row, or odd for NV12";
        case HT_DRAW_LIST_NULL_PLANE: return "NULL plane";
        case HT_DRAW_LIST_MISALIGNED: return "misaligned plane (RGBA, YUYV, UYVY: 4-byte alignment, NV12 chroma: an even address)";
        case HT_DRAW_LIST_BAD_RECT: return "source rect must lie wholly inside the source frame";
    }
    return "unknown";
}

// one entry: *d and *e are written only on success
inline int ht_draw_list_plan_entry(const ht_draw_source &s, int32_t W, int32_t H, HtDrawDesc *d, HtDrawExtent *e) {
    HtDrawDesc o = {};
    HtDrawExtent x = {};
    if (s.format == HT_DRAW_RGBA) {
        if (s.width <= 0 || s.height <= 0 || s.width > HT_YUV_MAX_DIM || s.height > HT_YUV_MAX_DIM) return HT_DRAW_LIST_BAD_SIZE;
        const size_t row = (size_t)s.width * 4;
        o.pitch0 = s.pitch0 ? s.pitch0 : row;
        if ((o.pitch0 & 3) || o.pitch0 < row || o.pitch0 > ((size_t)1 << 32)) return HT_DRAW_LIST_BAD_PITCH0;
        if (!s.p0) return HT_DRAW_LIST_NULL_PLANE;
        if ((uintptr_t)s.p0 & 3) return HT_DRAW_LIST_MISALIGNED;
        o.p0 = static_cast<const uint8_t *>(s.p0);
        x.base[0] = s.p0, x.bytes[0] = o.pitch0 * (size_t)(s.height - 1) + row;
    } else {
        HtYuvPlan p;
        switch (ht_yuv_plan(s.width, s.height, s.format, s.matrix, s.pitch0, s.pitch1, 0, 1, &p)) {
            case HT_YUV_PLAN_OK: break;
            case HT_YUV_PLAN_BAD_SIZE: return HT_DRAW_LIST_BAD_SIZE;
            case HT_YUV_PLAN_BAD_MATRIX: return HT_DRAW_LIST_BAD_MATRIX;
            case HT_YUV_PLAN_BAD_Y_PITCH: return HT_DRAW_LIST_BAD_PITCH0;
            case HT_YUV_PLAN_BAD_C_PITCH: return HT_DRAW_LIST_BAD_PITCH1;
            default: return HT_DRAW_LIST_BAD_FORMAT;  // (count and stride cannot fail for n = 1)
        }
        const bool nv12 = s.format == HT_YUV_FMT_NV12;
        if (ht_yuv_is_422(s.format)) {  // one plane: p1, p2 and pitch1 are not looked at
            if (!s.p0) return HT_DRAW_LIST_NULL_PLANE;
            if ((uintptr_t)s.p0 & 3) return HT_DRAW_LIST_MISALIGNED;
            o.p0 = static_cast<const uint8_t *>(s.p0);
        } else {
            if (!s.p0 || !s.p1 || (!nv12 && !s.p2)) return HT_DRAW_LIST_NULL_PLANE;
            if (nv12 && ((uintptr_t)s.p1 & 1)) return HT_DRAW_LIST_MISALIGNED;
            o.p0 = static_cast<const uint8_t *>(s.p0), o.p1 = static_cast<const uint8_t *>(s.p1);
            o.p2 = nv12 ? o.p1 : static_cast<const uint8_t *>(s.p2);
            x.base[1] = s.p1, x.bytes[1] = p.c_extent;
            if (!nv12) x.base[2] = s.p2, x.bytes[2] = p.c_extent;
        }
        o.pitch0 = p.y_pitch, o.pitch1 = p.c_pitch, o.cw = p.cw, o.kc = HT_YUV_COEF[s.matrix];
        x.base[0] = s.p0, x.bytes[0] = p.y_extent;
    }
    o.format = s.format;
    o.sx = o.sy = 0, o.sw = s.width, o.sh = s.height;
    const ht_cs_rect &r = s.rect;
    if (r.width != 0 || r.height != 0) {
        if (r.x < 0 || r.y < 0 || r.width <= 0 || r.height <= 0 || r.width > s.width - r.x || r.height > s.height - r.y) return HT_DRAW_LIST_BAD_RECT;
        o.sx = r.x, o.sy = r.y, o.sw = r.width, o.sh = r.height;
    }
    o.rx = (double)o.sw / (double)W, o.ry = (double)o.sh / (double)H;  // canvas_shim.js: one binary64 division each
    *d = o, *e = x;
    return HT_DRAW_LIST_OK;
}

// the whole list onto a W x H canvas: desc[n] and ext[n] are complete on HT_DRAW_LIST_OK; otherwise *bad = the first offending entry
// (-1 when the fault is the call's, not an entry's) and desc / ext hold the entries before it
inline int ht_draw_list_plan(const ht_draw_source *srcs, int32_t n, int32_t W, int32_t H, HtDrawDesc *desc, HtDrawExtent *ext, int32_t *bad) {
    *bad = -1;
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return HT_DRAW_LIST_BAD_COUNT;
    if (W <= 0 || H <= 0) return HT_DRAW_LIST_BAD_CANVAS;
    for (int32_t i = 0; i < n; i++) {
        const int st = ht_draw_list_plan_entry(srcs[i], W, H, desc + i, ext + i);
        if (st != HT_DRAW_LIST_OK) {
            *bad = i;
            return st;
        }
    }
    return HT_DRAW_LIST_OK;
}

// the first entry one of whose planes meets [dst, dst + nbytes), or -1
inline int32_t ht_draw_list_overlap(const HtDrawExtent *ext, int32_t n, const void *dst, size_t nbytes) {
    const uintptr_t d = (uintptr_t)dst;
    if (!dst || !nbytes) return -1;
    for (int32_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const uintptr_t b = (uintptr_t)ext[i].base[k];
            if (b && b < d + nbytes && d < b + ext[i].bytes[k]) return i;
        }
    return -1;
}

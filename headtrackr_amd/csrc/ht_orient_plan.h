// ht_orient_plan.h — the orientation of an ingested source (rotated and mirrored feeds: a phone in portrait, a hardware decoder's surface as
// stored, a mirrored selfie camera): the rule, and the host side of a draw-list entry that carries one, without HIP.
//
// Orientation k is 0 .. 7: rot = k & 3 counts the quarter turns CLOCKWISE that bring the stored frame upright, flip = k >> 2 is a horizontal
// mirror applied AFTER the turn.  A stored frame S of w x h gives the oriented frame O of ow x oh = (w, h) for even rot, (h, w) for odd rot.
// The mapping is a pure index permutation: with x' = flip ? ow - 1 - x : x, O(x, y) = S(u, v) and
//
//     rot 0: (u, v) = (x', y)      rot 1: (y, h - 1 - x')      rot 2: (w - 1 - x', h - 1 - y)      rot 3: (w - 1 - y, x')
//
// (numpy: np.rot90(S, -rot), then np.fliplr if flip).  Every call that takes an oriented entry gives, byte for byte, what it gives on the
// RGBA frame O = orient(convert(S)): YUV chroma is sited by the STORED frame (u >> 1, v >> 1; 4:2:2: the macropixel of stored row v) exactly
// as without an orientation, conversion first, permutation second; source rects, crop boxes and records are in O's coordinates.
//
// k rides in bits 8 .. 10 of the `format` field of ht_draw_source and ht_yuv_frames (HT_ORIENT(k) of headtrackr_hip.h); a value with any
// bit from 11 up is no format.  ht_draw_list_plan_entry and ht_yuv_plan are not touched: the bits are stripped here and they are asked about
// the STORED frame; the rect is validated against O (a rect inside O but outside S is legal, the converse is refused), the extents for
// the overlap refusals are the stored planes'.  The descriptor k_draw_list_oriented reads is HtDrawDesc (104 bytes, unchanged: the stored
// planes, pitches, cw, matrix, stored size in sw / sh, and the ratios of the ORIENTED rect) with the orientation, the destination frame and the
// oriented rect behind it, the way HtDrawMeanDesc wraps it.
//
// Plain C++17, shared as text by the host (ht_draw_list.hip, ht_ingest_yuv.hip, ht_draw_filter.hip, ht_face_calls.hip) and the device
// (ht_orient_kernels.hip); the CPU suite compiles this header alone (tests/host/orient_plan_harness.cc), also with AddressSanitizer + UBSan.
#pragma once

#include "ht_draw_list_plan.h"

#if defined(__HIPCC__)
#define HT_ORIENT_HD __host__ __device__
#else
#define HT_ORIENT_HD
#endif

static_assert(HT_ORIENT(0) == 0 && HT_ORIENT(7) == 0x700 && HT_ORIENT_OF(HT_DRAW_RGBA | HT_ORIENT(5)) == 5 && HT_FORMAT_OF(HT_DRAW_RGBA | HT_ORIENT(5)) == HT_DRAW_RGBA,
              "the orientation is bits 8..10 of a format");
constexpr int32_t HT_ORIENT_BITS = 0x7ff;  // the bits a format may use: the format number and the orientation

// a format field taken apart.  A value that uses a bit from 11 up (or the sign) is handed on whole as the base: no format, refused as one
HT_ORIENT_HD inline void ht_orient_split(int32_t format, int32_t *base, int32_t *k) {
    if (format & ~HT_ORIENT_BITS) *base = format, *k = 0;
    else *base = HT_FORMAT_OF(format), *k = HT_ORIENT_OF(format);
}
inline bool ht_orient_present(int32_t format) { return (format & ~0xff) != 0; }  // any bit above the format number: the entry goes through this header

HT_ORIENT_HD inline void ht_orient_size(int32_t k, int32_t w, int32_t h, int32_t *ow, int32_t *oh) { *ow = (k & 1) ? h : w, *oh = (k & 1) ? w : h; }

// O(x, y) = S(u, v); (w, h): the stored frame
HT_ORIENT_HD inline void ht_orient_map(int32_t k, int32_t w, int32_t h, int32_t x, int32_t y, int32_t *u, int32_t *v) {
    const int32_t rot = k & 3, ow = (k & 1) ? h : w, xp = (k >> 2) ? ow - 1 - x : x;
    switch (rot) {
        case 0: *u = xp, *v = y; break;
        case 1: *u = y, *v = h - 1 - xp; break;
        case 2: *u = w - 1 - xp, *v = h - 1 - y; break;
        default: *u = w - 1 - y, *v = xp; break;
    }
}

// what a workgroup of k_draw_list_oriented reads for its entry: 128 bytes
template <class PLANE>
struct HtOrientDescT {
    HtDrawDescT<PLANE> d;    // the STORED frame: planes, pitches, cw, format (the bare number), matrix; sx = sy = 0, sw x sh = w x h; rx, ry: orw / W, orh / H
    int32_t orient, frame;   // k; the destination frame the entry lands on
    int32_t ox, oy, orw, orh;  // the source rect, in O's coordinates
};
typedef HtOrientDescT<const uint8_t *> HtOrientDesc;
static_assert(sizeof(HtOrientDesc) == 128 && alignof(HtOrientDesc) == 8 && sizeof(HtDrawDesc) == 104, "descriptor layout");

// a rect (width == 0 && height == 0: the whole frame) against O: false when it does not lie wholly inside
inline bool ht_orient_rect(int32_t k, int32_t w, int32_t h, const ht_cs_rect *r, int32_t *ox, int32_t *oy, int32_t *orw, int32_t *orh) {
    int32_t ow, oh;
    ht_orient_size(k, w, h, &ow, &oh);
    *ox = *oy = 0, *orw = ow, *orh = oh;
    if (r && (r->width != 0 || r->height != 0)) {
        if (r->x < 0 || r->y < 0 || r->width <= 0 || r->height <= 0 || r->width > ow - r->x || r->height > oh - r->y) return false;
        *ox = r->x, *oy = r->y, *orw = r->width, *orh = r->height;
    }
    return true;
}

// one entry onto a W x H destination: ht_draw_list_plan_entry's statuses; *d and *e are written only on success (d->frame is left 0)
inline int ht_orient_plan_entry(const ht_draw_source &s, int32_t W, int32_t H, HtOrientDesc *d, HtDrawExtent *e) {
    HtOrientDesc o = {};
    HtDrawExtent x = {};
    ht_draw_source stored = s;
    ht_orient_split(s.format, &stored.format, &o.orient);
    stored.rect = ht_cs_rect{0, 0, 0, 0};  // the rect is O's: the stored frame is asked about as a whole
    const int st = ht_draw_list_plan_entry(stored, W, H, &o.d, &x);
    if (st != HT_DRAW_LIST_OK) return st;
    if (!ht_orient_rect(o.orient, s.width, s.height, &s.rect, &o.ox, &o.oy, &o.orw, &o.orh)) return HT_DRAW_LIST_BAD_RECT;
    o.d.rx = (double)o.orw / (double)W, o.d.ry = (double)o.orh / (double)H;  // canvas_shim.js: one binary64 division each
    *d = o, *e = x;
    return HT_DRAW_LIST_OK;
}

// the descriptor k_draw_list reads for an entry of orientation 0: ht_draw_list_plan_entry's own
inline HtDrawDesc ht_orient_as_plain(const HtOrientDesc &o) {
    HtDrawDesc d = o.d;
    d.sx = o.ox, d.sy = o.oy, d.sw = o.orw, d.sh = o.orh;
    return d;
}

// the whole list: ht_draw_list_plan's contract.  Entry i lands on frame i
inline int ht_orient_plan(const ht_draw_source *srcs, int32_t n, int32_t W, int32_t H, HtOrientDesc *desc, HtDrawExtent *ext, int32_t *bad) {
    *bad = -1;
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return HT_DRAW_LIST_BAD_COUNT;
    if (W <= 0 || H <= 0) return HT_DRAW_LIST_BAD_CANVAS;
    for (int32_t i = 0; i < n; i++) {
        const int st = ht_orient_plan_entry(srcs[i], W, H, desc + i, ext + i);
        if (st != HT_DRAW_LIST_OK) {
            *bad = i;
            return st;
        }
        desc[i].frame = i;
    }
    return HT_DRAW_LIST_OK;
}

// the 1 : 1 draw of the WHOLE of O onto a frame of O's own size, for the calls that orient first (the filtered draw, the face-patch calls):
// at ratio 1 every tap weight is (1, 0), so the frame drawn is O itself
inline HtOrientDesc ht_orient_whole(const HtOrientDesc &o) {
    HtOrientDesc j = o;
    j.frame = 0, j.ox = j.oy = 0;
    ht_orient_size(o.orient, o.d.sw, o.d.sh, &j.orw, &j.orh);
    j.d.rx = j.d.ry = 1.0;
    return j;
}

// the RGBA entry of O that an oriented entry becomes once its frame has been drawn 1 : 1 into `frame` (ow x oh packed rows): the rect stays
inline ht_draw_source ht_orient_upright(const ht_draw_source &s, int32_t k, const void *frame) {
    ht_draw_source u = s;
    ht_orient_size(k, s.width, s.height, &u.width, &u.height);
    u.p0 = frame, u.p1 = u.p2 = nullptr, u.pitch0 = (size_t)u.width * 4, u.pitch1 = 0, u.format = HT_DRAW_RGBA, u.matrix = 0;
    return u;
}

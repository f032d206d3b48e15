// ht_draw_dest_plan.h — where a canvas-draw call writes: the destination of the four device entry points (the two host forms always bind)
// resolved once, without HIP.  A call either BINDS (dst_dev == NULL: n packed frames into the context's own frame buffer, which become the
// bound frames) or writes n frames `stride` bytes apart into the caller's buffer.  Either way it writes [base, base + bytes): (n - 1) stride +
// fbytes from dst_dev, or — the own buffer may be freed and grown for the call — max(own_bytes, fbytes n) from the own buffer's base as it is
// now; the calls ask ht_draw_list_overlap (ht_draw_list_plan.h) about that range with their sources' extents.
//
// The checks are the same for every call; their ORDER is each call's own and is kept as it is (HtDrawCallKind):
//   FRAMES           [pointers: source and destination alignment in one check]  then  bind: capacity   |  caller's buffer: stride
//   YUV              [alignment]                                                then  bind: capacity   |  caller's buffer: stride
//   LIST, FILTERED   [alignment] [stride, caller's buffer only] [the entries]   then  bind: capacity
// "the entries" / "the source pointer": the caller's findings, handed in as source_fault.  A stride given with dst_dev == NULL is not looked at.
//
// Plain C++17: ht_draw_calls.hip resolves every call with ht_draw_dest_plan; the CPU suite compiles this header alone
// (tests/host/draw_dest_plan_harness.cc), also with AddressSanitizer + UBSan.
#pragma once

#include "ht_draw_list_plan.h"

enum HtDrawCallKind { HT_DRAW_CALL_FRAMES = 0, HT_DRAW_CALL_YUV, HT_DRAW_CALL_LIST, HT_DRAW_CALL_LIST_FILTERED };
inline bool ht_draw_call_is_list(int kind) { return kind == HT_DRAW_CALL_LIST || kind == HT_DRAW_CALL_LIST_FILTERED; }

enum HtDrawDestStatus {
    HT_DRAW_DEST_OK = 0,
    HT_DRAW_DEST_MISALIGNED,  // dst_dev not a multiple of 4; FRAMES: or the source pointer's fault (one check, one message)
    HT_DRAW_DEST_BAD_STRIDE,  // caller's buffer: smaller than a frame or not a multiple of 4
    HT_DRAW_DEST_SOURCES,     // LIST, FILTERED: the caller's source_fault, at its place in the order (the message is the caller's)
    HT_DRAW_DEST_CAPACITY,    // bind form: n above the geometry's batch capacity
};

struct HtDrawDest {
    bool bind;         // into the own buffer, bound on success
    size_t fbytes;     // bytes of one destination frame: 4 W H
    size_t stride;     // effective: fbytes in the bind form and for a stride of 0
    const void *base;  // the range the call will write
    size_t bytes;
};

// *d is complete on HT_DRAW_DEST_OK.  W, H: the canvas (positive: the calls test the geometry first), n >= 1
inline int ht_draw_dest_plan(int kind, int32_t W, int32_t H, int32_t n, const void *dst_dev, size_t dst_frame_stride, int32_t max_batch, const void *own_base,
                             size_t own_bytes, bool source_fault, HtDrawDest *d) {
    const bool list = ht_draw_call_is_list(kind);
    d->bind = !dst_dev;
    d->fbytes = (size_t)W * (size_t)H * 4;
    d->stride = dst_dev && dst_frame_stride ? dst_frame_stride : d->fbytes;
    const bool bad_stride = (d->stride & 3) || d->stride < d->fbytes;
    if (((uintptr_t)dst_dev & 3) || (kind == HT_DRAW_CALL_FRAMES && source_fault)) return HT_DRAW_DEST_MISALIGNED;
    if (list && bad_stride) return HT_DRAW_DEST_BAD_STRIDE;
    if (list && source_fault) return HT_DRAW_DEST_SOURCES;
    if (d->bind && n > max_batch) return HT_DRAW_DEST_CAPACITY;
    if (bad_stride) return HT_DRAW_DEST_BAD_STRIDE;
    d->base = d->bind ? own_base : dst_dev;
    d->bytes = d->bind ? (own_bytes > d->fbytes * (size_t)n ? own_bytes : d->fbytes * (size_t)n) : (size_t)(n - 1) * d->stride + d->fbytes;
    return HT_DRAW_DEST_OK;
}

// a refusal the call makes only behind its first use of the device (made current; a list probes the oriented draw's module), not in front
inline bool ht_draw_dest_behind_device(int kind, int st) { return st == HT_DRAW_DEST_CAPACITY || (st == HT_DRAW_DEST_BAD_STRIDE && !ht_draw_call_is_list(kind)); }

inline const char *ht_draw_dest_message(int kind, int st) {
    switch (st) {
        case HT_DRAW_DEST_OK: return "ok";
        case HT_DRAW_DEST_MISALIGNED:
            return kind == HT_DRAW_CALL_FRAMES ? "NULL source or misaligned pointer (4-byte alignment required)" : "misaligned destination (4-byte alignment required)";
        case HT_DRAW_DEST_BAD_STRIDE: return "destination frame stride smaller than a frame or not a multiple of 4";
        case HT_DRAW_DEST_SOURCES: return "a source is refused";
        case HT_DRAW_DEST_CAPACITY:  // (a list call names entry max_batch, the first that does not fit, in front)
            return ht_draw_call_is_list(kind) ? "more entries than the geometry's batch capacity" : "more frames than the geometry's batch capacity";
    }
    return "unknown";
}

// a source that meets the range the call will write (ht_draw_list_overlap on HtDrawDest's base and bytes; a list call names the entry in front)
inline const char *ht_draw_dest_overlap_message(int kind, bool bind) {
    if (kind == HT_DRAW_CALL_FRAMES) return bind ? "the source lies inside the context's own frame buffer" : "source and destination overlap";
    return bind ? "a source plane lies inside the context's own frame buffer" : "a source plane and the destination overlap";
}

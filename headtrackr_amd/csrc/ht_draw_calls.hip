// ht_draw_calls.hip — the host path of the six canvas-draw calls (ht_draw_frames, ht_draw_frames_yuv, their _device forms, ht_draw_list_device,
// ht_draw_list_filtered_device) and ht_draw_filter_factors, written once.  Included last in ht_ingest.hip, behind ht_draw_filter.hip: every
// kernel's launcher is defined by then and nothing is declared ahead of its definition (but dm_unpack_sources, which ht_face_calls.hip calls).
//
// A call: check its sources (ig_check, igy_check, the list plans), resolve its destination (ht_draw_dest_plan.h: the checks, in each call's
// own order), ask ht_draw_list_overlap about the range it will write, and draw_into the context's own frame buffer — bound on success — or
// the caller's.  Shared besides: ONE reserve of the ingest staging buffer, n frames of one description as list entries, the upright-first pass.
#include "ht_draw_dest_plan.h"

namespace {

// the context's ingest staging buffer holds >= need bytes.  A reallocation waits for the work in flight first, like every one of the library
ht_status draw_stage_reserve(ht_ctx *c, const char *fn, size_t need, const char *what) {
    if (c->ingest_src_cap >= need) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_ingest_src) (void)hipFree(c->d_ingest_src);
    c->d_ingest_src = nullptr, c->ingest_src_cap = 0;
    if (hipMalloc(reinterpret_cast<void **>(&c->d_ingest_src), need) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": hipMalloc failed (" + what + ")");
    }
    c->ingest_src_cap = need;
    return HT_OK;
}

// launch(dst, stride) into the resolved destination; bind form: the context's own frame buffer, bound on success.  Every argument error has been
// reported before anything is touched; a HIP failure here (hipMalloc for a buffer that has to grow: HT_ERR_NOMEM; the launch: HT_ERR_HIP) leaves the
// context usable but, when the buffer had to grow, without bound frames; the launch is ordered on the ctx stream behind every reader of that buffer
template <class LAUNCH>
ht_status draw_into(ht_ctx *c, const char *fn, const HtDrawDest &d, int32_t n, void *dst_dev, const LAUNCH &launch) {
    if (!d.bind) return launch(static_cast<uint8_t *>(dst_dev), d.stride);
    ht_status st = ht_frames_own_reserve(c, d.fbytes * (size_t)n, fn);
    if (st != HT_OK) return st;
    if ((st = launch(c->d_frames_own, d.fbytes)) != HT_OK) return st;
    ht_frames_bind_own(c, n);
    return HT_OK;
}

struct DrawSources {  // what a device call found about its sources
    const HtDrawExtent *ext;  // their extents, for the overlap refusal
    int32_t next;
    bool fault;               // FRAMES: the source pointer's; a list call's: entry `bad` with the plan's message (where: ht_draw_dest_plan.h)
    int32_t bad;
    const char *message;
};

// a device call behind its sources' checks: the destination resolved in the kind's order, the device made current (module: the call needs the
// oriented draw's; a missing one is reported before anything is touched), the overlap refusal against the range the call will write (the own
// buffer as it is now and as far as this call writes it: defensive only, its address is handed to nobody), then draw_into
template <class LAUNCH>
ht_status draw_resolved(ht_ctx *c, int kind, const char *fn, int32_t n, void *dst_dev, size_t dst_frame_stride, const DrawSources &src, bool module, const LAUNCH &launch) {
    const auto refuse = [&](int32_t entry, const char *text) {  // a list call names the entry in front
        return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": " + (entry >= 0 && ht_draw_call_is_list(kind) ? "entry " + std::to_string(entry) + ": " : std::string()) + text);
    };
    HtDrawDest d;
    const int ds = ht_draw_dest_plan(kind, c->W, c->H, n, dst_dev, dst_frame_stride, c->max_batch, c->d_frames_own, c->d_frames_own_bytes, src.fault, &d);
    if (ds == HT_DRAW_DEST_SOURCES) return refuse(src.bad, src.message);
    if (ds != HT_DRAW_DEST_OK && !ht_draw_dest_behind_device(kind, ds)) return refuse(-1, ht_draw_dest_message(kind, ds));
    HT_HIP(c, hipSetDevice(c->device));
    const OrModule *m = nullptr;
    const ht_status st = module ? or_module(c, fn, &m) : HT_OK;
    if (st != HT_OK) return st;
    if (ds != HT_DRAW_DEST_OK) return refuse(ds == HT_DRAW_DEST_CAPACITY ? c->max_batch : -1, ht_draw_dest_message(kind, ds));
    const int32_t bad = ht_draw_list_overlap(src.ext, src.next, d.base, d.bytes);
    if (bad >= 0) return refuse(bad, ht_draw_dest_overlap_message(kind, d.bind));
    return draw_into(c, fn, d, n, dst_dev, launch);
}

template <class LAUNCH>
ht_status draw_bound(ht_ctx *c, const char *fn, int32_t n, const LAUNCH &launch) {  // the host forms: always the bind form, n packed frames
    const size_t fbytes = (size_t)c->W * c->H * 4;
    return draw_into(c, fn, HtDrawDest{true, fbytes, fbytes, nullptr, 0}, n, nullptr, launch);
}

// the host forms behind their own checks: NULL, the batch capacity (always the bind form), then the staging buffer for the copy
ht_status draw_stage_host(ht_ctx *c, int kind, const char *fn, const void *host, int32_t n, size_t need) {
    if (!host) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": NULL source");
    if (n > c->max_batch) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": " + ht_draw_dest_message(kind, HT_DRAW_DEST_CAPACITY));
    HT_HIP(c, hipSetDevice(c->device));
    return draw_stage_reserve(c, fn, need, "source staging");
}

// ht_draw_frames_yuv*: frame f of the n frames of one description as a list entry, with the source rect — or, for an oriented call, whose
// rect is the oriented descriptor's, the stored frame as a whole
HtDrawDesc igy_entry(const IgYuvCall &q, const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t f, double rx, double ry) {
    const HtYuvPlan &p = q.plan;
    HtDrawDesc d = {};
    d.p0 = y + (size_t)f * p.stride, d.pitch0 = p.y_pitch, d.rx = rx, d.ry = ry;
    if (!ht_yuv_is_422(q.format)) d.p1 = u + (size_t)f * p.stride, d.p2 = q.format == HT_YUV_FMT_NV12 ? d.p1 : v + (size_t)f * p.stride, d.pitch1 = p.c_pitch;
    if (q.orient) d.sw = q.width, d.sh = q.height;
    else d.sx = q.sx, d.sy = q.sy, d.sw = q.sw, d.sh = q.sh;
    d.cw = p.cw, d.format = q.format, d.kc = HT_YUV_COEF[q.matrix];
    return d;
}

// The UNFILTERED draw of descriptors that hold packed 4:2:2 entries (a list's, or the n frames of a packed ht_draw_frames_yuv* call).  The
// packed pixel body lives in ht_draw_filter.hip's kernel alone (every other kernel is held to the registers it has), and factors (1, 1) are
// ht_draw_list_device's bytes by the declared rule: the same taps, one sample per pixel, (s + 0) / 1.  profiles/ingest_422.txt has the cost.
ht_status dm_launch_unfiltered(ht_ctx *c, const char *fn, const std::vector<HtDrawDesc> &desc, uint8_t *dst, size_t dstride) {
    std::vector<HtDrawMeanDesc> m(desc.size());
    for (size_t i = 0; i < desc.size(); i++) m[i].d = desc[i], m[i].nx = m[i].ny = 1;
    return dm_launch(c, fn, m, dst, dstride);
}

// an oriented call: one descriptor per frame through the module's kernel; a packed one: likewise through the one kernel that holds the
// packed pixel body (its timer); NV12 / I420 as stored: k_draw_yuv<>
ht_status igy_launch(ht_ctx *c, const char *fn, const IgYuvCall &q, const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, uint8_t *dst, size_t dstride) {
    if (!q.orient && !ht_yuv_is_422(q.format)) return igy_launch_planar(c, q, y, u, v, n, dst, dstride);
    const double rx = (double)q.sw / (double)c->W, ry = (double)q.sh / (double)c->H;  // canvas_shim.js: one binary64 division each
    std::vector<HtDrawDesc> desc((size_t)n);
    std::vector<HtOrientDesc> odesc(q.orient ? (size_t)n : 0);
    for (int32_t f = 0; f < n; f++) {
        desc[(size_t)f] = igy_entry(q, y, u, v, f, rx, ry);
        if (q.orient) odesc[(size_t)f] = HtOrientDesc{desc[(size_t)f], q.orient, f, q.sx, q.sy, q.sw, q.sh};
    }
    return q.orient ? or_launch(c, fn, odesc, dst, dstride) : dm_launch_unfiltered(c, fn, desc, dst, dstride);
}

// An entry a call's kernel cannot read as stored — an oriented entry (orient[i] != 0; orient NULL: none) of a face-patch call or of the
// filtered draw, whose kernels hold no orientation, and (packed_too) a packed 4:2:2 entry of a face-patch call, whose kernels hold no packed
// body — is drawn upright FIRST: its whole frame 1 : 1 — every tap weight (1, 0), so the frame drawn is the declared conversion itself,
// O = orient(convert(S)); an oriented packed entry is ONE pass, not two — onto an RGBA frame of SW x SH, O's size, carved from the context's
// staging buffer, and the entry becomes the RGBA entry of that frame: p0 the frame, rect and ratios as they were (the same bytes and the same
// record by the calls' own contract).  Oriented entries first (one table, or_upright), then the packed ones in list order (k_draw_list_mean_tile
// at factors (1, 1), one dm_launch each: the frames have sizes of their own): one more launch and the whole frame at 4 B/px per such entry, which
// a list without one never pays.  desc: (stored planes, O's size) per entry — ht_face_calls.hip's own descriptors, or dm_orient_first's
ht_status dm_unpack_sources(ht_ctx *c, const char *fn, std::vector<HtCropDesc> &desc, const int32_t *orient, bool packed_too) {
    const auto turned = [&](size_t i) { return orient && orient[i] != 0; };
    const auto packed = [&](size_t i) { return packed_too && !turned(i) && ht_yuv_is_422(desc[i].d.format); };
    size_t need = 0, at = 0;
    for (size_t i = 0; i < desc.size(); i++)
        if (turned(i) || packed(i)) need += (size_t)desc[i].SW * (size_t)desc[i].SH * 4;
    if (!need) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st = draw_stage_reserve(c, fn, need, packed_too ? "unpacked 4:2:2 / oriented sources" : "oriented sources");
    if (st != HT_OK) return st;
    const auto whole = [&](size_t i) {  // the stored frame as a whole at ratio 1 (its size back from O's: the swap is its own inverse)
        HtDrawDesc d = desc[i].d;
        ht_orient_size(orient ? orient[i] : 0, desc[i].SW, desc[i].SH, &d.sw, &d.sh);
        d.sx = d.sy = 0, d.rx = d.ry = 1.0;
        return d;
    };
    const auto upright = [&](size_t i) {  // entry i's frame, and the entry as the RGBA entry of it
        HtCropDesc &e = desc[i];
        uint8_t *frame = c->d_ingest_src + at;
        at += (size_t)e.SW * (size_t)e.SH * 4;
        e.d.p0 = frame, e.d.p1 = e.d.p2 = nullptr, e.d.pitch0 = (size_t)e.SW * 4, e.d.pitch1 = 0, e.d.cw = 0, e.d.format = HT_DRAW_RGBA, e.d.kc = HtYuvCoef{};
        return frame;
    };
    std::vector<HtOrientDesc> jobs;
    std::vector<uint8_t *> frames;
    for (size_t i = 0; i < desc.size(); i++) {
        if (!turned(i)) continue;
        HtOrientDesc o = {};
        o.d = whole(i), o.orient = orient[i];
        jobs.push_back(ht_orient_whole(o));
        frames.push_back(upright(i));
    }
    if ((st = or_upright(c, fn, jobs, frames)) != HT_OK) return st;
    std::vector<HtDrawMeanDesc> one(1);
    for (size_t i = 0; i < desc.size(); i++) {
        if (!packed(i)) continue;
        one[0] = HtDrawMeanDesc{whole(i), 1, 1};
        if ((st = dm_launch(c, fn, one, upright(i), 0, desc[i].SW, desc[i].SH)) != HT_OK) return st;
    }
    return HT_OK;
}

// The filtered draw of a list that holds oriented entries (odesc: ht_orient_plan's, every check of the call passed): each oriented entry is
// planned as the RGBA entry of its O, with the rect it had — the call's bytes by its own definition; the others, packed ones too, as they are
ht_status dm_orient_first(ht_ctx *c, const char *fn, const ht_draw_source *srcs, int32_t max_factor, const std::vector<HtOrientDesc> &odesc, std::vector<HtDrawMeanDesc> &desc) {
    std::vector<HtCropDesc> up(odesc.size());
    std::vector<int32_t> orient(odesc.size());
    for (size_t i = 0; i < odesc.size(); i++) {
        up[i].d = odesc[i].d, orient[i] = odesc[i].orient;
        ht_orient_size(orient[i], odesc[i].d.sw, odesc[i].d.sh, &up[i].SW, &up[i].SH);
    }
    const ht_status st = dm_unpack_sources(c, fn, up, orient.data(), false);
    if (st != HT_OK) return st;
    for (size_t i = 0; i < odesc.size(); i++) {
        ht_draw_source s = srcs[i];
        if (orient[i]) s = ht_orient_upright(srcs[i], orient[i], up[i].d.p0);
        else s.format = HT_FORMAT_OF(s.format);
        HtDrawExtent unused;
        const int ps = ht_draw_filter_plan_entry(s, c->W, c->H, max_factor, &desc[i], &unused);
        if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": entry " + std::to_string(i) + ": " + ht_draw_filter_message(ps));  // (ht_orient_plan admitted it)
    }
    return HT_OK;
}

// the two list calls: ht_draw_list_device is the max_factor-less form of ht_draw_list_filtered_device.  Everything is checked before anything is enqueued
struct DrawListCall {
    int kind;  // HT_DRAW_CALL_LIST | HT_DRAW_CALL_LIST_FILTERED
    const char *fn;
    int32_t max_factor;
    bool filtered() const { return kind == HT_DRAW_CALL_LIST_FILTERED; }
};

ht_status draw_list_call(ht_ctx *c, const DrawListCall &k, const ht_draw_source *srcs, int32_t n, void *dst_dev, size_t dst_frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range(k.fn);
    const std::string f(k.fn);
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_list_message(HT_DRAW_LIST_BAD_COUNT));
    if (k.filtered() && !ht_draw_filter_factor_ok(k.max_factor)) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_filter_message(HT_DRAW_FILTER_BAD_FACTOR));
    // a list with an oriented entry (any bit above the format number) is planned by ht_orient_plan — the rects against O, the extents of the stored
    // planes — and drawn, all of it, by the module's kernel; the filtered call ORIENTS FIRST.  A list without one takes the path it always took
    const bool oriented = std::any_of(srcs, srcs + n, [](const ht_draw_source &s) { return ht_orient_present(s.format); });
    std::vector<HtDrawDesc> desc(k.filtered() || oriented ? 0 : (size_t)n);
    std::vector<HtDrawMeanDesc> mdesc(k.filtered() ? (size_t)n : 0);
    std::vector<HtOrientDesc> odesc(oriented ? (size_t)n : 0);
    std::vector<HtDrawExtent> ext((size_t)n);
    int32_t bad = -1;
    const int ps = oriented       ? ht_orient_plan(srcs, n, c->W, c->H, odesc.data(), ext.data(), &bad)
                   : k.filtered() ? ht_draw_filter_plan(srcs, n, c->W, c->H, k.max_factor, mdesc.data(), ext.data(), &bad)
                                  : ht_draw_list_plan(srcs, n, c->W, c->H, desc.data(), ext.data(), &bad);
    const auto launch = [&](uint8_t *dst, size_t stride) -> ht_status {
        if (k.filtered()) {
            const ht_status st = oriented ? dm_orient_first(c, k.fn, srcs, k.max_factor, odesc, mdesc) : HT_OK;
            return st != HT_OK ? st : dm_launch(c, k.fn, mdesc, dst, stride);
        }
        if (oriented) return or_launch(c, k.fn, odesc, dst, stride);
        // a list with a packed 4:2:2 entry (YUYV / UYVY) is drawn by the filtered draw's kernel at factors (1, 1)
        const bool packed = std::any_of(desc.begin(), desc.end(), [](const HtDrawDesc &d) { return ht_yuv_is_422(d.format); });
        return packed ? dm_launch_unfiltered(c, k.fn, desc, dst, stride) : dl_launch(c, k.fn, desc, dst, stride);
    };
    return draw_resolved(c, k.kind, k.fn, n, dst_dev, dst_frame_stride, DrawSources{ext.data(), n, ps != HT_DRAW_LIST_OK, bad, ht_draw_filter_message(ps)}, oriented, launch);
}

}  // namespace

extern "C" ht_status ht_draw_frames_device(ht_ctx *c, const void *src_dev, int32_t n, int32_t src_width, int32_t src_height, size_t src_pitch,
                                           size_t src_frame_stride, const ht_cs_rect *src_rect, void *dst_dev, size_t dst_frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_frames_device");
    const char *fn = "ht_draw_frames_device";
    IgPlan p;
    const ht_status st = ig_check(c, fn, n, src_width, src_height, src_pitch, src_frame_stride, src_rect, &p);
    if (st != HT_OK) return st;
    const HtDrawExtent ext = {{src_dev}, {p.src_bytes}};
    return draw_resolved(c, HT_DRAW_CALL_FRAMES, fn, n, dst_dev, dst_frame_stride, DrawSources{&ext, 1, !src_dev || ((uintptr_t)src_dev & 3), -1, nullptr}, false,
                         [&](uint8_t *dst, size_t stride) { return ig_launch(c, p, static_cast<const uint8_t *>(src_dev), n, dst, stride); });
}

extern "C" ht_status ht_draw_frames(ht_ctx *c, const uint8_t *host_rgba, int32_t n, int32_t src_width, int32_t src_height, size_t src_frame_stride,
                                    const ht_cs_rect *src_rect) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_frames");
    const char *fn = "ht_draw_frames";
    IgPlan p;
    const size_t sbytes = (size_t)(src_width > 0 ? src_width : 0) * (size_t)(src_height > 0 ? src_height : 0) * 4;
    if (src_frame_stride && src_frame_stride < sbytes) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": source frame stride smaller than a frame");
    ht_status st = ig_check(c, fn, n, src_width, src_height, 0, 0, src_rect, &p);  // staged packed: the caller's stride is applied by the copy
    if (st != HT_OK) return st;
    const size_t need = sbytes * (size_t)n;
    if ((st = draw_stage_host(c, HT_DRAW_CALL_FRAMES, fn, host_rgba, n, need)) != HT_OK) return st;
    if (!src_frame_stride || src_frame_stride == sbytes) HT_HIP(c, hipMemcpyAsync(c->d_ingest_src, host_rgba, need, hipMemcpyHostToDevice, c->stream));
    else HT_HIP(c, hipMemcpy2DAsync(c->d_ingest_src, sbytes, host_rgba, src_frame_stride, sbytes, (size_t)n, hipMemcpyHostToDevice, c->stream));
    return draw_bound(c, fn, n, [&](uint8_t *dst, size_t stride) { return ig_launch(c, p, c->d_ingest_src, n, dst, stride); });
}

extern "C" ht_status ht_draw_frames_yuv_device(ht_ctx *c, const ht_yuv_frames *s, int32_t n, const ht_cs_rect *src_rect, void *dst_dev, size_t dst_frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_frames_yuv_device");
    const char *fn = "ht_draw_frames_yuv_device";
    if (!s) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": NULL source description");
    IgYuvCall q;
    const ht_status st = igy_check(c, fn, n, s->width, s->height, s->format, s->matrix, s->y_pitch, s->c_pitch, s->frame_stride, src_rect, &q);
    if (st != HT_OK) return st;
    const bool nv12 = q.format == HT_YUV_FMT_NV12, packed = ht_yuv_is_422(q.format);  // packed: one plane, u and v are not looked at
    if (!s->y || (!packed && (!s->u || (!nv12 && !s->v)))) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": NULL plane");
    if (nv12 && ((uintptr_t)s->u & 1)) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": the NV12 chroma plane must start at an even address");
    if (packed && ((uintptr_t)s->y & 3)) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": misaligned YUYV / UYVY plane (4-byte alignment required)");
    const uint8_t *y = static_cast<const uint8_t *>(s->y), *u = packed ? nullptr : static_cast<const uint8_t *>(s->u),
                  *v = nv12 || packed ? nullptr : static_cast<const uint8_t *>(s->v);
    const HtDrawExtent ext = {{y, u, v}, {q.plan.y_extent, q.plan.c_extent, q.plan.c_extent}};
    return draw_resolved(c, HT_DRAW_CALL_YUV, fn, n, dst_dev, dst_frame_stride, DrawSources{&ext, 1, false, -1, nullptr}, false,
                         [&](uint8_t *dst, size_t stride) { return igy_launch(c, fn, q, y, u, v, n, dst, stride); });
}

extern "C" ht_status ht_draw_frames_yuv(ht_ctx *c, const uint8_t *host, int32_t n, int32_t width, int32_t height, int32_t format, int32_t matrix,
                                        size_t frame_stride, const ht_cs_rect *src_rect) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_frames_yuv");
    const char *fn = "ht_draw_frames_yuv";
    // staged tightly packed, Y then chroma, at 1.5 B/px.  NV12 wants its chroma plane at an even address: a frame of odd width AND odd
    // height has an odd Y plane, so it is staged one byte into the buffer (the Y plane needs no alignment) and frames one byte further
    // apart.  A packed 4:2:2 frame is 4 cw h bytes at 2 B/px, a multiple of 4 already: no lead, and every frame starts on a macropixel
    HtYuvPlan p0;
    const int32_t given = format;  // with its orientation bits: igy_check takes them apart again
    int32_t orient = 0;
    ht_orient_split(given, &format, &orient);
    const size_t fsz = ht_yuv_plan(width, height, format, matrix, 0, 0, 0, 1, &p0) == HT_YUV_PLAN_OK ? p0.packed_frame : 0;
    const size_t lead = (format == HT_YUV_FMT_NV12) ? (fsz & 1) : 0, dstep = fsz + lead;
    IgYuvCall q;
    ht_status st = igy_check(c, fn, n, width, height, given, matrix, 0, 0, dstep, src_rect, &q);  // (reports what made fsz 0, if anything did)
    if (st != HT_OK) return st;
    if (frame_stride && frame_stride < fsz) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": source frame stride smaller than a frame");
    if ((st = draw_stage_host(c, HT_DRAW_CALL_YUV, fn, host, n, lead + dstep * (size_t)n)) != HT_OK) return st;
    uint8_t *stage = c->d_ingest_src + lead;
    const size_t sstep = frame_stride ? frame_stride : fsz;
    // one copy when both sides are packed; otherwise one per frame (a strided hipMemcpy2DAsync into the byte-offset staging left the head
    // of frame 0 stale on the GPU tests' pageable sources, and n is a batch of feeds, not of pixels)
    if (n == 1 || (sstep == fsz && dstep == fsz)) HT_HIP(c, hipMemcpyAsync(stage, host, n == 1 ? fsz : fsz * (size_t)n, hipMemcpyHostToDevice, c->stream));
    else
        for (int32_t f = 0; f < n; f++) HT_HIP(c, hipMemcpyAsync(stage + (size_t)f * dstep, host + (size_t)f * sstep, fsz, hipMemcpyHostToDevice, c->stream));
    const bool packed = ht_yuv_is_422(format);
    const uint8_t *y = stage, *u = packed ? nullptr : stage + (size_t)width * (size_t)height,
                  *v = format == HT_YUV_FMT_I420 ? u + (size_t)q.plan.cw * (size_t)q.plan.ch : nullptr;
    return draw_bound(c, fn, n, [&](uint8_t *dst, size_t stride) { return igy_launch(c, fn, q, y, u, v, n, dst, stride); });
}

extern "C" ht_status ht_draw_list_device(ht_ctx *c, const ht_draw_source *srcs, int32_t n, void *dst_dev, size_t dst_frame_stride) {
    return draw_list_call(c, {HT_DRAW_CALL_LIST, "ht_draw_list_device", 0}, srcs, n, dst_dev, dst_frame_stride);
}

extern "C" ht_status ht_draw_list_filtered_device(ht_ctx *c, const ht_draw_source *srcs, int32_t n, int32_t max_factor, void *dst_dev, size_t dst_frame_stride) {
    return draw_list_call(c, {HT_DRAW_CALL_LIST_FILTERED, "ht_draw_list_filtered_device", max_factor}, srcs, n, dst_dev, dst_frame_stride);
}

// the factors the filtered call takes for a source rect of src_width x src_height on a canvas: no context, no device
extern "C" ht_status ht_draw_filter_factors(int32_t src_width, int32_t src_height, int32_t canvas_width, int32_t canvas_height, int32_t max_factor, int32_t *nx,
                                            int32_t *ny) {
    if (!nx || !ny || src_width <= 0 || src_height <= 0 || src_width > HT_YUV_MAX_DIM || src_height > HT_YUV_MAX_DIM || canvas_width <= 0 || canvas_height <= 0 ||
        !ht_draw_filter_factor_ok(max_factor))
        return HT_ERR_INVALID;
    ht_draw_filter_factors_of(src_width, src_height, canvas_width, canvas_height, max_factor, nx, ny);
    return HT_OK;
}

// ht_ingest_yuv.hip — the video -> canvas draw for frames that arrive as YUV 4:2:0 (NV12 from hardware decoders, I420 from software
// decoders): the colour conversion a browser's drawImage(video, ..) hides, fused into the draw.  Included by ht_ingest.hip, so
// it is part of the same code object and shares that file's text: the tile constants, ig_channel.  The kernel, a call's checks (igy_check) and
// the planar launch are here; the two entry points and the routes below are ht_draw_calls.hip, the draw family's one host path.
//
// The result is DEFINED as what ht_draw_frames_device gives on the RGBA frame the declared conversion (ht_yuv_plan.h) makes of the
// planes, byte for byte, for every rect, ratio and size: a destination pixel's four tap pixels are converted to RGBA8 dwords with the
// integer formula and then go through ig_channel unchanged.  A 1 : 1 whole-frame draw is therefore the bare conversion.
//
// k_draw_yuv<FMT> tiles like k_draw_frames (64 x 16 destination pixels, 256 threads, taps once per tile in LDS, one column and four rows
// per thread).  Per row pair a thread reads
//   Y       the tap pair (a, a + 1) as ONE 2-byte read at byte granularity (anchored one pixel to the left at the rect's last column, as
//           k_draw_frames anchors its pixel pair; a 1-pixel-wide rect is read byte by byte);
//   chroma  the two chroma samples the pair can name, (a >> 1) and (a >> 1) + 1, as ONE read anchored at min(a >> 1, cw - 2): NV12 4
//           bytes U V U V at a 2-byte-aligned address (the chroma base and pitch are even), I420 2 bytes from each of the two planes;
//           a frame of 1 or 2 pixels' width has one chroma column and is read sample by sample.
// All 16 (NV12) or 24 (I420) reads of a thread are issued before the first use.  DESIGN.md §2.3 gives the reasoning.
//
// Packed 4:2:2 (YUYV, UYVY: one plane of 4-byte macropixels, ht_yuv_plan.h) takes the same calls, the same plan and the same pixel body
// (IG_BODY_YUV: per row pair ONE 8-byte read of the two macropixels the tap pair can name, anchored at min(a >> 1, cw - 2) at a
// 4-byte-aligned address, 8 reads per thread in front of the first use; Y, U and V by shifts out of the lane's registers), but not a
// k_draw_yuv<> of its own: the frames become n descriptors of the one list kernel that is compiled with the packed body,
// k_draw_list_mean_tile at factors (1, 1) (ht_draw_filter.hip; DESIGN.md §2.3.1 says why).
#include <vector>

#include "ht_draw_list_plan.h"
#include "ht_orient_plan.h"
#include "ht_yuv_plan.h"

static_assert(HT_YUV_NV12 == HT_YUV_FMT_NV12 && HT_YUV_I420 == HT_YUV_FMT_I420 && HT_YUV_YUYV == HT_YUV_FMT_YUYV && HT_YUV_UYVY == HT_YUV_FMT_UYVY,
              "format numbers of the header and of the plan");
static_assert(HT_YUV_BT601_LIMITED == 0 && HT_YUV_BT709_LIMITED == 1 && HT_YUV_BT601_FULL == 2 && HT_YUV_BT709_FULL == 3, "matrix numbers");

namespace {

// byte-granular reads: the address is aligned only as far as the type says (legal for global memory on gfx950)
typedef uint16_t ig_u16b __attribute__((aligned(1)));
typedef uint32_t ig_u32h __attribute__((aligned(2)));

// the chroma of one source row at the anchor column: NV12 form, bytes U0 V0 U1 V1 (sample 0 = the anchor, 1 = its right neighbour).  fmt:
// NV12, or I420 for every other value; a constant wherever the kernel's format is one
__device__ __forceinline__ uint32_t ig_chroma_read(const int fmt, const uint8_t *u, const uint8_t *v, size_t off, bool cpair) {
    if (fmt == HT_YUV_FMT_NV12) {
        if (cpair) return *reinterpret_cast<const ig_u32h *>(u + 2 * off);
        return *reinterpret_cast<const uint16_t *>(u + 2 * off);
    }
    uint32_t uu, vv;
    if (cpair) uu = *reinterpret_cast<const ig_u16b *>(u + off), vv = *reinterpret_cast<const ig_u16b *>(v + off);
    else uu = u[off], vv = v[off];
    return (uu & 0xffu) | ((vv & 0xffu) << 8) | ((uu & 0xff00u) << 8) | ((vv & 0xff00u) << 16);
}

// yp / up / vp: frame 0 of each plane (NV12: up = the interleaved plane, vp unused), rows y_pitch / c_pitch bytes, frames `stride` bytes
// apart in every plane; cw: chroma samples per row of the FRAME; the rest as k_draw_frames
template <int FMT>
__global__ __launch_bounds__(IG_NT) void k_draw_yuv(const uint8_t *__restrict__ yp, const uint8_t *__restrict__ up, const uint8_t *__restrict__ vp,
                                                    size_t y_pitch, size_t c_pitch, size_t stride, uint8_t *__restrict__ dst, size_t dst_stride, int sx,
                                                    int sy, int sw, int sh, int cw, int dw, int dh, double rx, double ry, HtYuvCoef kc) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
#define IG_BODY_PART 3  // IG_BODY_YUV: the four tap pixels converted by ht_yuv_to_rgba, then ig_channel(p00, p01, p10, p11, ..) per channel
#include "ht_ingest_bodies.inc"
}

struct IgYuvCall {  // a validated call: the source as the device will see it
    HtYuvPlan plan;
    int32_t format, matrix;  // format: the bare number
    int32_t orient, width, height;  // the orientation the format carried, and the STORED frame's size
    int32_t sx, sy, sw, sh;  // the source rect: in O's coordinates (orientation 0: O is the stored frame)
};

// the checks both entry points share (ht_draw_calls.hip)
ht_status igy_check(ht_ctx *c, const char *fn, int32_t n, int32_t width, int32_t height, int32_t format, int32_t matrix, size_t y_pitch, size_t c_pitch,
                    size_t frame_stride, const ht_cs_rect *rect, IgYuvCall *q) {
    const std::string f(fn);
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    ht_orient_split(format, &format, &q->orient);  // (a value with a bit from 11 up stays whole and is refused as no format)
    const int ps = ht_yuv_plan(width, height, format, matrix, y_pitch, c_pitch, frame_stride, n, &q->plan);
    if (ps != HT_YUV_PLAN_OK) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_yuv_plan_message(ps));
    q->format = format, q->matrix = matrix, q->width = width, q->height = height;
    q->sx = q->sy = 0, q->sw = width, q->sh = height;
    if (q->orient) {  // the rect is O's
        if (!ht_orient_rect(q->orient, width, height, rect, &q->sx, &q->sy, &q->sw, &q->sh))
            return ht_fail(c, HT_ERR_INVALID, f + ": source rect must lie wholly inside the oriented source frame");
    } else if (rect) {
        if (rect->x < 0 || rect->y < 0 || rect->width <= 0 || rect->height <= 0 || rect->width > width - rect->x || rect->height > height - rect->y)
            return ht_fail(c, HT_ERR_INVALID, f + ": source rect must lie wholly inside the source frame");
        q->sx = rect->x, q->sy = rect->y, q->sw = rect->width, q->sh = rect->height;
    }
    return HT_OK;
}

// NV12 (u: the interleaved plane, v unused) and I420; a packed 4:2:2 or an oriented call is not this kernel's (igy_launch, ht_draw_calls.hip)
ht_status igy_launch_planar(ht_ctx *c, const IgYuvCall &q, const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, uint8_t *dst, size_t dstride) {
    const double rx = (double)q.sw / (double)c->W, ry = (double)q.sh / (double)c->H;  // canvas_shim.js: one binary64 division each
    const HtYuvPlan &p = q.plan;
    const HtYuvCoef kc = HT_YUV_COEF[q.matrix];
    HtProfScope ps(c, "draw_yuv");
    const dim3 grid((c->W + IG_TW - 1) / IG_TW, (c->H + IG_TH - 1) / IG_TH, n);
    if (q.format == HT_YUV_FMT_NV12)
        hipLaunchKernelGGL(k_draw_yuv<HT_YUV_FMT_NV12>, grid, dim3(IG_NT), 0, c->stream, y, u, u, p.y_pitch, p.c_pitch, p.stride, dst, dstride, q.sx, q.sy, q.sw,
                           q.sh, p.cw, c->W, c->H, rx, ry, kc);
    else
        hipLaunchKernelGGL(k_draw_yuv<HT_YUV_FMT_I420>, grid, dim3(IG_NT), 0, c->stream, y, u, v, p.y_pitch, p.c_pitch, p.stride, dst, dstride, q.sx, q.sy, q.sw,
                           q.sh, p.cw, c->W, c->H, rx, ry, kc);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

}  // namespace

// ht_ingest.hip — the loop's video -> canvas copy on the device (reference: src/main.js:170, 312).
//
//   canvasContext.drawImage(videoElement, 0, 0, canvasElement.width, canvasElement.height)
//
// A source frame of any size (or a rectangle of it: the 9-argument drawImage) is scaled onto the W x H work canvas that every later
// stage reads.  The filter is the resampler DECLARED in oracle/canvas_shim.js — the one the pyramid kernels implement for gray planes —
// on all four channels: ratios divided on the host, taps by rs_tap (ht_resample_tap.h), then per channel top / bot / v with explicit
// __dmul_rn / __dadd_rn (never contracted) and a round-half-even store, the sequence of rs_pixels4 (ht_pyramid.hip).  Same size and
// whole rect is an exact copy by that arithmetic (t = 0, u = 1 everywhere).
//
// One launch covers all n frames: grid (tile column, tile row, frame), a tile = 64 x 16 destination pixels, 256 threads.  80 threads
// compute the tile's 64 column and 16 row taps into LDS (once per tile, not per pixel); then every thread produces 4 pixels of its
// column, 4 rows apart: all 8 source reads (two rows x one 8-byte tap pair each) are issued before the first use, a pixel is stored as
// one dword, a wavefront stores 256 contiguous bytes of a destination row.  Source pixels are NOT staged in LDS: neighbouring lanes'
// tap pairs overlap or abut for ratios <= 2 and fall into the same 64-byte lines up to ratio 16, which the vector cache serves
// (DESIGN.md §2.3 gives the reasoning; it is not backed by a measurement yet, profiles/ingest.txt lists what is open).
//
// A file of its own, compiled into the back-projection unit's code object (ht_backproject.hip includes it at its end): profiles/traffic.json
// ties the committed hardware counters to the machine code of the pyramid, scan and camshift code objects, which this code must not touch
// (benchlib/fingerprint.py finds a unit by a kernel-name substring; no kernel here may carry one), and the library keeps exactly one
// code object besides those three (tests/test_backproject_cpu.py).  The kernel, a call's checks (ig_check) and the launch are here; the entry
// points are ht_draw_calls.hip, the draw family's one host path, included last: behind every kernel file below and the launchers they define.
#include <algorithm>
#include <string>
#include <type_traits>

#include "ht_internal.h"
#include "ht_resample_tap.h"

namespace {

constexpr int IG_TW = 64, IG_TH = 16, IG_NT = 256, IG_RPT = IG_TH / (IG_NT / IG_TW);  // 4 rows per thread

// two neighbouring RGBA pixels as one access; the address is only pixel-aligned (legal for global memory on gfx950)
typedef uint32_t ig_u32x2 __attribute__((ext_vector_type(2), aligned(4)));

// one channel of one pixel: the declared sequence (rs_pixels4, ht_pyramid.hip), values within [0, 255]
__device__ __forceinline__ uint32_t ig_channel(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int sh, double cu, double ct, double ru, double rt) {
    const double s00 = (double)((p00 >> sh) & 0xffu), s01 = (double)((p01 >> sh) & 0xffu);
    const double s10 = (double)((p10 >> sh) & 0xffu), s11 = (double)((p11 >> sh) & 0xffu);
    const double top = __dadd_rn(__dmul_rn(s00, cu), __dmul_rn(s01, ct));
    const double bot = __dadd_rn(__dmul_rn(s10, cu), __dmul_rn(s11, ct));
    const double vv = __dadd_rn(__dmul_rn(top, ru), __dmul_rn(bot, rt));
    return (uint32_t)(int)__builtin_rint(vv) << sh;  // Uint8ClampedArray: round half to even
}

// src: frame 0 of the source, rows src_pitch bytes, frames src_stride bytes apart; (sx, sy, sw, sh): the source rect, inside the frame;
// dst: dw x dh packed rows, frames dst_stride bytes apart; rx = sw / dw, ry = sh / dh from the host.
__global__ __launch_bounds__(IG_NT) void k_draw_frames(const uint8_t *__restrict__ src, size_t src_pitch, size_t src_stride, uint8_t *__restrict__ dst,
                                                       size_t dst_stride, int sx, int sy, int sw, int sh, int dw, int dh, double rx, double ry) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
#define IG_BODY_PART 2  // IG_BODY_RGBA: per pixel, four times ig_channel(p00, p01, p10, p11, ..)
#include "ht_ingest_bodies.inc"
}

struct IgPlan {  // a validated call
    int32_t sx, sy, sw, sh;
    size_t pitch, sstride;  // effective source pitch / frame stride
    size_t src_bytes;       // extent of the n source frames from src
};

// the checks both entry points share (ht_draw_calls.hip; the source described as the device will see it)
ht_status ig_check(ht_ctx *c, const char *fn, int32_t n, int32_t src_width, int32_t src_height, size_t src_pitch, size_t src_frame_stride,
                   const ht_cs_rect *rect, IgPlan *p) {
    const std::string f(fn);
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (n <= 0) return ht_fail(c, HT_ERR_INVALID, f + ": bad frame count");
    if (src_width <= 0 || src_height <= 0 || src_width > 16384 || src_height > 16384)
        return ht_fail(c, HT_ERR_INVALID, f + ": source width/height must be 1..16384");
    p->pitch = src_pitch ? src_pitch : (size_t)src_width * 4;
    if ((p->pitch & 3) || p->pitch < (size_t)src_width * 4) return ht_fail(c, HT_ERR_INVALID, f + ": source pitch smaller than a row or not a multiple of 4");
    p->sstride = src_frame_stride ? src_frame_stride : p->pitch * (size_t)src_height;
    if ((p->sstride & 3) || p->sstride < p->pitch * (size_t)src_height)
        return ht_fail(c, HT_ERR_INVALID, f + ": source frame stride smaller than a frame or not a multiple of 4");
    p->sx = p->sy = 0, p->sw = src_width, p->sh = src_height;
    if (rect) {
        if (rect->x < 0 || rect->y < 0 || rect->width <= 0 || rect->height <= 0 || rect->width > src_width - rect->x || rect->height > src_height - rect->y)
            return ht_fail(c, HT_ERR_INVALID, f + ": source rect must lie wholly inside the source frame");
        p->sx = rect->x, p->sy = rect->y, p->sw = rect->width, p->sh = rect->height;
    }
    p->src_bytes = (size_t)(n - 1) * p->sstride + p->pitch * (size_t)src_height;
    return HT_OK;
}

ht_status ig_launch(ht_ctx *c, const IgPlan &p, const uint8_t *src, int32_t n, uint8_t *dst, size_t dstride) {
    HtProfScope ps(c, "draw_frames");
    const double rx = (double)p.sw / (double)c->W, ry = (double)p.sh / (double)c->H;  // canvas_shim.js: one binary64 division each
    const dim3 grid((c->W + IG_TW - 1) / IG_TW, (c->H + IG_TH - 1) / IG_TH, n);
    hipLaunchKernelGGL(k_draw_frames, grid, dim3(IG_NT), 0, c->stream, src, p.pitch, p.sstride, dst, dstride, p.sx, p.sy, p.sw, p.sh, c->W, c->H, rx, ry);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

}  // namespace

void ht_ingest_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_ingest_src) (void)hipFree(c->d_ingest_src);
    c->d_ingest_src = nullptr, c->ingest_src_cap = 0;
    ht_stage_free(&c->dl_tab);  // ht_draw_list_device's descriptor table (ht_draw_list.hip)
    ht_crop_free(c);  // the face crops' table, records and events (ht_face_calls.hip)
    ht_align_free(c);  // the aligned crops' likewise
}

#include "ht_ingest_yuv.hip"  // the same draw for YUV 4:2:0 frames (shares ig_channel and the tile constants)
#include "ht_draw_list.hip"   // one launch for a list of per-feed sources (shares the pixel bodies of both files)
// the face crops: each tracker's box cut from its feed (the draw list's kernel with a rect the device works out itself).  Its rule header
// is host AND device text; ht_cs_pairs.hip, later in this code object, spells HT_CSB_FN with the same tokens
#define HT_CSB_FN __host__ __device__ inline
#define HT_CROP_FN __host__ __device__ inline
#define HT_PATCH_FN __host__ __device__ inline  // ht_patch_plan.h: ht_face_calls.hip checks a tensor call's format, ht_patch.hip compiles the rule
#include "ht_crop.hip"
// the aligned crops: the rotated box of each tracker, upright (a kernel of its own: a gather along tilted lines, integer blend)
#define HT_ALIGN_FN __host__ __device__ inline
#include "ht_align.hip"
// model-input tensors from both: the same kernels with a planar / float output stage (ht_patch_plan.h states the rule)
#include "ht_patch.hip"
// prefiltered crops: each patch pixel the mean of a block of the unfiltered rule's samples (ht_filter_plan.h states the rule); the kernels
// compile the pixel bodies of both siblings as text, with an accumulating output stage
#define HT_FILTER_FN __host__ __device__ inline
#include "ht_filter_plan.h"
#include "ht_filter.hip"
// the calls of the four files above — one host path for the crop and the align family in all their forms — and their extern "C" entry points
#include "ht_face_calls.hip"
// the draw list with a prefilter: each canvas pixel the mean of a block of the unfiltered draw's samples (ht_draw_filter_plan.h states the
// rule and plans a call on the host); the kernel compiles the three pixel bodies through the crops' scaffold, with ht_filter.hip's accumulating output stage
#include "ht_draw_filter.hip"
// the calls of the draw family: one host path for the six canvas-draw entry points, behind every launcher they end up in
#include "ht_draw_calls.hip"

// ht_align.hip — the angle-aligned face crops: each tracker's ROTATED box cut from its feed and sampled upright, on the device
// (ht_camshift_align_pairs_device / ht_camshift_align_sources_device / ht_camshift_align_result / ht_camshift_align_records_device; the
// calls themselves are ht_face_calls.hip, the family's one host path).
//
// With calcAngles a track object's width and height lie along the blob's principal axes; the axis-aligned cut of ht_crop.hip is the right
// rectangle only at angle == pi / 2.  The tracker leaves `angle` in HtCsState next to the four fields k_crop_list reads, so the aligned patch
// needs nothing from the host either: the rule is ht_align_plan.h (host and device text: the angle in 4096 steps, a Q30 quarter-wave table,
// int64 Q16 affine terms), and a patch pixel is a bilinear blend with 8-bit integer weights of four taps of the source's declared RGBA view.
// Included at the end of ht_ingest.hip, behind ht_crop.hip: same code object, same anonymous-namespace helpers (the crop descriptor CrDesc
// with its mapping rect, source size and stream; DlDesc, dl_gptr, the tile constants), and ht_yuv_to_rgba for a YUV tap.
//
// k_align_list, the fused form (there is no resolve kernel): grid (tile column, tile row, entry), 64 x 16 patch pixels and 256 threads per
// workgroup, four rows per thread.  A workgroup reads its entry's descriptor and the five object fields of that stream's state with scalar
// loads (uniform index, const __restrict__) and runs the rule (workgroup-uniform, table lookups included).  Threads 0..63 then divide the
// tile's column terms, threads 64..79 its row terms, into LDS (1280 bytes); one barrier; per pixel two adds per axis, the range test in
// int64, four clamped taps, the blend and one dword store, contiguous along x.  The format is a workgroup-uniform branch.  An empty entry
// stores zeros for its tile and returns in front of the barrier (uniformly).  Workgroup (0, 0) of an entry writes its 64-byte record.
// The head (descriptor, state, rule, record, empty exit) and the term fill are ht_list_parts.inc's text, shared with ht_patch.hip.
#include "ht_align_plan.h"  // HT_ALIGN_FN is defined in front of this file's #include (ht_ingest.hip)

namespace {

static_assert(sizeof(ht_align_record) == 64 && sizeof(ht_align_params) == 16, "ht_align_record / ht_align_params");

// the source's RGBA view at (x, y), both inside the frame.  FMT: HT_DRAW_RGBA, HT_YUV_FMT_NV12 or HT_YUV_FMT_I420; the chroma of a YUV
// pixel is the sample at (x >> 1, y >> 1), addressed as ht_ingest_bodies.inc addresses it
template <int FMT>
__device__ __forceinline__ uint32_t al_tap(const uint8_t *__restrict__ p0, const uint8_t *__restrict__ p1, const uint8_t *__restrict__ p2, size_t pitch0, size_t pitch1,
                                           const HtYuvCoef &kc, int x, int y) {
    if (FMT == HT_DRAW_RGBA) return *reinterpret_cast<const uint32_t *>(p0 + (size_t)y * pitch0 + (size_t)x * 4);
    const uint32_t yy = p0[(size_t)y * pitch0 + (size_t)x];
    uint32_t u, v;
    if (FMT == HT_YUV_FMT_NV12) {
        const uint32_t uv = *reinterpret_cast<const uint16_t *>(p1 + 2 * ((size_t)(y >> 1) * (pitch1 / 2) + (size_t)(x >> 1)));  // an even address: the plan requires it
        u = uv & 0xffu, v = uv >> 8;
    } else {
        const size_t off = (size_t)(y >> 1) * pitch1 + (size_t)(x >> 1);
        u = p1[off], v = p2[off];
    }
    return ht_yuv_to_rgba((int32_t)yy, (int32_t)u, (int32_t)v, kc);
}

// the four rows of a thread's column, behind the barrier; every pixel ends in ONE output stage, store(o, x, y), o the pixel's RGBA8 dword
// (k_align_list: LpDwordStore; ht_patch.hip: the model-input tensors).  RPT rows per thread: a tile of RPT * 4 rows (ht_filter.hip takes 1)
template <int FMT, class STORE, int RPT = IG_RPT>
__device__ __forceinline__ void al_pixels(const DlDesc &d, int SW, int SH, const int64_t *s_cx, const int64_t *s_cy, const int64_t *s_rx, const int64_t *s_ry,
                                          const STORE &store, int dw, int dh) {
    static_assert(RPT >= 1 && RPT <= IG_RPT, "al_pixels: 1 .. 4 rows per thread; the default is the 64 x 16 tile");
    const int col = threadIdx.x & (IG_TW - 1), r0 = threadIdx.x / IG_TW, x = blockIdx.x * IG_TW + col, Y0 = blockIdx.y * (RPT * (IG_NT / IG_TW));
    if (x >= dw) return;
    const uint8_t *__restrict__ p0 = (const uint8_t *)d.p0, *__restrict__ p1 = (const uint8_t *)d.p1, *__restrict__ p2 = (const uint8_t *)d.p2;
    const size_t pitch0 = d.pitch0, pitch1 = d.pitch1;
    const HtYuvCoef kc = d.kc;
    const int64_t cfx = s_cx[col], cfy = s_cy[col];
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int j = r0 + k * (IG_NT / IG_TW), y = Y0 + j;
        if (y >= dh) continue;
        const int64_t fx = cfx + s_rx[j], fy = cfy + s_ry[j];
        uint32_t o = 0u;
        if (ht_align_inside(fx, fy, SW, SH)) {  // in here fx, fy fit int32: -32768 .. 16384 * 65536
            const int32_t gx = (int32_t)fx, gy = (int32_t)fy;
            const int xi = gx >> 16, yi = gy >> 16;  // -1 .. SW - 1, -1 .. SH - 1
            const uint32_t tx = ((uint32_t)gx & 65535u) >> 8, ty = ((uint32_t)gy & 65535u) >> 8;
            const int xa = max(xi, 0), xb = min(xi + 1, SW - 1), ya = max(yi, 0), yb = min(yi + 1, SH - 1);
            const uint32_t p00 = al_tap<FMT>(p0, p1, p2, pitch0, pitch1, kc, xa, ya), p01 = al_tap<FMT>(p0, p1, p2, pitch0, pitch1, kc, xb, ya);
            const uint32_t p10 = al_tap<FMT>(p0, p1, p2, pitch0, pitch1, kc, xa, yb), p11 = al_tap<FMT>(p0, p1, p2, pitch0, pitch1, kc, xb, yb);
#pragma unroll
            for (int ch = 0; ch < 4; ch++) o |= ht_align_channel(p00, p01, p10, p11, 8 * ch, tx, ty);
        }
        store(o, x, y);
    }
}

// the format is a workgroup-uniform branch into al_pixels' three forms, in a kernel that has format, d, SW, SH, dw, dh.  cx, cy / rx, ry:
// this pass's column and row terms; store: the output stage, of type STORE.  Text, not a function: see ht_list_parts.inc
#define AL_PIXELS_ANY(STORE, RPT, cx, cy, rx, ry, store)                                                                          \
    do {                                                                                                                          \
        if (format == HT_DRAW_RGBA) al_pixels<HT_DRAW_RGBA, STORE, RPT>(d, SW, SH, cx, cy, rx, ry, store, dw, dh);                \
        else if (format == HT_YUV_FMT_NV12) al_pixels<HT_YUV_FMT_NV12, STORE, RPT>(d, SW, SH, cx, cy, rx, ry, store, dw, dh);     \
        else al_pixels<HT_YUV_FMT_I420, STORE, RPT>(d, SW, SH, cx, cy, rx, ry, store, dw, dh);                                    \
    } while (0)

__global__ __launch_bounds__(IG_NT) void k_align_list(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                      int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, ht_align_record *__restrict__ recs) {
    __shared__ int64_t s_cx[IG_TW], s_cy[IG_TW], s_rx[IG_TH], s_ry[IG_TH];
#define LP_PART 2  // LP_UPRIGHT_HEAD
#include "ht_list_parts.inc"
    if (code != HT_ALIGN_FACE) return lp_empty_tile<IG_RPT>(lp_dword_store(dst, dst_stride, dw), dw, dh);  // uniform
#define LP_PART 3  // LP_UPRIGHT_TERMS
#include "ht_list_parts.inc"
    __syncthreads();
    const LpDwordStore store = lp_dword_store(dst, dst_stride, dw);
    AL_PIXELS_ANY(LpDwordStore, IG_RPT, s_cx, s_cy, s_rx, s_ry, store);
}

void align_launch_list(const FaceLaunch &a) {
    hipLaunchKernelGGL(k_align_list, a.grid, dim3(IG_NT), 0, a.c->stream, FACE_KARGS(a), static_cast<ht_align_record *>(a.recs));
}

}  // namespace

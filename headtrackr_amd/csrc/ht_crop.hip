// ht_crop.hip — the output side of the K-feed host: each tracker's box cut from its feed and scaled to a patch, on the device
// (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device / ht_camshift_crop_result / ht_camshift_crop_records_device; the calls
// themselves, with the whole family's host path, are ht_face_calls.hip).
//
// A track step leaves its track object in HtCsState on the device, in canvas coordinates.  The face PIXELS are in the feed's own frame
// (or, pairs form, in the bound canvas frame).  Mapping the box back, rounding it and scaling the rect to the patch size needs nothing from
// the host: the rule is integer arithmetic (ht_crop_plan.h, host and device text), the resampler is the text of ht_ingest_bodies.inc,
// which takes the destination size as dw, dh.  Included at the end of ht_ingest.hip, behind ht_draw_list.hip: same code object, same
// anonymous-namespace helpers (DlDesc, dl_gptr, the tile constants, ig_channel, ig_chroma_read).  This file is the first of the face-patch
// family (ht_align.hip, ht_patch.hip, ht_filter.hip follow) and holds what all of its kernels share besides ht_list_parts.inc: the
// descriptor, the RGBA8 output stage, the empty tile and the arguments of a launch.
//
// k_crop_list: grid (tile column, tile row, entry), 64 x 16 patch pixels and 256 threads per workgroup, the shape of k_draw_list.  A
// workgroup reads its entry's 120-byte descriptor — the draw list's descriptor, whose rect is the MAPPING rect, plus the source's size and
// the stream — and the four object fields of that stream's state with scalar loads (uniform index, const __restrict__), runs the rule
// (workgroup-uniform), divides the two ratios, and then is k_draw_list with (sx, sy, sw, sh) = the rule's rect and (dw, dh) = the patch
// size.  An empty entry stores zeros for its tile instead and returns in front of the barrier (uniformly).  Workgroup (0, 0) of an entry
// writes its 40-byte record.  All of that but the taps is ht_list_parts.inc: the cut head and the format scaffold.
#include "ht_crop_plan.h"  // HT_CROP_FN and HT_CSB_FN are defined in front of this file's #include (ht_ingest.hip)
#include "ht_patch_plan.h"  // the model-input tensors' format (ht_patch.hip), checked with everything else a call is checked for (ht_face_calls.hip)

namespace {

template <class PLANE>
struct HtCropDescT {
    HtDrawDescT<PLANE> d;  // planes, pitches, format, cw, matrix; (sx, sy, sw, sh) = the mapping rect; rx, ry unused
    int32_t SW, SH;        // the source's size
    int32_t stream, pad;
};
typedef HtCropDescT<const uint8_t *> HtCropDesc;
typedef HtCropDescT<dl_gptr> CrDesc;
static_assert(sizeof(HtCropDesc) == 120 && sizeof(CrDesc) == sizeof(HtCropDesc) && alignof(CrDesc) == alignof(HtCropDesc), "crop descriptor layout");
static_assert(sizeof(ht_crop_record) == 40, "ht_crop_record");

// the RGBA8 output stage of the family: the pixel's dword into packed rows of dw pixels
struct LpDwordStore {
    uint32_t *__restrict__ base;  // the entry's patch
    int dw;
    __device__ __forceinline__ void operator()(uint32_t o, int x, int y) const { (base + x)[(size_t)y * dw] = o; }
};

// an empty entry: f(0) — zero bytes, or bias[c] in the dtype — for this thread's pixels of the tile (64 columns, RPT * 4 rows) through the
// kernel's output stage, in front of the barrier
template <int RPT, class STORE>
__device__ __forceinline__ void lp_empty_tile(const STORE &store, int dw, int dh) {
    const int x = blockIdx.x * IG_TW + (threadIdx.x & (IG_TW - 1)), y0 = blockIdx.y * (RPT * (IG_NT / IG_TW)) + threadIdx.x / IG_TW;
    if (x >= dw) return;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int y = y0 + k * (IG_NT / IG_TW);
        if (y < dh) store(0u, x, y);
    }
}

// the RGBA8 output stage of entry blockIdx.z
__device__ __forceinline__ LpDwordStore lp_dword_store(uint8_t *dst, size_t dst_stride, int dw) {
    return LpDwordStore{reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride), dw};
}

__global__ __launch_bounds__(IG_NT) void k_crop_list(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                     int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, ht_crop_record *__restrict__ recs) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
#define LP_PART 1  // LP_CUT_HEAD
#include "ht_list_parts.inc"
    if (code != HT_CROP_FACE) return lp_empty_tile<IG_RPT>(lp_dword_store(dst, dst_stride, dw), dw, dh);  // uniform; the bodies store through IG_STORE_DWORD
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
#define LP_PART 4  // LP_SCAFFOLD
#include "ht_list_parts.inc"
}

// a launch of one of the family's kernels: what the host path (ht_face_calls.hip) hands to the form's launcher.  Every kernel begins with
// the same ten arguments (FACE_KARGS) and ends with its records; the tensor and mean forms have theirs in between
struct FaceLaunch {
    ht_ctx *c;
    dim3 grid;  // (tile columns, 64 x 16 tile rows, entries): a form with another tile sets y itself
    const CrDesc *tab;
    const HtCsState *states;
    uint8_t *out;
    size_t ostride;
    const ht_crop_params &p;
    int32_t max_factor;          // the mean forms
    const ht_patch_format *fmt;  // the tensor forms, and the mean forms with a format (nullptr: RGBA8)
    void *recs;                  // ht_crop_record or ht_align_record, the family's
};
#define FACE_KARGS(a) (a).tab, (a).states, (a).out, (a).ostride, (int)(a).p.out_width, (int)(a).p.out_height, (a).c->W, (a).c->H, (int)(a).p.margin_q8, (a).p.flags

void crop_launch_list(const FaceLaunch &a) {
    hipLaunchKernelGGL(k_crop_list, a.grid, dim3(IG_NT), 0, a.c->stream, FACE_KARGS(a), static_cast<ht_crop_record *>(a.recs));
}

}  // namespace

// ht_patch.hip — model-input tensors from face crops: the crop and align calls with another output stage
// (ht_camshift_crop_pairs_tensor_device / ht_camshift_crop_sources_tensor_device / ht_camshift_align_pairs_tensor_device /
// ht_camshift_align_sources_tensor_device; the calls themselves are ht_face_calls.hip, the family's one host path).
//
// A face embedder, landmark net or liveness net reads planar (or interleaved) floats in its own channel order and normalisation, not
// RGBA8.  The rule — which bits an RGBA8 patch becomes — is ht_patch_plan.h, host and device text.  The kernels are k_crop_list and
// k_align_list with the dword store at the end of a pixel replaced by ONE output stage, PtStore::operator()(o, x, y), o the pixel's
// RGBA8 dword: the heads and the sampling bodies are shared as text (ht_list_parts.inc; ht_ingest_bodies.inc's IG_STORE hook; al_pixels'
// STORE parameter), so the patch a tensor is made of is the RGBA call's by construction.  Included at the end of ht_ingest.hip, behind ht_align.hip: same code object.
//
// k_cut_tensor<DT> / k_upright_tensor<DT>: grid (tile column, tile row, entry), 64 x 16 patch pixels, 256 threads, four rows per thread —
// the RGBA kernels' shape; a wavefront is one row of the tile, lane l holds column X0 + l.  The dtype is a template parameter (the element
// size shapes the stores), layout and channels are workgroup-uniform branches, the format's six floats are kernel arguments.  An empty
// entry stores f(0) for its tile in front of the barrier.  Stores, per pixel:
//   F32 CHW   three dword stores, each contiguous along the wavefront
//   F32 HWC   three dwords at consecutive addresses (12 bytes; the patch is 4-byte aligned)
//   16-bit CHW and gray: one short store per element, 128 contiguous bytes per wavefront.  (Pairing neighbouring lanes through
//             __shfl_down so that even elements store packed dwords — with short stores left where the row's base is odd, at the last
//             column and at lane 63 — was built and measured: 9.40 us against 8.76 us for k_cut_tensor<f16>, 11.88 us against 11.28 us for
//             k_upright_tensor<f16> on the workload of tools/gpu_patch_tensor.py.  The shuffle and the divergent store cost more than the
//             halved store count saves in a kernel whose time is the gather; the short stores shipped.  LABLOG.md has the entry.)
//   16-bit HWC (three channels, 6 bytes per pixel): one dword and one short, the dword on the 4-byte aligned half of the pixel
// (names: the kernels are the crop's and the align call's, but tests/test_crop_cpu.py and tests/test_align_cpu.py hold that k_crop_list and
// k_align_list are the ONLY kernels with those words in their names — cut / upright say the same)
namespace {

static_assert(sizeof(ht_patch_format) == 40, "ht_patch_format");

struct PtFormat {  // what the kernels need of an ht_patch_format, by value
    int32_t layout, channels;
    float scale[3], bias[3];
};

template <int DT>
struct PtStore {
    uint8_t *__restrict__ base;  // the entry's patch, 4-byte aligned
    int dw, dh;
    PtFormat f;

    // element i of the patch (16-bit dtypes); a plane of odd size starts 2-byte aligned: a short store does not care
    __device__ __forceinline__ void put16(size_t i, uint32_t e) const { *reinterpret_cast<uint16_t *>(base + 2 * i) = (uint16_t)e; }

    __device__ __forceinline__ void operator()(uint32_t o, int x, int y) const {
        const size_t px = (size_t)y * dw + x;
        if (f.channels == HT_PATCH_GRAY) {  // one channel: CHW and HWC are the same bytes
            const uint32_t e = ht_patch_element(ht_patch_value(ht_gray_of(o), f.scale[0], f.bias[0]), DT);
            if (DT == HT_PATCH_F32) reinterpret_cast<uint32_t *>(base)[px] = e;
            else put16(px, e);
            return;
        }
        uint32_t e[3];
#pragma unroll
        for (int c = 0; c < 3; c++) e[c] = ht_patch_element(ht_patch_value(ht_patch_byte(o, f.channels, c), f.scale[c], f.bias[c]), DT);
        if (f.layout == HT_PATCH_CHW) {
            const size_t plane = (size_t)dw * dh;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                if (DT == HT_PATCH_F32) reinterpret_cast<uint32_t *>(base)[c * plane + px] = e[c];
                else put16(c * plane + px, e[c]);
            }
        } else if (DT == HT_PATCH_F32) {
            uint32_t *p = reinterpret_cast<uint32_t *>(base) + 3 * px;
            p[0] = e[0], p[1] = e[1], p[2] = e[2];
        } else {
            uint8_t *p = base + 6 * px;  // 4-byte aligned for an even pixel, 2 beyond for an odd one
            if ((px & 1) == 0) {
                *reinterpret_cast<uint32_t *>(p) = e[0] | (e[1] << 16);
                *reinterpret_cast<uint16_t *>(p + 4) = (uint16_t)e[2];
            } else {
                *reinterpret_cast<uint16_t *>(p) = (uint16_t)e[0];
                *reinterpret_cast<uint32_t *>(p + 2) = e[1] | (e[2] << 16);
            }
        }
    }
};

#undef IG_STORE
#define IG_STORE(o, x, y) ((void)out, store(o, x, y))

// k_crop_list (ht_crop.hip) with PtStore as its output stage: the same table, rule, record, taps and pixel bodies
template <int DT>
__global__ __launch_bounds__(IG_NT) void k_cut_tensor(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                      int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, PtFormat pf,
                                                      ht_crop_record *__restrict__ recs) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
#define LP_PART 1  // LP_CUT_HEAD
#include "ht_list_parts.inc"
    const PtStore<DT> store = {dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf};
    if (code != HT_CROP_FACE) return lp_empty_tile<IG_RPT>(store, dw, dh);  // uniform
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
#define LP_PART 4  // LP_SCAFFOLD
#include "ht_list_parts.inc"
}

#undef IG_STORE
#define IG_STORE IG_STORE_DWORD  // the default again, for whatever is compiled behind this file

// k_align_list (ht_align.hip) with PtStore as its output stage
template <int DT>
__global__ __launch_bounds__(IG_NT) void k_upright_tensor(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                          int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, PtFormat pf,
                                                          ht_align_record *__restrict__ recs) {
    __shared__ int64_t s_cx[IG_TW], s_cy[IG_TW], s_rx[IG_TH], s_ry[IG_TH];
#define LP_PART 2  // LP_UPRIGHT_HEAD
#include "ht_list_parts.inc"
    const PtStore<DT> store = {dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf};
    if (code != HT_ALIGN_FACE) return lp_empty_tile<IG_RPT>(store, dw, dh);  // uniform
#define LP_PART 3  // LP_UPRIGHT_TERMS
#include "ht_list_parts.inc"
    __syncthreads();
    AL_PIXELS_ANY(PtStore<DT>, IG_RPT, s_cx, s_cy, s_rx, s_ry, store);
}

PtFormat pt_format(const ht_patch_format &f) {
    PtFormat p;
    p.layout = f.layout, p.channels = f.channels;
    for (int c = 0; c < 3; c++) p.scale[c] = f.scale[c], p.bias[c] = f.bias[c];
    return p;
}

// the tensor forms' launches: the RGBA kernels' grid and arguments, the format's floats in front of the records; one kernel per dtype
template <class REC>
using PtKernel = void (*)(const CrDesc *, const HtCsState *, uint8_t *, size_t, int, int, int, int, int, uint32_t, PtFormat, REC *);

template <class REC>
void pt_launch(const FaceLaunch &a, PtKernel<REC> f32, PtKernel<REC> f16, PtKernel<REC> bf16) {
    PtKernel<REC> k = a.fmt->dtype == HT_PATCH_F32 ? f32 : a.fmt->dtype == HT_PATCH_F16 ? f16 : bf16;
    hipLaunchKernelGGL(k, a.grid, dim3(IG_NT), 0, a.c->stream, FACE_KARGS(a), pt_format(*a.fmt), static_cast<REC *>(a.recs));
}

void pt_launch_cut(const FaceLaunch &a) { pt_launch<ht_crop_record>(a, k_cut_tensor<HT_PATCH_F32>, k_cut_tensor<HT_PATCH_F16>, k_cut_tensor<HT_PATCH_BF16>); }
void pt_launch_upright(const FaceLaunch &a) {
    pt_launch<ht_align_record>(a, k_upright_tensor<HT_PATCH_F32>, k_upright_tensor<HT_PATCH_F16>, k_upright_tensor<HT_PATCH_BF16>);
}

}  // namespace

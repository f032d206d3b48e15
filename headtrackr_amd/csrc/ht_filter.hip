// ht_filter.hip — prefiltered face crops: each patch pixel the mean of an Nx x Ny block of the unfiltered rule's samples
// (ht_camshift_crop_pairs_filtered_device / ht_camshift_crop_sources_filtered_device / ht_camshift_align_pairs_filtered_device /
// ht_camshift_align_sources_filtered_device / ht_camshift_crop_filter_factors / ht_camshift_align_filter_factors; the four launching
// calls themselves are ht_face_calls.hip, the family's one host path).
//
// The crop, align and tensor calls sample one bilinear tap pair per patch pixel: right for a small face, aliasing for a large one (a face
// 792 source pixels wide cut to 112 reads 2 of every 7 rows and columns).  The rule — the factors per entry, the fine patch, the rounding —
// is ht_filter_plan.h, host and device text.  Included at the end of ht_ingest.hip, behind ht_patch.hip: same code object, same helpers.
//
// k_cut_mean<DT, RPT> / k_upright_mean<DT, RPT>: the siblings' grid (tile column, tile row, entry) and their 256 threads; a tile is 64 columns
// by RPT * 4 rows, RPT rows per thread.  RPT == 4 is the siblings' 64 x 16 tile and serves max_factor 1 and 2; from max_factor 3 on the host
// launches RPT == 1, a 64 x 4 tile: a block of up to 64 samples per pixel makes a workgroup long, and 8 entries of 112 x 112 are 112
// workgroups of 64 x 16 on 256 compute units but 448 of 64 x 4 (measured: profiles/filter.txt, LABLOG.md).  A workgroup reads its
// descriptor and the stream's state with scalar loads, runs the crop or align rule and derives Nx, Ny from it (workgroup-uniform: the block
// loop does not diverge).  The taps (crop) or Q16 terms (align) of the tile's FINE columns and rows go to LDS — Nx * 64 + Ny * 4 RPT of them,
// laid out [a][column] and [b][row]; the arrays hold factor 8: 15 KB of taps or 10 KB of terms at RPT 4, 13 KB or 8.5 KB at RPT 1 —, one
// barrier, then for
// every (b, a) of the block the unfiltered kernels' own pixel body runs on tap slice a / b with an output stage that ADDS the sample's four
// bytes to the thread's sums: the bodies are ht_ingest_bodies.inc through its IG_STORE hook and al_pixels through its STORE parameter, so
// a fine sample is the unfiltered rule's byte by construction (binary64 blend and v_rndne_f64 for the crop, YUV taps converted first; Q16
// terms and the 8-bit blend for the align call).  The sums are rounded (ht_filter_pixel) and the dword goes to the siblings' output
// stage: the RGBA dword store (DT == FM_RGBA8, format == NULL: ht_crop.hip's LpDwordStore) or ht_patch.hip's PtStore<DT>.  The heads and
// the crop kernels' format scaffold are ht_list_parts.inc's text.
namespace {

constexpr int FM_RGBA8 = -1;  // the DT of a call without a format
constexpr int FM_MAXF = HT_FILTER_MAX_FACTOR;

constexpr int FM_ROWS = IG_NT / IG_TW;  // rows a workgroup's threads cover at once: a tile is RPT * FM_ROWS rows

template <int DT>
__device__ __forceinline__ auto fm_store(uint8_t *base, int dw, int dh, const PtFormat &pf) {
    if constexpr (DT == FM_RGBA8) return LpDwordStore{reinterpret_cast<uint32_t *>(base), dw};
    else return PtStore<DT>{base, dw, dh, pf};
}

// a fine sample's four bytes onto the four sums of its output pixel
__device__ __forceinline__ void fm_add(uint32_t (&s)[4], uint32_t o) { s[0] += o & 0xffu, s[1] += (o >> 8) & 0xffu, s[2] += (o >> 16) & 0xffu, s[3] += o >> 24; }

// the thread's RPT output pixels: the sums rounded, the dword handed to the output stage
template <int RPT, class STORE>
__device__ __forceinline__ void fm_finish(const uint32_t (&acc)[RPT][4], uint32_t n, const STORE &store, int dw, int dh) {
    const int x = blockIdx.x * IG_TW + (threadIdx.x & (IG_TW - 1)), y0 = blockIdx.y * (RPT * FM_ROWS) + threadIdx.x / IG_TW;
    if (x >= dw) return;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int y = y0 + k * FM_ROWS;
        if (y < dh) store(ht_filter_pixel(acc[k], n), x, y);
    }
}

#undef IG_STORE
#define IG_STORE(o, x, y) ((void)out, (void)(x), (void)(y), fm_add(acc[k], o))  // k: the bodies' row index of the thread, a constant once unrolled

// k_crop_list (ht_crop.hip) over the fine patch, averaged: the same table, rule and record; the taps are the fine patch's
template <int DT, int RPT>
__global__ __launch_bounds__(IG_NT) void k_cut_mean(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                    int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, int max_factor, PtFormat pf,
                                                    ht_crop_record *__restrict__ recs) {
    constexpr int IG_RPT = RPT, IG_TH = RPT * FM_ROWS;  // the tile of THIS kernel: the shared text reads these two names
    __shared__ RsTap s_colf[FM_MAXF * IG_TW], s_rowf[FM_MAXF * IG_TH];
#define LP_RATIOS_OF_RECORD_ONLY  // the record the unfiltered call would have written: rx = w / P; the taps below have the fine patch's
#define LP_PART 1  // LP_CUT_HEAD
#include "ht_list_parts.inc"
    const auto store = fm_store<DT>(dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf);
    if (code != HT_CROP_FACE) return lp_empty_tile<IG_RPT>(store, dw, dh);  // uniform
    const int nx = ht_filter_crop_factor(sw, dw, max_factor), ny = ht_filter_crop_factor(sh, dh, max_factor);  // uniform
    // the fine patch's ratios: one correctly rounded binary64 division each
    const double rx = (double)sw / (double)(nx * dw), ry = (double)sh / (double)(ny * dh);
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    for (int t = threadIdx.x; t < nx * IG_TW; t += IG_NT)  // [a][column]: fine column nx * x + a
        s_colf[t] = rs_tap(nx * min(X0 + (t & (IG_TW - 1)), dw - 1) + t / IG_TW, rx, sw, sx);
    for (int t = threadIdx.x; t < ny * IG_TH; t += IG_NT)  // [b][row]
        s_rowf[t] = rs_tap(ny * min(Y0 + (t & (IG_TH - 1)), dh - 1) + t / IG_TH, ry, sh, sy);
    __syncthreads();
    uint32_t acc[IG_RPT][4] = {};
    // every (b, a) of the block runs the format's body on tap slice a / b
#define LP_EACH_PASS                                   \
    _Pragma("unroll 1") for (int b = 0; b < ny; b++)   \
    _Pragma("unroll 1") for (int a = 0; a < nx; a++)   \
    if (const RsTap *s_col = s_colf + a * IG_TW, *s_row = s_rowf + b * IG_TH; true)
#define LP_PART 4  // LP_SCAFFOLD
#include "ht_list_parts.inc"
    fm_finish<RPT>(acc, (uint32_t)(nx * ny), store, dw, dh);
}

#undef IG_STORE
#define IG_STORE IG_STORE_DWORD  // the default again, for whatever is compiled behind this file

// al_pixels' output stage for a block: store(o, x, y) adds the sample to the sums of the thread's row y (y0: its first row)
template <int RPT>
struct FmAccum {
    mutable uint32_t acc[RPT][4];
    int y0;
    __device__ __forceinline__ void operator()(uint32_t o, int, int y) const {
        const int k = (y - y0) / FM_ROWS;
#pragma unroll
        for (int q = 0; q < RPT; q++)  // static indices: the sums stay in registers
            if (q == k) fm_add(acc[q], o);
    }
};

// k_align_list (ht_align.hip) over the fine patch, averaged: the same table, rule and record; the terms are the fine patch's
template <int DT, int RPT>
__global__ __launch_bounds__(IG_NT) void k_upright_mean(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                        int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, int max_factor, PtFormat pf,
                                                        ht_align_record *__restrict__ recs) {
    constexpr int IG_RPT = RPT, IG_TH = RPT * FM_ROWS;  // the tile of THIS kernel, under the names the shared text reads
    __shared__ int64_t s_cx[FM_MAXF * IG_TW], s_cy[FM_MAXF * IG_TW], s_rx[FM_MAXF * IG_TH], s_ry[FM_MAXF * IG_TH];
#define LP_PART 2  // LP_UPRIGHT_HEAD
#include "ht_list_parts.inc"
    const auto store = fm_store<DT>(dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf);
    if (code != HT_ALIGN_FACE) return lp_empty_tile<IG_RPT>(store, dw, dh);  // uniform
    const int nx = ht_filter_align_factor(pl.ux, pl.uy, dw, max_factor), ny = ht_filter_align_factor(pl.vx, pl.vy, dh, max_factor);  // uniform
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    for (int t = threadIdx.x; t < nx * IG_TW; t += IG_NT) {  // [a][column]: fine column nx * x + a of nx * dw
        const int i = nx * min(X0 + (t & (IG_TW - 1)), dw - 1) + t / IG_TW;
        s_cx[t] = pl.cx - 32768 + ht_align_term(i, nx * dw, pl.ux);
        s_cy[t] = pl.cy - 32768 + ht_align_term(i, nx * dw, pl.uy);
    }
    for (int t = threadIdx.x; t < ny * IG_TH; t += IG_NT) {  // [b][row]
        const int j = ny * min(Y0 + (t & (IG_TH - 1)), dh - 1) + t / IG_TH;
        s_rx[t] = ht_align_term(j, ny * dh, pl.vx);
        s_ry[t] = ht_align_term(j, ny * dh, pl.vy);
    }
    __syncthreads();
    FmAccum<RPT> sum = {{}, Y0 + (int)(threadIdx.x / IG_TW)};
#pragma unroll 1
    for (int b = 0; b < ny; b++)
#pragma unroll 1
        for (int a = 0; a < nx; a++) {
            const int64_t *cx = s_cx + a * IG_TW, *cy = s_cy + a * IG_TW, *rx = s_rx + b * IG_TH, *ry = s_ry + b * IG_TH;
            AL_PIXELS_ANY(FmAccum<RPT>, RPT, cx, cy, rx, ry, sum);
        }
    fm_finish<RPT>(sum.acc, (uint32_t)(nx * ny), store, dw, dh);
}

// the tile of a call: the siblings' 64 x 16 up to max_factor 2, 64 x 4 beyond (more, shorter workgroups for the long block loops)
constexpr int FM_SMALL_FROM = 3;

// the mean forms' launches: the siblings' arguments with max_factor and the format's floats in front of the records; one kernel per
// output (RGBA8 without a format, else the dtype) and tile
template <class REC>
using FmKernel = void (*)(const CrDesc *, const HtCsState *, uint8_t *, size_t, int, int, int, int, int, uint32_t, int, PtFormat, REC *);

template <class REC>
void fm_launch(const FaceLaunch &a, int rpt, FmKernel<REC> rgba8, FmKernel<REC> f32, FmKernel<REC> f16, FmKernel<REC> bf16) {
    FmKernel<REC> k = !a.fmt ? rgba8 : a.fmt->dtype == HT_PATCH_F32 ? f32 : a.fmt->dtype == HT_PATCH_F16 ? f16 : bf16;
    dim3 grid = a.grid;
    grid.y = (a.p.out_height + rpt * FM_ROWS - 1) / (rpt * FM_ROWS);
    hipLaunchKernelGGL(k, grid, dim3(IG_NT), 0, a.c->stream, FACE_KARGS(a), (int)a.max_factor, a.fmt ? pt_format(*a.fmt) : PtFormat{}, static_cast<REC *>(a.recs));
}
#define FM_KERNELS(k, rpt) rpt, k<FM_RGBA8, rpt>, k<HT_PATCH_F32, rpt>, k<HT_PATCH_F16, rpt>, k<HT_PATCH_BF16, rpt>

void fm_launch_cut(const FaceLaunch &a) {
    if (a.max_factor < FM_SMALL_FROM) fm_launch<ht_crop_record>(a, FM_KERNELS(k_cut_mean, IG_RPT));
    else fm_launch<ht_crop_record>(a, FM_KERNELS(k_cut_mean, 1));
}

void fm_launch_upright(const FaceLaunch &a) {
    if (a.max_factor < FM_SMALL_FROM) fm_launch<ht_align_record>(a, FM_KERNELS(k_upright_mean, IG_RPT));
    else fm_launch<ht_align_record>(a, FM_KERNELS(k_upright_mean, 1));
}

}  // namespace

// the factors a filtered call of (out_width, out_height, max_factor) takes for an entry, from its record alone: no context, no device
extern "C" ht_status ht_camshift_crop_filter_factors(const ht_crop_record *record, int32_t out_width, int32_t out_height, int32_t max_factor, int32_t *nx, int32_t *ny) {
    if (!record || !nx || !ny || !ht_filter_args_ok(out_width, out_height, max_factor)) return HT_ERR_INVALID;
    ht_filter_crop_record_factors(*record, out_width, out_height, max_factor, nx, ny);
    return HT_OK;
}

extern "C" ht_status ht_camshift_align_filter_factors(const ht_align_record *record, int32_t out_width, int32_t out_height, int32_t max_factor, int32_t *nx, int32_t *ny) {
    if (!record || !nx || !ny || !ht_filter_args_ok(out_width, out_height, max_factor)) return HT_ERR_INVALID;
    ht_filter_align_record_factors(*record, out_width, out_height, max_factor, nx, ny);
    return HT_OK;
}

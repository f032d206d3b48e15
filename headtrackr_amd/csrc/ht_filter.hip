// ht_filter.hip — prefiltered face crops: each patch pixel the mean of an Nx x Ny block of the unfiltered rule's samples
// (ht_camshift_crop_pairs_filtered_device / ht_camshift_crop_sources_filtered_device / ht_camshift_align_pairs_filtered_device /
// ht_camshift_align_sources_filtered_device / ht_camshift_crop_filter_factors / ht_camshift_align_filter_factors).
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
// stage: the RGBA dword store (DT == FM_RGBA8, format == NULL) or ht_patch.hip's PtStore<DT>.
namespace {

constexpr int FM_RGBA8 = -1;  // the DT of a call without a format
constexpr int FM_MAXF = HT_FILTER_MAX_FACTOR;

// the RGBA8 output stage: the pixel's dword into packed rows of dw pixels (PtStore's interface)
struct FmDwordStore {
    uint32_t *__restrict__ base;  // the entry's patch
    int dw, dh;
    __device__ __forceinline__ void operator()(uint32_t o, int x, int y) const { (base + x)[(size_t)y * dw] = o; }
};

constexpr int FM_ROWS = IG_NT / IG_TW;  // rows a workgroup's threads cover at once: a tile is RPT * FM_ROWS rows

template <int DT>
__device__ __forceinline__ auto fm_store(uint8_t *base, int dw, int dh, const PtFormat &pf) {
    if constexpr (DT == FM_RGBA8) return FmDwordStore{reinterpret_cast<uint32_t *>(base), dw, dh};
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

// an empty entry: f(0) — zero bytes, or bias[c] in the dtype — for this thread's pixels of the tile, in front of the barrier
template <int RPT, class STORE>
__device__ __forceinline__ void fm_empty(const STORE &store, int dw, int dh) {
    const int x = blockIdx.x * IG_TW + (threadIdx.x & (IG_TW - 1)), y0 = blockIdx.y * (RPT * FM_ROWS) + threadIdx.x / IG_TW;
    if (x >= dw) return;
#pragma unroll
    for (int k = 0; k < RPT; k++) {
        const int y = y0 + k * FM_ROWS;
        if (y < dh) store(0u, x, y);
    }
}

#undef IG_STORE
#define IG_STORE(o, x, y) ((void)out, (void)(x), (void)(y), fm_add(acc[k], o))  // k: the bodies' row index of the thread, a constant once unrolled

// k_crop_list (ht_crop.hip) over the fine patch, averaged: the same table, rule and record; the taps are the fine patch's
template <int DT, int RPT>
__global__ __launch_bounds__(IG_NT) void k_cut_mean(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                    int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, int max_factor, PtFormat pf,
                                                    ht_crop_record *__restrict__ recs) {
    constexpr int IG_RPT = RPT, IG_TH = RPT * FM_ROWS;  // the tile of THIS kernel: the pixel bodies' text reads these two names
    __shared__ RsTap s_colf[FM_MAXF * IG_TW], s_rowf[FM_MAXF * IG_TH];
    const CrDesc &e = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = e.d;
    const int format = d.format, stream = e.stream;
    const HtCsState &st = states[stream];
    ht_cs_rect rc;
    const int32_t code = ht_crop_rule(st.x, st.y, st.width, st.height, cw_canvas, ch_canvas, e.SW, e.SH, d.sx, d.sy, d.sw, d.sh, margin_q8, flags, &rc);
    const int sx = rc.x, sy = rc.y, sw = rc.width, sh = rc.height;
    if ((blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) {  // the record the unfiltered call would have written: rx = w / P
        ht_crop_record r;
        r.code = code, r.stream = stream, r.rect = rc;
        r.rx = code == HT_CROP_FACE ? (double)sw / (double)dw : 0.0, r.ry = code == HT_CROP_FACE ? (double)sh / (double)dh : 0.0;
        recs[blockIdx.z] = r;
    }
    const auto store = fm_store<DT>(dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf);
    if (code != HT_CROP_FACE) {  // uniform
        fm_empty<RPT>(store, dw, dh);
        return;
    }
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
    if (format == HT_DRAW_RGBA) {
        const uint8_t *__restrict__ src = (const uint8_t *)d.p0;
        const size_t src_pitch = d.pitch0, src_stride = 0;
#pragma unroll 1
        for (int b = 0; b < ny; b++)
#pragma unroll 1
            for (int a = 0; a < nx; a++) {
                const RsTap *s_col = s_colf + a * IG_TW, *s_row = s_rowf + b * IG_TH;
#define IG_BODY_PART 2  // IG_BODY_RGBA
#include "ht_ingest_bodies.inc"
            }
    } else {
        const uint8_t *__restrict__ yp = (const uint8_t *)d.p0, *__restrict__ up = (const uint8_t *)d.p1, *__restrict__ vp = (const uint8_t *)d.p2;
        const size_t y_pitch = d.pitch0, c_pitch = d.pitch1, stride = 0;
        const int cw = d.cw;
        const HtYuvCoef kc = d.kc;
        if (format == HT_YUV_FMT_NV12) {
            constexpr int FMT = HT_YUV_FMT_NV12;
#pragma unroll 1
            for (int b = 0; b < ny; b++)
#pragma unroll 1
                for (int a = 0; a < nx; a++) {
                    const RsTap *s_col = s_colf + a * IG_TW, *s_row = s_rowf + b * IG_TH;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
                }
        } else {
            constexpr int FMT = HT_YUV_FMT_I420;
#pragma unroll 1
            for (int b = 0; b < ny; b++)
#pragma unroll 1
                for (int a = 0; a < nx; a++) {
                    const RsTap *s_col = s_colf + a * IG_TW, *s_row = s_rowf + b * IG_TH;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
                }
        }
    }
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
    constexpr int TH = RPT * FM_ROWS;  // the tile's rows
    __shared__ int64_t s_cx[FM_MAXF * IG_TW], s_cy[FM_MAXF * IG_TW], s_rx[FM_MAXF * TH], s_ry[FM_MAXF * TH];
    const CrDesc &e = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = e.d;
    const int format = d.format, stream = e.stream, SW = e.SW, SH = e.SH;
    const HtCsState &st = states[stream];
    HtAlignPlan pl;
    const int32_t code = ht_align_rule(st.x, st.y, st.width, st.height, st.angle, cw_canvas, ch_canvas, SW, SH, d.sx, d.sy, d.sw, d.sh, margin_q8, flags, &pl);
    if ((blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) {
        ht_align_record r;
        r.code = code, r.stream = stream, r.a12 = pl.a12, r.pad = 0;
        r.cx = pl.cx, r.cy = pl.cy, r.ux = pl.ux, r.uy = pl.uy, r.vx = pl.vx, r.vy = pl.vy;
        recs[blockIdx.z] = r;
    }
    const auto store = fm_store<DT>(dst + (size_t)blockIdx.z * dst_stride, dw, dh, pf);
    if (code != HT_ALIGN_FACE) {  // uniform
        fm_empty<RPT>(store, dw, dh);
        return;
    }
    const int nx = ht_filter_align_factor(pl.ux, pl.uy, dw, max_factor), ny = ht_filter_align_factor(pl.vx, pl.vy, dh, max_factor);  // uniform
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * TH;
    for (int t = threadIdx.x; t < nx * IG_TW; t += IG_NT) {  // [a][column]: fine column nx * x + a of nx * dw
        const int i = nx * min(X0 + (t & (IG_TW - 1)), dw - 1) + t / IG_TW;
        s_cx[t] = pl.cx - 32768 + ht_align_term(i, nx * dw, pl.ux);
        s_cy[t] = pl.cy - 32768 + ht_align_term(i, nx * dw, pl.uy);
    }
    for (int t = threadIdx.x; t < ny * TH; t += IG_NT) {  // [b][row]
        const int j = ny * min(Y0 + (t & (TH - 1)), dh - 1) + t / TH;
        s_rx[t] = ht_align_term(j, ny * dh, pl.vx);
        s_ry[t] = ht_align_term(j, ny * dh, pl.vy);
    }
    __syncthreads();
    FmAccum<RPT> sum = {{}, Y0 + (int)(threadIdx.x / IG_TW)};
#pragma unroll 1
    for (int b = 0; b < ny; b++)
#pragma unroll 1
        for (int a = 0; a < nx; a++) {
            const int64_t *cx = s_cx + a * IG_TW, *cy = s_cy + a * IG_TW, *rx = s_rx + b * TH, *ry = s_ry + b * TH;
            if (format == HT_DRAW_RGBA) al_pixels<HT_DRAW_RGBA, FmAccum<RPT>, RPT>(d, SW, SH, cx, cy, rx, ry, sum, dw, dh);
            else if (format == HT_YUV_FMT_NV12) al_pixels<HT_YUV_FMT_NV12, FmAccum<RPT>, RPT>(d, SW, SH, cx, cy, rx, ry, sum, dw, dh);
            else al_pixels<HT_YUV_FMT_I420, FmAccum<RPT>, RPT>(d, SW, SH, cx, cy, rx, ry, sum, dw, dh);
        }
    fm_finish<RPT>(sum.acc, (uint32_t)(nx * ny), store, dw, dh);
}

// the tile of a call: the siblings' 64 x 16 up to max_factor 2, 64 x 4 beyond (more, shorter workgroups for the long block loops)
constexpr int FM_SMALL_FROM = 3;

template <int RPT>
void fm_cut(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_crop_params &p, int32_t max_factor,
            const ht_patch_format *fmt, ht_crop_record *recs) {
    const PtFormat pf = fmt ? pt_format(*fmt) : PtFormat{};
    auto k = !fmt ? k_cut_mean<FM_RGBA8, RPT> : fmt->dtype == HT_PATCH_F32 ? k_cut_mean<HT_PATCH_F32, RPT> : fmt->dtype == HT_PATCH_F16 ? k_cut_mean<HT_PATCH_F16, RPT>
                                                                                                                                   : k_cut_mean<HT_PATCH_BF16, RPT>;
    grid.y = (p.out_height + RPT * FM_ROWS - 1) / (RPT * FM_ROWS);
    hipLaunchKernelGGL(k, grid, dim3(IG_NT), 0, c->stream, tab, states, out, ostride, (int)p.out_width, (int)p.out_height, c->W, c->H, (int)p.margin_q8, p.flags,
                       (int)max_factor, pf, recs);
}

void fm_launch_cut(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_crop_params &p, int32_t max_factor,
                   const ht_patch_format *fmt, ht_crop_record *recs) {
    if (max_factor < FM_SMALL_FROM) fm_cut<IG_RPT>(c, grid, tab, states, out, ostride, p, max_factor, fmt, recs);
    else fm_cut<1>(c, grid, tab, states, out, ostride, p, max_factor, fmt, recs);
}

template <int RPT>
void fm_upright(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_align_params &p, int32_t max_factor,
                const ht_patch_format *fmt, ht_align_record *recs) {
    const PtFormat pf = fmt ? pt_format(*fmt) : PtFormat{};
    auto k = !fmt ? k_upright_mean<FM_RGBA8, RPT> : fmt->dtype == HT_PATCH_F32 ? k_upright_mean<HT_PATCH_F32, RPT> : fmt->dtype == HT_PATCH_F16 ? k_upright_mean<HT_PATCH_F16, RPT>
                                                                                                                                           : k_upright_mean<HT_PATCH_BF16, RPT>;
    grid.y = (p.out_height + RPT * FM_ROWS - 1) / (RPT * FM_ROWS);
    hipLaunchKernelGGL(k, grid, dim3(IG_NT), 0, c->stream, tab, states, out, ostride, (int)p.out_width, (int)p.out_height, c->W, c->H, (int)p.margin_q8, p.flags,
                       (int)max_factor, pf, recs);
}

void fm_launch_upright(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_align_params &p, int32_t max_factor,
                       const ht_patch_format *fmt, ht_align_record *recs) {
    if (max_factor < FM_SMALL_FROM) fm_upright<IG_RPT>(c, grid, tab, states, out, ostride, p, max_factor, fmt, recs);
    else fm_upright<1>(c, grid, tab, states, out, ostride, p, max_factor, fmt, recs);
}

// max_factor is checked behind the context and in front of everything else of the call
ht_status fm_check_factor(ht_ctx *c, const char *fn, int32_t max_factor) {
    if (max_factor < HT_FILTER_MIN_FACTOR || max_factor > HT_FILTER_MAX_FACTOR) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": max_factor must be 1..8");
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_crop_pairs_filtered_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, int32_t max_factor,
                                                            const ht_patch_format *format, void *out_dev, size_t out_stride) {
    const char *fn = "ht_camshift_crop_pairs_filtered_device";
    if (!c) return HT_ERR_INVALID;
    const ht_status st = fm_check_factor(c, fn, max_factor);
    return st != HT_OK ? st : crop_pairs(c, fn, pairs, n, params, format != nullptr, format, out_dev, out_stride, max_factor);
}

extern "C" ht_status ht_camshift_crop_sources_filtered_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                              int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride) {
    const char *fn = "ht_camshift_crop_sources_filtered_device";
    if (!c) return HT_ERR_INVALID;
    const ht_status st = fm_check_factor(c, fn, max_factor);
    return st != HT_OK ? st : crop_sources(c, fn, streams, srcs, n, params, format != nullptr, format, out_dev, out_stride, max_factor);
}

extern "C" ht_status ht_camshift_align_pairs_filtered_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, int32_t max_factor,
                                                             const ht_patch_format *format, void *out_dev, size_t out_stride) {
    const char *fn = "ht_camshift_align_pairs_filtered_device";
    if (!c) return HT_ERR_INVALID;
    const ht_status st = fm_check_factor(c, fn, max_factor);
    return st != HT_OK ? st : align_pairs(c, fn, pairs, n, params, format != nullptr, format, out_dev, out_stride, max_factor);
}

extern "C" ht_status ht_camshift_align_sources_filtered_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                               int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride) {
    const char *fn = "ht_camshift_align_sources_filtered_device";
    if (!c) return HT_ERR_INVALID;
    const ht_status st = fm_check_factor(c, fn, max_factor);
    return st != HT_OK ? st : align_sources(c, fn, streams, srcs, n, params, format != nullptr, format, out_dev, out_stride, max_factor);
}

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

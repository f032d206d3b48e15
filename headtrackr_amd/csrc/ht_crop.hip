// ht_crop.hip — the output side of the K-feed host: each tracker's box cut from its feed and scaled to a patch, on the device
// (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device / ht_camshift_crop_result / ht_camshift_crop_records_device).
//
// A track step leaves its track object in HtCsState on the device, in canvas coordinates.  The face PIXELS are in the feed's own frame
// (or, pairs form, in the bound canvas frame).  Mapping the box back, rounding it and scaling the rect to the patch size needs nothing from
// the host: the rule is integer arithmetic (ht_crop_plan.h, host and device text), the resampler is the text of ht_ingest_bodies.inc,
// which takes the destination size as dw, dh.  Included at the end of ht_ingest.hip, behind ht_draw_list.hip: same code object, same
// anonymous-namespace helpers (DlDesc, dl_gptr, the tile constants, ig_channel, ig_chroma_read).
//
// k_crop_list: grid (tile column, tile row, entry), 64 x 16 patch pixels and 256 threads per workgroup, the shape of k_draw_list.  A
// workgroup reads its entry's 120-byte descriptor — the draw list's descriptor, whose rect is the MAPPING rect, plus the source's size and
// the stream — and the four object fields of that stream's state with scalar loads (uniform index, const __restrict__), runs the rule
// (workgroup-uniform), divides the two ratios, and then is k_draw_list with (sx, sy, sw, sh) = the rule's rect and (dw, dh) = the patch
// size.  An empty entry stores zeros for its tile instead and returns in front of the barrier (uniformly).  Workgroup (0, 0) of an entry
// writes its 40-byte record.  The table travels as dl_upload's does, through a ring and a device table of its own (ht_internal.h).
#include "ht_crop_plan.h"  // HT_CROP_FN and HT_CSB_FN are defined in front of this file's #include (ht_ingest.hip)
#include "ht_patch_plan.h"  // the model-input tensors' format (ht_patch.hip): checked here, with everything else a call is checked for

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

__global__ __launch_bounds__(IG_NT) void k_crop_list(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                     int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, ht_crop_record *__restrict__ recs) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
    const CrDesc &e = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = e.d;
    const int format = d.format, stream = e.stream;
    const HtCsState &st = states[stream];
    ht_cs_rect rc;
    const int32_t code = ht_crop_rule(st.x, st.y, st.width, st.height, cw_canvas, ch_canvas, e.SW, e.SH, d.sx, d.sy, d.sw, d.sh, margin_q8, flags, &rc);
    const int sx = rc.x, sy = rc.y, sw = rc.width, sh = rc.height;
    // one correctly rounded binary64 division each: the bits of the host's (double)sw / (double)dw
    const double rx = code == HT_CROP_FACE ? (double)sw / (double)dw : 0.0, ry = code == HT_CROP_FACE ? (double)sh / (double)dh : 0.0;
    if ((blockIdx.x | blockIdx.y) == 0 && threadIdx.x == 0) {
        ht_crop_record r;
        r.code = code, r.stream = stream, r.rect = rc, r.rx = rx, r.ry = ry;
        recs[blockIdx.z] = r;
    }
    if (code != HT_CROP_FACE) {  // uniform: zeros for this tile, in front of the barrier
        const int x = blockIdx.x * IG_TW + (threadIdx.x & (IG_TW - 1)), y0 = blockIdx.y * IG_TH + threadIdx.x / IG_TW;
        uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride);
        if (x < dw)
#pragma unroll
            for (int k = 0; k < IG_RPT; k++) {
                const int y = y0 + k * (IG_NT / IG_TW);
                if (y < dh) out[(size_t)y * dw + x] = 0u;
            }
        return;
    }
#define IG_BODY_PART 1  // IG_BODY_TAPS
#include "ht_ingest_bodies.inc"
    __syncthreads();
    if (format == HT_DRAW_RGBA) {
        const uint8_t *__restrict__ src = (const uint8_t *)d.p0;
        const size_t src_pitch = d.pitch0, src_stride = 0;
#define IG_BODY_PART 2  // IG_BODY_RGBA
#include "ht_ingest_bodies.inc"
    } else {
        const uint8_t *__restrict__ yp = (const uint8_t *)d.p0, *__restrict__ up = (const uint8_t *)d.p1, *__restrict__ vp = (const uint8_t *)d.p2;
        const size_t y_pitch = d.pitch0, c_pitch = d.pitch1, stride = 0;
        const int cw = d.cw;
        const HtYuvCoef kc = d.kc;
        if (format == HT_YUV_FMT_NV12) {
            constexpr int FMT = HT_YUV_FMT_NV12;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
        } else {
            constexpr int FMT = HT_YUV_FMT_I420;
#define IG_BODY_PART 3  // IG_BODY_YUV
#include "ht_ingest_bodies.inc"
        }
    }
}

// the buffers of a call of n entries: the device table with its ring of pinned slots (dl_upload's scheme) and the records with their pinned
// twin.  Allocates (and then waits for the stream) only on the first call or for a longer list.
ht_status crop_reserve(ht_ctx *c, const char *fn, size_t n) {
    if (c->crop_rec_cap >= n && c->ev_crop) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cap = std::max(n, (size_t)64);
    if (c->d_crop_tab) (void)hipFree(c->d_crop_tab);
    if (c->d_crop_rec) (void)hipFree(c->d_crop_rec);
    if (c->h_crop_rec) (void)hipHostFree(c->h_crop_rec);
    c->d_crop_tab = c->d_crop_rec = c->h_crop_rec = nullptr, c->crop_tab_cap = c->crop_rec_cap = 0, c->crop_n = 0;
    for (auto &h : c->h_crop_tab) {
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
    bool ok = hipMalloc(reinterpret_cast<void **>(&c->d_crop_tab), cap * sizeof(HtCropDesc)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&c->d_crop_rec), cap * sizeof(ht_crop_record)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&c->h_crop_rec), cap * sizeof(ht_crop_record), hipHostMallocDefault) == hipSuccess;
    for (int k = 0; ok && k < ht_ctx::HT_DL_STAGE; k++) {
        ok = hipHostMalloc(reinterpret_cast<void **>(&c->h_crop_tab[k]), cap * sizeof(HtCropDesc), hipHostMallocDefault) == hipSuccess;
        if (ok && !c->ev_crop_tab[k]) ok = hipEventCreateWithFlags(&c->ev_crop_tab[k], hipEventDisableTiming) == hipSuccess;
    }
    if (ok && !c->ev_crop) ok = hipEventCreateWithFlags(&c->ev_crop, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": allocation of the crop table failed");
    }
    c->crop_tab_cap = cap * sizeof(HtCropDesc), c->crop_rec_cap = cap;
    return HT_OK;
}

// the tensor forms' launches (ht_patch.hip, behind ht_align.hip): the same grid and arguments, another output stage
void pt_launch_cut(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_crop_params &p, const ht_patch_format &fmt,
                   ht_crop_record *recs);
// the prefiltered forms' launch (ht_filter.hip, behind ht_patch.hip): fmt == nullptr is RGBA8
void fm_launch_cut(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_crop_params &p, int32_t max_factor,
                   const ht_patch_format *fmt, ht_crop_record *recs);

// the checks both forms share, in front of their entries: the context's state first, then the call's own arguments.  tensor: the output
// is fmt's tensor (ht_patch_plan.h) instead of RGBA8 — fmt is checked here and a patch's bytes and the default stride are the tensor's
ht_status crop_check(ht_ctx *c, const std::string &f, bool pairs_form, const void *list, int32_t n, const ht_crop_params *p, const void *out_dev, size_t out_stride,
                     size_t *pbytes, size_t *ostride, bool tensor = false, const ht_patch_format *fmt = nullptr) {
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (c->cs_streams <= 0 || !c->d_cs) return ht_fail(c, HT_ERR_STATE, f + ": call ht_camshift_reserve first");
    if (pairs_form && (!c->d_frames || c->nframes <= 0)) return ht_fail(c, HT_ERR_STATE, f + ": bind frames first");
    if (!list || n <= 0 || n > HT_DRAW_LIST_MAX) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_list_message(HT_DRAW_LIST_BAD_COUNT));
    if (!p) return ht_fail(c, HT_ERR_INVALID, f + ": NULL params");
    if (p->out_width < 1 || p->out_width > HT_CROP_MAX_OUT || p->out_height < 1 || p->out_height > HT_CROP_MAX_OUT)
        return ht_fail(c, HT_ERR_INVALID, f + ": out_width / out_height must be 1..1024");
    if (p->margin_q8 < HT_CROP_MIN_MARGIN || p->margin_q8 > HT_CROP_MAX_MARGIN) return ht_fail(c, HT_ERR_INVALID, f + ": margin_q8 must be 64..1024");
    if (p->flags & ~(uint32_t)HT_CROP_SQUARE) return ht_fail(c, HT_ERR_INVALID, f + ": unknown flag");
    if (tensor) {
        if (!fmt) return ht_fail(c, HT_ERR_INVALID, f + ": NULL format");
        const int fs = ht_patch_check_format(fmt);
        if (fs != HT_PATCH_FMT_OK) return ht_fail(c, HT_ERR_INVALID, f + ": format: " + ht_patch_format_message(fs));
    }
    if (!out_dev || ((uintptr_t)out_dev & 3)) return ht_fail(c, HT_ERR_INVALID, f + ": NULL or misaligned output (4-byte alignment required)");
    *pbytes = tensor ? ht_patch_bytes(p->out_width, p->out_height, fmt->dtype, fmt->channels) : (size_t)p->out_width * p->out_height * 4;
    *ostride = out_stride ? out_stride : ht_patch_default_stride(*pbytes);
    if ((*ostride & 3) || *ostride < *pbytes) return ht_fail(c, HT_ERR_INVALID, f + ": output stride smaller than a patch or not a multiple of 4");
    return HT_OK;
}

// everything has been checked: table, kernel, records to the pinned twin
// max_factor != 0: a prefiltered call (ht_filter.hip)
ht_status crop_launch(ht_ctx *c, const char *fn, const std::vector<HtCropDesc> &desc, const ht_crop_params &p, uint8_t *out, size_t ostride,
                      const ht_patch_format *fmt = nullptr, int32_t max_factor = 0) {
    const size_t n = desc.size(), need = n * sizeof(HtCropDesc);
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st = crop_reserve(c, fn, n);
    if (st != HT_OK) return st;
    const int k = c->crop_stage_next;
    c->crop_stage_next = (k + 1) % ht_ctx::HT_DL_STAGE;
    HT_HIP(c, hipEventSynchronize(c->ev_crop_tab[k]));  // never recorded: returns at once
    std::memcpy(c->h_crop_tab[k], desc.data(), need);
    HT_HIP(c, hipMemcpyAsync(c->d_crop_tab, c->h_crop_tab[k], need, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_crop_tab[k], c->stream));
    c->crop_n = 0;  // until this call's copy is behind its kernel
    const dim3 grid((p.out_width + IG_TW - 1) / IG_TW, (p.out_height + IG_TH - 1) / IG_TH, (unsigned)n);
    if (max_factor) {
        HtProfScope ps(c, "cut_mean");
        fm_launch_cut(c, grid, reinterpret_cast<const CrDesc *>(c->d_crop_tab), (const HtCsState *)c->d_cs, out, ostride, p, max_factor, fmt, reinterpret_cast<ht_crop_record *>(c->d_crop_rec));
        HT_HIP(c, hipGetLastError());
    } else if (fmt) {
        HtProfScope ps(c, "cut_tensor");
        pt_launch_cut(c, grid, reinterpret_cast<const CrDesc *>(c->d_crop_tab), (const HtCsState *)c->d_cs, out, ostride, p, *fmt, reinterpret_cast<ht_crop_record *>(c->d_crop_rec));
        HT_HIP(c, hipGetLastError());
    } else {
        HtProfScope ps(c, "crop_list");
        hipLaunchKernelGGL(k_crop_list, grid, dim3(IG_NT), 0, c->stream, reinterpret_cast<const CrDesc *>(c->d_crop_tab), (const HtCsState *)c->d_cs, out, ostride,
                           (int)p.out_width, (int)p.out_height, c->W, c->H, (int)p.margin_q8, p.flags, reinterpret_cast<ht_crop_record *>(c->d_crop_rec));
        HT_HIP(c, hipGetLastError());
    }
    HT_HIP(c, hipMemcpyAsync(c->h_crop_rec, c->d_crop_rec, n * sizeof(ht_crop_record), hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_crop, c->stream));
    c->crop_n = (int)n;
    return HT_OK;
}

// both pairs-form calls: fn names the export; tensor: ht_camshift_crop_pairs_tensor_device (ht_patch.hip)
ht_status crop_pairs(ht_ctx *c, const char *fn, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, bool tensor, const ht_patch_format *fmt, void *out_dev,
                     size_t out_stride, int32_t max_factor = 0) {
    if (!c) return HT_ERR_INVALID;
    HtRange range(fn);
    const std::string f(fn);
    size_t pbytes = 0, ostride = 0;
    ht_status st = crop_check(c, f, true, pairs, n, params, out_dev, out_stride, &pbytes, &ostride, tensor, fmt);
    if (st != HT_OK) return st;
    const size_t fbytes = (size_t)c->W * c->H * 4, total = (size_t)(n - 1) * ostride + pbytes;
    std::vector<HtCropDesc> desc((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const int32_t s = pairs[i].stream, fr = pairs[i].frame;
        if (s < 0 || s >= c->cs_streams) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": stream " + std::to_string(s) + " is not reserved");
        if (fr < 0 || fr >= c->nframes) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": frame " + std::to_string(fr) + " is not bound");
        const uint8_t *frame = c->d_frames + (size_t)fr * c->frame_stride;
        if (ig_overlap(frame, fbytes, out_dev, total))
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": the bound frame and the output overlap");
        HtCropDesc e = {};
        e.d.p0 = frame, e.d.pitch0 = (size_t)c->W * 4, e.d.format = HT_DRAW_RGBA;
        e.d.sx = e.d.sy = 0, e.d.sw = c->W, e.d.sh = c->H;  // the canvas IS the source: drawn 1:1
        e.SW = c->W, e.SH = c->H, e.stream = s;
        desc[(size_t)i] = e;
    }
    return crop_launch(c, fn, desc, *params, static_cast<uint8_t *>(out_dev), ostride, fmt, max_factor);
}

// both sources-form calls
ht_status crop_sources(ht_ctx *c, const char *fn, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params, bool tensor,
                       const ht_patch_format *fmt, void *out_dev, size_t out_stride, int32_t max_factor = 0) {
    if (!c) return HT_ERR_INVALID;
    HtRange range(fn);
    const std::string f(fn);
    size_t pbytes = 0, ostride = 0;
    ht_status st = crop_check(c, f, false, srcs, n, params, out_dev, out_stride, &pbytes, &ostride, tensor, fmt);
    if (st != HT_OK) return st;
    if (!streams) return ht_fail(c, HT_ERR_INVALID, f + ": NULL streams");
    std::vector<HtCropDesc> desc((size_t)n);
    std::vector<HtDrawExtent> ext((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        if (streams[i] < 0 || streams[i] >= c->cs_streams)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": stream " + std::to_string(streams[i]) + " is not reserved");
        HtCropDesc e = {};
        const int ps = ht_draw_list_plan_entry(srcs[i], c->W, c->H, &e.d, &ext[(size_t)i]);  // an entry's rules are the draw list's: asked, not restated
        if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": " + ht_draw_list_message(ps));
        e.SW = srcs[i].width, e.SH = srcs[i].height, e.stream = streams[i];
        desc[(size_t)i] = e;
    }
    const int32_t bad = ht_draw_list_overlap(ext.data(), n, out_dev, (size_t)(n - 1) * ostride + pbytes);
    if (bad >= 0) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane and the output overlap");
    return crop_launch(c, fn, desc, *params, static_cast<uint8_t *>(out_dev), ostride, fmt, max_factor);
}

}  // namespace

extern "C" ht_status ht_camshift_crop_pairs_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, void *out_dev, size_t out_stride) {
    return crop_pairs(c, "ht_camshift_crop_pairs_device", pairs, n, params, false, nullptr, out_dev, out_stride);
}

extern "C" ht_status ht_camshift_crop_sources_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                     void *out_dev, size_t out_stride) {
    return crop_sources(c, "ht_camshift_crop_sources_device", streams, srcs, n, params, false, nullptr, out_dev, out_stride);
}

extern "C" ht_status ht_camshift_crop_result(ht_ctx *c, int32_t n, ht_crop_record *out) {
    if (!c) return HT_ERR_INVALID;
    if (c->crop_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_crop_result: no crop call to report on");
    if (n != c->crop_n) return ht_fail(c, HT_ERR_STATE, "ht_camshift_crop_result: n differs from the last crop call");
    if (!out) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_crop_result: NULL out");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventSynchronize(c->ev_crop));
    std::memcpy(out, c->h_crop_rec, (size_t)n * sizeof(ht_crop_record));
    return HT_OK;
}

extern "C" ht_status ht_camshift_crop_records_device(ht_ctx *c, const void **records, int32_t *n) {
    if (!c) return HT_ERR_INVALID;
    if (!records || !n) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_crop_records_device: NULL argument");
    if (c->crop_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_crop_records_device: no crop call yet");
    *records = c->d_crop_rec, *n = c->crop_n;
    return HT_OK;
}

void ht_crop_free(ht_ctx *c) {  // ht_ingest_free (ht_destroy: the stream has been synchronised)
    if (c->d_crop_tab) (void)hipFree(c->d_crop_tab);
    if (c->d_crop_rec) (void)hipFree(c->d_crop_rec);
    if (c->h_crop_rec) (void)hipHostFree(c->h_crop_rec);
    if (c->ev_crop) (void)hipEventDestroy(c->ev_crop);
    c->d_crop_tab = c->d_crop_rec = c->h_crop_rec = nullptr, c->ev_crop = nullptr, c->crop_tab_cap = c->crop_rec_cap = 0, c->crop_n = 0;
    for (int k = 0; k < ht_ctx::HT_DL_STAGE; k++) {
        if (c->h_crop_tab[k]) (void)hipHostFree(c->h_crop_tab[k]);
        if (c->ev_crop_tab[k]) (void)hipEventDestroy(c->ev_crop_tab[k]);
        c->h_crop_tab[k] = nullptr, c->ev_crop_tab[k] = nullptr;
    }
    c->crop_stage_next = 0;
}

// ht_align.hip — the angle-aligned face crops: each tracker's ROTATED box cut from its feed and sampled upright, on the device
// (ht_camshift_align_pairs_device / ht_camshift_align_sources_device / ht_camshift_align_result / ht_camshift_align_records_device).
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

// the output stage of k_align_list: the pixel's RGBA8 dword into packed rows of dw pixels
struct AlDwordStore {
    uint32_t *__restrict__ base;  // the entry's patch
    int dw;
    __device__ __forceinline__ void operator()(uint32_t o, int x, int y) const { (base + x)[(size_t)y * dw] = o; }
};

// the four rows of a thread's column, behind the barrier; every pixel ends in ONE output stage, store(o, x, y), o the pixel's RGBA8 dword
// (k_align_list: AlDwordStore; ht_patch.hip: the model-input tensors).  RPT rows per thread: a tile of RPT * 4 rows (ht_filter.hip takes 1)
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

__global__ __launch_bounds__(IG_NT) void k_align_list(const CrDesc *__restrict__ tab, const HtCsState *__restrict__ states, uint8_t *__restrict__ dst, size_t dst_stride,
                                                      int dw, int dh, int cw_canvas, int ch_canvas, int margin_q8, uint32_t flags, ht_align_record *__restrict__ recs) {
    __shared__ int64_t s_cx[IG_TW], s_cy[IG_TW], s_rx[IG_TH], s_ry[IG_TH];
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
    const int X0 = blockIdx.x * IG_TW, Y0 = blockIdx.y * IG_TH;
    if (code != HT_ALIGN_FACE) {  // uniform: zeros for this tile, in front of the barrier
        const int x = X0 + (threadIdx.x & (IG_TW - 1)), y0 = Y0 + threadIdx.x / IG_TW;
        uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride);
        if (x < dw)
#pragma unroll
            for (int k = 0; k < IG_RPT; k++) {
                const int y = y0 + k * (IG_NT / IG_TW);
                if (y < dh) out[(size_t)y * dw + x] = 0u;
            }
        return;
    }
    // the column terms carry the centre and the pixel-centre offset: a pixel adds its row's term and is done
    if (threadIdx.x < IG_TW) {
        const int i = min(X0 + (int)threadIdx.x, dw - 1);
        s_cx[threadIdx.x] = pl.cx - 32768 + ht_align_term(i, dw, pl.ux);
        s_cy[threadIdx.x] = pl.cy - 32768 + ht_align_term(i, dw, pl.uy);
    } else if (threadIdx.x < IG_TW + IG_TH) {
        const int j = min(Y0 + (int)threadIdx.x - IG_TW, dh - 1);
        s_rx[threadIdx.x - IG_TW] = ht_align_term(j, dh, pl.vx);
        s_ry[threadIdx.x - IG_TW] = ht_align_term(j, dh, pl.vy);
    }
    __syncthreads();
    const AlDwordStore store = {reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride), dw};
    if (format == HT_DRAW_RGBA) al_pixels<HT_DRAW_RGBA>(d, SW, SH, s_cx, s_cy, s_rx, s_ry, store, dw, dh);
    else if (format == HT_YUV_FMT_NV12) al_pixels<HT_YUV_FMT_NV12>(d, SW, SH, s_cx, s_cy, s_rx, s_ry, store, dw, dh);
    else al_pixels<HT_YUV_FMT_I420>(d, SW, SH, s_cx, s_cy, s_rx, s_ry, store, dw, dh);
}

// the buffers of a call of n entries, as crop_reserve's: allocates (and then waits for the stream) only on the first call or for a longer list
ht_status align_reserve(ht_ctx *c, const char *fn, size_t n) {
    if (c->align_rec_cap >= n && c->ev_align) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cap = std::max(n, (size_t)64);
    if (c->d_align_tab) (void)hipFree(c->d_align_tab);
    if (c->d_align_rec) (void)hipFree(c->d_align_rec);
    if (c->h_align_rec) (void)hipHostFree(c->h_align_rec);
    c->d_align_tab = c->d_align_rec = c->h_align_rec = nullptr, c->align_tab_cap = c->align_rec_cap = 0, c->align_n = 0;
    for (auto &h : c->h_align_tab) {
        if (h) (void)hipHostFree(h);
        h = nullptr;
    }
    bool ok = hipMalloc(reinterpret_cast<void **>(&c->d_align_tab), cap * sizeof(HtCropDesc)) == hipSuccess &&
              hipMalloc(reinterpret_cast<void **>(&c->d_align_rec), cap * sizeof(ht_align_record)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&c->h_align_rec), cap * sizeof(ht_align_record), hipHostMallocDefault) == hipSuccess;
    for (int k = 0; ok && k < ht_ctx::HT_DL_STAGE; k++) {
        ok = hipHostMalloc(reinterpret_cast<void **>(&c->h_align_tab[k]), cap * sizeof(HtCropDesc), hipHostMallocDefault) == hipSuccess;
        if (ok && !c->ev_align_tab[k]) ok = hipEventCreateWithFlags(&c->ev_align_tab[k], hipEventDisableTiming) == hipSuccess;
    }
    if (ok && !c->ev_align) ok = hipEventCreateWithFlags(&c->ev_align, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": allocation of the align table failed");
    }
    c->align_tab_cap = cap * sizeof(HtCropDesc), c->align_rec_cap = cap;
    return HT_OK;
}

// the checks both forms share, in front of their entries, are the crop calls' OWN (crop_check, ht_crop.hip): same fields, same bounds, same words
static_assert(HT_ALIGN_SQUARE == HT_CROP_SQUARE && sizeof(ht_align_params) == sizeof(ht_crop_params), "align params are crop params");
void pt_launch_upright(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_align_params &p,
                       const ht_patch_format &fmt, ht_align_record *recs);  // ht_patch.hip
void fm_launch_upright(ht_ctx *c, dim3 grid, const CrDesc *tab, const HtCsState *states, uint8_t *out, size_t ostride, const ht_align_params &p, int32_t max_factor,
                       const ht_patch_format *fmt, ht_align_record *recs);  // ht_filter.hip: the prefiltered forms; fmt == nullptr is RGBA8

ht_status align_check(ht_ctx *c, const std::string &f, bool pairs_form, const void *list, int32_t n, const ht_align_params *p, const void *out_dev, size_t out_stride,
                      size_t *pbytes, size_t *ostride, bool tensor = false, const ht_patch_format *fmt = nullptr) {
    ht_crop_params q = {};
    if (p) q.out_width = p->out_width, q.out_height = p->out_height, q.margin_q8 = p->margin_q8, q.flags = p->flags;
    return crop_check(c, f, pairs_form, list, n, p ? &q : nullptr, out_dev, out_stride, pbytes, ostride, tensor, fmt);
}

// everything has been checked: table, kernel, records to the pinned twin
// max_factor != 0: a prefiltered call (ht_filter.hip)
ht_status align_launch(ht_ctx *c, const char *fn, const std::vector<HtCropDesc> &desc, const ht_align_params &p, uint8_t *out, size_t ostride,
                       const ht_patch_format *fmt = nullptr, int32_t max_factor = 0) {
    const size_t n = desc.size(), need = n * sizeof(HtCropDesc);
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st = align_reserve(c, fn, n);
    if (st != HT_OK) return st;
    const int k = c->align_stage_next;
    c->align_stage_next = (k + 1) % ht_ctx::HT_DL_STAGE;
    HT_HIP(c, hipEventSynchronize(c->ev_align_tab[k]));  // never recorded: returns at once
    std::memcpy(c->h_align_tab[k], desc.data(), need);
    HT_HIP(c, hipMemcpyAsync(c->d_align_tab, c->h_align_tab[k], need, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_align_tab[k], c->stream));
    c->align_n = 0;  // until this call's copy is behind its kernel
    const dim3 grid((p.out_width + IG_TW - 1) / IG_TW, (p.out_height + IG_TH - 1) / IG_TH, (unsigned)n);
    if (max_factor) {
        HtProfScope ps(c, "upright_mean");
        fm_launch_upright(c, grid, reinterpret_cast<const CrDesc *>(c->d_align_tab), (const HtCsState *)c->d_cs, out, ostride, p, max_factor, fmt, reinterpret_cast<ht_align_record *>(c->d_align_rec));
        HT_HIP(c, hipGetLastError());
    } else if (fmt) {
        HtProfScope ps(c, "upright_tensor");
        pt_launch_upright(c, grid, reinterpret_cast<const CrDesc *>(c->d_align_tab), (const HtCsState *)c->d_cs, out, ostride, p, *fmt, reinterpret_cast<ht_align_record *>(c->d_align_rec));
        HT_HIP(c, hipGetLastError());
    } else {
        HtProfScope ps(c, "align_list");
        hipLaunchKernelGGL(k_align_list, grid, dim3(IG_NT), 0, c->stream, reinterpret_cast<const CrDesc *>(c->d_align_tab), (const HtCsState *)c->d_cs, out, ostride,
                           (int)p.out_width, (int)p.out_height, c->W, c->H, (int)p.margin_q8, p.flags, reinterpret_cast<ht_align_record *>(c->d_align_rec));
        HT_HIP(c, hipGetLastError());
    }
    HT_HIP(c, hipMemcpyAsync(c->h_align_rec, c->d_align_rec, n * sizeof(ht_align_record), hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_align, c->stream));
    c->align_n = (int)n;
    return HT_OK;
}

// both pairs-form calls: fn names the export; tensor: ht_camshift_align_pairs_tensor_device (ht_patch.hip)
ht_status align_pairs(ht_ctx *c, const char *fn, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, bool tensor, const ht_patch_format *fmt, void *out_dev,
                      size_t out_stride, int32_t max_factor = 0) {
    if (!c) return HT_ERR_INVALID;
    HtRange range(fn);
    const std::string f(fn);
    size_t pbytes = 0, ostride = 0;
    ht_status st = align_check(c, f, true, pairs, n, params, out_dev, out_stride, &pbytes, &ostride, tensor, fmt);
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
    return align_launch(c, fn, desc, *params, static_cast<uint8_t *>(out_dev), ostride, fmt, max_factor);
}

// both sources-form calls
ht_status align_sources(ht_ctx *c, const char *fn, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params, bool tensor,
                        const ht_patch_format *fmt, void *out_dev, size_t out_stride, int32_t max_factor = 0) {
    if (!c) return HT_ERR_INVALID;
    HtRange range(fn);
    const std::string f(fn);
    size_t pbytes = 0, ostride = 0;
    ht_status st = align_check(c, f, false, srcs, n, params, out_dev, out_stride, &pbytes, &ostride, tensor, fmt);
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
    return align_launch(c, fn, desc, *params, static_cast<uint8_t *>(out_dev), ostride, fmt, max_factor);
}

}  // namespace

extern "C" ht_status ht_camshift_align_pairs_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, void *out_dev, size_t out_stride) {
    return align_pairs(c, "ht_camshift_align_pairs_device", pairs, n, params, false, nullptr, out_dev, out_stride);
}

extern "C" ht_status ht_camshift_align_sources_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                      void *out_dev, size_t out_stride) {
    return align_sources(c, "ht_camshift_align_sources_device", streams, srcs, n, params, false, nullptr, out_dev, out_stride);
}

extern "C" ht_status ht_camshift_align_result(ht_ctx *c, int32_t n, ht_align_record *out) {
    if (!c) return HT_ERR_INVALID;
    if (c->align_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_align_result: no align call to report on");
    if (n != c->align_n) return ht_fail(c, HT_ERR_STATE, "ht_camshift_align_result: n differs from the last align call");
    if (!out) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_align_result: NULL out");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventSynchronize(c->ev_align));
    std::memcpy(out, c->h_align_rec, (size_t)n * sizeof(ht_align_record));
    return HT_OK;
}

extern "C" ht_status ht_camshift_align_records_device(ht_ctx *c, const void **records, int32_t *n) {
    if (!c) return HT_ERR_INVALID;
    if (!records || !n) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_align_records_device: NULL argument");
    if (c->align_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_align_records_device: no align call yet");
    *records = c->d_align_rec, *n = c->align_n;
    return HT_OK;
}

void ht_align_free(ht_ctx *c) {  // ht_ingest_free (ht_destroy: the stream has been synchronised)
    if (c->d_align_tab) (void)hipFree(c->d_align_tab);
    if (c->d_align_rec) (void)hipFree(c->d_align_rec);
    if (c->h_align_rec) (void)hipHostFree(c->h_align_rec);
    if (c->ev_align) (void)hipEventDestroy(c->ev_align);
    c->d_align_tab = c->d_align_rec = c->h_align_rec = nullptr, c->ev_align = nullptr, c->align_tab_cap = c->align_rec_cap = 0, c->align_n = 0;
    for (int k = 0; k < ht_ctx::HT_DL_STAGE; k++) {
        if (c->h_align_tab[k]) (void)hipHostFree(c->h_align_tab[k]);
        if (c->ev_align_tab[k]) (void)hipEventDestroy(c->ev_align_tab[k]);
        c->h_align_tab[k] = nullptr, c->ev_align_tab[k] = nullptr;
    }
    c->align_stage_next = 0;
}

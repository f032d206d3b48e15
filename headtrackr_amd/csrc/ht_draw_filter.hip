// ht_draw_filter.hip — the draw list with a prefilter for strong downscales (ht_draw_list_filtered_device / ht_draw_filter_factors): each
// canvas pixel the mean of an Nx x Ny block of the UNFILTERED draw's samples.  ht_draw_filter_plan.h states the rule and plans a call on the
// host; the rounding is ht_filter_plan.h's.  Included at the end of ht_ingest.hip: same code object as k_draw_list and k_cut_mean, whose
// helpers (fm_add, fm_finish, LpDwordStore) and shared text it takes.
//
// k_draw_list_mean_tile<RPT>: grid (tile column, tile row, entry), 256 threads; a tile is 64 columns by RPT * 4 rows, RPT rows per thread
// (the library launches RPT 1, a 64 x 4 tile, at every max_factor: see dm_rpt_of).  A
// workgroup reads its entry's 112-byte descriptor — HtDrawDesc with the FINE ratios, then Nx, Ny — with scalar loads (blockIdx.z is uniform,
// the table const __restrict__).  The taps of the tile's fine columns and rows go to LDS, Nx * 64 + Ny * 4 RPT of them laid out [a][column]
// and [b][row] (the arrays hold factor 8: 15 KB at RPT 4, 13 KB at RPT 1); one barrier; then for every (b, a) of the block — a
// workgroup-uniform loop — the format's pixel body of ht_ingest_bodies.inc runs on tap slice a / b, through ht_list_parts.inc's scaffold,
// with an IG_STORE that ADDS the sample's four bytes to the thread's sums.  A fine sample is therefore the unfiltered rule's byte by
// construction: the binary64 blend of ig_channel, never contracted, rounded half to even; YUV taps converted first.  ht_filter_pixel
// rounds the sums and the dword is stored.  Source rows are not staged in LDS: a block's Nx fine taps of one output pixel lie side by side
// in the source, and the vector cache serves the neighbours (DESIGN.md §2.3.8 has the measurement).
#include "ht_draw_filter_plan.h"

namespace {

typedef HtDrawMeanDescT<dl_gptr> DmDesc;
static_assert(sizeof(DmDesc) == sizeof(HtDrawMeanDesc) && alignof(DmDesc) == alignof(HtDrawMeanDesc), "the kernel's view of a descriptor is the host's");

#undef IG_STORE
#define IG_STORE(o, x, y) ((void)out, (void)(x), (void)(y), fm_add(acc[k], o))  // k: the bodies' row index of the thread, a constant once unrolled

// (the name: k_draw_list_mean with the tile behind it.  In a listing of the code object the kernels that END in _mean<..> are the face
// crops' — tests/test_filter_cpu.py names them all — and a thin k_draw_list_mean over a tile function template was tried: it reordered
// k_cut_mean<-1, 1>'s epilogue, which shares fm_finish.  As a kernel template of its own it leaves every neighbour's instructions alone.)
template <int RPT>
__global__ __launch_bounds__(IG_NT) void k_draw_list_mean_tile(const DmDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    constexpr int IG_RPT = RPT, IG_TH = RPT * FM_ROWS;  // the tile of THIS kernel: the shared text reads these two names
    __shared__ RsTap s_colf[FM_MAXF * IG_TW], s_rowf[FM_MAXF * IG_TH];
    const DmDesc &m = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const DlDesc &d = m.d;
    const int sx = d.sx, sy = d.sy, sw = d.sw, sh = d.sh, format = d.format;
    const int nx = min(max(m.nx, 1), FM_MAXF), ny = min(max(m.ny, 1), FM_MAXF);  // the plan's 1 .. 8; the clamp keeps the LDS index in bounds whatever the table holds
    const double rx = d.rx, ry = d.ry;  // the fine frame's: sw / (nx dw), sh / (ny dh), divided on the host
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
    // the 64 x 16 form draws YUYV / UYVY entries too: every draw of a packed 4:2:2 source is k_draw_list_mean_tile<IG_RPT>'s (dm_launch).  The
    // 64 x 4 form, which every other filtered call takes, stays the instructions it was: with the branch it measured 10 - 17 % slower on lists
    // WITHOUT a packed entry (81 against 74 us at max_factor 8, 57 against 49 us at 4)
#define LP_PACKED_422 (RPT == 4)
#define LP_PART 4  // LP_SCAFFOLD
#include "ht_list_parts.inc"
    fm_finish<RPT>(acc, (uint32_t)(nx * ny), LpDwordStore{reinterpret_cast<uint32_t *>(dst + (size_t)blockIdx.z * dst_stride), dw}, dw, dh);
}

#undef IG_STORE
#define IG_STORE IG_STORE_DWORD  // the default again, for whatever is compiled behind this file

// the tile of a call: 64 x 4 (RPT 1) at every max_factor.  Unlike the face crops' 112 x 112 patches a canvas has tiles enough for either form, and
// the short workgroups won at every factor: on eight feeds -> 320 x 240, 74 against 100 us at max_factor 8, 18.5 against 20.9 us at 2, 9.2
// against 10.0 us at 1 (profiles/draw_filter.txt).  The 64 x 16 form stays compiled behind the context option draw_filter_rows = 16, for
// tools/gpu_draw_filter.py's comparison and the tests that pin both forms to the same bytes.
int dm_rpt_of(const ht_ctx *c) { return c->draw_filter_rows ? c->draw_filter_rows / FM_ROWS : 1; }

// dw x dh: the destination frames' size — the canvas, or (dm_unpack_sources) a source's own size
ht_status dm_launch(ht_ctx *c, const char *fn, const std::vector<HtDrawMeanDesc> &desc, uint8_t *dst, size_t dstride, int dw = 0, int dh = 0) {
    ht_status st = dl_upload(c, fn, desc);  // the draw list's staged table (ht_draw_list.hip)
    if (st != HT_OK) return st;
    HtProfScope ps(c, "draw_list_mean");
    if (!dw) dw = c->W, dh = c->H;
    const bool packed = std::any_of(desc.begin(), desc.end(), [](const HtDrawMeanDesc &m) { return ht_yuv_is_422(m.d.format); });
    const int rpt = packed ? IG_RPT : dm_rpt_of(c);  // (LP_PACKED_422: the 64 x 16 form alone holds the packed pixel body)
    const dim3 grid((dw + IG_TW - 1) / IG_TW, (dh + rpt * FM_ROWS - 1) / (rpt * FM_ROWS), (unsigned)desc.size());
    const DmDesc *tab = reinterpret_cast<const DmDesc *>(c->dl_tab.d);
    hipLaunchKernelGGL(rpt == 1 ? k_draw_list_mean_tile<1> : k_draw_list_mean_tile<IG_RPT>, grid, dim3(IG_NT), 0, c->stream, tab, dst, dstride, dw, dh);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

// The UNFILTERED draw of a list that holds packed 4:2:2 entries (ht_draw_list_device, ht_draw_frames_yuv*: declared in ht_ingest_yuv.hip).
// k_draw_list, k_draw_yuv<> and the face-patch kernels are held to the registers they have (tests/golden/draw_filter_neighbours.json), so the
// packed pixel body lives in this file's kernel alone, and factors (1, 1) are ht_draw_list_device's bytes by the declared rule: the same
// taps and ratios, one sample per pixel, (s + 0) / 1.  It is not the shape one would build for it: profiles/ingest_422.txt has the cost
// (10.7 against 9.2 us for k_draw_yuv<NV12> on eight 1080p feeds -> 320 x 240, 125 against 84 us at 1 : 1).
ht_status dm_launch_unfiltered(ht_ctx *c, const char *fn, const HtDrawDesc *desc, size_t n, uint8_t *dst, size_t dstride) {
    std::vector<HtDrawMeanDesc> m(n);
    for (size_t i = 0; i < n; i++) m[i].d = desc[i], m[i].nx = m[i].ny = 1;
    return dm_launch(c, fn, m, dst, dstride);
}

// The face-patch calls on packed 4:2:2 sources (declared in ht_crop.hip, called by ht_face_calls.hip behind every check of the call).  Their
// kernels hold no packed body, so each packed entry's frame is first UNPACKED: drawn 1 : 1 onto an RGBA frame of its own size in the context's
// staging buffer — at ratio 1 every tap weight is (1, 0), so that frame is the declared conversion itself —, and the entry is rewritten to
// the RGBA entry of that frame (same size, rect, ratios, stream: the same bytes and the same record by the calls' own contract).  One launch
// per packed entry (the frames have sizes of their own), the whole frame at 4 B/px: a pass the fused kernels exist to avoid, and what a list
// without packed entries never pays.
//
// ORIENTED entries (orient[i] != 0, ht_orient_plan.h; any format) take the same route through the module's kernel (or_upright,
// ht_draw_list.hip): the frame drawn is O, orient(convert(S)), of SW x SH — an oriented packed entry is ONE pass, not two — and the entry,
// whose rect and size are O's already, becomes the RGBA entry of that frame.  The same cost in the same words: one more launch and the whole
// frame at 4 B/px per oriented entry.
ht_status dm_unpack_sources(ht_ctx *c, const char *fn, std::vector<HtCropDesc> &desc, const int32_t *orient) {
    size_t need = 0;
    const auto turned = [&](size_t i) { return orient && orient[i] != 0; };
    for (size_t i = 0; i < desc.size(); i++)
        if (turned(i) || ht_yuv_is_422(desc[i].d.format)) need += (size_t)desc[i].SW * (size_t)desc[i].SH * 4;
    if (!need) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    ht_status rs = or_stage_reserve(c, fn, need, "unpacked 4:2:2 / oriented sources");
    if (rs != HT_OK) return rs;
    size_t at = 0;
    std::vector<HtOrientDesc> jobs;
    std::vector<uint8_t *> frames;
    for (size_t i = 0; i < desc.size(); i++) {
        if (!turned(i)) continue;
        HtCropDesc &e = desc[i];
        HtOrientDesc o = {};
        o.d.p0 = (const uint8_t *)e.d.p0, o.d.p1 = (const uint8_t *)e.d.p1, o.d.p2 = (const uint8_t *)e.d.p2, o.d.pitch0 = e.d.pitch0, o.d.pitch1 = e.d.pitch1;
        o.d.cw = e.d.cw, o.d.format = e.d.format, o.d.kc = e.d.kc, o.orient = orient[i];
        ht_orient_size(orient[i], e.SW, e.SH, &o.d.sw, &o.d.sh);  // the stored size back from O's (the swap is its own inverse)
        jobs.push_back(ht_orient_whole(o));
        frames.push_back(c->d_ingest_src + at);
        e.d.p0 = frames.back(), e.d.p1 = e.d.p2 = nullptr, e.d.pitch0 = (size_t)e.SW * 4, e.d.pitch1 = 0, e.d.cw = 0, e.d.format = HT_DRAW_RGBA, e.d.kc = HtYuvCoef{};
        at += (size_t)e.SW * (size_t)e.SH * 4;
    }
    if ((rs = or_upright(c, fn, jobs, frames)) != HT_OK) return rs;
    std::vector<HtDrawMeanDesc> one(1);
    for (HtCropDesc &e : desc) {
        if (!ht_yuv_is_422(e.d.format)) continue;  // (an oriented packed entry is RGBA by now)
        HtDrawMeanDesc &m = one[0];
        m = HtDrawMeanDesc{};
        m.d.p0 = (const uint8_t *)e.d.p0, m.d.pitch0 = e.d.pitch0, m.d.rx = m.d.ry = 1.0;
        m.d.sx = m.d.sy = 0, m.d.sw = e.SW, m.d.sh = e.SH, m.d.cw = e.d.cw, m.d.format = e.d.format, m.d.kc = e.d.kc;
        m.nx = m.ny = 1;
        uint8_t *frame = c->d_ingest_src + at;
        const ht_status st = dm_launch(c, fn, one, frame, 0, e.SW, e.SH);
        if (st != HT_OK) return st;
        e.d.p0 = frame, e.d.p1 = e.d.p2 = nullptr, e.d.pitch0 = (size_t)e.SW * 4, e.d.pitch1 = 0, e.d.cw = 0, e.d.format = HT_DRAW_RGBA, e.d.kc = HtYuvCoef{};
        at += (size_t)e.SW * (size_t)e.SH * 4;
    }
    return HT_OK;
}

// The filtered draw of a list that holds oriented entries (odesc: ht_orient_plan's, every check of the call passed).  Each oriented entry's
// frame is drawn 1 : 1 into the staging buffer (or_upright) and the entry planned as the RGBA entry of that O, with the rect it had — the
// call's bytes by its own definition; the other entries are planned as they are.  The same cost as above: one more launch and the whole frame at
// 4 B/px per oriented entry.
ht_status dm_orient_first(ht_ctx *c, const char *fn, const ht_draw_source *srcs, int32_t max_factor, const std::vector<HtOrientDesc> &odesc, std::vector<HtDrawMeanDesc> &desc) {
    size_t need = 0;
    for (const HtOrientDesc &o : odesc)
        if (o.orient) need += (size_t)o.d.sw * (size_t)o.d.sh * 4;
    ht_status st = or_stage_reserve(c, fn, need, "oriented sources");
    if (st != HT_OK) return st;
    std::vector<HtOrientDesc> jobs;
    std::vector<uint8_t *> frames;
    size_t at = 0;
    for (const HtOrientDesc &o : odesc) {
        if (!o.orient) continue;
        jobs.push_back(ht_orient_whole(o));
        frames.push_back(c->d_ingest_src + at);
        at += (size_t)o.d.sw * (size_t)o.d.sh * 4;
    }
    if ((st = or_upright(c, fn, jobs, frames)) != HT_OK) return st;
    size_t j = 0;
    for (size_t i = 0; i < odesc.size(); i++) {
        ht_draw_source s = srcs[i];
        if (odesc[i].orient) s = ht_orient_upright(srcs[i], odesc[i].orient, frames[j++]);
        else s.format = HT_FORMAT_OF(s.format);
        HtDrawExtent unused;
        const int ps = ht_draw_filter_plan_entry(s, c->W, c->H, max_factor, &desc[i], &unused);
        if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": entry " + std::to_string(i) + ": " + ht_draw_filter_message(ps));  // (ht_orient_plan admitted it)
    }
    return HT_OK;
}

}  // namespace

// ht_draw_list_device's host path with ht_draw_filter_plan in the place of ht_draw_list_plan: everything is checked before anything is enqueued
extern "C" ht_status ht_draw_list_filtered_device(ht_ctx *c, const ht_draw_source *srcs, int32_t n, int32_t max_factor, void *dst_dev, size_t dst_frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_list_filtered_device");
    const char *fn = "ht_draw_list_filtered_device";
    const std::string f(fn);
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_list_message(HT_DRAW_LIST_BAD_COUNT));
    if (!ht_draw_filter_factor_ok(max_factor)) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_filter_message(HT_DRAW_FILTER_BAD_FACTOR));
    if ((uintptr_t)dst_dev & 3) return ht_fail(c, HT_ERR_INVALID, f + ": misaligned destination (4-byte alignment required)");
    const size_t fbytes = (size_t)c->W * c->H * 4, dstride = dst_dev && dst_frame_stride ? dst_frame_stride : fbytes;
    if ((dstride & 3) || dstride < fbytes) return ht_fail(c, HT_ERR_INVALID, f + ": destination frame stride smaller than a frame or not a multiple of 4");
    std::vector<HtDrawMeanDesc> desc((size_t)n);
    std::vector<HtDrawExtent> ext((size_t)n);
    int32_t bad = -1;
    // a list with an oriented entry (ht_orient_plan.h) is checked by ht_orient_plan — the rects against O, the extents of the stored planes —
    // and, behind every check of the call, ORIENTS FIRST (dm_orient_first): a list without one takes the path it always took
    std::vector<HtOrientDesc> odesc;
    const bool oriented = std::any_of(srcs, srcs + n, [](const ht_draw_source &s) { return ht_orient_present(s.format); });
    if (oriented) odesc.resize((size_t)n);
    const int ps = oriented ? ht_orient_plan(srcs, n, c->W, c->H, odesc.data(), ext.data(), &bad) : ht_draw_filter_plan(srcs, n, c->W, c->H, max_factor, desc.data(), ext.data(), &bad);
    if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": " + ht_draw_filter_message(ps));
    HT_HIP(c, hipSetDevice(c->device));
    if (oriented) {  // a missing module is reported before anything is touched
        const OrModule *m = nullptr;
        const ht_status st = or_module(c, fn, &m);
        if (st != HT_OK) return st;
    }
    if (!dst_dev) {
        if (n > c->max_batch)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(c->max_batch) + ": more entries than the geometry's batch capacity");
        // the buffer as it is now and as far as this call writes it: defensive only, see ht_draw_frames_device
        if ((bad = ht_draw_list_overlap(ext.data(), n, c->d_frames_own, std::max(c->d_frames_own_bytes, fbytes * (size_t)n))) >= 0)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane lies inside the context's own frame buffer");
        ht_status st = ht_frames_own_reserve(c, fbytes * (size_t)n, fn);  // the contract of ig_draw_bound from here on
        if (st != HT_OK) return st;
        if (oriented && (st = dm_orient_first(c, fn, srcs, max_factor, odesc, desc)) != HT_OK) return st;
        if ((st = dm_launch(c, fn, desc, c->d_frames_own, fbytes)) != HT_OK) return st;
        ht_frames_bind_own(c, n);
        return HT_OK;
    }
    if ((bad = ht_draw_list_overlap(ext.data(), n, dst_dev, (size_t)(n - 1) * dstride + fbytes)) >= 0)
        return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane and the destination overlap");
    if (oriented) {
        const ht_status st = dm_orient_first(c, fn, srcs, max_factor, odesc, desc);
        if (st != HT_OK) return st;
    }
    return dm_launch(c, fn, desc, static_cast<uint8_t *>(dst_dev), dstride);
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

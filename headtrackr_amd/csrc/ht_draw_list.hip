// ht_draw_list.hip — the K-feed form of the video -> canvas draw: ONE launch draws a list of sources that share nothing (the reference's
// loop is one drawImage per feed, main.js:170).  Every entry has its own device allocation(s), size, pitches, format (RGBA, NV12, I420; YUYV and UYVY: see dl_launch),
// matrix and source rect; entry i goes onto destination frame i with the bytes ht_draw_frames_device / ht_draw_frames_yuv_device give for
// it alone.  Included at the end of ht_ingest.hip, so it is part of the same code object and shares that file's and ht_ingest_yuv.hip's
// text: the tile constants, ig_channel, ig_chroma_read and, through ht_ingest_bodies.inc, the taps and the three pixel bodies.
//
// k_draw_list: grid (tile column, tile row, entry), 64 x 16 destination pixels and 256 threads per workgroup.  A workgroup reads its
// entry's 104-byte descriptor (ht_draw_list_plan.h) — blockIdx.z is uniform and the table is const __restrict__, so these are scalar
// loads —, computes the tile's 80 taps from that entry's ratios and rect into LDS, and behind the barrier takes a workgroup-uniform branch
// into one of the three bodies.  The table reaches the device
// through a staged table (HtStagedTable, ht_internal.h: a ring of pinned slots and one hipMemcpyAsync on the ctx stream per call), as
// every list call's table does.  DESIGN.md §2.3.2 gives the reasoning and the registers.
#include <cstring>
#include <vector>

#include "ht_draw_list_plan.h"

namespace {

// a plane pointer out of the table is a GLOBAL address (ht_draw_list_device takes device pointers), and the kernel's view of the table
// says so in the member type: the bodies' reads are then global_load like the single-source kernels', whose pointers are kernel
// arguments, and not flat_load (a generic pointer loaded from memory says nothing about its address space).  Same bytes, same layout.
typedef const __attribute__((address_space(1))) uint8_t *dl_gptr;
typedef HtDrawDescT<dl_gptr> DlDesc;
static_assert(sizeof(DlDesc) == sizeof(HtDrawDesc) && alignof(DlDesc) == alignof(HtDrawDesc), "the kernel's view of a descriptor is the host's");

// every piece below is ht_ingest_bodies.inc: the text k_draw_frames and k_draw_yuv<> compile, with their parameter names bound to the entry
__global__ __launch_bounds__(IG_NT) void k_draw_list(const DlDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    __shared__ RsTap s_col[IG_TW], s_row[IG_TH];
    const DlDesc &d = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const int sx = d.sx, sy = d.sy, sw = d.sw, sh = d.sh, format = d.format;
    const double rx = d.rx, ry = d.ry;
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

// the table of a call on the device: through the context's staged descriptor table (HtStagedTable, ht_internal.h).  DESC: HtDrawDesc, or
// the filtered draw's wider descriptor (ht_draw_filter.hip) — both calls are the draw list and share the table
template <class DESC>
ht_status dl_upload(ht_ctx *c, const char *fn, const std::vector<DESC> &desc) {
    const size_t need = desc.size() * sizeof(DESC);
    ht_status st = ht_stage_reserve(c, &c->dl_tab, need, 64 * sizeof(HtDrawDesc), std::string(fn) + ": allocation of the descriptor table failed");
    if (st != HT_OK) return st;
    uint8_t *slot = nullptr;
    if ((st = ht_stage_take(c, &c->dl_tab, &slot)) != HT_OK) return st;
    std::memcpy(slot, desc.data(), need);
    return ht_stage_commit(c, &c->dl_tab, need);
}

ht_status dl_launch(ht_ctx *c, const char *fn, const std::vector<HtDrawDesc> &desc, uint8_t *dst, size_t dstride) {
    // a list with a packed 4:2:2 entry (YUYV / UYVY) is drawn by the filtered draw's kernel at factors (1, 1): the same bytes, and the one
    // kernel that holds the packed pixel body (ht_draw_filter.hip)
    if (std::any_of(desc.begin(), desc.end(), [](const HtDrawDesc &d) { return ht_yuv_is_422(d.format); })) return dm_launch_unfiltered(c, fn, desc.data(), desc.size(), dst, dstride);
    ht_status st = dl_upload(c, fn, desc);
    if (st != HT_OK) return st;
    HtProfScope ps(c, "draw_list");
    const dim3 grid((c->W + IG_TW - 1) / IG_TW, (c->H + IG_TH - 1) / IG_TH, (unsigned)desc.size());
    hipLaunchKernelGGL(k_draw_list, grid, dim3(IG_NT), 0, c->stream, reinterpret_cast<const DlDesc *>(c->dl_tab.d), dst, dstride, c->W, c->H);
    HT_HIP(c, hipGetLastError());
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_draw_list_device(ht_ctx *c, const ht_draw_source *srcs, int32_t n, void *dst_dev, size_t dst_frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_draw_list_device");
    const char *fn = "ht_draw_list_device";
    const std::string f(fn);
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (!srcs || n <= 0 || n > HT_DRAW_LIST_MAX) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_list_message(HT_DRAW_LIST_BAD_COUNT));
    if ((uintptr_t)dst_dev & 3) return ht_fail(c, HT_ERR_INVALID, f + ": misaligned destination (4-byte alignment required)");
    const size_t fbytes = (size_t)c->W * c->H * 4, dstride = dst_dev && dst_frame_stride ? dst_frame_stride : fbytes;
    if ((dstride & 3) || dstride < fbytes) return ht_fail(c, HT_ERR_INVALID, f + ": destination frame stride smaller than a frame or not a multiple of 4");
    std::vector<HtDrawDesc> desc((size_t)n);
    std::vector<HtDrawExtent> ext((size_t)n);
    int32_t bad = -1;
    const int ps = ht_draw_list_plan(srcs, n, c->W, c->H, desc.data(), ext.data(), &bad);
    if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": " + ht_draw_list_message(ps));
    HT_HIP(c, hipSetDevice(c->device));
    if (!dst_dev) {
        if (n > c->max_batch)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(c->max_batch) + ": more entries than the geometry's batch capacity");
        // the buffer as it is now (it may be freed and reallocated for this call) and as far as this call writes it: defensive only, see
        // ht_draw_frames_device
        if ((bad = ht_draw_list_overlap(ext.data(), n, c->d_frames_own, std::max(c->d_frames_own_bytes, fbytes * (size_t)n))) >= 0)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane lies inside the context's own frame buffer");
        ht_status st = ht_frames_own_reserve(c, fbytes * (size_t)n, fn);  // the contract of ig_draw_bound from here on
        if (st != HT_OK) return st;
        if ((st = dl_launch(c, fn, desc, c->d_frames_own, fbytes)) != HT_OK) return st;
        ht_frames_bind_own(c, n);
        return HT_OK;
    }
    if ((bad = ht_draw_list_overlap(ext.data(), n, dst_dev, (size_t)(n - 1) * dstride + fbytes)) >= 0)
        return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane and the destination overlap");
    return dl_launch(c, fn, desc, static_cast<uint8_t *>(dst_dev), dstride);
}

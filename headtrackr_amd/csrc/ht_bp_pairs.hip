// ht_bp_pairs.hip — camshift's back-projection over an arbitrary list of (stream, frame) pairs (ht_camshift_backproject_pairs / _device).
//
// ht_camshift_backproject pairs stream first + i with bound frame i.  Here output i is bound frame pairs[i].frame through the model of
// stream pairs[i].stream: every tracker of one canvas (camshift.MultiTracker) or every tracking feed of a host gets its
// getBackProjectionImg() / getPdf() (camshift.js:172-196, 314-353) from ONE call.  The histogram depends on the frame alone and so does
// the pixel stream, so both are shared: three launches on the context's stream,
//
//   k_csp_hist         grid (chunks, distinct frames): the pair unit's histogram pass itself, into THIS unit's scratch (d_bp_hist)
//   k_bpp_lut          grid (64, groups) x 512: a block sums its 64 bins over the frame's chunk histograms once and writes the weight and
//                      the expanded pixel of every pair of its group
//   k_bpp_project      grid (chunks, groups) x 1024: the workgroup holds the LUTs of its whole group in LDS (4 x 16 KB RGBA8, 2 x 32 KB
//                      binary64), reads its chunk of the frame once and writes the chunk of every output of the group
//
// A group is up to G pairs of the call that share a frame (ht_bp_pairs_plan.h).  Bytes per pixel for M trackers on one frame:
// 4 (histogram) + 4 ceil(M / G) + out M, against M (8 + out) for M copies of the frame under ht_camshift_backproject.  Integer operations
// and single correctly rounded binary64 operations only: the bytes are the reference's and those of ht_camshift_backproject.
//
// Compiled as part of ht_backproject.hip (included at its end, behind ht_cs_pairs.hip, whose csp_plan / csp_upload / k_csp_hist it uses):
// the library keeps ONE code object besides the three that profiles/traffic.json fingerprints, and no kernel name here carries one of
// the fingerprint's markers.  The call uses the back-projection unit's scratch only — d_bp_hist, the LUT buffers, d_bp_out — and the pair
// table's staging ring: nothing a track call reads or writes besides the frames and the models, so it may sit between enqueue-only
// track steps.
#include "ht_bp_pairs_plan.h"

namespace {

// the group's pairs share the sum over the chunk histograms (k_bp_lut's order: wavefront q sums every 8th chunk from q, then q = 0 .. 7);
// wavefront j < count then writes the LUT entries of pair j of the group
__global__ __launch_bounds__(BP_LUT_NT) void k_bpp_lut(const uint32_t *__restrict__ hist, int nchunks, const HtCsState *__restrict__ states,
                                                       const CspEntry *__restrict__ entries, const HtBppGroup *__restrict__ groups,
                                                       double *__restrict__ lut_w, uint32_t *__restrict__ lut_px) {
    __shared__ uint32_t part[8][64];
    const HtBppGroup &g = groups[blockIdx.y];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, bin = blockIdx.x * 64 + lane;
    const uint32_t *cur = hist + (size_t)g.slot * nchunks * 4096 + bin;
    uint32_t ch = 0;
#pragma unroll 4
    for (int k = grp; k < nchunks; k += 8) ch += cur[(size_t)k * 4096];
    part[grp][lane] = ch;
    __syncthreads();
    if (grp < g.count) {  // count <= BPP_MAXG <= 8 wavefronts
        ch = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) ch += part[q][lane];
        const int pi = g.pair[grp];
        double p = 0.0;
        if (ch != 0) {
            p = __ddiv_rn((double)states[entries[pi].stream].model[bin], (double)ch);  // camshift.js:322-326
            p = p < 1.0 ? p : 1.0;
        }
        const uint32_t v = (uint32_t)floor(__dmul_rn(255.0, p));  // camshift.js:188
        lut_w[(size_t)pi * 4096 + bin] = p;
        lut_px[(size_t)pi * 4096 + bin] = v * 0x010101u | 0xFF000000u;  // camshift.js:189-192
    }
}

// workgroup (k, j) writes pixels [k chunk_px, (k + 1) chunk_px) of every output of group j.  The group's LUTs (64 KB when the group is
// full) go to LDS with four 16-byte loads per thread, issued in front of the first batch of pixel loads and stored behind it, as in
// k_bp_project; one barrier, then loads, LDS reads and stores: the bins of four pixels are computed once and looked up once per pair.
template <int KIND>
__global__ __launch_bounds__(BP_NT) void k_bpp_project(const uint8_t *__restrict__ frames, size_t frame_stride, uint32_t npix, uint32_t chunk_px,
                                                       const HtBppGroup *__restrict__ groups, const typename BpKind<KIND>::elem *__restrict__ lut_g,
                                                       uint8_t *__restrict__ out, size_t out_stride) {
    typedef typename BpKind<KIND>::elem elem;
    constexpr int G = (int)(65536 / (4096 * sizeof(elem)));         // LUTs in LDS: 4 (RGBA8) or 2 (F64)
    constexpr int LUT_V4 = (int)(4096 * sizeof(elem) / 16 / BP_NT);  // 16-byte pieces of ONE LUT per thread: 1 (RGBA8) or 2 (F64)
    __shared__ __attribute__((aligned(16))) elem lut[G][4096];
    const HtBppGroup &g = groups[blockIdx.y];
    const int cnt = g.count;  // 1 .. G
    const uint8_t *frame = frames + (size_t)g.frame * frame_stride;
    const uint32_t beg = blockIdx.x * chunk_px, end = min(beg + chunk_px, npix);  // chunk_px is a multiple of 4 * BP_NT; beg < npix
    const uint32_t nquad = (end - beg) / 4;
    const uint4 *img4 = reinterpret_cast<const uint4 *>(frame + (size_t)beg * 4);
    const uint32_t iters = chunk_px / (4 * BP_NT);  // >= 1
    // piece k = 0 .. 3 of the thread: 16 bytes of LUT k / LUT_V4 of the group (named registers: an array indexed under the workgroup-uniform
    // `pair exists` conditions is not promoted to registers)
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint4 lv0 = zero4, lv1 = zero4, lv2 = zero4, lv3 = zero4;
#define BPP_LUT_LOAD(k_) \
    if ((k_) / LUT_V4 < cnt) lv##k_ = reinterpret_cast<const uint4 *>(lut_g + (size_t)g.pair[(k_) / LUT_V4] * 4096)[((k_) % LUT_V4) * BP_NT + threadIdx.x]
#define BPP_LUT_STORE(k_) \
    if ((k_) / LUT_V4 < cnt) reinterpret_cast<uint4 *>(lut[(k_) / LUT_V4])[((k_) % LUT_V4) * BP_NT + threadIdx.x] = lv##k_
    static_assert(G * LUT_V4 == 4, "four 16-byte pieces per thread");
    BPP_LUT_LOAD(0);
    BPP_LUT_LOAD(1);
    BPP_LUT_LOAD(2);
    BPP_LUT_LOAD(3);
    for (uint32_t it0 = 0; it0 < iters; it0 += BP_UNROLL) {
        uint4 pv[BP_UNROLL];
        bool onv[BP_UNROLL];
#pragma unroll
        for (int u = 0; u < BP_UNROLL; u++) {
            const uint32_t i = (it0 + (uint32_t)u) * BP_NT + threadIdx.x;
            onv[u] = it0 + (uint32_t)u < iters && i < nquad;
            pv[u] = make_uint4(0u, 0u, 0u, 0u);
            if (onv[u]) pv[u] = img4[i];
        }
        if (it0 == 0) {  // workgroup-uniform: the LUTs land in LDS while the first pixels are on their way
            BPP_LUT_STORE(0);
            BPP_LUT_STORE(1);
            BPP_LUT_STORE(2);
            BPP_LUT_STORE(3);
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < BP_UNROLL; u++) {
            CS_BATCH_LOADED(pv[u].x);
            CS_BATCH_LOADED(pv[u].y);
            CS_BATCH_LOADED(pv[u].z);
            CS_BATCH_LOADED(pv[u].w);
        }
#pragma unroll
        for (int u = 0; u < BP_UNROLL; u++) {
            if (!onv[u]) continue;
            const uint32_t i = (it0 + (uint32_t)u) * BP_NT + threadIdx.x;
            const uint32_t b0 = cs_bin(pv[u].x), b1 = cs_bin(pv[u].y), b2 = cs_bin(pv[u].z), b3 = cs_bin(pv[u].w);
#pragma unroll
            for (int j = 0; j < G; j++)
                if (j < cnt) {
                    elem *dst = reinterpret_cast<elem *>(out + (size_t)g.pair[j] * out_stride);
                    bp_store4(dst + (size_t)beg + (size_t)i * 4, lut[j][b0], lut[j][b1], lut[j][b2], lut[j][b3]);
                }
        }
    }
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frame);
    for (uint32_t i = beg + nquad * 4 + threadIdx.x; i < end; i += BP_NT) {  // < 4 pixels
        const uint32_t b = cs_bin(img[i]);
#pragma unroll
        for (int j = 0; j < G; j++)
            if (j < cnt) reinterpret_cast<elem *>(out + (size_t)g.pair[j] * out_stride)[i] = lut[j][b];
    }
}

#undef BPP_LUT_LOAD
#undef BPP_LUT_STORE

int bpp_group_size(int32_t kind) { return kind == HT_BP_F64 ? 2 : 4; }

// every check of both entry points, before anything is enqueued: those of ht_camshift_backproject, with csp_plan's pair-list rules in
// place of the stream range
ht_status bpp_check(ht_ctx *c, const char *fn, const ht_cs_pair *pairs, int32_t n, int32_t kind, const void *out, size_t out_stride, CspPlan *plan,
                    size_t *frame_bytes, size_t *stride) {
    if (!c || !pairs || !out) return HT_ERR_INVALID;
    if (kind != HT_BP_RGBA8 && kind != HT_BP_F64) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": unknown output kind");
    ht_status st = csp_plan(c, fn, pairs, n, nullptr, plan);
    if (st != HT_OK) return st;
    *frame_bytes = (size_t)c->W * c->H * bp_elem(kind);
    *stride = out_stride ? out_stride : *frame_bytes;
    if (*stride < *frame_bytes) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": output stride smaller than a frame");
    return HT_OK;
}

// the three launches; d_out: device memory, output i `stride` bytes behind output i - 1
ht_status bpp_enqueue(ht_ctx *c, const char *fn, const CspPlan &plan, int32_t kind, void *d_out, size_t stride) {
    const uint32_t npix = (uint32_t)((size_t)c->W * c->H);
    if (npix == 0) return HT_OK;
    const int n = (int)plan.entries.size(), nd = (int)plan.frames.size();
    std::vector<int32_t> frames((size_t)n), slots((size_t)n);
    for (int i = 0; i < n; i++) frames[(size_t)i] = plan.entries[(size_t)i].frame, slots[(size_t)i] = plan.entries[(size_t)i].slot;
    const std::vector<HtBppGroup> groups = ht_bpp_plan(frames.data(), slots.data(), n, bpp_group_size(kind));
    const int ng = (int)groups.size();
    uint32_t chunk_px = 0, nchunks = 0;
    ht_cs_hist_plan(npix, nd, &chunk_px, &nchunks);
    ht_status st = bp_scratch(c, (size_t)nd, nchunks, (size_t)n);  // the back-projection unit's own: LUT slots by the pair's position in the call
    if (st != HT_OK) return st;
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr, *d_gwords = nullptr;
    st = csp_upload(c, fn, plan, &d_entries, &d_flist, groups.data(), (size_t)ng * (sizeof(HtBppGroup) / 4), &d_gwords);
    if (st != HT_OK) return st;
    const HtBppGroup *d_groups = reinterpret_cast<const HtBppGroup *>(d_gwords);
    {
        HtProfScope ps(c, "bpp_hist");
        hipLaunchKernelGGL(k_csp_hist, dim3(nchunks, nd), dim3(HIST_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px, d_flist, c->d_bp_hist);
        HT_HIP(c, hipGetLastError());
    }
    {
        HtProfScope ps(c, "bpp_lut");
        hipLaunchKernelGGL(k_bpp_lut, dim3(64, ng), dim3(BP_LUT_NT), 0, c->stream, c->d_bp_hist, (int)nchunks, c->d_cs, d_entries, d_groups, c->d_bp_lut_w,
                           c->d_bp_lut_px);
        HT_HIP(c, hipGetLastError());
    }
    {
        HtProfScope ps(c, "bpp_project");
        if (kind == HT_BP_RGBA8)
            hipLaunchKernelGGL(k_bpp_project<HT_BP_RGBA8>, dim3(nchunks, ng), dim3(BP_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px, d_groups,
                               c->d_bp_lut_px, static_cast<uint8_t *>(d_out), stride);
        else
            hipLaunchKernelGGL(k_bpp_project<HT_BP_F64>, dim3(nchunks, ng), dim3(BP_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px, d_groups,
                               c->d_bp_lut_w, static_cast<uint8_t *>(d_out), stride);
        HT_HIP(c, hipGetLastError());
    }
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_backproject_pairs_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out_dev, size_t out_stride) {
    HtRange range("ht_camshift_backproject_pairs_device");
    const char *fn = "ht_camshift_backproject_pairs_device";
    CspPlan plan;
    size_t frame_bytes = 0, stride = 0;
    ht_status st = bpp_check(c, fn, pairs, n, kind, out_dev, out_stride, &plan, &frame_bytes, &stride);
    if (st != HT_OK) return st;
    if (((uintptr_t)out_dev | stride) & (bp_elem(kind) - 1))
        return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": output pointer and stride must be multiples of the element size");
    if (plan.identity && !c->cs_pairs_force) return ht_camshift_backproject_device(c, plan.first, n, kind, out_dev, out_stride);
    HT_HIP(c, hipSetDevice(c->device));
    return bpp_enqueue(c, fn, plan, kind, out_dev, stride);
}

extern "C" ht_status ht_camshift_backproject_pairs(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out_host, size_t out_stride) {
    HtRange range("ht_camshift_backproject_pairs");
    const char *fn = "ht_camshift_backproject_pairs";
    CspPlan plan;
    size_t frame_bytes = 0, stride = 0;
    ht_status st = bpp_check(c, fn, pairs, n, kind, out_host, out_stride, &plan, &frame_bytes, &stride);
    if (st != HT_OK) return st;
    if (plan.identity && !c->cs_pairs_force) return ht_camshift_backproject(c, plan.first, n, kind, out_host, out_stride);
    if (frame_bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    st = bp_staging(c, (size_t)n * frame_bytes);
    if (st != HT_OK) return st;
    st = bpp_enqueue(c, fn, plan, kind, c->d_bp_out, frame_bytes);  // packed on the device; the caller's stride is applied by the copy
    if (st != HT_OK) return st;
    return bp_copy_out(c, out_host, stride, frame_bytes, n);
}

// ht_backproject.hip — camshift's back-projection on the device (reference: src/camshift.js).
//
//   getBackProjectionData  camshift.js:332-353   pdf(x, y) = w[bin(pixel(x, y))]
//   getWeights             camshift.js:314-330   w[b] = cur[b] ? min(model[b] / cur[b], 1) : 0
//   getBackProjectionImg   camshift.js:172-196   (v, v, v, 255), v = floor(255 * pdf)
//   getPdf                 camshift.js:172-175
//
// The track kernels (ht_camshift.hip) never write this image: they read the weights through a LUT straight into their moment sums.
// This unit materialises it on demand for the BOUND frames [0, n) through the models of streams [first, first + n), in three launches
// on the context's stream: (1) the chunk histograms of the frames — k_cs_hist itself, reached through ht_cs_hist_launch, into scratch
// of this unit; (2) k_bp_lut: per frame the 4096 weights (binary64) and the 4096 expanded pixels (u32); (3) k_bp_project: every
// workgroup copies its frame's LUT into LDS and streams its chunk of pixels through it.  Everything is an integer operation or ONE
// correctly rounded binary64 operation, so the output is the reference's, byte for byte.
//
// This unit also compiles ht_ingest.hip (the video -> canvas draw, included at the end of this file; its names are prefixed ig_ / IG_
// and share this file's anonymous namespace) and ht_cs_pairs.hip (camshift on (stream, frame) pairs, k_csp_*): the library keeps ONE code
// object besides the three fingerprinted ones.
//
// A translation unit of its own on purpose: profiles/traffic.json ties the committed hardware counters to the machine code of the
// pyramid, scan and camshift code objects (benchlib/fingerprint.py), which must not change for a debug surface.  The fingerprint finds
// a unit by a kernel-name substring; no kernel here may carry one of those markers in its name.
#include <algorithm>
#include <string>

#include "ht_internal.h"

namespace {

constexpr int BP_NT = 1024;   // threads of a k_bp_project workgroup: one chunk of the histogram pass's plan (a multiple of 4 * 1024 pixels)
constexpr int BP_UNROLL = 4;  // 16-byte loads of a thread in flight before the first lookup (k_cs_hist measured 4 as the optimum for this access pattern)
constexpr int BP_LUT_NT = 512;

// cs_bin, CS_BATCH_LOADED and the workgroup sizes of the histogram pass — and, for ht_cs_pairs.hip at the end of this file, every device
// helper of the camshift kernels
#include "ht_cs_device.h"

// LUTs of frame slot s from its chunk histograms and the model of stream first + s: grid (64, n) x 512 threads; a block owns 64 bins,
// its 8 wavefronts each sum every 8th chunk (the summation of k_cs_lut, without that kernel's cluster exchange slots).
__global__ __launch_bounds__(BP_LUT_NT) void k_bp_lut(const uint32_t *__restrict__ hist, int nchunks, const HtCsState *__restrict__ states, int first,
                                                      double *__restrict__ lut_w, uint32_t *__restrict__ lut_px) {
    __shared__ uint32_t part[8][64];
    const int s = blockIdx.y, lane = threadIdx.x & 63, grp = threadIdx.x >> 6, bin = blockIdx.x * 64 + lane;
    const uint32_t *cur = hist + (size_t)s * nchunks * 4096 + bin;
    uint32_t ch = 0;
#pragma unroll 4
    for (int k = grp; k < nchunks; k += 8) ch += cur[(size_t)k * 4096];
    part[grp][lane] = ch;
    __syncthreads();
    if (grp == 0) {
        ch = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) ch += part[q][lane];
        double p = 0.0;
        if (ch != 0) {
            p = __ddiv_rn((double)states[first + s].model[bin], (double)ch);  // camshift.js:322-326
            p = p < 1.0 ? p : 1.0;
        }
        const uint32_t v = (uint32_t)floor(__dmul_rn(255.0, p));  // camshift.js:188: binary64 product, then floor (0 .. 255)
        lut_w[(size_t)s * 4096 + bin] = p;
        lut_px[(size_t)s * 4096 + bin] = v * 0x010101u | 0xFF000000u;  // R = G = B = v, A = 255 (camshift.js:189-192)
    }
}

template <int KIND>
struct BpKind;
template <>
struct BpKind<HT_BP_RGBA8> {
    typedef uint32_t elem;  // one RGBA pixel
};
template <>
struct BpKind<HT_BP_F64> {
    typedef double elem;
};

// four consecutive output elements: one 16-byte store (RGBA8) or two (F64).  The base is only aligned to the element size when a packed
// frame's pixel count is not a multiple of 4 — like the 16-byte loads of the input side, legal for global memory on gfx950.
__device__ __forceinline__ void bp_store4(uint32_t *dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    *reinterpret_cast<uint4 *>(dst) = make_uint4(a, b, c, d);
}
__device__ __forceinline__ void bp_store4(double *dst, double a, double b, double c, double d) {
    reinterpret_cast<double2 *>(dst)[0] = make_double2(a, b);
    reinterpret_cast<double2 *>(dst)[1] = make_double2(c, d);
}

// grid (chunks, frames) like the histogram pass: workgroup (k, s) writes pixels [k chunk_px, (k + 1) chunk_px) of frame s.  The frame's LUT
// (16 KB u32 / 32 KB binary64) goes to LDS with one / two 16-byte loads per thread, issued in front of the first batch of pixel loads and
// stored behind it, so the LUT's round trip and the pixels' overlap; one barrier, then nothing but loads, LDS reads and stores.
template <int KIND>
__global__ __launch_bounds__(BP_NT) void k_bp_project(const uint8_t *__restrict__ frames, size_t frame_stride, uint32_t npix, uint32_t chunk_px,
                                                      const typename BpKind<KIND>::elem *__restrict__ lut_g, uint8_t *__restrict__ out, size_t out_stride) {
    typedef typename BpKind<KIND>::elem elem;
    constexpr int LUT_V4 = (int)(4096 * sizeof(elem) / 16 / BP_NT);  // 16-byte pieces of the LUT per thread: 1 (RGBA8) or 2 (F64)
    __shared__ __attribute__((aligned(16))) elem lut[4096];
    const uint8_t *frame = frames + (size_t)blockIdx.y * frame_stride;
    elem *dst = reinterpret_cast<elem *>(out + (size_t)blockIdx.y * out_stride);
    const uint32_t beg = blockIdx.x * chunk_px, end = min(beg + chunk_px, npix);  // chunk_px is a multiple of 4 * BP_NT; beg < npix
    const uint32_t nquad = (end - beg) / 4;
    const uint4 *img4 = reinterpret_cast<const uint4 *>(frame + (size_t)beg * 4);
    const uint32_t iters = chunk_px / (4 * BP_NT);  // >= 1
    const uint4 *lut4 = reinterpret_cast<const uint4 *>(lut_g + (size_t)blockIdx.y * 4096);
    uint4 lv[LUT_V4];
#pragma unroll
    for (int q = 0; q < LUT_V4; q++) lv[q] = lut4[q * BP_NT + threadIdx.x];
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
        if (it0 == 0) {  // workgroup-uniform: the LUT lands in LDS while the first pixels are on their way
#pragma unroll
            for (int q = 0; q < LUT_V4; q++) reinterpret_cast<uint4 *>(lut)[q * BP_NT + threadIdx.x] = lv[q];
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
            const uint4 p = pv[u];
            bp_store4(dst + (size_t)beg + (size_t)i * 4, lut[cs_bin(p.x)], lut[cs_bin(p.y)], lut[cs_bin(p.z)], lut[cs_bin(p.w)]);
        }
    }
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frame);
    for (uint32_t i = beg + nquad * 4 + threadIdx.x; i < end; i += BP_NT) dst[i] = lut[cs_bin(img[i])];  // < 4 pixels
}

size_t bp_elem(int32_t kind) { return kind == HT_BP_F64 ? sizeof(double) : sizeof(uint32_t); }

// the checks both entry points share; *frame_bytes = bytes of one output frame, *stride = the effective output stride
ht_status bp_check(ht_ctx *c, const char *fn, int32_t first, int32_t n, int32_t kind, const void *out, size_t out_stride, size_t *frame_bytes, size_t *stride) {
    if (!c || !out) return HT_ERR_INVALID;
    if (kind != HT_BP_RGBA8 && kind != HT_BP_F64) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": unknown output kind");
    if (!c->d_frames || n <= 0 || n > c->nframes) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": bind n frames first");
    if (first < 0 || first + n > c->cs_streams) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": stream range not reserved");
    *frame_bytes = (size_t)c->W * c->H * bp_elem(kind);
    *stride = out_stride ? out_stride : *frame_bytes;
    if (*stride < *frame_bytes) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": output stride smaller than a frame");
    return HT_OK;
}

// scratch of this unit, grown on demand, for both forms of the call (batch and pairs): the chunk histograms of `frames` frames and
// `luts` LUTs of either kind
ht_status bp_scratch(ht_ctx *c, size_t frames, uint32_t nchunks, size_t luts) {
    ht_status st = ht_grow_device(c, &c->d_bp_hist, &c->bp_hist_cap, frames * nchunks * 4096, "ht_camshift_backproject: hipMalloc failed (chunk histograms)");
    if (st == HT_OK) st = ht_grow_device(c, &c->d_bp_lut_w, &c->bp_lut_w_cap, luts * 4096, "ht_camshift_backproject: hipMalloc failed (weight LUTs)");
    if (st == HT_OK) st = ht_grow_device(c, &c->d_bp_lut_px, &c->bp_lut_px_cap, luts * 4096, "ht_camshift_backproject: hipMalloc failed (pixel LUTs)");
    return st;
}

// the host forms' result on the device (packed), then to the caller with the caller's stride; waits
ht_status bp_staging(ht_ctx *c, size_t bytes) {
    return ht_grow_device(c, &c->d_bp_out, &c->bp_out_cap, bytes, "ht_camshift_backproject: hipMalloc failed (output staging)");
}
ht_status bp_copy_out(ht_ctx *c, void *out_host, size_t stride, size_t frame_bytes, int32_t n) {
    if (stride == frame_bytes) HT_HIP(c, hipMemcpyAsync(out_host, c->d_bp_out, (size_t)n * frame_bytes, hipMemcpyDeviceToHost, c->stream));
    else HT_HIP(c, hipMemcpy2DAsync(out_host, stride, c->d_bp_out, frame_bytes, frame_bytes, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

// the three launches; d_out: device memory, n frames `stride` bytes apart
ht_status bp_enqueue(ht_ctx *c, int32_t first, int32_t n, int32_t kind, void *d_out, size_t stride) {
    const uint32_t npix = (uint32_t)((size_t)c->W * c->H);
    if (npix == 0) return HT_OK;
    uint32_t chunk_px = 0, nchunks = 0;
    ht_cs_hist_plan(npix, n, &chunk_px, &nchunks);
    ht_status st = bp_scratch(c, (size_t)n, nchunks, (size_t)n);
    if (st != HT_OK) return st;
    {
        HtProfScope ps(c, "cs_bp_hist");
        st = ht_cs_hist_launch(c, c->d_frames, c->frame_stride, n, npix, chunk_px, nchunks, c->d_bp_hist);
        if (st != HT_OK) return st;
    }
    {
        HtProfScope ps(c, "cs_bp_lut");
        hipLaunchKernelGGL(k_bp_lut, dim3(64, n), dim3(BP_LUT_NT), 0, c->stream, c->d_bp_hist, (int)nchunks, c->d_cs, first, c->d_bp_lut_w, c->d_bp_lut_px);
        HT_HIP(c, hipGetLastError());
    }
    {
        HtProfScope ps(c, "cs_backproject");
        if (kind == HT_BP_RGBA8)
            hipLaunchKernelGGL(k_bp_project<HT_BP_RGBA8>, dim3(nchunks, n), dim3(BP_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px,
                               c->d_bp_lut_px, static_cast<uint8_t *>(d_out), stride);
        else
            hipLaunchKernelGGL(k_bp_project<HT_BP_F64>, dim3(nchunks, n), dim3(BP_NT), 0, c->stream, c->d_frames, c->frame_stride, npix, chunk_px,
                               c->d_bp_lut_w, static_cast<uint8_t *>(d_out), stride);
        HT_HIP(c, hipGetLastError());
    }
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_backproject_device(ht_ctx *c, int32_t first, int32_t n, int32_t kind, void *out_dev, size_t out_stride) {
    HtRange range("ht_camshift_backproject_device");
    size_t frame_bytes = 0, stride = 0;
    ht_status st = bp_check(c, "ht_camshift_backproject_device", first, n, kind, out_dev, out_stride, &frame_bytes, &stride);
    if (st != HT_OK) return st;
    if (((uintptr_t)out_dev | stride) & (bp_elem(kind) - 1))
        return ht_fail(c, HT_ERR_INVALID, "ht_camshift_backproject_device: output pointer and stride must be multiples of the element size");
    HT_HIP(c, hipSetDevice(c->device));
    return bp_enqueue(c, first, n, kind, out_dev, stride);
}

extern "C" ht_status ht_camshift_backproject(ht_ctx *c, int32_t first, int32_t n, int32_t kind, void *out_host, size_t out_stride) {
    HtRange range("ht_camshift_backproject");
    size_t frame_bytes = 0, stride = 0;
    ht_status st = bp_check(c, "ht_camshift_backproject", first, n, kind, out_host, out_stride, &frame_bytes, &stride);
    if (st != HT_OK) return st;
    if (frame_bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    st = bp_staging(c, (size_t)n * frame_bytes);
    if (st != HT_OK) return st;
    st = bp_enqueue(c, first, n, kind, c->d_bp_out, frame_bytes);  // packed on the device; the caller's stride is applied by the copy
    if (st != HT_OK) return st;
    return bp_copy_out(c, out_host, stride, frame_bytes, n);
}

void ht_backproject_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_bp_hist) (void)hipFree(c->d_bp_hist);
    if (c->d_bp_lut_w) (void)hipFree(c->d_bp_lut_w);
    if (c->d_bp_lut_px) (void)hipFree(c->d_bp_lut_px);
    if (c->d_bp_out) (void)hipFree(c->d_bp_out);
    c->d_bp_hist = nullptr, c->d_bp_lut_px = nullptr, c->d_bp_lut_w = nullptr, c->d_bp_out = nullptr;
    c->bp_hist_cap = c->bp_lut_w_cap = c->bp_lut_px_cap = c->bp_out_cap = 0;
}

// The video -> canvas draw (ht_draw_frames / ht_draw_frames_device, k_draw_frames) is compiled as part of this unit: the library keeps one
// code object besides the three that profiles/traffic.json fingerprints, and tests/test_backproject_cpu.py counts them.
#include "ht_ingest.hip"

// So is the device grouping of a detect batch's raw hits (ht_detect_best_* / ht_group_hits, k_grp_*): the scan object stays as recorded.
#include "ht_group.hip"

// So are the pair forms of the camshift calls (ht_camshift_init_pairs / ht_camshift_track_pairs, k_csp_*): new kernels must not enter the
// fingerprinted camshift object, and the library keeps four code objects.  (ht_cs_pairs.hip ends by including ht_cs_best.hip: the
// record-driven initTracker, ht_camshift_init_best / k_csb_resolve, on this unit's grouping records and the pair unit's init kernels, and
// behind it ht_cs_faces.hip: ht_camshift_init_faces / k_csf_resolve, the same for every grouped face of a frame.)
#include "ht_cs_pairs.hip"

// And the back-projection over pairs (ht_camshift_backproject_pairs / _device, k_bpp_*), behind the pair unit whose plan, table upload and
// histogram kernel it uses.
#include "ht_bp_pairs.hip"

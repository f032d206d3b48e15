// ht_orient_kernels.hip — the device code of the oriented draw (rotated and mirrored feeds; ht_orient_plan.h states the rule).  DEVICE CODE
// ONLY, and not part of libheadtrackr_hip.so: build.py compiles this file alone into a plain gfx950 code object,
// libheadtrackr_hip_orient.hsaco next to the library, which the library's host code (ht_draw_list.hip: or_module) loads with hipModuleLoad on
// the first oriented call.  The library's own four code objects, their kernels and their registers stay what they are (the CPU suite pins
// them), which is why this code is not in one of them.
//
// k_draw_list_oriented / k_draw_list_oriented_turn: grid (tile column, tile row, entry), 256 threads.  A workgroup reads its entry's 128-byte
// descriptor (HtOrientDesc) with scalar loads — blockIdx.z is uniform and the table const __restrict__ —, computes the tile's column and row
// taps with rs_tap in O's coordinates, sends each tap's two coordinates through ht_orient_map ONCE (the permutation is separable: O's x
// names a stored column for even rot and a stored row for odd rot, O's y the other one) and keeps them in LDS.  Behind the barrier a pixel
// fetches its four tap pixels from the stored planes — YUV taps converted by ht_yuv_to_rgba first —, blends them with the declared binary64
// sequence (or_channel: ig_channel of ht_ingest.hip under another name, the CPU suite holds the two bodies equal as text), never
// contracted, rounds half to even and is stored as one dword.  All five formats, all eight orientations, behind a workgroup-uniform switch.
//
//   k_draw_list_oriented        tile 64 x 16, lanes along O's x, four rows per thread: loads and stores row-contiguous for even rot; for odd rot
//                               neighbouring lanes read a stored pitch apart
//   k_draw_list_oriented_turn   tile 32 x 32, lanes along O's y — the STORED row for odd rot —, four columns per thread; the tile is turned
//                               through LDS (32 rows of 33 dwords: a wavefront's half writes 32 consecutive banks and reads a stride of 33,
//                               both conflict-free), so loads and stores are both row-contiguous
//
// DESIGN.md §2.3.9 has the registers, the LDS and the measurement that chose between them.
#include <type_traits>

#include "ht_orient_plan.h"
#include "ht_resample_tap.h"
#include "ht_yuv_plan.h"

namespace {

constexpr int OR_NT = 256;

// plane pointers out of the table are GLOBAL addresses (device pointers by contract): the kernel's view of the table says so in the member
// type, and every read below stays a global_load
typedef const __attribute__((address_space(1))) uint8_t *or_gptr;
typedef const __attribute__((address_space(1))) uint16_t *or_g16;
typedef const __attribute__((address_space(1))) uint32_t *or_g32;
typedef HtOrientDescT<or_gptr> OrDesc;
static_assert(sizeof(OrDesc) == sizeof(HtOrientDesc) && alignof(OrDesc) == alignof(HtOrientDesc), "the kernel's view of a descriptor is the host's");

// one channel of one pixel: the declared sequence (rs_pixels4, ht_pyramid.hip), values within [0, 255]
__device__ __forceinline__ uint32_t or_channel(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int sh, double cu, double ct, double ru, double rt) {
    const double s00 = (double)((p00 >> sh) & 0xffu), s01 = (double)((p01 >> sh) & 0xffu);
    const double s10 = (double)((p10 >> sh) & 0xffu), s11 = (double)((p11 >> sh) & 0xffu);
    const double top = __dadd_rn(__dmul_rn(s00, cu), __dmul_rn(s01, ct));
    const double bot = __dadd_rn(__dmul_rn(s10, cu), __dmul_rn(s11, ct));
    const double vv = __dadd_rn(__dmul_rn(top, ru), __dmul_rn(bot, rt));
    return (uint32_t)(int)__builtin_rint(vv) << sh;  // Uint8ClampedArray: round half to even
}

struct OrPlanes {
    or_gptr p0, p1, p2;
    size_t pitch0, pitch1;
    HtYuvCoef kc;
};

// stored pixel (u, v) as the RGBA8 dword the draw kernels blend: the format's read, then the declared conversion
template <int FMT>
__device__ __forceinline__ uint32_t or_fetch(const OrPlanes &s, int u, int v) {
    if (FMT == HT_DRAW_RGBA) return *reinterpret_cast<or_g32>(s.p0 + (size_t)v * s.pitch0 + (size_t)u * 4);
    if (ht_yuv_is_422(FMT)) {  // the macropixel of stored row v as a dword, low byte first: YUYV Y0 U Y1 V, UYVY U Y0 V Y1
        const uint32_t m = *reinterpret_cast<or_g32>(s.p0 + (size_t)v * s.pitch0 + (size_t)(u >> 1) * 4);
        const int ush = FMT == HT_YUV_FMT_UYVY ? 0 : 8;
        return ht_yuv_to_rgba((m >> (8 - ush + 16 * (u & 1))) & 0xffu, (m >> ush) & 0xffu, (m >> ush >> 16) & 0xffu, s.kc);
    }
    const uint32_t y = s.p0[(size_t)v * s.pitch0 + (size_t)u];
    const size_t crow = (size_t)(v >> 1) * s.pitch1;
    if (FMT == HT_YUV_FMT_NV12) {  // the chroma base and pitch are even: an aligned U V pair
        const uint32_t uv = *reinterpret_cast<or_g16>(s.p1 + crow + 2 * (size_t)(u >> 1));
        return ht_yuv_to_rgba(y, uv & 0xffu, uv >> 8, s.kc);
    }
    return ht_yuv_to_rgba(y, s.p1[crow + (size_t)(u >> 1)], s.p2[crow + (size_t)(u >> 1)], s.kc);
}

// the tile's pixels of one thread.  TURN false: column f, rows s + 4 j; TURN true: row f, columns s + 8 j, through s_turn
template <bool TURN, int FMT>
__device__ __forceinline__ void or_pixels(const OrPlanes &pl, bool odd, const RsTap *s_col, const RsTap *s_row, uint32_t *s_turn, uint32_t *out, int X0, int Y0, int dw, int dh) {
    constexpr int FW = TURN ? 32 : 64, STEP = OR_NT / FW;
    const int f = threadIdx.x & (FW - 1), s = threadIdx.x / FW;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int xl = TURN ? s + STEP * j : f, yl = TURN ? f : s + STEP * j;
        if (X0 + xl >= dw || Y0 + yl >= dh) continue;
        const RsTap cx = s_col[xl], ry = s_row[yl];  // a, b: already stored coordinates (the column's for even rot, the row's for odd rot)
        uint32_t p00, p01, p10, p11;
        if (odd) p00 = or_fetch<FMT>(pl, ry.a, cx.a), p01 = or_fetch<FMT>(pl, ry.a, cx.b), p10 = or_fetch<FMT>(pl, ry.b, cx.a), p11 = or_fetch<FMT>(pl, ry.b, cx.b);
        else p00 = or_fetch<FMT>(pl, cx.a, ry.a), p01 = or_fetch<FMT>(pl, cx.b, ry.a), p10 = or_fetch<FMT>(pl, cx.a, ry.b), p11 = or_fetch<FMT>(pl, cx.b, ry.b);
        uint32_t o = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) o |= or_channel(p00, p01, p10, p11, 8 * ch, cx.u, cx.t, ry.u, ry.t);
        if (TURN) s_turn[xl * 33 + yl] = o;
        else out[(size_t)(Y0 + yl) * dw + X0 + xl] = o;
    }
}

template <bool TURN>
__device__ __forceinline__ void or_draw(const OrDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh, RsTap *s_col, RsTap *s_row, uint32_t *s_turn) {
    constexpr int TW = TURN ? 32 : 64, TH = TURN ? 32 : 16;
    const OrDesc &e = tab[blockIdx.z];  // uniform index into a read-only table: scalar loads
    const int k = e.orient & 7, w = e.d.sw, h = e.d.sh, format = e.d.format;
    const bool odd = k & 1;
    const int X0 = blockIdx.x * TW, Y0 = blockIdx.y * TH;
    if (threadIdx.x < TW + TH) {
        const bool col = threadIdx.x < TW;
        const int i = col ? threadIdx.x : threadIdx.x - TW;
        // the tap in O's coordinates, then its two coordinates through the mapping: a column tap keeps what O's x decides (u for even rot, v
        // for odd rot), a row tap what O's y decides
        RsTap tp = col ? rs_tap(min(X0 + i, dw - 1), e.d.rx, e.orw, e.ox) : rs_tap(min(Y0 + i, dh - 1), e.d.ry, e.orh, e.oy);
        int32_t ua, va, ub, vb;
        ht_orient_map(k, w, h, col ? tp.a : 0, col ? 0 : tp.a, &ua, &va);
        ht_orient_map(k, w, h, col ? tp.b : 0, col ? 0 : tp.b, &ub, &vb);
        tp.a = (col != odd) ? ua : va, tp.b = (col != odd) ? ub : vb;
        (col ? s_col : s_row)[i] = tp;
    }
    __syncthreads();
    OrPlanes pl;
    pl.p0 = e.d.p0, pl.p1 = e.d.p1, pl.p2 = e.d.p2, pl.pitch0 = e.d.pitch0, pl.pitch1 = e.d.pitch1, pl.kc = e.d.kc;
    uint32_t *out = reinterpret_cast<uint32_t *>(dst + (size_t)e.frame * dst_stride);
    switch (format) {  // workgroup-uniform
        case HT_DRAW_RGBA: or_pixels<TURN, HT_DRAW_RGBA>(pl, odd, s_col, s_row, s_turn, out, X0, Y0, dw, dh); break;
        case HT_YUV_FMT_NV12: or_pixels<TURN, HT_YUV_FMT_NV12>(pl, odd, s_col, s_row, s_turn, out, X0, Y0, dw, dh); break;
        case HT_YUV_FMT_I420: or_pixels<TURN, HT_YUV_FMT_I420>(pl, odd, s_col, s_row, s_turn, out, X0, Y0, dw, dh); break;
        case HT_YUV_FMT_YUYV: or_pixels<TURN, HT_YUV_FMT_YUYV>(pl, odd, s_col, s_row, s_turn, out, X0, Y0, dw, dh); break;
        case HT_YUV_FMT_UYVY: or_pixels<TURN, HT_YUV_FMT_UYVY>(pl, odd, s_col, s_row, s_turn, out, X0, Y0, dw, dh); break;
        default: break;  // (the plan admits no other number)
    }
    if (TURN) {  // the tile out of LDS with lanes along O's x: a wavefront's half stores 128 contiguous bytes of a destination row
        __syncthreads();
        const int xl = threadIdx.x & 31, s = threadIdx.x >> 5;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int yl = s + 8 * j;
            if (X0 + xl < dw && Y0 + yl < dh) out[(size_t)(Y0 + yl) * dw + X0 + xl] = s_turn[xl * 33 + yl];
        }
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(OR_NT) void k_draw_list_oriented(const OrDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    __shared__ RsTap s_col[64], s_row[16];
    or_draw<false>(tab, dst, dst_stride, dw, dh, s_col, s_row, nullptr);
}

extern "C" __global__ __launch_bounds__(OR_NT) void k_draw_list_oriented_turn(const OrDesc *__restrict__ tab, uint8_t *__restrict__ dst, size_t dst_stride, int dw, int dh) {
    __shared__ RsTap s_col[32], s_row[32];
    __shared__ uint32_t s_turn[32 * 33];
    or_draw<true>(tab, dst, dst_stride, dw, dh, s_col, s_row, s_turn);
}

// ht_cs_device.h — device helpers of the camshift kernels: the histogram bin (cs_bin), the workgroup sizes, the load-laundering macro, the
// wave-merged histogram update, the window moments, the mean-shift loop and the cluster exchange (cluster_moments, ClusterSync).  Included ONCE per translation unit, INSIDE the unit's
// anonymous namespace, ahead of its kernels: by ht_camshift.hip, and by ht_backproject.hip for its own kernels and for ht_cs_pairs.hip,
// which it compiles.  Every helper has this one definition (tests/test_pairs_cpu.py counts them).  A change here changes the camshift
// code object that profiles/traffic.json is tied to.

// camshift.js:63-66 (px = R | G<<8 | B<<16 | A<<24): bin = (R>>4)<<8 | (G>>4)<<4 | (B>>4).  Four instructions instead of the eight of
// the field-by-field form (the histogram pass of k_cs_track_fused spent 32 of its ~50 vector instructions per 16-byte load on its four
// bins): with t = px & 0xf0f0f0 = r<<4 | g<<12 | b<<20 (r, g, b the 4-bit fields), t + (t << 12) puts g at bit 24 next to b at bit 20
// (all fields of the sum are disjoint: no carries; b << 32 leaves the register), t << 24 puts r at bit 28, and the bin is bits 20-31.
// tests/test_oracle_golden.py proves the expression against the reference formula on every RGB value.
__device__ __forceinline__ uint32_t cs_bin(uint32_t px) {
    const uint32_t t = px & 0x00f0f0f0u;
    return ((t << 24) | (t + (t << 12))) >> 20;  // v_and, v_mul_u32_u24 0x1001, v_lshl_or_b32, v_lshrrev
}

#ifdef HT_CS_TIMELINE  // measurement build (tools/gpu_cs_timeline.py): shader-clock stamps of a workgroup's phases
#define CS_STAMP(arr, i)                                                      \
    do {                                                                      \
        __builtin_amdgcn_sched_barrier(0);                                    \
        if ((arr) && threadIdx.x == 0 && (i) < 30) (arr)[(i)] = __builtin_readcyclecounter(); \
        __builtin_amdgcn_sched_barrier(0);                                    \
    } while (0)
#else
#define CS_STAMP(arr, i)
#endif

// (the workgroup sizes CS_NT / HIST_NT / INIT_NT and CS_REGION_CAP: ht_cs_schedule.h, where the host plans its launches with them)
constexpr int HIST_UNROLL = 4;  // 16-byte loads of a thread in flight in the histogram pass (k_cs_hist)

// A batch of PREDICATED loads (`v = ok ? p[i] : 0`) followed by cs_bin: the optimiser folds the bin's first instruction (`& 0xf0f0f0`, which maps
// the 0 of the not-taken side to 0) into the load's own block, where it has to wait for the load on the spot — every load of the batch
// then costs its own round trip (k_cs_hist 16.4 -> 20 us at 8 x 1080p, seen in the code object: `s_waitcnt vmcnt(0)` behind every load).
// Laundering the loaded registers AFTER the whole batch keeps the consumers behind all of its loads.
#define CS_BATCH_LOADED(v_) asm volatile("" : "+v"(v_))

__device__ __forceinline__ int32_t toint32(double v) {  // ECMAScript ToInt32 (>>0, <<2)
    if (!(fabs(v) < 1.0e300)) return 0;                  // NaN, +-Infinity
    const double t = trunc(v);
    if (fabs(t) < 2147483648.0) return (int32_t)t;
    double m = fmod(t, 4294967296.0);
    if (m < 0) m += 4294967296.0;
    return (int32_t)(uint32_t)m;
}

// wave-merged LDS histogram update (see k_cs_hist in ht_cs_kernels.inc): the counts of all lanes that share the first active lane's bin
// go out as one atomic.  Counts are integers: any order gives the same histogram.
__device__ __forceinline__ void hist_add_wave(uint32_t *h, uint32_t bin, uint32_t count, bool active) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const uint32_t lead_lane = (uint32_t)__builtin_ctzll(act);
    const uint32_t lead_bin = (uint32_t)__builtin_amdgcn_readlane((int)bin, (int)lead_lane);
    const uint32_t lead_cnt = (uint32_t)__builtin_amdgcn_readlane((int)count, (int)lead_lane);
    const bool same = active && bin == lead_bin && count == lead_cnt;
    const unsigned long long m = __ballot(same);
    if ((threadIdx.x & 63u) == lead_lane) atomicAdd(&h[lead_bin], lead_cnt * (uint32_t)__popcll(m));
    if (active && !same) atomicAdd(&h[bin], count);
}

struct Mom {
    double m00, m10, m01, m11, m20, m02;
};

// binary64 wave sum with DPP row shifts / row broadcasts: a fixed tree (deterministic), VALU only.  The __shfl_xor tree it
// replaces is 6 dependent ds_bpermute round trips per value and half — 36 to 72 LDS round trips per moment pass, which was most
// of a pass's latency on the small windows of C3.  Lanes a shift does not reach read 0 (bound_ctrl) and add +0.0.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, BANK_MASK, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, BANK_MASK, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    double s = v + dpp_f64<0x111, 0xf, 0xf>(v);  // row_shr:1
    s += dpp_f64<0x112, 0xf, 0xf>(v);            // row_shr:2
    s += dpp_f64<0x113, 0xf, 0xf>(v);            // row_shr:3
    s += dpp_f64<0x114, 0xf, 0xe>(s);            // row_shr:4, banks 1-3
    s += dpp_f64<0x118, 0xf, 0xc>(s);            // row_shr:8, banks 2-3
    s += dpp_f64<0x142, 0xa, 0xf>(s);            // row_bcast:15 into rows 1, 3
    s += dpp_f64<0x143, 0xc, 0xf>(s);            // row_bcast:31 into rows 2, 3
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(s), 63), __builtin_amdgcn_readlane(__double2loint(s), 63));
}

// camshift.Moments (camshift.js:79-120) over columns [x, w) x rows [y, h) — w, h are the right / bottom EDGES.
// Mapping: lanes along a row (coalesced RGBA reads), wavefront wv takes rows wv, wv + NW, ...; a row's y factor leaves the pixel
// loop:  rs = sum val, ts = sum vx*val (us = sum vx^2*val) per row, then m00 += rs, m10 += ts, m01 += vy*rs (m11 += vy*ts,
// m20 += us, m02 += vy^2*rs) — 2 adds + 1 multiply per pixel for the first moments and no integer division.  Same real-number
// sums as the reference's column-major loop, different rounding order (see header).
//
// The pixels of a pass come either from global memory or — REG — from a copy of the neighbourhood of the search window that the
// workgroup made in LDS (12-bit histogram bin per pixel, CsRegion): measured on C3, a pass over a 90 x 90 window cost 7-10 us
// when its loads went out to memory (every CU streams its frame for the histogram at the same time, 4 frame versions do not
// fit the 256 MB Infinity Cache), although it is two rounds of independent loads; from LDS it is a fraction of a microsecond.
struct CsRegion {
    const uint16_t *bins;  // [rh][rw] bins, LDS
    int x0, y0, rw, rh;    // rw == 0: no region cached
};

// NW = wavefronts the rows are dealt out to, PW = wavefronts the workgroup really has (NW % PW == 0): with PW < NW a wavefront plays
// NW / PW of them in turn (rows, partial sums, wave sums and their slots of red[] are those of the NW-wavefront workgroup), so a
// 512-thread workgroup adds exactly what a 1024-thread one adds, in the same order — k_cs_track_fused<.., 512> below.
template <bool SECOND, int NW, bool REG, int PW = NW>
__device__ __forceinline__ Mom window_moments(const uint32_t *__restrict__ img, int W, const double *lut, const CsRegion &R, int x, int y, int w, int h,
                                              double (*red)[NW], unsigned long long *fine = nullptr) {
    Mom m = {0, 0, 0, 0, 0, 0};
    CS_STAMP(fine, 0);
    const int ww = w - x, hh = h - y;
    const int lane = threadIdx.x & 63;
    constexpr int VPP = NW / PW;
    static_assert(NW % PW == 0, "virtual wavefronts per physical one");
    double vs[VPP > 1 ? VPP - 1 : 1][6];  // wave sums of the wavefronts already played (wave-uniform)
#pragma unroll
    for (int vi = 0; vi < VPP; vi++) {
    const int wave = (int)(threadIdx.x >> 6) + vi * PW;
    m = Mom{0, 0, 0, 0, 0, 0};
    // Shader-clock stamps (HT_CS_TIMELINE) of a pass over an 83 x 83 window: pixel loop 9.3 k cycles, wave sums 0.8 k, final sums
    // 1.4 k, scalar mean-shift logic 0.45 k — the pixel loop was a chain of dependent round trips (bin -> LUT -> add), made
    // sequential by per-row early exits that kept the compiler from batching the loads.  So: every load of a batch of 8 rows is
    // unconditional (clamped address, value masked) and issued before the first use, and only as many wavefronts take part as
    // there are 8-row batches (at least 4 = one per SIMD); the others wait at the barriers with zero partial sums.
    const int nwa = min(NW, max(4, (hh + 7) >> 3));
    if (ww > 0 && hh > 0 && wave < nwa) {
        for (int j0 = wave; j0 < hh; j0 += 8 * nwa) {
            // per row: rs = sum val, ts = sum vx val (both are needed again times the row's y); the x^2 sum has no y factor and
            // goes straight into m20 (one accumulator instead of eight: the kernel sits at the 128-VGPR cap of a 1024-thread workgroup)
            double rs[8], ts[8];
#pragma unroll
            for (int r = 0; r < 8; r++) rs[r] = ts[r] = 0.0;
            for (int cb = 0; cb < ww; cb += 64) {  // cb: wave-uniform chunk base
                const int c = cb + lane, cc = min(c, ww - 1);
                uint32_t px[8];
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const int j = min(j0 + r * nwa, hh - 1);  // clamped address, value masked below
                    if (REG) px[r] = R.bins[(y + j - R.y0) * R.rw + (x + cc - R.x0)];
                    else px[r] = img[(size_t)(y + j) * W + (x + cc)];
                }
                if (!REG) {
                    // the eight loads are issued before the first bin is computed.  Left to the scheduler, one build of the 512-thread
                    // kernel (128-VGPR cap) fetched them one at a time into ONE register — eight dependent round trips per 64 columns on
                    // the path that streams with windows beyond the LDS region take: +9 % on the whole launch
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int r = 0; r < 8; r++) px[r] = cs_bin(px[r]);
                }
                double val[8];
#pragma unroll
                for (int r = 0; r < 8; r++) val[r] = lut[px[r]];
                const double vx = (double)c;
                const bool colok = c < ww;
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const double vv = (colok && j0 + r * nwa < hh) ? val[r] : 0.0;
                    rs[r] += vv;
                    ts[r] += vx * vv;
                    if (SECOND) m.m20 += vx * vx * vv;
                }
            }
#pragma unroll
            for (int r = 0; r < 8; r++) {
                const double vy = (double)(j0 + r * nwa);  // rows past the window have rs = ts = us = 0
                m.m00 += rs[r];
                m.m10 += ts[r];
                m.m01 += vy * rs[r];
                if (SECOND) {
                    m.m11 += vy * ts[r];
                    m.m02 += vy * vy * rs[r];
                }
            }
        }
    }
    if (vi + 1 < VPP) {  // not the last wavefront this one plays: its wave sums wait (scalar registers) for the barrier below
        const double vq[6] = {m.m00, m.m10, m.m01, m.m11, m.m20, m.m02};
#pragma unroll
        for (int k = 0; k < (SECOND ? 6 : 3); k++) vs[vi][k] = wave < nwa ? wave_sum_f64(vq[k]) : 0.0;
    }
    }  // vi
    const int wave = (int)(threadIdx.x >> 6) + (VPP - 1) * PW;
    const int nwa = min(NW, max(4, (hh + 7) >> 3));
    double v[6] = {m.m00, m.m10, m.m01, m.m11, m.m20, m.m02};
    constexpr int nv = SECOND ? 6 : 3;
    CS_STAMP(fine, 1);
    __syncthreads();  // red[] may still be read from the previous call
    CS_STAMP(fine, 2);
#pragma unroll
    for (int k = 0; k < nv; k++) {
        const double s = wave < nwa ? wave_sum_f64(v[k]) : 0.0;  // wave-uniform branch; idle waves contribute an exact 0
        if (lane == 0) red[k][wave] = s;
#pragma unroll
        for (int vi = 0; vi + 1 < VPP; vi++)
            if (lane == 0) red[k][(int)(threadIdx.x >> 6) + vi * PW] = vs[vi][k];
    }
    CS_STAMP(fine, 3);
    __syncthreads();
    CS_STAMP(fine, 4);
    // the workgroup's sums: lane k of EVERY wavefront adds the NW wave sums of moment k in the fixed order q = 0 .. NW-1 (the same
    // bits in every wavefront) and the results are broadcast as wave-uniform scalars.  (Every lane used to add all 6 x NW values
    // itself: 96 binary64 adds per thread — a quarter of a pass's VALU time, and 192 VGPRs of loads in flight that spilled.)
    {
        double sacc = 0.0;
        if (lane < nv) {
#pragma unroll
            for (int q = 0; q < NW; q++) sacc += red[lane][q];
        }
#pragma unroll
        for (int k = 0; k < nv; k++)
            v[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), k), __builtin_amdgcn_readlane(__double2loint(sacc), k));
    }
    CS_STAMP(fine, 5);
    m.m00 = v[0], m.m10 = v[1], m.m01 = v[2], m.m11 = v[3], m.m20 = v[4], m.m02 = v[5];
    return m;
}

template <bool SECOND, int NW, int PW = NW>
__device__ __forceinline__ Mom window_moments_any(const uint32_t *__restrict__ img, int W, const double *lut, const CsRegion &R, int x, int y, int w, int h,
                                                  double (*red)[NW], unsigned long long *fine = nullptr) {
    // workgroup-uniform: the whole window lies inside the cached region (it practically always does: the region is the search
    // window plus a margin, and a mean-shift step moves the window by a few pixels)
    if (R.rw > 0 && x >= R.x0 && y >= R.y0 && w <= R.x0 + R.rw && h <= R.y0 + R.rh) return window_moments<SECOND, NW, true, PW>(img, W, lut, R, x, y, w, h, red, fine);
    return window_moments<SECOND, NW, false, PW>(img, W, lut, R, x, y, w, h, red, fine);
}

// Copies the neighbourhood of the search window (the window clamped to the frame, grown by as large a margin as `cap` pixels
// allow, at most 16) into LDS as histogram bins.  All loads are independent: one round of memory latency for the whole region.
// workgroup-uniform integers (search window, region rectangle, loop bounds) are pinned to scalar registers: every thread computes the
// same values, but the compiler cannot know that of something read from LDS and would keep them — and the whole integer side of the
// mean-shift loop — in VGPRs, of which this 1024-thread kernel has exactly 128
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ CsRegion cs_region_rect(int W, int H, const int *s_sw, uint16_t *bins, int cap) {
    CsRegion R = {bins, 0, 0, 0, 0};
    const int sw0 = uni(s_sw[0]), sw1 = uni(s_sw[1]), sw2 = uni(s_sw[2]), sw3 = uni(s_sw[3]);
    const int x0 = max(sw0, 0), y0 = max(sw1, 0), x1 = min(x0 + sw2, W), y1 = min(y0 + sw3, H);
    const int w0 = x1 - x0, h0 = y1 - y0;
    if (w0 <= 0 || h0 <= 0 || (long long)w0 * h0 > cap) return R;
    int mg = 0;
    for (int t = 16; t > 0; t >>= 1)  // largest margin <= 16 px that still fits: a mean-shift step moves the window by a few pixels
        if ((long long)(min(x1 + mg + t, W) - max(x0 - mg - t, 0)) * (min(y1 + mg + t, H) - max(y0 - mg - t, 0)) <= cap && mg + t <= 16) mg += t;
    R.x0 = max(x0 - mg, 0), R.y0 = max(y0 - mg, 0);
    R.rw = min(x1 + mg, W) - R.x0, R.rh = min(y1 + mg, H) - R.y0;
    return R;
}

template <int NT_>
__device__ __forceinline__ CsRegion cs_cache_region(const uint32_t *__restrict__ img, int W, int H, const int *s_sw, uint16_t *bins, int cap) {
    const CsRegion R = cs_region_rect(W, H, s_sw, bins, cap);
    if (R.rw == 0) return R;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NWV = NT_ / 64;
    for (int j0 = wave; j0 < R.rh; j0 += 8 * NWV) {  // rows by wavefront, columns by lane: no division, 8 independent loads per batch
        for (int cb = 0; cb < R.rw; cb += 64) {
            const int c = min(cb + lane, R.rw - 1);
            uint32_t px[8];
#pragma unroll
            for (int r = 0; r < 8; r++) px[r] = img[(size_t)(R.y0 + min(j0 + r * NWV, R.rh - 1)) * W + (R.x0 + c)];
#pragma unroll
            for (int r = 0; r < 8; r++)
                if (cb + lane < R.rw && j0 + r * NWV < R.rh) bins[(j0 + r * NWV) * R.rw + cb + lane] = (uint16_t)cs_bin(px[r]);
        }
    }
    return R;  // the caller synchronises the workgroup before the first pass
}

// meanShift + camShift (camshift.js:222-312) once the weight LUT is in LDS; every thread runs the identical scalar logic,
// thread 0 writes the state.  NW = wavefronts of the workgroup.
// `moments(x, y, w, h)` computes camshift.Moments (all six sums) over the window for the whole workgroup (every thread gets the same Mom).
template <typename MOMENTS>
__device__ __forceinline__ void meanshift_body(int W, int H, const int *s_sw, HtCsState &st, int calc_angles, int max_it, ht_cs_trackobj *__restrict__ out_s,
                                               unsigned long long *stamps, bool writer, MOMENTS moments, uint32_t *done_flag = nullptr, uint32_t done_seq = 0u) {
    int swx = uni(s_sw[0]), swy = uni(s_sw[1]);
    int n_stamp = 4;
    (void)n_stamp;
    const int sww = uni(s_sw[2]), swh = uni(s_sw[3]);
    int prevx = swx, prevy = swy;  // camshift.js:280-281
    Mom m = {0, 0, 0, 0, 0, 0};
    int wadx = 0, wady = 0, wadw = 0, wadh = 0;
    unsigned long long visited = 0;  // window pixels read by the moment passes (B_track = 4*W*H + 4*sum(window))
    for (int it = 0; it < max_it; it++) {  // camshift.js:284-306; max_it = 10 (option cs_iters: measurement knob, wrong results)
        wadx = max(swx, 0);
        wady = max(swy, 0);
        wadw = min(wadx + sww, W);
        wadh = min(wady + swh, H);
        visited += (unsigned long long)max(wadw - wadx, 0) * (unsigned long long)max(wadh - wady, 0);
        // Every pass computes all six sums.  The reference computes the second moments only in its 10th iteration or, once the
        // window stopped moving, in ONE MORE pass over the same window (camshift.js:299-301) — whose first-moment sums are, operation
        // for operation, the ones this pass already has: the extra pass (a quarter of a typical call's passes) is not run.
        m = moments(wadx, wady, wadw, wadh);
        CS_STAMP(stamps, n_stamp);
        n_stamp++;
        if (it == 0) CS_STAMP(stamps, 22);
        const double inv = 1.0 / m.m00, xc = m.m10 * inv, yc = m.m01 * inv;  // camshift.js:109-111
        swx += uni(toint32(xc - (double)sww / 2));                               // camshift.js:295 (every thread holds the same sums)
        swy += uni(toint32(yc - (double)swh / 2));                               // camshift.js:296
        if (it == 0) CS_STAMP(stamps, 23);
        if (swx == prevx && swy == prevy) {                                      // camshift.js:299-301
            // `visited` keeps counting the reference's passes (B_track = 4 W H + 4 sum of the window passes)
            if (it != 9) visited += (unsigned long long)max(wadw - wadx, 0) * (unsigned long long)max(wadh - wady, 0);
            break;
        }
        prevx = swx;
        prevy = swy;
    }
    CS_STAMP(stamps, n_stamp);
    if (threadIdx.x != 0 || !writer) return;
    swx = max(0, min(swx, W));  // camshift.js:308-309
    swy = max(0, min(swy, H));
    const double invM00 = 1.0 / m.m00, xc = m.m10 * invM00, yc = m.m01 * invM00;
    const double mu20 = m.m20 - m.m10 * xc, mu02 = m.m02 - m.m01 * yc, mu11 = m.m11 - m.m01 * xc;  // camshift.js:116-118
    const double a = mu20 * invM00, c = mu02 * invM00;  // camshift.js:230-231
    double width, height, angle;
    if (calc_angles) {  // camshift.js:233-245
        const double b = mu11 * invM00, d = a + c;
        const double e = sqrt((4 * b * b) + ((a - c) * (a - c)));
        width = (double)(int32_t)((uint32_t)toint32(sqrt((d - e) * 0.5)) << 2);
        height = (double)(int32_t)((uint32_t)toint32(sqrt((d + e) * 0.5)) << 2);
        angle = atan2(2 * b, a - c + e);
        if (angle < 0) angle = angle + 3.141592653589793;
    } else {  // camshift.js:247-249
        width = (double)(int32_t)((uint32_t)toint32(sqrt(a)) << 2);
        height = (double)(int32_t)((uint32_t)toint32(sqrt(c)) << 2);
        angle = 3.141592653589793 / 2;
    }
    double cx = (double)swx + (double)sww / 2, cy = (double)swy + (double)swh / 2;  // camshift.js:253-254 (old window size)
    cx = cx < (double)W ? cx : (double)W;
    cy = cy < (double)H ? cy : (double)H;
    const double tx = floor(cx > 0 ? cx : 0.0), ty = floor(cy > 0 ? cy : 0.0);
    const int nsww = (int)floor(1.1 * width), nswh = (int)floor(1.1 * height);  // camshift.js:257-258
    st.sw[0] = swx, st.sw[1] = swy, st.sw[2] = nsww, st.sw[3] = nswh;
    st.x = tx, st.y = ty, st.width = width, st.height = height, st.angle = angle;
    st.win_px += visited;
    st.calls += 1;
    if (out_s) {
        ht_cs_trackobj o;
        o.x = tx, o.y = ty, o.width = width, o.height = height, o.angle = angle;
        o.sw_x = swx, o.sw_y = swy, o.sw_width = nsww, o.sw_height = nswh;
        *out_s = o;
    }
    if (done_flag) {  // enqueue-only call: the host polls this word of the pinned slot instead of waiting for an event
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope: the track object above is visible before the flag
        __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- the cluster mean-shift (k_cs_meanshift_cluster / k_csp_meanshift_cluster in ht_cs_kernels.inc): G workgroups share every moment pass ----
// "not written yet" mark of an exchange entry: a NaN no moment sum can be (the sums are finite and >= 0)
constexpr unsigned long long CL_UNWRITTEN = 0xFFF8C0DEC0DE0001ull;


// The wait is a spin on agent-scope loads, so it is BOUNDED: a thread that has waited `budget` shader-clock cycles (a quarter of a
// second by default, against ~1-2 us for a healthy exchange) raises the context's error word and its workgroup stops waiting — at this
// and every later exchange of the call (s_timeout is sticky).  The host reports HT_ERR_STATE with the next result read-back; the stream's
// state is then garbage for this call, but nothing hangs.  Co-residency (the premise of the spin) is arranged by the host: one cluster
// launch in flight per device and process, grid <= one workgroup per CU (launch_track).
// Ordering: an entry is ONE 8-byte word, written by an sc1 (agent-scope) store and read by sc1 loads — single-copy atomic, nothing else
// depends on it.  That is the gfx9 memory model; ht_create refuses any other arch.
struct ClusterSync {
    uint32_t *err;
    uint32_t *err_host;  // pinned host word (plain system-scope store of 1): an enqueue-only call's host side reads it without a copy
    long long budget;
    int *s_timeout;  // LDS flag of the workgroup
};
template <bool SECOND>
__device__ __forceinline__ Mom cluster_moments(const uint32_t *__restrict__ img, int W, const double *lut, int x, int y, int w, int h, double (*red)[CL_NT / 64],
                                               double *s_part, int g, int G, double *__restrict__ parts, const ClusterSync &sync, int slot) {
    constexpr int NW = CL_NT / 64, nv = SECOND ? 6 : 3;
    Mom m = {0, 0, 0, 0, 0, 0};
    const int ww = w - x, hh = h - y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (ww > 0 && hh > 0) {
        for (int j = g * NW + wave; j < hh; j += G * NW) {  // a row per (workgroup, wavefront); 8 column chunks of the row in flight
            double rs = 0.0, ts = 0.0, us = 0.0;
            const uint32_t *rowp = img + (size_t)(y + j) * W + x;
            for (int cb = 0; cb < ww; cb += 512) {
                uint32_t px[8];
#pragma unroll
                for (int u = 0; u < 8; u++) px[u] = rowp[min(cb + 64 * u + lane, ww - 1)];  // clamped address, value masked below
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int c = cb + 64 * u + lane;
                    const double val = c < ww ? lut[cs_bin(px[u])] : 0.0;
                    const double vx = (double)c;
                    rs += val;
                    ts += vx * val;
                    if (SECOND) us += vx * vx * val;
                }
            }
            const double vy = (double)j;
            m.m00 += rs;
            m.m10 += ts;
            m.m01 += vy * rs;
            if (SECOND) {
                m.m11 += vy * ts;
                m.m20 += us;
                m.m02 += vy * vy * rs;
            }
        }
    }
    double v[6] = {m.m00, m.m10, m.m01, m.m11, m.m20, m.m02};
    __syncthreads();  // red[] / s_part[] may still be read from the previous pass
#pragma unroll
    for (int k = 0; k < nv; k++) {
        const double sum = wave_sum_f64(v[k]);
        if (lane == 0) red[k][wave] = sum;
    }
    __syncthreads();
    // this workgroup's partial sums -> its entries of the pass's exchange slot (agent-scope stores, fire and forget); then every entry
    // of the slot is polled by a thread of its own until it no longer holds the "not written yet" mark k_cs_lut left there: the value
    // that ends the wait IS the partial sum — no arrival counter, no drain of the stores, no second read (a pass used to be
    // store -> s_waitcnt -> atomic add -> poll the counter -> read the G partials: three dependent round trips through L2).
    unsigned long long *slot_parts = reinterpret_cast<unsigned long long *>(parts) + (size_t)slot * CL_MAXG * 6;
    if (threadIdx.x < nv) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < NW; q++) sum += red[threadIdx.x][q];
        __hip_atomic_store(&slot_parts[g * 6 + threadIdx.x], (unsigned long long)__double_as_longlong(sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if ((int)threadIdx.x < G * 6) {
        unsigned long long bits = 0ull;  // +0.0 for the entries a first-moment pass does not use
        if ((int)(threadIdx.x % 6u) < nv) {
            bits = __hip_atomic_load(&slot_parts[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (bits == CL_UNWRITTEN && !*sync.s_timeout) {
                const long long t0 = (long long)__builtin_readcyclecounter();
                for (;;) {
                    __builtin_amdgcn_s_sleep(1);
                    bits = __hip_atomic_load(&slot_parts[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (bits != CL_UNWRITTEN) break;
                    if ((long long)__builtin_readcyclecounter() - t0 > sync.budget) {  // bounded spin: give up, flag it, never wait again
                        *sync.s_timeout = 1;
                        atomicOr(sync.err, 1u);
                        if (sync.err_host) __hip_atomic_store(sync.err_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        break;
                    }
                }
            }
            if (bits == CL_UNWRITTEN) bits = 0ull;  // timed out: the call's result is undefined (reported), but it stays a number
        }
        s_part[threadIdx.x] = __longlong_as_double((long long)bits);
    }
    __syncthreads();
    {  // lane k of every wavefront adds moment k's G partials in the fixed order q = 0 .. G-1: every workgroup of the cluster gets the same bits
        double sacc = 0.0;
        if (lane < nv)
            for (int q = 0; q < G; q++) sacc += s_part[q * 6 + lane];
#pragma unroll
        for (int k = 0; k < nv; k++)
            v[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(sacc), k), __builtin_amdgcn_readlane(__double2loint(sacc), k));
    }
    m.m00 = v[0], m.m10 = v[1], m.m01 = v[2], m.m11 = v[3], m.m20 = v[4], m.m02 = v[5];
    return m;
}

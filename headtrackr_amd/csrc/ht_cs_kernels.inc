// ht_cs_kernels.inc — the init, histogram and mean-shift kernels of camshift and their few-large-streams forms (row-split init, LUT,
// cluster mean-shift), written once and compiled by two units: ht_camshift.hip (k_cs_init / k_cs_hist / k_cs_meanshift / k_cs_init_rows /
// k_cs_lut / k_cs_meanshift_cluster: stream first + i on bound frame i) and ht_cs_pairs.hip (k_csp_*: any reserved stream on any
// bound frame, from a device table).  In the few-large-streams forms the LUT, the exchange slots and `out` are indexed by the
// workgroup's position s in the call in both units; only state, pixels, histogram slot and rect go through the look-ups.
// The two forms differ in their look-ups only — which stream, which frame, which histogram slot,
// which rect — and the including unit supplies those.  Included INSIDE the unit's anonymous namespace, after ht_cs_device.h.
//
// The including unit defines, before the #include:
//   CS_K(name)               the kernel's name: k_cs_##name / k_csp_##name
//   CsLookup                 type of the look-up argument `lk` of the init and mean-shift kernels (int first / const CspEntry *entries)
//   cs_stream_of(lk, s)      __device__ overloads: workgroup s works on states[cs_stream_of(lk, s)],
//   cs_frame_of(lk, s)         reads bound frame cs_frame_of(lk, s)
//   cs_slot_of(lk, s)          and finds that frame's chunk histograms in slot cs_slot_of(lk, s) of hist
//   CS_INIT_PARAMS           the init kernel's last parameters: `states` and `lk`, in the unit's order, plus what CS_INIT_RECT reads
//   CS_INIT_RECT(s)          the rect of workgroup s
//   CS_HIST_FRAMES_PARAM     the histogram kernel's parameter between chunk_px and hist: empty, or a frame list with its comma
//   CS_HIST_FRAME(y)         the bound frame of grid row y.  A macro, not a function: y is the UNSIGNED blockIdx.y, and an int
//                            in between costs the batch kernel a sign extension
//   CS_INIT_SKIP(s)          optional: a statement at the top of the two init kernels — a workgroup-uniform early return for workgroup s
//                            (ht_cs_pairs.hip: the pair was resolved to "leave the stream alone").  Empty unless the unit defines it
//   CS_KERNELS_PART          optional: 1 = only the init kernel, 2 = only the histogram and mean-shift kernels, 3 = only the row-split init
//                            kernel, 4 = only the LUT and cluster mean-shift kernels.  A code object's .text is laid out in definition
//                            order: ht_camshift.hip includes parts 1, 3, 2, defines k_cs_track_fused, then includes part 4 — the order
//                            its recorded object has.  Without it (ht_cs_pairs.hip): everything
//
// Shared as TEXT on purpose.  profiles/traffic.json is tied to the machine code of the camshift code object, and the same bodies as
// __device__ __forceinline__ functions called from thin kernels change it (the extra inlining level reorders the optimiser's passes:
// LABLOG.md).  Included as text, the batch kernels are the recorded instructions.

#ifndef CS_INIT_SKIP
#define CS_INIT_SKIP(s_)
#endif

#if !defined(CS_KERNELS_PART) || CS_KERNELS_PART == 1

// initTracker: one 1024-thread workgroup per stream; rows of the rect by wavefront, columns by lane (no per-pixel division),
// 8 independent loads per lane in flight (a 360 x 360 rect of a 1080p feed took 174 us with the one-pixel-at-a-time loop)
__global__ __launch_bounds__(INIT_NT) void CS_K(init)(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H, CS_INIT_PARAMS) {
    __shared__ uint32_t h[4096];
    const int s = blockIdx.x;
    CS_INIT_SKIP(s)
    for (int i = threadIdx.x; i < 4096; i += INIT_NT) h[i] = 0;
    __syncthreads();
    const ht_cs_rect r = CS_INIT_RECT(s);
    const int stream = cs_stream_of(lk, s);  // every look-up in front of the loops (one scalar load for a table entry's fields)
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)cs_frame_of(lk, s) * frame_stride);
    const int rw = max(r.width, 0), rh = max(r.height, 0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NWV = INIT_NT / 64;
    for (int j0 = wave; j0 - wave < rh; j0 += 8 * NWV) {      // same trip count for every wavefront's lanes (ballots inside)
        for (int cb = 0; cb < rw; cb += 64) {
            const int c = cb + lane;
            uint32_t px[8];
            bool in[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int y = r.y + j0 + u * NWV, x = r.x + c;
                in[u] = c < rw && j0 + u * NWV < rh;                                   // inside the rect
                const bool img_ok = in[u] && x >= 0 && x < W && y >= 0 && y < H;      // inside the canvas
                px[u] = img_ok ? img[(size_t)y * W + x] : 0u;  // getImageData outside the canvas: transparent black -> bin 0 (camshift.js:206)
            }
#pragma unroll
            for (int u = 0; u < 8; u++) CS_BATCH_LOADED(px[u]);
#pragma unroll
            for (int u = 0; u < 8; u++) hist_add_wave(h, cs_bin(px[u]), 1u, in[u]);
        }
    }
    __syncthreads();
    HtCsState &st = states[stream];
    for (int i = threadIdx.x; i < 4096; i += INIT_NT) st.model[i] = h[i];
    if (threadIdx.x == 0) {
        st.sw[0] = r.x, st.sw[1] = r.y, st.sw[2] = r.width, st.sw[3] = r.height;  // camshift.js:209
        st.x = st.y = st.width = st.height = st.angle = 0.0;                         // camshift.js:210
        st.win_px = st.calls = 0;
    }
}

#endif
#if !defined(CS_KERNELS_PART) || CS_KERNELS_PART == 2

// full-frame histogram (camshift.js:268): grid (chunks, frames) -> hist[grid row][chunk][4096] partial histograms.
// 4 pixels per 16-byte load.  LDS atomics on one address serialise lane by lane, and flat image regions put whole
// wavefronts into one bin (a flat 320x240 background cost 64 cycles per wave instruction: the kernel ran at a quarter of
// HBM speed), so counts are merged before they reach LDS: the 4 pixels of a thread when they share a bin, and all lanes
// that share the first active lane's bin through one ballot — one atomic for the whole wavefront on flat regions,
// a few extra scalar instructions elsewhere.  Counts are integers: any order gives the same histogram.
__global__ __launch_bounds__(HIST_NT) void CS_K(hist)(const uint8_t *__restrict__ frames, size_t frame_stride, uint32_t npix, uint32_t chunk_px,
                                                      CS_HIST_FRAMES_PARAM uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[4096];
    for (int i = threadIdx.x; i < 4096; i += HIST_NT) h[i] = 0;
    __syncthreads();
    const uint8_t *frame = frames + (size_t)CS_HIST_FRAME(blockIdx.y) * frame_stride;
    const uint32_t beg = blockIdx.x * chunk_px, end = min(beg + chunk_px, npix);  // chunk_px is a multiple of 4 * HIST_NT; beg < npix
    const uint32_t nquad = (end - beg) / 4;
    const uint4 *img4 = reinterpret_cast<const uint4 *>(frame + (size_t)beg * 4);
    const uint32_t iters = chunk_px / (4 * HIST_NT);
    // HIST_UNROLL loads of a thread in flight before the first bin is counted, written out: the wave-level merge below is convergent code,
    // which keeps the optimiser from unrolling the loop itself (`#pragma unroll` was refused), and with ONE 16-byte load in flight per
    // thread the pass was a chain of chunk_px / 1024 memory round trips (16 x ~1.3 us at 1080p = the kernel's whole duration)
    for (uint32_t it0 = 0; it0 < iters; it0 += HIST_UNROLL) {
        uint4 pv[HIST_UNROLL];
        bool onv[HIST_UNROLL];
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            const uint32_t i = (it0 + (uint32_t)u) * HIST_NT + threadIdx.x;
            onv[u] = it0 + (uint32_t)u < iters && i < nquad;
            pv[u] = make_uint4(0u, 0u, 0u, 0u);
            if (onv[u]) pv[u] = img4[i];
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            CS_BATCH_LOADED(pv[u].x);
            CS_BATCH_LOADED(pv[u].y);
            CS_BATCH_LOADED(pv[u].z);
            CS_BATCH_LOADED(pv[u].w);
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; u++) {
            if (it0 + (uint32_t)u >= iters) break;  // workgroup-uniform
            const uint4 p = pv[u];
            const bool on = onv[u];
            const uint32_t b0 = cs_bin(p.x), b1 = cs_bin(p.y), b2 = cs_bin(p.z), b3 = cs_bin(p.w);
            const bool flat = (b0 == b1) && (b2 == b3) && (b0 == b2);
            hist_add_wave(h, b0, flat ? 4u : 1u, on);
            if (on && !flat) {
                atomicAdd(&h[b1], 1u);
                atomicAdd(&h[b2], 1u);
                atomicAdd(&h[b3], 1u);
            }
        }
    }
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frame);
    for (uint32_t i = beg + nquad * 4 + threadIdx.x; i < end; i += HIST_NT) atomicAdd(&h[cs_bin(img[i])], 1u);  // < 4 pixels
    __syncthreads();
    // this chunk's partial histogram, written whole (no zeroing pass, no global atomics); the mean-shift kernel adds the chunks
    uint32_t *out = hist + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4096;
    for (int i = threadIdx.x; i < 4096; i += HIST_NT) out[i] = h[i];
}

// track() of workgroup blockIdx.x: ONE workgroup keeps the 4096-entry weight LUT in LDS and runs the whole mean-shift loop on its
// stream's state and its frame's pixels; the frame's histogram is the sum of the chunk histograms of its slot; the track object
// goes to out[blockIdx.x]
__global__ __launch_bounds__(CS_NT) void CS_K(meanshift)(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H,
                                                         const uint32_t *__restrict__ hist, int nchunks, HtCsState *__restrict__ states,
                                                         CsLookup lk, int calc_angles, int max_it, int region_cap, ht_cs_trackobj *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cs_dyn[];  // [region_cap] u16 bins of the cached search region
    __shared__ double lut[4096];
    __shared__ double red[6][CS_NT / 64];
    __shared__ int s_sw[4];
    const int s = blockIdx.x;
    HtCsState &st = states[cs_stream_of(lk, s)];
    const uint32_t *cur = hist + (size_t)cs_slot_of(lk, s) * nchunks * 4096;
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)cs_frame_of(lk, s) * frame_stride);
    {  // getWeights, camshift.js:314-330; the frame's histogram = sum of its chunk histograms (4 bins per 16-byte load)
        const uint4 *cur4 = reinterpret_cast<const uint4 *>(cur);
        const uint4 *model4 = reinterpret_cast<const uint4 *>(st.model);
        for (int i4 = threadIdx.x; i4 < 1024; i4 += CS_NT) {
            uint4 acc = make_uint4(0u, 0u, 0u, 0u);
            for (int k = 0; k < nchunks; k++) {
                const uint4 v = cur4[(size_t)k * 1024 + i4];
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
            const uint4 m = model4[i4];
            const uint32_t chv[4] = {acc.x, acc.y, acc.z, acc.w}, mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double p = 0.0;
                if (chv[q] != 0) {
                    p = (double)mv[q] / (double)chv[q];
                    p = p < 1.0 ? p : 1.0;
                }
                lut[i4 * 4 + q] = p;
            }
        }
    }
    if (threadIdx.x < 4) s_sw[threadIdx.x] = st.sw[threadIdx.x];
    __syncthreads();
    const CsRegion R = cs_cache_region<CS_NT>(img, W, H, s_sw, reinterpret_cast<uint16_t *>(cs_dyn), region_cap);
    __syncthreads();
    meanshift_body(W, H, s_sw, st, calc_angles, max_it, out ? out + s : nullptr, nullptr, true,
                   [&](int x, int y, int w, int h) { return window_moments_any<true, CS_NT / 64>(img, W, lut, R, x, y, w, h, red); });
}

#endif
#if !defined(CS_KERNELS_PART) || CS_KERNELS_PART == 3

// initTracker for a FEW streams with large rects (a live 1080p feed: 360 x 360 = 0.5 MB took the single workgroup above 54 us):
// grid (G, streams), workgroup g takes rows g*4 + wavefront, + 4 G, ...; LDS histogram per workgroup, non-zero bins added to the
// model (zeroed by the host) with global atomics — integer counts, any order gives the same model.
__global__ __launch_bounds__(256) void CS_K(init_rows)(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H, CS_INIT_PARAMS) {
    __shared__ uint32_t h[4096];
    const int s = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    CS_INIT_SKIP(s)
    for (int i = threadIdx.x; i < 4096; i += 256) h[i] = 0;
    __syncthreads();
    const ht_cs_rect r = CS_INIT_RECT(s);
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)cs_frame_of(lk, s) * frame_stride);
    const int rw = max(r.width, 0), rh = max(r.height, 0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = g * 4 + wave; j - wave < rh + 3; j += 4 * G) {  // same trip count for the four wavefronts of a workgroup
        const int y = r.y + j;
        for (int cb = 0; cb < rw; cb += 256) {
            uint32_t px[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int c = cb + 64 * u + lane, x = r.x + c;
                in[u] = c < rw && j < rh;
                px[u] = (in[u] && x >= 0 && x < W && y >= 0 && y < H) ? img[(size_t)y * W + x] : 0u;  // outside the canvas: transparent black (camshift.js:206)
            }
#pragma unroll
            for (int u = 0; u < 4; u++) CS_BATCH_LOADED(px[u]);
#pragma unroll
            for (int u = 0; u < 4; u++) hist_add_wave(h, cs_bin(px[u]), 1u, in[u]);
        }
    }
    __syncthreads();
    HtCsState &st = states[cs_stream_of(lk, s)];
    for (int i = threadIdx.x; i < 4096; i += 256)
        if (h[i]) atomicAdd(&st.model[i], h[i]);
    if (g == 0 && threadIdx.x == 0) {
        st.sw[0] = r.x, st.sw[1] = r.y, st.sw[2] = r.width, st.sw[3] = r.height;  // camshift.js:209
        st.x = st.y = st.width = st.height = st.angle = 0.0;                         // camshift.js:210
        st.win_px = st.calls = 0;
    }
}

#endif
#if !defined(CS_KERNELS_PART) || CS_KERNELS_PART == 4

// weight LUT of every stream from its chunk histograms (getWeights, camshift.js:314-330): grid (64, streams) x 512 threads;
// a block owns 64 bins, its 8 wavefronts each sum every 8th chunk (a single 1080p stream has 127 chunk histograms = 2 MB)
__global__ __launch_bounds__(512) void CS_K(lut)(const uint32_t *__restrict__ hist, int nchunks, const HtCsState *__restrict__ states, CsLookup lk,
                                                double *__restrict__ lut, unsigned long long *__restrict__ cluster_parts) {
    __shared__ uint32_t part[8][64];
    const int s = blockIdx.y, lane = threadIdx.x & 63, grp = threadIdx.x >> 6, bin = blockIdx.x * 64 + lane;
    {   // the stream's exchange slots of the cluster launch that follows: every entry "not written yet" (was a memset of its own)
        const uint32_t i = blockIdx.x * 512u + threadIdx.x;
        if (i < (uint32_t)(CL_SLOTS * CL_MAXG * 6)) cluster_parts[(size_t)s * CL_SLOTS * CL_MAXG * 6 + i] = CL_UNWRITTEN;
    }
    const uint32_t *cur = hist + (size_t)cs_slot_of(lk, s) * nchunks * 4096 + bin;
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
            p = (double)states[cs_stream_of(lk, s)].model[bin] / (double)ch;
            p = p < 1.0 ? p : 1.0;
        }
        lut[(size_t)s * 4096 + bin] = p;
    }
}

__global__ __launch_bounds__(CL_NT) void CS_K(meanshift_cluster)(const uint8_t *__restrict__ frames, size_t frame_stride, int W, int H, const double *__restrict__ lut_g,
                                                                HtCsState *__restrict__ states, CsLookup lk, int calc_angles, int max_it, int G,
                                                                double *__restrict__ parts,
                                                                uint32_t *__restrict__ err, uint32_t *__restrict__ err_host, long long budget,
                                                                ht_cs_trackobj *__restrict__ out, uint32_t *__restrict__ done_flags, uint32_t done_seq) {
    __shared__ double lut[4096];
    __shared__ double red[6][CL_NT / 64];
    __shared__ double s_part[CL_MAXG * 6];
    __shared__ int s_sw[4];
    __shared__ int s_timeout;
    if (threadIdx.x == 0) s_timeout = 0;
    const int s = blockIdx.x / G, g = blockIdx.x - s * G;
    HtCsState &st = states[cs_stream_of(lk, s)];
    const uint32_t *img = reinterpret_cast<const uint32_t *>(frames + (size_t)cs_frame_of(lk, s) * frame_stride);
    {
        const double2 *src = reinterpret_cast<const double2 *>(lut_g + (size_t)s * 4096);
        for (int i = threadIdx.x; i < 2048; i += CL_NT) reinterpret_cast<double2 *>(lut)[i] = src[i];
    }
    if (threadIdx.x < 4) s_sw[threadIdx.x] = st.sw[threadIdx.x];
    __syncthreads();
    double *my_parts = parts + (size_t)s * CL_SLOTS * CL_MAXG * 6;
    const ClusterSync sync = {err, err_host, budget, &s_timeout};
    int slot = 0;
    meanshift_body(W, H, s_sw, st, calc_angles, max_it, out ? out + s : nullptr, nullptr, g == 0, [&](int x, int y, int w, int h) {
        const int sl = slot++;
        return cluster_moments<true>(img, W, lut, x, y, w, h, red, s_part, g, G, my_parts, sync, sl);
    }, done_flags ? done_flags + s : nullptr, done_seq);
}

#endif
#undef CS_KERNELS_PART

// ht_group.hip — the last stage of detect_objects on the device: a batch's raw hits -> per frame the emission order, the seq rects,
// ccv's grouping and facetrackr's best face (reference: src/ccv.js:34-107, 227-234, 249-332; src/facetrackr.js:157-165).
//
// Three launches on the context's stream behind the batch in flight, none of which waits for another workgroup:
//   k_grp_bucket   one workgroup: hits per frame (one atomic per hit on the frame's counter), exclusive scan of the counts (bucket starts,
//                  scatter cursors), the hits scattered into the second hit buffer frame by frame, the batch's nhits next to the records;
//                  hits whose frame or scale is out of range are counted in the head's `bad` word and never used as an index
//   k_grp_frames   one workgroup per frame, one thread per hit, everything in LDS (two launches: a wavefront per frame with <= 64 hits,
//                  up to 1024 threads per frame above that):
//                  rank by counting on the packed key (scale, q, y, x) = emission order; seq rects from the level scales the HOST computed
//                  (ht_post_level_scales: V8's pow constants); connected components of the symmetric closure of ccv.js:252-261 by
//                  min-label propagation with pointer jumping — a label only ever decreases and is at most what plain propagation has
//                  after the same number of rounds, so n rounds bound the loop; every class summed by the thread of its smallest member in
//                  ascending member order from 0 (ccv.js:274-289); min_neighbors and nested-rect filters (ccv.js:293-330) and the
//                  strict-'>' arg-max in class order.
// The reference's result depends only on the emission order, not on the shape of its union-find trees, so this reproduces the bytes of
// ht_post_group_rects / ht_post_best_face.  Every binary64 operation is written as the separately rounded operation it is.
//
// A frame with more hits than the cap (1024: one thread and 47 bytes of LDS per hit; option group_cap lowers it) is NOT processed: its
// status word says so and the collect call finishes it on the host (ht_grp_complete_frame).
//
// Compiled as part of ht_backproject.hip's code object, like ht_ingest.hip: the pyramid, scan and camshift objects stay as recorded.
#include <algorithm>
#include <string>

#include "ht_group_plan.h"
#include "ht_internal.h"

namespace {

constexpr int GRP_SCAN_NT = 1024;  // threads of the bucket kernel's one workgroup
constexpr int GRP_CAP = (int)HT_GRP_CAP_MAX;
constexpr int GRP_WAVE = (int)HT_GRP_CAP_MIN;  // the one-wavefront form of k_grp_frames

__device__ __forceinline__ bool grp_hit_ok(const ht_hit &h, uint32_t nframes) { return h.frame < nframes && h.scale < HT_MAX_LEVELS; }

// exclusive prefix of v over the workgroup's threads (*total = the sum); s_w: one word per wavefront
__device__ __forceinline__ uint32_t grp_scan_u32(uint32_t v, uint32_t *s_w, uint32_t *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    __syncthreads();  // s_w may still be read from the previous use
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int q = 0; q < nw; q++) {
        const uint32_t t = s_w[q];
        base += q < w ? t : 0u;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

// Bucket by frame in ONE workgroup, so that its four phases are separated by workgroup barriers instead of launches (a launch costs more
// than a phase: a 256-frame batch has ~1.4 k hits, two per thread): zero the per-frame counters; count min(nhits, capacity) hits per
// frame; exclusive scan of the counts = bucket starts and scatter cursors; scatter into the second hit buffer (the order inside a bucket
// is arbitrary).  A hit whose frame or scale is out of range is counted in the head's `bad` word, never used as an index and not
// scattered.  The counters and cursors are only touched by atomics here (they execute in L2: no wavefront of this workgroup can see a
// stale cached copy of a word another wavefront has changed).  Linear in the hit count: ~1 ns per hit, next to a scan that needs
// ~150 ns of device time per hit it finds.
__global__ __launch_bounds__(GRP_SCAN_NT) void k_grp_bucket(const ht_hit *__restrict__ hits, const uint32_t *__restrict__ nhits_p, uint32_t capacity, uint32_t nframes,
                                                            uint32_t *__restrict__ count, uint32_t *__restrict__ start, uint32_t *__restrict__ cursor,
                                                            HtGrpHead *__restrict__ head, ht_hit *__restrict__ hits2) {
    __shared__ uint32_t s_w[GRP_SCAN_NT / 64];
    const uint32_t nh = *nhits_p, n = min(nh, capacity);
    for (uint32_t f = threadIdx.x; f < nframes; f += GRP_SCAN_NT) atomicExch(&count[f], 0u);
    if (threadIdx.x == 0) {
        head->nhits = nh, head->pad[0] = 0, head->pad[1] = 0;
        atomicExch(&head->bad, 0u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += GRP_SCAN_NT) {
        const ht_hit h = hits[i];
        if (grp_hit_ok(h, nframes)) atomicAdd(&count[h.frame], 1u);
        else atomicAdd(&head->bad, 1u);
    }
    __syncthreads();
    uint32_t carry = 0;
    for (uint32_t f0 = 0; f0 < nframes; f0 += GRP_SCAN_NT) {  // workgroup-uniform trip count
        const uint32_t f = f0 + threadIdx.x;
        const uint32_t v = f < nframes ? atomicAdd(&count[f], 0u) : 0u;
        uint32_t tot;
        const uint32_t ex = grp_scan_u32(v, s_w, &tot);
        if (f < nframes) {
            start[f] = carry + ex;
            atomicExch(&cursor[f], carry + ex);
        }
        carry += tot;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += GRP_SCAN_NT) {
        const ht_hit h = hits[i];
        if (!grp_hit_ok(h, nframes)) continue;
        const uint32_t pos = atomicAdd(&cursor[h.frame], 1u);  // < the frame's bucket end <= n <= capacity: the same hits were counted above
        if (pos < capacity) hits2[pos] = h;
    }
}

// exclusive prefix of a flag over the workgroup's threads
__device__ __forceinline__ uint32_t grp_scan_flag(bool flag, uint32_t *s_w, uint32_t *total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint32_t pre = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_w[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int q = 0; q < nw; q++) {
        const uint32_t t = s_w[q];
        base += q < w ? t : 0u;
        tot += t;
    }
    *total = tot;
    return base + pre;
}

__device__ __forceinline__ double grp_round_term(double w, double k) { return floor(__dadd_rn(__dmul_rn(w, k), 0.5)); }  // floor(w * k + 0.5)

__device__ __forceinline__ void grp_store_record(double *rec, double x, double y, double w, double h, double c, double nn, double frame) {
    reinterpret_cast<double2 *>(rec)[0] = make_double2(x, y);
    reinterpret_cast<double2 *>(rec)[1] = make_double2(w, h);
    reinterpret_cast<double2 *>(rec)[2] = make_double2(c, nn);
    reinterpret_cast<double2 *>(rec)[3] = make_double2(frame, 1.0);
}

// grid = frames, thread i holds hit i of the frame, then item i of every later list.  Two launches share the frames by their hit counts:
// <64> — one wavefront per frame, its barriers cost nothing — takes the frames with at most 64 hits (the empty ones included: a batch of
// the benchmark's mix has at most 25 per frame), <1024> with `cap` threads (a power of two in [128, 1024]) those with lo <= n <= cap; a
// frame above the cap is flagged by the launch told to (flag_above) and left to the host.  Every frame is written by exactly one of them.
template <int NT>
__global__ __launch_bounds__(NT) void k_grp_frames(const ht_hit *__restrict__ hits2, const uint32_t *__restrict__ start, const uint32_t *__restrict__ count,
                                                   const double *__restrict__ sx, uint32_t cw, uint32_t ch, int32_t min_neighbors, int32_t frame_base, uint32_t lo,
                                                   uint32_t flag_above, double *__restrict__ records, uint32_t *__restrict__ status,
                                                   uint32_t *__restrict__ ngrouped, ht_rect *__restrict__ rects) {
    __shared__ unsigned long long s_key[NT];  // the packed keys; later the widths of the averaged rects (binary64 bits)
    __shared__ double s_x[NT], s_y[NT], s_c[NT], s_h[NT];
    __shared__ int32_t s_nn[NT];
    __shared__ uint16_t s_lab[NT];
    __shared__ uint8_t s_sc[NT];  // level of a seq rect; later the keep flag of an averaged rect
    __shared__ double t_s[HT_MAX_LEVELS], t_w[HT_MAX_LEVELS], t_h[HT_MAX_LEVELS], t_w15[HT_MAX_LEVELS], t_d[HT_MAX_LEVELS];
    __shared__ uint32_t s_w[NT / 64];

    const uint32_t f = blockIdx.x, i = threadIdx.x;
    const uint32_t n = count[f], beg = start[f];
    double *rec = records + (size_t)f * HT_GRP_REC_F64;
    const double frame_index = (double)(frame_base + (int32_t)f);
    // workgroup-uniform exits: the other launch's frame; nothing to do; more than a workgroup takes (the host finishes the frame)
    if (n < lo || (n > blockDim.x && !flag_above)) return;
    if (n == 0 || n > blockDim.x) {
        if (i == 0) {
            grp_store_record(rec, 0.0, 0.0, 0.0, 0.0, -10000.0, 0.0, frame_index);  // facetrackr.js:233-241
            status[f] = n ? (uint32_t)HT_GRP_ST_OVER_CAP : 0u;
            ngrouped[f] = 0;
        }
        return;
    }
    const bool on = i < n;

    // level tables: scale, window width / height, floor(w * 1.5 + 0.5), floor(w * 0.25 + 0.5)
    for (uint32_t l = i; l < HT_MAX_LEVELS; l += blockDim.x) {
        const double s = sx[l], w = __dmul_rn((double)cw, s);
        t_s[l] = s, t_w[l] = w, t_h[l] = __dmul_rn((double)ch, s);
        t_w15[l] = grp_round_term(w, 1.5), t_d[l] = grp_round_term(w, 0.25);
    }
    ht_hit h = {0, 0, 0, 0, 0, 0, 0, 0.0};
    unsigned long long key = 0;
    if (on) {
        h = hits2[beg + i];
        key = ((unsigned long long)h.scale << 40) | ((unsigned long long)h.q << 32) | ((unsigned long long)h.y << 16) | (unsigned long long)h.x;
        s_key[i] = key;
    }
    __syncthreads();
    // emission order: the rank of the key among the frame's keys (ties, which the scan never emits, by bucket position)
    if (on) {
        uint32_t rank = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < n; j++) {
            const unsigned long long kj = s_key[j];
            rank += (kj < key || (kj == key && j < i)) ? 1u : 0u;
        }
        const uint32_t l = min((uint32_t)h.scale, (uint32_t)HT_MAX_LEVELS - 1u);  // (k_grp_bucket let no other level through)
        const double s = t_s[l];
        s_x[rank] = __dmul_rn((double)((int)h.x * 4 + ((int)h.q & 1) * 2), s);   // ccv.js:228
        s_y[rank] = __dmul_rn((double)((int)h.y * 4 + ((int)h.q >> 1) * 2), s);  // ccv.js:229
        s_c[rank] = h.sum;                                                      // ccv.js:233
        s_sc[rank] = (uint8_t)l;
    }
    __syncthreads();

    uint32_t n2 = n;  // rects in front of the nested-rect filter
    bool keep = on;
    if (min_neighbors > 0) {
        // ---- connected components (ccv.js:34-107 with the predicate of ccv.js:252-261) --------------------------------------------
        double xi = 0, yi = 0, wi = 0, w15i = 0, di = 0;
        if (on) {
            const uint32_t l = s_sc[i];
            xi = s_x[i], yi = s_y[i], wi = t_w[l], w15i = t_w15[l], di = t_d[l];
        }
        const double xh = __dadd_rn(xi, di), xl = __dadd_rn(xi, -di), yh = __dadd_rn(yi, di), yl = __dadd_rn(yi, -di);
        // is seq rect j joined with this thread's (ccv.js:252-261 in either direction)?  Broadcast LDS reads: every lane asks for the same j
        auto similar = [&](uint32_t j) {
            const uint32_t lj = s_sc[j];
            const double xj = s_x[j], yj = s_y[j], wj = t_w[lj], w15j = t_w15[lj], dj = t_d[lj];
            const bool pij = xj <= xh && xj >= xl && yj <= yh && yj >= yl && wj <= w15i && w15j >= wi;
            const bool pji = xi <= __dadd_rn(xj, dj) && xi >= __dadd_rn(xj, -dj) && yi <= __dadd_rn(yj, dj) && yi >= __dadd_rn(yj, -dj) && wi <= w15j && w15i >= wj;
            return (pij || pji) && j != i;
        };
        s_lab[i] = (uint16_t)i;
        unsigned long long adj = 0;  // the one-wavefront form: this rect's neighbours as a bit mask, formed once instead of once per round
        if (NT <= 64 && on) {
#pragma unroll 4
            for (uint32_t j = 0; j < n; j++) adj |= similar(j) ? 1ull << j : 0ull;
        }
        __syncthreads();
        for (uint32_t round = 0; round < n; round++) {  // workgroup-uniform exit below
            uint32_t lab = i, nl = i;
            if (on) {
                lab = s_lab[i];
                uint32_t m = lab;
                if (NT <= 64) {
                    for (unsigned long long a = adj; a != 0; a &= a - 1) m = min(m, (uint32_t)s_lab[__builtin_ctzll(a)]);
                } else {
#pragma unroll 4
                    for (uint32_t j = 0; j < n; j++)
                        if (similar(j)) m = min(m, (uint32_t)s_lab[j]);
                }
                nl = s_lab[m];  // pointer jump through the labels of this round's start: nl <= m <= lab
            }
            __syncthreads();  // every read of the round's labels is done
            if (on) s_lab[i] = (uint16_t)nl;
            if (!__syncthreads_or(on && nl != lab)) break;
        }
        // ---- class sums in ascending member order from 0 (ccv.js:274-289), by the thread of the class's smallest member -----------
        const bool root = on && s_lab[i] == i;
        double ax = 0, ay = 0, aw = 0, ah = 0, ac = 0;
        int32_t nn = 0;
        if (root) {
            for (uint32_t j = i; j < n; j++) {
                if (s_lab[j] != i) continue;
                const uint32_t lj = s_sc[j];
                const double cj = s_c[j];
                if (nn == 0) ac = cj;
                ++nn;
                ax = __dadd_rn(ax, s_x[j]), ay = __dadd_rn(ay, s_y[j]), aw = __dadd_rn(aw, t_w[lj]), ah = __dadd_rn(ah, t_h[lj]);
                ac = (ac < cj) ? cj : ac;  // std::max(ac, cj)
            }
        }
        const bool pass = root && nn >= min_neighbors;  // ccv.js:293-303, in class order = order of the smallest members
        const uint32_t k = grp_scan_flag(pass, s_w, &n2);  // (its barriers end every read of the seq arrays)
        if (pass) {
            const double dn = (double)nn, d2n = (double)(2 * nn);
            s_x[k] = __ddiv_rn(__dadd_rn(__dmul_rn(ax, 2.0), dn), d2n);
            s_y[k] = __ddiv_rn(__dadd_rn(__dmul_rn(ay, 2.0), dn), d2n);
            s_key[k] = (unsigned long long)__double_as_longlong(__ddiv_rn(__dadd_rn(__dmul_rn(aw, 2.0), dn), d2n));
            s_h[k] = __ddiv_rn(__dadd_rn(__dmul_rn(ah, 2.0), dn), d2n);
            s_c[k] = ac;
            s_nn[k] = nn;
        }
        __syncthreads();
        // ---- nested-rect filter (ccv.js:307-330) ---------------------------------------------------------------------------------
        keep = i < n2;
        if (keep) {
            const double x1 = s_x[i], y1 = s_y[i], w1 = __longlong_as_double((long long)s_key[i]), h1 = s_h[i];
            const double x1w = __dadd_rn(x1, w1), y1h = __dadd_rn(y1, h1);
            const int32_t n1 = s_nn[i];
#pragma unroll 2
            for (uint32_t j = 0; j < n2; j++) {  // (the reference stops at the first hit; the answer is the same)
                const double x2 = s_x[j], y2 = s_y[j], w2 = __longlong_as_double((long long)s_key[j]), h2 = s_h[j];
                const int32_t nn2 = s_nn[j];
                const double d = grp_round_term(w2, 0.25);
                if (j != i && x1 >= __dadd_rn(x2, -d) && y1 >= __dadd_rn(y2, -d) && x1w <= __dadd_rn(__dadd_rn(x2, w2), d) &&
                    y1h <= __dadd_rn(__dadd_rn(y2, h2), d) && (nn2 > max(3, n1) || n1 < 3))
                    keep = false;
            }
        }
    } else {
        // min_neighbors == 0: the grouped list is the seq list itself (ccv.js:249); the keys have been read for the last time above
        if (on) {
            const uint32_t l = s_sc[i];
            s_key[i] = (unsigned long long)__double_as_longlong(t_w[l]);
            s_h[i] = t_h[l];
            s_nn[i] = 1;
        }
    }
    uint32_t ng;
    const uint32_t ko = grp_scan_flag(keep, s_w, &ng);  // its barriers end the filter's reads and publish the min_neighbors == 0 path's writes
    s_sc[i] = keep ? 1 : 0;
    if (keep) {
        ht_rect r;
        r.x = s_x[i], r.y = s_y[i], r.width = __longlong_as_double((long long)s_key[i]), r.height = s_h[i], r.confidence = s_c[i];
        r.neighbors = s_nn[i], r.reserved = 0;
        rects[beg + ko] = r;  // ko < ng <= n: inside the frame's bucket
    }
    __syncthreads();
    if (i == 0) {  // facetrackr.js:157-165: strict '>', the first maximum stays
        bool first = true;
        uint32_t b = 0;
        double bc = -10000.0;
        for (uint32_t j = 0; j < n2; j++) {
            if (!s_sc[j]) continue;
            const double cj = s_c[j];
            if (first || cj > bc) b = j, bc = cj, first = false;
        }
        if (first) grp_store_record(rec, 0.0, 0.0, 0.0, 0.0, -10000.0, 0.0, frame_index);
        else grp_store_record(rec, s_x[b], s_y[b], __longlong_as_double((long long)s_key[b]), s_h[b], bc, (double)s_nn[b], frame_index);
        status[f] = 0;
        ngrouped[f] = ng;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------

inline HtPostCfg grp_cfg(const ht_ctx *c) { return HtPostCfg{c->interval, c->cascade.cw, c->cascade.ch}; }
inline uint32_t *grp_nword(ht_ctx *c) { return reinterpret_cast<uint32_t *>(c->d_grp_konst + HT_MAX_LEVELS); }

// this unit's buffers that grow with the batch, through the library's one grow helper
template <typename T>
ht_status grp_grow(ht_ctx *c, T *&p, size_t &cap, size_t need, const char *message) {
    return ht_grow_device(c, &p, &cap, need, message);
}

// the buffers of the route for a batch of nframes frames; allocates (and then waits for the stream) only on first use or growth
ht_status grp_reserve(ht_ctx *c, uint32_t nframes) {
    if (!c->d_grp_konst) {
        double sx[HT_MAX_LEVELS + 1];
        ht_post_level_scales(grp_cfg(c), sx);  // the host's pow constants: never recomputed on the device
        sx[HT_MAX_LEVELS] = 0;
        if (hipMalloc(reinterpret_cast<void **>(&c->d_grp_konst), sizeof(sx)) != hipSuccess) {
            (void)hipGetLastError();
            c->d_grp_konst = nullptr;
            return ht_fail(c, HT_ERR_NOMEM, "device grouping: hipMalloc failed (level scales)");
        }
        HT_HIP(c, hipMemcpy(c->d_grp_konst, sx, sizeof(sx), hipMemcpyHostToDevice));
    }
    if (!c->d_grp_hits2 && hipMalloc(reinterpret_cast<void **>(&c->d_grp_hits2), (size_t)c->hit_capacity * sizeof(ht_hit)) != hipSuccess) {
        (void)hipGetLastError();
        c->d_grp_hits2 = nullptr;
        return ht_fail(c, HT_ERR_NOMEM, "device grouping: hipMalloc failed (bucketed hits)");
    }
    if (!c->d_grp_rects && hipMalloc(reinterpret_cast<void **>(&c->d_grp_rects), (size_t)c->hit_capacity * sizeof(ht_rect)) != hipSuccess) {
        (void)hipGetLastError();
        c->d_grp_rects = nullptr;
        return ht_fail(c, HT_ERR_NOMEM, "device grouping: hipMalloc failed (grouped rects)");
    }
    const HtGrpLayout L = ht_grp_layout(nframes);
    ht_status st = grp_grow(c, c->d_grp_out, c->grp_out_cap, L.bytes, "device grouping: hipMalloc failed (result block)");
    if (st == HT_OK) st = grp_grow(c, c->d_grp_cursor, c->grp_cursor_cap, (size_t)nframes, "device grouping: hipMalloc failed (cursors)");
    if (st != HT_OK) return st;
    if (c->h_grp_out_cap < L.bytes) {
        HT_HIP(c, hipStreamSynchronize(c->stream));
        if (c->h_grp_out) (void)hipHostFree(c->h_grp_out);
        c->h_grp_out = nullptr, c->h_grp_out_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void **>(&c->h_grp_out), L.bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return ht_fail(c, HT_ERR_NOMEM, "device grouping: hipHostMalloc failed (result staging)");
        }
        c->h_grp_out_cap = L.bytes;
    }
    return HT_OK;
}

// the four launches: hits (n of them in *nhits_p, at most hit_capacity read) -> the result block, hits2, rects
ht_status grp_launch(ht_ctx *c, const ht_hit *d_hits, const uint32_t *d_nhits, uint32_t nframes, int32_t min_neighbors, int32_t frame_base) {
    const HtGrpLayout L = ht_grp_layout(nframes);
    HtGrpHead *head = reinterpret_cast<HtGrpHead *>(c->d_grp_out);
    double *records = reinterpret_cast<double *>(c->d_grp_out + L.records);
    uint32_t *status = reinterpret_cast<uint32_t *>(c->d_grp_out + L.status), *ngrouped = reinterpret_cast<uint32_t *>(c->d_grp_out + L.ngrouped);
    uint32_t *count = reinterpret_cast<uint32_t *>(c->d_grp_out + L.count), *start = reinterpret_cast<uint32_t *>(c->d_grp_out + L.start);
    const uint32_t cap = ht_grp_cap(c->grp_cap_opt);
    {  // (no memset: the bucket kernel zeroes what it counts in, and every other word of the block is written for every frame)
        HtProfScope ps(c, "grp_bucket");
        hipLaunchKernelGGL(k_grp_bucket, dim3(1), dim3(GRP_SCAN_NT), 0, c->stream, d_hits, d_nhits, c->hit_capacity, nframes, count, start, c->d_grp_cursor, head,
                           c->d_grp_hits2);
        HT_HIP(c, hipGetLastError());
    }
    {
        HtProfScope ps(c, "grp_frames");
        hipLaunchKernelGGL(k_grp_frames<GRP_WAVE>, dim3(nframes), dim3(GRP_WAVE), 0, c->stream, c->d_grp_hits2, start, count, c->d_grp_konst, c->cascade.cw, c->cascade.ch, min_neighbors,
                           frame_base, 0u, cap == (uint32_t)GRP_WAVE ? 1u : 0u, records, status, ngrouped, c->d_grp_rects);
        HT_HIP(c, hipGetLastError());
        if (cap > (uint32_t)GRP_WAVE) {
            hipLaunchKernelGGL(k_grp_frames<GRP_CAP>, dim3(nframes), dim3(cap), 0, c->stream, c->d_grp_hits2, start, count, c->d_grp_konst, c->cascade.cw, c->cascade.ch, min_neighbors,
                               frame_base, (uint32_t)GRP_WAVE + 1u, 1u, records, status, ngrouped, c->d_grp_rects);
            HT_HIP(c, hipGetLastError());
        }
    }
    return HT_OK;
}

// After the result block has reached h_grp_out: the per-frame tables into the context, one rect per frame into best, and the frames the
// kernel flagged finished on the host (their hits are fetched only here; their records on the device are completed too,
// and — lists_to_device: the collect, whose batch ht_camshift_init_faces may read afterwards — their grouped lists).
ht_status grp_take_results(ht_ctx *c, uint32_t nframes, int32_t min_neighbors, int32_t frame_base, ht_rect *best, const char *fn, bool lists_to_device) {
    const HtGrpLayout L = ht_grp_layout(nframes);
    const double *records = reinterpret_cast<const double *>(c->h_grp_out + L.records);
    const uint32_t *status = reinterpret_cast<const uint32_t *>(c->h_grp_out + L.status), *ngrouped = reinterpret_cast<const uint32_t *>(c->h_grp_out + L.ngrouped);
    const uint32_t *count = reinterpret_cast<const uint32_t *>(c->h_grp_out + L.count), *start = reinterpret_cast<const uint32_t *>(c->h_grp_out + L.start);
    c->h_grp_status.assign(status, status + nframes);
    c->h_grp_ngrouped.assign(ngrouped, ngrouped + nframes);
    c->h_grp_start.assign(start, start + nframes);
    c->h_grp_over.clear();
    for (uint32_t f = 0; f < nframes; f++) best[f] = ht_grp_record_to_rect(records + (size_t)f * HT_GRP_REC_F64);
    double sx[HT_MAX_LEVELS];
    bool have_sx = false;
    std::vector<ht_hit> fh;
    for (uint32_t f = 0; f < nframes; f++) {
        if (!(status[f] & HT_GRP_ST_OVER_CAP)) continue;
        const uint32_t n = count[f];
        if ((uint64_t)start[f] + n > c->hit_capacity) return ht_fail(c, HT_ERR_HIP, std::string(fn) + ": inconsistent bucket table");
        if (!have_sx) ht_post_level_scales(grp_cfg(c), sx), have_sx = true;
        if (c->h_grp_over.empty()) c->h_grp_over.resize(nframes);
        fh.resize(n);
        HT_HIP(c, hipMemcpy(fh.data(), c->d_grp_hits2 + start[f], (size_t)n * sizeof(ht_hit), hipMemcpyDeviceToHost));
        std::vector<ht_rect> &g = c->h_grp_over[f];
        g.resize(n);
        uint32_t ng = 0;
        const ht_status st = ht_grp_complete_frame(grp_cfg(c), sx, fh.data(), n, min_neighbors, &best[f], g.data(), &ng);
        if (st != HT_OK) return ht_fail(c, st, std::string(fn) + ": host completion of a frame over the cap failed");
        g.resize(ng);
        c->h_grp_ngrouped[f] = ng;
        c->grp_over_cap_frames++;
        double rec[HT_GRP_REC_F64];
        ht_grp_rect_to_record(best[f], (double)(frame_base + (int32_t)f), rec);
        HT_HIP(c, hipMemcpy(c->d_grp_out + L.records + (size_t)f * sizeof(rec), rec, sizeof(rec), hipMemcpyHostToDevice));
        if (!lists_to_device) continue;
        // ... and so is its grouped list, for ht_camshift_init_faces: ng <= n rects into the frame's own bucket, the count next to them
        if (ng) HT_HIP(c, hipMemcpy(c->d_grp_rects + start[f], g.data(), (size_t)ng * sizeof(ht_rect), hipMemcpyHostToDevice));
        HT_HIP(c, hipMemcpy(c->d_grp_out + L.ngrouped + (size_t)f * sizeof(uint32_t), &ng, sizeof(ng), hipMemcpyHostToDevice));
    }
    return HT_OK;
}

ht_status grp_collect(ht_ctx *c, ht_rect *best, uint32_t *total_hits, int64_t next_flags, const char *fn) {
    if (!c || !best) return HT_ERR_INVALID;
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": nothing enqueued");
    if (!c->grp_enqueued) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": call ht_detect_best_enqueue behind ht_detect_enqueue first");
    HT_HIP(c, hipSetDevice(c->device));
    const uint32_t nfr = (uint32_t)c->grp_nframes;
    const HtGrpLayout L = ht_grp_layout(nfr);
    // nhits, records, status words and bucket tables in ONE pinned copy (+ the whitebalance sums of this batch): ht_detect_collect's head
    ht_status st = ht_detect_fetch(c, c->h_grp_out, c->d_grp_out, L.bytes);
    if (st != HT_OK) return st;
    const HtGrpHead head = *reinterpret_cast<const HtGrpHead *>(c->h_grp_out);
    c->grp_enqueued = false;
    c->h_counters = HtCounters{head.nhits, 0, 0, 0};
    c->spec_hint = head.nhits;
    if (total_hits) *total_hits = head.nhits;
    const int32_t mn = c->grp_min_neighbors, fb = c->grp_frame_base;
    if (head.nhits > c->hit_capacity) st = ht_fail(c, HT_ERR_CAPACITY, std::string(fn) + ": more raw hits than ht_config.hit_capacity; results incomplete");
    else if (head.bad) st = ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": a raw hit's frame or scale is out of range");
    else if ((st = grp_take_results(c, nfr, mn, fb, best, fn, true)) == HT_OK) c->grp_valid = true;
    if (st != HT_OK) return st;
    if (next_flags >= 0) {  // the next batch of the bound frames and its grouping, right behind the synchronisation
        if ((st = ht_detect_enqueue(c, (uint32_t)next_flags)) != HT_OK) return st;
        return ht_detect_best_enqueue(c, mn, fb);
    }
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_detect_best_enqueue(ht_ctx *c, int32_t min_neighbors, int32_t frame_base) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_detect_best_enqueue");
    if (!c->enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_best_enqueue: no detect batch in flight (call ht_detect_enqueue first)");
    if (c->enq_nframes <= 0) return ht_fail(c, HT_ERR_STATE, "ht_detect_best_enqueue: the batch in flight has no frames");
    HT_HIP(c, hipSetDevice(c->device));
    const uint32_t nfr = (uint32_t)c->enq_nframes;
    ht_status st = grp_reserve(c, nfr);
    if (st != HT_OK) return st;
    c->grp_valid = false;  // the buffers of the batch collected before are about to be overwritten
    c->grp_enqueued = false;
    if ((st = grp_launch(c, c->d_hits, &c->d_counters->nhits, nfr, min_neighbors, frame_base)) != HT_OK) return st;
    c->grp_enqueued = true;
    c->grp_nframes = (int)nfr, c->grp_min_neighbors = min_neighbors, c->grp_frame_base = frame_base;
    return HT_OK;
}

extern "C" ht_status ht_detect_best_collect(ht_ctx *c, ht_rect *best, uint32_t *total_hits) {
    HtRange range("ht_detect_best_collect");
    return grp_collect(c, best, total_hits, -1, "ht_detect_best_collect");
}

extern "C" ht_status ht_detect_best_collect_requeue(ht_ctx *c, ht_rect *best, uint32_t *total_hits, uint32_t next_flags) {
    HtRange range("ht_detect_best_collect_requeue");
    return grp_collect(c, best, total_hits, (int64_t)next_flags, "ht_detect_best_collect_requeue");
}

extern "C" ht_status ht_detect_grouped(ht_ctx *c, int32_t frame, ht_rect *out, uint32_t cap, uint32_t *n) {
    if (!c || !n) return HT_ERR_INVALID;
    *n = 0;
    if (!c->grp_valid) return ht_fail(c, HT_ERR_STATE, "ht_detect_grouped: no device-grouped batch (collected, and not yet followed by another ht_detect_best_enqueue)");
    if (frame < 0 || frame >= c->grp_nframes) return ht_fail(c, HT_ERR_INVALID, "ht_detect_grouped: frame outside the collected batch");
    const uint32_t ng = c->h_grp_ngrouped[(size_t)frame], ncopy = std::min(ng, cap);
    *n = ng;
    if (ncopy && !out) return ht_fail(c, HT_ERR_INVALID, "ht_detect_grouped: out is NULL");
    if (ncopy) {
        if (!c->h_grp_over.empty() && (c->h_grp_status[(size_t)frame] & HT_GRP_ST_OVER_CAP)) {
            std::memcpy(out, c->h_grp_over[(size_t)frame].data(), (size_t)ncopy * sizeof(ht_rect));
        } else {
            if ((uint64_t)c->h_grp_start[(size_t)frame] + ng > c->hit_capacity) return ht_fail(c, HT_ERR_HIP, "ht_detect_grouped: inconsistent bucket table");
            HT_HIP(c, hipSetDevice(c->device));
            // complete since the collect call's synchronisation, and nothing has written the buffer since (grp_valid)
            HT_HIP(c, hipMemcpy(out, c->d_grp_rects + c->h_grp_start[(size_t)frame], (size_t)ncopy * sizeof(ht_rect), hipMemcpyDeviceToHost));
        }
    }
    if (ng > cap) return ht_fail(c, HT_ERR_CAPACITY, "ht_detect_grouped: caller buffer too small for the frame's list");
    return HT_OK;
}

extern "C" ht_status ht_detect_best_records_device(ht_ctx *c, const void **records, int32_t *nframes) {
    if (!c || !records || !nframes) return HT_ERR_INVALID;
    *records = nullptr, *nframes = 0;
    if (!c->grp_valid && !c->grp_enqueued) return ht_fail(c, HT_ERR_STATE, "ht_detect_best_records_device: no device-grouped batch");
    *records = c->d_grp_out + ht_grp_layout((uint32_t)c->grp_nframes).records;
    *nframes = c->grp_nframes;
    return HT_OK;
}

extern "C" ht_status ht_group_hits(ht_ctx *c, const ht_hit *hits, uint32_t n, int32_t nframes, int32_t min_neighbors, ht_rect *best, ht_rect *grouped,
                                   uint32_t *ngrouped) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_group_hits");
    const char *why = nullptr;
    const ht_status chk = ht_grp_check_hits(hits, n, nframes, c->hit_capacity, best, grouped, ngrouped, &why);
    if (chk != HT_OK) return ht_fail(c, chk, std::string("ht_group_hits: ") + why);
    if (c->grp_enqueued) return ht_fail(c, HT_ERR_STATE, "ht_group_hits: a device-grouped batch is in flight; collect it first");
    HT_HIP(c, hipSetDevice(c->device));
    const uint32_t nfr = (uint32_t)nframes;
    ht_status st = grp_reserve(c, nfr);
    if (st == HT_OK) st = grp_grow(c, c->d_grp_in, c->grp_in_cap, (size_t)std::max<uint32_t>(n, 1u), "ht_group_hits: hipMalloc failed (hit list)");
    if (st != HT_OK) return st;
    c->grp_valid = false;
    if (n) HT_HIP(c, hipMemcpyAsync(c->d_grp_in, hits, (size_t)n * sizeof(ht_hit), hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(grp_nword(c)), (int)n, 1, c->stream));
    if ((st = grp_launch(c, c->d_grp_in, grp_nword(c), nfr, min_neighbors, 0)) != HT_OK) return st;
    const HtGrpLayout L = ht_grp_layout(nfr);
    HT_HIP(c, hipMemcpyAsync(c->h_grp_out, c->d_grp_out, L.bytes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    const HtGrpHead head = *reinterpret_cast<const HtGrpHead *>(c->h_grp_out);
    if ((st = grp_take_results(c, nfr, min_neighbors, 0, best, "ht_group_hits", false)) != HT_OK) return st;
    if (grouped) {  // the frames' lists back to back in frame order
        size_t k = 0;
        for (uint32_t f = 0; f < nfr; f++) {
            const uint32_t ng = c->h_grp_ngrouped[f];
            ngrouped[f] = ng;
            if (!ng) continue;
            if (k + ng > n) return ht_fail(c, HT_ERR_HIP, "ht_group_hits: inconsistent group counts");
            if (!c->h_grp_over.empty() && (c->h_grp_status[f] & HT_GRP_ST_OVER_CAP)) std::memcpy(grouped + k, c->h_grp_over[f].data(), (size_t)ng * sizeof(ht_rect));
            else HT_HIP(c, hipMemcpy(grouped + k, c->d_grp_rects + c->h_grp_start[f], (size_t)ng * sizeof(ht_rect), hipMemcpyDeviceToHost));
            k += ng;
        }
    }
    if (head.bad) return ht_fail(c, HT_ERR_INVALID, "ht_group_hits: a hit's frame or scale is out of range (skipped)");
    return HT_OK;
}

void ht_group_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_grp_hits2) (void)hipFree(c->d_grp_hits2);
    if (c->d_grp_rects) (void)hipFree(c->d_grp_rects);
    if (c->d_grp_out) (void)hipFree(c->d_grp_out);
    if (c->h_grp_out) (void)hipHostFree(c->h_grp_out);
    if (c->d_grp_cursor) (void)hipFree(c->d_grp_cursor);
    if (c->d_grp_konst) (void)hipFree(c->d_grp_konst);
    if (c->d_grp_in) (void)hipFree(c->d_grp_in);
    c->d_grp_hits2 = nullptr, c->d_grp_rects = nullptr, c->d_grp_out = nullptr, c->h_grp_out = nullptr, c->d_grp_cursor = nullptr;
    c->d_grp_konst = nullptr, c->d_grp_in = nullptr;
    c->grp_out_cap = c->h_grp_out_cap = c->grp_cursor_cap = c->grp_in_cap = 0;
    c->grp_enqueued = c->grp_valid = false;
}

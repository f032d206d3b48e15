// ht_cs_faces.hip — a tracker per grouped face, straight from the device's grouped lists (ht_camshift_init_faces / _result).
//
// ht_camshift_init_best hands ONE face per frame to ONE tracker.  Here every pair of the call that names a frame is one of that frame's
// slots, and the frame's grouped list (k_grp_frames: d_grp_rects with the start / ngrouped tables) is dealt to the slots by the rule of
// ht_cs_faces_plan.h — by confidence rank, or, under HT_CSF_ASSOCIATE, so that a tracker whose search window overlaps a detection keeps
// its slot:
//
//   k_csf_resolve   one wavefront per distinct frame of the call.  Selection: at most 16 rounds of a wave-wide arg-max on (confidence,
//                   -index) over the frame's list, the lanes striding over it (nothing is sorted).  Association: the at most 16 x 16
//                   int64 overlaps of the slots' search windows (HtCsState.sw) with the faces' floored rects in LDS, arg-max rounds over
//                   that table, four entries per lane.  The rect and the skip flag go into each slot's CspEntry, the 32-byte records into
//                   the result array (copied to a pinned twin behind the call's kernels).
//   k_csp_init, or k_csp_zero_models + k_csp_init_rows: the pair unit's init kernels on that table, planned as ht_camshift_init_best
//                   plans them (the frame height as the tallest possible rect).
//
// The kernel reads the search windows in front of the init kernels of its own call, in stream order: the windows the last enqueued init
// or track step left.  Plain C++, ordinary vector stores, no atomics.
//
// Compiled as part of ht_backproject.hip's code object: included at the end of ht_cs_pairs.hip, behind ht_cs_best.hip.
#include "ht_cs_faces_plan.h"

namespace {

constexpr int CSF_NT = 64;  // one wavefront
constexpr int CSF_K = HT_CSF_MAX_SLOTS;
static_assert(CSF_K * CSF_K == 4 * CSF_NT, "k_csf_resolve: four table entries per lane");

// the wave's best (confidence, index) by ht_csf_face_before; idx < 0: none
__device__ __forceinline__ void csf_wave_best_face(double &c, int32_t &idx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double oc = __shfl_xor(c, d, 64);
        const int32_t oi = __shfl_xor(idx, d, 64);
        if (oi >= 0 && (idx < 0 || ht_csf_face_before(oc, oi, c, idx))) c = oc, idx = oi;
    }
}

// the wave's best (overlap, table position) by ht_csf_match_before; e < 0: none
__device__ __forceinline__ void csf_wave_best_match(long long &o, int32_t &e) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long oo = __shfl_xor(o, d, 64);
        const int32_t oe = __shfl_xor(e, d, 64);
        if (oe >= 0 && (e < 0 || ht_csf_match_before((int64_t)oo, oe, (int64_t)o, e))) o = oo, e = oe;
    }
}

__global__ __launch_bounds__(CSF_NT) void k_csf_resolve(CspEntry *__restrict__ entries, const int32_t *__restrict__ groups, const int32_t *__restrict__ order,
                                                        const ht_rect *__restrict__ rects, const uint32_t *__restrict__ start, const uint32_t *__restrict__ ngrouped,
                                                        const uint32_t *__restrict__ count, const uint32_t *__restrict__ status, const HtGrpHead *__restrict__ head,
                                                        uint32_t hit_capacity, int collected, double min_confidence, uint32_t flags,
                                                        const HtCsState *__restrict__ states, ht_csf_record *__restrict__ out) {
    __shared__ long long s_ov[CSF_K * CSF_K];  // overlap of slot j's window with the face of rank r at [j * 16 + r]
    __shared__ ht_cs_rect s_rect[CSF_K];       // the kept faces' floored rects, by rank
    __shared__ int32_t s_face[CSF_K];          // ... and their indices in the frame's list
    __shared__ int32_t s_sw[CSF_K][4];         // the slots' search windows
    __shared__ int32_t s_rank[CSF_K];          // slot -> rank of its face, or -1

    const int lane = threadIdx.x;
    const int32_t f = groups[3 * blockIdx.x], first = groups[3 * blockIdx.x + 1];
    const int32_t k = min(groups[3 * blockIdx.x + 2], CSF_K);  // (the plan refuses more)
    const int32_t pi = lane < k ? order[first + lane] : 0;     // lane j < k owns slot j = pair pi of the call
    const ht_cs_rect zero = {0, 0, 0, 0};

    if (ht_csf_not_final(status[f], head->nhits, head->bad, hit_capacity, collected != 0)) {  // wave-uniform
        if (lane < k) {
            entries[pi].pad |= HT_CSB_F_SKIP;
            entries[pi].rect = zero;
            out[pi] = ht_csf_make_record(HT_CSB_DEFERRED, -1, zero, 0);
        }
        return;
    }
    // the frame's list: inside its bucket of the rect buffer whatever the tables say
    const uint32_t beg = start[f];
    uint32_t m = min(ngrouped[f], count[f]);
    if (beg > hit_capacity || m > hit_capacity - beg) m = 0;
    const ht_rect *G = rects + beg;

    if (lane < k) {
        const int4 w = *reinterpret_cast<const int4 *>(states[entries[pi].stream].sw);
        s_sw[lane][0] = w.x, s_sw[lane][1] = w.y, s_sw[lane][2] = w.z, s_sw[lane][3] = w.w;
        s_rank[lane] = -1;
    }
    // ---- selection: round q takes the first eligible face behind the one of round q - 1 -------------------------------------------------
    // (the first 64 faces stay in registers, one per lane: a frame rarely has more, and the rounds then read no memory)
    const double c0 = (uint32_t)lane < m ? G[lane].confidence : 0.0;
    const bool e0 = (uint32_t)lane < m && ht_csf_eligible(c0, G[lane].neighbors, min_confidence);
    int32_t eligible = e0 ? 1 : 0;
    for (uint32_t i = lane + CSF_NT; i < m; i += CSF_NT) eligible += ht_csf_eligible(G[i].confidence, G[i].neighbors, min_confidence) ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) eligible += __shfl_xor(eligible, d, 64);
    int32_t q = 0, prev_i = -1;
    double prev_c = 0.0;
    for (; q < k; q++) {
        double bc = 0.0;
        int32_t bi = -1;
        if (e0 && (prev_i < 0 || ht_csf_face_before(prev_c, prev_i, c0, lane))) bc = c0, bi = lane;
        for (uint32_t i = lane + CSF_NT; i < m; i += CSF_NT) {
            const double ci = G[i].confidence;
            if (!ht_csf_eligible(ci, G[i].neighbors, min_confidence)) continue;
            if (prev_i >= 0 && !ht_csf_face_before(prev_c, prev_i, ci, (int32_t)i)) continue;
            if (bi < 0 || ht_csf_face_before(ci, (int32_t)i, bc, bi)) bc = ci, bi = (int32_t)i;
        }
        csf_wave_best_face(bc, bi);
        if (bi < 0) break;  // wave-uniform: every lane holds the same result
        if (lane == 0) {
            const ht_rect g = G[bi];
            s_face[q] = bi, s_rect[q] = ht_csf_rect(g.x, g.y, g.width, g.height);
        }
        prev_c = bc, prev_i = bi;
    }
    const int32_t dropped = eligible - q;
    __syncthreads();

    if (flags & HT_CSF_ASSOCIATE) {
        // ---- association: the overlap table, then arg-max rounds over it --------------------------------------------------------------
        const unsigned long long lb = __ballot(lane < k && ht_csf_live(s_sw[lane < k ? lane : 0]));
        const uint32_t live = (uint32_t)lb;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int e = lane * 4 + t, j = e / CSF_K, r = e % CSF_K;
            s_ov[e] = (j < k && r < q && ((live >> j) & 1u)) ? (long long)ht_csf_overlap(s_sw[j], s_rect[r]) : 0ll;
        }
        __syncthreads();
        uint32_t slot_taken = 0, face_taken = 0;
        for (int32_t round = 0; round < k; round++) {
            long long bo = 0;
            int32_t be = -1;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int e = lane * 4 + t, j = e / CSF_K, r = e % CSF_K;
                const long long o = s_ov[e];
                if (o <= 0 || ((slot_taken >> j) & 1u) || ((face_taken >> r) & 1u)) continue;
                if (be < 0 || ht_csf_match_before((int64_t)o, e, (int64_t)bo, be)) bo = o, be = e;
            }
            csf_wave_best_match(bo, be);
            if (be < 0) break;  // wave-uniform
            if (lane == 0) s_rank[be / CSF_K] = be % CSF_K;
            slot_taken |= 1u << (be / CSF_K), face_taken |= 1u << (be % CSF_K);
        }
        __syncthreads();
        if (lane == 0) ht_csf_fill(k, q, live, face_taken, s_rank);
    } else if (lane < q) {
        s_rank[lane] = lane;
    }
    __syncthreads();

    if (lane < k) {
        const int32_t r = s_rank[lane];
        const ht_cs_rect rc = r >= 0 ? s_rect[r] : zero;
        const int32_t pad = entries[pi].pad;
        entries[pi].pad = r >= 0 ? (pad & ~HT_CSB_F_SKIP) : (pad | HT_CSB_F_SKIP);
        entries[pi].rect = rc;
        out[pi] = ht_csf_make_record(r >= 0 ? HT_CSB_FACE : HT_CSB_UNTOUCHED, r >= 0 ? s_face[r] : -1, rc, dropped);
    }
}

// the result buffers hold >= n records; allocates (and then waits for the stream) only on first use or after a larger reservation
ht_status csf_reserve(ht_ctx *c, int32_t n) {
    if (c->csf_cap >= (size_t)n && c->ev_csf) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_csf_res) (void)hipFree(c->d_csf_res);
    if (c->h_csf_res) (void)hipHostFree(c->h_csf_res);
    c->d_csf_res = c->h_csf_res = nullptr, c->csf_cap = 0, c->csf_n = 0;
    const size_t cap = (size_t)std::max(n, c->cs_streams), bytes = cap * sizeof(ht_csf_record);
    bool ok = hipMalloc(reinterpret_cast<void **>(&c->d_csf_res), bytes) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&c->h_csf_res), bytes, hipHostMallocDefault) == hipSuccess;
    if (ok && !c->ev_csf) ok = hipEventCreateWithFlags(&c->ev_csf, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (c->d_csf_res) (void)hipFree(c->d_csf_res);
        if (c->h_csf_res) (void)hipHostFree(c->h_csf_res);
        c->d_csf_res = c->h_csf_res = nullptr;
        return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_init_faces: allocation of the result buffers failed");
    }
    c->csf_cap = cap;
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_init_faces(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, double min_confidence, uint32_t flags) {
    HtRange range("ht_camshift_init_faces");
    const char *fn = "ht_camshift_init_faces";
    if (!c || !pairs) return HT_ERR_INVALID;
    if (!c->grp_enqueued && !c->grp_valid)
        return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_faces: no device-grouped batch (ht_detect_best_enqueue in flight, or collected and not yet overwritten)");
    CspPlan plan;
    ht_status st = csp_plan(c, fn, pairs, n, nullptr, &plan);  // the rules of ht_camshift_init_pairs, and the table of the init kernels
    if (st != HT_OK) return st;
    HtCsfPlan fp;
    std::string why;
    if (ht_csf_plan(pairs, n, c->grp_nframes, min_confidence, flags, &fp, &why) != HT_OK) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": " + why);
    HT_HIP(c, hipSetDevice(c->device));
    if ((st = csf_reserve(c, n)) != HT_OK) return st;
    std::vector<int32_t> extra(fp.groups);
    extra.insert(extra.end(), fp.order.begin(), fp.order.end());
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr, *d_extra = nullptr;
    if ((st = csp_upload(c, fn, plan, &d_entries, &d_flist, extra.data(), extra.size(), &d_extra)) != HT_OK) return st;
    c->csf_n = 0;  // until this call's copy is behind its kernels
    const HtGrpLayout L = ht_grp_layout((uint32_t)c->grp_nframes);
    ht_csf_record *d_out = reinterpret_cast<ht_csf_record *>(c->d_csf_res);
    {
        HtProfScope ps(c, "csf_resolve");
        hipLaunchKernelGGL(k_csf_resolve, dim3((uint32_t)fp.ngroups()), dim3(CSF_NT), 0, c->stream, const_cast<CspEntry *>(d_entries), d_extra, d_extra + fp.groups.size(),
                           c->d_grp_rects, reinterpret_cast<const uint32_t *>(c->d_grp_out + L.start), reinterpret_cast<const uint32_t *>(c->d_grp_out + L.ngrouped),
                           reinterpret_cast<const uint32_t *>(c->d_grp_out + L.count), reinterpret_cast<const uint32_t *>(c->d_grp_out + L.status),
                           reinterpret_cast<const HtGrpHead *>(c->d_grp_out), c->hit_capacity, c->grp_enqueued ? 0 : 1, min_confidence, flags, c->d_cs, d_out);
        HT_HIP(c, hipGetLastError());
    }
    const HtCsInitPlan ip = ht_cs_plan_init_pairs(c->cs_pairs_cluster, n, c->H, c->num_cus);  // the frame height: the tallest possible rect
    if (ip.rows) {
        HtProfScope ps(c, "csp_init_rows");
        hipLaunchKernelGGL(k_csp_zero_models, dim3(n), dim3(1024), 0, c->stream, d_entries, c->d_cs);
        hipLaunchKernelGGL(k_csp_init_rows, dim3(ip.G, n), dim3(CS_INIT_ROWS_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_entries, c->d_cs);
        HT_HIP(c, hipGetLastError());
    } else {
        HtProfScope ps(c, "csp_init");
        hipLaunchKernelGGL(k_csp_init, dim3(n), dim3(INIT_NT), 0, c->stream, c->d_frames, c->frame_stride, c->W, c->H, d_entries, c->d_cs);
        HT_HIP(c, hipGetLastError());
    }
    // the records -> the pinned twin with one copy; the event behind it is all ht_camshift_init_faces_result waits for
    HT_HIP(c, hipMemcpyAsync(c->h_csf_res, c->d_csf_res, (size_t)n * sizeof(ht_csf_record), hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_csf, c->stream));
    c->csf_n = n, c->csf_states = c->d_cs;
    return HT_OK;
}

extern "C" ht_status ht_camshift_init_faces_result(ht_ctx *c, int32_t n, ht_csf_record *out) {
    if (!c || !out) return HT_ERR_INVALID;
    if (c->csf_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_faces_result: no ht_camshift_init_faces to report on");
    if (c->csf_states != c->d_cs) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_faces_result: ht_camshift_reserve has replaced the trackers since");
    if (n != c->csf_n) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_faces_result: n differs from the last ht_camshift_init_faces");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventSynchronize(c->ev_csf));
    std::memcpy(out, c->h_csf_res, (size_t)n * sizeof(ht_csf_record));
    return HT_OK;
}

void ht_cs_faces_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_csf_res) (void)hipFree(c->d_csf_res);
    if (c->h_csf_res) (void)hipHostFree(c->h_csf_res);
    if (c->ev_csf) (void)hipEventDestroy(c->ev_csf);
    c->d_csf_res = c->h_csf_res = nullptr, c->ev_csf = nullptr, c->csf_cap = 0, c->csf_n = 0, c->csf_states = nullptr;
}

// ht_cs_best.hip — initTracker straight from the device's best-face records (ht_camshift_init_best / ht_camshift_init_best_result).
//
// ht_detect_best_enqueue leaves one 64-byte record per frame on the device, ht_camshift_init_pairs initialises any stream on any bound
// frame from a device table; the step between them in the reference (facetrackr.js:97-107: `confidence > threshold`, floor the rect,
// initTracker) is two comparisons and four floors on values the device already holds.  Here it runs there:
//
//   k_csb_resolve   one launch, one thread per pair: the pair's table entry, its frame's record, status word and the batch head ->
//                   the decision of ht_cs_best_plan.h; the rect and a skip flag go into the pair's CspEntry, code and rect into the
//                   result array (copied to a pinned twin behind the call's kernels)
//   k_csp_init, or k_csp_zero_models + k_csp_init_rows: ht_cs_pairs.hip's init kernels on that table.  A workgroup whose entry is
//                   flagged skip returns before it touches model or state (CS_INIT_SKIP).
//
// The rect is unknown on the host, so the row form (option cs_pairs_cluster=1, < 64 pairs) is planned for the frame height as the
// tallest possible rect; it is correct for any G — workgroups without rows add nothing — and the model is the same bits in both forms.
//
// Compiled as part of ht_backproject.hip's code object: included at the end of ht_cs_pairs.hip, behind ht_group.hip; it shares their
// anonymous namespace.
namespace {

static_assert(HT_CSB_ST_OVER_CAP == (uint32_t)HT_GRP_ST_OVER_CAP, "ht_cs_best_plan.h: status bit");
constexpr int CSB_NT = 256;

__global__ __launch_bounds__(CSB_NT) void k_csb_resolve(CspEntry *__restrict__ entries, int n, const double *__restrict__ records, const uint32_t *__restrict__ status,
                                                        const HtGrpHead *__restrict__ head, uint32_t hit_capacity, int collected, double min_confidence,
                                                        int32_t *__restrict__ codes, ht_cs_rect *__restrict__ rects) {
    const uint32_t nhits = head->nhits, bad = head->bad;
    for (int i = threadIdx.x; i < n; i += CSB_NT) {
        const int4 e = reinterpret_cast<const int4 *>(entries + i)[0];  // stream, frame, slot, flags
        const ht_cs_rect fb = entries[i].rect;
        const double2 *r2 = reinterpret_cast<const double2 *>(records + (size_t)e.y * HT_GRP_REC_F64);
        const double2 a = r2[0], b = r2[1], cn = r2[2];
        const double rec[6] = {a.x, a.y, b.x, b.y, cn.x, cn.y};
        ht_cs_rect r;
        const int32_t code = ht_csb_decide(rec, status[e.y], nhits, bad, hit_capacity, collected != 0, min_confidence, (e.w & HT_CSB_F_HAS_FALLBACK) != 0, fb, &r);
        const bool init = code == HT_CSB_FACE || code == HT_CSB_FALLBACK;
        entries[i].pad = (e.w & ~HT_CSB_F_SKIP) | (init ? 0 : HT_CSB_F_SKIP);
        entries[i].rect = r;
        codes[i] = code;
        rects[i] = r;
    }
}

// the result buffers hold >= n pairs; allocates (and then waits for the stream) only on first use or after a larger reservation
ht_status csb_reserve(ht_ctx *c, int32_t n) {
    if (c->csb_cap >= (size_t)n && c->ev_csb) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    if (c->d_csb_res) (void)hipFree(c->d_csb_res);
    if (c->h_csb_res) (void)hipHostFree(c->h_csb_res);
    c->d_csb_res = c->h_csb_res = nullptr, c->csb_cap = 0, c->csb_n = 0;
    const size_t cap = (size_t)std::max(n, c->cs_streams), bytes = cap * 5 * sizeof(int32_t);
    bool ok = hipMalloc(reinterpret_cast<void **>(&c->d_csb_res), bytes) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&c->h_csb_res), bytes, hipHostMallocDefault) == hipSuccess;
    if (ok && !c->ev_csb) ok = hipEventCreateWithFlags(&c->ev_csb, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (c->d_csb_res) (void)hipFree(c->d_csb_res);
        if (c->h_csb_res) (void)hipHostFree(c->h_csb_res);
        c->d_csb_res = c->h_csb_res = nullptr;
        return ht_fail(c, HT_ERR_NOMEM, "ht_camshift_init_best: allocation of the result buffers failed");
    }
    c->csb_cap = cap;
    return HT_OK;
}

}  // namespace

extern "C" ht_status ht_camshift_init_best(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, double min_confidence, const ht_cs_rect *fallback) {
    HtRange range("ht_camshift_init_best");
    const char *fn = "ht_camshift_init_best";
    if (!c || !pairs) return HT_ERR_INVALID;
    if (!c->grp_enqueued && !c->grp_valid)
        return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_best: no device-grouped batch (ht_detect_best_enqueue in flight, or collected and not yet overwritten)");
    if (min_confidence != min_confidence) return ht_fail(c, HT_ERR_INVALID, "ht_camshift_init_best: min_confidence is NaN");
    CspPlan plan;
    ht_status st = csp_plan(c, fn, pairs, n, fallback, &plan);
    if (st != HT_OK) return st;
    for (int32_t i = 0; i < n; i++)
        if (pairs[i].frame >= c->grp_nframes)
            return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": frame " + std::to_string(pairs[i].frame) + " is outside the device-grouped batch");
    if (fallback)
        for (CspEntry &e : plan.entries) e.pad = HT_CSB_F_HAS_FALLBACK;
    HT_HIP(c, hipSetDevice(c->device));
    if ((st = csb_reserve(c, n)) != HT_OK) return st;
    const CspEntry *d_entries = nullptr;
    const int32_t *d_flist = nullptr;
    if ((st = csp_upload(c, fn, plan, &d_entries, &d_flist)) != HT_OK) return st;
    c->csb_n = 0;  // until this call's copy is behind its kernels
    const HtGrpLayout L = ht_grp_layout((uint32_t)c->grp_nframes);
    int32_t *d_codes = c->d_csb_res;
    ht_cs_rect *d_rects = reinterpret_cast<ht_cs_rect *>(c->d_csb_res + n);
    {
        HtProfScope ps(c, "csb_resolve");
        hipLaunchKernelGGL(k_csb_resolve, dim3(1), dim3(CSB_NT), 0, c->stream, const_cast<CspEntry *>(d_entries), (int)n,
                           reinterpret_cast<const double *>(c->d_grp_out + L.records), reinterpret_cast<const uint32_t *>(c->d_grp_out + L.status),
                           reinterpret_cast<const HtGrpHead *>(c->d_grp_out), c->hit_capacity, c->grp_enqueued ? 0 : 1, min_confidence, d_codes, d_rects);
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
    // codes and rects -> the pinned twin with one copy; the event behind it is all ht_camshift_init_best_result waits for
    HT_HIP(c, hipMemcpyAsync(c->h_csb_res, c->d_csb_res, (size_t)n * 5 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipEventRecord(c->ev_csb, c->stream));
    c->csb_n = n, c->csb_states = c->d_cs;
    return HT_OK;
}

extern "C" ht_status ht_camshift_init_best_result(ht_ctx *c, int32_t n, int32_t *codes, ht_cs_rect *rects) {
    if (!c) return HT_ERR_INVALID;
    if (c->csb_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_best_result: no ht_camshift_init_best to report on");
    if (c->csb_states != c->d_cs) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_best_result: ht_camshift_reserve has replaced the trackers since");
    if (n != c->csb_n) return ht_fail(c, HT_ERR_STATE, "ht_camshift_init_best_result: n differs from the last ht_camshift_init_best");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventSynchronize(c->ev_csb));
    if (codes) std::memcpy(codes, c->h_csb_res, (size_t)n * sizeof(int32_t));
    if (rects) std::memcpy(rects, c->h_csb_res + n, (size_t)n * sizeof(ht_cs_rect));
    return HT_OK;
}

void ht_cs_best_free(ht_ctx *c) {  // ht_destroy (the stream has been synchronised)
    if (c->d_csb_res) (void)hipFree(c->d_csb_res);
    if (c->h_csb_res) (void)hipHostFree(c->h_csb_res);
    if (c->ev_csb) (void)hipEventDestroy(c->ev_csb);
    c->d_csb_res = c->h_csb_res = nullptr, c->ev_csb = nullptr, c->csb_cap = 0, c->csb_n = 0, c->csb_states = nullptr;
}

// ht_face_calls.hip — the host path of the face-patch calls, written once: the crop family (ht_crop.hip) and the align family (ht_align.hip),
// each in its plain (RGBA8), tensor (ht_patch.hip) and filtered (ht_filter.hip) form, from a pairs list or a sources list, with the result
// and records-device calls.  Included at the end of ht_ingest.hip, behind ht_filter.hip: every kernel's launcher is defined by then.
//
// A call: check (the context's state, the list, the params, the format, the output, then entry by entry), descriptors, the family's buffers
// (face_reserve), the table through the family's staged table (HtStagedTable, ht_internal.h), ONE kernel, the records to their pinned twin
// and the event ht_camshift_*_result waits for.  What differs between the two families is FaceFamily: the record's size, where the
// context keeps the family's buffers and last-call count, the three launchers with their profile-scope names, and one word of the messages.
// ht_align_params IS ht_crop_params (the same four fields at the same places): the host path takes the latter.
namespace {

static_assert(HT_ALIGN_SQUARE == HT_CROP_SQUARE && sizeof(ht_align_params) == sizeof(ht_crop_params) && offsetof(ht_align_params, out_width) == offsetof(ht_crop_params, out_width) &&
                  offsetof(ht_align_params, out_height) == offsetof(ht_crop_params, out_height) && offsetof(ht_align_params, margin_q8) == offsetof(ht_crop_params, margin_q8) &&
                  offsetof(ht_align_params, flags) == offsetof(ht_crop_params, flags),
              "align params are crop params");
const ht_crop_params *face_params(const ht_align_params *p) { return reinterpret_cast<const ht_crop_params *>(p); }

enum FaceForm { FACE_RGBA8 = 0, FACE_TENSOR = 1, FACE_FILTERED = 2 };  // a call's form: the index of its launcher

struct FaceFamily {
    const char *word;                       // the family's word in the messages
    size_t rec_bytes;                       // ht_crop_record / ht_align_record
    HtFaceCalls ht_ctx::*calls;             // the family's buffers and last-call count in the context
    void (*launch[3])(const FaceLaunch &);  // by FaceForm
    const char *scope[3];                   // ... and their profile scopes
};
const FaceFamily CROP = {"crop", sizeof(ht_crop_record), &ht_ctx::crop, {crop_launch_list, pt_launch_cut, fm_launch_cut}, {"crop_list", "cut_tensor", "cut_mean"}};
const FaceFamily ALIGN = {"align", sizeof(ht_align_record), &ht_ctx::align, {align_launch_list, pt_launch_upright, fm_launch_upright},
                          {"align_list", "upright_tensor", "upright_mean"}};

// the checks every call shares, in front of its entries: the context's state first, then the call's own arguments.  tensor: the output
// is fmt's tensor (ht_patch_plan.h) instead of RGBA8 — fmt is checked here and a patch's bytes and the default stride are the tensor's
ht_status face_check(ht_ctx *c, const std::string &f, bool pairs_form, const void *list, int32_t n, const ht_crop_params *p, const void *out_dev, size_t out_stride,
                     size_t *pbytes, size_t *ostride, bool tensor, const ht_patch_format *fmt) {
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, f + ": call ht_set_geometry first");
    if (c->cs_streams <= 0 || !c->d_cs) return ht_fail(c, HT_ERR_STATE, f + ": call ht_camshift_reserve first");
    if (pairs_form && (!c->d_frames || c->nframes <= 0)) return ht_fail(c, HT_ERR_STATE, f + ": bind frames first");
    if (!list || n <= 0 || n > HT_DRAW_LIST_MAX) return ht_fail(c, HT_ERR_INVALID, f + ": " + ht_draw_list_message(HT_DRAW_LIST_BAD_COUNT));
    if (!p) return ht_fail(c, HT_ERR_INVALID, f + ": NULL params");
    if (p->out_width < 1 || p->out_width > HT_CROP_MAX_OUT || p->out_height < 1 || p->out_height > HT_CROP_MAX_OUT)
        return ht_fail(c, HT_ERR_INVALID, f + ": out_width / out_height must be 1..1024");
    if (p->margin_q8 < HT_CROP_MIN_MARGIN || p->margin_q8 > HT_CROP_MAX_MARGIN) return ht_fail(c, HT_ERR_INVALID, f + ": margin_q8 must be 64..1024");
    if (p->flags & ~(uint32_t)HT_CROP_SQUARE) return ht_fail(c, HT_ERR_INVALID, f + ": unknown flag");
    if (tensor) {
        if (!fmt) return ht_fail(c, HT_ERR_INVALID, f + ": NULL format");
        const int fs = ht_patch_check_format(fmt);
        if (fs != HT_PATCH_FMT_OK) return ht_fail(c, HT_ERR_INVALID, f + ": format: " + ht_patch_format_message(fs));
    }
    if (!out_dev || ((uintptr_t)out_dev & 3)) return ht_fail(c, HT_ERR_INVALID, f + ": NULL or misaligned output (4-byte alignment required)");
    *pbytes = tensor ? ht_patch_bytes(p->out_width, p->out_height, fmt->dtype, fmt->channels) : (size_t)p->out_width * p->out_height * 4;
    *ostride = out_stride ? out_stride : ht_patch_default_stride(*pbytes);
    if ((*ostride & 3) || *ostride < *pbytes) return ht_fail(c, HT_ERR_INVALID, f + ": output stride smaller than a patch or not a multiple of 4");
    return HT_OK;
}

// the buffers of a call of n entries: the family's staged table and the records with their pinned twin, all for max(n, 64) entries.
// Allocates (and then waits for the stream) only on the first call or for a longer list.
ht_status face_reserve(ht_ctx *c, const FaceFamily &fam, const char *fn, size_t n) {
    HtFaceCalls &s = c->*fam.calls;
    if (s.rec_cap >= n && s.ev) return HT_OK;
    const std::string message = std::string(fn) + ": allocation of the " + fam.word + " table failed";
    s.n = 0;
    ht_status st = ht_stage_reserve(c, &s.tab, n * sizeof(HtCropDesc), 64 * sizeof(HtCropDesc), message);
    if (st != HT_OK) return st;
    HT_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cap = std::max(n, (size_t)64);
    if (s.d_rec) (void)hipFree(s.d_rec);
    if (s.h_rec) (void)hipHostFree(s.h_rec);
    s.d_rec = s.h_rec = nullptr, s.rec_cap = 0;
    bool ok = hipMalloc(reinterpret_cast<void **>(&s.d_rec), cap * fam.rec_bytes) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void **>(&s.h_rec), cap * fam.rec_bytes, hipHostMallocDefault) == hipSuccess;
    if (ok && !s.ev) ok = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, message);
    }
    s.rec_cap = cap;
    return HT_OK;
}

// everything has been checked: table, kernel, records to the pinned twin.  max_factor != 0: a filtered call; else fmt != nullptr: a tensor call
ht_status face_launch(ht_ctx *c, const FaceFamily &fam, const char *fn, const std::vector<HtCropDesc> &desc, const ht_crop_params &p, uint8_t *out, size_t ostride,
                      const ht_patch_format *fmt, int32_t max_factor) {
    HtFaceCalls &s = c->*fam.calls;
    const size_t n = desc.size(), need = n * sizeof(HtCropDesc);
    HT_HIP(c, hipSetDevice(c->device));
    ht_status st = face_reserve(c, fam, fn, n);
    if (st != HT_OK) return st;
    uint8_t *slot = nullptr;
    if ((st = ht_stage_take(c, &s.tab, &slot)) != HT_OK) return st;
    std::memcpy(slot, desc.data(), need);
    if ((st = ht_stage_commit(c, &s.tab, need)) != HT_OK) return st;
    s.n = 0;  // until this call's copy is behind its kernel
    const int form = max_factor ? FACE_FILTERED : fmt ? FACE_TENSOR : FACE_RGBA8;
    const dim3 grid((p.out_width + IG_TW - 1) / IG_TW, (p.out_height + IG_TH - 1) / IG_TH, (unsigned)n);
    {
        HtProfScope ps(c, fam.scope[form]);
        fam.launch[form](FaceLaunch{c, grid, reinterpret_cast<const CrDesc *>(s.tab.d), (const HtCsState *)c->d_cs, out, ostride, p, max_factor, fmt, s.d_rec});
        HT_HIP(c, hipGetLastError());
    }
    HT_HIP(c, hipMemcpyAsync(s.h_rec, s.d_rec, n * fam.rec_bytes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipEventRecord(s.ev, c->stream));
    s.n = (int)n;
    return HT_OK;
}

// what every form hands on behind its list.  max_factor is checked behind the context and in front of everything else of the call
struct FaceCall {
    const FaceFamily &fam;
    FaceForm form;
    const char *fn;  // the export's name
    const ht_crop_params *params;
    int32_t max_factor;  // FACE_FILTERED
    const ht_patch_format *fmt;  // FACE_TENSOR; FACE_FILTERED: nullptr is RGBA8
    void *out_dev;
    size_t out_stride;
    bool tensor() const { return form == FACE_TENSOR || (form == FACE_FILTERED && fmt); }
    ht_status enter(ht_ctx *c) const {
        if (!c) return HT_ERR_INVALID;
        if (form == FACE_FILTERED && (max_factor < HT_FILTER_MIN_FACTOR || max_factor > HT_FILTER_MAX_FACTOR))
            return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": max_factor must be 1..8");
        return HT_OK;
    }
    ht_status launch(ht_ctx *c, const std::vector<HtCropDesc> &desc, size_t ostride) const {
        return face_launch(c, fam, fn, desc, *params, static_cast<uint8_t *>(out_dev), ostride, form == FACE_RGBA8 ? nullptr : fmt, form == FACE_FILTERED ? max_factor : 0);
    }
};

// every pairs-form call
ht_status face_pairs(ht_ctx *c, const FaceCall &k, const ht_cs_pair *pairs, int32_t n) {
    ht_status st = k.enter(c);
    if (st != HT_OK) return st;
    HtRange range(k.fn);
    const std::string f(k.fn);
    size_t pbytes = 0, ostride = 0;
    st = face_check(c, f, true, pairs, n, k.params, k.out_dev, k.out_stride, &pbytes, &ostride, k.tensor(), k.fmt);
    if (st != HT_OK) return st;
    const size_t fbytes = (size_t)c->W * c->H * 4, total = (size_t)(n - 1) * ostride + pbytes;
    std::vector<HtCropDesc> desc((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const int32_t s = pairs[i].stream, fr = pairs[i].frame;
        if (s < 0 || s >= c->cs_streams) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": stream " + std::to_string(s) + " is not reserved");
        if (fr < 0 || fr >= c->nframes) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": frame " + std::to_string(fr) + " is not bound");
        const uint8_t *frame = c->d_frames + (size_t)fr * c->frame_stride;
        const HtDrawExtent bound = {{frame}, {fbytes}};
        if (ht_draw_list_overlap(&bound, 1, k.out_dev, total) >= 0)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": the bound frame and the output overlap");
        HtCropDesc e = {};
        e.d.p0 = frame, e.d.pitch0 = (size_t)c->W * 4, e.d.format = HT_DRAW_RGBA;
        e.d.sx = e.d.sy = 0, e.d.sw = c->W, e.d.sh = c->H;  // the canvas IS the source: drawn 1:1
        e.SW = c->W, e.SH = c->H, e.stream = s;
        desc[(size_t)i] = e;
    }
    return k.launch(c, desc, ostride);
}

// packed 4:2:2 and oriented (orient[i] != 0) entries become the RGBA entries of their upright frames: ht_draw_calls.hip, behind ht_draw_filter.hip's launcher
ht_status dm_unpack_sources(ht_ctx *c, const char *fn, std::vector<HtCropDesc> &desc, const int32_t *orient, bool packed_too);

// every sources-form call
ht_status face_sources(ht_ctx *c, const FaceCall &k, const int32_t *streams, const ht_draw_source *srcs, int32_t n) {
    ht_status st = k.enter(c);
    if (st != HT_OK) return st;
    HtRange range(k.fn);
    const std::string f(k.fn);
    size_t pbytes = 0, ostride = 0;
    st = face_check(c, f, false, srcs, n, k.params, k.out_dev, k.out_stride, &pbytes, &ostride, k.tensor(), k.fmt);
    if (st != HT_OK) return st;
    if (!streams) return ht_fail(c, HT_ERR_INVALID, f + ": NULL streams");
    std::vector<HtCropDesc> desc((size_t)n);
    std::vector<HtDrawExtent> ext((size_t)n);
    std::vector<int32_t> orient;  // filled only when an entry carries an orientation (ht_orient_plan.h)
    for (int32_t i = 0; i < n; i++) {
        if (streams[i] < 0 || streams[i] >= c->cs_streams)
            return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": stream " + std::to_string(streams[i]) + " is not reserved");
        HtCropDesc e = {};
        int ps;
        if (ht_orient_present(srcs[i].format)) {  // the stored planes, with the rect and the size of O: the frame the entry becomes below
            HtOrientDesc o;
            if ((ps = ht_orient_plan_entry(srcs[i], c->W, c->H, &o, &ext[(size_t)i])) == HT_DRAW_LIST_OK) {
                e.d = ht_orient_as_plain(o);
                ht_orient_size(o.orient, srcs[i].width, srcs[i].height, &e.SW, &e.SH);
                if (orient.empty()) orient.assign((size_t)n, 0);
                orient[(size_t)i] = o.orient;
            }
        } else {
            ps = ht_draw_list_plan_entry(srcs[i], c->W, c->H, &e.d, &ext[(size_t)i]);  // an entry's rules are the draw list's: asked, not restated
            e.SW = srcs[i].width, e.SH = srcs[i].height;
        }
        if (ps != HT_DRAW_LIST_OK) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(i) + ": " + ht_draw_list_message(ps));
        e.stream = streams[i];
        desc[(size_t)i] = e;
    }
    const int32_t bad = ht_draw_list_overlap(ext.data(), n, k.out_dev, (size_t)(n - 1) * ostride + pbytes);
    if (bad >= 0) return ht_fail(c, HT_ERR_INVALID, f + ": entry " + std::to_string(bad) + ": a source plane and the output overlap");
    // packed 4:2:2 entries become the RGBA entries of their unpacked frames, oriented entries those of their oriented frames
    // (ht_draw_calls.hip); a list without either is untouched
    if ((st = dm_unpack_sources(c, k.fn, desc, orient.empty() ? nullptr : orient.data(), true)) != HT_OK) return st;
    return k.launch(c, desc, ostride);
}

// ht_camshift_*_result: the records of the family's last call, once their copy has arrived
ht_status face_result(ht_ctx *c, const FaceFamily &fam, const char *fn, int32_t n, void *out) {
    if (!c) return HT_ERR_INVALID;
    HtFaceCalls &s = c->*fam.calls;
    const std::string f(fn);
    if (s.n <= 0) return ht_fail(c, HT_ERR_STATE, f + ": no " + fam.word + " call to report on");
    if (n != s.n) return ht_fail(c, HT_ERR_STATE, f + ": n differs from the last " + fam.word + " call");
    if (!out) return ht_fail(c, HT_ERR_INVALID, f + ": NULL out");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventSynchronize(s.ev));
    std::memcpy(out, s.h_rec, (size_t)n * fam.rec_bytes);
    return HT_OK;
}

// ht_camshift_*_records_device: the same records where the kernel wrote them
ht_status face_records_device(ht_ctx *c, const FaceFamily &fam, const char *fn, const void **records, int32_t *n) {
    if (!c) return HT_ERR_INVALID;
    HtFaceCalls &s = c->*fam.calls;
    if (!records || !n) return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": NULL argument");
    if (s.n <= 0) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": no " + fam.word + " call yet");
    *records = s.d_rec, *n = s.n;
    return HT_OK;
}

void face_free(ht_ctx *c, const FaceFamily &fam) {  // ht_ingest_free (ht_destroy: the stream has been synchronised)
    HtFaceCalls &s = c->*fam.calls;
    ht_stage_free(&s.tab);
    if (s.d_rec) (void)hipFree(s.d_rec);
    if (s.h_rec) (void)hipHostFree(s.h_rec);
    if (s.ev) (void)hipEventDestroy(s.ev);
    s = HtFaceCalls();
}

}  // namespace

// ---- the crop family ------------------------------------------------------------------------------------------------------------------------
extern "C" ht_status ht_camshift_crop_pairs_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, void *out_dev, size_t out_stride) {
    return face_pairs(c, {CROP, FACE_RGBA8, "ht_camshift_crop_pairs_device", params, 0, nullptr, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_crop_sources_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                     void *out_dev, size_t out_stride) {
    return face_sources(c, {CROP, FACE_RGBA8, "ht_camshift_crop_sources_device", params, 0, nullptr, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_crop_pairs_tensor_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, const ht_patch_format *format,
                                                          void *out_dev, size_t out_stride) {
    return face_pairs(c, {CROP, FACE_TENSOR, "ht_camshift_crop_pairs_tensor_device", params, 0, format, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_crop_sources_tensor_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                            const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_sources(c, {CROP, FACE_TENSOR, "ht_camshift_crop_sources_tensor_device", params, 0, format, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_crop_pairs_filtered_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, int32_t max_factor,
                                                            const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_pairs(c, {CROP, FACE_FILTERED, "ht_camshift_crop_pairs_filtered_device", params, max_factor, format, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_crop_sources_filtered_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                              int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_sources(c, {CROP, FACE_FILTERED, "ht_camshift_crop_sources_filtered_device", params, max_factor, format, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_crop_result(ht_ctx *c, int32_t n, ht_crop_record *out) { return face_result(c, CROP, "ht_camshift_crop_result", n, out); }

extern "C" ht_status ht_camshift_crop_records_device(ht_ctx *c, const void **records, int32_t *n) {
    return face_records_device(c, CROP, "ht_camshift_crop_records_device", records, n);
}

void ht_crop_free(ht_ctx *c) { face_free(c, CROP); }

// ---- the align family -----------------------------------------------------------------------------------------------------------------------
extern "C" ht_status ht_camshift_align_pairs_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, void *out_dev, size_t out_stride) {
    return face_pairs(c, {ALIGN, FACE_RGBA8, "ht_camshift_align_pairs_device", face_params(params), 0, nullptr, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_align_sources_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                      void *out_dev, size_t out_stride) {
    return face_sources(c, {ALIGN, FACE_RGBA8, "ht_camshift_align_sources_device", face_params(params), 0, nullptr, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_align_pairs_tensor_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, const ht_patch_format *format,
                                                           void *out_dev, size_t out_stride) {
    return face_pairs(c, {ALIGN, FACE_TENSOR, "ht_camshift_align_pairs_tensor_device", face_params(params), 0, format, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_align_sources_tensor_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                             const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_sources(c, {ALIGN, FACE_TENSOR, "ht_camshift_align_sources_tensor_device", face_params(params), 0, format, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_align_pairs_filtered_device(ht_ctx *c, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, int32_t max_factor,
                                                             const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_pairs(c, {ALIGN, FACE_FILTERED, "ht_camshift_align_pairs_filtered_device", face_params(params), max_factor, format, out_dev, out_stride}, pairs, n);
}

extern "C" ht_status ht_camshift_align_sources_filtered_device(ht_ctx *c, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                               int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride) {
    return face_sources(c, {ALIGN, FACE_FILTERED, "ht_camshift_align_sources_filtered_device", face_params(params), max_factor, format, out_dev, out_stride}, streams, srcs, n);
}

extern "C" ht_status ht_camshift_align_result(ht_ctx *c, int32_t n, ht_align_record *out) { return face_result(c, ALIGN, "ht_camshift_align_result", n, out); }

extern "C" ht_status ht_camshift_align_records_device(ht_ctx *c, const void **records, int32_t *n) {
    return face_records_device(c, ALIGN, "ht_camshift_align_records_device", records, n);
}

void ht_align_free(ht_ctx *c) { face_free(c, ALIGN); }

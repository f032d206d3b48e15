// ht_napi.cc — thin N-API (raw node_api.h, no node-addon-api) shim over the C ABI in include/headtrackr_hip.h.
// It contains no algorithm: argument unpacking, one C-ABI call, result packing.  The JavaScript facade
// (headtrackr_amd/js/headtrackr.js) builds the reference's API (headtrackr.ccv / camshift / facetrackr) on top of it.
// This comment is the one list of the JavaScript signatures; the usage strings in the error messages repeat them.
//
//   createContext({device, interval, cascade:<Buffer HTCB>, hitCapacity, queueCapacity, options}) -> ctx (external)
//   destroy(ctx)                                          exitNow(code): destroys every live context and leaves with _exit
//   setGeometry(ctx, w, h, maxBatch, Int32Array levelDims | null)
//   detect(ctx, Uint8Array rgba, n, w, h, flags)        -> {frame,x,y,scale,q,sum, counts}   (sync; the drop-in path)
//   detectAsync(ctx, rgba, n, w, h, flags)              -> Promise of the same              (napi_create_async_work)
//   grayscale(ctx, Uint8Array rgba, n, w, h)            -> undefined (in place)
//   whitebalance(ctx, Uint8Array rgba, n, w, h)         -> Float64Array(n)
//   camshiftReserve(ctx, nstreams)
//   camshiftInit(ctx, rgba, n, w, h, first, Int32Array rects[4n])
//   camshiftTrack(ctx, rgba, n, w, h, first, calcAngles) -> Float64Array(9n): x,y,width,height,angle,swx,swy,sww,swh
//   info(ctx) -> {levels, windowsPerFrame, pyramidBytesPerFrame}
//   deviceCount() -> number of visible GPUs
//   allgatherBest([ctx0, ctx1, ...], [Float64Array(6*f) per rank: x,y,width,height,confidence,neighbors], framesPerRank)
//        -> Float64Array(6 * nranks * framesPerRank): every rank's best-face rects after the RCCL all-gather (ht_allgather_best_faces)
//
// The pipelined path (what the throughput numbers are made of; every C-ABI export has a JS name):
//   hostAlloc(bytes) -> Uint8Array over PINNED host memory (ht_host_alloc)         hostFree(Uint8Array returned by hostAlloc)
//   deviceAlloc(ctx, bytes) -> device buffer (external)    deviceFree(ctx, dev)
//   deviceUpload(ctx, dev, byteOffset, Uint8Array)
//   deviceDownload(ctx, dev, byteOffset, Uint8Array)    ht_device_download: fills the array from the buffer, behind the enqueued work; waits
//   upload(ctx, rgba, n, w, h)            ht_upload_frames: bind host frames once, then any number of *Bound calls on them
//   bindDevice(ctx, dev, byteOffset, n, frameStride)     ht_bind_frames_device
//   uploadAsync(ctx, rgba, n) / swapFrames(ctx)          double-buffered ingest (rgba should come from hostAlloc)
//   detectEnqueue(ctx, flags)             ht_detect_enqueue           detectCollect(ctx) -> hits object (ht_detect_collect)
//   collectBest(ctx, minNeighbors, requeueFlags = -1) -> {best: Float64Array(6 n), hits}   ht_detect_collect_best(_requeue)
//   detectBestEnqueue(ctx, minNeighbors, frameBase = 0)   ht_detect_best_enqueue: grouping + best face of the batch in flight on the device
//   collectBestDevice(ctx, requeueFlags = -1) -> {best: Float64Array(6 n), hits}   ht_detect_best_collect(_requeue)
//   detectGrouped(ctx, frame) -> Float64Array(6 k)       ht_detect_grouped: the full grouped list of one frame of that batch
//   detectBestRecords(ctx) -> Float64Array(8 n)          the 64-byte records behind ht_detect_best_records_device, downloaded
//   groupHits(ctx, Uint8Array hits, nframes, minNeighbors) -> {best: Float64Array(6 nframes), grouped: Float64Array(6 k), counts: Uint32Array(nframes)}
//        ht_group_hits: hits = 24-byte ht_hit records in any order
//   detectWhitebalance(ctx, n) -> Float64Array(n)        whitebalanceBound(ctx, n) -> Float64Array(n)
//   camshiftInitBound(ctx, n, first, Int32Array rects[4n])   camshiftTrackBound(ctx, n, first, calcAngles, fetch = true) -> Float64Array(9n) | undefined
//   camshiftTrackCollect(ctx, n) -> Float64Array(9n)
//   camshiftInitPairs(ctx, Int32Array pairs[2n], Int32Array rects[4n])   pairs = stream0, frame0, stream1, frame1, ... (ht_cs_pair)
//   camshiftTrackPairs(ctx, Int32Array pairs[2n], calcAngles, fetch = true) -> Float64Array(9n) | undefined
//   camshiftInitBest(ctx, Int32Array pairs[2n], minConfidence, Int32Array fallback[4n] | null = null)   ht_camshift_init_best: initTracker from the
//        device's best-face records of the device-grouped batch, enqueue only
//   camshiftInitBestResult(ctx, n) -> {codes: Int32Array(n), rects: Int32Array(4n)}   ht_camshift_init_best_result: what the last such call decided
//   camshiftInitFaces(ctx, Int32Array pairs[2n], minConfidence, flags = 0)   ht_camshift_init_faces: a tracker per grouped face of each frame (the
//        frame's pairs are its slots; CSF_ASSOCIATE: a tracker that overlaps a face keeps its slot), enqueue only
//   camshiftInitFacesResult(ctx, n) -> Int32Array(8n)   ht_camshift_init_faces_result: per pair code, face, x, y, width, height, dropped, 0
//   camshiftTrackSequence(ctx, first, n, calcAngles, dev, Float64Array byteOffsets, frameStride, outAll, fetch) -> Float64Array | undefined
//   camshiftSequenceCollect(ctx, n, ncalls, outAll) -> Float64Array
//   camshiftBackProject(ctx, n, first, kind) -> Uint8Array(4 n w h) (BP_RGBA8) | Float64Array(n w h) (BP_F64): back-projection of the bound frames
//   camshiftBackProjectDevice(ctx, n, first, kind, dev, byteOffset, stride)   the same into a deviceAlloc() buffer, enqueue only
//   camshiftBackProjectPairs(ctx, Int32Array pairs[2n], kind) -> Uint8Array(4 n w h) | Float64Array(n w h): bound frame pairs[2i + 1] through stream pairs[2i]
//   camshiftBackProjectPairsDevice(ctx, Int32Array pairs[2n], kind, dev, byteOffset, stride)   the same into a deviceAlloc() buffer, enqueue only
//   drawFrames(ctx, Uint8Array rgba, n, sw, sh, Int32Array rect[4] | null)   ht_draw_frames: the loop's video -> canvas drawImage (main.js:170) of n host
//        frames of sw x sh onto the context's geometry, on the device; the result becomes the bound frames
//   drawFramesDevice(ctx, srcDev, srcOffset, n, sw, sh, pitch, stride, rect | null, dstDev | null, dstOffset, dstStride, wait)   ht_draw_frames_device between
//        deviceAlloc() buffers (dstDev null: into the context's own buffer, bound); wait = true ends with ht_synchronize
//   drawFramesYuv(ctx, Uint8Array planes, n, w, h, format, matrix, Int32Array rect[4] | null)   ht_draw_frames_yuv: the same draw for n host frames in
//       YUV 4:2:0 (format 0 = NV12, 1 = I420; matrix 0 .. 3), each tightly packed (Y, then UV or U, V); the conversion is fused into the draw
//   drawFramesYuvDevice(ctx, srcDev, srcOffset, n, w, h, format, matrix, stride, rect | null, dstDev | null, dstOffset, dstStride, wait)
//       ht_draw_frames_yuv_device on frames packed the same way inside a device buffer, `stride` bytes apart (0 = packed)
//   drawListDevice(ctx, entries, dstDev | null, dstStride, dstOffset = 0, wait = false)   ht_draw_list_device: ONE launch draws entries[i] onto
//       frame i; an entry is {dev, offset, width, height, format (YUV_NV12 | YUV_I420 | DRAW_RGBA), matrix, rect: Int32Array[4] | null} and
//       names ONE frame packed at byte `offset` of its own deviceAlloc() buffer (RGBA rows; Y, then UV or U, V)
//   drawListFilteredDevice(ctx, entries, maxFactor, dstDev | null, dstStride, dstOffset = 0, wait = false)   ht_draw_list_filtered_device: the same
//       draw with every canvas pixel the mean of a block of the unfiltered draw's samples, the block's factors up to maxFactor (1..8) per entry
//   drawFilterFactors(Int32Array sizes[2n], canvasWidth, canvasHeight, maxFactor) -> Int32Array(2n)   ht_draw_filter_factors: Nx, Ny of entries
//       whose source rect is sizes[2i] x sizes[2i + 1]
//   framesBound(ctx), framesEnqueued(ctx), graphLaunches(ctx)
#include <node_api.h>

#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <unistd.h>

#include "headtrackr_hip.h"

namespace {

#define NAPI_OK(call)                                                  \
    do {                                                               \
        if ((call) != napi_ok) {                                       \
            napi_throw_error(env, nullptr, "N-API call failed: " #call); \
            return nullptr;                                            \
        }                                                              \
    } while (0)

napi_value throw_ht(napi_env env, ht_ctx *ctx, ht_status st, const char *where) {
    std::string msg = std::string(where) + ": status " + std::to_string(st) + ": " + ht_last_error(ctx);
    napi_throw_error(env, nullptr, msg.c_str());
    return nullptr;
}
// throw and return nullptr — "no result" for an entry point, `false` for a helper that returns bool
napi_value type_error(napi_env env, const char *msg) {
    napi_throw_type_error(env, nullptr, msg);
    return nullptr;
}
napi_value range_error(napi_env env, const char *msg) {
    napi_throw_range_error(env, nullptr, msg);
    return nullptr;
}

// What the JS side holds (a napi external): the context plus the lock that serialises every use of it.  An ht_ctx is not
// thread-safe (include/headtrackr_hip.h) but detectAsync() runs on a libuv pool thread while the JS thread may call any
// synchronous entry point on the same cached context (headtrackr.js shares one context per cascade): every entry point
// takes `mu` for the duration of its C-ABI calls, so overlapping calls run one after the other, in lock-acquisition order.
// The two kinds of handles the addon gives out are napi externals; a tag in front tells them apart, so that a device buffer passed where a
// context is expected (or the other way round) is a TypeError, not a reinterpretation of the other struct's bytes.  Neither kind is ever freed.
constexpr uint32_t SLOT_TAG = 0x4c535448u, DEVBUF_TAG = 0x42445448u;  // "HTSL", "HTDB"
struct Slot {
    uint32_t tag = SLOT_TAG;
    ht_ctx *ctx = nullptr;
    std::recursive_mutex mu;
    napi_env env = nullptr;  // the environment (main thread or a worker_threads Worker) that created the context: its cleanup hook destroys it
};
// a device buffer: freed explicitly (deviceFree) or, at the latest, with the context it was allocated on
struct DevBuf {
    uint32_t tag = DEVBUF_TAG;
    Slot *slot = nullptr;  // Slots are never freed (a few bytes per context): a JS handle may outlive destroy()
    void *ptr = nullptr;
    size_t bytes = 0;
};

bool get_slot(napi_env env, napi_value v, Slot **out) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || static_cast<Slot *>(p)->tag != SLOT_TAG) {
        napi_throw_type_error(env, nullptr, "expected a headtrackr_hip context");
        return false;
    }
    *out = static_cast<Slot *>(p);
    return true;
}
bool get_devbuf(napi_env env, napi_value v, DevBuf **out) {
    void *p = nullptr;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || static_cast<DevBuf *>(p)->tag != DEVBUF_TAG || !static_cast<DevBuf *>(p)->ptr ||
        !static_cast<DevBuf *>(p)->slot->ctx) {
        napi_throw_type_error(env, nullptr, "expected a live device buffer (deviceAlloc) of a live context");
        return false;
    }
    *out = static_cast<DevBuf *>(p);
    return true;
}

// Locks the slot and yields its context; throws (and returns false) when the context was destroyed.
struct Locked {
    std::unique_lock<std::recursive_mutex> lk;
    ht_ctx *ctx = nullptr;
};
bool lock_ctx(napi_env env, napi_value v, Locked *out) {
    Slot *s = nullptr;
    if (!get_slot(env, v, &s)) return false;
    out->lk = std::unique_lock<std::recursive_mutex>(s->mu);
    out->ctx = s->ctx;
    if (!out->ctx) {
        out->lk.unlock();
        napi_throw_error(env, nullptr, "context was destroyed");
        return false;
    }
    return true;
}

// fewer arguments than the entry point needs: a TypeError, not a silent `undefined` (found by tests/js/addon_args.js)
bool too_few(napi_env env, size_t argc, size_t need) {
    if (argc >= need) return false;
    napi_throw_type_error(env, nullptr, ("headtrackr_hip: " + std::to_string(need) + " arguments expected, " + std::to_string(argc) + " given").c_str());
    return true;
}

bool get_i32(napi_env env, napi_value v, int32_t *out) { return napi_get_value_int32(env, v, out) == napi_ok; }

// a typed array's element type, length and storage; get(.., want, min): of that type with at least min elements
struct View {
    napi_typedarray_type type;
    size_t len = 0, off = 0;
    void *p = nullptr;
    napi_value ab;
    bool get(napi_env env, napi_value v) { return napi_get_typedarray_info(env, v, &type, &len, &p, &ab, &off) == napi_ok; }
    bool get(napi_env env, napi_value v, napi_typedarray_type want, size_t min) { return get(env, v) && type == want && len >= min; }
    template <class T>
    const T *as() const { return static_cast<const T *>(p); }
};

// Uint8Array / Uint8ClampedArray / Buffer -> pointer + length
bool get_bytes(napi_env env, napi_value v, uint8_t **data, size_t *len) {
    bool is_ta = false;
    if (napi_is_typedarray(env, v, &is_ta) == napi_ok && is_ta) {
        View a;
        if (!a.get(env, v) || (a.type != napi_uint8_array && a.type != napi_uint8_clamped_array && a.type != napi_int8_array)) return false;
        *data = static_cast<uint8_t *>(a.p);
        *len = a.len;
        return true;
    }
    bool is_buf = false;
    void *p;
    if (napi_is_buffer(env, v, &is_buf) != napi_ok || !is_buf || napi_get_buffer_info(env, v, &p, len) != napi_ok) return false;
    *data = static_cast<uint8_t *>(p);
    return true;
}

// byte offsets and strides arrive as doubles: 0 .. 2.5e11 (more than any device has), checked BEFORE the conversion to size_t
bool to_offset(double d, size_t *out) {
    if (!(d >= 0) || d > 2.5e11) return false;
    *out = (size_t)d;
    return true;
}
bool get_offset(napi_env env, napi_value v, size_t *out) {
    double d = 0;
    return napi_get_value_double(env, v, &d) == napi_ok && to_offset(d, out);
}

// Int32Array pairs[2n] = stream0, frame0, stream1, frame1, ... (ht_cs_pair); *n = pairs
bool get_pairs(napi_env env, napi_value v, const ht_cs_pair **pairs, int32_t *n) {
    View a;
    if (!a.get(env, v, napi_int32_array, 2) || (a.len & 1) || a.len > (size_t)1 << 24) return false;
    *pairs = a.as<ht_cs_pair>();
    *n = (int32_t)(a.len / 2);
    return true;
}

// rect argument of the draw calls: null / undefined (the whole source frame) or an Int32Array [x, y, width, height]
bool get_rect(napi_env env, napi_value v, ht_cs_rect *r, const ht_cs_rect **out) {
    napi_valuetype vt;
    *out = nullptr;
    if (napi_typeof(env, v, &vt) == napi_ok && (vt == napi_null || vt == napi_undefined)) return true;
    View a;
    if (!a.get(env, v, napi_int32_array, 4)) return false;
    memcpy(r, a.p, sizeof(*r));
    *out = r;
    return true;
}

// n frames, `stride` bytes apart and `frame` bytes each, from byte `off` of a buffer of `bytes`: off + (n - 1) stride + frame <= bytes.
// Every range an entry point hands to the library together with a DevBuf's pointer goes through here (the library cannot know the sizes
// of the buffers the handles stand for).  No product can wrap: a factor is first bounded by a division through the size it has to fit into.
bool frames_fit(size_t off, size_t n, size_t stride, size_t frame, size_t bytes) {
    if (off > bytes || frame > bytes - off) return false;
    return n == 1 || stride <= (bytes - off - frame) / (n - 1);
}

// One entry point's arguments: napi_get_cb_info once for the `max` arguments of its signature (14 = the longest, drawFramesYuvDevice; those
// of them that the caller left out read as undefined; argv[max] and beyond are never read), the arity check, and typed getters by argument
// index.  Lives on the stack of the entry point: this is the Node host's per-frame path.
struct Args {
    napi_env env;
    size_t argc;  // in: max; out: what the caller passed, which may be more
    napi_value argv[14];
    bool ok;
    Args(napi_env e, napi_callback_info info, size_t max) : env(e), argc(max) { ok = napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) == napi_ok; }
    bool arity(size_t need) const {
        if (!ok) napi_throw_error(env, nullptr, "N-API call failed: napi_get_cb_info");
        return ok && !too_few(env, argc, need);
    }
    // the usual opening: at least `need` arguments, the first of them a live context, locked from here on
    bool ctx(size_t need, Locked *L) const { return arity(need) && lock_ctx(env, argv[0], L); }
    bool i32(size_t i, int32_t *out) const { return get_i32(env, argv[i], out); }
    bool offset(size_t i, size_t *out) const { return get_offset(env, argv[i], out); }
    bool bytes(size_t i, uint8_t **data, size_t *len) const { return get_bytes(env, argv[i], data, len); }
    // optional trailing arguments: absent or of another type, the default stays
    void opt_i32(size_t i, int32_t *out) const {
        if (argc > i) get_i32(env, argv[i], out);
    }
    void opt_bool(size_t i, bool *out) const {
        if (argc > i) napi_get_value_bool(env, argv[i], out);
    }
    bool i32s(size_t i, size_t min, View *a) const { return a->get(env, argv[i], napi_int32_array, min); }
    bool f64s(size_t i, size_t min, View *a) const { return a->get(env, argv[i], napi_float64_array, min); }
    bool devbuf(size_t i, DevBuf **out) const { return get_devbuf(env, argv[i], out); }
    bool devbuf_or_null(size_t i, DevBuf **out) const {  // null / undefined: *out stays nullptr
        napi_valuetype vt;
        if (napi_typeof(env, argv[i], &vt) != napi_ok) return false;
        return vt == napi_null || vt == napi_undefined || get_devbuf(env, argv[i], out);
    }
};

// Every live Slot, so that the environment's cleanup hook can destroy the contexts while the HIP runtime is still up: finalizers
// of externals may run during environment teardown or not at all, and a context destroyed after the runtime's own static
// destructors crashes the process at exit.
std::mutex g_slots_mu;
std::vector<Slot *> g_slots;

// Cleanup hook of ONE environment (arg = its napi_env): a Worker that exits destroys the contexts IT created, not the main thread's.
// arg == nullptr (exitNow: the whole process is leaving): every environment's contexts.
void env_cleanup(void *arg) {
    std::lock_guard<std::mutex> lk(g_slots_mu);
    for (Slot *s : g_slots) {
        if (arg && s->env != static_cast<napi_env>(arg)) continue;
        std::lock_guard<std::recursive_mutex> l2(s->mu);
        if (s->ctx) ht_destroy(s->ctx);
        s->ctx = nullptr;
    }
}

// hostAlloc registry: hostFree releases exactly the pointers hostAlloc returned, once (a subarray, a second view or a foreign
// Uint8Array must never reach hipHostFree), and detaches the ArrayBuffer so that JS cannot touch the unmapped pages afterwards
std::mutex g_host_mu;
std::vector<std::pair<void *, size_t>> g_host_allocs;

// ---- result packing ---------------------------------------------------------------------------------------------

// a new Float64Array(n); *data = its storage, for the caller to fill (results are written in place, not copied)
napi_value f64_result(napi_env env, size_t n, double **data) {
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, n * 8, &p, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_float64_array, n, ab, 0, &ta));
    *data = static_cast<double *>(p);
    return ta;
}

// 9 numbers per stream: x, y, width, height, angle, then the search window
napi_value trackobjs_result(napi_env env, const std::vector<ht_cs_trackobj> &out) {
    double *d = nullptr;
    napi_value ta = f64_result(env, out.size() * 9, &d);
    for (size_t i = 0; ta && i < out.size(); i++) {
        const ht_cs_trackobj &o = out[i];
        double *r = d + 9 * i;
        r[0] = o.x, r[1] = o.y, r[2] = o.width, r[3] = o.height, r[4] = o.angle;
        r[5] = o.sw_x, r[6] = o.sw_y, r[7] = o.sw_width, r[8] = o.sw_height;
    }
    return ta;
}

// the 6-number rect layout of the JS side: x, y, width, height, confidence, neighbors
napi_value rect6_result(napi_env env, const ht_rect *r, size_t n) {
    double *d = nullptr;
    napi_value ta = f64_result(env, n * 6, &d);
    for (size_t k = 0; ta && k < n; k++) {
        double *o = d + 6 * k;
        o[0] = r[k].x, o[1] = r[k].y, o[2] = r[k].width, o[3] = r[k].height, o[4] = r[k].confidence, o[5] = r[k].neighbors;
    }
    return ta;
}
ht_rect rect6_unpack(const double *d) { return ht_rect{d[0], d[1], d[2], d[3], d[4], (int32_t)d[5], 0}; }

// NO finalizers on the handles this addon hands to JavaScript.  Node 12 runs finalizers that are still pending while it tears the
// environment down, through N-API's own phantom-callback wrapper, and that wrapper crashes inside libnode (SIGSEGV at exit in
// GlobalHandles::InvokeSecondPassPhantomCallbacks -> libnode, seen in one of two runs of tests/js/bench_host.js whatever the callback
// did).  Native resources are therefore released explicitly — destroy(ctx), deviceFree(ctx, buf), hostFree(arr) — and, for whatever is
// still alive at exit, by the environment's cleanup hook (env_cleanup), which is an ordinary callback, not a finalizer.  A handle that
// is dropped without destroy() keeps its GPU memory until the process exits.

// the optional properties of createContext's argument; an int32 one that is absent or not a number leaves *out alone
bool get_prop(napi_env env, napi_value obj, const char *name, napi_value *v) {
    bool has;
    return napi_has_named_property(env, obj, name, &has) == napi_ok && has && napi_get_named_property(env, obj, name, v) == napi_ok;
}
template <class T>
void prop_i32(napi_env env, napi_value obj, const char *name, T *out) {
    napi_value v;
    int32_t i;
    if (get_prop(env, obj, name, &v) && get_i32(env, v, &i)) *out = (T)i;
}

napi_value CreateContext(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    if (!a.arity(0)) return nullptr;
    napi_value arg = a.argv[0], v;
    ht_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    cfg.interval = 5;
    prop_i32(env, arg, "device", &cfg.device);
    prop_i32(env, arg, "interval", &cfg.interval);
    prop_i32(env, arg, "hitCapacity", &cfg.hit_capacity);
    prop_i32(env, arg, "queueCapacity", &cfg.queue_capacity);
    std::string options;  // ht_config.options: "key=value,..." schedule selectors (tests, A/B runs)
    if (get_prop(env, arg, "options", &v)) {
        size_t len = 0;
        if (napi_get_value_string_utf8(env, v, nullptr, 0, &len) == napi_ok) {
            options.resize(len + 1);
            NAPI_OK(napi_get_value_string_utf8(env, v, &options[0], len + 1, &len));
            options.resize(len);
            cfg.options = options.c_str();
        }
    }
    uint8_t *blob = nullptr;
    size_t blob_len = 0;
    NAPI_OK(napi_get_named_property(env, arg, "cascade", &v));
    if (!get_bytes(env, v, &blob, &blob_len)) return type_error(env, "createContext: `cascade` must be a Buffer/Uint8Array holding an HTCB blob");
    ht_ctx *ctx = nullptr;
    ht_status st = ht_create(&cfg, blob, blob_len, &ctx);
    if (st != HT_OK) return throw_ht(env, nullptr, st, "ht_create");
    Slot *slot = new Slot();
    slot->ctx = ctx;
    slot->env = env;
    {
        std::lock_guard<std::mutex> lk(g_slots_mu);
        g_slots.push_back(slot);
    }
    napi_value ext;
    NAPI_OK(napi_create_external(env, slot, nullptr, nullptr, &ext));  // no finalizer, see above
    return ext;
}

napi_value Destroy(napi_env env, napi_callback_info info) {  // idempotent; anything but a context is ignored
    Args a(env, info, 1);
    void *p = nullptr;
    if (a.ok && a.argc >= 1 && napi_get_value_external(env, a.argv[0], &p) == napi_ok && p && static_cast<Slot *>(p)->tag == SLOT_TAG) {
        Slot *slot = static_cast<Slot *>(p);
        std::lock_guard<std::recursive_mutex> lk(slot->mu);  // waits for an asynchronous job in flight on this context
        if (slot->ctx) ht_destroy(slot->ctx);
        slot->ctx = nullptr;
    }
    return nullptr;
}

napi_value SetGeometry(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    Locked L;
    int32_t w, h, nb;
    if (!a.ctx(0, &L)) return nullptr;
    if (!a.i32(1, &w) || !a.i32(2, &h) || !a.i32(3, &nb)) return type_error(env, "setGeometry(ctx, w, h, maxBatch, levelDims)");
    View dims;  // anything but a typed array (null, undefined): the library computes the level sizes
    bool is_ta = false;
    if (napi_is_typedarray(env, a.argv[4], &is_ta) == napi_ok && is_ta && (!a.i32s(4, 0, &dims) || (dims.len & 1)))
        return type_error(env, "levelDims must be an Int32Array [w0,h0,w1,h1,...]");
    ht_status st = ht_set_geometry(L.ctx, w, h, nb, dims.as<int32_t>(), (int32_t)(dims.len / 2));
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_set_geometry");
    return nullptr;
}

// ---- detect ----------------------------------------------------------------------------------------------------

struct DetectJob {
    Slot *slot = nullptr;
    uint8_t *rgba = nullptr;
    int32_t n = 0, w = 0, h = 0;
    uint32_t flags = 0;
    std::vector<ht_hit> hits;
    std::vector<uint32_t> counts;
    uint32_t total = 0;
    ht_status st = HT_OK;
    std::string err;
    napi_async_work work = nullptr;
    napi_deferred deferred = nullptr;
    napi_ref rgba_ref = nullptr;
    napi_ref ctx_ref = nullptr;  // keeps the context external (and so the Slot) alive until the job completed
};

void run_detect(DetectJob *j) {
    std::lock_guard<std::recursive_mutex> lk(j->slot->mu);
    ht_ctx *ctx = j->slot->ctx;
    if (!ctx) {
        j->st = HT_ERR_STATE;
        j->err = "context was destroyed";
        return;
    }
    uint32_t cap = 4096;
    for (int attempt = 0; attempt < 3; attempt++) {
        j->hits.resize(cap);
        j->counts.assign((size_t)j->n, 0);
        j->st = ht_detect_batch(ctx, j->rgba, j->n, j->w, j->h, (size_t)j->w * j->h * 4, j->flags, j->hits.data(), cap, j->counts.data(), &j->total);
        if (j->st == HT_ERR_CAPACITY && j->total > cap) {  // caller buffer too small: retry with the exact size
            cap = j->total;
            continue;
        }
        break;
    }
    if (j->st != HT_OK) j->err = ht_last_error(ctx);
}
std::string detect_error(const DetectJob &j) { return "ht_detect_batch: status " + std::to_string(j.st) + ": " + j.err; }

// the typed array whose elements are T
template <class T> constexpr napi_typedarray_type array_type_of();
template <> constexpr napi_typedarray_type array_type_of<uint8_t>() { return napi_uint8_array; }
template <> constexpr napi_typedarray_type array_type_of<uint16_t>() { return napi_uint16_array; }
template <> constexpr napi_typedarray_type array_type_of<uint32_t>() { return napi_uint32_array; }
template <> constexpr napi_typedarray_type array_type_of<double>() { return napi_float64_array; }

// obj[name] = the first n elements' member M as a typed array of M's own type
template <class S, class T>
bool set_column(napi_env env, napi_value obj, const char *name, const S *rows, size_t n, T S::*M) {
    napi_value ab, ta;
    void *p = nullptr;
    if (napi_create_arraybuffer(env, n * sizeof(T), &p, &ab) != napi_ok) return false;
    for (size_t i = 0; i < n; i++) static_cast<T *>(p)[i] = rows[i].*M;
    return napi_create_typedarray(env, array_type_of<T>(), n, ab, 0, &ta) == napi_ok && napi_set_named_property(env, obj, name, ta) == napi_ok;
}

// the hits as one typed array per ht_hit member + counts per frame
napi_value pack_hits(napi_env env, const DetectJob &j) {
    napi_value obj;
    NAPI_OK(napi_create_object(env, &obj));
    const ht_hit *h = j.hits.data();
    const size_t n = j.total;
    if (!set_column(env, obj, "frame", h, n, &ht_hit::frame) || !set_column(env, obj, "x", h, n, &ht_hit::x) || !set_column(env, obj, "y", h, n, &ht_hit::y) ||
        !set_column(env, obj, "scale", h, n, &ht_hit::scale) || !set_column(env, obj, "q", h, n, &ht_hit::q) || !set_column(env, obj, "sum", h, n, &ht_hit::sum)) {
        napi_throw_error(env, nullptr, "N-API call failed: pack_hits");
        return nullptr;
    }
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, j.counts.size() * 4, &p, &ab));
    if (!j.counts.empty()) std::memcpy(p, j.counts.data(), j.counts.size() * 4);
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, j.counts.size(), ab, 0, &ta));
    NAPI_OK(napi_set_named_property(env, obj, "counts", ta));
    return obj;
}

bool parse_detect_args(const Args &a, DetectJob *j) {
    napi_env env = a.env;
    if (!a.ok || a.argc < 5) return type_error(env, "detect(ctx, rgba, n, w, h, flags)");
    if (!get_slot(env, a.argv[0], &j->slot)) return false;
    size_t len = 0;
    int32_t fl = 0;
    if (!a.bytes(1, &j->rgba, &len) || !a.i32(2, &j->n) || !a.i32(3, &j->w) || !a.i32(4, &j->h)) return type_error(env, "detect(ctx, rgba, n, w, h, flags): bad argument");
    a.opt_i32(5, &fl);
    j->flags = (uint32_t)fl;
    if (j->n <= 0 || j->w <= 0 || j->h <= 0 || len < (size_t)j->n * j->w * j->h * 4) return range_error(env, "detect: rgba buffer smaller than n*w*h*4");
    return true;
}

napi_value Detect(napi_env env, napi_callback_info info) {
    Args a(env, info, 6);
    DetectJob j;
    if (!parse_detect_args(a, &j)) return nullptr;
    run_detect(&j);
    if (j.st != HT_OK) {
        napi_throw_error(env, nullptr, detect_error(j).c_str());
        return nullptr;
    }
    return pack_hits(env, j);
}

void detect_execute(napi_env, void *data) { run_detect(static_cast<DetectJob *>(data)); }

void detect_complete(napi_env env, napi_status, void *data) {
    DetectJob *j = static_cast<DetectJob *>(data);
    if (j->st == HT_OK) {
        napi_value v = pack_hits(env, *j);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg, err;
        napi_create_string_utf8(env, detect_error(*j).c_str(), NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, nullptr, msg, &err);
        napi_reject_deferred(env, j->deferred, err);
    }
    napi_delete_reference(env, j->rgba_ref);
    napi_delete_reference(env, j->ctx_ref);
    napi_delete_async_work(env, j->work);
    delete j;
}

napi_value DetectAsync(napi_env env, napi_callback_info info) {
    Args a(env, info, 6);
    DetectJob *j = new DetectJob();
    if (!parse_detect_args(a, j)) {
        delete j;
        return nullptr;
    }
    napi_value promise, name;
    NAPI_OK(napi_create_promise(env, &j->deferred, &promise));
    NAPI_OK(napi_create_reference(env, a.argv[1], 1, &j->rgba_ref));  // keep the frame buffer alive while the GPU works
    NAPI_OK(napi_create_reference(env, a.argv[0], 1, &j->ctx_ref));
    NAPI_OK(napi_create_string_utf8(env, "headtrackr_hip.detect", NAPI_AUTO_LENGTH, &name));
    NAPI_OK(napi_create_async_work(env, nullptr, name, detect_execute, detect_complete, j, &j->work));
    NAPI_OK(napi_queue_async_work(env, j->work));
    return promise;
}

// ---- host frames: grayscale / whitebalance / camshift / upload / drawFrames ---------------------------------------------

struct FrameArgs {
    Locked L;  // the context stays locked for the lifetime of the argument block = the whole entry point
    ht_ctx *ctx;
    uint8_t *rgba;
    int32_t n, w, h;
};

// (ctx, rgba, n, w, h, ...) of an entry point that needs `need` arguments
bool parse_frames(const Args &a, size_t need, FrameArgs *f) {
    size_t len = 0;
    if (!a.ctx(need, &f->L)) return false;
    f->ctx = f->L.ctx;
    if (!a.bytes(1, &f->rgba, &len) || !a.i32(2, &f->n) || !a.i32(3, &f->w) || !a.i32(4, &f->h) || f->n <= 0 || f->w <= 0 || f->h <= 0 ||
        len < (size_t)f->n * f->w * f->h * 4)
        return type_error(a.env, "expected (ctx, Uint8Array rgba, n, w, h, ...) with rgba.length >= n*w*h*4");
    return true;
}

ht_status bind_host_frames(const FrameArgs &a) {
    ht_status st = ht_set_geometry(a.ctx, a.w, a.h, a.n, nullptr, 0);  // no-op when unchanged
    if (st != HT_OK) return st;
    return ht_upload_frames(a.ctx, a.rgba, a.n, (size_t)a.w * a.h * 4);
}

napi_value Grayscale(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    FrameArgs f;
    if (!parse_frames(a, 5, &f)) return nullptr;
    ht_status st = ht_grayscale_batch(f.ctx, f.rgba, f.n, f.w, f.h, (size_t)f.w * f.h * 4);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_grayscale_batch");
    return nullptr;
}

// getWhitebalance of the first n bound frames, or (fused) of the batch enqueued with DETECT_WHITEBALANCE
napi_value wb_result(napi_env env, ht_ctx *ctx, int32_t n, bool fused) {
    double *out = nullptr;
    napi_value ta = f64_result(env, (size_t)n, &out);
    if (!ta) return nullptr;
    ht_status st = fused ? ht_detect_whitebalance(ctx, out, n) : ht_whitebalance_batch(ctx, out, n);
    if (st != HT_OK) return throw_ht(env, ctx, st, fused ? "ht_detect_whitebalance" : "ht_whitebalance_batch");
    return ta;
}

napi_value Whitebalance(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    FrameArgs f;
    if (!parse_frames(a, 5, &f)) return nullptr;
    ht_status st = bind_host_frames(f);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_upload_frames");
    return wb_result(env, f.ctx, f.n, false);
}

napi_value wb_common(napi_env env, napi_callback_info info, bool fused) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0) return type_error(env, "(ctx, n)");
    return wb_result(env, L.ctx, n, fused);
}
napi_value DetectWhitebalance(napi_env env, napi_callback_info info) { return wb_common(env, info, true); }
napi_value WhitebalanceBound(napi_env env, napi_callback_info info) { return wb_common(env, info, false); }

napi_value Upload(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    FrameArgs f;
    if (!parse_frames(a, 5, &f)) return nullptr;
    ht_status st = bind_host_frames(f);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_upload_frames");
    return nullptr;
}

napi_value DrawFrames(napi_env env, napi_callback_info info) {
    Args a(env, info, 6);
    FrameArgs f;
    ht_cs_rect r;
    const ht_cs_rect *rp = nullptr;
    if (!parse_frames(a, 5, &f)) return nullptr;
    if (!get_rect(env, a.argv[5], &r, &rp)) return type_error(env, "drawFrames(ctx, Uint8Array rgba, n, sw, sh, Int32Array rect[4] | null)");
    ht_status st = ht_draw_frames(f.ctx, f.rgba, f.n, f.w, f.h, 0, rp);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_draw_frames");
    return nullptr;
}

// a format number without the orientation it may carry in bits 8..10 (HT_ORIENT: the facade packs a feed's orientation there, and the layout
// of a frame in memory does not depend on it); a value with a bit from 11 up is no format, stays whole and is refused by the library
int32_t bare_format(int32_t format) { return (format & ~0x7ff) ? format : HT_FORMAT_OF(format); }

bool yuv_packed_422(int32_t format) { return bare_format(format) == HT_YUV_YUYV || bare_format(format) == HT_YUV_UYVY; }

// bytes of one tightly packed YUV frame: 4:2:0 (Y, then the chroma planes) w h + 2 cw ch, packed 4:2:2 (YUYV / UYVY: one plane of 4-byte
// macropixels) 4 cw h; 0: no such frame.  A format the library does not know is sized as 4:2:0 and refused by the library
size_t yuv_frame_bytes(int32_t w, int32_t h, int32_t format) {
    if (w <= 0 || h <= 0 || w > 16384 || h > 16384) return 0;
    if (yuv_packed_422(format)) return 4 * (size_t)((w + 1) / 2) * (size_t)h;
    return (size_t)w * h + 2 * (size_t)((w + 1) / 2) * ((h + 1) / 2);
}

napi_value DrawFramesYuv(napi_env env, napi_callback_info info) {
    static const char *usage = "drawFramesYuv(ctx, Uint8Array planes, n, w, h, format, matrix, Int32Array rect[4] | null) with planes.length >= n * (w*h + 2*ceil(w/2)*ceil(h/2)), YUYV / UYVY: n * 4*ceil(w/2)*h";
    Args a(env, info, 8);
    Locked L;
    uint8_t *data = nullptr;
    size_t len = 0;
    int32_t n = 0, w = 0, h = 0, format = 0, matrix = 0;
    ht_cs_rect r;
    const ht_cs_rect *rp = nullptr;
    if (!a.ctx(7, &L)) return nullptr;
    if (!a.bytes(1, &data, &len) || !a.i32(2, &n) || !a.i32(3, &w) || !a.i32(4, &h) || !a.i32(5, &format) || !a.i32(6, &matrix) || !get_rect(env, a.argv[7], &r, &rp) || n <= 0)
        return type_error(env, usage);
    const size_t fsz = yuv_frame_bytes(w, h, format);
    if (!fsz || !frames_fit(0, (size_t)n, fsz, fsz, len)) return range_error(env, usage);
    ht_status st = ht_draw_frames_yuv(L.ctx, data, n, w, h, format, matrix, 0, rp);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_draw_frames_yuv");
    return nullptr;
}

// ---- camshift ---------------------------------------------------------------------------------------------------

napi_value CamshiftReserve(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n;
    if (!a.ctx(0, &L)) return nullptr;
    if (!a.i32(1, &n)) return type_error(env, "camshiftReserve(ctx, nstreams)");
    ht_status st = ht_camshift_reserve(L.ctx, n);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_reserve");
    return nullptr;
}

napi_value CamshiftInit(napi_env env, napi_callback_info info) {
    Args a(env, info, 7);
    FrameArgs f;
    int32_t first;
    View rects;
    if (!parse_frames(a, 7, &f)) return nullptr;
    if (!a.i32(5, &first) || !a.i32s(6, (size_t)f.n * 4, &rects)) return type_error(env, "camshiftInit(ctx, rgba, n, w, h, first, Int32Array rects[4n])");
    ht_status st = bind_host_frames(f);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_upload_frames");
    st = ht_camshift_init_batch(f.ctx, first, f.n, rects.as<ht_cs_rect>());
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_camshift_init_batch");
    return nullptr;
}

napi_value CamshiftTrack(napi_env env, napi_callback_info info) {
    Args a(env, info, 7);
    FrameArgs f;
    int32_t first, calc;
    if (!parse_frames(a, 7, &f)) return nullptr;
    if (!a.i32(5, &first) || !a.i32(6, &calc)) return type_error(env, "camshiftTrack(ctx, rgba, n, w, h, first, calcAngles)");
    ht_status st = bind_host_frames(f);
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_upload_frames");
    std::vector<ht_cs_trackobj> out((size_t)f.n);
    st = ht_camshift_track_batch(f.ctx, first, f.n, calc, out.data());
    if (st != HT_OK) return throw_ht(env, f.ctx, st, "ht_camshift_track_batch");
    return trackobjs_result(env, out);
}

napi_value CamshiftInitBound(napi_env env, napi_callback_info info) {
    Args a(env, info, 4);
    Locked L;
    int32_t n = 0, first = 0;
    View rects;
    if (!a.ctx(4, &L)) return nullptr;
    if (!a.i32(1, &n) || !a.i32(2, &first) || n <= 0 || !a.i32s(3, (size_t)n * 4, &rects)) return type_error(env, "camshiftInitBound(ctx, n, first, Int32Array rects[4n])");
    ht_status st = ht_camshift_init_batch(L.ctx, first, n, rects.as<ht_cs_rect>());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_batch");
    return nullptr;
}

napi_value CamshiftTrackBound(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    Locked L;
    int32_t n = 0, first = 0, calc = 1;
    bool fetch = true;
    if (!a.ctx(4, &L)) return nullptr;
    if (!a.i32(1, &n) || !a.i32(2, &first) || !a.i32(3, &calc) || n <= 0) return type_error(env, "camshiftTrackBound(ctx, n, first, calcAngles, fetch)");
    a.opt_bool(4, &fetch);
    std::vector<ht_cs_trackobj> out((size_t)n);
    ht_status st = ht_camshift_track_batch(L.ctx, first, n, calc, fetch ? out.data() : nullptr);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_track_batch");
    return fetch ? trackobjs_result(env, out) : nullptr;
}

napi_value CamshiftInitPairs(napi_env env, napi_callback_info info) {
    Args a(env, info, 3);
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0;
    View rects;
    if (!a.ctx(3, &L)) return nullptr;
    if (!get_pairs(env, a.argv[1], &pairs, &n) || !a.i32s(2, (size_t)n * 4, &rects)) return type_error(env, "camshiftInitPairs(ctx, Int32Array pairs[2n], Int32Array rects[4n])");
    ht_status st = ht_camshift_init_pairs(L.ctx, pairs, n, rects.as<ht_cs_rect>());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_pairs");
    return nullptr;
}

napi_value CamshiftInitBest(napi_env env, napi_callback_info info) {
    Args a(env, info, 4);
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0;
    double min_conf = 0;
    View fb;
    const ht_cs_rect *fallback = nullptr;
    const char *usage = "camshiftInitBest(ctx, Int32Array pairs[2n], minConfidence, Int32Array fallback[4n] | null)";
    if (!a.ctx(3, &L)) return nullptr;
    if (!get_pairs(env, a.argv[1], &pairs, &n) || napi_get_value_double(env, a.argv[2], &min_conf) != napi_ok) return type_error(env, usage);
    napi_valuetype vt = napi_undefined;
    if (a.argc > 3 && napi_typeof(env, a.argv[3], &vt) != napi_ok) return type_error(env, usage);
    if (vt != napi_undefined && vt != napi_null) {
        if (!a.i32s(3, (size_t)n * 4, &fb)) return type_error(env, usage);
        fallback = fb.as<ht_cs_rect>();
    }
    ht_status st = ht_camshift_init_best(L.ctx, pairs, n, min_conf, fallback);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_best");
    return nullptr;
}

napi_value CamshiftInitBestResult(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0 || n > (1 << 24)) return type_error(env, "camshiftInitBestResult(ctx, n)");
    std::vector<int32_t> codes((size_t)n);
    std::vector<ht_cs_rect> rects((size_t)n);
    ht_status st = ht_camshift_init_best_result(L.ctx, n, codes.data(), rects.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_best_result");
    napi_value obj, ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 4, &p, &ab));
    memcpy(p, codes.data(), (size_t)n * 4);
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)n, ab, 0, &ta));
    NAPI_OK(napi_set_named_property(env, obj, "codes", ta));
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 16, &p, &ab));
    memcpy(p, rects.data(), (size_t)n * 16);
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)n * 4, ab, 0, &ta));
    NAPI_OK(napi_set_named_property(env, obj, "rects", ta));
    return obj;
}

napi_value CamshiftInitFaces(napi_env env, napi_callback_info info) {
    Args a(env, info, 4);
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0, flags = 0;
    double min_conf = 0;
    const char *usage = "camshiftInitFaces(ctx, Int32Array pairs[2n], minConfidence, flags = 0)";
    if (!a.ctx(3, &L)) return nullptr;
    if (!get_pairs(env, a.argv[1], &pairs, &n) || napi_get_value_double(env, a.argv[2], &min_conf) != napi_ok) return type_error(env, usage);
    napi_valuetype vt = napi_undefined;
    if (a.argc > 3 && napi_typeof(env, a.argv[3], &vt) == napi_ok && vt != napi_undefined && vt != napi_null && !a.i32(3, &flags)) return type_error(env, usage);
    ht_status st = ht_camshift_init_faces(L.ctx, pairs, n, min_conf, (uint32_t)flags);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_faces");
    return nullptr;
}

napi_value CamshiftInitFacesResult(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0 || n > (1 << 24)) return type_error(env, "camshiftInitFacesResult(ctx, n)");
    std::vector<ht_csf_record> recs((size_t)n);
    ht_status st = ht_camshift_init_faces_result(L.ctx, n, recs.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_init_faces_result");
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * sizeof(ht_csf_record), &p, &ab));
    memcpy(p, recs.data(), (size_t)n * sizeof(ht_csf_record));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)n * 8, ab, 0, &ta));
    return ta;
}

napi_value CamshiftTrackPairs(napi_env env, napi_callback_info info) {
    Args a(env, info, 4);
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0, calc = 1;
    bool fetch = true;
    if (!a.ctx(3, &L)) return nullptr;
    if (!get_pairs(env, a.argv[1], &pairs, &n) || !a.i32(2, &calc)) return type_error(env, "camshiftTrackPairs(ctx, Int32Array pairs[2n], calcAngles, fetch)");
    a.opt_bool(3, &fetch);
    std::vector<ht_cs_trackobj> out((size_t)n);
    ht_status st = ht_camshift_track_pairs(L.ctx, pairs, n, calc, fetch ? out.data() : nullptr);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_track_pairs");
    return fetch ? trackobjs_result(env, out) : nullptr;
}

napi_value CamshiftTrackCollect(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0) return type_error(env, "camshiftTrackCollect(ctx, n)");
    std::vector<ht_cs_trackobj> out((size_t)n);
    ht_status st = ht_camshift_track_collect(L.ctx, n, out.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_track_collect");
    return trackobjs_result(env, out);
}

napi_value CamshiftTrackSequence(napi_env env, napi_callback_info info) {
    Args a(env, info, 9);
    Locked L;
    DevBuf *d = nullptr;
    int32_t first = 0, n = 0, calc = 1;
    size_t stride = 0;
    bool out_all = false, fetch = true;
    View offs;
    if (!a.ctx(7, &L)) return nullptr;
    if (!a.i32(1, &first) || !a.i32(2, &n) || !a.i32(3, &calc) || !a.devbuf(4, &d)) return nullptr;
    if (!a.f64s(5, 1, &offs) || offs.len > 100000 || !a.offset(6, &stride) || n <= 0)
        return type_error(env, "camshiftTrackSequence(ctx, first, n, calcAngles, dev, Float64Array byteOffsets, frameStride, outAll, fetch)");
    a.opt_bool(7, &out_all);
    a.opt_bool(8, &fetch);
    const size_t ncalls = offs.len;
    std::vector<const void *> ptrs(ncalls);
    for (size_t k = 0; k < ncalls; k++) {
        size_t o = 0;
        if (!to_offset(offs.as<double>()[k], &o) || !frames_fit(o, (size_t)n, stride, stride, d->bytes))
            return range_error(env, "camshiftTrackSequence: a call's frames lie outside the device buffer");
        ptrs[k] = static_cast<const char *>(d->ptr) + o;
    }
    std::vector<ht_cs_trackobj> out(fetch ? (size_t)n * (out_all ? ncalls : 1) : 0);
    ht_status st = ht_camshift_track_sequence(L.ctx, first, n, calc, ptrs.data(), (int32_t)ncalls, stride, fetch ? out.data() : nullptr, out_all ? 1 : 0);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_track_sequence");
    return fetch ? trackobjs_result(env, out) : nullptr;
}

napi_value CamshiftSequenceCollect(napi_env env, napi_callback_info info) {
    Args a(env, info, 4);
    Locked L;
    int32_t n = 0, ncalls = 0;
    bool out_all = false;
    if (!a.ctx(3, &L)) return nullptr;
    if (!a.i32(1, &n) || !a.i32(2, &ncalls) || n <= 0 || ncalls <= 0) return type_error(env, "camshiftSequenceCollect(ctx, n, ncalls, outAll)");
    a.opt_bool(3, &out_all);
    std::vector<ht_cs_trackobj> out((size_t)n * (out_all ? (size_t)ncalls : 1));
    ht_status st = ht_camshift_sequence_collect(L.ctx, n, ncalls, out_all ? 1 : 0, out.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_sequence_collect");
    return trackobjs_result(env, out);
}

// bytes of one frame of the context's geometry at `elem` bytes per pixel (level 0 of the pyramid is the frame itself); 0, with `who`'s
// exception pending, when the context has no geometry yet
size_t frame_bytes(napi_env env, ht_ctx *ctx, size_t elem, const char *who) {
    ht_plane_info pl;
    if (ht_plane(ctx, 0, 0, &pl) == HT_OK && pl.width > 0 && pl.height > 0) return (size_t)pl.width * (size_t)pl.height * elem;  // <= 16384 * 16384 * 8
    napi_throw_error(env, nullptr, (std::string(who) + ": no geometry (setGeometry first)").c_str());
    return 0;
}

// The four back-projection exports are two functions, host and device, over two forms of saying which (stream, frame) pairs:
// the batch form (n, first) — streams [first, first + n) on bound frames [0, n) — or a pair list.
struct BpForm {
    bool pairs;
    const char *name, *where, *usage, *range;
};
const BpForm BP_HOST[2] = {{false, "camshiftBackProject", "ht_camshift_backproject", "camshiftBackProject(ctx, n, first, kind = BP_RGBA8 | BP_F64)", nullptr},
                           {true, "camshiftBackProjectPairs", "ht_camshift_backproject_pairs", "camshiftBackProjectPairs(ctx, Int32Array pairs[2n], kind = BP_RGBA8 | BP_F64)", nullptr}};
const BpForm BP_DEVICE[2] = {
    {false, "camshiftBackProjectDevice", "ht_camshift_backproject_device", "camshiftBackProjectDevice(ctx, n, first, kind = BP_RGBA8 | BP_F64, dev, byteOffset, stride)",
     "camshiftBackProjectDevice(ctx, n, first, kind, dev, byteOffset, stride): outside the device buffer"},
    {true, "camshiftBackProjectPairsDevice", "ht_camshift_backproject_pairs_device",
     "camshiftBackProjectPairsDevice(ctx, Int32Array pairs[2n], kind = BP_RGBA8 | BP_F64, dev, byteOffset, stride)",
     "camshiftBackProjectPairsDevice(ctx, pairs, kind, dev, byteOffset, stride): outside the device buffer"}};

struct BpCall {
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0, first = 0, kind = 0;
    size_t rest = 0;  // index of the first argument after `kind`
};
// (ctx, n, first | pairs, kind, `more` further arguments): the context, the form's arguments and a valid kind
bool bp_begin(const Args &a, const BpForm &f, size_t more, BpCall *c) {
    c->rest = f.pairs ? 3 : 4;
    if (!a.ctx(c->rest + more, &c->L)) return false;
    const bool which = f.pairs ? get_pairs(a.env, a.argv[1], &c->pairs, &c->n) : a.i32(1, &c->n) && a.i32(2, &c->first);
    if (!which || !a.i32(c->rest - 1, &c->kind) || c->n <= 0 || (c->kind != HT_BP_RGBA8 && c->kind != HT_BP_F64)) return type_error(a.env, f.usage);
    return true;
}

napi_value bp_host(napi_env env, napi_callback_info info, const BpForm &f) {
    Args a(env, info, f.pairs ? 3 : 4);
    BpCall c;
    if (!bp_begin(a, f, 0, &c)) return nullptr;
    const size_t elem = c.kind == HT_BP_F64 ? 8 : 4, frame = frame_bytes(env, c.L.ctx, elem, f.name);
    if (!frame) return nullptr;
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, (size_t)c.n * frame, &p, &ab));
    // the stride is passed explicitly: the library refuses one that is smaller than ITS frame, so the buffer can never be too small
    ht_status st = f.pairs ? ht_camshift_backproject_pairs(c.L.ctx, c.pairs, c.n, c.kind, p, frame) : ht_camshift_backproject(c.L.ctx, c.first, c.n, c.kind, p, frame);
    if (st != HT_OK) return throw_ht(env, c.L.ctx, st, f.where);
    if (c.kind == HT_BP_F64) NAPI_OK(napi_create_typedarray(env, napi_float64_array, (size_t)c.n * frame / 8, ab, 0, &ta));
    else NAPI_OK(napi_create_typedarray(env, napi_uint8_array, (size_t)c.n * frame, ab, 0, &ta));
    return ta;
}

napi_value bp_device(napi_env env, napi_callback_info info, const BpForm &f) {
    Args a(env, info, f.pairs ? 6 : 7);
    BpCall c;
    DevBuf *d = nullptr;
    size_t off = 0, stride = 0;
    if (!bp_begin(a, f, 3, &c) || !a.devbuf(c.rest, &d)) return nullptr;
    const size_t frame = frame_bytes(env, c.L.ctx, c.kind == HT_BP_F64 ? 8 : 4, f.name);
    if (!frame) return nullptr;
    if (!a.offset(c.rest + 1, &off) || !a.offset(c.rest + 2, &stride) || (stride != 0 && stride < frame)) return range_error(env, f.range);
    if (!stride) stride = frame;  // 0 = packed
    if (!frames_fit(off, (size_t)c.n, stride, frame, d->bytes)) return range_error(env, f.range);
    void *out = static_cast<char *>(d->ptr) + off;
    ht_status st = f.pairs ? ht_camshift_backproject_pairs_device(c.L.ctx, c.pairs, c.n, c.kind, out, stride) : ht_camshift_backproject_device(c.L.ctx, c.first, c.n, c.kind, out, stride);
    if (st != HT_OK) return throw_ht(env, c.L.ctx, st, f.where);
    return nullptr;
}
napi_value CamshiftBackProject(napi_env env, napi_callback_info info) { return bp_host(env, info, BP_HOST[0]); }
napi_value CamshiftBackProjectPairs(napi_env env, napi_callback_info info) { return bp_host(env, info, BP_HOST[1]); }
napi_value CamshiftBackProjectDevice(napi_env env, napi_callback_info info) { return bp_device(env, info, BP_DEVICE[0]); }
napi_value CamshiftBackProjectPairsDevice(napi_env env, napi_callback_info info) { return bp_device(env, info, BP_DEVICE[1]); }

// ---- info / multi-GPU ----------------------------------------------------------------------------------------------

napi_value Info(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    Locked L;
    if (!a.ctx(0, &L)) return nullptr;
    napi_value obj, v;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_create_int32(env, ht_num_levels(L.ctx), &v));
    NAPI_OK(napi_set_named_property(env, obj, "levels", v));
    NAPI_OK(napi_create_double(env, (double)ht_windows_per_frame(L.ctx), &v));
    NAPI_OK(napi_set_named_property(env, obj, "windowsPerFrame", v));
    NAPI_OK(napi_create_double(env, (double)ht_pyramid_bytes_per_frame(L.ctx), &v));
    NAPI_OK(napi_set_named_property(env, obj, "pyramidBytesPerFrame", v));
    return obj;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
    napi_value v;
    NAPI_OK(napi_create_int32(env, ht_device_count(), &v));
    return v;
}

napi_value AllgatherBest(napi_env env, napi_callback_info info) {
    Args a(env, info, 3);
    uint32_t nctx = 0, nbest = 0;
    int32_t per = 0;
    if (!a.ok || a.argc < 3 || napi_get_array_length(env, a.argv[0], &nctx) != napi_ok || napi_get_array_length(env, a.argv[1], &nbest) != napi_ok || nctx == 0 ||
        nctx != nbest || !a.i32(2, &per) || per <= 0)
        return type_error(env, "allgatherBest([ctx...], [Float64Array...], framesPerRank)");
    std::vector<Locked> locks(nctx);  // every rank's context stays locked for the exchange (slots are distinct: no lock-order issue
                                      // as long as callers pass the contexts in the same order, which headtrackr.js does)
    std::vector<ht_ctx *> ctxs(nctx);
    std::vector<std::vector<ht_rect>> rects(nctx, std::vector<ht_rect>((size_t)per));
    std::vector<const ht_rect *> ptrs(nctx);
    for (uint32_t i = 0; i < nctx; i++) {
        napi_value cv, bv;
        NAPI_OK(napi_get_element(env, a.argv[0], i, &cv));
        NAPI_OK(napi_get_element(env, a.argv[1], i, &bv));
        Slot *slot = nullptr;
        if (!get_slot(env, cv, &slot)) return nullptr;
        for (uint32_t k = 0; k < i; k++)
            if (locks[k].lk.mutex() == &slot->mu) {
                napi_throw_error(env, nullptr, "allgatherBest: the same context was passed twice (one context per GPU)");
                return nullptr;
            }
        if (!lock_ctx(env, cv, &locks[i])) return nullptr;
        ctxs[i] = locks[i].ctx;
        View best;
        if (!best.get(env, bv, napi_float64_array, (size_t)per * 6)) return type_error(env, "allgatherBest: every rank needs a Float64Array of 6 * framesPerRank numbers");
        for (int f = 0; f < per; f++) rects[i][(size_t)f] = rect6_unpack(best.as<double>() + 6 * f);
        ptrs[i] = rects[i].data();
    }
    std::vector<ht_rect> out((size_t)nctx * per);
    ht_status st = ht_allgather_best_faces(ctxs.data(), (int32_t)nctx, ptrs.data(), per, out.data());
    if (st != HT_OK) return throw_ht(env, ctxs[0], st, "ht_allgather_best_faces");
    return rect6_result(env, out.data(), out.size());
}

// ---- pipelined path ------------------------------------------------------------------------------------------------------------

napi_value HostAlloc(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    double bytes = 0;
    if (!a.ok || a.argc < 1 || napi_get_value_double(env, a.argv[0], &bytes) != napi_ok || !(bytes >= 1) || bytes > 1e12) return type_error(env, "hostAlloc(bytes)");
    void *p = nullptr;
    ht_status st = ht_host_alloc((size_t)bytes, &p);
    if (st != HT_OK) return throw_ht(env, nullptr, st, "ht_host_alloc");
    napi_value ab, ta;
    if (napi_create_external_arraybuffer(env, p, (size_t)bytes, nullptr, nullptr, &ab) != napi_ok) {  // no finalizer: hostFree(arr)
        ht_host_free(p);
        napi_throw_error(env, nullptr, "hostAlloc: napi_create_external_arraybuffer failed");
        return nullptr;
    }
    NAPI_OK(napi_create_typedarray(env, napi_uint8_array, (size_t)bytes, ab, 0, &ta));
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_allocs.emplace_back(p, (size_t)bytes);
    }
    return ta;
}

// releases the pinned memory; the array must not be used afterwards
napi_value HostFree(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    View v;
    bool is_ta = false;
    if (!a.ok || a.argc < 1 || napi_is_typedarray(env, a.argv[0], &is_ta) != napi_ok || !is_ta || !v.get(env, a.argv[0]) || !v.p)
        return type_error(env, "hostFree(Uint8Array returned by hostAlloc)");
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        auto it = g_host_allocs.end();
        if (v.off == 0)
            for (auto i = g_host_allocs.begin(); i != g_host_allocs.end(); ++i)
                if (i->first == v.p && i->second == v.len) it = i;
        if (it == g_host_allocs.end()) {  // a subarray / second view / foreign array / already freed: nothing is released
            napi_throw_error(env, nullptr, "hostFree: not a live hostAlloc() array (pass the array hostAlloc returned, whole, once)");
            return nullptr;
        }
        g_host_allocs.erase(it);
    }
    ht_host_free(v.p);
    (void)napi_detach_arraybuffer(env, v.ab);  // every view now has length 0: no use-after-free from JavaScript
    return nullptr;
}

// exitNow(code): destroys every live context (stream synchronised, device memory freed) and leaves with _exit — no atexit handlers,
// no static destructors, no environment teardown.  For hosts that are done: a Node 12 process that used HIP from libuv pool threads
// (detectAsync) has been seen to crash with SIGSEGV inside the runtime's own exit path after a complete, correct run.
napi_value ExitNow(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    int32_t code = 0;
    if (a.ok) a.opt_i32(0, &code);
    env_cleanup(nullptr);
    fflush(stdout);
    fflush(stderr);
    _exit(code);
    return nullptr;
}

napi_value DeviceAlloc(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    double bytes = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (napi_get_value_double(env, a.argv[1], &bytes) != napi_ok || !(bytes >= 1) || bytes > 2.5e11) return type_error(env, "deviceAlloc(ctx, bytes)");
    DevBuf *d = new DevBuf();
    ht_status st = ht_device_alloc(L.ctx, (size_t)bytes, &d->ptr);
    if (st != HT_OK) {
        delete d;
        return throw_ht(env, L.ctx, st, "ht_device_alloc");
    }
    get_slot(env, a.argv[0], &d->slot);
    d->bytes = (size_t)bytes;
    napi_value ext;
    NAPI_OK(napi_create_external(env, d, nullptr, nullptr, &ext));  // no finalizer: freed by deviceFree or with its context
    return ext;
}

napi_value DeviceFree(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    DevBuf *d = nullptr;
    if (!a.ctx(2, &L) || !a.devbuf(1, &d)) return nullptr;
    ht_status st = ht_device_free(L.ctx, d->ptr);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_device_free");  // e.g. the wrong context, or still bound elsewhere: the handle stays valid
    d->ptr = nullptr;
    return nullptr;
}

// deviceUpload / deviceDownload(ctx, dev, byteOffset, Uint8Array): the array's bytes to / from byteOffset of the buffer
napi_value device_copy(napi_env env, napi_callback_info info, bool up) {
    Args a(env, info, 4);
    Locked L;
    DevBuf *d = nullptr;
    uint8_t *host = nullptr;
    size_t len = 0, off = 0;
    if (!a.ctx(4, &L) || !a.devbuf(1, &d)) return nullptr;
    if (!a.offset(2, &off) || !a.bytes(3, &host, &len) || !frames_fit(off, 1, 0, len, d->bytes))
        return range_error(env, up ? "deviceUpload(ctx, dev, byteOffset, Uint8Array): outside the device buffer" : "deviceDownload(ctx, dev, byteOffset, Uint8Array): outside the device buffer");
    char *dev = static_cast<char *>(d->ptr) + off;
    ht_status st = up ? ht_device_upload(L.ctx, dev, host, len) : ht_device_download(L.ctx, host, dev, len);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, up ? "ht_device_upload" : "ht_device_download");
    return nullptr;
}
napi_value DeviceUpload(napi_env env, napi_callback_info info) { return device_copy(env, info, true); }
napi_value DeviceDownload(napi_env env, napi_callback_info info) { return device_copy(env, info, false); }

napi_value BindDevice(napi_env env, napi_callback_info info) {
    Args a(env, info, 5);
    Locked L;
    DevBuf *d = nullptr;
    size_t off = 0, stride = 0;
    int32_t n = 0;
    if (!a.ctx(5, &L) || !a.devbuf(1, &d)) return nullptr;
    if (!a.offset(2, &off) || !a.i32(3, &n) || !a.offset(4, &stride) || n <= 0 || !frames_fit(off, (size_t)n, stride, stride, d->bytes))
        return range_error(env, "bindDevice(ctx, dev, byteOffset, n, frameStride): outside the device buffer");
    ht_status st = ht_bind_frames_device(L.ctx, static_cast<char *>(d->ptr) + off, n, stride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_bind_frames_device");
    return nullptr;
}

napi_value UploadAsync(napi_env env, napi_callback_info info) {
    Args a(env, info, 3);
    Locked L;
    uint8_t *src = nullptr;
    size_t len = 0;
    int32_t n = 0;
    if (!a.ctx(3, &L)) return nullptr;
    if (!a.bytes(1, &src, &len) || !a.i32(2, &n) || n <= 0 || len % (size_t)n) return type_error(env, "uploadAsync(ctx, Uint8Array rgba (n frames, ideally from hostAlloc), n)");
    ht_status st = ht_upload_frames_async(L.ctx, src, n, len / (size_t)n);  // rgba must stay untouched until swapFrames
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_upload_frames_async");
    return nullptr;
}

napi_value SwapFrames(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    Locked L;
    if (!a.ctx(1, &L)) return nullptr;
    ht_status st = ht_swap_frames(L.ctx);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_swap_frames");
    return nullptr;
}

napi_value DetectEnqueue(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t fl = 0;
    if (!a.ctx(1, &L)) return nullptr;
    a.opt_i32(1, &fl);
    ht_status st = ht_detect_enqueue(L.ctx, (uint32_t)fl);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_enqueue");
    return nullptr;
}

napi_value DetectCollect(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    Locked L;
    if (!a.ctx(1, &L)) return nullptr;
    DetectJob j;
    j.n = ht_frames_enqueued(L.ctx);  // the batch in flight, not whatever is bound by now
    j.hits.resize(1u << 16);
    j.counts.assign((size_t)j.n, 0);
    j.st = ht_detect_collect(L.ctx, j.hits.data(), (uint32_t)j.hits.size(), j.counts.data(), &j.total);
    if (j.st == HT_ERR_CAPACITY && j.total > j.hits.size()) {
        napi_throw_error(env, nullptr, "detectCollect: more than 65536 raw hits in one batch; use collectBest or smaller batches");
        return nullptr;
    }
    if (j.st != HT_OK) return throw_ht(env, L.ctx, j.st, "ht_detect_collect");
    return pack_hits(env, j);
}

napi_value CollectBest(napi_env env, napi_callback_info info) {
    Args a(env, info, 3);
    Locked L;
    int32_t mn = 1, rq = -1;
    if (!a.ctx(1, &L)) return nullptr;
    a.opt_i32(1, &mn);
    a.opt_i32(2, &rq);
    const int32_t n = ht_frames_enqueued(L.ctx);
    std::vector<ht_rect> best((size_t)(n > 0 ? n : 1));
    uint32_t total = 0;
    ht_status st = rq >= 0 ? ht_detect_collect_best_requeue(L.ctx, mn, best.data(), &total, (uint32_t)rq) : ht_detect_collect_best(L.ctx, mn, best.data(), &total);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_collect_best");
    napi_value obj, v, ta = rect6_result(env, best.data(), (size_t)(n > 0 ? n : 0));
    if (!ta) return nullptr;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_set_named_property(env, obj, "best", ta));
    NAPI_OK(napi_create_uint32(env, total, &v));
    NAPI_OK(napi_set_named_property(env, obj, "hits", v));
    return obj;
}

// ---- the device route of the same post-processing (ht_group.hip).  Each entry point calls its export directly (no table of function
// pointers): the symbols stay lazily bound, so an addon linked against a C ABI without them still loads.

napi_value DetectBestEnqueue(napi_env env, napi_callback_info info) {
    Args a(env, info, 3);
    Locked L;
    int32_t mn = 1, base = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &mn)) return type_error(env, "detectBestEnqueue(ctx, minNeighbors, frameBase = 0)");
    a.opt_i32(2, &base);
    const ht_status st = ht_detect_best_enqueue(L.ctx, mn, base);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_best_enqueue");
    return nullptr;
}

napi_value CollectBestDevice(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t rq = -1;
    if (!a.ctx(1, &L)) return nullptr;
    a.opt_i32(1, &rq);
    const int32_t n = ht_frames_enqueued(L.ctx);
    std::vector<ht_rect> best((size_t)(n > 0 ? n : 1));
    uint32_t total = 0;
    ht_status st;
    if (rq >= 0) st = ht_detect_best_collect_requeue(L.ctx, best.data(), &total, (uint32_t)rq);
    else st = ht_detect_best_collect(L.ctx, best.data(), &total);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_best_collect");
    napi_value obj, v, ta = rect6_result(env, best.data(), (size_t)(n > 0 ? n : 0));
    if (!ta) return nullptr;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_set_named_property(env, obj, "best", ta));
    NAPI_OK(napi_create_uint32(env, total, &v));
    NAPI_OK(napi_set_named_property(env, obj, "hits", v));
    return obj;
}

napi_value DetectGrouped(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t frame = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &frame)) return type_error(env, "detectGrouped(ctx, frame)");
    uint32_t n = 0;
    ht_status st = ht_detect_grouped(L.ctx, frame, nullptr, 0, &n);  // the length first
    if (st != HT_OK && st != HT_ERR_CAPACITY) return throw_ht(env, L.ctx, st, "ht_detect_grouped");
    std::vector<ht_rect> g((size_t)(n ? n : 1));
    if (n && (st = ht_detect_grouped(L.ctx, frame, g.data(), n, &n)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_grouped");
    return rect6_result(env, g.data(), n);
}

napi_value DetectBestRecords(napi_env env, napi_callback_info info) {
    Args a(env, info, 1);
    Locked L;
    if (!a.ctx(1, &L)) return nullptr;
    const void *rec = nullptr;
    int32_t n = 0;
    ht_status st = ht_detect_best_records_device(L.ctx, &rec, &n);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_detect_best_records_device");
    double *d = nullptr;
    napi_value ta = f64_result(env, (size_t)n * 8, &d);
    if (!ta) return nullptr;
    if (n > 0 && (st = ht_device_download(L.ctx, d, rec, (size_t)n * 64)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_device_download");
    return ta;
}

napi_value GroupHits(napi_env env, napi_callback_info info) {
    static const char *usage = "groupHits(ctx, Uint8Array hits /* 24-byte ht_hit records */, nframes, minNeighbors)";
    Args a(env, info, 4);
    Locked L;
    uint8_t *bytes = nullptr;
    size_t len = 0;
    int32_t nframes = 0, mn = 1;
    if (!a.ctx(4, &L)) return nullptr;
    if (!a.bytes(1, &bytes, &len) || !a.i32(2, &nframes) || !a.i32(3, &mn) || len % sizeof(ht_hit)) return type_error(env, usage);
    if (nframes <= 0 || nframes > (1 << 20) || len / sizeof(ht_hit) > 0xffffffffu) return range_error(env, usage);
    const size_t n = len / sizeof(ht_hit);
    std::vector<ht_hit> hits(n ? n : 1);  // a typed array's storage need not be aligned for ht_hit
    if (n) std::memcpy(hits.data(), bytes, len);
    std::vector<ht_rect> best((size_t)nframes), grouped(n ? n : 1);
    std::vector<uint32_t> ng((size_t)nframes);
    const ht_status st = ht_group_hits(L.ctx, n ? hits.data() : nullptr, (uint32_t)n, nframes, mn, best.data(), grouped.data(), ng.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_group_hits");
    size_t total = 0;
    for (uint32_t k : ng) total += k;
    if (total > n) return throw_ht(env, L.ctx, HT_ERR_INVALID, "ht_group_hits (group counts)");
    napi_value obj, ab, counts, tb = rect6_result(env, best.data(), (size_t)nframes), tg = tb ? rect6_result(env, grouped.data(), total) : nullptr;
    if (!tb || !tg) return nullptr;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, ng.size() * 4, &p, &ab));
    std::memcpy(p, ng.data(), ng.size() * 4);
    NAPI_OK(napi_create_typedarray(env, napi_uint32_array, ng.size(), ab, 0, &counts));
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_set_named_property(env, obj, "best", tb));
    NAPI_OK(napi_set_named_property(env, obj, "grouped", tg));
    NAPI_OK(napi_set_named_property(env, obj, "counts", counts));
    return obj;
}

napi_value DrawFramesDevice(napi_env env, napi_callback_info info) {
    static const char *usage = "drawFramesDevice(ctx, srcDev, srcOffset, n, sw, sh, pitch, stride, rect | null, dstDev | null, dstOffset, dstStride, wait)";
    Args a(env, info, 13);
    Locked L;
    DevBuf *src = nullptr, *dst = nullptr;
    int32_t n = 0, sw = 0, sh = 0;
    size_t soff = 0, pitch = 0, stride = 0, doff = 0, dstride = 0;
    ht_cs_rect r;
    const ht_cs_rect *rp = nullptr;
    bool wait = false;
    if (!a.ctx(12, &L) || !a.devbuf(1, &src) || !a.devbuf_or_null(9, &dst)) return nullptr;
    if (!a.offset(2, &soff) || !a.i32(3, &n) || !a.i32(4, &sw) || !a.i32(5, &sh) || !a.offset(6, &pitch) || !a.offset(7, &stride) || !get_rect(env, a.argv[8], &r, &rp) ||
        !a.offset(10, &doff) || !a.offset(11, &dstride) || n <= 0 || sw <= 0 || sh <= 0)
        return type_error(env, usage);
    a.opt_bool(12, &wait);
    // what the library checks itself — strides smaller than a frame, alignment, overlap — is left to it
    const size_t p = pitch ? pitch : (size_t)sw * 4;
    bool inside = p <= src->bytes / (size_t)sh;  // p * sh: one source frame
    const size_t sframe = inside ? p * (size_t)sh : 0, ss = stride ? stride : sframe;
    inside = inside && frames_fit(soff, (size_t)n, ss, sframe, src->bytes);
    if (dst) {
        const size_t fb = frame_bytes(env, L.ctx, 4, "drawFramesDevice");
        if (!fb) return nullptr;
        inside = inside && frames_fit(doff, (size_t)n, dstride ? dstride : fb, fb, dst->bytes);
    }
    if (!inside) return range_error(env, (std::string(usage) + ": outside the device buffer").c_str());
    ht_status st = ht_draw_frames_device(L.ctx, static_cast<char *>(src->ptr) + soff, n, sw, sh, pitch, stride, rp, dst ? static_cast<char *>(dst->ptr) + doff : nullptr, dstride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_draw_frames_device");
    if (wait && (st = ht_synchronize(L.ctx)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_synchronize");
    return nullptr;
}

napi_value DrawFramesYuvDevice(napi_env env, napi_callback_info info) {
    static const char *usage = "drawFramesYuvDevice(ctx, srcDev, srcOffset, n, w, h, format, matrix, stride, rect | null, dstDev | null, dstOffset, dstStride, wait)";
    Args a(env, info, 14);
    Locked L;
    DevBuf *src = nullptr, *dst = nullptr;
    int32_t n = 0, w = 0, h = 0, format = 0, matrix = 0;
    size_t soff = 0, stride = 0, doff = 0, dstride = 0;
    ht_cs_rect r;
    const ht_cs_rect *rp = nullptr;
    bool wait = false;
    if (!a.ctx(13, &L) || !a.devbuf(1, &src) || !a.devbuf_or_null(10, &dst)) return nullptr;
    if (!a.offset(2, &soff) || !a.i32(3, &n) || !a.i32(4, &w) || !a.i32(5, &h) || !a.i32(6, &format) || !a.i32(7, &matrix) || !a.offset(8, &stride) ||
        !get_rect(env, a.argv[9], &r, &rp) || !a.offset(11, &doff) || !a.offset(12, &dstride) || n <= 0)
        return type_error(env, usage);
    a.opt_bool(13, &wait);
    // what the library checks itself — format, matrix, strides smaller than a plane, alignment, overlap — is left to it
    const size_t fsz = yuv_frame_bytes(w, h, format);
    const bool packed = yuv_packed_422(format);
    if (packed && (soff & 3)) return range_error(env, "drawFramesYuvDevice: srcOffset of a YUYV / UYVY frame must be a multiple of 4");
    bool inside = fsz && frames_fit(soff, (size_t)n, stride ? stride : fsz, fsz, src->bytes);
    if (dst) {
        const size_t fb = frame_bytes(env, L.ctx, 4, "drawFramesYuvDevice");
        if (!fb) return nullptr;
        inside = inside && frames_fit(doff, (size_t)n, dstride ? dstride : fb, fb, dst->bytes);
    }
    if (!inside) return range_error(env, (std::string(usage) + ": outside the device buffer").c_str());
    ht_yuv_frames d;
    std::memset(&d, 0, sizeof(d));
    const char *base = static_cast<char *>(src->ptr) + soff;
    const size_t cplane = (size_t)((w + 1) / 2) * ((h + 1) / 2);
    d.y = base;  // YUYV / UYVY: the one packed plane; u and v stay NULL
    if (!packed) d.u = base + (size_t)w * h, d.v = bare_format(format) == HT_YUV_I420 ? base + (size_t)w * h + cplane : nullptr;
    d.frame_stride = stride ? stride : (n > 1 ? fsz : 0);
    d.width = w, d.height = h, d.format = format, d.matrix = matrix;
    ht_status st = ht_draw_frames_yuv_device(L.ctx, &d, n, rp, dst ? static_cast<char *>(dst->ptr) + doff : nullptr, dstride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_draw_frames_yuv_device");
    if (wait && (st = ht_synchronize(L.ctx)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_synchronize");
    return nullptr;
}

// one entry of drawListDevice: the properties through the getters every entry point uses, the frame checked against its buffer
bool get_draw_entry(napi_env env, napi_value e, ht_draw_source *s) {
    napi_valuetype vt;
    napi_value v;
    DevBuf *dev = nullptr;
    size_t off = 0;
    std::memset(s, 0, sizeof(*s));
    if (napi_typeof(env, e, &vt) != napi_ok || vt != napi_object) return type_error(env, "drawListDevice: an entry is {dev, offset, width, height, format, matrix, rect}") != nullptr;
    if (!get_prop(env, e, "dev", &v) || !get_devbuf(env, v, &dev)) {
        bool pending = false;
        if (napi_is_exception_pending(env, &pending) == napi_ok && !pending) type_error(env, "drawListDevice: entry.dev must be a live device buffer");
        return false;
    }
    if (!get_prop(env, e, "width", &v) || !get_i32(env, v, &s->width) || !get_prop(env, e, "height", &v) || !get_i32(env, v, &s->height))
        return type_error(env, "drawListDevice: entry.width and entry.height are integers") != nullptr;
    if (!get_prop(env, e, "format", &v) || !get_i32(env, v, &s->format)) return type_error(env, "drawListDevice: entry.format is YUV_NV12, YUV_I420, YUV_YUYV, YUV_UYVY or DRAW_RGBA") != nullptr;
    // optional like the trailing arguments of the entry points: absent or undefined is 0; anything else has to be a byte offset
    if (get_prop(env, e, "offset", &v) && napi_typeof(env, v, &vt) == napi_ok && vt != napi_undefined && !get_offset(env, v, &off))
        return type_error(env, "drawListDevice: entry.offset is a byte offset") != nullptr;
    prop_i32(env, e, "matrix", &s->matrix);
    const ht_cs_rect *rp = nullptr;
    if (get_prop(env, e, "rect", &v) && !get_rect(env, v, &s->rect, &rp)) return type_error(env, "drawListDevice: entry.rect is null or an Int32Array [x, y, width, height]") != nullptr;
    if (rp && rp->width == 0 && rp->height == 0) s->rect.width = -1;  // an empty rect is an error, not "the whole source": the library refuses it
    // what the library checks itself — format, matrix, alignment, the rect, overlap — is left to it
    const bool rgba = bare_format(s->format) == HT_DRAW_RGBA;
    const size_t ysz = s->width > 0 && s->height > 0 && s->width <= 16384 && s->height <= 16384 ? (size_t)s->width * (size_t)s->height : 0;
    const bool packed = yuv_packed_422(s->format);
    const size_t fsz = rgba ? ysz * 4 : yuv_frame_bytes(s->width, s->height, s->format);
    if (!fsz || !frames_fit(off, 1, fsz, fsz, dev->bytes)) return range_error(env, "drawListDevice: an entry's frame lies outside its device buffer") != nullptr;
    if (packed && (off & 3)) return range_error(env, "drawListDevice: entry.offset of a YUYV / UYVY frame must be a multiple of 4") != nullptr;
    const char *base = static_cast<char *>(dev->ptr) + off;
    s->p0 = base;
    if (!rgba && !packed) {
        s->p1 = base + ysz;
        s->p2 = bare_format(s->format) == HT_YUV_I420 ? base + ysz + (size_t)((s->width + 1) / 2) * ((s->height + 1) / 2) : nullptr;
    }
    return true;
}

// drawListDevice and drawListFilteredDevice: ONE reader and ONE range check; the filtered form has maxFactor (1..8) behind the entries
napi_value draw_list_call(napi_env env, napi_callback_info info, bool filtered) {
    const char *usage = filtered ? "drawListFilteredDevice(ctx, entries, maxFactor, dstDev | null, dstStride, dstOffset = 0, wait = false)"
                                 : "drawListDevice(ctx, entries, dstDev | null, dstStride, dstOffset = 0, wait = false)";
    const char *cname = filtered ? "ht_draw_list_filtered_device" : "ht_draw_list_device";
    const size_t k = filtered ? 1 : 0;  // the arguments behind maxFactor lie one further
    Args a(env, info, 6 + k);
    Locked L;
    DevBuf *dst = nullptr;
    size_t dstride = 0, doff = 0;
    bool wait = false, is_array = false;
    uint32_t n = 0;
    int32_t max_factor = 0;
    if (!a.ctx(4 + k, &L) || !a.devbuf_or_null(2 + k, &dst)) return nullptr;
    if (napi_is_array(env, a.argv[1], &is_array) != napi_ok || !is_array || napi_get_array_length(env, a.argv[1], &n) != napi_ok || (filtered && !a.i32(2, &max_factor)) ||
        !a.offset(3 + k, &dstride) || (a.argc > 4 + k && !a.offset(4 + k, &doff)))
        return type_error(env, usage);
    a.opt_bool(5 + k, &wait);
    if (n < 1 || n > 65535) return range_error(env, (std::string(usage) + ": 1..65535 entries").c_str());
    if (filtered && (max_factor < 1 || max_factor > 8)) return range_error(env, (std::string(usage) + ": maxFactor is 1..8").c_str());
    std::vector<ht_draw_source> srcs(n);
    for (uint32_t i = 0; i < n; i++) {
        napi_value e;
        NAPI_OK(napi_get_element(env, a.argv[1], i, &e));
        if (!get_draw_entry(env, e, &srcs[i])) return nullptr;
    }
    if (dst) {
        const size_t fb = frame_bytes(env, L.ctx, 4, filtered ? "drawListFilteredDevice" : "drawListDevice");
        if (!fb) return nullptr;
        if (!frames_fit(doff, (size_t)n, dstride ? dstride : fb, fb, dst->bytes)) return range_error(env, (std::string(usage) + ": outside the device buffer").c_str());
    }
    void *out = dst ? static_cast<char *>(dst->ptr) + doff : nullptr;
    ht_status st = filtered ? ht_draw_list_filtered_device(L.ctx, srcs.data(), (int32_t)n, max_factor, out, dstride) : ht_draw_list_device(L.ctx, srcs.data(), (int32_t)n, out, dstride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, cname);
    if (wait && (st = ht_synchronize(L.ctx)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_synchronize");
    return nullptr;
}
napi_value DrawListDevice(napi_env env, napi_callback_info info) { return draw_list_call(env, info, false); }
napi_value DrawListFilteredDevice(napi_env env, napi_callback_info info) { return draw_list_call(env, info, true); }

// drawFilterFactors(Int32Array sizes[2n] = source (or rect) width, height per entry, canvasWidth, canvasHeight, maxFactor) -> Int32Array [2n] = Nx, Ny
// per entry: the library's own rule (ht_draw_filter_factors), no context
napi_value DrawFilterFactors(napi_env env, napi_callback_info info) {
    static const char *usage = "drawFilterFactors(Int32Array sizes[2n], canvasWidth, canvasHeight, maxFactor)";
    Args a(env, info, 4);
    View sizes;
    int32_t w = 0, h = 0, mf = 0;
    if (!a.arity(4)) return nullptr;
    if (!a.i32s(0, 0, &sizes) || sizes.len % 2 || !a.i32(1, &w) || !a.i32(2, &h) || !a.i32(3, &mf)) return type_error(env, usage);
    if (w < 1 || h < 1 || mf < 1 || mf > 8) return range_error(env, (std::string(usage) + ": the canvas is positive, maxFactor is 1..8").c_str());
    const size_t n = sizes.len / 2;
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, n * 8, &p, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, n * 2, ab, 0, &ta));
    int32_t *out = static_cast<int32_t *>(p);
    const int32_t *v = sizes.as<int32_t>();
    for (size_t i = 0; i < n; i++)
        if (ht_draw_filter_factors(v[2 * i], v[2 * i + 1], w, h, mf, out + 2 * i, out + 2 * i + 1) != HT_OK)
            return range_error(env, (std::string(usage) + ": a source width / height is 1..16384").c_str());
    return ta;
}

// ---- face crops and angle-aligned face crops: each tracker's box cut from its feed (ht_camshift_crop_*_device / ht_camshift_align_*_device) ----

// the arguments every launching call shares behind its list: Int32Array params [width, height, marginQ8, flags] at argument i, then outDev, outStride,
// outOffset = 0, wait = false.  The patch size is checked here because the range handed to the library with the buffer's pointer depends on it;
// margin and flags are the library's to refuse.
struct CropOut {
    ht_crop_params prm;
    char *out = nullptr;
    size_t stride = 0;
    bool wait = false;
};
// fmt (the tensor forms, and the filtered forms with a format): a patch is the tensor's C * width * height elements and the default stride
// its bytes rounded up to 4.  between: the arguments between the params and outDev (the tensor forms' format object: 1; the filtered forms'
// maxFactor and format | null: 2)
bool get_crop_out(const Args &a, size_t i, size_t n, const char *usage, CropOut *c, const ht_patch_format *fmt, size_t between) {
    View prm;
    DevBuf *out = nullptr;
    size_t off = 0;
    const size_t o = i + 1 + between;  // outDev: behind the params, or behind what the form has between the two
    if (!a.devbuf(o, &out)) return false;
    if (!a.i32s(i, 4, &prm) || prm.len != 4 || !a.offset(o + 1, &c->stride) || (a.argc > o + 2 && !a.offset(o + 2, &off))) return type_error(a.env, usage) != nullptr;
    a.opt_bool(o + 3, &c->wait);
    const int32_t *v = prm.as<int32_t>();
    c->prm.out_width = v[0], c->prm.out_height = v[1], c->prm.margin_q8 = v[2], c->prm.flags = (uint32_t)v[3];
    if (v[0] < 1 || v[0] > 1024 || v[1] < 1 || v[1] > 1024) return range_error(a.env, (std::string(usage) + ": width and height are 1..1024").c_str()) != nullptr;
    const size_t pb = (size_t)v[0] * (size_t)v[1] * (fmt ? (size_t)(fmt->channels == HT_PATCH_GRAY ? 1 : 3) * (fmt->dtype == HT_PATCH_F32 ? 4 : 2) : 4);
    if (!frames_fit(off, n, c->stride ? c->stride : (pb + 3) & ~(size_t)3, pb, out->bytes)) return range_error(a.env, (std::string(usage) + ": outside the device buffer").c_str()) != nullptr;
    c->out = static_cast<char *>(out->ptr) + off;
    return true;
}

// the format object of the tensor forms (ht_patch_format): {dtype, layout, channels: integers, scale, bias: Float32Array[3]}, in front of
// outDev.  Its kinds are checked here; its values are the library's to refuse.
bool get_patch_format(napi_env env, napi_value v, const char *usage, ht_patch_format *f) {
    napi_valuetype vt;
    napi_value p;
    View scale, bias;
    std::memset(f, 0, sizeof(*f));
    if (napi_typeof(env, v, &vt) != napi_ok || vt != napi_object || !get_prop(env, v, "dtype", &p) || !get_i32(env, p, &f->dtype) || !get_prop(env, v, "layout", &p) ||
        !get_i32(env, p, &f->layout) || !get_prop(env, v, "channels", &p) || !get_i32(env, p, &f->channels) || !get_prop(env, v, "scale", &p) ||
        !scale.get(env, p, napi_float32_array, 3) || scale.len != 3 || !get_prop(env, v, "bias", &p) || !bias.get(env, p, napi_float32_array, 3) || bias.len != 3)
        return type_error(env, usage) != nullptr;
    std::memcpy(f->scale, scale.as<float>(), sizeof f->scale);
    std::memcpy(f->bias, bias.as<float>(), sizeof f->bias);
    return true;
}

// the filtered forms (ht_camshift_*_filtered_device) have maxFactor (1..8) and format | null behind the params: argument i and i + 1
bool get_filter_args(const Args &a, size_t i, const char *usage, int32_t *max_factor, bool *has_fmt) {
    napi_valuetype vt;
    if (!a.i32(i, max_factor) || napi_typeof(a.env, a.argv[i + 1], &vt) != napi_ok) return type_error(a.env, usage) != nullptr;
    if (*max_factor < 1 || *max_factor > 8) return range_error(a.env, (std::string(usage) + ": maxFactor is 1..8").c_str()) != nullptr;
    *has_fmt = vt != napi_null && vt != napi_undefined;  // null: RGBA8
    return true;
}

// The 12 launching calls: family (crop, align) x list (pairs, sources) x mode (0: RGBA8; 1: the tensor form, the format object in front of
// outDev; 2: the filtered form, maxFactor and format | null there).  ONE pairs call and ONE sources call read the arguments; FaceFns is the
// table that gives each (family, mode) its C function and that function's name for throw_ht, FACE_USAGE the usage strings.
template <class F>
struct Named {
    F *fn;
    const char *name;
};
#define NAMED(f) {f, #f}
template <class P>  // the family's params: ht_crop_params or ht_align_params, the same four fields
struct FaceFns {
    const char *word;  // the family's word, in front of every usage string
    Named<ht_status(ht_ctx *, const ht_cs_pair *, int32_t, const P *, void *, size_t)> pairs;
    Named<ht_status(ht_ctx *, const ht_cs_pair *, int32_t, const P *, const ht_patch_format *, void *, size_t)> pairs_tensor;
    Named<ht_status(ht_ctx *, const ht_cs_pair *, int32_t, const P *, int32_t, const ht_patch_format *, void *, size_t)> pairs_filtered;
    Named<ht_status(ht_ctx *, const int32_t *, const ht_draw_source *, int32_t, const P *, void *, size_t)> sources;
    Named<ht_status(ht_ctx *, const int32_t *, const ht_draw_source *, int32_t, const P *, const ht_patch_format *, void *, size_t)> sources_tensor;
    Named<ht_status(ht_ctx *, const int32_t *, const ht_draw_source *, int32_t, const P *, int32_t, const ht_patch_format *, void *, size_t)> sources_filtered;
};
const FaceFns<ht_crop_params> CROP_FNS = {"crop", NAMED(ht_camshift_crop_pairs_device), NAMED(ht_camshift_crop_pairs_tensor_device), NAMED(ht_camshift_crop_pairs_filtered_device),
                                          NAMED(ht_camshift_crop_sources_device), NAMED(ht_camshift_crop_sources_tensor_device), NAMED(ht_camshift_crop_sources_filtered_device)};
const FaceFns<ht_align_params> ALIGN_FNS = {"align", NAMED(ht_camshift_align_pairs_device), NAMED(ht_camshift_align_pairs_tensor_device), NAMED(ht_camshift_align_pairs_filtered_device),
                                            NAMED(ht_camshift_align_sources_device), NAMED(ht_camshift_align_sources_tensor_device), NAMED(ht_camshift_align_sources_filtered_device)};
const char *const FACE_USAGE[2][3] = {  // [list: 0 pairs, 1 sources][mode], behind the family's word
    {"PairsDevice(ctx, Int32Array pairs[2n], Int32Array params[4], outDev, outStride, outOffset = 0, wait = false)",
     "PairsTensorDevice(ctx, Int32Array pairs[2n], Int32Array params[4], format, outDev, outStride, outOffset = 0, wait = false)",
     "PairsFilteredDevice(ctx, Int32Array pairs[2n], Int32Array params[4], maxFactor, format | null, outDev, outStride, outOffset = 0, wait = false)"},
    {"SourcesDevice(ctx, Int32Array streams[n], entries[n], Int32Array params[4], outDev, outStride, outOffset = 0, wait = false)",
     "SourcesTensorDevice(ctx, Int32Array streams[n], entries[n], Int32Array params[4], format, outDev, outStride, outOffset = 0, wait = false)",
     "SourcesFilteredDevice(ctx, Int32Array streams[n], entries[n], Int32Array params[4], maxFactor, format | null, outDev, outStride, outOffset = 0, wait = false)"}};

// what every launching call has behind its list: the params at argument i, the mode's maxFactor and format, then the output
struct FaceOut {
    CropOut c;
    int32_t max_factor = 0;
    bool has_fmt = false;
    ht_patch_format fmt;
    const ht_patch_format *format() const { return has_fmt ? &fmt : nullptr; }
    template <class P>
    P params() const {
        P p;
        p.out_width = c.prm.out_width, p.out_height = c.prm.out_height, p.margin_q8 = c.prm.margin_q8, p.flags = c.prm.flags;
        return p;
    }
};
bool get_face_out(const Args &a, size_t i, size_t n, int mode, const char *usage, FaceOut *o) {
    const bool tensor = mode == 1, filtered = mode == 2;
    o->has_fmt = tensor;
    if (filtered && !get_filter_args(a, i + 1, usage, &o->max_factor, &o->has_fmt)) return false;
    if (o->has_fmt && !get_patch_format(a.env, a.argv[i + 1 + (filtered ? 1 : 0)], usage, &o->fmt)) return false;
    return get_crop_out(a, i, n, usage, &o->c, o->format(), filtered ? 2 : tensor ? 1 : 0);
}

template <class P>
napi_value face_pairs_call(napi_env env, napi_callback_info info, const FaceFns<P> &f, int mode) {
    const std::string usage_s = std::string(f.word) + FACE_USAGE[0][mode];
    const char *usage = usage_s.c_str();
    Args a(env, info, 7 + (size_t)mode);  // mode: also the number of arguments between the params and outDev
    Locked L;
    const ht_cs_pair *pairs = nullptr;
    int32_t n = 0;
    FaceOut o;
    if (!a.ctx(5 + (size_t)mode, &L)) return nullptr;
    if (!get_pairs(env, a.argv[1], &pairs, &n)) return type_error(env, usage);
    if (n > 65535) return range_error(env, (std::string(usage) + ": 1..65535 pairs").c_str());
    if (!get_face_out(a, 2, (size_t)n, mode, usage, &o)) return nullptr;
    const P prm = o.template params<P>();
    ht_status st = mode == 2   ? f.pairs_filtered.fn(L.ctx, pairs, n, &prm, o.max_factor, o.format(), o.c.out, o.c.stride)
                   : mode == 1 ? f.pairs_tensor.fn(L.ctx, pairs, n, &prm, &o.fmt, o.c.out, o.c.stride)
                               : f.pairs.fn(L.ctx, pairs, n, &prm, o.c.out, o.c.stride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, mode == 2 ? f.pairs_filtered.name : mode == 1 ? f.pairs_tensor.name : f.pairs.name);
    if (o.c.wait && (st = ht_synchronize(L.ctx)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_synchronize");
    return nullptr;
}

template <class P>
napi_value face_sources_call(napi_env env, napi_callback_info info, const FaceFns<P> &f, int mode) {
    const std::string usage_s = std::string(f.word) + FACE_USAGE[1][mode];
    const char *usage = usage_s.c_str();
    Args a(env, info, 8 + (size_t)mode);
    Locked L;
    View streams;
    bool is_array = false;
    uint32_t n = 0;
    FaceOut o;
    if (!a.ctx(6 + (size_t)mode, &L)) return nullptr;
    if (!a.i32s(1, 0, &streams) || napi_is_array(env, a.argv[2], &is_array) != napi_ok || !is_array || napi_get_array_length(env, a.argv[2], &n) != napi_ok)
        return type_error(env, usage);
    if (n < 1 || n > 65535) return range_error(env, (std::string(usage) + ": 1..65535 entries").c_str());
    if (streams.len != n) return range_error(env, (std::string(usage) + ": one stream per entry").c_str());
    std::vector<ht_draw_source> srcs(n);
    for (uint32_t i = 0; i < n; i++) {  // an entry is drawListDevice's: {dev, offset, width, height, format, matrix, rect}
        napi_value e;
        NAPI_OK(napi_get_element(env, a.argv[2], i, &e));
        if (!get_draw_entry(env, e, &srcs[i])) return nullptr;
    }
    if (!get_face_out(a, 3, (size_t)n, mode, usage, &o)) return nullptr;
    const P prm = o.template params<P>();
    const int32_t *st_ids = streams.as<int32_t>();
    ht_status st = mode == 2   ? f.sources_filtered.fn(L.ctx, st_ids, srcs.data(), (int32_t)n, &prm, o.max_factor, o.format(), o.c.out, o.c.stride)
                   : mode == 1 ? f.sources_tensor.fn(L.ctx, st_ids, srcs.data(), (int32_t)n, &prm, &o.fmt, o.c.out, o.c.stride)
                               : f.sources.fn(L.ctx, st_ids, srcs.data(), (int32_t)n, &prm, o.c.out, o.c.stride);
    if (st != HT_OK) return throw_ht(env, L.ctx, st, mode == 2 ? f.sources_filtered.name : mode == 1 ? f.sources_tensor.name : f.sources.name);
    if (o.c.wait && (st = ht_synchronize(L.ctx)) != HT_OK) return throw_ht(env, L.ctx, st, "ht_synchronize");
    return nullptr;
}

napi_value CropPairsDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, CROP_FNS, 0); }
napi_value CropPairsTensorDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, CROP_FNS, 1); }
napi_value CropPairsFilteredDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, CROP_FNS, 2); }
napi_value CropSourcesDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, CROP_FNS, 0); }
napi_value CropSourcesTensorDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, CROP_FNS, 1); }
napi_value CropSourcesFilteredDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, CROP_FNS, 2); }
napi_value AlignPairsDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, ALIGN_FNS, 0); }
napi_value AlignPairsTensorDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, ALIGN_FNS, 1); }
napi_value AlignPairsFilteredDevice(napi_env env, napi_callback_info info) { return face_pairs_call(env, info, ALIGN_FNS, 2); }
napi_value AlignSourcesDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, ALIGN_FNS, 0); }
napi_value AlignSourcesTensorDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, ALIGN_FNS, 1); }
napi_value AlignSourcesFilteredDevice(napi_env env, napi_callback_info info) { return face_sources_call(env, info, ALIGN_FNS, 2); }

// {records: Int32Array [6n] = code, stream, x, y, width, height per entry; ratios: Float64Array [2n] = rx, ry}
napi_value CropResult(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0 || n > 65535) return type_error(env, "cropResult(ctx, n)");
    std::vector<ht_crop_record> rec((size_t)n);
    ht_status st = ht_camshift_crop_result(L.ctx, n, rec.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_crop_result");
    napi_value obj, ab, ta;
    void *p = nullptr;
    double *ratios = nullptr;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 24, &p, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)n * 6, ab, 0, &ta));
    NAPI_OK(napi_set_named_property(env, obj, "records", ta));
    napi_value rt = f64_result(env, (size_t)n * 2, &ratios);
    if (!rt) return nullptr;
    NAPI_OK(napi_set_named_property(env, obj, "ratios", rt));
    for (int32_t i = 0; i < n; i++) {
        memcpy(static_cast<char *>(p) + (size_t)i * 24, &rec[(size_t)i], 24);  // code, stream and the rect lead the record
        ratios[2 * i] = rec[(size_t)i].rx, ratios[2 * i + 1] = rec[(size_t)i].ry;
    }
    return obj;
}

// ---- angle-aligned face crops: each tracker's rotated box, upright (ht_camshift_align_*_device): the launching calls are above -------------

// {records: Int32Array [4n] = code, stream, a12, 0 per entry; terms: Float64Array [6n] = cx, cy, ux, uy, vx, vy in Q16 source pixels
// (|value| < 2^52: exact in a binary64)}
napi_value AlignResult(napi_env env, napi_callback_info info) {
    Args a(env, info, 2);
    Locked L;
    int32_t n = 0;
    if (!a.ctx(2, &L)) return nullptr;
    if (!a.i32(1, &n) || n <= 0 || n > 65535) return type_error(env, "alignResult(ctx, n)");
    std::vector<ht_align_record> rec((size_t)n);
    ht_status st = ht_camshift_align_result(L.ctx, n, rec.data());
    if (st != HT_OK) return throw_ht(env, L.ctx, st, "ht_camshift_align_result");
    napi_value obj, ab, ta;
    void *p = nullptr;
    double *terms = nullptr;
    NAPI_OK(napi_create_object(env, &obj));
    NAPI_OK(napi_create_arraybuffer(env, (size_t)n * 16, &p, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, (size_t)n * 4, ab, 0, &ta));
    NAPI_OK(napi_set_named_property(env, obj, "records", ta));
    napi_value tt = f64_result(env, (size_t)n * 6, &terms);
    if (!tt) return nullptr;
    NAPI_OK(napi_set_named_property(env, obj, "terms", tt));
    for (int32_t i = 0; i < n; i++) {
        const ht_align_record &r = rec[(size_t)i];
        memcpy(static_cast<char *>(p) + (size_t)i * 16, &r, 16);  // code, stream, a12 and pad lead the record
        const int64_t q[6] = {r.cx, r.cy, r.ux, r.uy, r.vx, r.vy};
        for (int k = 0; k < 6; k++) terms[6 * i + k] = (double)q[k];
    }
    return obj;
}

// cropFilterFactors(records Int32Array[6n] as cropResult gives them, width, height, maxFactor) and
// alignFilterFactors(records Int32Array[4n], terms Float64Array[6n] as alignResult gives them, width, height, maxFactor)
// -> Int32Array [2n] = Nx, Ny per entry (0, 0 for an empty one): the library's own rule (ht_camshift_*_filter_factors), no context
napi_value filter_factors_call(napi_env env, napi_callback_info info, bool align) {
    const char *usage = align ? "alignFilterFactors(Int32Array records[4n], Float64Array terms[6n], width, height, maxFactor)" : "cropFilterFactors(Int32Array records[6n], width, height, maxFactor)";
    const size_t t = align ? 1 : 0, per = align ? 4 : 6;
    Args a(env, info, 4 + t);
    View rec, terms;
    int32_t w = 0, h = 0, mf = 0;
    if (!a.arity(4 + t)) return nullptr;
    if (!a.i32s(0, 0, &rec) || rec.len % per || (align && (!a.f64s(1, 0, &terms) || terms.len * 4 != rec.len * 6)) || !a.i32(1 + t, &w) || !a.i32(2 + t, &h) || !a.i32(3 + t, &mf))
        return type_error(env, usage);
    if (w < 1 || w > 1024 || h < 1 || h > 1024 || mf < 1 || mf > 8) return range_error(env, (std::string(usage) + ": width and height are 1..1024, maxFactor is 1..8").c_str());
    const size_t n = rec.len / per;
    napi_value ab, ta;
    void *p = nullptr;
    NAPI_OK(napi_create_arraybuffer(env, n * 8, &p, &ab));
    NAPI_OK(napi_create_typedarray(env, napi_int32_array, n * 2, ab, 0, &ta));
    int32_t *out = static_cast<int32_t *>(p);
    const int32_t *v = rec.as<int32_t>();
    for (size_t i = 0; i < n; i++) {
        ht_status st;
        if (align) {
            const double *q = terms.as<double>() + 6 * i;
            ht_align_record r = {};
            r.code = v[4 * i], r.stream = v[4 * i + 1], r.a12 = v[4 * i + 2];
            r.cx = (int64_t)q[0], r.cy = (int64_t)q[1], r.ux = (int64_t)q[2], r.uy = (int64_t)q[3], r.vx = (int64_t)q[4], r.vy = (int64_t)q[5];
            st = ht_camshift_align_filter_factors(&r, w, h, mf, out + 2 * i, out + 2 * i + 1);
        } else {
            ht_crop_record r = {};
            r.code = v[6 * i], r.stream = v[6 * i + 1], r.rect.x = v[6 * i + 2], r.rect.y = v[6 * i + 3], r.rect.width = v[6 * i + 4], r.rect.height = v[6 * i + 5];
            st = ht_camshift_crop_filter_factors(&r, w, h, mf, out + 2 * i, out + 2 * i + 1);
        }
        if (st != HT_OK) return range_error(env, usage);
    }
    return ta;
}
napi_value CropFilterFactors(napi_env env, napi_callback_info info) { return filter_factors_call(env, info, false); }
napi_value AlignFilterFactors(napi_env env, napi_callback_info info) { return filter_factors_call(env, info, true); }

napi_value ctx_counter(napi_env env, napi_callback_info info, int which) {
    Args a(env, info, 1);
    Locked L;
    if (!a.ctx(1, &L)) return nullptr;
    napi_value v;
    const double x = which == 0 ? (double)ht_frames_bound(L.ctx) : which == 1 ? (double)ht_frames_enqueued(L.ctx) : (double)ht_graph_launches(L.ctx);
    NAPI_OK(napi_create_double(env, x, &v));
    return v;
}
napi_value FramesBound(napi_env env, napi_callback_info info) { return ctx_counter(env, info, 0); }
napi_value FramesEnqueued(napi_env env, napi_callback_info info) { return ctx_counter(env, info, 1); }
napi_value GraphLaunches(napi_env env, napi_callback_info info) { return ctx_counter(env, info, 2); }

napi_value Init(napi_env env, napi_value exports) {
    napi_add_env_cleanup_hook(env, env_cleanup, env);
    struct {
        const char *name;
        napi_callback fn;
    } fns[] = {{"createContext", CreateContext}, {"destroy", Destroy},         {"setGeometry", SetGeometry},
               {"detect", Detect},               {"detectAsync", DetectAsync}, {"grayscale", Grayscale},
               {"whitebalance", Whitebalance},   {"camshiftReserve", CamshiftReserve},
               {"camshiftInit", CamshiftInit},   {"camshiftTrack", CamshiftTrack}, {"info", Info},
               {"deviceCount", DeviceCount},     {"allgatherBest", AllgatherBest},
               {"exitNow", ExitNow},
               {"hostAlloc", HostAlloc},         {"hostFree", HostFree},       {"deviceAlloc", DeviceAlloc}, {"deviceFree", DeviceFree}, {"deviceUpload", DeviceUpload}, {"deviceDownload", DeviceDownload},
               {"upload", Upload},               {"bindDevice", BindDevice},   {"uploadAsync", UploadAsync}, {"swapFrames", SwapFrames},
               {"detectEnqueue", DetectEnqueue}, {"detectCollect", DetectCollect}, {"collectBest", CollectBest},
               {"detectWhitebalance", DetectWhitebalance}, {"whitebalanceBound", WhitebalanceBound},
               {"camshiftInitBound", CamshiftInitBound}, {"camshiftTrackBound", CamshiftTrackBound}, {"camshiftTrackCollect", CamshiftTrackCollect},
               {"camshiftInitPairs", CamshiftInitPairs}, {"camshiftTrackPairs", CamshiftTrackPairs},
               {"camshiftInitBest", CamshiftInitBest}, {"camshiftInitBestResult", CamshiftInitBestResult},
               {"camshiftInitFaces", CamshiftInitFaces}, {"camshiftInitFacesResult", CamshiftInitFacesResult},
               {"camshiftTrackSequence", CamshiftTrackSequence}, {"camshiftSequenceCollect", CamshiftSequenceCollect},
               {"camshiftBackProject", CamshiftBackProject}, {"camshiftBackProjectDevice", CamshiftBackProjectDevice},
               {"camshiftBackProjectPairs", CamshiftBackProjectPairs}, {"camshiftBackProjectPairsDevice", CamshiftBackProjectPairsDevice},
               {"drawFrames", DrawFrames},       {"drawFramesDevice", DrawFramesDevice},
               {"drawFramesYuv", DrawFramesYuv}, {"drawFramesYuvDevice", DrawFramesYuvDevice}, {"drawListDevice", DrawListDevice},
               {"drawListFilteredDevice", DrawListFilteredDevice}, {"drawFilterFactors", DrawFilterFactors},
               {"cropPairsDevice", CropPairsDevice}, {"cropSourcesDevice", CropSourcesDevice}, {"cropResult", CropResult},
               {"alignPairsDevice", AlignPairsDevice}, {"alignSourcesDevice", AlignSourcesDevice}, {"alignResult", AlignResult},
               {"cropPairsTensorDevice", CropPairsTensorDevice}, {"cropSourcesTensorDevice", CropSourcesTensorDevice},
               {"alignPairsTensorDevice", AlignPairsTensorDevice}, {"alignSourcesTensorDevice", AlignSourcesTensorDevice},
               {"cropPairsFilteredDevice", CropPairsFilteredDevice}, {"cropSourcesFilteredDevice", CropSourcesFilteredDevice},
               {"alignPairsFilteredDevice", AlignPairsFilteredDevice}, {"alignSourcesFilteredDevice", AlignSourcesFilteredDevice},
               {"cropFilterFactors", CropFilterFactors}, {"alignFilterFactors", AlignFilterFactors},
               {"detectBestEnqueue", DetectBestEnqueue}, {"collectBestDevice", CollectBestDevice}, {"detectGrouped", DetectGrouped},
               {"detectBestRecords", DetectBestRecords}, {"groupHits", GroupHits},
               {"framesBound", FramesBound},     {"framesEnqueued", FramesEnqueued}, {"graphLaunches", GraphLaunches}};
    for (auto &f : fns) {
        napi_value fn;
        if (napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &fn) != napi_ok) return nullptr;
        if (napi_set_named_property(env, exports, f.name, fn) != napi_ok) return nullptr;
    }
    const struct {
        const char *name;
        int32_t value;
    } consts[] = {{"abiVersion", ht_abi_version()},   {"INPUT_GRAY_IN_R", HT_INPUT_GRAY_IN_R}, {"INPUT_RGBA", HT_INPUT_RGBA}, {"DETECT_WHITEBALANCE", HT_DETECT_WHITEBALANCE},
                  {"SCAN_STATS", HT_SCAN_STATS},      {"BP_RGBA8", HT_BP_RGBA8},               {"BP_F64", HT_BP_F64},
                  {"YUV_NV12", HT_YUV_NV12},          {"YUV_I420", HT_YUV_I420},               {"DRAW_RGBA", HT_DRAW_RGBA},
                  {"YUV_YUYV", HT_YUV_YUYV},          {"YUV_UYVY", HT_YUV_UYVY},
                  {"CSB_UNTOUCHED", HT_CSB_UNTOUCHED}, {"CSB_FACE", HT_CSB_FACE},              {"CSB_FALLBACK", HT_CSB_FALLBACK}, {"CSB_DEFERRED", HT_CSB_DEFERRED},
                  {"CSF_ASSOCIATE", HT_CSF_ASSOCIATE}, {"CSF_MAX_SLOTS", HT_CSF_MAX_SLOTS},
                  {"CROP_EMPTY", HT_CROP_EMPTY},      {"CROP_FACE", HT_CROP_FACE},             {"CROP_SQUARE", HT_CROP_SQUARE},
                  {"ALIGN_EMPTY", HT_ALIGN_EMPTY},    {"ALIGN_FACE", HT_ALIGN_FACE},           {"ALIGN_SQUARE", HT_ALIGN_SQUARE},
                  {"PATCH_F32", HT_PATCH_F32},        {"PATCH_F16", HT_PATCH_F16},             {"PATCH_BF16", HT_PATCH_BF16},
                  {"PATCH_CHW", HT_PATCH_CHW},        {"PATCH_HWC", HT_PATCH_HWC},             {"PATCH_RGB", HT_PATCH_RGB},
                  {"PATCH_BGR", HT_PATCH_BGR},        {"PATCH_GRAY", HT_PATCH_GRAY}};
    for (auto &c : consts) {
        napi_value v;
        napi_create_int32(env, c.value, &v);
        napi_set_named_property(env, exports, c.name, v);
    }
    return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)

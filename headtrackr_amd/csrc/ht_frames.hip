// ht_frames.hip — the frames a context detects on: its own buffer and the back buffer of the asynchronous upload, the caller's device
// buffers (ht_device_alloc) and the binding of either.  Included by ht_context.hip (no device code).
//
// ht_frames_set is the ONLY place that assigns c->d_frames, c->frame_stride and c->nframes; it also publishes the binding to the
// context's slot of the frame registry (ht_frame_registry.h), which is all another context's thread ever looks at.

void ht_frames_set(ht_ctx *c, const uint8_t *frames, size_t frame_stride, int n) {  // frames == nullptr: unbound
    c->d_frames = frames;
    c->frame_stride = frame_stride;
    c->nframes = n;
    HtFrameRegistry::publish(&c->frame_slot, frames);
}

// A context's frames moved (bind / upload / swap / free): orphans that no live context is bound inside any more are released here as
// well, not only by some later ht_destroy — a host that re-binds its last binder elsewhere and never destroys anything would keep
// the HBM for the life of the process.  One relaxed load when there are no orphans (the streaming hosts bind per step).
static void sweep_orphans(ht_ctx *c) {
    const std::vector<HtFrameBuffer> release = g_frames.sweep();
    if (release.empty()) return;
    release_buffers(release);
    (void)hipSetDevice(c->device);
}

// One of the context's two frame buffers holds >= need bytes afterwards.  `wait_for`: the stream whose work may still touch the old
// buffer.  The own buffer may be the one the context is bound inside (the caller binds the new one), and its failed hipMalloc's sticky
// error is cleared; the back buffer's never was (the next HIP call of ht_upload_frames_async's caller reports it): kept as it is.
static ht_status frames_grow(ht_ctx *c, uint8_t **buf, size_t *bytes, size_t need, hipStream_t wait_for, bool own, const char *fn) {
    if (*bytes >= need) return HT_OK;
    HT_HIP(c, hipStreamSynchronize(wait_for));
    if (own && c->d_frames == *buf) ht_frames_set(c, nullptr, 0, 0);
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr, *bytes = 0;
    if (hipMalloc(buf, need) != hipSuccess) {
        if (own) (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, std::string(fn) + ": hipMalloc failed");
    }
    *bytes = need;
    return HT_OK;
}

// The context's own frame buffer, grown on demand (what ht_upload_frames and the bind form of the draw calls write), and the binding of
// its first n frames.
ht_status ht_frames_own_reserve(ht_ctx *c, size_t need, const char *fn) {
    return frames_grow(c, &c->d_frames_own, &c->d_frames_own_bytes, need, c->stream, true, fn);
}
void ht_frames_bind_own(ht_ctx *c, int n) {
    ht_frames_set(c, c->d_frames_own, (size_t)c->W * c->H * 4, n);
    sweep_orphans(c);
}

// what both uploads refuse, in this order; selects the device
static ht_status upload_check(ht_ctx *c, const char *fn, const uint8_t *host_rgba, int32_t n, size_t frame_stride) {
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, std::string(fn) + ": call ht_set_geometry first");
    if (!host_rgba || n <= 0 || n > c->max_batch || frame_stride < (size_t)c->W * c->H * 4)
        return ht_fail(c, HT_ERR_INVALID, std::string(fn) + ": bad frame count or stride");
    HT_HIP(c, hipSetDevice(c->device));
    return HT_OK;
}

// n host frames, packed or frame_stride apart, packed into dst on `stream`
static ht_status upload_copy(ht_ctx *c, uint8_t *dst, const uint8_t *host_rgba, int32_t n, size_t frame_stride, hipStream_t stream) {
    const size_t fbytes = (size_t)c->W * c->H * 4;
    if (frame_stride == fbytes) {
        HT_HIP(c, hipMemcpyAsync(dst, host_rgba, fbytes * (size_t)n, hipMemcpyHostToDevice, stream));
    } else {
        HT_HIP(c, hipMemcpy2DAsync(dst, fbytes, host_rgba, frame_stride, fbytes, (size_t)n, hipMemcpyHostToDevice, stream));
    }
    return HT_OK;
}

extern "C" ht_status ht_upload_frames(ht_ctx *c, const uint8_t *host_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    HtRange range("ht_upload_frames");
    ht_status st = upload_check(c, "ht_upload_frames", host_rgba, n, frame_stride);
    if (st != HT_OK) return st;
    if ((st = ht_frames_own_reserve(c, (size_t)c->W * c->H * 4 * (size_t)n, "ht_upload_frames")) != HT_OK) return st;
    if ((st = upload_copy(c, c->d_frames_own, host_rgba, n, frame_stride, c->stream)) != HT_OK) return st;
    ht_frames_bind_own(c, n);
    return HT_OK;
}

extern "C" ht_status ht_upload_frames_async(ht_ctx *c, const uint8_t *host_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    ht_status st = upload_check(c, "ht_upload_frames_async", host_rgba, n, frame_stride);
    if (st != HT_OK) return st;
    if (!c->copy_stream) {
        HT_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        HT_HIP(c, hipEventCreateWithFlags(&c->ev_copy_done, hipEventDisableTiming));
        HT_HIP(c, hipEventCreateWithFlags(&c->ev_front_free, hipEventDisableTiming));
    }
    st = frames_grow(c, &c->d_frames_back, &c->d_frames_back_bytes, (size_t)c->W * c->H * 4 * (size_t)n, c->copy_stream, false, "ht_upload_frames_async");
    if (st != HT_OK) return st;
    // the back buffer was the front buffer until the last swap: kernels enqueued before that swap may still read it
    HT_HIP(c, hipStreamWaitEvent(c->copy_stream, c->ev_front_free, 0));
    if ((st = upload_copy(c, c->d_frames_back, host_rgba, n, frame_stride, c->copy_stream)) != HT_OK) return st;
    HT_HIP(c, hipEventRecord(c->ev_copy_done, c->copy_stream));
    c->back_n = n;
    return HT_OK;
}

extern "C" ht_status ht_swap_frames(ht_ctx *c) {
    if (!c) return HT_ERR_INVALID;
    if (c->back_n <= 0) return ht_fail(c, HT_ERR_STATE, "ht_swap_frames: no ht_upload_frames_async pending");
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipEventRecord(c->ev_front_free, c->stream));            // everything enqueued so far used the old front buffer
    HT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_copy_done, 0));      // later kernels wait for the copy, the host does not
    std::swap(c->d_frames_own, c->d_frames_back);
    std::swap(c->d_frames_own_bytes, c->d_frames_back_bytes);
    const int n = c->back_n;
    c->back_n = 0;
    ht_frames_bind_own(c, n);
    return HT_OK;
}

extern "C" ht_status ht_bind_frames_device(ht_ctx *c, const void *dev_rgba, int32_t n, size_t frame_stride) {
    if (!c) return HT_ERR_INVALID;
    if (c->W == 0) return ht_fail(c, HT_ERR_STATE, "ht_bind_frames_device: call ht_set_geometry first");
    if (!dev_rgba || n <= 0 || n > c->max_batch || frame_stride < (size_t)c->W * c->H * 4 || (frame_stride & 3) ||
        ((uintptr_t)dev_rgba & 3))
        return ht_fail(c, HT_ERR_INVALID, "ht_bind_frames_device: bad pointer, frame count or stride (4-byte alignment required)");
    ht_frames_set(c, (const uint8_t *)dev_rgba, frame_stride, n);
    sweep_orphans(c);
    return HT_OK;
}

extern "C" int32_t ht_frames_bound(const ht_ctx *c) { return c ? c->nframes : 0; }
extern "C" int32_t ht_frames_enqueued(const ht_ctx *c) { return (c && c->enqueued) ? c->enq_nframes : 0; }

extern "C" ht_status ht_host_alloc(size_t bytes, void **out) {
    if (!out || bytes == 0) return HT_ERR_INVALID;
    *out = nullptr;
    if (hipHostMalloc(out, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(nullptr, HT_ERR_NOMEM, "ht_host_alloc: hipHostMalloc failed");
    }
    return HT_OK;
}
extern "C" void ht_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}
extern "C" ht_status ht_device_alloc(ht_ctx *c, size_t bytes, void **out) {
    if (!c || !out || bytes == 0) return HT_ERR_INVALID;
    *out = nullptr;
    HT_HIP(c, hipSetDevice(c->device));
    if (hipMalloc(out, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return ht_fail(c, HT_ERR_NOMEM, "ht_device_alloc: hipMalloc failed");
    }
    c->user_allocs.emplace_back(*out, bytes);
    return HT_OK;
}
extern "C" ht_status ht_device_free(ht_ctx *c, void *p) {
    if (!c) return HT_ERR_INVALID;
    if (!p) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipStreamSynchronize(c->stream));  // nothing enqueued on this context may still read it
    auto it = std::find_if(c->user_allocs.begin(), c->user_allocs.end(), [p](const std::pair<void *, size_t> &a) { return a.first == p; });
    if (it == c->user_allocs.end()) return ht_fail(c, HT_ERR_INVALID, "ht_device_free: not a live ht_device_alloc buffer of this context");
    // a buffer that other contexts of this device have bound (ht_bind_frames_device: a batch host shares one frame buffer between
    // its pipelined contexts) is NOT freed under them: their next enqueue would read freed HBM.  Rebind or destroy them first.
    if (g_frames.bound_inside(&c->frame_slot, c->device, p, it->second))
        return ht_fail(c, HT_ERR_STATE, "ht_device_free: another live context still has frames bound inside this buffer (rebind or destroy it first)");
    const uint8_t *pb = static_cast<const uint8_t *>(p);
    if (c->d_frames && c->d_frames >= pb && c->d_frames < pb + it->second) {  // frames bound inside it
        ht_frames_set(c, nullptr, 0, 0);
        destroy_graphs(c);  // their keys hold the freed pointer: an allocation that reuses the address must not replay them
    }
    c->user_allocs.erase(it);
    HT_HIP(c, hipFree(p));
    sweep_orphans(c);
    return HT_OK;
}
extern "C" ht_status ht_device_upload(ht_ctx *c, void *dst_dev, const void *src_host, size_t bytes) {
    if (!c || !dst_dev || !src_host) return HT_ERR_INVALID;
    if (bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

extern "C" ht_status ht_device_download(ht_ctx *c, void *dst_host, const void *src_dev, size_t bytes) {
    if (!c || !dst_host || !src_dev) return HT_ERR_INVALID;
    if (bytes == 0) return HT_OK;
    HT_HIP(c, hipSetDevice(c->device));
    HT_HIP(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HT_HIP(c, hipStreamSynchronize(c->stream));
    return HT_OK;
}

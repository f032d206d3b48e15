/*
 * headtrackr_hip.h — C ABI of libheadtrackr_hip.so: the MI355X (gfx950) implementation of headtrackr's per-frame
 * detect / track hot path.
 *
 * The reference (auduno/headtrackr) has no FFI; its boundary is the set of JavaScript functions that
 * facetrackr.Tracker calls once per frame.  Every entry point below names the reference interface it replaces
 * (paths are /root/reference/src/...).  The N-API shim (headtrackr_amd/csrc/ht_napi.cc) and the JS facade
 * (headtrackr_amd/js/headtrackr.js) bind exactly these symbols; INTEGRATION.md shows the binding.
 *
 * Conventions: plain C, no exceptions; every function returns ht_status (0 = OK) and records a message readable
 * with ht_last_error(); the caller owns every buffer it passes; a ctx is bound to one GPU and is not thread-safe
 * (one call in flight per ctx).  Host buffers may be pageable; *_device entry points take device pointers and never
 * copy.  All work is enqueued on one HIP stream (the caller's, if given in ht_config.stream).
 */
#ifndef HEADTRACKR_HIP_H
#define HEADTRACKR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HT_ABI_VERSION 2
#define HT_MAX_LEVELS 96

typedef int32_t ht_status;
enum {
    HT_OK = 0,
    HT_ERR_INVALID = -1,   /* bad argument / unsupported geometry */
    HT_ERR_HIP = -2,       /* a HIP runtime call failed (message has the HIP error string) */
    HT_ERR_NOMEM = -3,     /* host or device allocation failed */
    HT_ERR_CAPACITY = -4,  /* an output did not fit the caller's buffer (results truncated, counts are exact) */
    HT_ERR_NO_DEVICE = -5, /* no usable gfx950 device */
    HT_ERR_STATE = -6      /* call sequence error (e.g. detect before frames were bound) */
};

typedef struct ht_ctx ht_ctx;

/* flags for ht_detect_* */
enum {
    HT_INPUT_RGBA = 0,      /* colour frame: ccv.grayscale (ccv.js:22-32) is fused into the pyramid build */
    HT_INPUT_GRAY_IN_R = 1, /* byte 0 of each pixel is already gray: exactly what ccv.detect_objects reads (ccv.js:115,171) */
    HT_SCAN_FUSED_TAIL = 0, /* default scan schedule */
    HT_SCAN_NO_SPLIT = 2,   /* run every cascade stage in the tile kernel (no second "deep" kernel); debugging / A-B */
    HT_SCAN_SIMPLE = 4,     /* one thread per window straight from HBM (slow reference kernel); debugging / A-B */
    HT_SCAN_GENERIC = 8,    /* table-driven stage code even for the built-in cascade (no generated straight-line stages) */
    HT_SCAN_STATS = 16,     /* also count the windows entering every stage (ht_stage_counts); costs a few atomics per workgroup */
    HT_DETECT_WHITEBALANCE = 32 /* the gray pass also accumulates getWhitebalance's channel sums (whitebalance.js:5-30): the frame is
                                 * read once for both; fetch the values with ht_detect_whitebalance after ht_detect_collect */
};

typedef struct ht_config {
    uint32_t struct_size;   /* = sizeof(ht_config) */
    int32_t device;         /* HIP device ordinal */
    int32_t interval;       /* ccv.detect_objects `interval` (facetrackr.js:148 passes 5) */
    uint32_t hit_capacity;  /* max raw hits kept per batch (0 = default 1<<20) */
    void *stream;           /* hipStream_t to enqueue on; NULL = library-owned non-blocking stream */
    uint32_t queue_capacity;/* survivors handed from the tile kernel to the deep kernel per batch (0 = auto) */
    uint32_t flags;         /* reserved, 0 */
    const char *options;    /* NULL, or "key=value,key=value,...": per-context schedule selectors for tests and A/B measurements
                             * (ABI 2; a caller that passes the ABI-1 struct_size has none).  The library reads NO environment
                             * variable: what a context computes depends on its arguments alone.  Every key below selects among
                             * schedules that produce IDENTICAL results; an unknown key fails ht_create with HT_ERR_INVALID.
                             *   cs_fused_min=N       streams per call from which camshift runs as one launch (default 192)
                             *   cs_fused_nt=512|1024 threads per workgroup of that launch (0 = per launch: 512 — two workgroups per CU — when it has more
                             *                        streams than the device has CUs or another context of the device that tracks on this path has
                             *                        work in flight at launch time, else 1024)
                             *   cs_seq_fused=0|1     track sequences inside one launch (1)       cs_keep_hist=1   keep histograms for ht_camshift_debug_hist
                             *   cs_cluster=0|1, cs_cluster_min_px=N, cs_region=N                 cluster / LDS-region paths of the few-stream schedule
                             *   cs_barrier_budget=N  shader-clock cycles a cluster exchange may wait before the call fails with HT_ERR_STATE
                             *   cs_flags=0|1         enqueue-only track calls of the cluster path are completed by marks in the pinned slot (1) or an event
                             *   cs_sync_ring=0|1     a synchronous track call takes the enqueue-only route and collects at once (1) or copies back + synchronises (0)
                             *   cs_pairs_force=1     ht_camshift_*_pairs calls whose pairs are (first + i, i) run the pair kernels too instead of the batch schedules
                             *   cs_pairs_cluster=1   ht_camshift_track_pairs on a few pairs of large frames (the cluster rule of track_batch with n = pairs, and
                             *                        cs_cluster set) runs G workgroups per pair; ht_camshift_init_pairs splits tall rects of < 64 pairs by rows (0)
                             *   fp_sparse=0|1        tile kernel: sparse stages one lane per (window, feature) pair when <= 256 pairs are left (1)
                             *   graph_max_frames=N   batches up to N frames replay a captured hipGraph (256; 0 = never)
                             *   split=S, deep_bias=B, deep_v=2|4, deep_grid=N                    tile kernel -> deep kernel hand-off (grid kept >= 16 wavefronts)
                             *   force_exact=1        every integer stage decision re-run on the sequential binary64 path
                             *   rs_bands=0|1         pyramid generations by k_resample_bands (1: LDS-DMA into wave-private source bands) or k_resample (0)
                             *   early_scan=1, rs_rpt, rs_minwg, rs_k, rs_group, rs_tailtable, rs_tailcap, rs_notail, rs_nofast, rs_nosort, rs_gennames
                             *   host_threads=N       worker threads of the host post-processing (0 = single-threaded)
                             *   force_rccl=1         ht_allgather_* goes through RCCL even with one rank
                             *   group_cap=N          raw hits of one frame the device grouping takes (a power of two, 64 .. 1024 = default); frames above
                             *                        it are finished on the host by the collect call
                             *   draw_filter_rows=4|16  ht_draw_list_filtered_device: the kernel's tile is 64 x 4 (the default) or 64 x 16 pixels
                             *   orient_lanes=1|2     the oriented draw, entries of odd rot: lanes along O's x (1) or along the stored row with the tile
                             *                        turned through LDS (2); 0 = the shipped choice.  Same bytes either way
                             * Keys that make results incomplete by design (stop_stage, cs_iters, rs_maxgen) exist only in builds
                             * compiled with -DHT_DEBUG_KNOBS (tools/build_alt.py); the product library rejects them. */
} ht_config;

/* One raw detection = one element of ccv.detect_objects' `seq` (ccv.js:227-234) in index form:
 * rect = { x:(4*x+2*(q&1))*s, y:(4*y+2*(q>>1))*s, width:cw*s, height:ch*s, confidence:sum }, s = scale^i. */
typedef struct ht_hit {
    uint32_t frame;
    uint16_t x, y;     /* window index on the quarter-resolution plane */
    uint8_t scale;     /* i, ccv.js:154 */
    uint8_t q;         /* half-pixel phase, ccv.js:151-152,178 */
    uint16_t reserved0;
    uint32_t reserved1;
    double sum;        /* last stage's sum (binary64, accumulated in the reference's order) */
} ht_hit;

typedef struct ht_rect { /* element of detect_objects' result (ccv.js:228-233 raw, 297-302 grouped) */
    double x, y, width, height, confidence;
    int32_t neighbors;
    int32_t reserved;
} ht_rect;

typedef struct ht_plane_info {
    int32_t width, height; /* canvas size of the pyramid level */
    int32_t stride;        /* bytes per row in the device arena */
    int32_t present;       /* 0 if this (level, slot) does not exist */
    uint64_t offset;       /* byte offset inside one frame's arena */
} ht_plane_info;

typedef struct ht_cs_rect { int32_t x, y, width, height; } ht_cs_rect;
typedef struct ht_cs_pair { int32_t stream, frame; } ht_cs_pair; /* tracker `stream` meets BOUND frame `frame` (ht_camshift_*_pairs) */

/* camshift.Tracker's persistent per-stream state (camshift.js:153-160): lives on the device, one per stream. */
typedef struct ht_cs_trackobj { /* camshift.TrackObj, camshift.js:362-378 (+ the search window, camshift.js:162-165) */
    double x, y, width, height, angle;
    int32_t sw_x, sw_y, sw_width, sw_height;
} ht_cs_trackobj;

typedef struct ht_kernel_time { /* per-kernel device time of the last ht_detect_* call when profiling is on */
    char name[32];
    double ms;
    uint32_t launches;
    uint32_t reserved;
} ht_kernel_time;

/* ---- lifetime ------------------------------------------------------------------------------------------ */

/* Creates a context on cfg->device holding the cascade (an "HTCB" blob, see headtrackr_amd/js/cascade_pack.js)
 * = the `cascade` argument of ccv.detect_objects (ccv.js:109; data: cascade.js:19). */
ht_status ht_create(const ht_config *cfg, const void *cascade_blob, size_t cascade_len, ht_ctx **out);
/* Lifetime of shared frame buffers: a buffer of ht_device_alloc that OTHER live contexts still have frames bound inside
 * (ht_bind_frames_device) is not freed by its owner's ht_destroy — it stays alive as an orphan.  Orphans are looked at whenever a
 * context's frames move — at the end of ht_upload_frames, ht_swap_frames, ht_bind_frames_device, ht_device_free, the bind form of the
 * draw calls — and in every ht_destroy: an orphan that no live context is bound inside any more is released by that call, whichever
 * context makes it.  Such a release waits for the orphan's whole device first (hipDeviceSynchronize: work of any context may still
 * read it), so the call that happens to release one is slow once; while no orphan exists these calls pay one relaxed load.  The
 * recommended order is still binders first, owner last.
 * Threads: every context publishes where it is bound, and only that is read by other contexts' calls — contexts used by one thread
 * each need no lock between them for any of this.  What remains a caller error: binding a context INTO a buffer (another thread)
 * concurrently with the call that releases it — the ht_device_free or ht_destroy of its owner or, for an orphan, the call after
 * which no context is bound inside it.  The release may have decided before the binding was published. */
void ht_destroy(ht_ctx *ctx);
/* Message of the last failure on ctx (ctx == NULL: last failure of ht_create on this thread). Never NULL. */
const char *ht_last_error(const ht_ctx *ctx);
int32_t ht_abi_version(void);

/* ---- geometry ------------------------------------------------------------------------------------------ */

/* Fixes frame size and batch capacity; (re)allocates the pyramid arena.  level_dims (optional, 2*nlevels int32:
 * w0,h0,w1,h1,...) lets a JavaScript host pass the sizes V8 computed with Math.pow/Math.floor (ccv.js:119-120,
 * 126-127); NULL = computed here (identical for interval 5, see oracle/ht_oracle.c HO_V8_SCALE6_POW).
 * level_dims are refused (HT_ERR_INVALID, the current geometry stays) unless level 0 is the frame, every level lies within
 * 0 .. the frame's size, and level i + interval + 1 is at most floor(size / 2) of level i in both directions: the scan
 * reads one window on levels i, i + next and i + 2 next at 4, 2 and 1 times its coordinates, and nothing on the device
 * clamps those reads into the planes (headtrackr_amd/csrc/ht_geometry_plan.h, ht_check_level_dims). */
ht_status ht_set_geometry(ht_ctx *ctx, int32_t width, int32_t height, int32_t max_batch, const int32_t *level_dims,
                          int32_t nlevels);
int32_t ht_num_levels(const ht_ctx *ctx);
ht_status ht_plane(const ht_ctx *ctx, int32_t level, int32_t slot, ht_plane_info *out);
uint64_t ht_windows_per_frame(const ht_ctx *ctx);   /* sliding windows scanned per frame */
uint64_t ht_pyramid_bytes_per_frame(const ht_ctx *ctx); /* sum of w*h over all planes (gray bytes) */

/* ---- frames -------------------------------------------------------------------------------------------- */

/* Copies n RGBA frames (frame_stride bytes apart, rows packed) from host memory into the ctx's device buffer. */
ht_status ht_upload_frames(ht_ctx *ctx, const uint8_t *host_rgba, int32_t n, size_t frame_stride);
/* Double-buffered ingest for live feeds (the reference's per-frame video -> canvas copy, main.js:170):
 * ht_upload_frames_async copies the NEXT frames from pinned host memory into the ctx's back buffer on a separate copy
 * stream, so the copy overlaps the kernels working on the current frames; ht_swap_frames makes the back buffer current
 * (the compute stream waits for the copy, no host synchronisation).  host_rgba must stay valid until the swap. */
ht_status ht_upload_frames_async(ht_ctx *ctx, const uint8_t *host_rgba, int32_t n, size_t frame_stride);
ht_status ht_swap_frames(ht_ctx *ctx);
/* Uses frames already resident in device memory (no copy; must stay valid until the results were collected).  dev_rgba: any 4-byte-aligned
 * address; frame_stride: any multiple of 4 that is >= width * height * 4 (anything else is HT_ERR_INVALID and leaves the binding as it was).
 * Strided and 4- but not 16-byte-aligned bindings are exercised by tests/test_gpu_frame_layouts.py. */
ht_status ht_bind_frames_device(ht_ctx *ctx, const void *dev_rgba, int32_t n, size_t frame_stride);

/* Frames currently bound (ht_upload_frames / ht_swap_frames / ht_bind_frames_device) and frames of the batch enqueued last: the
 * collect calls report on the ENQUEUED batch — size counts[] / best[] with ht_frames_enqueued, not with what is bound by then. */
int32_t ht_frames_bound(const ht_ctx *ctx);
int32_t ht_frames_enqueued(const ht_ctx *ctx);

/* Memory for hosts that have no HIP binding of their own (the Node addon): pinned host buffers — frames in them cross PCIe at link
 * speed and may be handed to ht_upload_frames_async — and device buffers for frames that stay resident in HBM across calls
 * (ht_bind_frames_device, ht_camshift_track_sequence).  ht_device_upload copies host -> device and returns when src may be reused;
 * ht_device_download copies device -> host behind everything enqueued on the ctx stream so far (e.g. an ht_draw_frames_device into that
 * buffer) and returns when dst_host holds the bytes. */
ht_status ht_host_alloc(size_t bytes, void **out);
void ht_host_free(void *p);
ht_status ht_device_alloc(ht_ctx *ctx, size_t bytes, void **out);
/* Frees a buffer of ht_device_alloc on the context that allocated it.  Fails with HT_ERR_STATE (nothing freed) while ANOTHER live
 * context still has frames bound inside it (ht_bind_frames_device): rebind or destroy that context first. */
ht_status ht_device_free(ht_ctx *ctx, void *p);
ht_status ht_device_upload(ht_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
ht_status ht_device_download(ht_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);

/* ---- ingest: the loop's video -> canvas copy (main.js:170, 312) ------------------------------------------ */

/* drawImage(video, sx,sy,sw,sh, 0,0,W,H) for n frames. W x H = the context's geometry. src_rect NULL = whole source frame (the 5-argument
 * form main.js uses). One rect for all n frames. Declared resampler of oracle/canvas_shim.js on all four channels, every byte equal.
 * dst_dev NULL: the result goes into the context's own frame buffer and becomes the bound frames (ht_frames_bound() == n), exactly as
 * after ht_upload_frames. Otherwise into the caller's buffer, frames dst_frame_stride apart (0 = packed), binding untouched.
 * Enqueued on the ctx stream; never copies to the host, never waits.  Argument errors change nothing; HT_ERR_NOMEM / HT_ERR_HIP from the
 * bind form when the context's buffer has to grow leave the context usable but without bound frames (the same holds for ht_upload_frames). */
ht_status ht_draw_frames_device(ht_ctx *ctx, const void *src_dev, int32_t n, int32_t src_width, int32_t src_height,
                                size_t src_pitch /* bytes per source row, 0 = packed */, size_t src_frame_stride /* 0 = packed */,
                                const ht_cs_rect *src_rect, void *dst_dev, size_t dst_frame_stride);
/* The same for host-resident source frames (rows packed). Staged through a context-owned device buffer that grows on demand.
 * Result bound as above. Same completion contract as ht_upload_frames (host_rgba reusable on return). */
ht_status ht_draw_frames(ht_ctx *ctx, const uint8_t *host_rgba, int32_t n, int32_t src_width, int32_t src_height,
                         size_t src_frame_stride, const ht_cs_rect *src_rect);

/* The same draw for frames that arrive as YUV 4:2:0, 8 bits per sample: the colour conversion a browser's drawImage(video, ..) hides is
 * fused into the draw.  The conversion is DECLARED (csrc/ht_yuv_plan.h), integer-only and so the same bits everywhere: with C = Y - yoff,
 * D = U - 128, E = V - 128, R = clamp((cy C + crv E + 128) >> 8), G = clamp((cy C + cgu D + cgv E + 128) >> 8), B = clamp((cy C + cbu D +
 * 128) >> 8), A = 255.  The chroma sample of source pixel (x, y) is sample (x >> 1, y >> 1) of the FRAME, replicated; odd widths and
 * heights are legal, the chroma planes are ceil(w / 2) x ceil(h / 2).  The result is, byte for byte, what ht_draw_frames_device gives on
 * the RGBA frame that conversion produces.
 *
 * Packed 4:2:2 (what an uncompressed webcam or a capture card delivers: UVC "YUY2" = V4L2 YUYV; SDI bridges UYVY) rides the same calls:
 * ht_draw_frames_yuv, ht_draw_frames_yuv_device, ht_draw_list_device, ht_draw_list_filtered_device and, as an ht_draw_source entry, the
 * ht_camshift_crop_sources_* / ht_camshift_align_sources_* calls (those unpack each packed entry's whole frame to RGBA in a context-owned
 * buffer first — one more launch and 4 B/px per packed entry — and then are the call on that RGBA entry).  A
 * frame is ONE plane; with cw = ceil(w / 2), row y holds cw macropixels of 4 bytes: HT_YUV_YUYV Y(2m) U(m) Y(2m+1) V(m), HT_YUV_UYVY U(m)
 * Y(2m) V(m) Y(2m+1).  Pixel (x, y) takes its own Y byte and the U and V of macropixel (x >> 1) of ROW y of the frame (replicated
 * horizontally, not interpolated, sited by the frame and not by a source rect: the 4:2:0 rule without the vertical halving); the triple
 * goes through the same conversion and matrices, and the result of every call is, byte for byte, what the same call gives on the RGBA frame
 * that conversion produces.  Odd widths are legal: the last macropixel's second luma byte is in memory and never selected.  Base address and
 * row pitch are multiples of 4 (a macropixel is one aligned dword), pitch >= 4 cw (0 = 4 cw), width / height 1..16384, matrix 0..3; for
 * n > 1 the frame stride is a multiple of 4 and at least pitch (h - 1) + 4 cw; a tightly packed host frame is 4 cw h bytes.  In
 * ht_yuv_frames the plane is y with y_pitch (u, v, c_pitch are not looked at); in ht_draw_source it is p0 with pitch0 (p1, p2, pitch1 are
 * not looked at).  The numbers 2, 3, 6 and every other are no format and stay refused.  Not part of this: 10-bit layouts (P010, Y210), other
 * byte orders (YVYU, VYUY), planar or semi-planar 4:2:2 (I422, NV16), chroma interpolation, and the *_pairs_* calls, which read the RGBA
 * canvas and are untouched. */
enum { HT_YUV_NV12 = 0 /* Y plane + one plane of interleaved U V pairs */, HT_YUV_I420 = 1 /* Y, U, V planes */,
       HT_YUV_YUYV = 4 /* one plane of Y U Y V macropixels */, HT_YUV_UYVY = 5 /* one plane of U Y V Y macropixels */ };
enum { HT_YUV_BT601_LIMITED = 0, HT_YUV_BT709_LIMITED = 1, HT_YUV_BT601_FULL = 2, HT_YUV_BT709_FULL = 3 };
typedef struct ht_yuv_frames {
    const void *y, *u, *v;   /* NV12: u = the interleaved UV plane, v = NULL.  YUYV / UYVY: y = the packed plane, u and v not looked at */
    size_t y_pitch;          /* 0 = width (YUYV / UYVY: 0 = 4 ceil(width / 2)) */
    size_t c_pitch;          /* 0 = packed */
    size_t frame_stride;     /* added to every plane pointer per frame; 0 = device form refuses n > 1 */
    int32_t width, height, format, matrix;  /* format: | HT_ORIENT(k) for rotated / mirrored frames (below, at ht_draw_source) */
} ht_yuv_frames;
/* Device-resident planes.  dst_dev, dst_frame_stride, src_rect, binding and errors as ht_draw_frames_device; the overlap refusals apply
 * per plane.  NV12's chroma base, chroma pitch and frame stride must be even; the Y plane and I420's chroma planes need no alignment;
 * a YUYV / UYVY plane's base, pitch and frame stride are multiples of 4. */
ht_status ht_draw_frames_yuv_device(ht_ctx *ctx, const ht_yuv_frames *src_dev, int32_t n, const ht_cs_rect *src_rect, void *dst_dev,
                                    size_t dst_frame_stride);
/* Host-resident frames, each tightly packed: Y, then UV (NV12) or U, then V (I420), w h + 2 cw ch bytes; YUYV / UYVY: 4 cw h bytes.  Frames
 * frame_stride apart (0 = packed; for the host form any stride of at least a frame).  Staged through the context-owned device buffer of
 * ht_draw_frames at 1.5 B/px (4:2:2: 2 B/px); result bound; host reusable on return. */
ht_status ht_draw_frames_yuv(ht_ctx *ctx, const uint8_t *host, int32_t n, int32_t width, int32_t height, int32_t format, int32_t matrix,
                             size_t frame_stride, const ht_cs_rect *src_rect);

/* The K-feed form of the draw (the reference's loop is one drawImage per feed, main.js:170): ONE launch draws a list of sources that share
 * nothing — every entry names its own device allocation(s), size, pitches, format, matrix and source rect.  Entry i is
 * drawImage(source_i, sx,sy,sw,sh, 0,0,W,H) onto destination frame i, with the bytes ht_draw_frames_device (HT_DRAW_RGBA) or
 * ht_draw_frames_yuv_device (HT_YUV_NV12 / HT_YUV_I420 / HT_YUV_YUYV / HT_YUV_UYVY) gives for that entry alone.  Plane pointers of different entries may be equal or
 * overlap (one decoded surface under several rects).  Per entry, the rules of those calls with n = 1: RGBA, YUYV and UYVY base and pitch
 * multiples of 4; NV12 chroma base and pitch even; width / height 1..16384; matrix 0..3 (ignored for RGBA); rect wholly inside the source, or width == 0
 * && height == 0 for the whole source (x, y are then not looked at).  HT_DRAW_RGBA lies outside the HT_YUV_* format range: the YUV entry
 * points refuse it. */
enum { HT_DRAW_RGBA = 16 };
/* Rotated and mirrored feeds (a phone in portrait: landscape surfaces plus a rotation flag — container `rotate` / display matrix, WebRTC CVO,
 * EXIF on stills; a hardware decoder's surface as stored; a mirrored selfie camera).  An ORIENTATION k = 0..7 rides in bits 8..10 of the
 * `format` field of ht_draw_source and ht_yuv_frames (and of ht_draw_frames_yuv's format argument): format = HT_YUV_NV12 | HT_ORIENT(5).
 * rot = k & 3 counts the quarter turns clockwise that bring the stored frame upright, flip = k >> 2 is a horizontal mirror applied after the
 * turn.  The stored frame S of w x h gives the oriented frame O of (w, h) for even rot, (h, w) for odd rot, a pure index permutation: with
 * x' = flip ? ow - 1 - x : x, O(x, y) = S(u, v), (u, v) = (x', y) | (y, h - 1 - x') | (w - 1 - x', h - 1 - y) | (w - 1 - y, x') for rot 0 | 1 |
 * 2 | 3 (numpy: np.rot90(S, -rot), then np.fliplr if flip; EXIF orientations 1..8 are k = 0, 4, 2, 6, 5, 1, 7, 3).  Every call that takes
 * such a format gives, byte for byte, what it gives today on the RGBA frame O = orient(convert(S)): width, height, pitches and planes
 * describe the STORED frame, YUV chroma is sited by the stored frame exactly as without an orientation (conversion first, permutation
 * second), and source rects, crop boxes and records are in O's coordinates (a rect inside O but outside S is legal, the converse is
 * refused).  Every value that was legal before means what it meant; a value with any bit from 11 up stays no format.
 *   ht_draw_list_device, ht_draw_frames_yuv, ht_draw_frames_yuv_device: ONE fused launch (k_draw_list_oriented) — the permutation is applied
 *     to the few source samples the draw reads.  A list without an oriented entry takes the path it took.
 *   ht_draw_list_filtered_device and the ht_camshift_crop_sources_* / ht_camshift_align_sources_* calls orient each oriented entry's whole
 *     frame into a context-owned buffer first — one more launch and 4 B/px per oriented entry (an oriented YUYV / UYVY entry: one pass, not
 *     two) — and then are the call on that RGBA entry of O.
 * The kernel lives in a code object of its own, libheadtrackr_hip_orient.hsaco NEXT TO the library, loaded on the first oriented call of a
 * process (once per device); without that file every oriented call returns HT_ERR_STATE with the path in ht_last_error, and every other call
 * works as before.  Not part of this: ht_draw_frames / ht_draw_frames_device (no format argument: an RGBA feed uses a one-entry list), the
 * *_pairs_* calls (they read the canvas), arbitrary angles, a format-preserving rotation. */
#define HT_ORIENT(k) ((int32_t)(k) << 8)
#define HT_FORMAT_OF(f) ((int32_t)(f) & 0xff)
#define HT_ORIENT_OF(f) (((int32_t)(f) >> 8) & 7)
typedef struct ht_draw_source {
    const void *p0, *p1, *p2; /* RGBA: p0.  NV12: Y, UV.  I420: Y, U, V.  YUYV / UYVY: p0.  Device pointers; the unused ones are not looked at. */
    size_t pitch0, pitch1;    /* bytes per row of p0 / of the chroma plane(s); 0 = packed */
    int32_t width, height;    /* of THIS source */
    int32_t format;           /* HT_YUV_NV12, HT_YUV_I420, HT_YUV_YUYV, HT_YUV_UYVY or HT_DRAW_RGBA; | HT_ORIENT(k) for a rotated / mirrored source */
    int32_t matrix;           /* HT_YUV_* matrix; ignored for RGBA */
    ht_cs_rect rect;          /* width == 0 && height == 0: whole source */
} ht_draw_source;
/* srcs: a HOST array of n entries, 1 <= n <= 65535, read before the call returns.  dst_dev NULL: into the context's own frame buffer, n
 * frames bound (n <= max_batch), exactly as ht_draw_frames_device does; otherwise frames dst_frame_stride apart (0 = packed) in the
 * caller's buffer, binding untouched.  Every plane of every entry is refused when it overlaps the destination range (bind form: the
 * context's own buffer).  Every check happens before anything is enqueued: a refused call (HT_ERR_INVALID) changes nothing and its message
 * names the first offending entry as "entry <i>".  Enqueue-only: the descriptor table travels through pinned staging slots and one
 * hipMemcpyAsync on the ctx stream (a slot is reused only after an event shows its copy has run), so the call never copies to the host and
 * never waits in the steady state; the first call of a context, or a longer list, allocates. */
ht_status ht_draw_list_device(ht_ctx *ctx, const ht_draw_source *srcs, int32_t n, void *dst_dev, size_t dst_frame_stride);

/* The same draw with a prefilter for strong downscales.  ht_draw_list_device reads one bilinear tap pair per canvas pixel: 1920 x 1080 onto
 * 320 x 240 touches 2 of every 6 columns and 2 of every 4.5 rows, and the rest aliases into everything downstream.  Here each canvas pixel
 * is the mean of an Nx x Ny block of the UNFILTERED rule's samples.  For an entry whose source rect is sw x sh on the W x H canvas, with
 * max_factor 1..8: Nx = min(max_factor, max(1, ceil(sw / W))), Ny likewise from sh and H.  The fine frame F is what ht_draw_list_device
 * gives for the same entry on a canvas of Nx W x Ny H (the same rect, rx' = sw / (Nx W), ry' = sh / (Ny H) as one binary64 division each,
 * the same edge clamps, YUV taps converted first); per channel, alpha included, with n = Nx Ny:
 *   out(x, y) = (sum of F(Nx x + a, Ny y + b) over a < Nx, b < Ny  +  (n >> 1)) / n          (integer division)
 * Factors (1, 1) — max_factor 1, a source rect not larger than the canvas, an upscale — give ht_draw_list_device's bytes; where sw == Nx W
 * and sh == Ny H an RGBA entry's output is the exact integer box mean of the source block; a ratio above max_factor is clamped: the fine
 * frame then decimates itself, and the result is defined all the same.  srcs, n, dst_dev, dst_frame_stride, the binding, the overlap
 * refusals, the "entry <i>" messages and the enqueue-only contract are ht_draw_list_device's; max_factor outside 1..8 is HT_ERR_INVALID.
 * ONE launch.  Not part of this: filters other than the block mean, factors above 8, the single-source calls (ht_draw_frames*). */
ht_status ht_draw_list_filtered_device(ht_ctx *ctx, const ht_draw_source *srcs, int32_t n, int32_t max_factor, void *dst_dev, size_t dst_frame_stride);
/* The factors that call takes for a source rect of src_width x src_height (1..16384 each) on a canvas_width x canvas_height canvas: the
 * library's own rule, without a context or a device.  HT_ERR_INVALID (nothing written) for a NULL pointer or an argument out of range. */
ht_status ht_draw_filter_factors(int32_t src_width, int32_t src_height, int32_t canvas_width, int32_t canvas_height, int32_t max_factor, int32_t *nx,
                                 int32_t *ny);

/* ---- detect: ccv.grayscale + ccv.detect_objects (ccv.js:22-32, 109-246) ---------------------------------- */

/* Enqueues gray -> pyramid -> cascade scan for the bound frames on the stream and returns immediately. */
ht_status ht_detect_enqueue(ht_ctx *ctx, uint32_t flags);
/* Waits for the enqueued work, copies the raw hits back, sorted in the reference's emission order
 * (frame, scale, q, y, x) (ccv.js:154,178,181-182).  counts[f] = hits of frame f (counts may be NULL);
 * *total = all hits found.  HT_ERR_CAPACITY if total > cap (first cap hits in order are returned). */
ht_status ht_detect_collect(ht_ctx *ctx, ht_hit *hits, uint32_t cap, uint32_t *counts, uint32_t *total);
/* Convenience: set geometry if needed + upload + enqueue + collect, for host-resident frames. */
ht_status ht_detect_batch(ht_ctx *ctx, const uint8_t *host_rgba, int32_t n, int32_t width, int32_t height,
                          size_t frame_stride, uint32_t flags, ht_hit *hits, uint32_t cap, uint32_t *counts,
                          uint32_t *total);
/* Test hook: copies one pyramid plane of one frame back, rows packed (width*height bytes). */
ht_status ht_pyramid_readback(ht_ctx *ctx, int32_t frame, int32_t level, int32_t slot, uint8_t *out, size_t cap);
/* Scan statistics of the last collected batch (only if it was enqueued with HT_SCAN_STATS): windows that entered
 * stage j, j = 0..nstages (nstages = full survivors). */
ht_status ht_stage_counts(ht_ctx *ctx, uint64_t *counts, int32_t n);

/* ccv.grayscale drop-in on host RGBA frames, in place (R=G=B=gray, A untouched; ccv.js:22-32). */
ht_status ht_grayscale_batch(ht_ctx *ctx, uint8_t *host_rgba, int32_t n, int32_t width, int32_t height,
                             size_t frame_stride);
/* headtrackr.getWhitebalance (whitebalance.js:5-30) for the bound frames. */
ht_status ht_whitebalance_batch(ht_ctx *ctx, double *out, int32_t n);
/* The same values for the first n frames of the batch last enqueued with HT_DETECT_WHITEBALANCE (fused into the gray pass:
 * facetrackr's white-balance gate, facetrackr.js:79-95, and its detection read the frame once). Call after ht_detect_collect. */
ht_status ht_detect_whitebalance(ht_ctx *ctx, double *out, int32_t n);

/* ---- host-side post-processing of raw hits (O(n^2) on tens of rects) ------------------------------------ */

/* seq elements from hits (ccv.js:228-233, scale_x by repeated multiplication ccv.js:244-245). */
ht_status ht_hits_to_rects(const ht_ctx *ctx, const ht_hit *hits, uint32_t n, ht_rect *out);
/* ccv.array_group + averaging + nested-rect filter (ccv.js:34-107, 249-332). *nout <= n. */
ht_status ht_group_rects(const ht_rect *seq, uint32_t n, int32_t min_neighbors, ht_rect *out, uint32_t *nout);

/* facetrackr.Tracker.doVJDetection's selection for a whole batch (facetrackr.js:147-175): per frame, group the raw hits
 * with min_neighbors and keep the rect with the highest confidence (strict '>', first wins).  best[f].neighbors == 0 and
 * confidence == -10000 when frame f has no detection (facetrackr.js:239). counts[f] = raw hits of frame f, hits sorted as
 * ht_detect_collect returns them. */
ht_status ht_best_faces(const ht_ctx *ctx, const ht_hit *hits, const uint32_t *counts, int32_t nframes, int32_t min_neighbors,
                        ht_rect *best);

/* ht_detect_collect + ht_best_faces in one call for batch hosts: waits for the enqueued batch, sorts and groups its raw hits and
 * writes one rect per frame of the batch (facetrackr.js:147-175); the hits stay in the context.  *total_hits = raw hits found. */
ht_status ht_detect_collect_best(ht_ctx *ctx, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits);
/* The same, and as soon as the batch's raw hits are in host memory the NEXT batch of the currently bound frames is enqueued with
 * next_flags (ht_detect_enqueue) — before this batch is sorted and grouped, so the GPU is not one batch short while the host
 * post-processes.  A streaming host that swaps in new frames first (ht_swap_frames) gets them in that next batch. */
ht_status ht_detect_collect_best_requeue(ht_ctx *ctx, int32_t min_neighbors, ht_rect *best, uint32_t *total_hits, uint32_t next_flags);

/* ---- the same post-processing on the device: grouping and best face behind the scan, nothing but records crosses to the host ------ */

/* Enqueues, behind the detect batch in flight, the bucketing of its raw hits by frame and one workgroup per frame that orders them
 * (scale, q, y, x), forms the seq rects, runs ccv's grouping (ccv.js:34-107, 249-332) with min_neighbors and selects facetrackr's best
 * face (facetrackr.js:157-165).  Per frame f it leaves, in device buffers that live until the next call of this kind on the context, one
 * 64-byte record [x, y, width, height, confidence, neighbors, frame_base + f, 1.0] (binary64; no face: confidence -10000, neighbors 0,
 * rect 0), the frame's grouped list and a status word.  Legal between ht_detect_enqueue and the collect of that batch (HT_ERR_STATE
 * otherwise); waits for nothing in the steady state (the first call of a context, or a larger batch, allocates).  Every byte equals
 * ht_detect_collect_best's.  A frame with more raw hits than one workgroup takes (1024; option group_cap=N lowers it, results
 * unchanged) is flagged and finished on the host by the collect call. */
ht_status ht_detect_best_enqueue(ht_ctx *ctx, int32_t min_neighbors, int32_t frame_base);
/* Collects a batch that ht_detect_best_enqueue followed: ONE pinned device-to-host copy (hit count, records, status words) and one
 * synchronisation; best[f] for every frame of the batch, *total_hits = raw hits found.  HT_ERR_CAPACITY when the batch had more raw hits
 * than ht_config.hit_capacity.  The batch counts as collected exactly as after ht_detect_collect (ht_frames_enqueued,
 * ht_detect_whitebalance, ht_stage_counts). */
ht_status ht_detect_best_collect(ht_ctx *ctx, ht_rect *best, uint32_t *total_hits);
/* The same, and right behind the synchronisation the NEXT batch of the bound frames is enqueued with next_flags together with its
 * ht_detect_best_enqueue (same min_neighbors and frame_base).  That overwrites the device buffers: afterwards ht_detect_grouped and
 * ht_detect_best_records_device speak about the batch in flight, not the one just returned. */
ht_status ht_detect_best_collect_requeue(ht_ctx *ctx, ht_rect *best, uint32_t *total_hits, uint32_t next_flags);
/* The full grouped list of one frame of the batch collected last through ht_detect_best_collect — what ccv.detect_objects returns for
 * it.  *n = its length; HT_ERR_CAPACITY when cap is smaller (the first cap rects are returned); HT_ERR_STATE when no such batch exists
 * or a later ht_detect_best_enqueue / ht_group_hits has reused the buffers. */
ht_status ht_detect_grouped(ht_ctx *ctx, int32_t frame, ht_rect *out, uint32_t cap, uint32_t *n);
/* Device pointer of the 64-byte records (*nframes of them) for ht_allgather_records or a tensor view; fixed from ht_detect_best_enqueue
 * on, complete for work enqueued on the ctx stream or once the collect call has returned, valid until the next ht_detect_best_enqueue /
 * ht_group_hits on the context.  HT_ERR_STATE while no device-grouped batch exists. */
ht_status ht_detect_best_records_device(ht_ctx *ctx, const void **records, int32_t *nframes);
/* The device twin of ht_best_faces for hosts that hold raw hits: n hits in ANY order (each names its frame < nframes) go through the same
 * kernels.  best[nframes]; grouped (may be NULL together with ngrouped): room for n rects, the frames' grouped lists back to back in frame
 * order, ngrouped[f] rects each.  Waits for its result.  n <= ht_config.hit_capacity.  A hit whose frame or scale is out of range is
 * skipped and the call returns HT_ERR_INVALID.  Two hits of one frame with the same (scale, q, y, x) — the scan never emits that — are
 * ordered in an unspecified way.  HT_ERR_STATE while a device-grouped batch is in flight. */
ht_status ht_group_hits(ht_ctx *ctx, const ht_hit *hits, uint32_t n, int32_t nframes, int32_t min_neighbors, ht_rect *best, ht_rect *grouped,
                        uint32_t *ngrouped);

/* ---- camshift: camshift.Tracker (camshift.js:148-354), one tracker per stream ----------------------------- */

/* (Re)allocates per-stream tracker state for n streams. */
ht_status ht_camshift_reserve(ht_ctx *ctx, int32_t nstreams);
/* initTracker (camshift.js:198-211) for streams [first, first+n) using bound frames [0, n) and one rect each. */
ht_status ht_camshift_init_batch(ht_ctx *ctx, int32_t first, int32_t n, const ht_cs_rect *rects);
/* track (camshift.js:213-312) for streams [first, first+n) on bound frames [0, n); out[n] (may be NULL: enqueue only).  With out != NULL the call
 * returns the track objects; when no enqueue-only call is outstanding it takes the same route internally (pinned slot + completion marks, no
 * device-to-host copy, no stream synchronisation: option cs_sync_ring) — the results are the same either way. */
ht_status ht_camshift_track_batch(ht_ctx *ctx, int32_t first, int32_t n, int32_t calc_angles, ht_cs_trackobj *out);
/* Results of the OLDEST outstanding ht_camshift_track_batch that was enqueued with out == NULL (same n): waits for that call only and
 * copies its track objects.  Up to 4 enqueue-only calls may be outstanding per context (a fifth fails with HT_ERR_STATE): their kernels
 * write the track objects into a ring of pinned host slots, so a streaming host enqueues the track() of frame i + 1 before it waits for
 * frame i (the search window that links them lives on the device), and a host that serves several feeds on several contexts enqueues every
 * feed's track() first and collects afterwards (the reference's loop, main.js:168-180, is one feed; this is its K-feed form).
 * ht_camshift_reserve drops uncollected results. */
ht_status ht_camshift_track_collect(ht_ctx *ctx, int32_t n, ht_cs_trackobj *out);
/* The same two calls over an arbitrary list of (stream, frame) pairs: several trackers on one frame (one per face of a canvas, as the
 * reference allows), or the tracking feeds of a host whose feeds are in different states (main.js:229-244).  Streams are any reserved
 * slots in any order, each at most once per call; frames are any indices below ht_frames_bound(), repeats allowed.  The full-frame
 * histogram (camshift.js:268) is computed once per DISTINCT frame of the call and shared by the streams paired with it.  All argument
 * checks happen before anything is enqueued and a failed call changes no tracker state: HT_ERR_INVALID for a duplicate or unreserved
 * stream, a frame that is not bound, n <= 0, n > reserved streams, NULL pairs / rects; HT_ERR_STATE without bound frames.
 * initTracker (camshift.js:198-211) of pairs[i].stream on bound frame pairs[i].frame with rects[i]. */
ht_status ht_camshift_init_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_cs_rect *rects);
/* One track() (camshift.js:213-353) of pairs[i].stream on bound frame pairs[i].frame; out[n] in pair order.  out == NULL: enqueue only —
 * the results go into the same ring of pinned slots as ht_camshift_track_batch's (pair steps and batch steps may be outstanding
 * together, four in total, oldest first) and ht_camshift_track_collect(ctx, n, out) fetches them in pair order.  The results are the
 * bits of ht_camshift_track_batch's few-stream schedule (one mean-shift workgroup per stream).  Pairs (first + i, i), i = 0 .. n - 1, ARE
 * ht_camshift_track_batch(first, n) and take its schedules (option cs_pairs_force=1 sends them through the pair kernels).  Afterwards
 * ht_camshift_debug_hist(stream, .., current) returns the histogram of the frame the stream was paired with.
 * Option cs_pairs_cluster=1: a call of <= 64 pairs on frames of >= cs_cluster_min_px pixels runs a cluster of workgroups per pair, with
 * the bits of ht_camshift_track_batch's cluster schedule; a cluster that was not co-resident ends this call, or the collect of its slot,
 * with HT_ERR_STATE (the paired streams' state is then undefined: re-initialise them), as ht_camshift_track_batch does. */
ht_status ht_camshift_track_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t calc_angles, ht_cs_trackobj *out);
/* The hand-off from detection to tracking on the device (facetrackr.js:97-107: `confidence > threshold`, floor the rect, initTracker):
 * pairs[i].frame names a bound frame AND that frame's best-face record of the context's device-grouped batch — the batch
 * ht_detect_best_enqueue was issued behind, in flight or collected and not yet overwritten (HT_ERR_STATE without one).  Per pair, decided
 * once on the device: HT_CSB_DEFERRED when the record is not final there (more raw hits than ht_config.hit_capacity, a raw hit out of
 * range, or a frame over the grouping cap whose batch has not been collected yet: the collect completes it) — the stream keeps every
 * byte; HT_CSB_FACE when neighbors > 0 and confidence > min_confidence (strict; the reference's threshold is -10): initTracker
 * (camshift.js:198-211) of pairs[i].stream on bound frame pairs[i].frame with floor(x, y, width, height) of the record (int32, saturated,
 * NaN -> 0); otherwise HT_CSB_FALLBACK: initTracker with fallback[i] when fallback != NULL; otherwise HT_CSB_UNTOUCHED: model, search
 * window and track object keep every byte.  Enqueue only: ordered by the ctx stream behind the grouping and in front of whatever is
 * enqueued next, never copies a record to the host, never waits in the steady state (the first call of a context allocates).  The pair
 * list obeys the rules of ht_camshift_init_pairs; in addition pairs[i].frame must be below the grouped batch's frame count and
 * min_confidence must not be NaN (HT_ERR_INVALID).  Every check happens before anything is enqueued; a refused call changes no tracker
 * state.  The models are the bits ht_camshift_init_pairs produces for the same rects. */
enum { HT_CSB_UNTOUCHED = 0, HT_CSB_FACE = 1, HT_CSB_FALLBACK = 2, HT_CSB_DEFERRED = 3 };
ht_status ht_camshift_init_best(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, double min_confidence, const ht_cs_rect *fallback);
/* What the LAST ht_camshift_init_best of the context decided (same n): waits for that call only (an event behind its kernels) and returns
 * per pair the code and the rect that was used (zeros for untouched and deferred pairs); either pointer may be NULL.  May be called
 * repeatedly.  HT_ERR_STATE when there is no such call, when n differs, or after an ht_camshift_reserve that grew the reservation. */
ht_status ht_camshift_init_best_result(ht_ctx *ctx, int32_t n, int32_t *codes, ht_cs_rect *rects);
/* The same hand-off for EVERY grouped face of a frame: one tracker per face, decided on the device from the frame's grouped list (what
 * ht_detect_grouped returns) without copying it to the host.  The pairs of one frame, in list order, are that frame's slots S[0 .. k),
 * 1 <= k <= HT_CSF_MAX_SLOTS.  Per frame: when the frame is not final on the device (the three conditions of HT_CSB_DEFERRED above) every
 * slot gets HT_CSB_DEFERRED and keeps every byte.  Otherwise the eligible faces — neighbors > 0 && confidence > min_confidence, strict,
 * so a NaN confidence never is — are ordered by confidence descending, then list index ascending; the first k are kept, `dropped` counts
 * the eligible ones beyond them.  A face's rect is floor(x, y, width, height) as in ht_camshift_init_best.  Without HT_CSF_ASSOCIATE the
 * face of rank r goes to slot r.  With it, a slot is live when its stream's search window (the int32 window the last enqueued init or
 * track step left on the device; zeros since ht_camshift_reserve for a stream never initialised) has sw_width > 0 && sw_height > 0;
 * overlap(slot, face) is the area of the intersection of that window with the face's rect, in 64-bit integers (a rect with width or
 * height <= 0 has none); greedily, among unassigned live slots and unassigned faces with overlap > 0 the largest overlap is assigned —
 * ties to the lowest slot position, then the lowest rank — until no such pair is left; the remaining faces in rank order then take the
 * remaining slots: the not-live ones in ascending position first, then the unmatched live ones in ascending position.  So a tracker that
 * overlaps a detection keeps its slot across re-detections: the slot is the identity.  A slot with a face: HT_CSB_FACE and initTracker
 * (camshift.js:198-211) of its stream on the frame with the face's rect; any other slot: HT_CSB_UNTOUCHED, every byte kept.  Integer and
 * binary64 comparisons only: no tolerance anywhere.
 * Enqueue only; legal whenever ht_camshift_init_best is (HT_ERR_STATE otherwise); never waits in the steady state.  The pair list obeys
 * the rules of ht_camshift_init_pairs; in addition HT_ERR_INVALID for a frame outside the grouped batch, more than HT_CSF_MAX_SLOTS
 * slots on one frame, a NaN min_confidence and unknown flag bits; the message names the offending pair or frame.  Every check happens
 * before anything is enqueued; a refused call changes nothing.  The models are the bits ht_camshift_init_pairs produces for the same
 * rects. */
enum { HT_CSF_ASSOCIATE = 1 };
#define HT_CSF_MAX_SLOTS 16
typedef struct ht_csf_record {
    int32_t code, face;        /* HT_CSB_UNTOUCHED / _FACE / _DEFERRED; the face's index in the frame's grouped list, or -1 */
    ht_cs_rect rect;           /* the rect used; zeros for untouched and deferred slots */
    int32_t dropped, reserved; /* eligible faces of the frame beyond its slots (the same in every slot of the frame); 0 */
} ht_csf_record;               /* 32 bytes */
ht_status ht_camshift_init_faces(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, double min_confidence, uint32_t flags);
/* What the LAST ht_camshift_init_faces of the context decided (same n), one record per pair in pair order: waits for that call only.  May
 * be called repeatedly.  HT_ERR_STATE when there is no such call, when n differs, or after an ht_camshift_reserve that grew the
 * reservation. */
ht_status ht_camshift_init_faces_result(ht_ctx *ctx, int32_t n, ht_csf_record *out);
/* ncalls successive track() calls (camshift.js:213-220 called once per video frame, main.js:168-180) for streams
 * [first, first+n) in ONE host call: call k uses the n device-resident frames at dev_frames[k] (frame_stride bytes apart;
 * same geometry as ht_set_geometry).  A stream's calls are sequentially dependent (its search window), so they are
 * enqueued back to back on the ctx stream with no host round trip in between.  out (may be NULL: enqueue only) receives
 * the track objects of the LAST call (out_all == 0, n entries) or of every call (out_all != 0, ncalls*n entries, call-major). */
ht_status ht_camshift_track_sequence(ht_ctx *ctx, int32_t first, int32_t n, int32_t calc_angles, const void *const *dev_frames,
                                     int32_t ncalls, size_t frame_stride, ht_cs_trackobj *out, int32_t out_all);
/* Results of the last ht_camshift_track_sequence that was enqueued with out == NULL (same n / ncalls / out_all): waits for it and
 * copies the track objects.  Lets a host overlap the tracking of one batch of streams with other work on another context
 * (the reference's main.js:168-180 consumes the track object of frame k while the camera already delivers frame k+1). */
ht_status ht_camshift_sequence_collect(ht_ctx *ctx, int32_t n, int32_t ncalls, int32_t out_all, ht_cs_trackobj *out);
/* Measurement hook (B_track = 4*W*H + 4*sum of window areas): per stream, the pixels read by the window
 * moment passes (camshift.js:79-120 called from camshift.js:284-306) and the number of track() calls since the last reset. */
ht_status ht_camshift_stats(ht_ctx *ctx, int32_t first, int32_t n, uint64_t *window_pixels, uint64_t *calls, int32_t reset);
/* Test hook: one stream's model histogram (camshift.js:206-208) and the full-frame histogram of its last track() call
 * (camshift.js:268), 4096 bins each (camshift.Histogram, camshift.js:49-72).  Either pointer may be NULL. */
ht_status ht_camshift_debug_hist(ht_ctx *ctx, int32_t stream, uint32_t *model, uint32_t *current);

/* Output kinds of the back-projection calls: 4 bytes (v, v, v, 255) per pixel, v = floor(255 * pdf) — the bytes of
 * getBackProjectionImg().data (camshift.js:177-196) —, or one binary64 per pixel: getPdf()[x][y] stored at [y][x]. */
enum { HT_BP_RGBA8 = 0, HT_BP_F64 = 1 };
/* back-projection (camshift.js:172-196, 314-353) of bound frames [0, n) through the models of streams [first, first+n): per frame the
 * weights w[b] = cur[b] ? min(model[b] / cur[b], 1) : 0 of its own histogram against the stream's model, looked up for every pixel; rows
 * packed, frames out_stride bytes apart (0 = packed).  When the bound frame is the frame of the stream's last track() this is the
 * reference's _pdf.  Needs nothing a track call leaves behind and changes no tracker state; a reserved stream that was never
 * initialised yields zeros.  Waits for its result.  Every byte equals the reference's (integer and single binary64 operations only). */
ht_status ht_camshift_backproject(ht_ctx *ctx, int32_t first, int32_t n, int32_t kind, void *out_host, size_t out_stride);
/* The same into device memory (pointer and stride multiples of the element size: 4 bytes for HT_BP_RGBA8, 8 for HT_BP_F64): enqueued on the
 * ctx stream behind the outstanding track steps, never copies or waits. */
ht_status ht_camshift_backproject_device(ht_ctx *ctx, int32_t first, int32_t n, int32_t kind, void *out_dev, size_t out_stride);
/* The same two calls over an arbitrary list of (stream, frame) pairs: output i is bound frame pairs[i].frame through the model of stream
 * pairs[i].stream (every tracker of one canvas, or the tracking feeds of a host whose feeds are in different states).  kind, stride,
 * alignment and blocking / enqueue-only behaviour as above; the pair list obeys the rules of ht_camshift_track_pairs, and every check
 * happens before anything is enqueued.  The frame histogram is computed once per DISTINCT frame, and pairs that share a frame share one
 * pass over its pixels (groups of 4 for HT_BP_RGBA8, of 2 for HT_BP_F64).  Pairs (first + i, i) ARE the batch call above (option
 * cs_pairs_force=1 sends them through the pair kernels).  Uses the back-projection's own scratch: it may sit between enqueue-only pair or
 * batch track steps and changes nothing they or ht_camshift_stats / ht_camshift_debug_hist read.  The bytes are those of the batch call
 * on replicated frames. */
ht_status ht_camshift_backproject_pairs(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out_host, size_t out_stride);
ht_status ht_camshift_backproject_pairs_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, int32_t kind, void *out_dev, size_t out_stride);

/* ---- face crops: each tracker's box cut from its feed, on the device ------------------------------------------------------ */

/* Patch i is the box of a stream's track object — as the last track step enqueued before this call leaves it on the device —, widened by
 * margin_q8 / 256 around its centre (camshift.js:253-254: x, y is the centre), mapped from canvas coordinates back into the source through
 * the rect that was drawn onto the canvas, rounded outwards to whole source pixels, with HT_CROP_SQUARE grown to a square around its
 * middle, clamped to the source frame, and scaled to out_width x out_height by the declared resampler: drawImage(source, l, t, w, h, 0, 0,
 * out_width, out_height), byte for byte what ht_draw_list_device gives for that rect on a canvas of the patch size.  The rule is integer
 * arithmetic on the floored object (headtrackr_amd/csrc/ht_crop_plan.h states it); the ratios rx = w / out_width and ry = h / out_height
 * are one binary64 division each, done on the device.  HT_CROP_EMPTY — a lost 0 x 0 object, a stream that was never tracked, a box wider
 * than 65536 or centred beyond +-2^20, a box wholly outside the source — writes every byte of the patch as 0.  Rotation by the object's
 * angle is not part of this. */
enum { HT_CROP_EMPTY = 0, HT_CROP_FACE = 1 };
enum { HT_CROP_SQUARE = 1 };
typedef struct ht_crop_params {
    int32_t out_width, out_height; /* 1..1024 */
    int32_t margin_q8;             /* 64..1024; 256 is the box as tracked */
    uint32_t flags;                /* HT_CROP_SQUARE or 0 */
} ht_crop_params;
typedef struct ht_crop_record {
    int32_t code, stream; /* HT_CROP_*; the stream of the entry */
    ht_cs_rect rect;      /* source pixels; zeros when empty */
    double rx, ry;        /* 0 when empty */
} ht_crop_record;         /* 40 bytes */
/* Both calls: enqueue-only on the ctx stream behind whatever is outstanding; they never copy to the host and never wait in the steady state
 * (the first call of a context, or a longer list, allocates), and change nothing a later track step, ht_camshift_stats or
 * ht_camshift_debug_hist reads.  Patches are out_width * out_height * 4 bytes, out_stride apart (0 = packed, otherwise a multiple of 4 and
 * >= a patch) from out_dev (device memory, 4-byte aligned, not NULL).  1 <= n <= 65535; streams are any reserved slots and may repeat.
 * Any source plane that overlaps the output range is refused.  Every check happens before anything is enqueued: a refused call changes
 * nothing and names the offending entry as "entry <i>".  HT_ERR_STATE without geometry, without reserved streams and (pairs form)
 * without bound frames; HT_ERR_INVALID otherwise.
 * Pairs form: the source of pair i is bound frame pairs[i].frame (W x H RGBA, drawn 1:1), any index below ht_frames_bound(). */
ht_status ht_camshift_crop_pairs_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, void *out_dev, size_t out_stride);
/* Sources form: the source of entry i is srcs[i], described and checked as an entry of ht_draw_list_device; srcs[i].rect is the rect that
 * was drawn onto the canvas stream streams[i] tracks on (width == 0 && height == 0: the whole source). */
ht_status ht_camshift_crop_sources_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                          void *out_dev, size_t out_stride);
/* One record per entry of the LAST crop call of the context (same n): waits for that call only (an event behind its kernel).  May be called
 * repeatedly.  HT_ERR_STATE when there is no such call or n differs. */
ht_status ht_camshift_crop_result(ht_ctx *ctx, int32_t n, ht_crop_record *out);
/* Device pointer of those records (*n of them), complete for work enqueued on the ctx stream behind the crop call; valid until the next
 * crop call of the context.  HT_ERR_STATE while there is none. */
ht_status ht_camshift_crop_records_device(ht_ctx *ctx, const void **records, int32_t *n);

/* ---- angle-aligned face crops: each tracker's ROTATED box cut from its feed, upright, on the device ---------------------- */

/* With calcAngles (camshift.Tracker's default) width and height lie along the blob's principal axes and angle is the direction of the long
 * one; main.js:213-216 draws translate(x, y); rotate(angle - pi / 2); strokeRect(-w / 2, -h / 2, w, h).  Patch i is that rotated box of a
 * stream's track object — as the last track step enqueued before this call leaves it on the device —, widened by margin_q8 / 256 around its
 * centre, with HT_ALIGN_SQUARE both sides the longer one, mapped from canvas coordinates back into the source through the rect that was drawn
 * onto the canvas (an affine image: the mapping may be anisotropic), and sampled at out_width x out_height pixel centres: patch +x is
 * (sin a, -cos a) on the canvas, patch +y is (cos a, sin a), so at angle == pi / 2 the patch is the box as it stands.  The angle is rounded
 * to the nearest of 4096 steps per turn (a12); everything behind it is integer arithmetic in Q16 source pixels
 * (headtrackr_amd/csrc/ht_align_plan.h states the rule).  Each pixel is a bilinear blend, with 8-bit weights, of the source's declared RGBA
 * view, taps clamped to the source frame; a pixel whose sample centre lies outside the source frame is four zero bytes.  HT_ALIGN_EMPTY — a
 * lost 0 x 0 object, a stream that was never tracked, a box wider than 65536 or centred beyond +-2^20, an angle that is not finite or beyond
 * +-1024 — writes every byte of the patch as 0.  Not part of this: sub-pixel centres (x, y are floored as the crop calls floor them).
 * (Planar or float output: the _tensor calls below.  A prefilter for strong downscales: the _filtered calls below.) */
enum { HT_ALIGN_EMPTY = 0, HT_ALIGN_FACE = 1 };
enum { HT_ALIGN_SQUARE = 1 };
typedef struct ht_align_params {
    int32_t out_width, out_height; /* 1..1024 */
    int32_t margin_q8;             /* 64..1024; 256 is the box as tracked */
    uint32_t flags;                /* HT_ALIGN_SQUARE or 0 */
} ht_align_params;
typedef struct ht_align_record {
    int32_t code, stream, a12, pad; /* HT_ALIGN_*; the stream of the entry; the angle in 1/4096 turn (0 when empty); 0 */
    int64_t cx, cy;                 /* the box centre in the source, Q16; zeros when empty, as everything below */
    int64_t ux, uy;                 /* the patch's full-width vector in the source, Q16 */
    int64_t vx, vy;                 /* the patch's full-height vector in the source, Q16 */
} ht_align_record;                  /* 64 bytes */
/* Arguments, checks, refusals ("entry <i>"), status codes, output layout (RGBA8 patches out_stride apart, 0 = packed), the overlap refusal
 * and the enqueue-only contract are those of ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device.  The calls keep a descriptor
 * table, staging ring and records of their own: an align call and a crop call of one step share nothing. */
ht_status ht_camshift_align_pairs_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, void *out_dev, size_t out_stride);
ht_status ht_camshift_align_sources_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                           void *out_dev, size_t out_stride);
/* One record per entry of the LAST align call of the context (same n): waits for that call only.  HT_ERR_STATE when there is no such call
 * or n differs. */
ht_status ht_camshift_align_result(ht_ctx *ctx, int32_t n, ht_align_record *out);
/* Device pointer of those records (*n of them), complete for work enqueued on the ctx stream behind the align call; valid until the next
 * align call of the context.  HT_ERR_STATE while there is none. */
ht_status ht_camshift_align_records_device(ht_ctx *ctx, const void **records, int32_t *n);

/* ---- model-input tensors from face crops: planar float patches on the device ------------------------------------------- */

/* The crop and align calls above write RGBA8.  These four write the tensor a network reads, in the same single enqueue-only launch: f(patch),
 * where `patch` is byte for byte what the call of the same name without `_tensor` gives for the same arguments on the same tracker state,
 * and f is, per pixel and output channel c (headtrackr_amd/csrc/ht_patch_plan.h states the rule):
 *   b = the source byte: HT_PATCH_RGB bytes R, G, B; HT_PATCH_BGR bytes B, G, R; HT_PATCH_GRAY one channel, the ccv.grayscale byte of
 *       (R, G, B) (binary64, round half to even); alpha is dropped;
 *   v = fl32(fl32((float)b * scale[c]) + bias[c]): two binary32 operations, round to nearest even, never fused, subnormals kept;
 *   the element: the bits of v (HT_PATCH_F32), v rounded to binary16 (HT_PATCH_F16: nearest even, gradual underflow, overflow to infinity)
 *       or to bfloat16 (HT_PATCH_BF16: nearest even);
 *   HT_PATCH_CHW: C planes of out_height x out_width elements, packed; HT_PATCH_HWC: C elements per pixel, packed.
 * An EMPTY entry, and a pixel of an aligned patch whose sample centre lies outside the source, is therefore f of the zero byte — bias[c]
 * in the dtype —, not zero bytes; the record's `code` tells an empty entry from a black face.
 * scale[c] and bias[c] must be finite and 0 or of a magnitude within 2^-64 .. 2^64 (then no binary32 intermediate is subnormal or NaN);
 * the slots of channels the mode does not have (gray: 1 and 2) must be 0; pad must be 0.
 * Not part of this: an alpha or validity-mask channel, sub-pixel centres, per-entry formats, integer-quantised (int8) output.  (A prefilter
 * for strong downscales: the _filtered calls below, which take a format too.) */
enum { HT_PATCH_F32 = 0, HT_PATCH_F16 = 1, HT_PATCH_BF16 = 2 };
enum { HT_PATCH_CHW = 0, HT_PATCH_HWC = 1 };
enum { HT_PATCH_RGB = 0, HT_PATCH_BGR = 1, HT_PATCH_GRAY = 2 };
typedef struct ht_patch_format {
    int32_t dtype, layout, channels, pad; /* HT_PATCH_F32 .., HT_PATCH_CHW .., HT_PATCH_RGB ..; 0 */
    float scale[3], bias[3];              /* per output channel */
} ht_patch_format;                        /* 40 bytes */
/* Arguments, list rules, the "entry <i>" refusals, status codes and the enqueue-only contract are those of the call of the same name
 * without `_tensor`; format is not NULL and is checked, with everything else, before anything is enqueued.  A patch is C * out_width *
 * out_height * (4 or 2) bytes (C = 3, gray: 1); out_dev is 4-byte aligned; out_stride is 0 (a patch's bytes rounded up to 4) or a multiple
 * of 4 that is at least a patch's bytes, so a 16-bit plane of odd out_width * out_height starts 2-byte aligned.  The overlap refusal
 * uses the tensor's own byte range.  A tensor call IS the context's last crop (or align) call: ht_camshift_crop_result /
 * ht_camshift_crop_records_device (ht_camshift_align_result / ht_camshift_align_records_device) report on it, with the records the RGBA
 * call would have written. */
ht_status ht_camshift_crop_pairs_tensor_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, const ht_patch_format *format,
                                               void *out_dev, size_t out_stride);
ht_status ht_camshift_crop_sources_tensor_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                 const ht_patch_format *format, void *out_dev, size_t out_stride);
ht_status ht_camshift_align_pairs_tensor_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, const ht_patch_format *format,
                                                void *out_dev, size_t out_stride);
ht_status ht_camshift_align_sources_tensor_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                  const ht_patch_format *format, void *out_dev, size_t out_stride);

/* ---- prefiltered face crops: block-mean patches for strong downscales ----------------------------------------------------- */

/* The calls above sample one bilinear tap pair per patch pixel: a face 792 source pixels wide cut to 112 x 112 reads 2 of every 7 source
 * rows and columns, and the rest aliases.  These four write each patch pixel as the mean of an Nx x Ny block of the UNFILTERED rule's
 * samples, in the same single enqueue-only launch (headtrackr_amd/csrc/ht_filter_plan.h states the rule).  The factors are chosen per
 * entry on the device, from the tracked box, with P x Q = out_width x out_height and max_factor 1..8:
 *   crop:   Nx = min(max_factor, max(1, ceil(w / P))), Ny = min(max_factor, max(1, ceil(h / Q))), (l, t, w, h) the crop rule's rect;
 *   align:  Nx = min(max_factor, max(1, ceil((|ux| + |uy|) / (P * 65536)))), Ny the same with (vx, vy) and Q: the L1 norm never
 *           under-samples, and upright (a12 == 1024) it is the crop's w / P.
 * The fine patch F is what the unfiltered call of the same name gives for the same entry at Nx * P x Ny * Q (crop: drawImage of the same
 * rect with rx' = w / (Nx * P), ry' = h / (Ny * Q), one binary64 division each; align: the terms of column i of Nx * P and row j of
 * Ny * Q with the same centre and vectors, the range test and the four zero bytes of a sample outside the frame as they are), and per
 * channel, alpha included, with n = Nx * Ny:
 *   out(x, y) = (sum of F(Nx * x + a, Ny * y + b) over a < Nx, b < Ny + (n >> 1)) / n        (integer division)
 * So with Nx == Ny == 1 — max_factor 1, or a box that is not downscaled — the patch is byte for byte the unfiltered call's; where
 * w == Nx * P and h == Ny * Q exactly it is the exact integer box mean of the source block; an empty entry is zeros; an aligned patch's edge
 * fades where fine samples fall outside the frame.  format == NULL: RGBA8, the output layout of the RGBA calls.  Otherwise the output is
 * f(filtered patch) with f, the layout, the stride rule and the format check of the _tensor calls (gray is taken from the filtered R, G, B).
 * Arguments, list rules, the "entry <i>" refusals, the overlap refusal, status codes and the enqueue-only contract are those of the call of
 * the same name without `_filtered`, whose table, ring and records are used: a filtered call IS the context's last crop (or align) call,
 * and ht_camshift_crop_result / ht_camshift_align_result report the records the unfiltered call would have written (crop: rx = w / P).
 * max_factor outside 1..8: HT_ERR_INVALID, before anything is enqueued.
 * Not part of this: filters other than the block mean, factors above 8, sub-pixel centres, per-entry formats, int8 output.  (The canvas
 * draw has the same prefilter: ht_draw_list_filtered_device.) */
ht_status ht_camshift_crop_pairs_filtered_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_crop_params *params, int32_t max_factor,
                                                 const ht_patch_format *format, void *out_dev, size_t out_stride);
ht_status ht_camshift_crop_sources_filtered_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_crop_params *params,
                                                   int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride);
ht_status ht_camshift_align_pairs_filtered_device(ht_ctx *ctx, const ht_cs_pair *pairs, int32_t n, const ht_align_params *params, int32_t max_factor,
                                                  const ht_patch_format *format, void *out_dev, size_t out_stride);
ht_status ht_camshift_align_sources_filtered_device(ht_ctx *ctx, const int32_t *streams, const ht_draw_source *srcs, int32_t n, const ht_align_params *params,
                                                    int32_t max_factor, const ht_patch_format *format, void *out_dev, size_t out_stride);
/* The factors a filtered call of (out_width, out_height, max_factor) takes for the entry of *record: a pure function of the record, so a
 * caller never restates the rule.  No context, no device.  An empty record gives 0, 0.  HT_ERR_INVALID for a NULL argument, out_width or
 * out_height outside 1..1024, max_factor outside 1..8. */
ht_status ht_camshift_crop_filter_factors(const ht_crop_record *record, int32_t out_width, int32_t out_height, int32_t max_factor, int32_t *nx, int32_t *ny);
ht_status ht_camshift_align_filter_factors(const ht_align_record *record, int32_t out_width, int32_t out_height, int32_t max_factor, int32_t *nx, int32_t *ny);

/* ---- multi-GPU: fixed-size result records, all-gathered over RCCL/xGMI ------------------------------------ */

/* Single-process helper for hosts that drive several GPUs from one process (the Node addon): ctxs[i] are contexts
 * on distinct devices; records_dev[i] points to nranks*bytes_per_rank bytes of device memory on ctxs[i]'s device
 * with rank i's own records already at offset i*bytes_per_rank.  Performs one ncclAllGather per rank in a group. */
ht_status ht_allgather_records(ht_ctx *const *ctxs, int32_t nranks, void *const *records_dev, size_t bytes_per_rank);
/* The exchange step of the frame-sharded path for a single-process host (BASELINE.json: "RCCL all-gather of bounding boxes"):
 * best[i] = rank i's ht_best_faces output for its frames_per_rank frames (host memory; pad short ranks with zero rects).
 * Uploads every rank's rects into its own GPU's slot, runs ht_allgather_records, reads every rank's table back, requires
 * them to be identical and returns the table (nranks*frames_per_rank rects, rank-major) — what facetrackr.Tracker.doVJDetection
 * (facetrackr.js:147-175) would have produced for every frame of the batch, now known on every GPU. */
ht_status ht_allgather_best_faces(ht_ctx *const *ctxs, int32_t nranks, const ht_rect *const *best, int32_t frames_per_rank,
                                  ht_rect *gathered);
/* Number of HIP devices visible to the process (0 if none); the `devices` option of the JS batch entry points indexes them. */
int32_t ht_device_count(void);

/* ---- measurement --------------------------------------------------------------------------------------- */

/* on != 0: bracket every kernel of subsequent ht_detect_* / camshift calls with HIP events on the ctx stream. */
ht_status ht_profile(ht_ctx *ctx, int32_t on);
/* Device times accumulated since profiling was switched on (or last reset); *n in: capacity, out: entries.  Profiling on or off, the
 * entries cs_fused_launches_1024 / cs_fused_launches_512 (ms = 0) count the single-launch camshift kernel's launches per form since the
 * last reset (the form is chosen per launch, option cs_fused_nt). */
ht_status ht_kernel_times(ht_ctx *ctx, ht_kernel_time *out, int32_t *n, int32_t reset);
void *ht_stream(const ht_ctx *ctx); /* the hipStream_t the ctx enqueues on */
/* ht_detect_enqueue calls served by replaying a captured hipGraph (batches of <= 256 frames, option graph_max_frames: the ~10 dependent launches of a detect
 * sequence are captured once per (frames pointer, count, flags) and replayed with one hipGraphLaunch). */
uint64_t ht_graph_launches(const ht_ctx *ctx);
ht_status ht_synchronize(ht_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* HEADTRACKR_HIP_H */

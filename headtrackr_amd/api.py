"""Host-side Python mirror of the reference's per-frame interface, on top of the C ABI (include/headtrackr_hip.h).

The primary host language of this project is JavaScript (headtrackr_amd/js/headtrackr.js over the N-API addon); this
module exposes the same operations to Python so that the parity tests (pytest) and bench.py can drive the same C ABI.
Names follow the reference: ccv.grayscale / ccv.detect_objects (src/ccv.js:22,109), camshift.Tracker
(src/camshift.js:148), getWhitebalance (src/whitebalance.js:5).  Every method calls the HIP library; none computes on
the CPU except ccv's own O(n^2) grouping of a few dozen rectangles on the default route (detect_collect_best); detect_best_enqueue /
detect_best_collect run that stage on the device too.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import native
from .cascade import Cascade, load_cascade
from .native import (HIT_DTYPE, HT_INPUT_GRAY_IN_R, HT_INPUT_RGBA, HT_SCAN_NO_SPLIT, HT_SCAN_SIMPLE, RECT_DTYPE,  # noqa: F401
                     HtError)


class PatchFormat:
    """The output of a tensor call (ht_patch_format): every element is fl32(fl32(byte * scale[c]) + bias[c]) rounded to `dtype` — "f32",
    "f16" or "bf16" — in `layout` "chw" or "hwc" with `channels` "rgb", "bgr" or "gray" (one channel: the grayscale byte).  scale and bias
    are one number for all channels or one per output channel; each is 0 or of a magnitude within 2^-64 .. 2^64."""

    def __init__(self, dtype: str = "f16", layout: str = "chw", channels: str = "rgb", scale=1.0 / 255.0, bias=0.0):
        for what, value, table in (("dtype", dtype, native.PATCH_DTYPES), ("layout", layout, native.PATCH_LAYOUTS), ("channels", channels, native.PATCH_CHANNELS)):
            if value not in table:
                raise ValueError(f"PatchFormat: {what} must be one of {sorted(table)}, not {value!r}")
        self.dtype, self.layout, self.channels = dtype, layout, channels
        self.scale, self.bias = self._per_channel("scale", scale), self._per_channel("bias", bias)

    @property
    def nchannels(self) -> int:
        return 1 if self.channels == "gray" else 3

    @property
    def itemsize(self) -> int:
        return 4 if self.dtype == "f32" else 2

    def _per_channel(self, what, v):
        n = self.nchannels
        vals = [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]
        if len(vals) == 1:
            vals = vals * n
        if len(vals) != n:
            raise ValueError(f"PatchFormat: {what} takes one value or {n} (one per output channel)")
        return tuple(float(np.float32(x)) for x in vals)  # binary64 -> binary32, round to nearest even

    @classmethod
    def mean_std(cls, mean, std, dtype: str = "f16", layout: str = "chw", channels: str = "rgb"):
        """(byte / 255 - mean) / std per output channel: scale = 1 / (255 std), bias = -mean / std, computed in binary64 and then rounded
        to binary32"""
        mean, std = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(std, dtype=np.float64).reshape(-1)
        return cls(dtype, layout, channels, scale=1.0 / (255.0 * std), bias=-mean / std)

    def patch_bytes(self, width: int, height: int) -> int:
        return self.nchannels * int(width) * int(height) * self.itemsize

    def default_stride(self, width: int, height: int) -> int:
        return (self.patch_bytes(width, height) + 3) & ~3

    def shape(self, width: int, height: int):
        return (self.nchannels, int(height), int(width)) if self.layout == "chw" else (int(height), int(width), self.nchannels)

    def struct(self) -> "native.PATCH_FORMAT":
        f = native.PATCH_FORMAT(native.PATCH_DTYPES[self.dtype], native.PATCH_LAYOUTS[self.layout], native.PATCH_CHANNELS[self.channels], 0)
        for c in range(self.nchannels):
            f.scale[c], f.bias[c] = self.scale[c], self.bias[c]
        return f

    @classmethod
    def of(cls, fmt):
        """a PatchFormat, or a dict of its constructor's arguments"""
        return fmt if isinstance(fmt, cls) else cls(**fmt)


class Context:
    """One ht_ctx: one GPU, one cascade, one stream."""

    def __init__(self, cascade: Cascade | None = None, device: int = 0, interval: int = 5, stream: int | None = None,
                 hit_capacity: int = 0, queue_capacity: int = 0, options: str | dict | None = None):
        """options: ht_config.options — "key=value,..." or a dict (schedule selectors for tests / A-B runs; results never change)"""
        self._lib = native.lib()
        self.cascade = cascade or load_cascade()
        if isinstance(options, dict):
            options = ",".join(f"{k}={int(v)}" for k, v in options.items())
        cfg = native.Config(C.sizeof(native.Config), device, interval, hit_capacity, stream, queue_capacity, 0, options.encode() if options else None)
        h = C.c_void_p()
        blob = self.cascade.blob
        st = self._lib.ht_create(C.byref(cfg), blob, len(blob), C.byref(h))
        if st != 0:
            raise HtError(st, self._lib.ht_last_error(None).decode())
        self._h = h
        self.device = device
        self.interval = interval
        self.width = self.height = 0
        self._collected_n = 0
        self.nframes = 0   # frames currently bound (upload / bind_device / swap_frames)

    # -- plumbing -------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.ht_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, allow=()):
        if st != 0 and st not in allow:
            raise HtError(st, self._lib.ht_last_error(self._h).decode())
        return st

    # -- geometry / frames ------------------------------------------------------------------------------------
    def set_geometry(self, width: int, height: int, max_batch: int, level_dims=None):
        if level_dims is not None:
            ld = np.ascontiguousarray(level_dims, dtype=np.int32).reshape(-1)
            self._check(self._lib.ht_set_geometry(self._h, width, height, max_batch, ld.ctypes.data, ld.size // 2))
        else:
            self._check(self._lib.ht_set_geometry(self._h, width, height, max_batch, None, 0))
        self.width, self.height = width, height

    @property
    def num_levels(self) -> int:
        return self._lib.ht_num_levels(self._h)

    @property
    def windows_per_frame(self) -> int:
        return self._lib.ht_windows_per_frame(self._h)

    @property
    def pyramid_bytes_per_frame(self) -> int:
        return self._lib.ht_pyramid_bytes_per_frame(self._h)

    def plane(self, level: int, slot: int = 0):
        p = native.PlaneInfo()
        self._check(self._lib.ht_plane(self._h, level, slot, C.byref(p)))
        return p

    def upload(self, frames: np.ndarray):
        """frames: uint8 [n, H, W, 4] host array."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n, h, w, c = frames.shape
        assert c == 4 and (w, h) == (self.width, self.height), "call set_geometry(w, h, max_batch) first"
        self._check(self._lib.ht_upload_frames(self._h, frames.ctypes.data, n, w * h * 4))
        self.nframes = n

    def upload_ptr(self, host_ptr: int, n: int, frame_stride: int | None = None):
        """Like upload(), from a raw host pointer (e.g. pinned memory: the copy then runs at PCIe speed)."""
        self._check(self._lib.ht_upload_frames(self._h, host_ptr, n, frame_stride or self.width * self.height * 4))
        self.nframes = n

    def upload_async_ptr(self, host_ptr: int, n: int, frame_stride: int | None = None):
        """Starts copying the NEXT n frames from pinned host memory into the back buffer on the copy stream; the kernels of
        the current frames keep running.  swap_frames() makes them current."""
        self._check(self._lib.ht_upload_frames_async(self._h, host_ptr, n, frame_stride or self.width * self.height * 4))
        self._back_n = n

    def swap_frames(self):
        self._check(self._lib.ht_swap_frames(self._h))
        self.nframes = self._back_n

    def bind_device(self, dev_ptr: int, n: int, frame_stride: int | None = None):
        """Use n RGBA frames already resident in device memory (e.g. a torch cuda tensor's data_ptr())."""
        self._check(self._lib.ht_bind_frames_device(self._h, dev_ptr, n, frame_stride or self.width * self.height * 4))
        self.nframes = n

    def device_download(self, dev_ptr: int, nbytes: int) -> np.ndarray:
        """nbytes of device memory at dev_ptr as a uint8 array, copied behind everything enqueued on the context's stream so far"""
        out = np.empty(nbytes, dtype=np.uint8)
        self._check(self._lib.ht_device_download(self._h, out.ctypes.data, dev_ptr, nbytes))
        return out

    # -- ingest: the loop's video -> canvas drawImage (main.js:170) ----------------------------------------------
    @staticmethod
    def _cs_rect(rect):
        if rect is None:
            return None
        r = np.zeros(1, dtype=native.CS_RECT_DTYPE)
        r[0] = tuple(int(v) for v in rect)
        return r

    def draw_frames(self, src: np.ndarray, rect=None):
        """drawImage(video, sx, sy, sw, sh, 0, 0, W, H) for a host array src, uint8 [n, sh, sw, 4], onto the context's W x H geometry
        (rect = (x, y, width, height) inside the source, None = the whole frame): scaled on the device, result bound like upload()."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        n, h, w, c = src.shape
        assert c == 4
        r = self._cs_rect(rect)
        self._check(self._lib.ht_draw_frames(self._h, src.ctypes.data, n, w, h, 0, r.ctypes.data if r is not None else None))
        self.nframes = n

    def draw_frames_device(self, ptr: int, n: int, sw: int, sh: int, pitch: int = 0, stride: int = 0, rect=None, dst: int | None = None,
                           dst_stride: int = 0):
        """The same for n device-resident source frames of sw x sh pixels at ptr (rows `pitch` bytes, frames `stride` bytes apart,
        0 = packed).  dst None: into the context's own frame buffer, which becomes the bound frames; otherwise into device memory at
        dst (frames dst_stride apart), binding untouched.  Enqueued on the context's stream, no copy, no wait."""
        r = self._cs_rect(rect)
        self._check(self._lib.ht_draw_frames_device(self._h, ptr, n, sw, sh, pitch, stride, r.ctypes.data if r is not None else None, dst, dst_stride))
        if dst is None:
            self.nframes = n

    # -- the same draw for YUV frames (4:2:0 NV12 / I420, packed 4:2:2 YUYV / UYVY): conversion fused into the draw ----
    @staticmethod
    def _yuv_code(table, v, what):
        if isinstance(v, str):
            if v not in table:
                raise ValueError(f"{what} is one of {sorted(table)}")
            return table[v]
        return int(v)

    @staticmethod
    def _oriented(code: int, orientation) -> int:
        """a format code with the orientation 0..7 in bits 8..10 (HT_ORIENT of headtrackr_hip.h)"""
        return int(code) | orientation_bits(orientation)

    def draw_frames_yuv(self, planes, fmt="nv12", matrix="bt601", rect=None, width=None, height=None, orientation=0):
        """planes: host arrays of n frames — NV12: (y uint8 [n, h, w], uv uint8 [n, ch, cw, 2]); I420: (y, u [n, ch, cw], v [n, ch, cw]) with
        cw = ceil(w / 2), ch = ceil(h / 2) — packed frame by frame and drawn like draw_frames(): converted with the declared integer matrix
        ('bt601', 'bt709', 'bt601-full', 'bt709-full' or 0 .. 3), scaled on the device, result bound.
        fmt 'yuyv' / 'uyvy' (packed 4:2:2): planes is ONE uint8 array, [n, h, 4 cw] (rows of cw macropixels; width defaults to 2 cw, pass
        width = 2 cw - 1 for an odd frame) or flat with width and height given (n = size / (4 cw h)); staged at 2 B/px.
        orientation 0..7 (orientation_from_exif / orientation_from_rotation): the planes are the frames AS STORED, the draw is that of the
        oriented frame and rect is in its coordinates."""
        orient = orientation_bits(orientation)
        fmt, matrix = self._yuv_code(native.YUV_FORMATS, fmt, "fmt"), self._yuv_code(native.YUV_MATRICES, matrix, "matrix")
        if fmt in native.YUV_PACKED_422:
            host = np.ascontiguousarray(planes, dtype=np.uint8)
            if host.ndim == 3:
                n, h, row = host.shape
                w = int(width) if width is not None else row // 2
                if height is not None and int(height) != h:
                    raise ValueError("draw_frames_yuv: height differs from the array's rows")
            else:
                if host.ndim != 1 or width is None or height is None:
                    raise ValueError("draw_frames_yuv: a packed 4:2:2 array is [n, h, 4 * ceil(w / 2)], or flat with width and height given")
                w, h = int(width), int(height)
                row = 4 * ((w + 1) // 2)
                n = host.size // (row * h) if row * h > 0 else 0
            if w <= 0 or h <= 0 or row != 4 * ((w + 1) // 2) or n <= 0 or host.size != n * row * h:
                raise ValueError("draw_frames_yuv: a packed 4:2:2 frame is h rows of 4 * ceil(w / 2) bytes (width is 2 cw or 2 cw - 1)")
            return self.draw_frames_yuv_ptr(host.ctypes.data, n, w, h, fmt | orient, matrix, 0, rect)
        planes = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
        n, h, w = planes[0].shape
        assert len(planes) == (2 if fmt == native.HT_YUV_NV12 else 3) and all(len(p) == n for p in planes)
        host = np.concatenate([p.reshape(n, -1) for p in planes], axis=1)
        assert host.shape[1] == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2), "chroma planes are ceil(w / 2) x ceil(h / 2)"
        self.draw_frames_yuv_ptr(host.ctypes.data, n, w, h, fmt | orient, matrix, 0, rect)

    def draw_frames_yuv_ptr(self, host_ptr: int, n: int, w: int, h: int, fmt: int, matrix: int, frame_stride: int = 0, rect=None):
        """ht_draw_frames_yuv on a raw host pointer: n tightly packed frames (Y, then UV or U, V; YUYV / UYVY: the one packed plane),
        frame_stride bytes apart (0 = packed).  fmt: the format code, with HT_ORIENT bits if the frames are oriented"""
        r = self._cs_rect(rect)
        self._check(self._lib.ht_draw_frames_yuv(self._h, host_ptr, n, w, h, fmt, matrix, frame_stride, r.ctypes.data if r is not None else None))
        self.nframes = n

    def draw_frames_yuv_device(self, y: int, u: int, v: int | None, n: int, w: int, h: int, fmt="nv12", matrix="bt601", y_pitch: int = 0, c_pitch: int = 0,
                               stride: int = 0, rect=None, dst: int | None = None, dst_stride: int = 0, orientation=0):
        """The same for planes resident in device memory at y / u / v (NV12: u = the interleaved plane, v None), rows y_pitch / c_pitch bytes
        (0 = packed), frames `stride` bytes apart in every plane.  fmt 'yuyv' / 'uyvy': only y and y_pitch are read (the packed plane, base
        and pitch multiples of 4); u, v and c_pitch are not looked at.  dst as draw_frames_device().  orientation 0..7: w, h, the
        pitches and the planes describe the frames as stored; rect is in the oriented frame's coordinates."""
        d = native.YUV_FRAMES(y, u, v, y_pitch, c_pitch, stride, w, h, self._oriented(self._yuv_code(native.YUV_FORMATS, fmt, "fmt"), orientation), self._yuv_code(native.YUV_MATRICES, matrix, "matrix"))
        r = self._cs_rect(rect)
        self._check(self._lib.ht_draw_frames_yuv_device(self._h, C.byref(d), n, r.ctypes.data if r is not None else None, dst, dst_stride))
        if dst is None:
            self.nframes = n

    # -- one launch for a list of per-feed sources ----------------------------------------------------------------
    def draw_list(self, entries, dst: int | None = None, dst_stride: int = 0, prefilter: int | None = None):
        """entries: one dict per feed, drawn onto destination frame i in ONE launch (ht_draw_list_device) —
        {"format": 'rgba' | 'nv12' | 'i420' | 'yuyv' | 'uyvy' (or the code), "width", "height", "p0", "p1", "p2" (device pointers: RGBA p0;
        NV12 Y, UV; I420 Y, U, V; YUYV / UYVY p0 alone — p1, p2 and pitch1 are not read), "pitch0", "pitch1" (bytes per row, 0 = packed), "matrix" (as draw_frames_yuv_device, ignored for RGBA), "rect" (x, y,
        width, height) or None = the whole source, "orientation" 0..7 (orientation_from_exif / orientation_from_rotation; default 0): width,
        height, pitches and pointers describe the frame AS STORED, the entry is drawn as the oriented frame and rect is in ITS coordinates}.  Every feed may have its own allocation, size, format, matrix and rect; pointers may
        repeat.  dst as draw_frames_device().  prefilter = 1..8: ht_draw_list_filtered_device with that max_factor — every canvas pixel the
        mean of a block of the unfiltered draw's samples (draw_filter_factors gives the block per entry); None: the unfiltered call."""
        n = len(entries)
        if prefilter is None:
            self._check(self._lib.ht_draw_list_device(self._h, self._draw_sources(entries), n, dst, dst_stride))
        else:
            self._check(self._lib.ht_draw_list_filtered_device(self._h, self._draw_sources(entries), n, int(prefilter), dst, dst_stride))
        if dst is None:
            self.nframes = n

    def _draw_sources(self, entries):
        """the ht_draw_source array of a list of entry dicts (draw_list, camshift_crop_sources_device)"""
        arr = (native.DRAW_SOURCE * max(len(entries), 1))()
        for s, e in zip(arr, entries):
            s.p0, s.p1, s.p2 = e.get("p0"), e.get("p1"), e.get("p2")
            s.pitch0, s.pitch1 = int(e.get("pitch0", 0)), int(e.get("pitch1", 0))
            s.width, s.height = int(e["width"]), int(e["height"])
            s.format = self._oriented(self._yuv_code(native.DRAW_LIST_FORMATS, e.get("format", "rgba"), "format"), e.get("orientation", 0))
            s.matrix = self._yuv_code(native.YUV_MATRICES, e.get("matrix", "bt601"), "matrix")
            if e.get("rect") is not None:
                s.rect = native.CS_RECT(*(int(v) for v in e["rect"]))
        return arr

    # -- detect -----------------------------------------------------------------------------------------------
    def detect_enqueue(self, flags: int = HT_INPUT_RGBA):
        self._check(self._lib.ht_detect_enqueue(self._h, flags))

    # The library sizes what it writes (counts[], best[]) by the batch that was ENQUEUED, not by what is bound at collect time
    # (a streaming host binds or swaps in the next frames in between): the buffers below follow ht_frames_enqueued.
    def detect_collect(self, cap: int = 1 << 16):
        n = self._collected_n = int(self._lib.ht_frames_enqueued(self._h))  # the library's own count of the batch in flight
        buf = getattr(self, "_hitbuf", None)
        if buf is None or len(buf) < cap:
            buf = self._hitbuf = np.empty(cap, dtype=HIT_DTYPE)  # reused across calls
        counts = np.empty(max(1, n), dtype=np.uint32)
        total = C.c_uint32(0)
        self._check(self._lib.ht_detect_collect(self._h, buf.ctypes.data, cap, counts.ctypes.data, C.byref(total)))
        return buf[: total.value].copy(), counts[:n]

    def detect_collect_best(self, min_neighbors: int = 1, out: np.ndarray | None = None):
        """ht_detect_collect + ht_best_faces in one C call: (best rect per frame of the enqueued batch, raw hit count)."""
        n = self._collected_n = int(self._lib.ht_frames_enqueued(self._h))  # the library's own count of the batch in flight
        if out is None or len(out) < n:
            out = np.zeros(max(1, n), dtype=RECT_DTYPE)
        total = C.c_uint32(0)
        self._check(self._lib.ht_detect_collect_best(self._h, min_neighbors, out.ctypes.data, C.byref(total)))
        return out[:n], total.value

    def detect_collect_best_requeue(self, min_neighbors: int = 1, out: np.ndarray | None = None, next_flags: int = HT_INPUT_RGBA):
        """detect_collect_best, and the next batch of the bound frames is enqueued as soon as this batch's raw hits are on the host
        (before they are sorted and grouped)."""
        n = self._collected_n = int(self._lib.ht_frames_enqueued(self._h))  # the library's own count of the batch in flight
        if out is None or len(out) < n:
            out = np.zeros(max(1, n), dtype=RECT_DTYPE)
        total = C.c_uint32(0)
        self._check(self._lib.ht_detect_collect_best_requeue(self._h, min_neighbors, out.ctypes.data, C.byref(total), next_flags))
        return out[:n], total.value

    # -- the same on the device: grouping and best face behind the scan (ht_group.hip) -----------------------------------------
    def detect_best_enqueue(self, min_neighbors: int = 1, frame_base: int = 0):
        """behind detect_enqueue(): bucket the batch's raw hits by frame, group them and select each frame's best face on the device"""
        self._check(self._lib.ht_detect_best_enqueue(self._h, min_neighbors, frame_base))

    def detect_best_collect(self, out: np.ndarray | None = None):
        """collects a batch that detect_best_enqueue() followed: (best rect per frame, raw hit count) — one pinned copy, one wait"""
        n = self._collected_n = int(self._lib.ht_frames_enqueued(self._h))
        if out is None or len(out) < n:
            out = np.zeros(max(1, n), dtype=RECT_DTYPE)
        total = C.c_uint32(0)
        self._check(self._lib.ht_detect_best_collect(self._h, out.ctypes.data, C.byref(total)))
        return out[:n], total.value

    def detect_best_collect_requeue(self, out: np.ndarray | None = None, next_flags: int = HT_INPUT_RGBA):
        """detect_best_collect, and the next batch of the bound frames with its device grouping is enqueued right behind the wait"""
        n = self._collected_n = int(self._lib.ht_frames_enqueued(self._h))
        if out is None or len(out) < n:
            out = np.zeros(max(1, n), dtype=RECT_DTYPE)
        total = C.c_uint32(0)
        self._check(self._lib.ht_detect_best_collect_requeue(self._h, out.ctypes.data, C.byref(total), next_flags))
        return out[:n], total.value

    def detect_grouped(self, frame: int) -> np.ndarray:
        """the full grouped list (ccv.detect_objects' result) of one frame of the batch detect_best_collect() returned last"""
        n = C.c_uint32(0)
        st = self._lib.ht_detect_grouped(self._h, frame, None, 0, C.byref(n))
        self._check(st, allow=(native.HT_ERR_CAPACITY,))
        out = np.zeros(max(1, n.value), dtype=RECT_DTYPE)
        if n.value:
            self._check(self._lib.ht_detect_grouped(self._h, frame, out.ctypes.data, n.value, C.byref(n)))
        return out[: n.value]

    def detect_best_records_ptr(self):
        """(device pointer, frames) of the 64-byte per-frame records [x, y, width, height, confidence, neighbors, frame index, 1.0] of the
        device-grouped batch: valid until the next detect_best_enqueue() / group_hits() on this context"""
        p, n = C.c_void_p(0), C.c_int32(0)
        self._check(self._lib.ht_detect_best_records_device(self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def group_hits(self, hits: np.ndarray, nframes: int, min_neighbors: int = 1):
        """the device twin of best_faces() for an unsorted hit list: (best rect per frame, grouped rects of all frames back to back in
        frame order, their per-frame counts)"""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        best = np.zeros(max(1, nframes), dtype=RECT_DTYPE)
        grouped = np.zeros(max(1, len(hits)), dtype=RECT_DTYPE)
        ngrouped = np.zeros(max(1, nframes), dtype=np.uint32)
        self._check(self._lib.ht_group_hits(self._h, hits.ctypes.data if len(hits) else None, len(hits), nframes, min_neighbors, best.ctypes.data,
                                            grouped.ctypes.data, ngrouped.ctypes.data))
        return best[:nframes], grouped[: int(ngrouped[:nframes].sum())], ngrouped[:nframes]

    def detect_raw(self, frames: np.ndarray, flags: int = HT_INPUT_RGBA, cap: int = 1 << 16):
        """ccv.grayscale + ccv.detect_objects(..., min_neighbors = 0) for a batch: (hits, per-frame counts)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim == 3:
            frames = frames[None]
        n, h, w, _ = frames.shape
        if (w, h) != (self.width, self.height) or n > getattr(self, "_max_batch", 0):
            self.set_geometry(w, h, n)
            self._max_batch = n
        self.upload(frames)
        self.detect_enqueue(flags)
        return self.detect_collect(cap)

    def hits_to_rects(self, hits: np.ndarray) -> np.ndarray:
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        out = np.zeros(len(hits), dtype=RECT_DTYPE)
        if len(hits):
            self._check(self._lib.ht_hits_to_rects(self._h, hits.ctypes.data, len(hits), out.ctypes.data))
        return out

    def group_rects(self, rects: np.ndarray, min_neighbors: int = 1) -> np.ndarray:
        rects = np.ascontiguousarray(rects, dtype=RECT_DTYPE)
        out = np.zeros(max(1, len(rects)), dtype=RECT_DTYPE)
        n = C.c_uint32(0)
        self._check(self._lib.ht_group_rects(rects.ctypes.data, len(rects), min_neighbors, out.ctypes.data, C.byref(n)))
        return out[: n.value].copy()

    def best_faces(self, hits: np.ndarray, counts: np.ndarray, min_neighbors: int = 1) -> np.ndarray:
        """facetrackr's choice per frame (facetrackr.js:147-175): the grouped rect with the highest confidence."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        out = np.zeros(len(counts), dtype=RECT_DTYPE)
        self._check(self._lib.ht_best_faces(self._h, hits.ctypes.data if len(hits) else None, counts.ctypes.data, len(counts), min_neighbors,
                                            out.ctypes.data))
        return out

    def detect_objects(self, frames: np.ndarray, min_neighbors: int = 1, flags: int = HT_INPUT_RGBA):
        """Per frame: the list ccv.detect_objects(canvas, cascade, interval, min_neighbors) returns (ccv.js:109-333)."""
        hits, counts = self.detect_raw(frames, flags)
        out, k = [], 0
        for c in counts:
            r = self.hits_to_rects(hits[k : k + int(c)])
            out.append(self.group_rects(r, min_neighbors) if min_neighbors > 0 else r)
            k += int(c)
        return out

    def pyramid_readback(self, frame: int, level: int, slot: int = 0) -> np.ndarray:
        p = self.plane(level, slot)
        out = np.zeros((p.height, p.width), dtype=np.uint8)
        self._check(self._lib.ht_pyramid_readback(self._h, frame, level, slot, out.ctypes.data, out.size))
        return out

    def stage_counts(self) -> np.ndarray:
        n = self.cascade.count + 1
        out = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.ht_stage_counts(self._h, out.ctypes.data, n))
        return out

    def grayscale(self, frames: np.ndarray) -> np.ndarray:
        """ccv.grayscale for a batch of host RGBA frames; returns the gray RGBA copy."""
        out = np.ascontiguousarray(frames, dtype=np.uint8).copy()
        if out.ndim == 3:
            out = out[None]
        n, h, w, _ = out.shape
        self._check(self._lib.ht_grayscale_batch(self._h, out.ctypes.data, n, w, h, w * h * 4))
        return out

    def detect_whitebalance(self, n: int | None = None) -> np.ndarray:
        """getWhitebalance of the frames of the batch COLLECTED last, if it was enqueued with HT_DETECT_WHITEBALANCE (fused into
        its gray pass; the sums are snapshotted by the collect call, so a batch re-enqueued meanwhile does not disturb them)."""
        n = self._collected_n if n is None else n
        out = np.zeros(max(n, 1), dtype=np.float64)[:n]
        self._check(self._lib.ht_detect_whitebalance(self._h, out.ctypes.data, n))
        return out

    def whitebalance(self) -> np.ndarray:
        """headtrackr.getWhitebalance for every bound frame."""
        out = np.zeros(self.nframes, dtype=np.float64)
        self._check(self._lib.ht_whitebalance_batch(self._h, out.ctypes.data, self.nframes))
        return out

    # -- camshift -----------------------------------------------------------------------------------------------
    def camshift_reserve(self, nstreams: int):
        self._check(self._lib.ht_camshift_reserve(self._h, nstreams))

    def camshift_init(self, rects, first: int = 0):
        r = np.zeros(len(rects), dtype=native.CS_RECT_DTYPE)
        for i, (x, y, w, h) in enumerate(rects):
            r[i] = (x, y, w, h)
        self._check(self._lib.ht_camshift_init_batch(self._h, first, len(rects), r.ctypes.data))

    def camshift_track(self, n: int, calc_angles: bool = True, first: int = 0, fetch: bool = True):
        out = np.zeros(n, dtype=native.CS_TRACKOBJ_DTYPE)
        self._check(self._lib.ht_camshift_track_batch(self._h, first, n, int(calc_angles), out.ctypes.data if fetch else None))
        return out

    def camshift_track_collect(self, n: int):
        """Track objects of the OLDEST outstanding camshift_track(n, fetch=False): waits for that call only.  Up to 4 enqueue-only calls
        may be outstanding (results land in a ring of pinned slots), so a streaming host enqueues step i + 1 before it waits for step i,
        and a host with several feeds (contexts) enqueues every feed's track() first and collects afterwards."""
        out = np.zeros(n, dtype=native.CS_TRACKOBJ_DTYPE)
        self._check(self._lib.ht_camshift_track_collect(self._h, n, out.ctypes.data))
        return out

    @staticmethod
    def _pairs(pairs):
        if isinstance(pairs, np.ndarray) and pairs.dtype == native.PAIR_DTYPE:
            return np.ascontiguousarray(pairs)
        p = np.zeros(len(pairs), dtype=native.PAIR_DTYPE)
        for i, (s, f) in enumerate(pairs):
            p[i] = (s, f)
        return p

    def camshift_init_pairs(self, pairs, rects):
        """initTracker of stream pairs[i][0] on BOUND frame pairs[i][1] with rects[i] = (x, y, w, h): any reserved streams in any order,
        frames may repeat (several trackers on one frame)."""
        p = self._pairs(pairs)
        if len(rects) != len(p):
            raise ValueError("camshift_init_pairs: one rect per pair")
        r = np.zeros(len(rects), dtype=native.CS_RECT_DTYPE)
        for i, (x, y, w, h) in enumerate(rects):
            r[i] = (x, y, w, h)
        self._check(self._lib.ht_camshift_init_pairs(self._h, p.ctypes.data, len(p), r.ctypes.data))

    def camshift_init_best(self, pairs, min_confidence: float = -10.0, fallback=None):
        """The detect -> track hand-off on the device (facetrackr.js:97-107): stream pairs[i][0] is initialised on BOUND frame pairs[i][1]
        from that frame's best-face record of the device-grouped batch (detect_best_enqueue: in flight, or collected) when the record has
        neighbors > 0 and confidence > min_confidence, with the floored rect; otherwise with fallback[i] = (x, y, w, h) when fallback is
        given, otherwise the stream keeps every byte.  A record that is not final on the device yet (a frame over the grouping cap before
        the collect) defers the pair.  Enqueue only: no record crosses to the host; camshift_init_best_result tells what was decided."""
        p = self._pairs(pairs)
        fb = None
        if fallback is not None:
            if len(fallback) != len(p):
                raise ValueError("camshift_init_best: one fallback rect per pair")
            fb = np.zeros(len(p), dtype=native.CS_RECT_DTYPE)
            for i, (x, y, w, h) in enumerate(fallback):
                fb[i] = (x, y, w, h)
        self._check(self._lib.ht_camshift_init_best(self._h, p.ctypes.data, len(p), float(min_confidence), fb.ctypes.data if fb is not None else None))

    def camshift_init_best_result(self, n: int):
        """(codes int32 [n], rects CS_RECT_DTYPE [n]) of the LAST camshift_init_best (same n): waits for that call only.  Codes are
        native.HT_CSB_UNTOUCHED / _FACE / _FALLBACK / _DEFERRED; the rect is zeros for untouched and deferred pairs."""
        codes = np.zeros(max(n, 0), dtype=np.int32)
        rects = np.zeros(max(n, 0), dtype=native.CS_RECT_DTYPE)
        self._check(self._lib.ht_camshift_init_best_result(self._h, n, codes.ctypes.data, rects.ctypes.data))
        return codes, rects

    def camshift_init_faces(self, pairs, min_confidence: float = -10.0, associate: bool = False):
        """A tracker per grouped face, decided on the device: the pairs naming one BOUND frame are, in list order, that frame's slots (at
        most native.HT_CSF_MAX_SLOTS), and the frame's grouped list of the device-grouped batch (detect_best_enqueue: in flight, or
        collected) is dealt to them — the eligible faces (neighbors > 0, confidence > min_confidence) by confidence rank, or with
        associate=True so that a tracker whose search window overlaps a face keeps its slot (largest overlap first; the other faces take
        the slots that were never initialised, then the unmatched ones).  Slots without a face keep every byte; a frame that is not final
        on the device yet defers its slots.  Enqueue only; camshift_init_faces_result tells what was decided."""
        p = self._pairs(pairs)
        flags = native.HT_CSF_ASSOCIATE if associate else 0
        self._check(self._lib.ht_camshift_init_faces(self._h, p.ctypes.data, len(p), float(min_confidence), flags))

    def camshift_init_faces_result(self, n: int):
        """records native.CSF_RECORD_DTYPE [n] of the LAST camshift_init_faces (same n), in pair order: code (native.HT_CSB_UNTOUCHED /
        _FACE / _DEFERRED), face (index in the frame's grouped list, or -1), the rect used (zeros without a face) and dropped (eligible
        faces of the frame beyond its slots).  Waits for that call only."""
        out = np.zeros(max(n, 0), dtype=native.CSF_RECORD_DTYPE)
        self._check(self._lib.ht_camshift_init_faces_result(self._h, n, out.ctypes.data))
        return out

    def camshift_track_pairs(self, pairs, calc_angles: bool = True, fetch: bool = True):
        """One track() of stream pairs[i][0] on bound frame pairs[i][1]; track objects in pair order.  The full-frame histogram is computed
        once per distinct frame.  fetch=False: enqueue only, collected with camshift_track_collect(len(pairs))."""
        p = self._pairs(pairs)
        out = np.zeros(len(p), dtype=native.CS_TRACKOBJ_DTYPE)
        self._check(self._lib.ht_camshift_track_pairs(self._h, p.ctypes.data, len(p), int(calc_angles), out.ctypes.data if fetch else None))
        return out

    def camshift_track_sequence(self, dev_ptrs, n: int, calc_angles: bool = True, first: int = 0, frame_stride: int | None = None,
                                fetch: str = "last", keep_all: bool = False):
        """len(dev_ptrs) successive track() calls in one host call; call k reads the n device-resident frames at dev_ptrs[k].
        fetch: "last" -> [n] track objects of the last call, "all" -> [calls, n], "none" -> enqueue only (camshift_sequence_collect
        fetches later: the last call's objects, or every call's if keep_all)."""
        k = len(dev_ptrs)
        ptrs = (C.c_void_p * k)(*[int(p) for p in dev_ptrs])
        stride = frame_stride or self.width * self.height * 4
        if fetch == "none":
            self._check(self._lib.ht_camshift_track_sequence(self._h, first, n, int(calc_angles), ptrs, k, stride, None, int(keep_all)))
            return None
        out = np.zeros((k, n) if fetch == "all" else (n,), dtype=native.CS_TRACKOBJ_DTYPE)
        self._check(self._lib.ht_camshift_track_sequence(self._h, first, n, int(calc_angles), ptrs, k, stride, out.ctypes.data, int(fetch == "all")))
        return out

    def camshift_sequence_collect(self, n: int, ncalls: int, fetch: str = "last"):
        """Results of the last camshift_track_sequence(..., fetch="none"): waits for it ("last" -> [n], "all" -> [ncalls, n])."""
        out = np.zeros((ncalls, n) if fetch == "all" else (n,), dtype=native.CS_TRACKOBJ_DTYPE)
        self._check(self._lib.ht_camshift_sequence_collect(self._h, n, ncalls, int(fetch == "all"), out.ctypes.data))
        return out

    def camshift_stats(self, n: int, first: int = 0, reset: bool = True):
        """(window pixels read by the moment passes, track() calls) per stream since the last reset (SURVEY.md 8d B_track)."""
        px = np.zeros(n, dtype=np.uint64)
        calls = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.ht_camshift_stats(self._h, first, n, px.ctypes.data, calls.ctypes.data, int(reset)))
        return px, calls

    def camshift_debug_hist(self, stream: int, current: bool = True):
        """(model histogram, full-frame histogram of the last track() call) of one stream, 4096 bins each (test hook)."""
        model = np.zeros(4096, dtype=np.uint32)
        cur = np.zeros(4096, dtype=np.uint32)
        self._check(self._lib.ht_camshift_debug_hist(self._h, stream, model.ctypes.data, cur.ctypes.data if current else None))
        return model, cur

    _BP_KINDS = {"rgba8": native.HT_BP_RGBA8, "f64": native.HT_BP_F64}

    def camshift_backproject(self, n: int, first: int = 0, kind: str = "rgba8") -> np.ndarray:
        """Back-projection (camshift.js:172-196, 314-353) of bound frames [0, n) through the models of streams [first, first + n):
        kind "rgba8" -> uint8 [n, H, W, 4], the bytes of getBackProjectionImg().data; "f64" -> float64 [n, H, W], getPdf()[x][y] at
        [y, x].  Computed on the device; changes no tracker state."""
        k = self._BP_KINDS.get(kind, kind)  # an unknown kind reaches the library, which reports it
        shape = (n, self.height, self.width) if k == native.HT_BP_F64 else (n, self.height, self.width, 4)
        out = np.zeros(shape if n > 0 else (0,), dtype=np.float64 if k == native.HT_BP_F64 else np.uint8)
        self._check(self._lib.ht_camshift_backproject(self._h, first, n, int(k), out.ctypes.data, 0))
        return out

    def camshift_backproject_device(self, dev_ptr: int, n: int, first: int = 0, kind: str = "rgba8", stride: int = 0):
        """The same into device memory at dev_ptr (frames `stride` bytes apart, 0 = packed; pointer and stride multiples of the
        element size): enqueued on the context's stream, no copy, no wait."""
        self._check(self._lib.ht_camshift_backproject_device(self._h, first, n, int(self._BP_KINDS.get(kind, kind)), dev_ptr, stride))

    def camshift_backproject_pairs(self, pairs, kind: str = "rgba8") -> np.ndarray:
        """Back-projection of bound frame pairs[i][1] through the model of stream pairs[i][0], in pair order: "rgba8" -> uint8
        [n, H, W, 4], "f64" -> float64 [n, H, W].  Any reserved streams, frames may repeat: the frame's histogram is computed once and
        the trackers of one frame share one pass over its pixels."""
        p = self._pairs(pairs)
        n = len(p)
        k = self._BP_KINDS.get(kind, kind)
        shape = (n, self.height, self.width) if k == native.HT_BP_F64 else (n, self.height, self.width, 4)
        out = np.zeros(shape if n > 0 else (0,), dtype=np.float64 if k == native.HT_BP_F64 else np.uint8)
        self._check(self._lib.ht_camshift_backproject_pairs(self._h, p.ctypes.data, n, int(k), out.ctypes.data, 0))
        return out

    def camshift_backproject_pairs_device(self, dev_ptr: int, pairs, kind: str = "rgba8", stride: int = 0):
        """The same into device memory at dev_ptr (outputs `stride` bytes apart, 0 = packed): enqueued on the context's stream, no copy,
        no wait."""
        p = self._pairs(pairs)
        self._check(self._lib.ht_camshift_backproject_pairs_device(self._h, p.ctypes.data, len(p), int(self._BP_KINDS.get(kind, kind)), dev_ptr, stride))

    # -- face crops: each tracker's box cut from its feed ----------------------------------------------------------
    @staticmethod
    def _crop_params(width: int, height: int, margin: float, square: bool):
        return native.CROP_PARAMS(int(width), int(height), int(round(float(margin) * 256)), native.HT_CROP_SQUARE if square else 0)

    @staticmethod
    def _face_extra(name: str, fmt, max_factor):
        """what a form has between the params and the output: the tensor forms' format; the filtered forms' max_factor and format | NULL"""
        if name.endswith("_tensor_device"):
            return (C.byref(PatchFormat.of(fmt).struct()),)
        if name.endswith("_filtered_device"):
            fp = Context._filter_format(fmt)[1]
            return (int(max_factor), fp)
        return ()

    def _face_pairs(self, name: str, dev_ptr: int, pairs, size, stride: int, fmt=None, max_factor=None):
        """the pairs form of every face-patch call: ht_<name>(ctx, pairs, n, params, [max_factor,] [format,] out, stride); size = (width, height,
        margin, square)"""
        p = self._pairs(pairs)
        extra = self._face_extra(name, fmt, max_factor)
        prm = (self._align_params if "_align_" in name else self._crop_params)(*size)
        self._check(getattr(self._lib, "ht_" + name)(self._h, p.ctypes.data, len(p), C.byref(prm), *extra, dev_ptr, stride))

    def _face_sources(self, name: str, dev_ptr: int, streams, entries, size, stride: int, fmt=None, max_factor=None):
        """the sources form: ht_<name>(ctx, streams, entries, n, params, [max_factor,] [format,] out, stride)"""
        if len(streams) != len(entries):
            raise ValueError(name + ": one stream per entry")
        st = np.ascontiguousarray(np.asarray(streams, dtype=np.int32).reshape(-1))
        extra = self._face_extra(name, fmt, max_factor)
        prm = (self._align_params if "_align_" in name else self._crop_params)(*size)
        self._check(getattr(self._lib, "ht_" + name)(self._h, st.ctypes.data if len(st) else None, self._draw_sources(entries), len(entries), C.byref(prm), *extra,
                                                     dev_ptr, stride))

    def camshift_crop_pairs_device(self, dev_ptr: int, pairs, width: int, height: int, margin: float = 1.0, square: bool = False, stride: int = 0):
        """Patch i = the box of stream pairs[i][0]'s track object cut from BOUND frame pairs[i][1] and scaled to width x height RGBA by the
        declared resampler, into device memory at dev_ptr (patches `stride` bytes apart, 0 = packed).  margin widens the box around its
        centre (1.0 = as tracked; it becomes 1/256 steps, 0.25 .. 4); square grows the shorter side first.  A lost or never tracked stream
        gives zeros.  Enqueued behind the outstanding track steps: no copy, no wait.  Streams may repeat."""
        self._face_pairs("camshift_crop_pairs_device", dev_ptr, pairs, (width, height, margin, square), stride)

    def camshift_crop_sources_device(self, dev_ptr: int, streams, entries, width: int, height: int, margin: float = 1.0, square: bool = False, stride: int = 0):
        """The same from the feeds' own frames: entries[i] as in draw_list, its "rect" the rect that was drawn onto the canvas stream
        streams[i] tracks on; the box is mapped back through it and may reach beyond it, up to the source's edges."""
        self._face_sources("camshift_crop_sources_device", dev_ptr, streams, entries, (width, height, margin, square), stride)

    def camshift_crop_result(self, n: int) -> np.ndarray:
        """CROP_RECORD_DTYPE [n] of the LAST crop call (same n): code (native.HT_CROP_EMPTY / _FACE), stream, the rect in source pixels and
        the two ratios.  Waits for that call only."""
        out = np.zeros(max(n, 0), dtype=native.CROP_RECORD_DTYPE)
        self._check(self._lib.ht_camshift_crop_result(self._h, n, out.ctypes.data))
        return out

    def camshift_crop_records_ptr(self):
        """(device pointer, n) of the last crop call's records, valid until the next crop call"""
        ptr, n = C.c_void_p(), C.c_int32()
        self._check(self._lib.ht_camshift_crop_records_device(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    # -- angle-aligned face crops: each tracker's rotated box, upright ---------------------------------------------
    @staticmethod
    def _align_params(width: int, height: int, margin: float, square: bool):
        return native.ALIGN_PARAMS(int(width), int(height), int(round(float(margin) * 256)), native.HT_ALIGN_SQUARE if square else 0)

    def camshift_align_pairs_device(self, dev_ptr: int, pairs, width: int, height: int, margin: float = 1.0, square: bool = False, stride: int = 0):
        """Patch i = the ROTATED box of stream pairs[i][0]'s track object (width and height along the blob's axes, turned by its angle as
        the overlay draws it) sampled upright from BOUND frame pairs[i][1] into width x height RGBA at dev_ptr (patches `stride` bytes
        apart, 0 = packed).  margin and square as for camshift_crop_pairs_device; square makes both sides the longer one.  Pixels whose
        sample centre lies outside the frame are zeros, and so is the patch of a lost or never tracked stream.  Enqueued behind the
        outstanding track steps: no copy, no wait.  Streams may repeat."""
        self._face_pairs("camshift_align_pairs_device", dev_ptr, pairs, (width, height, margin, square), stride)

    def camshift_align_sources_device(self, dev_ptr: int, streams, entries, width: int, height: int, margin: float = 1.0, square: bool = False, stride: int = 0):
        """The same from the feeds' own frames: entries[i] as in draw_list, its "rect" the rect that was drawn onto the canvas stream
        streams[i] tracks on; the box is mapped back through it (an affine image) and may reach beyond it, up to the source's edges."""
        self._face_sources("camshift_align_sources_device", dev_ptr, streams, entries, (width, height, margin, square), stride)

    def camshift_align_result(self, n: int) -> np.ndarray:
        """ALIGN_RECORD_DTYPE [n] of the LAST align call (same n): code (native.HT_ALIGN_EMPTY / _FACE), stream, the angle in 1/4096 turn,
        the centre and the patch's two vectors in Q16 source pixels.  Waits for that call only."""
        out = np.zeros(max(n, 0), dtype=native.ALIGN_RECORD_DTYPE)
        self._check(self._lib.ht_camshift_align_result(self._h, n, out.ctypes.data))
        return out

    def camshift_align_records_ptr(self):
        """(device pointer, n) of the last align call's records, valid until the next align call"""
        ptr, n = C.c_void_p(), C.c_int32()
        self._check(self._lib.ht_camshift_align_records_device(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    # -- model-input tensors: the crop and align calls with a float output stage -----------------------------------
    def camshift_crop_pairs_tensor_device(self, dev_ptr: int, pairs, width: int, height: int, fmt, margin: float = 1.0, square: bool = False, stride: int = 0):
        """camshift_crop_pairs_device with fmt (a PatchFormat or a dict of its arguments) as the output: patch i becomes the model's input
        tensor — fmt.nchannels * width * height elements of fmt.dtype, `stride` bytes apart (0 = a patch's bytes rounded up to 4) —, every
        element fl32(fl32(byte * scale[c]) + bias[c]) rounded to the dtype, in the same single launch.  A lost or never tracked stream gives
        bias[c] everywhere (read camshift_crop_result's code).  This IS the context's last crop call."""
        self._face_pairs("camshift_crop_pairs_tensor_device", dev_ptr, pairs, (width, height, margin, square), stride, fmt)

    def camshift_crop_sources_tensor_device(self, dev_ptr: int, streams, entries, width: int, height: int, fmt, margin: float = 1.0, square: bool = False, stride: int = 0):
        """camshift_crop_sources_device with fmt as the output (see camshift_crop_pairs_tensor_device)"""
        self._face_sources("camshift_crop_sources_tensor_device", dev_ptr, streams, entries, (width, height, margin, square), stride, fmt)

    def camshift_align_pairs_tensor_device(self, dev_ptr: int, pairs, width: int, height: int, fmt, margin: float = 1.0, square: bool = False, stride: int = 0):
        """camshift_align_pairs_device with fmt as the output; a pixel whose sample centre lies outside the source is bias[c], as every
        element of an empty entry is.  This IS the context's last align call."""
        self._face_pairs("camshift_align_pairs_tensor_device", dev_ptr, pairs, (width, height, margin, square), stride, fmt)

    def camshift_align_sources_tensor_device(self, dev_ptr: int, streams, entries, width: int, height: int, fmt, margin: float = 1.0, square: bool = False, stride: int = 0):
        """camshift_align_sources_device with fmt as the output (see camshift_align_pairs_tensor_device)"""
        self._face_sources("camshift_align_sources_tensor_device", dev_ptr, streams, entries, (width, height, margin, square), stride, fmt)

    # -- prefiltered face crops: each patch pixel the mean of a block of the unfiltered rule's samples ------------------------
    @staticmethod
    def _filter_format(fmt):
        """(the struct to keep alive, the pointer argument): None is RGBA8"""
        if fmt is None:
            return None, None
        f = PatchFormat.of(fmt).struct()
        return f, C.byref(f)

    def camshift_crop_pairs_filtered_device(self, dev_ptr: int, pairs, width: int, height: int, max_factor: int = 8, fmt=None, margin: float = 1.0, square: bool = False,
                                            stride: int = 0):
        """camshift_crop_pairs_device for strong downscales: every patch pixel is the rounded mean of an Nx x Ny block of the unfiltered
        rule's samples (the patch that call gives at Nx * width x Ny * height), Nx = min(max_factor, max(1, ceil(w / width))) and Ny
        likewise, chosen per entry on the device from the tracked box; max_factor 1..8.  With factors 1, 1 the patch is byte for byte the
        unfiltered call's.  fmt None: RGBA8; otherwise a PatchFormat (or a dict of its arguments) and the output is the model-input tensor
        of the filtered patch, as camshift_crop_pairs_tensor_device lays it out.  ONE enqueue-only launch; this IS the context's last crop
        call (camshift_crop_result gives the unfiltered call's records; crop_filter_factors turns them into the factors)."""
        self._face_pairs("camshift_crop_pairs_filtered_device", dev_ptr, pairs, (width, height, margin, square), stride, fmt, max_factor)

    def camshift_crop_sources_filtered_device(self, dev_ptr: int, streams, entries, width: int, height: int, max_factor: int = 8, fmt=None, margin: float = 1.0,
                                              square: bool = False, stride: int = 0):
        """camshift_crop_sources_device with the block-mean prefilter (see camshift_crop_pairs_filtered_device)"""
        self._face_sources("camshift_crop_sources_filtered_device", dev_ptr, streams, entries, (width, height, margin, square), stride, fmt, max_factor)

    def camshift_align_pairs_filtered_device(self, dev_ptr: int, pairs, width: int, height: int, max_factor: int = 8, fmt=None, margin: float = 1.0, square: bool = False,
                                             stride: int = 0):
        """camshift_align_pairs_device with the block-mean prefilter: Nx = min(max_factor, max(1, ceil((|ux| + |uy|) / (width * 65536)))),
        Ny the same with (vx, vy) and height, from the entry's align record; the patch's edge fades where fine samples fall outside the
        frame.  This IS the context's last align call (align_filter_factors turns its records into the factors)."""
        self._face_pairs("camshift_align_pairs_filtered_device", dev_ptr, pairs, (width, height, margin, square), stride, fmt, max_factor)

    def camshift_align_sources_filtered_device(self, dev_ptr: int, streams, entries, width: int, height: int, max_factor: int = 8, fmt=None, margin: float = 1.0,
                                               square: bool = False, stride: int = 0):
        """camshift_align_sources_device with the block-mean prefilter (see camshift_align_pairs_filtered_device)"""
        self._face_sources("camshift_align_sources_filtered_device", dev_ptr, streams, entries, (width, height, margin, square), stride, fmt, max_factor)

    # -- measurement --------------------------------------------------------------------------------------------
    def profile(self, on: bool = True):
        self._check(self._lib.ht_profile(self._h, int(on)))

    def kernel_times(self, reset: bool = True) -> dict:
        # the entry count first (no buffer, nothing reset), then a buffer that holds them all: with a fixed 32 entries the pseudo-timers
        # the library appends behind the real ones (cs_fused_launches_*) fell off the end once many timers existed
        n = C.c_int32(0)
        self._check(self._lib.ht_kernel_times(self._h, None, C.byref(n), 0))
        cap = max(int(n.value), 1)
        buf = np.zeros(cap, dtype=native.KERNEL_TIME_DTYPE)
        n = C.c_int32(cap)
        self._check(self._lib.ht_kernel_times(self._h, buf.ctypes.data, C.byref(n), int(reset)))
        if n.value > cap:
            raise RuntimeError(f"ht_kernel_times: {n.value} entries for a buffer of {cap}")
        return {b["name"].decode(): dict(ms=float(b["ms"]), launches=int(b["launches"])) for b in buf[: n.value]}

    @property
    def graph_launches(self) -> int:
        """detect_enqueue calls that were served by replaying a captured hipGraph"""
        return int(self._lib.ht_graph_launches(self._h))

    def synchronize(self):
        self._check(self._lib.ht_synchronize(self._h))

    @property
    def stream(self) -> int:
        return int(self._lib.ht_stream(self._h) or 0)


def _filter_factors(fn, records, dtype, width: int, height: int, max_factor: int) -> np.ndarray:
    rec = np.ascontiguousarray(records, dtype=dtype).reshape(-1)
    out = np.zeros((len(rec), 2), dtype=np.int32)
    nx, ny = C.c_int32(), C.c_int32()
    for i in range(len(rec)):
        st = fn(rec[i:i + 1].ctypes.data, int(width), int(height), int(max_factor), C.byref(nx), C.byref(ny))
        if st != 0:
            raise HtError(st, "filter factors: out_width / out_height must be 1..1024 and max_factor 1..8")
        out[i] = nx.value, ny.value
    return out


def crop_filter_factors(records, width: int, height: int, max_factor: int = 8) -> np.ndarray:
    """int32 [n, 2]: the (Nx, Ny) a filtered crop call of (width, height, max_factor) takes for each CROP_RECORD_DTYPE record (what
    camshift_crop_result returns); 0, 0 for an empty one.  The library's own rule (ht_camshift_crop_filter_factors): needs no device."""
    return _filter_factors(native.lib().ht_camshift_crop_filter_factors, records, native.CROP_RECORD_DTYPE, width, height, max_factor)


def align_filter_factors(records, width: int, height: int, max_factor: int = 8) -> np.ndarray:
    """the same for ALIGN_RECORD_DTYPE records and the filtered align calls (ht_camshift_align_filter_factors)"""
    return _filter_factors(native.lib().ht_camshift_align_filter_factors, records, native.ALIGN_RECORD_DTYPE, width, height, max_factor)


def draw_filter_factors(entries_or_sizes, width: int, height: int, max_factor: int = 8) -> np.ndarray:
    """int32 [n, 2]: the (Nx, Ny) Context.draw_list(entries, prefilter=max_factor) takes for each entry on a width x height canvas.  An
    item is a draw_list entry dict (its "rect" counts, else its whole "width" x "height") or a (source width, source height) pair.  The
    library's own rule (ht_draw_filter_factors): needs no device."""
    fn = native.lib().ht_draw_filter_factors
    out = np.zeros((len(entries_or_sizes), 2), dtype=np.int32)
    nx, ny = C.c_int32(), C.c_int32()
    for i, e in enumerate(entries_or_sizes):
        if isinstance(e, dict):
            sw, sh = (e["rect"][2], e["rect"][3]) if e.get("rect") is not None else (e["width"], e["height"])
        else:
            sw, sh = e
        st = fn(int(sw), int(sh), int(width), int(height), int(max_factor), C.byref(nx), C.byref(ny))
        if st != 0:
            raise HtError(st, f"draw filter factors: entry {i}: source width / height must be 1..16384, the canvas positive and max_factor 1..8")
        out[i] = nx.value, ny.value
    return out


# -- rotated and mirrored feeds: the orientation of a draw_list entry, of draw_frames_yuv* and of the face calls' entries -------------------
# k = 0..7: k & 3 quarter turns CLOCKWISE bring the stored frame upright, k >> 2 mirrors it horizontally AFTER the turn
# (numpy: np.rot90(stored, -(k & 3)), then np.fliplr if k >> 2).  It travels in bits 8..10 of the format number (HT_ORIENT).
_EXIF_ORIENTATION = {1: 0, 2: 4, 3: 2, 4: 6, 5: 5, 6: 1, 7: 7, 8: 3}


def orientation_bits(orientation) -> int:
    """HT_ORIENT(k): the bits an orientation adds to a format number; anything but an integer 0..7 raises"""
    k = int(orientation)
    if k != orientation or not 0 <= k <= 7:
        raise ValueError("orientation is an integer 0..7 (orientation_from_exif / orientation_from_rotation)")
    return k << 8


def orientation_from_exif(n: int) -> int:
    """the orientation of an image whose EXIF Orientation tag is n (1..8)"""
    if n not in _EXIF_ORIENTATION:
        raise ValueError("an EXIF orientation is 1..8")
    return _EXIF_ORIENTATION[n]


def orientation_from_rotation(degrees: int, mirror: bool = False) -> int:
    """the orientation of a feed that has to be turned `degrees` clockwise for display (a container's `rotate` / display matrix, WebRTC's
    CVO; any multiple of 90, negative ones included) and, with mirror, flipped horizontally after the turn (a selfie camera)"""
    if int(degrees) != degrees or int(degrees) % 90:
        raise ValueError("a rotation is a multiple of 90 degrees")
    return (int(degrees) // 90) % 4 | (4 if mirror else 0)


def device_count() -> int:
    return int(native.lib().ht_device_count())


def allgather_best_faces(ctxs, best_per_rank) -> np.ndarray:
    """Single-process multi-GPU exchange (ht_allgather_best_faces): ctxs[i] lives on GPU i and produced best_per_rank[i]
    (ht_best_faces output, equal lengths).  Returns the gathered [nranks, frames_per_rank] table after every rank's copy was
    checked to be identical."""
    n = len(ctxs)
    per = len(best_per_rank[0])
    arrs = [np.ascontiguousarray(b, dtype=RECT_DTYPE) for b in best_per_rank]
    assert all(len(a) == per for a in arrs)
    cp = (C.c_void_p * n)(*[c._h.value for c in ctxs])
    bp = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    out = np.zeros((n, per), dtype=RECT_DTYPE)
    st = native.lib().ht_allgather_best_faces(cp, n, bp, per, out.ctypes.data)
    if st != 0:
        raise HtError(st, native.lib().ht_last_error(ctxs[0]._h).decode())
    return out

"""Every refusal of the six canvas-draw entry points as a table: (call, case) -> the malformed call.  replay() makes each call on a real
context and returns {"canvas": [W, H], "cases": {"call/case": [status, ht_last_error text]}}; tests/golden/draw_call_refusals.json is
that table as the library answered it BEFORE the calls' host path was written once (csrc/ht_draw_calls.hip), and tests/test_gpu_ingest.py
replays it on the built library and compares for equality.  Every case is an argument error: nothing is enqueued, no kernel runs.  A case
named "a+b" holds two faults that are adjacent in the call's check order; the answer is the earlier check's, which is what pins the order.
(The missing-module refusal of an oriented list carries a path and has a test of its own: tests/test_gpu_orient.py.)"""
import ctypes as C

import numpy as np

from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray

NV12, I420, YUYV, RGBA = native.HT_YUV_NV12, native.HT_YUV_I420, native.HT_YUV_YUYV, native.HT_DRAW_RGBA
MAX_BATCH = 2
CANVASES = [(8, 8), (40, 30)]  # the first geometry ht_set_geometry accepts; sources are canvas-sized


def orient(k):
    return k << 8


def build(W, H, src, dst, hostbuf):
    """the table: [(key, thunk(lib, handle) -> status)] for a W x H canvas, device buffers src / dst (8 KiB each) and a host buffer"""
    fb, row = W * H * 4, W * 4
    cw, ch = (W + 1) // 2, (H + 1) // 2
    yf = W * H  # a Y plane; frames of every plane are spaced by it

    def rect_of(rect):
        return C.byref(native.CS_RECT(*rect)) if rect is not None else None

    def dev(ptr=src, n=2, w=W, h=H, pitch=0, stride=0, rect=None, to=dst, dstride=0):
        return lambda L, c: L.ht_draw_frames_device(c, ptr, n, w, h, pitch, stride, rect_of(rect), to, dstride)

    def host(ptr=hostbuf, n=2, w=W, h=H, stride=0, rect=None):
        return lambda L, c: L.ht_draw_frames(c, ptr, n, w, h, stride, rect_of(rect))

    def yuvd(desc=True, y=src, u=src + 2048, v=src + 4096, yp=0, cp=0, stride=yf, w=W, h=H, fmt=NV12, matrix=0, n=2, rect=None, to=dst, dstride=0):
        d = native.YUV_FRAMES(y, u, v, yp, cp, stride, w, h, fmt, matrix)
        return lambda L, c: L.ht_draw_frames_yuv_device(c, C.byref(d) if desc else None, n, rect_of(rect), to, dstride)

    def yuvh(ptr=hostbuf, n=2, w=W, h=H, fmt=NV12, matrix=0, stride=0, rect=None):
        return lambda L, c: L.ht_draw_frames_yuv(c, ptr, n, w, h, fmt, matrix, stride, rect_of(rect))

    def E(p0=src, p1=None, p2=None, pitch0=0, pitch1=0, w=W, h=H, fmt=RGBA, matrix=0, rect=(0, 0, 0, 0)):
        return native.DRAW_SOURCE(p0, p1, p2, pitch0, pitch1, w, h, fmt, matrix, native.CS_RECT(*rect))

    def lists(entries=None, n=None, null=False, to=dst, dstride=0, factor=None):
        entries = [E(), E(src + fb)] if entries is None else entries
        arr = (native.DRAW_SOURCE * len(entries))(*entries)
        n = len(entries) if n is None else n
        if factor is None:
            return lambda L, c: L.ht_draw_list_device(c, None if null else arr, n, to, dstride)
        return lambda L, c: L.ht_draw_list_filtered_device(c, None if null else arr, n, factor, to, dstride)

    t = []

    def add(call, case, thunk):
        t.append((f"{call}/{case}", thunk))

    # ---- ht_draw_frames_device: count, size, pitch, stride, rect, pointers (source and destination alignment in ONE check), then the form
    f = "ht_draw_frames_device"
    add(f, "n = 0", dev(n=0))
    add(f, "n < 0", dev(n=-1))
    add(f, "zero width", dev(w=0))
    add(f, "height above 16384", dev(h=16385))
    add(f, "pitch not a multiple of 4", dev(pitch=row + 2))
    add(f, "pitch smaller than a row", dev(pitch=row - 4))
    add(f, "source stride not a multiple of 4", dev(stride=fb + 2))
    add(f, "source stride smaller than a frame", dev(stride=fb - 4))
    add(f, "rect beyond the right edge", dev(rect=(1, 0, W, H)))
    add(f, "rect with a negative origin", dev(rect=(-1, 0, 2, 2)))
    add(f, "empty rect", dev(rect=(0, 0, 0, 5)))
    add(f, "NULL source", dev(ptr=None))
    add(f, "misaligned source", dev(ptr=src + 2))
    add(f, "misaligned destination", dev(to=dst + 1))
    add(f, "bind form: n above the batch capacity", dev(n=MAX_BATCH + 1, to=None))
    add(f, "destination stride smaller than a frame", dev(dstride=fb - 4))
    add(f, "destination stride not a multiple of 4", dev(dstride=fb + 2))
    add(f, "destination inside the source", dev(to=src + row))
    add(f, "source inside the destination", dev(ptr=dst + fb, to=dst, dstride=2 * fb))
    add(f, "source meets the last written byte", dev(ptr=dst + 2 * fb - 4))
    add(f, "count+size", dev(n=0, w=0))
    add(f, "size+pitch", dev(w=0, pitch=2))
    add(f, "pitch+stride", dev(pitch=row + 2, stride=fb + 2))
    add(f, "stride+rect", dev(stride=fb - 4, rect=(1, 0, W, H)))
    add(f, "rect+NULL source", dev(rect=(1, 0, W, H), ptr=None))
    add(f, "misaligned destination+destination stride", dev(to=dst + 1, dstride=fb + 2))
    add(f, "NULL source+bind form capacity", dev(ptr=None, n=MAX_BATCH + 1, to=None))
    add(f, "bind form capacity+destination stride (not looked at)", dev(n=MAX_BATCH + 1, to=None, dstride=fb + 2))
    add(f, "destination stride+overlap", dev(to=src + row, dstride=fb + 2))

    # ---- ht_draw_frames: the caller's stride FIRST (in front of the context's state), the shared checks, NULL, capacity
    f = "ht_draw_frames"
    add(f, "source stride smaller than a frame", host(stride=fb - 1))
    add(f, "n = 0", host(n=0))
    add(f, "negative height", host(h=-3))
    add(f, "rect beyond the bottom edge", host(rect=(0, 1, W, H)))
    add(f, "NULL source", host(ptr=None))
    add(f, "n above the batch capacity", host(n=MAX_BATCH + 1))
    add(f, "stride+count", host(stride=fb - 1, n=0))
    add(f, "count+size", host(n=0, w=0))
    add(f, "size+rect", host(w=0, rect=(0, 1, W, H)))
    add(f, "rect+NULL source", host(rect=(0, 1, W, H), ptr=None))
    add(f, "NULL source+capacity", host(ptr=None, n=MAX_BATCH + 1))

    # ---- ht_draw_frames_yuv_device: description, ht_yuv_plan's statuses in its order, rect, planes, destination alignment, then the form
    f = "ht_draw_frames_yuv_device"
    add(f, "NULL description", yuvd(desc=False))
    add(f, "n = 0", yuvd(n=0))
    add(f, "zero width", yuvd(w=0))
    add(f, "no such format", yuvd(fmt=2))
    add(f, "RGBA is no format of this call", yuvd(fmt=RGBA))
    add(f, "a format bit above the orientation", yuvd(fmt=NV12 | 0x800))
    add(f, "no such matrix", yuvd(matrix=4))
    add(f, "Y pitch smaller than a row", yuvd(yp=W - 1))
    add(f, "YUYV pitch not a multiple of 4", yuvd(fmt=YUYV, yp=4 * cw + 2, stride=4 * cw * H + 2 * H))
    add(f, "NV12 chroma pitch odd", yuvd(cp=2 * cw + 1))
    add(f, "I420 chroma pitch smaller than a row", yuvd(fmt=I420, cp=cw - 1))
    add(f, "frame stride missing for n = 2", yuvd(stride=0))
    add(f, "frame stride smaller than a Y plane", yuvd(stride=yf - 2))
    add(f, "NV12 frame stride odd", yuvd(stride=yf + 1))
    add(f, "YUYV frame stride not a multiple of 4", yuvd(fmt=YUYV, stride=4 * cw * H + 2))
    add(f, "rect beyond the right edge", yuvd(rect=(1, 0, W, H)))
    add(f, "empty rect", yuvd(rect=(0, 0, 0, 5)))
    add(f, "oriented: rect outside the oriented frame", yuvd(fmt=NV12 | orient(1), w=W, h=H - 2, stride=W * (H - 2), rect=(0, 0, W, H - 2)))
    add(f, "NULL Y plane", yuvd(y=None))
    add(f, "NULL NV12 chroma plane", yuvd(u=None))
    add(f, "NULL I420 V plane", yuvd(fmt=I420, v=None))
    add(f, "NULL YUYV plane", yuvd(fmt=YUYV, y=None, stride=4 * cw * H))
    add(f, "NV12 chroma at an odd address", yuvd(u=src + 2049))
    add(f, "misaligned YUYV plane", yuvd(fmt=YUYV, y=src + 2, stride=4 * cw * H))
    add(f, "misaligned destination", yuvd(to=dst + 2))
    add(f, "bind form: n above the batch capacity", yuvd(n=MAX_BATCH + 1, to=None))
    add(f, "destination stride smaller than a frame", yuvd(dstride=fb - 4))
    add(f, "destination stride not a multiple of 4", yuvd(dstride=fb + 2))
    add(f, "Y plane inside the destination", yuvd(y=dst + 4))
    add(f, "NV12 chroma plane inside the destination", yuvd(u=dst + 2 * fb - 2))
    add(f, "I420 V plane inside the destination", yuvd(fmt=I420, v=dst + fb))
    add(f, "count+size", yuvd(n=0, w=0))
    add(f, "size+format", yuvd(w=0, fmt=2))
    add(f, "format+matrix", yuvd(fmt=2, matrix=4))
    add(f, "matrix+Y pitch", yuvd(matrix=4, yp=W - 1))
    add(f, "Y pitch+chroma pitch", yuvd(yp=W - 1, cp=2 * cw + 1))
    add(f, "chroma pitch+frame stride", yuvd(cp=2 * cw + 1, stride=0))
    add(f, "frame stride+rect", yuvd(stride=0, rect=(1, 0, W, H)))
    add(f, "rect+NULL plane", yuvd(rect=(1, 0, W, H), y=None))
    add(f, "NULL plane+odd chroma", yuvd(y=None, u=src + 2049))
    add(f, "odd chroma+misaligned destination", yuvd(u=src + 2049, to=dst + 2))
    add(f, "misaligned YUYV plane+misaligned destination", yuvd(fmt=YUYV, y=src + 2, stride=4 * cw * H, to=dst + 2))
    add(f, "misaligned destination+destination stride", yuvd(to=dst + 2, dstride=fb + 2))
    add(f, "bind form capacity+destination stride (not looked at)", yuvd(n=MAX_BATCH + 1, to=None, dstride=fb + 2))
    add(f, "destination stride+overlap", yuvd(y=dst + 4, dstride=fb + 2))

    # ---- ht_draw_frames_yuv: the shared checks, the caller's stride, NULL, capacity
    f = "ht_draw_frames_yuv"
    add(f, "n = 0", yuvh(n=0))
    add(f, "zero height", yuvh(h=0))
    add(f, "no such format", yuvh(fmt=3))
    add(f, "no such matrix", yuvh(matrix=-1))
    add(f, "rect beyond the bottom edge", yuvh(rect=(0, 1, W, H)))
    add(f, "oriented: rect outside the oriented frame", yuvh(fmt=I420 | orient(3), h=H - 2, rect=(0, 0, W, H - 2)))
    add(f, "source stride smaller than a frame", yuvh(stride=yf))
    add(f, "NULL source", yuvh(ptr=None))
    add(f, "n above the batch capacity", yuvh(n=MAX_BATCH + 1))
    add(f, "matrix+rect", yuvh(matrix=-1, rect=(0, 1, W, H)))
    add(f, "rect+stride", yuvh(rect=(0, 1, W, H), stride=yf))
    add(f, "stride+NULL source", yuvh(stride=yf, ptr=None))
    add(f, "NULL source+capacity", yuvh(ptr=None, n=MAX_BATCH + 1))

    # ---- the two list calls: count, (max_factor,) destination alignment, stride, the entries, then the form
    nv12 = dict(p1=src + 2048, fmt=NV12)
    i420 = dict(p1=src + 2048, p2=src + 4096, fmt=I420)
    entry_faults = [
        ("no such format", [E(), E(fmt=2)]),
        ("a format bit above the orientation", [E(fmt=RGBA | 0x800)]),
        ("zero width", [E(), E(w=0)]),
        ("YUV height above 16384", [E(h=16385, **nv12)]),
        ("no such matrix", [E(), E(matrix=4, **nv12)]),
        ("RGBA pitch not a multiple of 4", [E(pitch0=row + 2)]),
        ("Y pitch smaller than a row", [E(), E(pitch0=W - 1, **i420)]),
        ("NV12 chroma pitch odd", [E(pitch1=2 * cw + 1, **nv12)]),
        ("NULL RGBA plane", [E(), E(p0=None)]),
        ("NULL I420 V plane", [E(p1=src + 2048, fmt=I420)]),
        ("misaligned RGBA plane", [E(p0=src + 2)]),
        ("misaligned YUYV plane", [E(), E(p0=src + 2, fmt=YUYV)]),
        ("NV12 chroma at an odd address", [E(p1=src + 2049, fmt=NV12)]),
        ("rect beyond the right edge", [E(), E(), E(rect=(1, 0, W, H))]),
        ("oriented: rect outside the oriented frame", [E(), E(h=H - 2, fmt=RGBA | orient(1), rect=(0, 0, W, H - 2))]),
        ("oriented: no such format", [E(fmt=2 | orient(4))]),
    ]
    for f, factor in (("ht_draw_list_device", None), ("ht_draw_list_filtered_device", 2)):
        kw = dict(factor=factor)
        add(f, "NULL list", lists(null=True, **kw))
        add(f, "n = 0", lists(n=0, **kw))
        add(f, "n above 65535", lists(n=65536, **kw))
        if factor is not None:
            add(f, "max_factor 0", lists(factor=0))
            add(f, "max_factor 9", lists(factor=9))
            add(f, "count+max_factor", lists(n=0, factor=0))
            add(f, "max_factor+misaligned destination", lists(factor=9, to=dst + 2))
        add(f, "misaligned destination", lists(to=dst + 2, **kw))
        add(f, "destination stride smaller than a frame", lists(dstride=fb - 4, **kw))
        add(f, "destination stride not a multiple of 4", lists(dstride=fb + 2, **kw))
        for what, entries in entry_faults:
            add(f, "entry: " + what, lists(entries, **kw))
        add(f, "bind form: n above the batch capacity", lists([E()] * (MAX_BATCH + 1), to=None, **kw))
        add(f, "RGBA entry inside the destination", lists([E(), E(dst + 2 * fb - 4)], **kw))
        add(f, "NV12 chroma plane inside the destination", lists([E(p1=dst + 4, fmt=NV12)], **kw))
        add(f, "I420 V plane inside the destination", lists([E(), E(), E(p1=src + 2048, p2=dst, fmt=I420)], **kw))
        add(f, "count+misaligned destination", lists(n=0, to=dst + 2, **kw))
        add(f, "misaligned destination+destination stride", lists(to=dst + 2, dstride=fb + 2, **kw))
        add(f, "destination stride+entry", lists([E(w=0)], dstride=fb + 2, **kw))
        add(f, "bind form: destination stride is not looked at+entry", lists([E(w=0)], to=None, dstride=fb + 2, **kw))
        add(f, "entry+bind form capacity", lists([E()] * MAX_BATCH + [E(w=0)], to=None, **kw))
        add(f, "entry+overlap", lists([E(dst), E(w=0)], **kw))
    return t


def replay():
    """every case on a real device -> {"canvas": [W, H], "cases": {key: [status, text]}}; "no geometry" cases run on a fresh context"""
    fresh, c = Context(), Context()
    src = DeviceArray(np.zeros(8192, dtype=np.uint8))
    dst = DeviceArray(np.zeros(8192, dtype=np.uint8))
    hostbuf = np.zeros(8192, dtype=np.uint8)
    try:
        for W, H in CANVASES:
            try:
                c.set_geometry(W, H, MAX_BATCH)
                break
            except HtError:
                continue
        else:
            raise RuntimeError("no canvas of CANVASES is a geometry")
        table = build(W, H, src.ptr, dst.ptr, hostbuf.ctypes.data)
        L = c._lib
        out = {}
        ok = dict(table)
        # ht_set_geometry not yet called: a well-formed call of each entry point, and the faults that sit next to that check
        first = {"ht_draw_frames_device": ["n = 0"], "ht_draw_frames": ["n = 0", "source stride smaller than a frame"], "ht_draw_frames_yuv_device": ["n = 0", "NULL description"],
                 "ht_draw_frames_yuv": ["n = 0"], "ht_draw_list_device": ["NULL list"], "ht_draw_list_filtered_device": ["NULL list", "max_factor 0"]}
        calls = {"ht_draw_frames_device": lambda L, h: L.ht_draw_frames_device(h, src.ptr, 2, W, H, 0, 0, None, dst.ptr, 0),
                 "ht_draw_frames": lambda L, h: L.ht_draw_frames(h, hostbuf.ctypes.data, 2, W, H, 0, None),
                 "ht_draw_frames_yuv_device": lambda L, h: L.ht_draw_frames_yuv_device(h, C.byref(native.YUV_FRAMES(src.ptr, src.ptr + 2048, None, 0, 0, W * H, W, H, NV12, 0)), 2, None, dst.ptr, 0),
                 "ht_draw_frames_yuv": lambda L, h: L.ht_draw_frames_yuv(h, hostbuf.ctypes.data, 2, W, H, NV12, 0, 0, None),
                 "ht_draw_list_device": lambda L, h: L.ht_draw_list_device(h, (native.DRAW_SOURCE * 1)(native.DRAW_SOURCE(src.ptr, None, None, 0, 0, W, H, RGBA, 0, native.CS_RECT(0, 0, 0, 0))), 1, dst.ptr, 0),
                 "ht_draw_list_filtered_device": lambda L, h: L.ht_draw_list_filtered_device(h, (native.DRAW_SOURCE * 1)(native.DRAW_SOURCE(src.ptr, None, None, 0, 0, W, H, RGBA, 0, native.CS_RECT(0, 0, 0, 0))), 1, 2, dst.ptr, 0)}
        for f, call in calls.items():
            out[f"{f}/no geometry"] = [int(call(L, fresh._h)), L.ht_last_error(fresh._h).decode()]
            for case in first[f]:
                out[f"{f}/no geometry+{case}"] = [int(ok[f"{f}/{case}"](L, fresh._h)), L.ht_last_error(fresh._h).decode()]
        for key, thunk in table:
            assert key not in out, key
            out[key] = [int(thunk(L, c._h)), L.ht_last_error(c._h).decode()]
        return {"canvas": [W, H], "cases": out}
    finally:
        fresh.close()
        c.close()
        src.free()
        dst.free()

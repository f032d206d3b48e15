"""The YUV ingest (ht_draw_frames_yuv / ht_draw_frames_yuv_device: NV12 and I420 frames drawn onto the work canvas, the colour conversion
fused into the draw) against tests/yuv_cases.py's `expected`: the declared integer conversion (pinned to csrc/ht_yuv_plan.h over all 2^24
triples by tests/test_ingest_yuv_cpu.py) followed by the oracle's resampler.  Both are exact sequences of operations, so there is no
tolerance: every comparison of pixels is equality of every byte.  Without the feature every test here fails at its first call: the library
has no ht_draw_frames_yuv symbol."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import ingest_cases as ic
import yuv_cases as yc
from conftest import ROOT, load_golden
from headtrackr_amd import native, synth
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_ingest import bound_equals, d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
FMT_IDS = {yc.NV12: "nv12", yc.I420: "i420"}


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _even(v):
    return v + (v & 1)


def draw_yuv_device(c, frames, w, h, fmt, matrix, dw, dh, rect=None, y_pad=0, c_pad=0, stride_pad=0, separate=True, dstride_pad=0, lead=0, bound=False):
    """ht_draw_frames_yuv_device of host frames (a list of plane tuples) through device buffers laid out as asked (source padding filled
    with 0x5A, the destination buffer with 0xA5):
      separate   every plane in an allocation of its own, frames `stride` apart in each (stride = the largest plane + stride_pad);
                 otherwise ONE allocation, per frame the pitch-padded Y plane directly followed by the chroma plane(s)
      bound      dst NULL: into the context's own buffer (returns None); otherwise -> (frames [n, dh, dw, 4], the whole destination)"""
    n = len(frames)
    cw, ch = yc.chroma_dims(w, h)
    crow = 2 * cw if fmt == yc.NV12 else cw
    yp, cp = w + y_pad, crow + c_pad
    ybytes, cbytes = yp * h, cp * ch
    nplanes = 2 if fmt == yc.NV12 else 3

    def fill(buf, off, plane, rows, pitch, rowbytes):
        view = buf[off:off + rows * pitch].reshape(rows, pitch)
        view[:, :rowbytes] = np.ascontiguousarray(plane).reshape(rows, rowbytes)

    arrays = []
    if separate:
        stride = _even(max(ybytes, cbytes) + stride_pad)
        hosts = [np.full((n - 1) * stride + (ybytes if k == 0 else cbytes), 0x5A, dtype=np.uint8) for k in range(nplanes)]
        for f in range(n):
            fill(hosts[0], f * stride, frames[f][0], h, yp, w)
            for k in range(1, nplanes):
                fill(hosts[k], f * stride, frames[f][k], ch, cp, crow)
        arrays = [DeviceArray(hh) for hh in hosts]
        ptrs = [a.ptr for a in arrays]
    else:
        first = ybytes & 1  # NV12 wants an even chroma base: start the Y plane one byte in when its size is odd (harmless for I420)
        block = ybytes + (nplanes - 1) * cbytes
        stride = _even(block + stride_pad)
        host = np.full(first + (n - 1) * stride + block, 0x5A, dtype=np.uint8)
        for f in range(n):
            fill(host, first + f * stride, frames[f][0], h, yp, w)
            for k in range(1, nplanes):
                fill(host, first + f * stride + ybytes + (k - 1) * cbytes, frames[f][k], ch, cp, crow)
        arrays = [DeviceArray(host)]
        ptrs = [arrays[0].ptr + first + (0 if k == 0 else ybytes + (k - 1) * cbytes) for k in range(nplanes)]
    fb = dw * dh * 4
    dstride = fb + dstride_pad
    ddst = None if bound else DeviceArray(np.full(lead + n * dstride + 64, 0xA5, dtype=np.uint8))
    try:
        c.draw_frames_yuv_device(ptrs[0], ptrs[1], ptrs[2] if nplanes == 3 else None, n, w, h, fmt, matrix, y_pitch=yp if y_pad else 0, c_pitch=cp if c_pad else 0,
                                 stride=stride if n > 1 else 0, rect=rect, dst=None if bound else ddst.ptr + lead, dst_stride=dstride if dstride_pad else 0)
        c.synchronize()
        if bound:
            return None
        buf = d2h(ddst.ptr, ddst.nbytes)
    finally:
        for a in arrays:
            a.free()
        if ddst is not None:
            ddst.free()
    return np.stack([buf[lead + f * dstride:lead + f * dstride + fb].reshape(dh, dw, 4) for f in range(n)]), buf


# ---- 1 : 1, the whole frame: the bare conversion ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [yc.NV12, yc.I420], ids=FMT_IDS.get)
@pytest.mark.parametrize("size", [(97, 81), (2, 2), (1, 1), (1, 57), (61, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_to_one_is_the_bare_conversion(ctx, size, fmt):
    """same size, whole rect: every tap weight is (1, 0), so the result is the declared conversion itself — all four matrices, the grid of
    extreme values (all 216 triples at 97x81) and raw noise (most pixels clamp).  Where ht_set_geometry has no canvas as small as the
    source (the pyramid may not), the same planes are drawn onto 40x30 instead: the one-column / one-row / one-chroma-sample read paths
    are the source's, not the canvas's."""
    w, h = size
    dw, dh = w, h
    try:
        ctx.set_geometry(dw, dh, 2)
    except HtError as e:
        assert min(w, h) <= 2 and e.status == HT_ERR_INVALID, (size, str(e))
        dw, dh = 40, 30
        ctx.set_geometry(dw, dh, 2)
    for matrix in range(4):
        frames = [yc.extremes(w, h, fmt), yc.raw_noise(w, h, fmt, 7 + w + matrix)]
        got, _ = draw_yuv_device(ctx, frames, w, h, fmt, matrix, dw, dh)
        for f, what in enumerate(("extremes", "raw_noise")):
            rgba = yc.to_rgba(frames[f], w, h, fmt, matrix)
            same(got[f], ic.expected(rgba, None, dw, dh), f"{size} {FMT_IDS[fmt]} matrix {matrix} {what}")
            if (dw, dh) == (w, h):
                same(got[f], rgba, f"{size} {FMT_IDS[fmt]} matrix {matrix} {what}: 1:1 is the bare conversion")


# ---- ratio families ----------------------------------------------------------------------------------------------------------------------------

RATIO_CASES = [r for r in ic.RATIOS if r[0][0] * r[0][1] <= 400 * 400] + [((1920, 1080), (320, 240))]


@pytest.mark.parametrize("ratio", RATIO_CASES, ids=lambda r: f"{r[0][0]}x{r[0][1]}-to-{r[1][0]}x{r[1][1]}")
def test_ratio_families(ctx, ratio):
    """every ratio family of the RGBA draw whose source is at most 400x400, and 1920x1080 -> 320x240 at n = 2: NV12 and I420, matrices 0
    and 1, in-gamut content (smooth and noise frames, forward-converted).  A 1-pixel-wide or -high canvas is drawn if ht_set_geometry
    accepts the geometry."""
    (sw, sh), (dw, dh) = ratio
    try:
        ctx.set_geometry(dw, dh, 2)
    except HtError as e:
        assert min(dw, dh) == 1 and e.status == HT_ERR_INVALID, (ratio, str(e))
        return  # the library has no such geometry: nothing to draw onto
    big = sw * sh > 10 ** 6
    for fmt in (yc.NV12, yc.I420):
        for matrix in (0, 1):
            if big and (fmt, matrix) not in ((yc.NV12, 1), (yc.I420, 0)):
                continue  # (the large shape once per format: its expectation is most of this test's time)
            kinds = ("smooth",) if big else ("smooth", "noise")
            frames = [yc.from_rgb_frames(kind, sw, sh, 1, fmt, matrix, seed=sw + 7 * dh + k)[0] for k, kind in enumerate(kinds)]
            if big:
                frames.append(yc.from_rgb(synth.face_frame(sw, sh, [(700, 300, 500)]), fmt, matrix))
            got, _ = draw_yuv_device(ctx, frames, sw, sh, fmt, matrix, dw, dh)
            for f in range(len(frames)):
                same(got[f], yc.expected(frames[f], sw, sh, fmt, matrix, None, dw, dh), f"{ratio} {FMT_IDS[fmt]} matrix {matrix} frame {f}")


# ---- source rects ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [yc.NV12, yc.I420], ids=FMT_IDS.get)
@pytest.mark.parametrize("case", yc.RECT_CASES, ids=lambda r: f"{r[0][0]}x{r[0][1]}-to-{r[1][0]}x{r[1][1]}")
def test_source_rects_clamp_to_the_rect_and_site_chroma_by_the_frame(ctx, case, fmt):
    """odd origins, rects touching the last column and row, 1-pixel rects.  Frame 0 is the plain frame, frame 1 the same with everything
    outside the rect replaced (Y outside the rect, chroma outside the samples the rect names — yuv_cases.outside_filled): both must give
    the oracle's result for the plain frame.  A draw that clamps its taps to the frame, or sites chroma relative to the rect, fails."""
    (sw, sh), (dw, dh) = case
    ctx.set_geometry(dw, dh, 2)
    matrix = 1 if fmt == yc.NV12 else 0
    base = yc.from_rgb_frames("noise", sw, sh, 1, fmt, matrix, seed=5)[0]
    rgba = yc.to_rgba(base, sw, sh, fmt, matrix)
    for ri, rect in enumerate(ic.rects_for(sw, sh)):
        filled = yc.outside_filled(base, sw, sh, fmt, rect, 90 + ri)
        got, _ = draw_yuv_device(ctx, [base, filled], sw, sh, fmt, matrix, dw, dh, rect=rect)
        want = ic.expected(rgba, rect, dw, dh)
        same(got[0], want, f"{case} {FMT_IDS[fmt]} rect {rect}")
        same(got[1], want, f"{case} {FMT_IDS[fmt]} rect {rect}, outside replaced")
        x, y, w, h = rect
        same(got[0], ic.expected(np.ascontiguousarray(rgba[y:y + h, x:x + w]), None, dw, dh), f"{case} {FMT_IDS[fmt]} rect {rect} vs the cropped frame")


# ---- layout ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [yc.NV12, yc.I420], ids=FMT_IDS.get)
@pytest.mark.parametrize("layout", ["pitches", "separate-n3-stride", "one-allocation-pitched", "one-allocation-n3"])
def test_pitches_strides_allocations_and_sentinels(ctx, layout, fmt):
    """Y pitch = w + 13 and chroma pitch = packed + 6; planes in separate allocations; n = 3 with a frame stride larger than a frame; the
    chroma plane directly behind a pitch-padded Y plane in one allocation (333 x 217 and pitch 346: the Y plane of one frame is 75 082
    bytes, so NV12's chroma base is even; frames an even stride apart); the destination at an offset that is only 4-byte aligned with a
    stride: every frame equals the oracle and every destination byte outside the frames keeps its sentinel"""
    (sw, sh), (dw, dh) = (333, 217), (160, 120)
    ctx.set_geometry(dw, dh, 2)  # the device form into a caller's buffer is not limited by the batch capacity
    bound_before = ctx._lib.ht_frames_bound(ctx._h)
    kw = {"pitches": dict(n=1, y_pad=13, c_pad=6), "separate-n3-stride": dict(n=3, stride_pad=4 * 41), "one-allocation-pitched": dict(n=1, y_pad=13, c_pad=6, separate=False),
          "one-allocation-n3": dict(n=3, y_pad=13, stride_pad=102, separate=False)}[layout]
    n = kw.pop("n")
    matrix = 1
    frames = yc.from_rgb_frames("noise", sw, sh, n, fmt, matrix, seed=300 + n)
    rect = (3, 5, sw - 7, sh - 9)
    lead, dpad = 12, 20
    got, buf = draw_yuv_device(ctx, frames, sw, sh, fmt, matrix, dw, dh, rect=rect, dstride_pad=dpad, lead=lead, **kw)
    fb = dw * dh * 4
    assert (buf[:lead] == 0xA5).all()
    for f in range(n):
        same(got[f], yc.expected(frames[f], sw, sh, fmt, matrix, rect, dw, dh), f"{layout} frame {f}")
        gap = buf[lead + f * (fb + dpad) + fb:lead + (f + 1) * (fb + dpad)]
        assert len(gap) == dpad and (gap == 0xA5).all(), (layout, f)
    assert (buf[lead + n * (fb + dpad):] == 0xA5).all()
    assert ctx._lib.ht_frames_bound(ctx._h) == bound_before  # a draw into a caller's buffer binds nothing


def test_bound_form_and_host_form_equal_the_device_form(ctx):
    """dst NULL binds the result; the host form (packed frames, also at a frame stride beyond packed, also an odd x odd NV12 frame, which is
    staged one byte into the buffer) binds the same frames as the device form writes"""
    (sw, sh), (dw, dh), n = (333, 217), (160, 120), 3
    ctx.set_geometry(dw, dh, n)
    for fmt, matrix in ((yc.NV12, 0), (yc.I420, 3)):
        frames = yc.from_rgb_frames("smooth", sw, sh, n, fmt, matrix, seed=41)
        for rect in (None, (5, 3, 122, 77)):
            dev, _ = draw_yuv_device(ctx, frames, sw, sh, fmt, matrix, dw, dh, rect=rect)
            want = np.stack([yc.expected(frames[f], sw, sh, fmt, matrix, rect, dw, dh) for f in range(n)])
            same(dev, want, f"device form, {FMT_IDS[fmt]} rect {rect}")
            draw_yuv_device(ctx, frames, sw, sh, fmt, matrix, dw, dh, rect=rect, bound=True)
            bound_equals(ctx, want, f"bound form, {FMT_IDS[fmt]} rect {rect}")
            y, *chroma = [np.stack([fr[k] for fr in frames]) for k in range(len(frames[0]))]
            ctx.draw_frames_yuv([y] + chroma, FMT_IDS[fmt], yc.MATRIX_NAMES[matrix], rect=rect)
            bound_equals(ctx, want, f"host form, {FMT_IDS[fmt]} rect {rect}")
        # frames 101 bytes further apart than packed, two of them
        fsz = yc.frame_bytes(sw, sh)
        host = np.full(2 * (fsz + 101), 0x5A, dtype=np.uint8)
        for f in range(2):
            host[f * (fsz + 101):f * (fsz + 101) + fsz] = yc.pack(frames[f + 1])
        ctx.draw_frames_yuv_ptr(host.ctypes.data, 2, sw, sh, fmt, matrix, fsz + 101)
        bound_equals(ctx, np.stack([yc.expected(frames[f + 1], sw, sh, fmt, matrix, None, dw, dh) for f in range(2)]), f"host form at a stride, {FMT_IDS[fmt]}")


# ---- the bound form feeds the pipeline ---------------------------------------------------------------------------------------------------------

def test_bound_form_feeds_detect_and_camshift(cascade):
    """draw_frames_yuv of a forward-converted golden detect frame, then detect: identical to upload of to_rgba of the same planes, then
    detect (and to the oracle's hits on that frame); then camshift init + one track on the next frame, same comparison"""
    from test_gpu_detect import assert_hits_equal, oracle_hits

    case = next(c for c in load_golden("detect.json")["cases"] if "interval3" not in c["name"])
    w, h = case["w"], case["h"]
    src = [synth.make(case["gen"], w, h), np.roll(synth.make(case["gen"], w, h), 3, axis=1)]
    a, b = Context(), Context()
    try:
        for c in (a, b):
            c.set_geometry(w, h, 1)
            c.camshift_reserve(1)
        for fmt, matrix in ((yc.NV12, 0), (yc.I420, 1)):
            planes = [yc.from_rgb(s, fmt, matrix) for s in src]
            rgba = [yc.to_rgba(p, w, h, fmt, matrix) for p in planes]
            a.draw_frames_yuv([p[None] for p in planes[0]], fmt, matrix)
            b.upload(rgba[0][None])
            res = []
            for c in (a, b):
                c.detect_enqueue(0)
                res.append(c.detect_collect())
            assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
            assert_hits_equal(res[0][0], oracle_hits(rgba[0], cascade, 0))
            assert len(res[0][0]) > 0, "the forward-converted golden frame still has detections"
            assert [float(v) for v in a.whitebalance()] == [float(v) for v in b.whitebalance()] == [ho.whitebalance(rgba[0])]
            rect = (w // 4, h // 4, w // 2, h // 2)
            a.camshift_init([rect])
            b.camshift_init([rect])
            a.draw_frames_yuv([p[None] for p in planes[1]], fmt, matrix)
            b.upload(rgba[1][None])
            ta, tb = a.camshift_track(1, calc_angles=True), b.camshift_track(1, calc_angles=True)
            assert ta.tobytes() == tb.tobytes(), (ta, tb)
            o = ho.Camshift(True)
            o.init_tracker(rgba[0], rect)
            sw_, to = o.track(rgba[1])
            assert [int(ta[0][k]) for k in ("sw_x", "sw_y", "sw_width", "sw_height")] == list(sw_)
            assert all(float(ta[0][k]) == to[k] for k in ("x", "y", "width", "height"))
    finally:
        a.close()
        b.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_as_it_was():
    """one refused call per check of the C ABI: its status, a message, the binding untouched — the bound frames still read back whole
    through the pyramid and getWhitebalance (bound_equals runs a detect) — and the next call on the same context succeeds"""
    (sw, sh), (dw, dh), n = (63, 47), (40, 30), 2
    cw, ch = yc.chroma_dims(sw, sh)
    frames = {fmt: yc.from_rgb_frames("noise", sw, sh, n, fmt, 0, seed=9) for fmt in (yc.NV12, yc.I420)}
    want = np.stack([yc.expected(frames[yc.NV12][f], sw, sh, yc.NV12, 0, None, dw, dh) for f in range(n)])
    stride = 4096  # >= every plane of a 63 x 47 frame (2961 / 1536 / 768 bytes), even
    assert stride >= sw * sh and stride >= 2 * cw * ch

    def planes_of(fmt, k):
        buf = np.full(n * stride, 0x5A, dtype=np.uint8)
        for f in range(n):
            p = np.ascontiguousarray(frames[fmt][f][k]).reshape(-1)
            buf[f * stride:f * stride + len(p)] = p
        return DeviceArray(buf)

    dev = {(fmt, k): planes_of(fmt, k) for fmt in (yc.NV12, yc.I420) for k in range(2 if fmt == yc.NV12 else 3)}
    fb = dw * dh * 4
    ddst = DeviceArray(np.zeros(2 * n * fb, dtype=np.uint8))
    host = {fmt: np.concatenate([yc.pack(frames[fmt][f]) for f in range(n)]) for fmt in (yc.NV12, yc.I420)}
    c = Context()
    L, h = c._lib, c._h

    def devcall(fmt=yc.NV12, n_=n, w=sw, h_=sh, matrix=0, y=None, u=None, v=None, yp=0, cp=0, st=stride, rect=None, dst=ddst.ptr, dstride=0, fmt_code=None, desc=True):
        d = native.YUV_FRAMES(dev[(fmt, 0)].ptr if y is None else y, dev[(fmt, 1)].ptr if u is None else u,
                              (dev[(fmt, 2)].ptr if fmt == yc.I420 else None) if v is None else v, yp, cp, st, w, h_, fmt if fmt_code is None else fmt_code, matrix)
        r = Context._cs_rect(rect)
        return L.ht_draw_frames_yuv_device(h, C.byref(d) if desc else None, n_, r.ctypes.data if r is not None else None, dst, dstride)

    def hostcall(fmt=yc.NV12, ptr="data", n_=n, w=sw, h_=sh, fmt_code=None, matrix=0, st=0, rect=None):
        r = Context._cs_rect(rect)
        return L.ht_draw_frames_yuv(h, host[fmt].ctypes.data if ptr == "data" else ptr, n_, w, h_, fmt if fmt_code is None else fmt_code, matrix, st, r.ctypes.data if r is not None else None)

    try:
        assert devcall() == HT_ERR_STATE and hostcall() == HT_ERR_STATE  # no geometry yet
        assert b"ht_set_geometry" in L.ht_last_error(h)
        c.set_geometry(dw, dh, n)
        c.draw_frames_yuv_ptr(host[yc.NV12].ctypes.data, n, sw, sh, yc.NV12, 0)
        bound_equals(c, want, "before the refused calls")
        bad = [
            ("NULL description", lambda: devcall(desc=False)), ("NULL Y plane", lambda: devcall(y=0)), ("NULL chroma plane", lambda: devcall(u=0)),
            ("NULL V plane (I420)", lambda: devcall(fmt=yc.I420, v=0)), ("NULL host source", lambda: hostcall(ptr=None)),
            ("format out of range", lambda: devcall(fmt_code=2)), ("negative format, host form", lambda: hostcall(fmt_code=-1)),
            ("matrix out of range", lambda: devcall(matrix=4)), ("negative matrix, host form", lambda: hostcall(matrix=-1)),
            ("Y pitch smaller than a row", lambda: devcall(yp=sw - 1)), ("chroma pitch smaller than a row (NV12)", lambda: devcall(cp=2 * cw - 2)),
            ("chroma pitch smaller than a row (I420)", lambda: devcall(fmt=yc.I420, cp=cw - 1)), ("odd chroma pitch (NV12)", lambda: devcall(cp=2 * cw + 1)),
            ("odd chroma base (NV12)", lambda: devcall(u=dev[(yc.NV12, 1)].ptr + 1)), ("odd frame stride (NV12)", lambda: devcall(st=stride + 1)),
            ("no frame stride for n > 1", lambda: devcall(st=0)), ("frame stride smaller than a Y plane", lambda: devcall(st=sw * sh - 1)),
            ("host frame stride smaller than a frame", lambda: hostcall(st=yc.frame_bytes(sw, sh) - 1)),
            ("rect beyond the right edge", lambda: devcall(rect=(10, 0, sw - 9, sh))), ("rect beyond the bottom edge", lambda: hostcall(rect=(0, 1, sw, sh))),
            ("rect with a negative origin", lambda: devcall(rect=(-1, 0, 8, 8))), ("empty rect", lambda: hostcall(rect=(0, 0, 0, 5))),
            ("n = 0", lambda: devcall(n_=0)), ("n < 0", lambda: hostcall(n_=-1)), ("zero width", lambda: devcall(w=0)), ("negative height", lambda: hostcall(h_=-3)),
            ("n above the batch capacity, bound form", lambda: devcall(n_=n + 1, dst=None, st=stride)), ("n above the batch capacity, host form", lambda: hostcall(n_=n + 1)),
            ("misaligned destination", lambda: devcall(dst=ddst.ptr + 2)), ("destination stride too small", lambda: devcall(dstride=fb - 4)),
            ("destination inside the Y plane", lambda: devcall(dst=dev[(yc.NV12, 0)].ptr + 4)), ("destination inside the chroma plane", lambda: devcall(dst=dev[(yc.NV12, 1)].ptr + 8)),
            ("destination inside the V plane (I420)", lambda: devcall(fmt=yc.I420, dst=dev[(yc.I420, 2)].ptr)),
        ]
        for what, call in bad:
            assert call() == HT_ERR_INVALID, what
            assert len(L.ht_last_error(h)) > 10, what
            assert L.ht_frames_bound(h) == n, what
            bound_equals(c, want, f"after: {what}")
            assert devcall() == 0, what  # ... and the next call on the same context succeeds
            same(c.device_download(ddst.ptr, n * fb).reshape(n, dh, dw, 4), want, f"draw after: {what}")
        for p in dev.values():  # the refused overlaps wrote nothing into the planes
            assert (d2h(p.ptr, p.nbytes)[stride - 8:stride] == 0x5A).all()
    finally:
        c.close()
        for p in dev.values():
            p.free()
        ddst.free()


# ---- Node ----------------------------------------------------------------------------------------------------------------------------------------

def test_node_facade_draws_yuv_on_the_device(tmp_path, cascade):
    """tests/js/ingest_yuv_gpu.js on the real addon: ccv.drawFrames of NV12 and I420 video-like objects at 333x217 -> 160x120 (whole frame
    and a rect) and a ccv.DeviceBatch with sourceFormat: uploadSource, draw, drawBound and the step functions on the result"""
    from headtrackr_amd import build

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    (sw, sh), (dw, dh), n = (333, 217), (160, 120), 2
    rect = (21, 13, 280, 190)
    job = dict(sw=sw, sh=sh, w=dw, h=dh, n=n, rect=list(rect), dir=str(tmp_path), videos=[])
    rgb = np.stack([synth.face_frame(sw, sh, [(90 + 30 * f, 30, 150)]) for f in range(n)])
    for fmt, matrix in ((yc.NV12, 0), (yc.I420, 1)):
        frames = [yc.from_rgb(rgb[f], fmt, matrix) for f in range(n)]
        name = f"video_{FMT_IDS[fmt]}.yuv"
        np.concatenate([yc.pack(p) for p in frames]).tofile(tmp_path / name)
        want = np.stack([yc.expected(p, sw, sh, fmt, matrix, None, dw, dh) for p in frames])
        want_rect = np.stack([yc.expected(p, sw, sh, fmt, matrix, rect, dw, dh) for p in frames])
        want.tofile(tmp_path / f"want_{FMT_IDS[fmt]}.raw")
        want_rect.tofile(tmp_path / f"want_rect_{FMT_IDS[fmt]}.raw")
        best = ho.best_faces(want, cascade.blob, 1)
        job["videos"].append(dict(file=name, format=FMT_IDS[fmt], matrix=yc.MATRIX_NAMES[matrix], want=f"want_{FMT_IDS[fmt]}.raw", want_rect=f"want_rect_{FMT_IDS[fmt]}.raw",
                                  wb=[ho.whitebalance(want[f]) for f in range(n)], wb_rect=[ho.whitebalance(want_rect[f]) for f in range(n)],
                                  best=[{k: float(best[k][f]) for k in ("x", "y", "width", "height", "confidence")} for f in range(n)]))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "ingest_yuv_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ingest_yuv_gpu: ok" in r.stdout, r.stdout[-2000:]

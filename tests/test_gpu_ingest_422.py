"""Packed YUV 4:2:2 frames (HT_YUV_YUYV / HT_YUV_UYVY) through the draw calls — ht_draw_frames_yuv, ht_draw_frames_yuv_device,
ht_draw_list_device, ht_draw_list_filtered_device — and the face-patch calls (ht_camshift_crop_sources_* / ht_camshift_align_sources_*)
against tests/yuv422_cases.py: the declared conversion (one plane of 4-byte macropixels, chroma of pixel (x, y) = macropixel (x >> 1) of
row y) followed by the oracle's resampler, and against the existing kernels on the RGBA frame that conversion produces.  Every comparison is
equality of every byte.  The case list is yuv422_cases.CASES, whose sufficiency tests/test_ingest_422_cpu.py proves from the restatement
alone.  Each call runs in a fresh context of the case's geometry.  On the parent commit every call here fails with HT_ERR_INVALID (format 4
is refused)."""
import contextlib

import numpy as np
import pytest

import ingest_cases as ic
import yuv422_cases as y4
import yuv_cases as yc
from headtrackr_amd.api import Context, HtError, draw_filter_factors
from hipmem import DeviceArray
from test_gpu_ingest import bound_equals, d2h, draw_device, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID = -1
FMTS = (y4.YUYV, y4.UYVY)
PAD, GUARD = 0x5A, 0xA5


@contextlib.contextmanager
def fresh(dw, dh, n=1):
    c = Context()
    try:
        c.set_geometry(dw, dh, n)
        yield c
    finally:
        c.close()


def resident(case, frames):
    """the frames of a case in ONE allocation laid out as the case says: base_off bytes in, rows `pitch` apart, frames `stride` apart, every
    byte that is no frame's 0x5A -> (DeviceArray, pointer of frame 0)"""
    host = np.full(case.base_off + (len(frames) - 1) * case.stride + case.extent, PAD, dtype=np.uint8)
    for f, fr in enumerate(frames):
        for r in range(case.h):
            o = case.base_off + f * case.stride + r * case.pitch
            host[o:o + 4 * case.cw] = fr[r]
    arr = DeviceArray(host)
    return arr, arr.ptr + case.base_off


def draw_device_422(c, case, frames, fmt, matrix, rect=None):
    """ht_draw_frames_yuv_device into a guarded caller's buffer -> frames [n, dh, dw, 4]"""
    n, fb = len(frames), case.dw * case.dh * 4
    arr, ptr = resident(case, frames)
    dst = DeviceArray(np.full(n * fb + 64, GUARD, dtype=np.uint8))
    try:
        c.draw_frames_yuv_device(ptr, None, None, n, case.w, case.h, fmt, matrix, y_pitch=case.pitch if case.pitch_pad else 0, stride=case.stride if n > 1 else 0,
                                 rect=rect, dst=dst.ptr)
        c.synchronize()
        buf = d2h(dst.ptr, dst.nbytes)
    finally:
        arr.free()
        dst.free()
    assert (buf[n * fb:] == GUARD).all()
    return buf[:n * fb].reshape(n, case.dh, case.dw, 4)


def content(case, fmt, matrix, kind, seed):
    if kind == "extremes":
        return [y4.extremes(case.w, case.h, fmt) for _ in range(case.n)]
    if kind == "raw":
        return [y4.raw_noise(case.w, case.h, fmt, seed + 17 * f) for f in range(case.n)]
    return y4.from_rgb_frames(kind, case.w, case.h, case.n, fmt, matrix, seed=seed)


# ---- 1: single source ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", y4.CASES, ids=lambda c: c.name)
def test_single_source_equals_the_restatement_and_the_rgba_draw(case):
    """both formats x four matrices over the case (in-gamut noise), extremes and raw noise on one matrix each: the device form equals
    yuv422_cases.expected AND ht_draw_frames_device (k_draw_frames, the second witness) on to_rgba(frame) uploaded as RGBA; the host form
    binds the same frames and ht_frames_bound() == n"""
    runs = [(fmt, m, "noise") for fmt in FMTS for m in range(4)] + [(y4.YUYV, 1, "extremes"), (y4.UYVY, 2, "raw")]
    for fmt, matrix, kind in runs:
        frames = content(case, fmt, matrix, kind, 40 + case.w + matrix)
        rgba = np.stack([y4.to_rgba(fr, case.w, case.h, fmt, matrix) for fr in frames])
        for rect in case.rects if kind == "noise" else case.rects[:1]:
            what = f"{case.name} {y4.FORMAT_NAMES[fmt]} matrix {matrix} {kind} rect {rect}"
            want = np.stack([ic.expected(rgba[f], rect, case.dw, case.dh) for f in range(case.n)])
            with fresh(case.dw, case.dh, case.n) as c:
                same(draw_device_422(c, case, frames, fmt, matrix, rect), want, what)
            with fresh(case.dw, case.dh, case.n) as c:
                same(draw_device(c, rgba, case.dw, case.dh, rect=rect)[0], want, what + ": k_draw_frames on to_rgba")
            with fresh(case.dw, case.dh, case.n) as c:
                if case.gap:  # the host form with frames `stride` apart and a gap between them: one copy per frame into the staging buffer
                    fsz, step = y4.frame_bytes(case.w, case.h), y4.frame_bytes(case.w, case.h) + case.gap
                    host = np.full((case.n - 1) * step + fsz, PAD, dtype=np.uint8)
                    for f, fr in enumerate(frames):
                        host[f * step:f * step + fsz] = fr.reshape(-1)
                    c.draw_frames_yuv_ptr(host.ctypes.data, case.n, case.w, case.h, fmt, matrix, step, rect)
                else:
                    c.draw_frames_yuv(np.stack(frames), y4.FORMAT_NAMES[fmt], yc.MATRIX_NAMES[matrix], rect=rect, width=case.w)
                assert c._lib.ht_frames_bound(c._h) == case.n
                bound_equals(c, want, what + ": host form")


# ---- 2: the 4:2:0 identity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", y4.CASES[:2], ids=lambda c: c.name)
def test_doubled_chroma_rows_equal_the_i420_draw(case):
    """for I420 planes p, the draw of from_i420(p) as YUYV and as UYVY equals the draw of p through the existing k_draw_yuv<I420>"""
    from test_gpu_ingest_yuv import draw_yuv_device

    matrix = 1
    planes = yc.from_rgb_frames("noise", case.w, case.h, 1, yc.I420, matrix, seed=77)[0]
    with fresh(case.dw, case.dh) as c:
        want, _ = draw_yuv_device(c, [planes], case.w, case.h, yc.I420, matrix, case.dw, case.dh)
    for fmt in FMTS:
        with fresh(case.dw, case.dh) as c:
            same(draw_device_422(c, case, [y4.from_i420(planes, fmt)], fmt, matrix), want, f"{case.name} {y4.FORMAT_NAMES[fmt]} against I420")


# ---- 3, 4: the draw list and the filtered draw list ----------------------------------------------------------------------------------------------

class Feeds:
    """[YUYV, NV12, UYVY, RGBA, I420, YUYV-with-rect] in separate allocations (the last shares the first's plane pointer)"""

    def __init__(self):
        import draw_list_cases as dl

        a, b = y4.CASES[0], y4.CASES[2]  # 97 x 81 packed; 333 x 217 pitched, 4 bytes into its allocation
        self.w, self.h = a.dw, a.dh
        self.y0 = y4.from_rgb_frames("noise", a.w, a.h, 1, y4.YUYV, 0, seed=5)[0]
        self.u2 = y4.raw_noise(b.w, b.h, y4.UYVY, 6)
        self.arr0, p0 = resident(a, [self.y0])
        self.arr2, p2 = resident(b, [self.u2])
        self.planar = [dl.Source(yc.NV12, 23, 23, seed=14, matrix=3, pad0=1, pad1=2), dl.Source(dl.RGBA, 97, 81, seed=11, pad0=12), dl.Source(yc.I420, 97, 81, seed=16, matrix=2, pad0=7, pad1=9)]
        self.parrs = [[DeviceArray(x) for x in s.plane_buffers()] for s in self.planar]
        pe = [s.entry([x.ptr for x in arrs]) for s, arrs in zip(self.planar, self.parrs)]
        rect = ic.rects_for(a.w, a.h)[5]  # (3, 5, w - 7, h - 9): odd origin
        e0 = dict(format="yuyv", width=a.w, height=a.h, matrix=0, p0=p0, rect=None)
        e2 = dict(format="uyvy", width=b.w, height=b.h, matrix=2, p0=p2, pitch0=b.pitch, rect=None)
        e5 = dict(format=y4.YUYV, width=a.w, height=a.h, matrix=1, p0=p0, rect=rect)
        self.entries = [e0, pe[0], e2, pe[1], pe[2], e5]
        self.planar_entries = pe
        r0, r2 = y4.to_rgba(self.y0, a.w, a.h, y4.YUYV, 0), y4.to_rgba(self.u2, b.w, b.h, y4.UYVY, 2)
        r5 = y4.to_rgba(self.y0, a.w, a.h, y4.YUYV, 1)
        self.rgba_views = [(r0, None), (self.planar[0].rgba, None), (r2, None), (self.planar[1].rgba, None), (self.planar[2].rgba, None), (r5, rect)]

    def free(self):
        for x in [self.arr0, self.arr2] + [x for arrs in self.parrs for x in arrs]:
            x.free()


@pytest.fixture(scope="module")
def feeds():
    f = Feeds()
    yield f
    f.free()


def list_call(feeds, entries, prefilter=None):
    n, fb = len(entries), feeds.w * feeds.h * 4
    dst = DeviceArray(np.full(n * fb + 64, GUARD, dtype=np.uint8))
    try:
        with fresh(feeds.w, feeds.h, n) as c:
            c.draw_list(entries, dst=dst.ptr, prefilter=prefilter)
            c.synchronize()
        buf = d2h(dst.ptr, dst.nbytes)
    finally:
        dst.free()
    assert (buf[n * fb:] == GUARD).all()
    return buf[:n * fb].reshape(n, feeds.h, feeds.w, 4)


def test_draw_list_of_mixed_formats_in_one_launch(feeds):
    """one launch over [YUYV, NV12, UYVY, RGBA, I420, YUYV-with-rect]: every frame equals the restatement (which the single-source test pins
    the single-source call to); the NV12 / RGBA / I420 frames equal what the list without the packed entries gives (k_draw_list); two entries
    share one plane pointer"""
    assert feeds.entries[0]["p0"] == feeds.entries[5]["p0"]
    got = list_call(feeds, feeds.entries)
    for i, (rgba, rect) in enumerate(feeds.rgba_views):
        same(got[i], ic.expected(rgba, rect, feeds.w, feeds.h), f"entry {i}")
    planar = list_call(feeds, feeds.planar_entries)
    for k, i in enumerate((1, 3, 4)):
        same(got[i], planar[k], f"entry {i} against the list without the packed entries")


@pytest.mark.parametrize("canvas_factor", [((40, 48), (3, 2)), ((97, 81), (1, 1))], ids=["3x2", "1x1"])
def test_filtered_draw_list_converts_the_taps_first(canvas_factor):
    """a packed entry at factors (3, 2) and (1, 1) equals ht_draw_list_filtered_device on the RGBA entry holding to_rgba(frame); factors
    (1, 1) equal the unfiltered call"""
    (W, H), (nx, ny) = canvas_factor
    case = y4.CASES[0]
    for fmt, matrix in ((y4.YUYV, 1), (y4.UYVY, 2)):
        frame = y4.raw_noise(case.w, case.h, fmt, 31 + fmt)
        rgba = y4.to_rgba(frame, case.w, case.h, fmt, matrix)
        arr, ptr = resident(case, [frame])
        rarr = DeviceArray(rgba)
        dst = DeviceArray(np.zeros(3 * W * H * 4, dtype=np.uint8))
        fb = W * H * 4
        try:
            with fresh(W, H) as c:
                assert tuple(int(v) for v in draw_filter_factors([(case.w, case.h)], W, H, 8)[0]) == (nx, ny)
                e = dict(format=fmt, width=case.w, height=case.h, matrix=matrix, p0=ptr)
                c.draw_list([e], dst=dst.ptr, prefilter=8)
                c.draw_list([dict(format="rgba", width=case.w, height=case.h, p0=rarr.ptr)], dst=dst.ptr + fb, prefilter=8)
                c.draw_list([e], dst=dst.ptr + 2 * fb)
                c.synchronize()
            got = d2h(dst.ptr, dst.nbytes).reshape(3, H, W, 4)
        finally:
            for x in (arr, rarr, dst):
                x.free()
        same(got[0], got[1], f"{y4.FORMAT_NAMES[fmt]} factors {(nx, ny)} against the RGBA entry")
        if (nx, ny) == (1, 1):
            same(got[0], got[2], f"{y4.FORMAT_NAMES[fmt]} factors (1, 1) against the unfiltered call")
            same(got[0], ic.expected(rgba, None, W, H), f"{y4.FORMAT_NAMES[fmt]} factors (1, 1) against the restatement")


# ---- 6: refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    """misaligned base, pitch not a multiple of 4, pitch too small, a rect outside: HT_ERR_INVALID each, `entry <i>` in the message of the
    list calls, the destination and the binding as they were (the destination is downloaded before and after)"""
    case = y4.CASES[0]
    frame = y4.from_rgb_frames("smooth", case.w, case.h, 1, y4.YUYV, 0, seed=3)[0]
    arr, ptr = resident(Case_with_room(case), [frame])
    dw, dh, fb = case.dw, case.dh, case.dw * case.dh * 4
    dst = DeviceArray(np.full(2 * fb, GUARD, dtype=np.uint8))
    good = dict(format="yuyv", width=case.w, height=case.h, matrix=0, p0=ptr, pitch0=4 * case.cw + 8)
    rgba = dict(format="rgba", width=2, height=2, p0=ptr)
    bad = [("misaligned base", dict(good, p0=ptr + 2)), ("pitch not a multiple of 4", dict(good, pitch0=4 * case.cw + 6)), ("pitch too small", dict(good, pitch0=4 * case.cw - 4)),
           ("rect outside", dict(good, rect=(10, 0, case.w - 9, case.h)))]
    try:
        with fresh(dw, dh, 2) as c:
            c.draw_list([rgba, good])  # bound: two frames
            want = np.stack([ic.expected(np.frombuffer(d2h(ptr, 16).tobytes(), dtype=np.uint8).reshape(2, 2, 4), None, dw, dh),
                             ic.expected(y4.to_rgba(frame, case.w, case.h, y4.YUYV, 0), None, dw, dh)])
            bound_equals(c, want, "before the refused calls")
            for what, e in bad:
                before = d2h(dst.ptr, dst.nbytes)
                for prefilter in (None, 4):
                    with pytest.raises(HtError) as ei:
                        c.draw_list([rgba, e], dst=dst.ptr, prefilter=prefilter)
                    assert ei.value.status == HT_ERR_INVALID and "entry 1" in str(ei.value), (what, str(ei.value))
                with pytest.raises(HtError) as ei:
                    c.draw_frames_yuv_device(e["p0"], None, None, 1, case.w, case.h, "yuyv", 0, y_pitch=e["pitch0"], rect=e.get("rect"), dst=dst.ptr)
                assert ei.value.status == HT_ERR_INVALID, what
                c.synchronize()
                assert np.array_equal(d2h(dst.ptr, dst.nbytes), before), what
                assert c._lib.ht_frames_bound(c._h) == 2, what
            bound_equals(c, want, "after the refused calls")
    finally:
        arr.free()
        dst.free()


def Case_with_room(case):
    """the 97 x 81 case with 8 spare bytes per row, so that every malformed description above still names memory that exists"""
    return y4.Case(case.name + "-room", (case.w, case.h), (case.dw, case.dh), pitch_pad=8)


# ---- 5: face patches ---------------------------------------------------------------------------------------------------------------------------

def tilted_picture(w, h):
    """a dark frame with a bright diagonal band (tilted against both axes) and a bright upright block: two blobs for two trackers"""
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 4), dtype=np.uint8)
    f[..., :3] = (30, 40, 90)
    f[np.abs((xx - 30) - 0.6 * (yy - 40)) < 5] = (230, 120, 60, 255)
    f[20:60, 70:86] = (60, 220, 110, 255)
    f[..., 3] = 255
    return f


@pytest.mark.parametrize("kind", ["crop", "align"])
def test_face_patches_from_a_packed_feed_equal_those_from_its_rgba_conversion(kind):
    """two trackers (one on an upright block, one on a tilted band) on a 97 x 81 feed drawn onto its canvas: crop_sources / align_sources
    with the feed given as YUYV, then as the RGBA entry of to_rgba(frame) — RGBA8, f16 CHW tensors and filtered with max_factor 4, at
    margins 1 and 3 (a box that leaves the frame: the zeros outside must match too) — give the same bytes and the same records"""
    from headtrackr_amd.api import PatchFormat

    case = y4.CASES[0]
    w, h, P, Q = case.w, case.h, 70, 19
    frame = y4.from_rgb(tilted_picture(w, h), y4.YUYV, 2)
    rgba = y4.to_rgba(frame, w, h, y4.YUYV, 2)
    arr, ptr = resident(case, [frame])
    rarr = DeviceArray(rgba)
    packed = dict(format="yuyv", width=w, height=h, matrix=2, p0=ptr)
    plain = dict(format="rgba", width=w, height=h, p0=rarr.ptr)
    fmt = PatchFormat("f16", "chw", "rgb")
    forms = {"rgba8": (P * Q * 4, lambda c, o, e, m: getattr(c, f"camshift_{kind}_sources_device")(o, [0, 1], e, P, Q, margin=m)),
             "f16-chw": (3 * P * Q * 2, lambda c, o, e, m: getattr(c, f"camshift_{kind}_sources_tensor_device")(o, [0, 1], e, P, Q, fmt, margin=m)),
             "filtered": (P * Q * 4, lambda c, o, e, m: getattr(c, f"camshift_{kind}_sources_filtered_device")(o, [0, 1], e, P, Q, max_factor=4, margin=m))}
    outside = 0
    try:
        with fresh(w, h, 2) as c:  # the canvas has the feed's size: the trackers' boxes are the feed's pixels
            c.draw_list([packed, packed])
            c.camshift_reserve(2)
            c.camshift_init_pairs([(0, 0), (1, 1)], [(66, 16, 24, 48), (14, 14, 40, 56)])
            objs = c.camshift_track_pairs([(0, 0), (1, 1)], calc_angles=True)
            assert abs(float(objs[0]["angle"]) - float(objs[1]["angle"])) > 0.2, objs  # one upright, one tilted
            for name, (pb, call) in forms.items():
                for margin in (1.0, 3.0):
                    got = []
                    for entry in (packed, plain):
                        out = DeviceArray(np.full(2 * pb + 64, GUARD, dtype=np.uint8))
                        try:
                            call(c, out.ptr, [entry, entry], margin)
                            rec = getattr(c, f"camshift_{kind}_result")(2)
                            c.synchronize()
                            got.append((d2h(out.ptr, out.nbytes), rec.tobytes()))
                        finally:
                            out.free()
                    what = f"{kind} {name} margin {margin}"
                    same(got[0][0], got[1][0], what + ": bytes")
                    assert got[0][1] == got[1][1], what + ": records"
                    assert (got[0][0][2 * pb:] == GUARD).all() and not (got[0][0][:2 * pb] == GUARD).all(), what
                    if kind == "align" and name == "rgba8" and margin == 3.0:
                        px = got[0][0][:2 * pb].reshape(-1, 4)
                        outside = int((px == 0).all(axis=1).sum())
                        assert 0 < outside < len(px), what + ": the box leaves the frame, and not wholly"
    finally:
        arr.free()
        rarr.free()


# ---- 5b: the staging buffer the routes share --------------------------------------------------------------------------------------------------

def test_the_routes_share_one_staging_buffer():
    """ONE context, a 40 x 30 canvas, sources of 34 x 18 at the most; every step against the CPU oracle of its case module, byte for byte.
      1. ht_draw_frames from host RGBA: stages 2448 bytes into the context's ingest staging buffer (the first allocation);
      2. at once, without a wait in between, crop_sources of [YUYV, NV12 under rot 1, RGBA]: the same buffer GROWS to 4896 bytes while step
         1's draw may still read the old one, and is carved into the oriented job's frame (offset 0) and the unpacked YUYV frame (offset
         2448).  (Freeing device memory waits by itself, so this does not prove the reserve's own wait; it pins the offsets and the order);
      3. ht_draw_frames_yuv from host I420 and from host NV12 at 33 x 17 (odd x odd: NV12 is staged one byte into the buffer), two frames;
      4. ht_draw_list_filtered_device of one oriented entry at max_factor 2 (factors (1, 2)): orient first, into the same buffer.
    Step 1's frame is read back after step 2, every later step's result after the step: the routes do not tread on each other."""
    import crop_cases as cr
    import draw_filter_cases as dfc
    import draw_list_cases as dl
    import orient_cases as oc
    from test_gpu_crop import record_tuples
    from test_gpu_orient import Resident, upright_source

    W, H, w, h, P, Q = 40, 30, 34, 18, 20, 11
    scene = np.zeros((H, W, 4), dtype=np.uint8)
    scene[...] = (30, 40, 90, 255)
    scene[9:21, 12:28] = (230, 120, 60, 255)
    host1 = ic.frames_of("noise", w, h, 1, seed=71)
    yuyv, nv12, rgba = oc.source(y4.YUYV, w, h, seed=72, matrix=1), oc.source(yc.NV12, w, h, seed=73, matrix=2), oc.source(dl.RGBA, w, h, seed=74)
    ups = [upright_source(yuyv.rgba), upright_source(oc.orient(nv12.rgba, 1)), rgba]  # what the three entries are to the crop: O of each
    streams = [0, 1, 0]
    res, sarr = Resident([yuyv, nv12, rgba]), DeviceArray(scene)
    out = DeviceArray(np.full(3 * P * Q * 4 + 64, GUARD, dtype=np.uint8))
    dst = DeviceArray(np.full(W * H * 4 + 64, GUARD, dtype=np.uint8))
    try:
        with fresh(W, H, 2) as c:
            # the trackers, from frames drawn out of device memory: the staging buffer is not touched yet
            c.draw_list([dict(format="rgba", width=W, height=H, p0=sarr.ptr)] * 2)
            c.camshift_reserve(2)
            c.camshift_init_pairs([(0, 0), (1, 1)], [(12, 9, 16, 12)] * 2)
            objs = [tuple(float(v) for v in cr.obj_of(o)) for o in c.camshift_track_pairs([(0, 0), (1, 1)], calc_angles=True)]
            # 1 and 2, back to back
            c.draw_frames(host1)
            c.camshift_crop_sources_device(out.ptr, streams, [res.entry(yuyv, 0), res.entry(nv12, 1), res.entry(rgba, 0)], P, Q)
            rec = c.camshift_crop_result(3)
            c.synchronize()
            got = d2h(out.ptr, out.nbytes)
            bound_equals(c, ic.expected(host1[0], None, W, H)[None], "step 1: the host RGBA frame, read after step 2 grew its staging buffer")
            want = [cr.record(st, objs[st], W, H, up.w, up.h, None, 256, 0, P, Q) for up, st in zip(ups, streams)]
            assert record_tuples(rec) == want and all(r[0] == cr.FACE for r in want), (record_tuples(rec), want)
            for i, (up, st) in enumerate(zip(ups, streams)):
                same(got[i * P * Q * 4:(i + 1) * P * Q * 4].reshape(Q, P, 4), cr.patch(up, objs[st], W, H, None, 256, 0, P, Q), f"step 2: entry {i}")
            assert (got[3 * P * Q * 4:] == GUARD).all()
            # 3: the host YUV forms, odd x odd
            for fmt, matrix in ((yc.I420, 3), (yc.NV12, 0)):
                frames = yc.from_rgb_frames("noise", 33, 17, 2, fmt, matrix, seed=75 + fmt)
                c.draw_frames_yuv([np.stack([f[k] for f in frames]) for k in range(len(frames[0]))], fmt, matrix)
                bound_equals(c, np.stack([yc.expected(f, 33, 17, fmt, matrix, None, W, H) for f in frames]), f"step 3: host format {fmt} at 33 x 17")
            # 4: the filtered draw orients first
            c.draw_list([res.entry(nv12, 1)], dst=dst.ptr, prefilter=2)
            c.synchronize()
            buf = d2h(dst.ptr, dst.nbytes)
            want4, factors = dfc.expected_rgba(oc.orient(nv12.rgba, 1), None, W, H, 2)
            assert factors == (1, 2), factors
            same(buf[:W * H * 4].reshape(H, W, 4), want4, "step 4: the oriented entry, filtered")
            assert (buf[W * H * 4:] == GUARD).all()
    finally:
        for x in (sarr, out, dst):
            x.free()
        res.free()


# ---- 7: Node -------------------------------------------------------------------------------------------------------------------------------------

def test_node_facade_draws_and_crops_packed_feeds_on_the_device(tmp_path):
    """tests/js/ingest_422_gpu.js on the real addon, ONE child process: ccv.drawFrames of YUYV and UYVY videos (whole frame and a rect),
    ccv.DeviceBatch with sourceFormat and with mixed sources, and cropFeeds on them, against files written here from the restatement"""
    import json
    import os
    import shutil
    import subprocess

    from conftest import ROOT
    from headtrackr_amd import build
    from oracle import ht_oracle as ho

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    case = y4.CASES[0]
    (sw, sh), (w, h), rect, matrix = (case.w, case.h), (case.w, case.h), (21, 13, 60, 50), 2
    picture = tilted_picture(sw, sh)
    job = dict(sw=sw, sh=sh, w=w, h=h, rect=list(rect), dir=str(tmp_path), rgba="rgba.raw", track=[66, 16, 24, 48], videos=[])
    yuyv = y4.from_rgb(picture, y4.YUYV, matrix)
    yy, u, v = y4.unpack(yuyv, sw, sh, y4.YUYV)
    rgba = y4.to_rgba(yuyv, sw, sh, y4.YUYV, matrix)
    rgba.tofile(tmp_path / "rgba.raw")
    for fmt in FMTS:
        name = y4.FORMAT_NAMES[fmt]
        frame = y4.pack(yy, u, v, fmt)  # the same content in the other byte order
        assert np.array_equal(y4.to_rgba(frame, sw, sh, fmt, matrix), rgba)
        frame.tofile(tmp_path / f"video_{name}.bin")
        want = y4.expected(frame, sw, sh, fmt, matrix, None, w, h)
        want.tofile(tmp_path / f"want_{name}.raw")
        y4.expected(frame, sw, sh, fmt, matrix, rect, w, h).tofile(tmp_path / f"want_rect_{name}.raw")
        job["videos"].append(dict(file=f"video_{name}.bin", format=name, matrix=yc.MATRIX_NAMES[matrix], want=f"want_{name}.raw", want_rect=f"want_rect_{name}.raw", wb=ho.whitebalance(want)))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "ingest_422_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ingest_422_gpu: ok" in r.stdout, r.stdout[-2000:]

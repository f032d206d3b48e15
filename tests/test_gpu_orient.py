"""Oriented feeds (an orientation 0..7 in bits 8..10 of a source's format: rotated and mirrored frames) through every call that takes them —
ht_draw_list_device, ht_draw_frames_yuv / _device, ht_draw_list_filtered_device, the ht_camshift_crop_sources_* / align_sources_* calls and
the JavaScript host — against tests/orient_cases.py: the expectation of a call on an oriented source is the expectation of the same call
on the RGBA frame orient(convert(stored), k), built by numpy's rot90 / fliplr, the declared conversion and the oracle's resampler.  Nothing
expected comes from the code under test; every comparison is equality of every byte.  Geometry 97 x 81: two tile columns and six tile rows
of the 64 x 16 tile (four and three of the 32 x 32 one), partial both ways.  On the parent commit every call here is refused as bad format
(or finds no header / module): every test fails."""
import contextlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_filter_cases as dfc
import draw_list_cases as dl
import ingest_cases as ic
import orient_cases as oc
import yuv422_cases as y4
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd.api import Context, HtError, PatchFormat
from hipmem import DeviceArray
from test_gpu_ingest import bound_equals, d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
GUARD_BYTES = 64
DW, DH = 97, 81


@contextlib.contextmanager
def fresh(dw, dh, n=1, options=None):
    c = Context(options=options) if options else Context()
    try:
        c.set_geometry(dw, dh, n)
        yield c
    finally:
        c.close()


class Resident:
    """sources in device memory, every plane in an allocation of its own (a source that appears twice is uploaded once)"""

    def __init__(self, sources):
        self.arrays = {}
        for s in sources:
            if id(s) not in self.arrays:
                self.arrays[id(s)] = [DeviceArray(b) for b in s.plane_buffers()]

    def entry(self, s, k, rect=None):
        return oc.entry(s, [a.ptr for a in self.arrays[id(s)]], k, rect)

    def free(self):
        for planes in self.arrays.values():
            for a in planes:
                a.free()


def draw(c, entries, dw, dh, dstride=None, prefilter=None):
    """draw_list into a guarded caller's buffer -> (frames [n, dh, dw, 4], the whole buffer)"""
    n, fb = len(entries), dw * dh * 4
    dstride = dstride or fb
    dst = DeviceArray(np.full(n * dstride + GUARD_BYTES, dl.GUARD, dtype=np.uint8))
    try:
        c.draw_list(entries, dst=dst.ptr, dst_stride=dstride, prefilter=prefilter)
        c.synchronize()
        buf = d2h(dst.ptr, dst.nbytes)
    finally:
        dst.free()
    return np.stack([buf[i * dstride:i * dstride + fb].reshape(dh, dw, 4) for i in range(n)]), buf


def expected_buffer(wants, dw, dh, dstride):
    fb = dw * dh * 4
    buf = np.full(len(wants) * dstride + GUARD_BYTES, dl.GUARD, dtype=np.uint8)
    for i, w in enumerate(wants):
        buf[i * dstride:i * dstride + fb] = w.reshape(-1)
    return buf


LANES = [None, "orient_lanes=1", "orient_lanes=2"]  # the shipped lane mapping for odd rot, and both forms by name: the same bytes


# ---- 1: one list, every format under every orientation -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", LANES, ids=["shipped", "lanes-x", "lanes-turned"])
def test_every_format_under_every_orientation_in_one_list(options):
    """5 formats x 8 orientations of 37 x 23 sources (odd x odd), a 2 x 2 I420 and a 1 x 5 RGBA source under all eight k; own pitch padding
    and matrix per source, every other entry under an odd-origin rect of O; the destination strided and guarded, every byte compared"""
    plan = oc.list_of_40()
    assert len(plan) == 56 and {(s.fmt, k) for s, k, _ in plan[:40]} == {(f, k) for f in oc.FORMATS for k in oc.ORIENTATIONS}
    assert sum(r is not None for _, _, r in plan[:40]) == 20 and all(r is None or (r[0] % 2 and r[1] % 2) for _, _, r in plan)
    res = Resident([s for s, _, _ in plan])
    dstride = DW * DH * 4 + 52
    try:
        with fresh(DW, DH, 2, options) as c:
            got, buf = draw(c, [res.entry(s, k, r) for s, k, r in plan], DW, DH, dstride)
    finally:
        res.free()
    wants = [oc.expected(s, k, r, DW, DH) for s, k, r in plan]
    for i, (s, k, r) in enumerate(plan):  # per entry first: a failure names the entry
        same(got[i], wants[i], f"entry {i} ({oc.FORMAT_NAMES[s.fmt]} {s.w}x{s.h} k {k} rect {r})")
    same(buf, expected_buffer(wants, DW, DH, dstride), "the whole destination")


# ---- 2: the permutation itself -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", LANES, ids=["shipped", "lanes-x", "lanes-turned"])
def test_one_to_one_draw_is_the_permutation(options):
    """81 x 97 stored under rot 1 and under rot 3 + flip onto the 97 x 81 canvas is O itself, byte for byte, in every format; the same
    orientations at 333 x 217 (a downscale) and 23 x 23 (an upscale) equal the oracle's resampler on O"""
    sources = [oc.source(fmt, 81, 97, seed=200 + f, matrix=f % 4, pad0=4 * (f % 2), content="raw" if fmt != dl.RGBA else "noise") for f, fmt in enumerate(oc.FORMATS)]
    others = [oc.source(yc.NV12, 333, 217, seed=210, matrix=1, pad0=3, pad1=2), oc.source(y4.UYVY, 333, 217, seed=211, matrix=2, pad0=12), oc.source(dl.RGBA, 23, 23, seed=212),
              oc.source(yc.I420, 23, 23, seed=213, matrix=3, pad1=1)]
    plan = [(s, k) for s in sources + others for k in (1, 7)]
    res = Resident(sources + others)
    try:
        with fresh(DW, DH, 2, options) as c:
            got, _ = draw(c, [res.entry(s, k) for s, k in plan], DW, DH)
    finally:
        res.free()
    for i, (s, k) in enumerate(plan):
        what = f"{oc.FORMAT_NAMES[s.fmt]} {s.w}x{s.h} k {k}"
        if (s.w, s.h) == (81, 97):
            same(got[i], oc.orient(s.rgba, k), what + ": 1 : 1 is O")
        same(got[i], oc.expected(s, k, None, DW, DH), what)


# ---- 3: a mixed list, bound --------------------------------------------------------------------------------------------------------------------

def test_mixed_list_in_the_bind_form_feeds_the_pipeline():
    """oriented and plain entries in one list, dst NULL on 40 x 30, n = 5: entry i is bound frame i (read through the pyramid and
    getWhitebalance, as tests/test_gpu_draw_list.py reads them) and ht_frames_bound() == 5; a second, plain list afterwards binds its own"""
    dw, dh = 40, 30
    srcs = [oc.source(dl.RGBA, 23, 23, seed=31, pad0=4, content="smooth"), oc.source(yc.NV12, 37, 23, seed=32, matrix=1, pad1=2), oc.source(y4.YUYV, 37, 23, seed=33, matrix=2),
            oc.source(yc.I420, 23, 23, seed=34, matrix=3, content="smooth"), oc.source(y4.UYVY, 23, 23, seed=35, pad0=8)]
    plan = [(0, 0, None), (1, 3, (1, 1, 22, 36)), (2, 0, (3, 5, 30, 14)), (3, 6, None), (4, 5, None)]
    res = Resident(srcs)
    c = Context()
    try:
        c.set_geometry(dw, dh, 5)
        c.draw_list([res.entry(srcs[i], k, r) for i, k, r in plan])
        want = np.stack([oc.expected(srcs[i], k, r, dw, dh) for i, k, r in plan])
        assert c._lib.ht_frames_bound(c._h) == 5
        bound_equals(c, want, "mixed list, bound")
        c.draw_list([res.entry(srcs[i], 0, None) for i in (3, 0)])
        bound_equals(c, np.stack([oc.expected(srcs[i], 0, None, dw, dh) for i in (3, 0)]), "a plain list afterwards")
    finally:
        c.close()
        res.free()


# ---- 4: the single-source YUV calls ------------------------------------------------------------------------------------------------------------

def test_draw_frames_yuv_host_and_device_forms_under_an_orientation():
    """n = 3 frames a stride with a gap apart, NV12 (37 x 23, odd x odd: its chroma plane at an even address one byte into the slot) under
    k = 5 and YUYV under k = 3, whole and under a rect of O: the device form into a guarded buffer and the host form (bound) equal the
    expectation on O"""
    w, h, n, gap = 37, 23, 3, 148
    for fmt, k, matrix in ((yc.NV12, 5, 1), (y4.YUYV, 3, 2)):
        packed = fmt == y4.YUYV
        srcs = [oc.source(fmt, w, h, seed=300 + 7 * f + fmt, matrix=matrix) for f in range(n)]
        frames = [s.packed() for s in srcs]
        fsz = len(frames[0])
        assert fsz == (y4.frame_bytes(w, h) if packed else w * h + 2 * 19 * 12)
        lead = 0 if packed else 1                      # NV12: Y at an odd address, so that Y + w h (odd) is even
        step = fsz + gap + (0 if packed else 1)        # ... and an even stride
        host = np.full(lead + (n - 1) * step + fsz, dl.PAD, dtype=np.uint8)
        for f, fr in enumerate(frames):
            host[lead + f * step:lead + f * step + fsz] = fr
        ow, oh = oc.oriented_size(k, w, h)
        for rect in (None, (1, 1, ow - 1, oh - 1)):
            want = np.stack([oc.expected(s, k, rect, DW, DH) for s in srcs])
            what = f"{oc.FORMAT_NAMES[fmt]} k {k} rect {rect}"
            arr = DeviceArray(host)
            dst = DeviceArray(np.full(n * DW * DH * 4 + GUARD_BYTES, dl.GUARD, dtype=np.uint8))
            try:
                with fresh(DW, DH, n) as c:
                    y = arr.ptr + lead
                    c.draw_frames_yuv_device(y, None if packed else y + w * h, None, n, w, h, fmt, matrix, stride=step, rect=rect, dst=dst.ptr, orientation=k)
                    c.synchronize()
                    buf = d2h(dst.ptr, dst.nbytes)
            finally:
                arr.free()
                dst.free()
            same(buf[:n * DW * DH * 4].reshape(n, DH, DW, 4), want, what + ": device form")
            assert (buf[n * DW * DH * 4:] == dl.GUARD).all(), what
            with fresh(DW, DH, n) as c:
                c.draw_frames_yuv_ptr(host.ctypes.data + lead, n, w, h, fmt | k << 8, matrix, step, rect)
                assert c._lib.ht_frames_bound(c._h) == n
                bound_equals(c, want, what + ": host form")


# ---- 5: the filtered draw ----------------------------------------------------------------------------------------------------------------------

def test_filtered_draw_orients_first():
    """draw_list(prefilter = 8) of 333 x 217 NV12 under k = 1 and UYVY under k = 6 (whole, and under an odd-origin rect of O), beside a plain
    RGBA entry: tests/draw_filter_cases.py's restatement — the block mean of the fine draw — on O"""
    srcs = [oc.source(yc.NV12, 333, 217, seed=401, matrix=1, pad0=3, pad1=2), oc.source(y4.UYVY, 333, 217, seed=402, matrix=3, pad0=12), oc.source(dl.RGBA, 333, 217, seed=403, pad0=4)]
    plan = [(0, 1, None), (2, 0, None), (1, 6, None), (0, 1, (3, 5, 210, 320)), (1, 6, (3, 5, 326, 208))]
    res = Resident(srcs)
    try:
        with fresh(DW, DH, 2) as c:
            got, buf = draw(c, [res.entry(srcs[i], k, r) for i, k, r in plan], DW, DH, prefilter=8)
    finally:
        res.free()
    factors = []
    for j, (i, k, r) in enumerate(plan):
        want, f = dfc.expected_rgba(oc.orient(srcs[i].rgba, k), r, DW, DH, 8)
        factors.append(f)
        same(got[j], want, f"entry {j} ({oc.FORMAT_NAMES[srcs[i].fmt]} k {k} rect {r}) factors {f}")
    assert factors[0] == (3, 5) and factors[1] == (4, 3) and factors[2] == (4, 3), factors  # O of 217 x 333 is filtered as 217 x 333
    assert (buf[len(plan) * DW * DH * 4:] == dl.GUARD).all()


# ---- 6: the face calls -------------------------------------------------------------------------------------------------------------------------

def picture(w, h):
    """a dark frame with a bright diagonal band and a bright upright block (two blobs for two trackers), nowhere symmetric: every
    orientation of it is another picture"""
    yy, xx = np.mgrid[0:h, 0:w]
    f = np.zeros((h, w, 4), dtype=np.uint8)
    f[..., :3] = (30, 40, 90)
    f[np.abs((xx - 30) - 0.6 * (yy - 40)) < 5] = (230, 120, 60, 255)
    f[20:60, 70:86] = (60, 220, 110, 255)
    f[..., 3] = 255
    return f


def bbox(mask):
    ys, xs = np.nonzero(mask)
    return (int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))


def upright_source(o):
    """the RGBA frame O as a draw_list_cases.Source, so that its patches are crop_cases' / align_cases' like every other"""
    s = dl.Source(dl.RGBA, o.shape[1], o.shape[0], seed=1)
    s.rgba = o
    return s


@pytest.mark.parametrize("fmt_k", [(yc.NV12, 1), (yc.I420, 4), (y4.YUYV, 7)], ids=["nv12-k1", "i420-k4", "yuyv-k7"])
def test_face_calls_on_an_oriented_feed(fmt_k):
    """two trackers on a 97 x 81 feed stored under k and drawn, oriented, onto a canvas of O's size: crop_sources and align_sources — RGBA8,
    one tensor form and the filtered form — with the feed given oriented equal the same call on the RGBA entry of O that this test uploads,
    bytes and records; the RGBA8 forms also equal crop_cases' / align_cases' expectation on O at the device's track objects"""
    from test_gpu_align import record_tuples as align_tuples
    from test_gpu_crop import record_tuples as crop_tuples

    fmt, k = fmt_k
    w, h, P, Q, matrix = 97, 81, 70, 19, 2
    planes = y4.from_rgb(picture(w, h), fmt, matrix) if fmt == y4.YUYV else yc.from_rgb(picture(w, h), fmt, matrix)
    src = oc.source(fmt, w, h, seed=1, matrix=matrix)
    if fmt == y4.YUYV:
        src.frame, src.rgba = planes, y4.to_rgba(planes, w, h, fmt, matrix)
    else:
        src.planes, src.rgba = planes, yc.to_rgba(planes, w, h, fmt, matrix)
    O = oc.orient(src.rgba, k)
    ow, oh = oc.oriented_size(k, w, h)
    up = upright_source(O)
    rects = [bbox(O[..., 1] > 180), bbox((O[..., 0] > 180) & (O[..., 1] < 180))]  # the block, the band: found in O, whatever k made of them
    res = Resident([src])
    rarr = DeviceArray(O)
    oriented = res.entry(src, k)
    plain = dict(format="rgba", width=ow, height=oh, p0=rarr.ptr)
    tfmt = PatchFormat("f16", "chw", "rgb")
    try:
        with fresh(ow, oh, 2) as c:
            c.draw_list([oriented, oriented])
            bound_equals(c, np.stack([O, O]), "the oriented feed drawn onto a canvas of its own size")
            c.camshift_reserve(2)
            c.camshift_init_pairs([(0, 0), (1, 1)], rects)
            objs = c.camshift_track_pairs([(0, 0), (1, 1)], calc_angles=True)
            for kind in ("crop", "align"):
                forms = {"rgba8": (P * Q * 4, lambda o, e, m: getattr(c, f"camshift_{kind}_sources_device")(o, [0, 1], e, P, Q, margin=m)),
                         "f16-chw": (3 * P * Q * 2, lambda o, e, m: getattr(c, f"camshift_{kind}_sources_tensor_device")(o, [0, 1], e, P, Q, tfmt, margin=m)),
                         "filtered": (P * Q * 4, lambda o, e, m: getattr(c, f"camshift_{kind}_sources_filtered_device")(o, [0, 1], e, P, Q, max_factor=4, margin=m))}
                for name, (pb, call) in forms.items():
                    for margin in (1.0, 3.0):
                        got = []
                        for entry in (oriented, plain):
                            out = DeviceArray(np.full(2 * pb + GUARD_BYTES, dl.GUARD, dtype=np.uint8))
                            try:
                                call(out.ptr, [entry, entry], margin)
                                rec = getattr(c, f"camshift_{kind}_result")(2)
                                c.synchronize()
                                got.append((d2h(out.ptr, out.nbytes), rec))
                            finally:
                                out.free()
                        what = f"{kind} {name} margin {margin} {oc.FORMAT_NAMES[fmt]} k {k}"
                        same(got[0][0], got[1][0], what + ": bytes against the RGBA entry of O")
                        assert got[0][1].tobytes() == got[1][1].tobytes(), what + ": records against the RGBA entry of O"
                        assert (got[0][0][2 * pb:] == dl.GUARD).all() and not (got[0][0][:2 * pb] == dl.GUARD).all(), what
                        if name != "rgba8":
                            continue
                        mq8 = int(margin * 256)
                        for s in range(2):
                            patch = got[0][0][s * pb:(s + 1) * pb].reshape(Q, P, 4)
                            if kind == "crop":
                                obj = tuple(float(v) for v in cr.obj_of(objs[s]))
                                same(patch, cr.patch(up, obj, ow, oh, None, mq8, 0, P, Q), what + f": stream {s} against crop_cases on O")
                                assert crop_tuples(got[0][1])[s] == cr.record(s, obj, ow, oh, ow, oh, None, mq8, 0, P, Q), what
                            else:
                                obj = tuple(float(v) for v in al.obj_of(objs[s]))
                                same(patch, al.patch(up, obj, ow, oh, None, mq8, 0, P, Q), what + f": stream {s} against align_cases on O")
                                assert align_tuples(got[0][1])[s] == al.record(s, obj, ow, oh, ow, oh, None, mq8, 0), what
    finally:
        res.free()
        rarr.free()


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_and_write_nothing():
    """a bit from 11 up, a format number that is none under an orientation, a rect inside the stored frame but outside O, a rect beyond O's
    edge: HT_ERR_INVALID naming `entry <i>`, in the plain and in the filtered call; the destination still all 0xA5, the binding as it was;
    the good list draws afterwards"""
    dw, dh = 40, 30
    srcs = [oc.source(dl.RGBA, 23, 23, seed=51), oc.source(yc.NV12, 37, 23, seed=52, matrix=1), oc.source(y4.UYVY, 37, 23, seed=53)]
    res = Resident(srcs)
    fb = dw * dh * 4
    ddst = DeviceArray(np.full(3 * fb + GUARD_BYTES, dl.GUARD, dtype=np.uint8))
    c = Context()
    try:
        c.set_geometry(dw, dh, 3)
        c.upload(np.stack([ic.noise(dw, dh, 60 + j) for j in range(2)]))
        good = [res.entry(srcs[0], 2), res.entry(srcs[1], 1, (0, 0, 23, 37)), res.entry(srcs[2], 7)]

        def refused(entries, index):
            for prefilter in (None, 4):
                with pytest.raises(HtError) as e:
                    c.draw_list(entries, dst=ddst.ptr, prefilter=prefilter)
                assert e.value.status == HT_ERR_INVALID, str(e.value)
                assert f"entry {index}:" in str(e.value), (index, str(e.value))
            c.synchronize()
            assert (d2h(ddst.ptr, ddst.nbytes) == dl.GUARD).all(), index
            assert c._lib.ht_frames_bound(c._h) == 2, index

        bad = [dict(e) for e in good]
        bad[2]["format"], bad[2]["orientation"] = y4.UYVY | 1 << 11, 0          # a bit from 11 up
        refused(bad, 2)
        bad = [dict(e) for e in good]
        bad[0]["format"] = 6                                                     # no format, under orientation 2
        refused(bad, 0)
        bad = [dict(e) for e in good]
        bad[1]["rect"] = (0, 0, 37, 23)                                          # inside the stored 37 x 23, outside O (23 x 37)
        refused(bad, 1)
        bad = [dict(e) for e in good]
        bad[2]["rect"] = (10, 0, 14, 37)                                         # one column beyond O's right edge (O is 23 x 37)
        refused(bad, 2)
        with pytest.raises(HtError) as e:
            c.draw_frames_yuv_device(res.arrays[id(srcs[2])][0].ptr, None, None, 1, 37, 23, y4.UYVY, 0, rect=(0, 0, 37, 23), dst=ddst.ptr, orientation=7)
        assert e.value.status == HT_ERR_INVALID and "oriented" in str(e.value), str(e.value)
        c.synchronize()
        assert (d2h(ddst.ptr, ddst.nbytes) == dl.GUARD).all()
        c.draw_list(good, dst=ddst.ptr)
        c.synchronize()
        wants = [oc.expected(srcs[0], 2, None, dw, dh), oc.expected(srcs[1], 1, (0, 0, 23, 37), dw, dh), oc.expected(srcs[2], 7, None, dw, dh)]
        same(d2h(ddst.ptr, ddst.nbytes), expected_buffer(wants, dw, dh, fb), "after the refusals")
    finally:
        c.close()
        res.free()
        ddst.free()


# ---- 8: Node -----------------------------------------------------------------------------------------------------------------------------------

def test_node_facade_draws_oriented_feeds_on_the_device(tmp_path):
    """tests/js/orient_gpu.js on the real addon, ONE child process: ccv.drawFrames of an oriented NV12 video under a rect of O, and a
    ccv.DeviceBatch whose opts.sources carry `orientation` (YUYV under rot 1, RGBA under flip, I420 under rot 3 + flip and a rect)"""
    from headtrackr_amd import build

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    dw, dh = 160, 120
    video = oc.source(yc.NV12, 333, 217, seed=81, matrix=1, content="smooth")
    vk, vrect = 3, (3, 5, 200, 300)
    video.packed().tofile(tmp_path / "video.raw")
    oc.expected(video, vk, vrect, dw, dh).tofile(tmp_path / "video_want.raw")
    job = dict(w=dw, h=dh, dir=str(tmp_path), feeds=[],
               video=dict(file="video.raw", want="video_want.raw", width=video.w, height=video.h, format="nv12", matrix=yc.MATRIX_NAMES[1], orientation=vk, rect=list(vrect)))
    feeds = [(oc.source(y4.YUYV, 333, 217, seed=82, matrix=2, content="smooth"), 1, None), (oc.source(dl.RGBA, 320, 240, seed=83, content="smooth"), 4, (21, 13, 280, 190)),
             (oc.source(yc.I420, 23, 37, seed=84, matrix=3), 7, (1, 1, 35, 21))]
    for j, (s, k, rect) in enumerate(feeds):
        s.packed().tofile(tmp_path / f"feed{j}.raw")
        oc.expected(s, k, rect, dw, dh).tofile(tmp_path / f"want{j}.raw")
        job["feeds"].append(dict(file=f"feed{j}.raw", want=f"want{j}.raw", width=s.w, height=s.h, format=oc.FORMAT_NAMES[s.fmt], matrix=yc.MATRIX_NAMES[s.matrix], orientation=k,
                                 rect=list(rect) if rect else None))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "orient_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "orient_gpu: ok" in r.stdout, r.stdout[-2000:]


# ---- 9: without the module ---------------------------------------------------------------------------------------------------------------------

def test_without_the_module_only_the_oriented_calls_fail(tmp_path):
    """a fresh child process on a COPY of the library in a directory without the .hsaco (HEADTRACKR_HIP_LIB): a plain draw_list works, an
    oriented one is HT_ERR_STATE with the module's path in ht_last_error (tests/orient_missing_module_job.py)"""
    from headtrackr_amd import build

    lib = str(tmp_path / "libheadtrackr_hip.so")
    shutil.copy(build.LIB, lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "orient_missing_module_job.py")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HEADTRACKR_HIP_LIB=lib))
    assert r.returncode == 0 and r.stdout.strip().endswith("OK missing module"), (r.returncode, r.stdout[-1500:], r.stderr[-3000:])

"""The model-input tensors on the device — ht_camshift_crop_pairs_tensor_device / ht_camshift_crop_sources_tensor_device /
ht_camshift_align_pairs_tensor_device / ht_camshift_align_sources_tensor_device — against tests/patch_tensor_cases.py.  The track objects
are the ORACLE's, the RGBA8 patch is the Python restatement of the crop / align rule (tests/crop_cases.py, tests/align_cases.py) and the
tensor is the restated f of that patch: nothing expected comes from the code under test, and every comparison is equality of every byte,
padding and the 64-byte guard included.  The precondition of each test is the existing tests' own: the device tracked what the oracle
tracked, and (align) its angle quantises to an admissible a12.  Without the feature every test fails at its first tensor call."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_list_cases as dl
import patch_tensor_cases as pt
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError, PatchFormat
from test_gpu_align import objects_agree
from test_gpu_align import record_tuples as align_tuples
from test_gpu_crop import CROP_LIST, ResidentFeeds, canvas_source, expected_buffer, guarded, oracle_step, start_pairs
from test_gpu_crop import record_tuples as crop_tuples
from test_gpu_ingest import d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
W, H = cr.CANVAS
SIZES = [(70, 19), (7, 3), (1, 1)]  # partial tiles both ways and an even width; odd width and odd plane (16-bit planes 2-byte aligned); one pixel
CONFIGS = [(64, 0), (1024, 0), (64, cr.SQUARE), (1024, cr.SQUARE)]
NO_BOX = (0.0, 0.0, 0.0, 0.0)
# all 18 formats under 2/255, -1; the tie, overflow and subnormal pairs at f16 / bf16 CHW
FORMAT_PAIRS = [(fmt, "signed") for fmt in pt.FORMATS] + [((d, "chw", "rgb"), name) for name in pt.ROUNDING_PAIRS for d in ("f16", "bf16")]


def fmt_of(fmt, pair):
    return PatchFormat(fmt[0], fmt[1], fmt[2], scale=pair[0][:pt.nchannels(fmt[2])], bias=pair[1][:pt.nchannels(fmt[2])])


class Kind:
    """the crop calls or the align calls: the RGBA call, the tensor call, the records and the restatement of each"""

    def __init__(self, name):
        self.name = name
        self.crop = name == "crop"

    def rgba_pairs(self, c, ptr, pairs, P, Q, margin, flags, stride=0):
        (c.camshift_crop_pairs_device if self.crop else c.camshift_align_pairs_device)(ptr, pairs, P, Q, margin=margin / 256, square=bool(flags), stride=stride)

    def tensor_pairs(self, c, ptr, pairs, P, Q, fmt, margin, flags, stride=0):
        (c.camshift_crop_pairs_tensor_device if self.crop else c.camshift_align_pairs_tensor_device)(ptr, pairs, P, Q, fmt, margin=margin / 256, square=bool(flags), stride=stride)

    def rgba_sources(self, c, ptr, streams, entries, P, Q, margin, flags):
        (c.camshift_crop_sources_device if self.crop else c.camshift_align_sources_device)(ptr, streams, entries, P, Q, margin=margin / 256, square=bool(flags))

    def tensor_sources(self, c, ptr, streams, entries, P, Q, fmt, margin, flags):
        (c.camshift_crop_sources_tensor_device if self.crop else c.camshift_align_sources_tensor_device)(ptr, streams, entries, P, Q, fmt, margin=margin / 256, square=bool(flags))

    def result(self, c, n):
        return c.camshift_crop_result(n) if self.crop else c.camshift_align_result(n)

    def tuples(self, rec):
        return crop_tuples(rec) if self.crop else align_tuples(rec)

    def obj(self, to, angle=None):
        if to is None:
            return NO_BOX if self.crop else al.NO_OBJECT
        if self.crop:
            return cr.obj_of(to)
        return al.obj_of(to) if angle is None else al.obj_tracked(to, angle)

    def patch(self, source, obj, mapping, margin, flags, P, Q):
        return (cr.patch if self.crop else al.patch)(source, obj, W, H, mapping, margin, flags, P, Q)

    def record(self, stream, obj, SW, SH, mapping, margin, flags, P, Q):
        if self.crop:
            return cr.record(stream, obj, W, H, SW, SH, mapping, margin, flags, P, Q)
        return al.record(stream, obj, W, H, SW, SH, mapping, margin, flags)


KINDS = {"crop": Kind("crop"), "align": Kind("align")}


def tensors(patches, fmt, pair):
    return [pt.f(p, fmt, pair) for p in patches]


@pytest.fixture(scope="module")
def pairs_ctx():
    """one context that has tracked step 1 of the pairs scene on two bound frames; every pairs-form test reads it"""
    a, b = cr.pairs_scene()
    c = Context()
    c.set_geometry(W, H, 2)
    c.upload(np.stack([a.frames[0], b.frames[0]]))
    pairs = start_pairs(c)
    c.upload(np.stack([a.frames[1], b.frames[1]]))
    got = c.camshift_track_pairs(pairs)
    want = oracle_step(1)
    objects_agree(got, [want[s] for s, _f in pairs], "pairs scene, step 1")
    yield c, want, [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
    c.close()


# ---- 1: the pairs form ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", ["crop", "align"])
def test_pairs_form_every_byte_of_every_format(pairs_ctx, kind, size):
    """the 97 x 81 pairs scene and CROP_LIST (FACE entries, both EMPTY kinds, one stream twice) -> 70 x 19, 7 x 3 and 1 x 1; margins 64 and
    1024, square on and off; all 18 formats under (2 / 255, -1) and the tie, overflow and subnormal pairs at f16 / bf16 CHW; a strided
    output (a patch's bytes rounded up to 4, + 52).  Expected: f of the restated patch; the records are the restated records AND those of
    the RGBA call issued just before on the same state.  Align at 1024 keeps out-of-frame pixels in play: at least two patches contain
    some (70 x 19 and 7 x 3; the one pixel of a 1 x 1 patch is the box's centre and lies inside)."""
    c, objs, sources = pairs_ctx
    k = KINDS[kind]
    P, Q = size
    n = len(CROP_LIST)
    outside = 0
    for (margin, flags) in CONFIGS:
        obj = [k.obj(objs.get(s)) for s, _f in CROP_LIST]
        patches = [k.patch(sources[f], o, None, margin, flags, P, Q) for o, (_s, f) in zip(obj, CROP_LIST)]
        want_rec = [k.record(s, o, W, H, None, margin, flags, P, Q) for o, (s, _f) in zip(obj, CROP_LIST)]
        assert [r[0] for r in want_rec] == [1, 0, 1, 1, 0, 1]
        rgba = guarded(n, P * Q * 4)
        try:
            k.rgba_pairs(c, rgba.ptr, CROP_LIST, P, Q, margin, flags)
            rgba_rec = k.result(c, n).tobytes()
        finally:
            rgba.free()
        if not k.crop:
            outside += sum(int((p[..., 3] == 0).any()) for p, r in zip(patches, want_rec) if r[0] == al.FACE)
        for fmt, name in FORMAT_PAIRS:
            pair = pt.pair_for(name, fmt[2])
            pb = pt.patch_bytes(P, Q, fmt[0], fmt[2])
            stride = pt.default_stride(P, Q, fmt[0], fmt[2]) + 52
            out = guarded(n, stride)
            try:
                k.tensor_pairs(c, out.ptr, CROP_LIST, P, Q, fmt_of(fmt, pair), margin, flags, stride=stride)
                rec = k.result(c, n)
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            want = tensors(patches, fmt, pair)
            where = f"{kind} {fmt} {name} margin {margin} flags {flags} -> {P}x{Q}"
            for i, t in enumerate(want):  # per entry first: a failure names the entry
                assert t.size == pb
                same(got[i * stride:i * stride + pb], t, f"entry {i} {CROP_LIST[i]} {where}")
            same(got, expected_buffer(want, stride), f"the whole output, {where}")
            assert k.tuples(rec) == want_rec, where
            assert rec.tobytes() == rgba_rec, where
    assert k.crop or (P, Q) == (1, 1) or outside >= 2


# ---- 2: structural, not through the restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_tensor_is_f_of_the_rgba_calls_own_bytes(pairs_ctx, kind):
    """on the same state the RGBA call and the tensor call: f applied in numpy to the RGBA call's downloaded bytes equals the tensor
    call's bytes — 70 x 19 and 7 x 3, margin 1024 square, every format under the ImageNet pair"""
    c, _objs, _sources = pairs_ctx
    k = KINDS[kind]
    n = len(CROP_LIST)
    for (P, Q) in ((70, 19), (7, 3)):
        rgba = guarded(n, P * Q * 4)
        try:
            k.rgba_pairs(c, rgba.ptr, CROP_LIST, P, Q, 1024, cr.SQUARE)
            c.synchronize()
            patches = d2h(rgba.ptr, n * P * Q * 4).reshape(n, Q, P, 4)
        finally:
            rgba.free()
        assert patches.any()
        for fmt in pt.FORMATS:
            pair = pt.pair_for("imagenet", fmt[2])
            stride = pt.default_stride(P, Q, fmt[0], fmt[2])
            out = guarded(n, stride)
            try:
                k.tensor_pairs(c, out.ptr, CROP_LIST, P, Q, fmt_of(fmt, pair), 1024, cr.SQUARE)
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            want = expected_buffer(tensors(list(patches), fmt, pair), stride)
            if stride != pt.patch_bytes(P, Q, fmt[0], fmt[2]):  # 7 x 3 at 16 bits: 126 bytes, 2 of padding that stay as they were
                assert stride - pt.patch_bytes(P, Q, fmt[0], fmt[2]) == 2
            same(got, want, f"{kind} {fmt} {P}x{Q}")


# ---- 3: the sources form -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_sources_form_from_a_mixed_list(kind):
    """crop_cases.feeds() — padded RGBA, NV12 under an odd-origin rect, I420 upscaled, the one-pixel-wide sources, every matrix — through
    ResidentFeeds, 24 x 24 and 70 x 19; f16 CHW RGB, bf16 HWC BGR and f32 CHW GRAY"""
    k = KINDS[kind]
    feeds, objs = cr.feeds(), cr.feed_objects()
    n = len(feeds)
    streams = [4, 0, 6, 2, 8, 1, 5]
    res = ResidentFeeds()
    c = Context()
    try:
        c.set_geometry(W, H, n)
        c.draw_list(res.entries())
        c.camshift_reserve(9)
        pairs = [(streams[i], i) for i in range(n)]
        c.camshift_init_pairs(pairs, [cr.canvas_rect_of(i) for i in range(n)])
        tracked = c.camshift_track_pairs(pairs)
        objects_agree(tracked, objs, "feeds")
        obj = [k.obj(to, float(g["angle"])) for to, g in zip(objs, tracked)]
        for (P, Q) in ((24, 24), (70, 19)):
            for (margin, flags) in ((256, 0), (1024, cr.SQUARE)):
                patches = [k.patch(src, o, m, margin, flags, P, Q) for (src, m), o in zip(feeds, obj)]
                want_rec = [k.record(st, o, src.w, src.h, m, margin, flags, P, Q) for (src, m), o, st in zip(feeds, obj, streams)]
                for fmt, name in ((("f16", "chw", "rgb"), "imagenet"), (("bf16", "hwc", "bgr"), "signed"), (("f32", "chw", "gray"), "unit")):
                    pair = pt.pair_for(name, fmt[2])
                    stride = pt.default_stride(P, Q, fmt[0], fmt[2])
                    out = guarded(n, stride)
                    try:
                        k.tensor_sources(c, out.ptr, streams, res.entries(), P, Q, fmt_of(fmt, pair), margin, flags)
                        rec = k.result(c, n)
                        c.synchronize()
                        got = d2h(out.ptr, out.nbytes)
                    finally:
                        out.free()
                    want = tensors(patches, fmt, pair)
                    for i, t in enumerate(want):
                        same(got[i * stride:i * stride + t.size], t, f"{kind} feed {i} ({dl.FORMAT_NAMES[feeds[i][0].fmt]}) {fmt} margin {margin} flags {flags} -> {P}x{Q}")
                    same(got, expected_buffer(want, stride), f"the whole output, {kind} {fmt} margin {margin} flags {flags} -> {P}x{Q}")
                    assert k.tuples(rec) == want_rec, (kind, fmt, margin, flags, P, Q)
    finally:
        c.close()
        res.free()


# ---- 4: into a torch tensor --------------------------------------------------------------------------------------------------------------------

def test_into_a_torch_tensor():
    """tests/patch_tensor_torch_job.py in a process of its own, because torch must be imported BEFORE the library there (torch brings a HIP
    runtime of its own and cannot initialise behind another): empty_patches(n, 24, 24, fmt, "cuda") for f16 CHW and bf16 HWC, filled
    through the wrappers; after synchronize() the tensor's bits are the restatement's; a non-contiguous, wrong-dtype or short tensor is
    refused and nothing is written"""
    if importlib.util.find_spec("torch") is None:  # (not imported here: this process has loaded the library's HIP runtime already)
        pytest.skip("torch is not installed")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "patch_tensor_torch_job.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK 4 tensors"), (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


# ---- 5: the tensor calls leave everything else as it is ------------------------------------------------------------------------------------------

def test_tensor_calls_leave_the_trackers_and_the_rgba_calls_of_the_same_step_as_they_are():
    """a twin context without tensor calls returns the same track objects, histograms and statistics on the following step — the oracle's —,
    and a crop call and an align call of the same step, issued among the tensor calls, give the bytes and records they give alone"""
    a, b = cr.pairs_scene()
    res = ResidentFeeds()
    ctxs = [Context(), Context()]
    n = len(CROP_LIST)
    pb = 70 * 19 * 4
    fmt = PatchFormat.mean_std(pt.IMAGENET_MEAN, pt.IMAGENET_STD)
    outs = [guarded(n + 1, 112 * 112 * 6), guarded(n, pb), guarded(n, pb), guarded(n, pb), guarded(n, pb)]
    try:
        results, rgba = [], []
        for with_tensor, c, crop_out, align_out in zip((True, False), ctxs, outs[1:3], outs[3:5]):
            c.set_geometry(W, H, 2)
            c.upload(np.stack([a.frames[0], b.frames[0]]))
            pairs = start_pairs(c)
            c.camshift_stats(cr.RESERVED, reset=True)
            c.upload(np.stack([a.frames[1], b.frames[1]]))
            c.camshift_track_pairs(pairs, fetch=False)
            if with_tensor:
                c.camshift_align_pairs_tensor_device(outs[0].ptr, CROP_LIST, 112, 112, fmt, margin=4.0, square=True)
            c.camshift_crop_pairs_device(crop_out.ptr, CROP_LIST, 70, 19)
            crop_rec = c.camshift_crop_result(n).tobytes()
            if with_tensor:
                c.camshift_crop_sources_tensor_device(outs[0].ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 70, 19, dict(dtype="f32", layout="hwc", channels="bgr"))
                assert len(c.camshift_crop_result(7)) == 7
            c.camshift_align_pairs_device(align_out.ptr, CROP_LIST, 70, 19)
            align_rec = c.camshift_align_result(n).tobytes()
            if with_tensor:
                c.camshift_align_sources_tensor_device(outs[0].ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 7, 3, dict(dtype="bf16", layout="chw", channels="gray", scale=1.0))
                c.camshift_crop_pairs_tensor_device(outs[0].ptr, CROP_LIST, 1, 1, fmt)
            first = c.camshift_track_collect(3)
            c.synchronize()
            rgba.append((crop_rec, align_rec, d2h(crop_out.ptr, crop_out.nbytes).tobytes(), d2h(align_out.ptr, align_out.nbytes).tobytes()))
            c.upload(np.stack([a.frames[2], b.frames[2]]))
            second = c.camshift_track_pairs(pairs)
            tracked = {s for s, _f in pairs}
            hists = [c.camshift_debug_hist(s, current=s in tracked) for s in range(cr.RESERVED)]
            results.append((first.tobytes(), second.tobytes(), [(m.tobytes(), h.tobytes()) for m, h in hists], [v.tobytes() for v in c.camshift_stats(cr.RESERVED, reset=False)]))
        objects_agree(np.frombuffer(results[0][1], dtype=native.CS_TRACKOBJ_DTYPE), [oracle_step(2)[s] for s, _f in pairs], "step 2 behind the tensor calls")
        assert results[0] == results[1]
        assert rgba[0] == rgba[1]
        objs = oracle_step(1)
        srcs = [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
        want = [cr.patch(srcs[f], cr.obj_of(objs[s]) if s in objs else NO_BOX, W, H, None, 256, 0, 70, 19) for s, f in CROP_LIST]
        same(np.frombuffer(rgba[0][2], dtype=np.uint8), expected_buffer(want, pb), "the crop call among the tensor calls")
    finally:
        for c in ctxs:
            c.close()
        res.free()
        for o in outs:
            o.free()


# ---- 6: refusals change nothing ------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pairs_ctx):
    """every format refusal, a NULL format, a misaligned or NULL output, a stride that is no multiple of 4 or shorter than a patch, and a
    source plane that overlaps the TENSOR's byte range at an offset an RGBA patch list of the same call would not reach: the status, the
    words, the guarded output still all 0xA5 and the previous call's records unchanged"""
    c, _objs, _sources = pairs_ctx
    L, h = c._lib, c._h
    P, Q = 7, 3
    n = len(CROP_LIST)
    res = ResidentFeeds()
    out = guarded(8, P * Q * 4)
    fill = guarded(8, P * Q * 12)
    try:
        entries = res.entries()
        srcs = c._draw_sources(entries)
        streams7 = np.array([5, 0, 2, 4, 3, 5, 0], dtype=np.int32)
        pairs6 = c._pairs(CROP_LIST)
        good = pt.pack_format(1, 0, 0, 0, *pt.PAIRS["signed"])
        pb16 = pt.patch_bytes(P, Q, "f16", "rgb")
        assert pb16 == 126 and pt.default_stride(P, Q, "f16", "rgb") == 128
        nan, inf = float("nan"), float("inf")
        z3, one3 = (0.0,) * 3, (1.0,) * 3
        bad_formats = [pt.pack_format(3, 0, 0, 0, one3, z3), pt.pack_format(-1, 0, 0, 0, one3, z3), pt.pack_format(0, 2, 0, 0, one3, z3), pt.pack_format(0, 0, 3, 0, one3, z3),
                       pt.pack_format(0, 0, 0, 1, one3, z3), pt.pack_format(1, 0, 0, 0, (1.0, nan, 1.0), z3), pt.pack_format(1, 0, 0, 0, one3, (0.0, 0.0, inf)),
                       pt.pack_format(1, 0, 0, 0, (2.0 ** -65, 1.0, 1.0), z3), pt.pack_format(1, 0, 0, 0, one3, (-(2.0 ** 65), 0.0, 0.0)),
                       pt.pack_format(1, 0, 2, 0, (1.0, 1.0, 0.0), z3), pt.pack_format(1, 0, 2, 0, (1.0, 0.0, 0.0), (0.0, 0.0, 0.5))]
        for kind in ("crop", "align"):
            k = KINDS[kind]
            k.rgba_pairs(c, out.ptr, CROP_LIST, P, Q, 256, 0)
            before = k.result(c, n).tobytes()
            c.synchronize()
            prm_t = native.CROP_PARAMS if k.crop else native.ALIGN_PARAMS
            fn_pairs = L.ht_camshift_crop_pairs_tensor_device if k.crop else L.ht_camshift_align_pairs_tensor_device
            fn_sources = L.ht_camshift_crop_sources_tensor_device if k.crop else L.ht_camshift_align_sources_tensor_device

            def refused(call, status, index=None, text=None):
                with pytest.raises(HtError) as e:
                    call()
                assert e.value.status == status, str(e.value)
                if index is not None:
                    assert f"entry {index}:" in str(e.value), (index, str(e.value))
                if text is not None:
                    assert text in str(e.value), (text, str(e.value))
                c.synchronize()
                assert (d2h(fill.ptr, fill.nbytes) == dl.GUARD).all(), str(e.value)
                assert k.result(c, n).tobytes() == before, str(e.value)

            def pairs_call(fmt=good, ptr=fill.ptr, stride=0):
                p = prm_t(P, Q, 256, 0)
                f = native.PATCH_FORMAT.from_buffer_copy(fmt) if fmt is not None else None
                return lambda: c._check(fn_pairs(h, pairs6.ctypes.data, len(pairs6), C.byref(p), C.byref(f) if f is not None else None, ptr, stride))

            def sources_call(arr=srcs, fmt=good, ptr=fill.ptr, stride=0):
                p = prm_t(P, Q, 256, 0)
                f = native.PATCH_FORMAT.from_buffer_copy(fmt) if fmt is not None else None
                return lambda: c._check(fn_sources(h, streams7.ctypes.data, arr, 7, C.byref(p), C.byref(f) if f is not None else None, ptr, stride))

            for call in (pairs_call, sources_call):
                for bf in bad_formats:
                    refused(call(fmt=bf), HT_ERR_INVALID, text="format")
                refused(call(fmt=None), HT_ERR_INVALID, text="NULL format")
                refused(call(ptr=fill.ptr + 2), HT_ERR_INVALID)       # misaligned
                refused(call(ptr=None), HT_ERR_INVALID)               # no output
                refused(call(stride=pb16), HT_ERR_INVALID)            # 126: a patch's bytes, but no multiple of 4
                refused(call(stride=pb16 - 2), HT_ERR_INVALID)        # 124: a multiple of 4, shorter than a patch
            # the tensor's own byte range: 7 patches 128 bytes apart end at byte 894; an RGBA list of this call would end at 7 x 84 = 588
            e = [dict(x) for x in entries]
            e[2]["p1"] = fill.ptr + 893                               # entry 2's U plane begins on the range's last byte
            refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 2, "overlap")
    finally:
        res.free()
        out.free()
        fill.free()

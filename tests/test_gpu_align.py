"""The angle-aligned face crops on the device — ht_camshift_align_pairs_device / ht_camshift_align_sources_device /
ht_camshift_align_result — against tests/align_cases.py.  The track objects are the ORACLE's (ho.Camshift on crop_cases' scenes), the
affine terms and the patch are the Python restatement of the rule on the source's declared RGBA view.  Nothing expected comes from the
code under test; every comparison is equality of every byte and of every record field.  The precondition of each test: the device tracked
what the oracle tracked in x, y, width and height, and its angle quantises to the oracle's a12 (tests/test_align_cpu.py proves from the
oracle alone that these angles are far from every rounding boundary; at the two strip feeds, whose blobs are horizontal to rounding, the
oracle's own angle is 0 or pi depending on its summation order, and the device's must round to one of those two steps).  Without the feature every test fails at its first align call."""
import ctypes as C
import math

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_list_cases as dl
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_crop import CROP_LIST, ResidentFeeds, canvas_source, expected_buffer, guarded, oracle_step, start_pairs
from test_gpu_ingest import d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
W, H = cr.CANVAS
FIELDS = ("code", "stream", "a12", "pad", "cx", "cy", "ux", "uy", "vx", "vy")


def record_tuples(rec):
    return [tuple(int(r[f]) for f in FIELDS) for r in rec]


def objects_agree(got, want, where):
    """precondition of the byte comparisons: the device tracked what the oracle tracked, and its angle rounds to the same step"""
    for g, to in zip(got, want):
        assert (float(g["x"]), float(g["y"]), float(g["width"]), float(g["height"])) == cr.obj_of(to), (where, g, to)
        assert al.a12_of(float(g["angle"])) in al.admissible_a12(to["angle"]), (where, float(g["angle"]), to["angle"])


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


# ---- 1: the pairs form -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", cr.SIZES)
def test_pairs_form_every_output_byte_and_every_record_field(pairs_ctx, size):
    """97 x 81 canvas, 3 trackers on 2 bound frames (a12 on both sides of upright), a stream that was initialised but never tracked and one
    that was never initialised (both EMPTY: zeros), one stream twice; outputs 70 x 19 (partial tiles both ways), 1 x 1 and 112 x 112;
    margins 64 / 256 / 1024, square on and off.  The strided output is compared whole — padding between the patches and the 64-byte guard
    included — and the records field by field."""
    c, objs, sources = pairs_ctx
    P, Q = size
    pb = P * Q * 4
    outside = 0
    for (margin, flags) in cr.CONFIGS:
        stride = pb + 52
        out = guarded(len(CROP_LIST), stride)
        try:
            c.camshift_align_pairs_device(out.ptr, CROP_LIST, P, Q, margin=margin / 256, square=bool(flags), stride=stride)
            rec = c.camshift_align_result(len(CROP_LIST))
            c.synchronize()
            got = d2h(out.ptr, out.nbytes)
        finally:
            out.free()
        obj = [al.obj_of(objs[s]) if s in objs else al.NO_OBJECT for s, _f in CROP_LIST]
        patches = [al.patch(sources[f], o, W, H, None, margin, flags, P, Q) for o, (_s, f) in zip(obj, CROP_LIST)]
        for i, p in enumerate(patches):  # per entry first: a failure names the entry
            same(got[i * stride:i * stride + pb].reshape(Q, P, 4), p, f"entry {i} {CROP_LIST[i]} margin {margin} flags {flags} -> {P}x{Q}")
        same(got, expected_buffer(patches, stride), f"the whole output, margin {margin} flags {flags}")
        want = [al.record(s, o, W, H, W, H, None, margin, flags) for o, (s, _f) in zip(obj, CROP_LIST)]
        assert record_tuples(rec) == want, (margin, flags, record_tuples(rec), want)
        assert [r[0] for r in want] == [al.FACE, al.EMPTY, al.FACE, al.FACE, al.EMPTY, al.FACE]
        outside += sum(int((p[..., 3] == 0).any()) for p, r in zip(patches, want) if r[0] == al.FACE)
    assert (P, Q) == (1, 1) or outside >= 2  # a wide margin takes the corner blobs' patches out of the frame: both branches of the range test


# ---- 2: the sources form ---------------------------------------------------------------------------------------------------------------------

def test_sources_form_from_a_mixed_list_every_matrix():
    """the canvases are drawn with ht_draw_list_device from crop_cases.feeds() — a padded RGBA 333 x 217, an NV12 333 x 217 under an
    odd-origin mapping rect, an I420 23 x 23 that the canvas upscales, both YUV allocations again under other rects and matrices, an RGBA
    and an NV12 source one pixel wide —, initialised and tracked on those canvases, then aligned from the SAME sources: tilts on both
    sides of upright and a12 = 2048; 70 x 19 and 24 x 24; all configs"""
    feeds, objs = cr.feeds(), cr.feed_objects()
    n = len(feeds)
    streams = [4, 0, 6, 2, 8, 1, 5]
    res = ResidentFeeds()
    c = Context()
    inside = set()
    try:
        c.set_geometry(W, H, n)
        c.draw_list(res.entries())  # bound: frame k = feed k's canvas
        c.camshift_reserve(9)
        pairs = [(streams[k], k) for k in range(n)]
        c.camshift_init_pairs(pairs, [cr.canvas_rect_of(k) for k in range(n)])
        tracked = c.camshift_track_pairs(pairs)
        objects_agree(tracked, objs, "feeds")
        obj5 = [al.obj_tracked(to, float(g["angle"])) for to, g in zip(objs, tracked)]  # (differs from the oracle's own at the strip feeds' wrap only)
        for (P, Q) in ((70, 19), (24, 24)):
            pb = P * Q * 4
            for (margin, flags) in cr.CONFIGS:
                out = guarded(n, pb)
                try:
                    c.camshift_align_sources_device(out.ptr, streams, res.entries(), P, Q, margin=margin / 256, square=bool(flags))
                    rec = c.camshift_align_result(n)
                    c.synchronize()
                    got = d2h(out.ptr, out.nbytes)
                finally:
                    out.free()
                patches = [al.patch(src, o, W, H, m, margin, flags, P, Q) for (src, m), o in zip(feeds, obj5)]
                for i, p in enumerate(patches):
                    same(got[i * pb:(i + 1) * pb].reshape(Q, P, 4), p, f"feed {i} ({dl.FORMAT_NAMES[feeds[i][0].fmt]} {feeds[i][0].w}x{feeds[i][0].h}) margin {margin} flags {flags} -> {P}x{Q}")
                same(got, expected_buffer(patches, pb), f"the whole output, margin {margin} flags {flags} -> {P}x{Q}")
                want = [al.record(st, o, W, H, src.w, src.h, m, margin, flags) for (src, m), o, st in zip(feeds, obj5, streams)]
                assert record_tuples(rec) == want, (margin, flags, P, Q)
                inside |= {(margin, flags, bool((p[..., 3] == 0).any())) for p in patches}
        ptr, cnt = c.camshift_align_records_ptr()
        assert cnt == n and record_tuples(np.frombuffer(d2h(ptr, 64 * n).tobytes(), dtype=native.ALIGN_RECORD_DTYPE)) == want  # the device's copy of the last call's records
    finally:
        c.close()
        res.free()
    assert [r[2] for r in want][:5] == [689, 1015, 1396, 976, 1347] and {r[2] for r in want[5:]} <= {0, 2048}  # tilts on both sides of upright; an exact quarter turn
    assert (256, 0, False) in inside and (1024, al.SQUARE, True) in inside


# ---- 3: upright identity on the device ---------------------------------------------------------------------------------------------------------

def test_upright_identity_is_the_bound_frames_block():
    """a structural check that does not pass through the restatement: one step tracked with calc_angles = 0 leaves angle == pi / 2 exactly;
    with P, Q = the object's width, height (multiples of 4) and margin 256 the aligned patch is the bound frame's block
    [cx - w / 2, cx + w / 2) x [cy - h / 2, cy + h / 2) itself, byte for byte, with zeros where the block leaves the frame"""
    a, b = cr.pairs_scene()
    seqs = (a, b)
    c = Context()
    try:
        c.set_geometry(W, H, 2)
        c.upload(np.stack([a.frames[0], b.frames[0]]))
        pairs = start_pairs(c)
        c.upload(np.stack([a.frames[1], b.frames[1]]))
        got = c.camshift_track_pairs(pairs, calc_angles=False)
        for g, (s, f, q, j) in zip(got, cr.pairs_trackers()):
            o = ho.Camshift(False)
            o.init_tracker(seqs[q].frames[0], seqs[q].rects[j])
            _sw, to = o.track(seqs[q].frames[1])
            assert (float(g["x"]), float(g["y"]), float(g["width"]), float(g["height"])) == cr.obj_of(to) and float(g["angle"]) == math.pi / 2 == to["angle"], (g, to)
            cx, cy, w, h = (int(v) for v in cr.obj_of(to))
            assert w > 0 and h > 0 and w % 4 == 0 and h % 4 == 0
            out = guarded(1, w * h * 4)
            try:
                c.camshift_align_pairs_device(out.ptr, [(s, f)], w, h)
                rec = c.camshift_align_result(1)
                c.synchronize()
                patch = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            padded = np.zeros((H + 2 * 128, W + 2 * 128, 4), dtype=np.uint8)
            padded[128:128 + H, 128:128 + W] = seqs[q].frames[1]
            block = padded[128 + cy - h // 2:128 + cy + h // 2, 128 + cx - w // 2:128 + cx + w // 2]
            same(patch, expected_buffer([block], w * h * 4), f"stream {s}: the block {w}x{h} around ({cx}, {cy})")
            assert record_tuples(rec) == [(al.FACE, s, 1024, 0, cx * 65536, cy * 65536, w * 65536, 0, 0, h * 65536)]
    finally:
        c.close()


# ---- 4: the largest coordinates ----------------------------------------------------------------------------------------------------------------

def test_a_source_of_16384_by_2(pairs_ctx):
    """a 128 KB RGBA source 16384 x 2 paired with tracked streams (the sources form does not require that the canvas was drawn from it): the
    largest Q16 coordinates the kernel forms, one x step of the canvas is 169 source pixels and the two rows are all there is in y"""
    c, objs, _sources = pairs_ctx
    src = dl.Source(dl.RGBA, 16384, 2, seed=77)
    buf = DeviceArray(src.plane_buffers()[0])
    streams = [5, 0, 2, cr.NEVER_TRACKED]
    entries = [src.entry([buf.ptr], None)] * len(streams)
    try:
        for (P, Q, margin, flags) in ((70, 19, 256, 0), (112, 112, 1024, al.SQUARE), (1024, 3, 64, 0)):
            pb = P * Q * 4
            out = guarded(len(streams), pb)
            try:
                c.camshift_align_sources_device(out.ptr, streams, entries, P, Q, margin=margin / 256, square=bool(flags))
                rec = c.camshift_align_result(len(streams))
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            obj = [al.obj_of(objs[s]) if s in objs else al.NO_OBJECT for s in streams]
            patches = [al.patch(src, o, W, H, None, margin, flags, P, Q) for o in obj]
            same(got, expected_buffer(patches, pb), f"16384 x 2, margin {margin} flags {flags} -> {P}x{Q}")
            want = [al.record(s, o, W, H, 16384, 2, None, margin, flags) for s, o in zip(streams, obj)]
            assert record_tuples(rec) == want
            assert max(r[4] for r in want) > 8000 * 65536 and any(p.any() for p in patches)
    finally:
        buf.free()


# ---- 5: enqueue-only, no tracker state is touched ----------------------------------------------------------------------------------------------

def test_align_calls_leave_the_trackers_and_a_crop_call_of_the_same_step_as_they_are():
    """a twin context without align calls returns the same track objects, histograms and statistics on the following step; a crop call
    issued between two align calls of the same step gives the bytes and records of a crop call alone"""
    a, b = cr.pairs_scene()
    res = ResidentFeeds()
    ctxs = [Context(), Context()]
    n = len(CROP_LIST)
    pb = 70 * 19 * 4
    outs = [guarded(n, 112 * 112 * 4), guarded(n, pb), guarded(n, pb)]
    try:
        results, crops = [], []
        for with_align, c, crop_out in zip((True, False), ctxs, outs[1:]):
            c.set_geometry(W, H, 2)
            c.upload(np.stack([a.frames[0], b.frames[0]]))
            pairs = start_pairs(c)
            c.camshift_stats(cr.RESERVED, reset=True)
            c.upload(np.stack([a.frames[1], b.frames[1]]))
            first = c.camshift_track_pairs(pairs, fetch=False)
            if with_align:
                c.camshift_align_pairs_device(outs[0].ptr, CROP_LIST, 112, 112, margin=4.0, square=True)
            c.camshift_crop_pairs_device(crop_out.ptr, CROP_LIST, 70, 19)
            if with_align:
                c.camshift_align_sources_device(outs[0].ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 70, 19)
                assert len(c.camshift_align_result(7)) == 7
            first = c.camshift_track_collect(3)
            c.synchronize()
            crops.append((c.camshift_crop_result(n).tobytes(), d2h(crop_out.ptr, crop_out.nbytes).tobytes()))
            c.upload(np.stack([a.frames[2], b.frames[2]]))
            second = c.camshift_track_pairs(pairs)
            tracked = {s for s, _f in pairs}
            hists = [c.camshift_debug_hist(s, current=s in tracked) for s in range(cr.RESERVED)]
            results.append((first.tobytes(), second.tobytes(), [(m.tobytes(), h.tobytes()) for m, h in hists], [v.tobytes() for v in c.camshift_stats(cr.RESERVED, reset=False)]))
        objects_agree(np.frombuffer(results[0][1], dtype=native.CS_TRACKOBJ_DTYPE), [oracle_step(2)[s] for s, _f in pairs], "step 2 behind the align calls")
        assert results[0] == results[1]
        assert crops[0] == crops[1]
        objs = oracle_step(1)
        srcs = [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
        want = [cr.patch(srcs[f], cr.obj_of(objs[s]) if s in objs else (0.0, 0.0, 0.0, 0.0), W, H, None, 256, 0, 70, 19) for s, f in CROP_LIST]
        same(np.frombuffer(crops[0][1], dtype=np.uint8), expected_buffer(want, pb), "the crop call between the align calls")
    finally:
        for c in ctxs:
            c.close()
        res.free()
        for o in outs:
            o.free()


# ---- 6: refusals change nothing ----------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pairs_ctx):
    """every malformed call: the status, `entry <i>` where an entry is at fault, the output buffer still all 0xA5 and the previous
    align_result unchanged; HT_ERR_STATE without geometry, reservation or (pairs form) bound frames"""
    c, _objs, _sources = pairs_ctx
    L, h = c._lib, c._h
    P, Q = 7, 3
    pb = P * Q * 4
    res = ResidentFeeds()
    out = guarded(8, pb)
    fill = guarded(8, pb)
    frames = DeviceArray(np.zeros((2, H, W, 4), dtype=np.uint8))
    fresh = []
    try:
        c.camshift_align_pairs_device(out.ptr, CROP_LIST, P, Q)
        before = c.camshift_align_result(len(CROP_LIST)).tobytes()
        c.synchronize()
        entries = res.entries()
        srcs = c._draw_sources(entries)
        streams7 = np.array([5, 0, 2, 4, 3, 5, 0], dtype=np.int32)
        pairs6 = c._pairs(CROP_LIST)

        def refused(call, status, index=None):
            with pytest.raises(HtError) as e:
                call()
            assert e.value.status == status, str(e.value)
            if index is not None:
                assert f"entry {index}:" in str(e.value), (index, str(e.value))
            c.synchronize()
            assert (d2h(fill.ptr, fill.nbytes) == dl.GUARD).all(), str(e.value)
            assert c.camshift_align_result(len(CROP_LIST)).tobytes() == before, str(e.value)

        def pairs_call(pairs=pairs6, n=None, prm=(P, Q, 256, 0), ptr=fill.ptr, stride=0):
            p = native.ALIGN_PARAMS(*prm)
            return lambda: c._check(L.ht_camshift_align_pairs_device(h, pairs.ctypes.data, len(pairs) if n is None else n, C.byref(p), ptr, stride))

        def sources_call(arr=srcs, streams=streams7, n=7, prm=(P, Q, 256, 0), ptr=fill.ptr, stride=0):
            p = native.ALIGN_PARAMS(*prm)
            return lambda: c._check(L.ht_camshift_align_sources_device(h, streams.ctypes.data, arr, n, C.byref(p), ptr, stride))

        many = np.zeros(65536, dtype=native.PAIR_DTYPE)
        for call in (pairs_call, sources_call):
            refused(call(n=0), HT_ERR_INVALID)
            for prm in ((0, Q, 256, 0), (P, 0, 256, 0), (1025, Q, 256, 0), (P, 1025, 256, 0), (P, Q, 63, 0), (P, Q, 1025, 0), (P, Q, 256, 2), (P, Q, 256, 0x80000000)):
                refused(call(prm=prm), HT_ERR_INVALID)
            refused(call(ptr=fill.ptr + 2), HT_ERR_INVALID)   # misaligned
            refused(call(ptr=None), HT_ERR_INVALID)           # no output
            refused(call(stride=pb - 4), HT_ERR_INVALID)      # undersized stride
            refused(call(stride=pb + 2), HT_ERR_INVALID)      # not a multiple of 4
        refused(pairs_call(pairs=many), HT_ERR_INVALID)        # n = 65536
        refused(sources_call(n=65536), HT_ERR_INVALID)
        bad = pairs6.copy()
        bad[3]["stream"] = cr.RESERVED
        refused(pairs_call(pairs=bad), HT_ERR_INVALID, 3)      # an unreserved stream
        bad = pairs6.copy()
        bad[4]["frame"] = 2
        refused(pairs_call(pairs=bad), HT_ERR_INVALID, 4)      # an unbound frame
        bad = streams7.copy()
        bad[6] = -1
        refused(sources_call(streams=bad), HT_ERR_INVALID, 6)
        e = [dict(x) for x in entries]
        e[5]["rect"] = (0, 0, 2, 5)                            # a rect outside its one-pixel-wide source, at entry 5 of 7
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 5)
        e = [dict(x) for x in entries]
        e[1]["p1"] += 1                                        # odd NV12 chroma base
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 1)
        e = [dict(x) for x in entries]
        e[2]["p1"] = fill.ptr + 3 * pb + 1                     # entry 2's U plane lies inside the output range
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 2)
        # the pairs form's source is a bound frame: an output inside the bound buffer overlaps it
        c.bind_device(frames.ptr, 2)
        with pytest.raises(HtError) as err:
            pairs_call(ptr=frames.ptr + W * H * 4 - 8)()
        assert err.value.status == HT_ERR_INVALID and "entry 0:" in str(err.value)
        c.synchronize()
        assert not d2h(frames.ptr, frames.nbytes).any() and c.camshift_align_result(len(CROP_LIST)).tobytes() == before
        # HT_ERR_STATE: no geometry; geometry but no reservation; (pairs form) no bound frames
        for stage in range(3):
            f = Context()
            fresh.append(f)
            if stage >= 1:
                f.set_geometry(W, H, 2)
            if stage >= 2:
                f.camshift_reserve(cr.RESERVED)
            p = native.ALIGN_PARAMS(P, Q, 256, 0)
            assert L.ht_camshift_align_pairs_device(f._h, pairs6.ctypes.data, len(pairs6), C.byref(p), fill.ptr, 0) == HT_ERR_STATE, stage
            out2 = guarded(8, pb)
            try:
                st = L.ht_camshift_align_sources_device(f._h, streams7.ctypes.data, srcs, 7, C.byref(p), out2.ptr, 0)
                assert st == (HT_ERR_STATE if stage < 2 else 0), (stage, st)  # the sources form needs no bound frames
                assert L.ht_camshift_align_result(f._h, 7, np.zeros(7, dtype=native.ALIGN_RECORD_DTYPE).ctypes.data) == (HT_ERR_STATE if stage < 2 else 0)
                f.synchronize()
                got = d2h(out2.ptr, out2.nbytes)
                if stage == 2:  # never tracked streams: 7 patches of zeros, nothing behind them
                    assert not got[:7 * pb].any() and (got[7 * pb:] == dl.GUARD).all()
                else:
                    assert (got == dl.GUARD).all()
            finally:
                out2.free()
        assert (d2h(fill.ptr, fill.nbytes) == dl.GUARD).all()
    finally:
        a, b = cr.pairs_scene()
        c.upload(np.stack([a.frames[1], b.frames[1]]))  # the shared context gets its step-1 frames back
        for f in fresh:
            f.close()
        res.free()
        out.free()
        fill.free()
        frames.free()

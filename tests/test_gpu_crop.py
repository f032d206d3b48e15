"""The face crops on the device — ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device / ht_camshift_crop_result — against
tests/crop_cases.py.  The track objects are the ORACLE's (ho.Camshift on the scenes' frames; tests/test_crop_cpu.py proves from the oracle
alone that the reference does not depend on the summation order on them), the rect is the Python restatement of the rule, the patch is
Source.expected — the oracle's resampler on the declared conversion.  Nothing expected comes from the code under test, every comparison
is equality of every byte (records: of every bit), there is no tolerance.  Without the feature every test fails at its first crop call."""
import ctypes as C

import numpy as np
import pytest

import crop_cases as cr
import draw_list_cases as dl
import yuv_cases as yc
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from test_gpu_ingest import d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
GUARD_BYTES = 64
W, H = cr.CANVAS
CROP_LIST = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]  # a stream never tracked, one never initialised, one twice


def guarded(n, stride):
    return DeviceArray(np.full(n * stride + GUARD_BYTES, dl.GUARD, dtype=np.uint8))


def expected_buffer(patches, stride):
    """the whole output: 0xA5 everywhere but in the patches, 64 guard bytes behind the last"""
    buf = np.full(len(patches) * stride + GUARD_BYTES, dl.GUARD, dtype=np.uint8)
    for i, p in enumerate(patches):
        buf[i * stride:i * stride + p.size] = p.reshape(-1)
    return buf


def record_tuples(rec):
    """CROP_RECORD_DTYPE rows -> (code, stream, x, y, width, height, rx bits, ry bits)"""
    return [(int(r["code"]), int(r["stream"]), int(r["x"]), int(r["y"]), int(r["width"]), int(r["height"]), cr.f64_bits(float(r["rx"])), cr.f64_bits(float(r["ry"])))
            for r in rec]


def canvas_source(frame):
    """a bound canvas frame as a Source, so that its patches are Source.expected like every other"""
    s = dl.Source(dl.RGBA, W, H, seed=1)
    s.rgba = frame
    return s


def oracle_step(k):
    """{stream: the oracle's track object after step k (1-based)} for the pairs scene's trackers"""
    seqs = cr.pairs_scene()
    return {s: seqs[q].oracle_calls(j)[k - 1][2] for (s, _f, q, j) in cr.pairs_trackers()}


def objects_equal(got, want, where):
    """precondition of the byte comparisons: the device tracked what the oracle tracked"""
    for g, to in zip(got, want):
        assert (float(g["x"]), float(g["y"]), float(g["width"]), float(g["height"])) == cr.obj_of(to), (where, g, to)


def start_pairs(c, first_frame=0):
    """geometry, 6 reserved streams, the scene's three trackers initialised on bound frames first_frame / first_frame + 1 and stream
    NEVER_TRACKED on the second of them"""
    a, b = cr.pairs_scene()
    seqs, tr = (a, b), cr.pairs_trackers()
    c.camshift_reserve(cr.RESERVED)
    c.camshift_init_pairs([(s, first_frame + f) for (s, f, _q, _j) in tr] + [(cr.NEVER_TRACKED, first_frame + 1)], [seqs[q].rects[j] for (_s, _f, q, j) in tr] + [b.rects[0]])
    return [(s, f) for (s, f, _q, _j) in tr]


@pytest.fixture(scope="module")
def pairs_ctx():
    """one context that has tracked step 1 of the pairs scene on two bound frames; the crops of every size read it"""
    a, b = cr.pairs_scene()
    c = Context()
    c.set_geometry(W, H, 2)
    c.upload(np.stack([a.frames[0], b.frames[0]]))
    pairs = start_pairs(c)
    c.upload(np.stack([a.frames[1], b.frames[1]]))
    got = c.camshift_track_pairs(pairs)
    want = oracle_step(1)
    objects_equal(got, [want[s] for s, _f in pairs], "pairs scene, step 1")
    yield c, want, [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
    c.close()


# ---- 1: the pairs form -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", cr.SIZES)
def test_pairs_form_every_output_byte_and_every_record_bit(pairs_ctx, size):
    """97 x 81 canvas, 3 trackers on 2 bound frames, a stream that was initialised but never tracked and one that was never initialised
    (both EMPTY: zeros), one stream twice; outputs 70 x 19 (partial tiles both ways), 1 x 1 and 112 x 112; margins 64 / 256 / 1024, square on
    and off.  The strided output is compared whole — padding between the patches and the 64-byte guard included — and the records,
    rx / ry included, bit for bit."""
    c, objs, sources = pairs_ctx
    P, Q = size
    pb = P * Q * 4
    seen = set()
    for (margin, flags) in cr.CONFIGS:
        stride = pb + 52
        out = guarded(len(CROP_LIST), stride)
        try:
            c.camshift_crop_pairs_device(out.ptr, CROP_LIST, P, Q, margin=margin / 256, square=bool(flags), stride=stride)
            rec = c.camshift_crop_result(len(CROP_LIST))
            c.synchronize()
            got = d2h(out.ptr, out.nbytes)
        finally:
            out.free()
        obj = [cr.obj_of(objs[s]) if s in objs else (0.0, 0.0, 0.0, 0.0) for s, _f in CROP_LIST]
        patches = [cr.patch(sources[f], o, W, H, None, margin, flags, P, Q) for o, (_s, f) in zip(obj, CROP_LIST)]
        for i, p in enumerate(patches):  # per entry first: a failure names the entry
            same(got[i * stride:i * stride + pb].reshape(Q, P, 4), p, f"entry {i} {CROP_LIST[i]} margin {margin} flags {flags} -> {P}x{Q}")
        same(got, expected_buffer(patches, stride), f"the whole output, margin {margin} flags {flags}")
        want = [cr.record(s, o, W, H, W, H, None, margin, flags, P, Q) for o, (s, _f) in zip(obj, CROP_LIST)]
        assert record_tuples(rec) == want, (margin, flags, record_tuples(rec), want)
        seen |= cr.classify([(r[0], r[2:6], W, H) for r in want], P, Q)
        assert [r[0] for r in want] == [cr.FACE, cr.EMPTY, cr.FACE, cr.FACE, cr.EMPTY, cr.FACE]
    # what this case covered: an empty entry, crops clamped on each of the four sides, and the scaling direction(s) of its size
    assert seen >= {"empty", "left", "top", "right", "bottom"} and seen & {"up", "down"}
    assert (P, Q) != (112, 112) or "up" in seen
    assert (P, Q) != (1, 1) or "down" in seen
    assert (P, Q) != (70, 19) or {"up", "down"} <= seen


# ---- 2: the sources form ---------------------------------------------------------------------------------------------------------------------

class ResidentFeeds:
    """the feeds of crop_cases.feeds() in device memory: every plane of every UNSHARED source in an allocation of its own; a source that
    shares another's planes names that one's allocations"""

    def __init__(self):
        self.feeds = cr.feeds()
        self.arrays = {}
        for src, _m in self.feeds:
            if src.share is None:
                self.arrays[id(src)] = [DeviceArray(b) for b in src.plane_buffers()]

    def entry(self, k):
        src, m = self.feeds[k]
        planes = self.arrays[id(src.share if src.share is not None else src)]
        return src.entry([a.ptr for a in planes], m)

    def entries(self):
        return [self.entry(k) for k in range(len(self.feeds))]

    def free(self):
        for planes in self.arrays.values():
            for a in planes:
                a.free()


def test_sources_form_from_a_mixed_list_every_matrix():
    """the canvases are drawn with ht_draw_list_device from a mixed list — a padded RGBA 333 x 217, an NV12 333 x 217 under an odd-origin
    mapping rect, an I420 23 x 23 that the canvas upscales, both YUV allocations again under other rects and matrices, an RGBA and an NV12
    source one pixel wide —, then initialised and tracked on those canvases, then cropped from the SAME sources.  All four matrices;
    streams scattered; 70 x 19, 1 x 1 and 112 x 112."""
    feeds, objs = cr.feeds(), cr.feed_objects()
    n = len(feeds)
    streams = [4, 0, 6, 2, 8, 1, 5]
    assert {s.matrix for s, _ in feeds if s.fmt != dl.RGBA} == {0, 1, 2, 3} and {s.fmt for s, _ in feeds} == {dl.RGBA, yc.NV12, yc.I420}
    assert feeds[0][0].pad0 and feeds[1][1][0] % 2 == 1 and feeds[3][0].share is feeds[1][0] and feeds[4][0].share is feeds[2][0]
    res = ResidentFeeds()
    c = Context()
    seen = set()
    try:
        c.set_geometry(W, H, n)
        c.draw_list(res.entries())  # bound: frame k = feed k's canvas
        c.camshift_reserve(9)
        pairs = [(streams[k], k) for k in range(n)]
        c.camshift_init_pairs(pairs, [cr.canvas_rect_of(k) for k in range(n)])
        objects_equal(c.camshift_track_pairs(pairs), objs, "feeds")
        for (P, Q) in cr.SIZES:
            pb = P * Q * 4
            for (margin, flags) in cr.CONFIGS:
                out = guarded(n, pb)
                try:
                    c.camshift_crop_sources_device(out.ptr, streams, res.entries(), P, Q, margin=margin / 256, square=bool(flags))
                    rec = c.camshift_crop_result(n)
                    c.synchronize()
                    got = d2h(out.ptr, out.nbytes)
                finally:
                    out.free()
                patches = [cr.patch(src, cr.obj_of(to), W, H, m, margin, flags, P, Q) for (src, m), to in zip(feeds, objs)]
                for i, p in enumerate(patches):
                    same(got[i * pb:(i + 1) * pb].reshape(Q, P, 4), p, f"feed {i} ({dl.FORMAT_NAMES[feeds[i][0].fmt]} {feeds[i][0].w}x{feeds[i][0].h}) margin {margin} flags {flags} -> {P}x{Q}")
                same(got, expected_buffer(patches, pb), f"the whole output, margin {margin} flags {flags} -> {P}x{Q}")
                want = [cr.record(st, cr.obj_of(to), W, H, src.w, src.h, m, margin, flags, P, Q) for (src, m), to, st in zip(feeds, objs, streams)]
                assert record_tuples(rec) == want, (margin, flags, P, Q)
                seen |= cr.classify([(r[0], r[2:6], src.w, src.h) for r, (src, _m) in zip(want, feeds)], P, Q)
        ptr, cnt = c.camshift_crop_records_ptr()
        assert cnt == n and record_tuples(np.frombuffer(d2h(ptr, 40 * n).tobytes(), dtype=native.CROP_RECORD_DTYPE)) == want  # the device's copy of the last call's records
    finally:
        c.close()
        res.free()
    assert seen >= {"left", "top", "right", "bottom", "one-wide", "one-high", "up", "down"} and "empty" not in seen


# ---- 3: stream order without the host ----------------------------------------------------------------------------------------------------------

def test_each_crop_reads_the_object_of_its_own_step_without_a_host_round_trip():
    """six bound frames (init, step 1, step 2 of both canvases): track_pairs(out = NULL), crop, track_pairs(out = NULL) on the moved blobs,
    crop — and only then are the track objects collected and the patches read.  Each crop equals the rect of ITS step's oracle object,
    and the two differ."""
    a, b = cr.pairs_scene()
    P, Q, margin, flags = 70, 19, 256, 0
    pb = P * Q * 4
    frames = DeviceArray(np.stack([a.frames[0], b.frames[0], a.frames[1], b.frames[1], a.frames[2], b.frames[2]]))
    outs = [guarded(3, pb), guarded(3, pb)]
    c = Context()
    try:
        c.set_geometry(W, H, 6)
        c.bind_device(frames.ptr, 6)
        pairs = start_pairs(c)
        for k in (1, 2):
            step = [(s, 2 * k + f) for s, f in pairs]
            c.camshift_track_pairs(step, fetch=False)
            c.camshift_crop_pairs_device(outs[k - 1].ptr, step, P, Q, margin=margin / 256, square=bool(flags))
        tracked = [c.camshift_track_collect(3), c.camshift_track_collect(3)]
        rec = c.camshift_crop_result(3)
        c.synchronize()
        got = [d2h(o.ptr, o.nbytes) for o in outs]
    finally:
        c.close()
        frames.free()
        for o in outs:
            o.free()
    rects = []
    for k in (1, 2):
        objs = oracle_step(k)
        objects_equal(tracked[k - 1], [objs[s] for s, _f in pairs], f"step {k}")
        srcs = [canvas_source(a.frames[k]), canvas_source(b.frames[k])]
        same(got[k - 1], expected_buffer([cr.patch(srcs[f], cr.obj_of(objs[s]), W, H, None, margin, flags, P, Q) for s, f in pairs], pb), f"the crops of step {k}")
        rects.append([cr.rule(cr.obj_of(objs[s]), W, H, W, H, None, margin, flags)[1] for s, _f in pairs])
    assert all(r1 != r2 for r1, r2 in zip(*rects)), rects  # every tracker moved: a crop that read the other step's object would show
    assert [r[2:6] for r in record_tuples(rec)] == rects[1]  # the records are the LAST call's


# ---- 4: no tracker state is touched ---------------------------------------------------------------------------------------------------------

def test_crop_calls_leave_the_trackers_as_they_are():
    """a twin context without crop calls returns the same track objects, histograms and statistics on the following step"""
    a, b = cr.pairs_scene()
    res = ResidentFeeds()
    ctxs = [Context(), Context()]
    out = guarded(len(CROP_LIST), 112 * 112 * 4)
    try:
        results = []
        for with_crops, c in zip((True, False), ctxs):
            c.set_geometry(W, H, 2)
            c.upload(np.stack([a.frames[0], b.frames[0]]))
            pairs = start_pairs(c)
            c.camshift_stats(cr.RESERVED, reset=True)
            c.upload(np.stack([a.frames[1], b.frames[1]]))
            first = c.camshift_track_pairs(pairs)
            if with_crops:
                c.camshift_crop_pairs_device(out.ptr, CROP_LIST, 112, 112, margin=4.0, square=True)
                c.camshift_crop_sources_device(out.ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 70, 19)
                assert len(c.camshift_crop_result(7)) == 7
            c.upload(np.stack([a.frames[2], b.frames[2]]))
            second = c.camshift_track_pairs(pairs)
            tracked = {s for s, _f in pairs}
            hists = [c.camshift_debug_hist(s, current=s in tracked) for s in range(cr.RESERVED)]  # (the frame histogram exists for the tracked streams only)
            results.append((first.tobytes(), second.tobytes(), [(m.tobytes(), h.tobytes()) for m, h in hists], [v.tobytes() for v in c.camshift_stats(cr.RESERVED, reset=False)]))
        objects_equal(np.frombuffer(results[0][1], dtype=native.CS_TRACKOBJ_DTYPE), [oracle_step(2)[s] for s, _f in pairs], "step 2 behind the crops")
        assert results[0] == results[1]
    finally:
        for c in ctxs:
            c.close()
        res.free()
        out.free()


# ---- 5: refusals change nothing -------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pairs_ctx):
    """every malformed call: the status, `entry <i>` where an entry is at fault, the output buffer still all 0xA5 and the previous
    crop_result unchanged; HT_ERR_STATE without geometry, reservation or (pairs form) bound frames"""
    c, _objs, _sources = pairs_ctx
    L, h = c._lib, c._h
    P, Q = 7, 3
    pb = P * Q * 4
    res = ResidentFeeds()
    out = guarded(8, pb)
    frames = DeviceArray(np.zeros((2, H, W, 4), dtype=np.uint8))
    fresh = []
    try:
        c.camshift_crop_pairs_device(out.ptr, CROP_LIST, P, Q)
        before = c.camshift_crop_result(len(CROP_LIST)).tobytes()
        c.synchronize()
        _rt_fill = DeviceArray(np.full(out.nbytes, dl.GUARD, dtype=np.uint8))  # a second guarded buffer: `out` now holds patches
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
            assert (d2h(_rt_fill.ptr, _rt_fill.nbytes) == dl.GUARD).all(), str(e.value)
            assert c.camshift_crop_result(len(CROP_LIST)).tobytes() == before, str(e.value)

        def pairs_call(pairs=pairs6, n=None, prm=(P, Q, 256, 0), ptr=_rt_fill.ptr, stride=0):
            p = native.CROP_PARAMS(*prm)
            return lambda: c._check(L.ht_camshift_crop_pairs_device(h, pairs.ctypes.data, len(pairs) if n is None else n, C.byref(p), ptr, stride))

        def sources_call(arr=srcs, streams=streams7, n=7, prm=(P, Q, 256, 0), ptr=_rt_fill.ptr, stride=0):
            p = native.CROP_PARAMS(*prm)
            return lambda: c._check(L.ht_camshift_crop_sources_device(h, streams.ctypes.data, arr, n, C.byref(p), ptr, stride))

        many = np.zeros(65536, dtype=native.PAIR_DTYPE)
        for call in (pairs_call, sources_call):
            refused(call(n=0), HT_ERR_INVALID)
            for prm in ((0, Q, 256, 0), (P, 0, 256, 0), (1025, Q, 256, 0), (P, 1025, 256, 0), (P, Q, 63, 0), (P, Q, 1025, 0), (P, Q, 256, 2), (P, Q, 256, 0x80000000)):
                refused(call(prm=prm), HT_ERR_INVALID)
            refused(call(ptr=_rt_fill.ptr + 2), HT_ERR_INVALID)   # misaligned
            refused(call(ptr=None), HT_ERR_INVALID)               # no output
            refused(call(stride=pb - 4), HT_ERR_INVALID)          # undersized stride
            refused(call(stride=pb + 2), HT_ERR_INVALID)          # not a multiple of 4
        refused(pairs_call(pairs=many), HT_ERR_INVALID)            # n = 65536
        refused(sources_call(n=65536), HT_ERR_INVALID)
        bad = pairs6.copy()
        bad[3]["stream"] = cr.RESERVED
        refused(pairs_call(pairs=bad), HT_ERR_INVALID, 3)          # an unreserved stream
        bad = pairs6.copy()
        bad[4]["frame"] = 2
        refused(pairs_call(pairs=bad), HT_ERR_INVALID, 4)          # an unbound frame
        bad = streams7.copy()
        bad[6] = -1
        refused(sources_call(streams=bad), HT_ERR_INVALID, 6)
        e = [dict(x) for x in entries]
        e[5]["rect"] = (0, 0, 2, 5)                                # a rect outside its one-pixel-wide source, at entry 5 of 7
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 5)
        e = [dict(x) for x in entries]
        e[1]["p1"] += 1                                            # odd NV12 chroma base
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 1)
        e = [dict(x) for x in entries]
        e[2]["p1"] = _rt_fill.ptr + 3 * pb + 1                     # entry 2's U plane lies inside the output range
        refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 2)
        # the pairs form's source is a bound frame: an output inside the bound buffer overlaps it
        c.bind_device(frames.ptr, 2)
        with pytest.raises(HtError) as err:
            pairs_call(ptr=frames.ptr + W * H * 4 - 8)()
        assert err.value.status == HT_ERR_INVALID and "entry 0:" in str(err.value)
        c.synchronize()
        assert not d2h(frames.ptr, frames.nbytes).any() and c.camshift_crop_result(len(CROP_LIST)).tobytes() == before
        # HT_ERR_STATE: no geometry; geometry but no reservation; (pairs form) no bound frames
        for stage in range(3):
            f = Context()
            fresh.append(f)
            if stage >= 1:
                f.set_geometry(W, H, 2)
            if stage >= 2:
                f.camshift_reserve(cr.RESERVED)
            p = native.CROP_PARAMS(P, Q, 256, 0)
            assert L.ht_camshift_crop_pairs_device(f._h, pairs6.ctypes.data, len(pairs6), C.byref(p), _rt_fill.ptr, 0) == HT_ERR_STATE, stage
            st = L.ht_camshift_crop_sources_device(f._h, streams7.ctypes.data, srcs, 7, C.byref(p), out.ptr, 0)
            assert st == (HT_ERR_STATE if stage < 2 else 0), (stage, st)  # the sources form needs no bound frames
            assert L.ht_camshift_crop_result(f._h, 7, np.zeros(7, dtype=native.CROP_RECORD_DTYPE).ctypes.data) == (HT_ERR_STATE if stage < 2 else 0)
            f.synchronize()
        assert (d2h(_rt_fill.ptr, _rt_fill.nbytes) == dl.GUARD).all()
        assert not d2h(out.ptr, 7 * pb).any() and (d2h(out.ptr + 7 * pb, out.nbytes - 7 * pb) == dl.GUARD).all()  # never tracked streams: 7 patches of zeros, nothing behind them
        _rt_fill.free()
    finally:
        a, b = cr.pairs_scene()
        c.upload(np.stack([a.frames[1], b.frames[1]]))  # the shared context gets its step-1 frames back
        for f in fresh:
            f.close()
        res.free()
        out.free()
        frames.free()

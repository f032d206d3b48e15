"""ht_draw_list_filtered_device (the draw list with a prefilter: each canvas pixel the mean of an Nx x Ny block of the unfiltered draw's
samples) against tests/draw_filter_cases.py: the fine frame is ingest_cases.expected / yuv_cases.expected on the canvas of Nx W x Ny H — the
oracle's resampler and the declared conversion, pinned by the CPU suite — and the mean is filter_cases.block_mean.  Both are exact sequences
of operations, so there is no tolerance: every comparison is equality of every byte.  tests/test_draw_filter_cpu.py proves what the scenes
cover.  Without the feature every test here fails at its first filtered call: the library has no ht_draw_list_filtered_device."""
import math

import numpy as np
import pytest

import crop_cases as cr
import draw_filter_cases as dfc
import draw_list_cases as dl
import filter_cases as fc
import ingest_cases as ic
import yuv_cases as yc
from headtrackr_amd import synth
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_crop import ResidentFeeds, objects_equal, record_tuples
from test_gpu_draw_list import GUARD_BYTES, Resident, expected_buffer, guarded
from test_gpu_ingest import bound_equals, d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def resident():
    """every scene's sources in device memory, uploaded once: {scene: Resident}"""
    res = {name: Resident(dfc.scene(name)[1]) for name in dfc.SCENES if name != "small"}
    res["small"] = res["long"]  # the same eight sources
    yield res
    for name in dfc.SCENES:
        if name != "small":
            res[name].free()


def describe(name, i):
    _, srcs, plan = dfc.scene(name)
    s, rect = srcs[plan[i][0]], plan[i][1]
    return f"{name} entry {i} ({dl.FORMAT_NAMES[s.fmt]} {s.w}x{s.h} rect {rect})"


# ---- 1: every scene x max_factor, every byte ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_factor", dfc.MAX_FACTORS)
@pytest.mark.parametrize("name", dfc.SCENES)
def test_every_scene_every_destination_byte(ctx, resident, name, max_factor):
    """into the caller's buffer, the frames a stride beyond a frame apart: every byte of the destination — the frames, the padding between
    them (0xA5) and the guard behind the last — is the restatement's; max_factor 8, 3, 2 and 1"""
    (dw, dh), _srcs, plan = dfc.scene(name)
    ctx.set_geometry(dw, dh, 2)  # the form into a caller's buffer is not limited by the batch capacity
    res = resident[name]
    fb = dw * dh * 4
    dstride = fb + 52
    ddst = guarded(len(plan), dw, dh, dstride)
    try:
        ctx.draw_list([res.entry(k, rect) for k, rect in plan], dst=ddst.ptr, dst_stride=dstride, prefilter=max_factor)
        ctx.synchronize()
        got = d2h(ddst.ptr, ddst.nbytes)
    finally:
        ddst.free()
    wants = [w for w, _f in dfc.scene_expected(name, max_factor)]
    for i, w in enumerate(wants):  # per entry first: a failure names the entry
        same(got[i * dstride:i * dstride + fb].reshape(dh, dw, 4), w, f"{describe(name, i)} max_factor {max_factor} factors {dfc.scene_expected(name, max_factor)[i][1]}")
    same(got, expected_buffer(wants, dw, dh, dstride), "the whole destination")


@pytest.mark.parametrize("max_factor", [8, 2])
def test_bind_form_binds_the_filtered_frames(resident, max_factor):
    """dst NULL on 40 x 30 with all twelve entries: the bound frames are the restatement (read through the pyramid, bound_equals) and
    ht_frames_bound() is the list's length"""
    (dw, dh), _srcs, plan = dfc.scene("canvas")
    res = resident["canvas"]
    c = Context()
    try:
        c.set_geometry(dw, dh, len(plan))
        c.draw_list([res.entry(k, rect) for k, rect in plan], prefilter=max_factor)
        want = np.stack([w for w, _f in dfc.scene_expected("canvas", max_factor)])
        assert c._lib.ht_frames_bound(c._h) == len(plan)
        bound_equals(c, want, f"bound form, max_factor {max_factor}")
    finally:
        c.close()


@pytest.mark.parametrize("max_factor", [8, 2])
@pytest.mark.parametrize("name", ["wide", "canvas", "pixel"])
def test_the_64_x_16_tile_form_gives_the_same_bytes(resident, name, max_factor):
    """the tile is a template parameter; the library launches 64 x 4 and keeps 64 x 16 behind the context option draw_filter_rows = 16 (the
    measurement compares them).  On 70 x 19 the last tile row is partial in both forms (19 = 4 * 4 + 3 = 16 + 3): every byte again"""
    (dw, dh), _srcs, plan = dfc.scene(name)
    res = resident[name]
    fb = dw * dh * 4
    ddst = guarded(len(plan), dw, dh, fb)
    c = Context(options="draw_filter_rows=16")
    try:
        c.set_geometry(dw, dh, 2)
        c.draw_list([res.entry(k, rect) for k, rect in plan], dst=ddst.ptr, prefilter=max_factor)
        c.synchronize()
        got = d2h(ddst.ptr, ddst.nbytes)
    finally:
        c.close()
        ddst.free()
    same(got, expected_buffer([w for w, _f in dfc.scene_expected(name, max_factor)], dw, dh, fb), f"{name}, max_factor {max_factor}, tile 64 x 16")


# ---- 2: the same kernel text against the existing kernel ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("factors,canvas", [((2, 2), (40, 30)), ((3, 5), (40, 30)), ((8, 8), (70, 19))])
def test_block_mean_of_the_existing_kernels_fine_frames(ctx, factors, canvas):
    """a twin context of geometry (Nx W, Ny H) draws the same entries with ht_draw_list_device; the numpy block mean of what it wrote is
    the filtered call's output, byte for byte — and both are the restatement"""
    (nx, ny), (dw, dh) = factors, canvas
    srcs = dfc.uniform_list(nx, ny, dw, dh)
    res = Resident(srcs)
    fine_ctx = Context()
    fb, ffb = dw * dh * 4, nx * dw * ny * dh * 4
    dfine, dgot = guarded(len(srcs), nx * dw, ny * dh, ffb), guarded(len(srcs), dw, dh, fb)
    try:
        fine_ctx.set_geometry(nx * dw, ny * dh, 1)
        fine_ctx.draw_list([res.entry(k) for k in range(len(srcs))], dst=dfine.ptr)
        fine_ctx.synchronize()
        fine = d2h(dfine.ptr, dfine.nbytes)
        ctx.set_geometry(dw, dh, 1)
        ctx.draw_list([res.entry(k) for k in range(len(srcs))], dst=dgot.ptr, prefilter=8)
        ctx.synchronize()
        got = d2h(dgot.ptr, dgot.nbytes)
    finally:
        fine_ctx.close()
        res.free()
        dfine.free()
        dgot.free()
    for i, s in enumerate(srcs):
        f = fine[i * ffb:(i + 1) * ffb].reshape(ny * dh, nx * dw, 4)
        same(f, s.expected(None, nx * dw, ny * dh), f"the twin context's fine frame {i}")
        same(got[i * fb:(i + 1) * fb].reshape(dh, dw, 4), fc.block_mean(f, nx, ny), f"entry {i} ({dl.FORMAT_NAMES[s.fmt]}) at factors {factors}")
        assert dfc.expected(s, None, dw, dh, 8)[1] == factors
    assert (got[len(srcs) * fb:] == dl.GUARD).all()


# ---- 3: factor 1 is the unfiltered call -------------------------------------------------------------------------------------------------------------

def test_factor_1_equals_the_unfiltered_call(ctx, resident):
    """max_factor 1 on the 70 x 19 scene (sources up to 8 x the canvas), and max_factor 8 on a list whose sources are not larger than the
    canvas (equal size, smaller, one pixel wide, under a small rect): the bytes ht_draw_list_device writes for the same list"""
    (dw, dh), _srcs, plan = dfc.scene("wide")
    small = [dl.Source(dl.RGBA, 70, 19, seed=161, pad0=4), dl.Source(yc.NV12, 23, 19, seed=162, matrix=1, pad0=1), dl.Source(yc.I420, 69, 7, seed=163, matrix=3, pad1=3),
             dl.Source(dl.RGBA, 1, 5, seed=164), dl.Source(yc.NV12, 333, 131, seed=165, matrix=2)]
    small_plan = [(0, None), (1, None), (2, None), (3, None), (4, (101, 33, 70, 19)), (4, (1, 1, 2, 2))]
    res_small = Resident(small)
    ctx.set_geometry(dw, dh, 2)
    fb = dw * dh * 4
    try:
        for what, entries, mf in (("max_factor 1", [resident["wide"].entry(k, rect) for k, rect in plan], 1), ("sources not larger than the canvas", [res_small.entry(k, rect) for k, rect in small_plan], 8)):
            a, b = guarded(len(entries), dw, dh, fb), guarded(len(entries), dw, dh, fb)
            try:
                ctx.draw_list(entries, dst=a.ptr)
                ctx.draw_list(entries, dst=b.ptr, prefilter=mf)
                ctx.synchronize()
                same(d2h(b.ptr, b.nbytes), d2h(a.ptr, a.nbytes), what)
            finally:
                a.free()
                b.free()
        assert all(dfc.factors(*dfc.size_of((small[k].w, small[k].h), rect), dw, dh, 8) == (1, 1) for k, rect in small_plan)
    finally:
        res_small.free()


# ---- 4: the bind form feeds the pipeline, in order ----------------------------------------------------------------------------------------------------

def face_sources(frames):
    """synth RGBA frames as RGBA sources of the list"""
    out = []
    for f in frames:
        s = dl.Source(dl.RGBA, f.shape[1], f.shape[0], seed=1)
        s.rgba = f
        out.append(s)
    return out


def test_filtered_bound_frames_feed_detect_and_camshift():
    """640 x 480 synth frames drawn filtered (factors 4, 4) and bound on 160 x 120, the smallest geometry the detect tests use: the raw hits,
    and the track objects of one camshift init + track on the next filtered draw, are bit-equal to a twin context that got the same
    filtered bytes through ht_upload_frames — and those bytes are the restatement's"""
    from test_gpu_detect import assert_hits_equal

    (sw, sh), (dw, dh), n = (640, 480), (160, 120), 2
    vids = [[synth.face_frame(sw, sh, [(200 + 40 * f + 12 * k, 120 + 8 * k, 192)]) for f in range(n)] for k in range(2)]
    srcs = [face_sources(v) for v in vids]
    want = [np.stack([dfc.expected(s, None, dw, dh, 8)[0] for s in ss]) for ss in srcs]
    assert dfc.factors(sw, sh, dw, dh, 8) == (4, 4) and not np.array_equal(want[0][0], ic.expected(vids[0][0], None, dw, dh))
    res = [Resident(ss) for ss in srcs]
    c, twin = Context(), Context()
    try:
        for x in (c, twin):
            x.set_geometry(dw, dh, n)
            x.camshift_reserve(n)
        c.draw_list([res[0].entry(k) for k in range(n)], prefilter=8)
        twin.upload(want[0])
        c.detect_enqueue(0)
        hits, counts = c.detect_collect()
        twin.detect_enqueue(0)
        thits, tcounts = twin.detect_collect()
        assert len(hits) > 0 and counts.tolist() == tcounts.tolist() and (counts > 0).all()
        assert_hits_equal(hits, thits)
        best = c.best_faces(hits, counts, 1)
        rects = [tuple(int(math.floor(best[k][f])) for k in ("x", "y", "width", "height")) for f in range(n)]
        c.camshift_init(rects)
        twin.camshift_init(rects)
        c.draw_list([res[1].entry(k) for k in range(n)], prefilter=8)
        twin.upload(want[1])
        got, tgot = c.camshift_track(n, calc_angles=True), twin.camshift_track(n, calc_angles=True)
        assert got.tobytes() == tgot.tobytes() and (got["width"] > 0).all(), (got, tgot)
        bound_equals(c, want[1], "the filtered bound frames")
    finally:
        c.close()
        twin.close()
        for r in res:
            r.free()


def test_two_filtered_draws_into_the_same_buffer_each_get_their_own_detections():
    """the bind form writes the context's own frame buffer, whose pointer does not change, and the detect sequence of a small batch is
    replayed from a captured graph keyed on that pointer: the replay runs behind the filtered draw on the context's stream and must see
    the NEW pixels.  Two contents alternate for six rounds; every round's hits are those of a twin context that uploaded the restated
    canvases of the content drawn last"""
    from test_gpu_detect import assert_hits_equal

    (sw, sh), (dw, dh), n = (640, 480), (160, 120), 2
    a = [synth.face_frame(sw, sh, [(200, 120, 192)]), synth.face_frame(sw, sh, [(80, 60, 160), (380, 220, 224)])]
    b = [synth.face_frame(sw, sh, [(300, 200, 240)]), ic.smooth(sw, sh, 3)]
    sa, sb = face_sources(a), face_sources(b)
    wa, wb = (np.stack([dfc.expected(s, None, dw, dh, 8)[0] for s in ss]) for ss in (sa, sb))
    ra, rb = Resident(sa), Resident(sb)
    c, twin = Context(), Context()
    try:
        c.set_geometry(dw, dh, n)
        twin.set_geometry(dw, dh, n)
        ref = []
        for w in (wa, wb):
            twin.upload(w)
            twin.detect_enqueue(0)
            ref.append(twin.detect_collect()[0].copy())
        assert len(ref[0]) > 0 and len(ref[1]) > 0 and (len(ref[0]) != len(ref[1]) or not np.array_equal(ref[0]["sum"], ref[1]["sum"]))  # the contents do differ
        for rnd in range(6):
            r = (ra, rb)[rnd % 2]
            c.draw_list([r.entry(k) for k in range(n)], prefilter=8)
            c.detect_enqueue(0)
            hits, _ = c.detect_collect()
            assert_hits_equal(hits, ref[rnd % 2])
        assert c.graph_launches >= 4, c.graph_launches  # rounds 1 .. 5 were replays (round 1 captures and launches)
    finally:
        c.close()
        twin.close()
        ra.free()
        rb.free()


# ---- 5: refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_entry_and_change_nothing(resident):
    """max_factor 0 and 9, a source plane overlapping the destination, a rect outside its source, more entries than the batch capacity in
    the bind form: HT_ERR_INVALID, the entry's index (or max_factor) in ht_last_error, the destination still all 0xA5, the bound frames
    as they were — and the next valid call draws the restatement"""
    (dw, dh), _srcs, plan = dfc.scene("canvas")
    res = resident["canvas"]
    fb = dw * dh * 4
    ddst = guarded(len(plan), dw, dh, fb)
    c = Context()
    try:
        c.set_geometry(dw, dh, 3)
        bound = np.stack([ic.noise(dw, dh, 60 + k) for k in range(2)])
        c.upload(bound)
        good = [res.entry(k, rect) for k, rect in plan]

        def refused(entries, needle, dst=ddst.ptr, mf=8):
            with pytest.raises(HtError) as e:
                c.draw_list(entries, dst=dst, prefilter=mf)
            assert e.value.status == HT_ERR_INVALID, str(e.value)
            assert needle in str(e.value) and "ht_draw_list_filtered_device" in str(e.value), (needle, str(e.value))
            c.synchronize()
            assert (d2h(ddst.ptr, ddst.nbytes) == dl.GUARD).all(), needle
            assert c._lib.ht_frames_bound(c._h) == 2, needle

        refused(good, "max_factor must be 1..8", mf=0)
        refused(good, "max_factor must be 1..8", mf=9)
        refused(good, "max_factor must be 1..8", dst=None, mf=9)
        bad = [dict(e) for e in good]
        bad[4]["p1"] = ddst.ptr + 2 * fb + 16                          # entry 4's U plane lies inside destination frame 2
        refused(bad, "entry 4:")
        bad = [dict(e) for e in good]
        bad[9]["p0"] = ddst.ptr + len(plan) * fb - 1                   # entry 9's Y plane begins at the destination's last byte
        refused(bad, "entry 9:")
        bad = [dict(e) for e in good]
        bad[7]["rect"] = (1, 0, 80, 60)                                # one column beyond the right edge
        refused(bad, "entry 7:")
        refused(good[:4], "entry 3:", dst=None)                        # four entries, max_batch 3: entry 3 is the first without a frame
        bound_equals(c, bound, "the bound frames after the refusals")
        c.draw_list(good, dst=ddst.ptr, prefilter=8)                   # ... and the same context draws the good list afterwards
        c.synchronize()
        same(d2h(ddst.ptr, ddst.nbytes), expected_buffer([w for w, _f in dfc.scene_expected("canvas", 8)], dw, dh, fb), "after the refusals")
    finally:
        c.close()
        ddst.free()


# ---- 6: the face crops on a filtered canvas -----------------------------------------------------------------------------------------------------

def test_crop_feeds_on_a_filtered_canvas():
    """the rect -> canvas mapping does not depend on the filter: crop_cases.feeds() drawn FILTERED onto the 97 x 81 canvas (factors up to
    (4, 3)), trackers initialised and tracked there — the oracle's objects on the restated filtered canvases —, then
    ht_camshift_crop_sources_device with the rects that were drawn gives the patches and records of the crop restatement"""
    W, H = cr.CANVAS
    feeds = cr.feeds()
    n = len(feeds)
    streams = [4, 0, 6, 2, 8, 1, 5]
    canvases = [dfc.expected(src, m, W, H, 8) for src, m in feeds]
    assert {f for _c, f in canvases} >= {(4, 3), (1, 1)} and not np.array_equal(canvases[0][0], cr.canvas_of(0))
    objs = []
    for k in range(n):
        o = ho.Camshift(True)
        o.init_tracker(canvases[k][0], cr.canvas_rect_of(k))
        objs.append(o.track(canvases[k][0])[1])
    res = ResidentFeeds()
    c = Context()
    try:
        c.set_geometry(W, H, n)
        c.draw_list(res.entries(), prefilter=8)  # bound: frame k = feed k's filtered canvas
        c.camshift_reserve(9)
        pairs = [(streams[k], k) for k in range(n)]
        c.camshift_init_pairs(pairs, [cr.canvas_rect_of(k) for k in range(n)])
        objects_equal(c.camshift_track_pairs(pairs), objs, "feeds on the filtered canvas")
        for (P, Q, margin, flags) in ((70, 19, 256, 0), (16, 7, 1024, cr.SQUARE)):
            pb = P * Q * 4
            out = DeviceArray(np.full(n * pb + GUARD_BYTES, dl.GUARD, dtype=np.uint8))
            try:
                c.camshift_crop_sources_device(out.ptr, streams, res.entries(), P, Q, margin=margin / 256, square=bool(flags))
                rec = c.camshift_crop_result(n)
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            for i, ((src, m), to) in enumerate(zip(feeds, objs)):
                same(got[i * pb:(i + 1) * pb].reshape(Q, P, 4), cr.patch(src, cr.obj_of(to), W, H, m, margin, flags, P, Q), f"feed {i} margin {margin} flags {flags} -> {P}x{Q}")
            assert (got[n * pb:] == dl.GUARD).all()
            assert record_tuples(rec) == [cr.record(st, cr.obj_of(to), W, H, src.w, src.h, m, margin, flags, P, Q) for (src, m), to, st in zip(feeds, objs, streams)]
        bound_equals(c, np.stack([cv for cv, _f in canvases]), "the filtered canvases, still bound")
    finally:
        c.close()
        res.free()


# ---- 7: from Node on the real addon ---------------------------------------------------------------------------------------------------------------

def test_node_facade_draws_a_filtered_list_on_the_device(tmp_path):
    """tests/js/draw_filter_gpu.js on the real addon: a ccv.DeviceBatch with mixed opts.sources (NV12 odd x odd, RGBA under a rect, I420
    under a rect with an odd origin) — drawList(.., {prefilter: 8}) writes the Python-side bytes into the frame set; drawListBound with
    it feeds whitebalance and detectStep; without opts the unfiltered canvases, as before"""
    import json
    import os
    import shutil
    import subprocess

    from conftest import ROOT
    from headtrackr_amd import build

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    dw, dh = 160, 120
    srcs = [dl.Source(yc.NV12, 333, 217, seed=71, matrix=1, content="smooth"), dl.Source(dl.RGBA, 640, 480, seed=72, content="smooth"),
            dl.Source(yc.I420, 23, 23, seed=73, matrix=2), dl.Source(yc.I420, 1279, 719, seed=74, matrix=3)]
    rects = [None, (21, 13, 600, 450), (1, 1, 21, 21), None]
    job = dict(w=dw, h=dh, dir=str(tmp_path), prefilter=8, feeds=[])
    for k, (s, rect) in enumerate(zip(srcs, rects)):
        s.packed().tofile(tmp_path / f"feed{k}.raw")
        want, f = dfc.expected(s, rect, dw, dh, 8)
        want.tofile(tmp_path / f"want{k}.raw")
        s.expected(rect, dw, dh).tofile(tmp_path / f"plain{k}.raw")
        job["feeds"].append(dict(file=f"feed{k}.raw", want=f"want{k}.raw", plain=f"plain{k}.raw", width=s.w, height=s.h, format=dl.FORMAT_NAMES[s.fmt],
                                 matrix=yc.MATRIX_NAMES[s.matrix], rect=list(rect) if rect else None, factors=list(f)))
    assert [f["factors"] for f in job["feeds"]] == [[3, 2], [4, 4], [1, 1], [8, 6]]
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "draw_filter_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "draw_filter_gpu: ok" in r.stdout, r.stdout[-2000:]

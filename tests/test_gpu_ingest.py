"""The device drawImage (ht_draw_frames / ht_draw_frames_device; the loop's video -> canvas copy, main.js:170) against
tests/ingest_cases.py's `expected` — the oracle's ho_resample per channel, pinned by tests/test_ingest_cpu.py to oracle/canvas_shim.js,
to headtrackr_amd/js/canvas.js and to the canvases the unmodified reference drew (tests/golden/ingest.json).  The declared resampler is
a fixed sequence of correctly rounded binary64 operations, so there is no tolerance: every comparison of pixels is equality of every
byte.  Without the feature every test here fails at its first call: the library has no ht_draw_frames symbol."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import bp_cases
import ingest_cases as ic
from conftest import ROOT
from cs_cases import ANGLE_TOL
from headtrackr_amd import synth
from headtrackr_amd.api import HT_INPUT_GRAY_IN_R, Context, HtError
from hipmem import DeviceArray, _rt
from oracle import ht_oracle as ho
from test_gpu_camshift import assert_all_exact as cs_all_exact, check as cs_check

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ; first at {tuple(bad[0])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def d2h(ptr, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    assert _rt().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def draw_device(c, src, dw, dh, rect=None, pitch_pad=0, sstride_pad=0, dstride_pad=0, lead=0):
    """ht_draw_frames_device of host frames src [n, sh, sw, 4] through device buffers laid out with the given paddings (bytes, multiples
    of 4; source padding filled with 0x5A, the destination buffer with 0xA5) -> (frames [n, dh, dw, 4], the whole destination buffer)"""
    n, sh, sw, _ = src.shape
    pitch, fb = sw * 4 + pitch_pad, dw * dh * 4
    sstride, dstride = pitch * sh + sstride_pad, fb + dstride_pad
    host = np.full(n * sstride, 0x5A, dtype=np.uint8)
    for f in range(n):
        rows = host[f * sstride:f * sstride + pitch * sh].reshape(sh, pitch)
        rows[:, :sw * 4] = src[f].reshape(sh, sw * 4)
    dsrc = DeviceArray(host)
    ddst = DeviceArray(np.full(lead + n * dstride + 64, 0xA5, dtype=np.uint8))
    try:
        c.draw_frames_device(dsrc.ptr, n, sw, sh, pitch=pitch if pitch_pad else 0, stride=sstride if (pitch_pad or sstride_pad) else 0, rect=rect,
                             dst=ddst.ptr + lead, dst_stride=dstride if dstride_pad else 0)
        c.synchronize()
        buf = d2h(ddst.ptr, ddst.nbytes)
    finally:
        dsrc.free()
        ddst.free()
    frames = np.stack([buf[lead + f * dstride:lead + f * dstride + fb].reshape(dh, dw, 4) for f in range(n)])
    return frames, buf


def bound_equals(c, want, what):
    """the BOUND frames hold `want` [n, H, W, 4]: the library exposes no read-back of frames, so they are read through the stages that
    consume them — level 0 of the pyramid with HT_INPUT_GRAY_IN_R is the R channel byte for byte, with RGBA input it is ccv.grayscale of
    (R, G, B), and getWhitebalance is the mean of that gray plane (A is read by no stage)"""
    n = len(want)
    assert c._lib.ht_frames_bound(c._h) == n == c.nframes, what
    c.detect_enqueue(HT_INPUT_GRAY_IN_R)
    c.detect_collect()
    for f in range(n):
        same(c.pyramid_readback(f, 0), want[f][..., 0], f"{what}: R channel of bound frame {f}")
    c.detect_enqueue(0)
    c.detect_collect()
    for f in range(n):
        same(c.pyramid_readback(f, 0), ho.grayscale_rgba(want[f])[..., 0], f"{what}: gray plane of bound frame {f}")
    wb = c.whitebalance()
    for f in range(n):
        assert wb[f] == ho.whitebalance(want[f]), (what, f)


# ---- ratio families x content ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", ic.RATIOS, ids=lambda r: f"{r[0][0]}x{r[0][1]}-to-{r[1][0]}x{r[1][1]}")
def test_ratio_families_and_content(ctx, ratio):
    """every ratio family with noise (all four channels random), smooth, all-0 and all-255 frames; the exact 2:1 also with constructed
    .5 ties of both parities.  A 1-pixel-wide or -high canvas is drawn if ht_set_geometry accepts the geometry (the pyramid may not)."""
    (sw, sh), (dw, dh) = ratio
    try:
        ctx.set_geometry(dw, dh, 4)
    except HtError as e:
        assert min(dw, dh) == 1 and e.status == HT_ERR_INVALID, (ratio, str(e))
        return  # the library has no such geometry: nothing to draw onto
    families = ["noise", "smooth", "zeros", "ones"] + (["ties"] if (sw, sh) == (2 * dw, 2 * dh) else [])
    for family in families:
        n = 1 if family in ("zeros", "ones") or sw * sh > 10 ** 6 else 2
        src = ic.frames_of(family, sw, sh, n, seed=sw + 7 * dh)
        got, _ = draw_device(ctx, src, dw, dh)
        for f in range(n):
            want = ic.expected(src[f], None, dw, dh)
            same(got[f], want, f"{ratio} {family} frame {f}")
            if (sw, sh) == (dw, dh):
                same(got[f], src[f], f"{ratio} {family}: 1:1 is the exact copy")
            if family == "ties":  # the construction worked: half of the means round down to an even q, half up to an even q + 1
                q = (src[f][0::2, 0::2].astype(int) + src[f][0::2, 1::2] + src[f][1::2, 0::2] + src[f][1::2, 1::2] - 2) // 4
                assert ((src[f][0::2, 0::2].astype(int) + src[f][0::2, 1::2] + src[f][1::2, 0::2] + src[f][1::2, 1::2]) % 4 == 2).all()
                assert np.array_equal(want, q + (q & 1)) and (q & 1).any() and not (q & 1).all()


# ---- source rects ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [((333, 217), (97, 81)), ((160, 120), (320, 240)), ((1280, 720), (320, 240)), ((61, 45), (61, 45))],
                         ids=lambda r: f"{r[0][0]}x{r[0][1]}-to-{r[1][0]}x{r[1][1]}")
def test_source_rects_clamp_to_the_rect(ctx, ratio):
    """odd origins, rects touching every edge and corner; the area outside the rect is filled with another pattern and the result must
    equal the oracle on the CROPPED source drawn whole — a draw that clamps its edge taps to the frame instead of the rect fails"""
    (sw, sh), (dw, dh) = ratio
    ctx.set_geometry(dw, dh, 2)
    base = ic.frames_of("noise", sw, sh, 2, seed=5)
    for ri, rect in enumerate(ic.rects_for(sw, sh)):
        x, y, w, h = rect
        src = np.stack([ic.outside_filled(base[f], rect, 90 + ri + f) for f in range(2)])
        got, _ = draw_device(ctx, src, dw, dh, rect=rect)
        for f in range(2):
            crop = np.ascontiguousarray(base[f][y:y + h, x:x + w])
            same(got[f], ic.expected(crop, None, dw, dh), f"{ratio} rect {rect} frame {f} vs the cropped source")
            same(got[f], ic.expected(src[f], rect, dw, dh), f"{ratio} rect {rect} frame {f} vs the oracle with the rect")


# ---- layout ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 64])
def test_pitch_strides_and_sentinels(ctx, n):
    """pitch larger than a row, frame strides larger than a frame on both sides, the destination at an offset that is only 4-byte
    aligned, n distinct frames in one launch: every frame equals the oracle, and every destination byte outside the frames — in front
    of the first, between frames, behind the last — keeps its sentinel"""
    (sw, sh), (dw, dh) = (333, 217), (160, 120)
    ctx.set_geometry(dw, dh, 2)  # the device form into a caller's buffer is not limited by the batch capacity
    bound_before = ctx._lib.ht_frames_bound(ctx._h)
    src = ic.frames_of("noise", sw, sh, n, seed=300 + n)
    rect = (3, 5, sw - 7, sh - 9)
    lead, dpad = 12, 20
    got, buf = draw_device(ctx, src, dw, dh, rect=rect, pitch_pad=28, sstride_pad=4 * 41, dstride_pad=dpad, lead=lead)
    fb = dw * dh * 4
    assert (buf[:lead] == 0xA5).all()
    for f in range(n):
        same(got[f], ic.expected(src[f], rect, dw, dh), f"n = {n} frame {f}")
        gap = buf[lead + f * (fb + dpad) + fb:lead + (f + 1) * (fb + dpad)]
        assert len(gap) == dpad and (gap == 0xA5).all(), (n, f)
    assert (buf[lead + n * (fb + dpad):] == 0xA5).all()
    assert ctx._lib.ht_frames_bound(ctx._h) == bound_before  # a draw into a caller's buffer binds nothing


# ---- host form and bind form -------------------------------------------------------------------------------------------------------------

def test_host_form_equals_device_form_and_binds(ctx):
    (sw, sh), (dw, dh), n = (333, 217), (160, 120), 3
    ctx.set_geometry(dw, dh, n)
    src = ic.frames_of("smooth", sw, sh, n, seed=41)
    for rect in (None, (7, 0, sw - 7, sh), (5, 3, 122, 77)):
        dev, _ = draw_device(ctx, src, dw, dh, rect=rect)
        want = np.stack([ic.expected(src[f], rect, dw, dh) for f in range(n)])
        same(dev, want, f"device form, rect {rect}")
        ctx.draw_frames(src, rect=rect)
        bound_equals(ctx, want, f"host form, rect {rect}")
    # the device form with dst == NULL binds the same
    d = DeviceArray(src)
    try:
        ctx.draw_frames_device(d.ptr, 2, sw, sh)
        bound_equals(ctx, np.stack([ic.expected(src[f], None, dw, dh) for f in range(2)]), "bind form")
    finally:
        ctx.synchronize()
        d.free()


def hits_of(c, cascade, want):
    """detect on the bound frames == the oracle's raw hits on `want`, bit for bit"""
    from test_gpu_detect import assert_hits_equal, oracle_hits

    c.detect_enqueue(0)
    hits, counts = c.detect_collect()
    ref = np.concatenate([oracle_hits(want[f], cascade, f) for f in range(len(want))])
    assert_hits_equal(hits, ref)
    return hits, counts


def test_every_stage_reads_the_drawn_frames(ctx, cascade):
    """draw 3 x 640x480 face frames onto 320x240 and run every consumer on the bound result: detect_objects (raw hits and grouped best
    faces), getWhitebalance, camshift init + track (the next drawn frames), back-projection — all equal the oracle run on `expected`"""
    (sw, sh), (dw, dh), n = (640, 480), (320, 240), 3
    ctx.set_geometry(dw, dh, n)
    ctx.camshift_reserve(n)
    vids = [np.stack([synth.face_frame(sw, sh, [(200 + 20 * f + 3 * k, 120 + 2 * k, 192)]) for f in range(n)]) for k in range(4)]
    want = [np.stack([ic.expected(v[f], None, dw, dh) for f in range(n)]) for v in vids]
    ctx.draw_frames(vids[0])
    assert ctx._lib.ht_frames_bound(ctx._h) == n
    hits, counts = hits_of(ctx, cascade, want[0])
    best = ctx.best_faces(hits, counts, 1)
    ref_best = ho.best_faces(want[0], cascade.blob, 1)
    for k in ("x", "y", "width", "height", "confidence", "neighbors"):
        assert np.array_equal(best[k], ref_best[k]), k
    assert (best["neighbors"] > 0).all() and (best["confidence"] > -10).all()
    wb = ctx.whitebalance()
    assert [float(v) for v in wb] == [ho.whitebalance(want[0][f]) for f in range(n)]
    rects = [tuple(int(math.floor(best[k][f])) for k in ("x", "y", "width", "height")) for f in range(n)]
    ctx.camshift_init(rects)
    oracles = []
    for f in range(n):
        o = ho.Camshift(True)
        o.init_tracker(want[0][f], rects[f])
        oracles.append(o)
    stats = []
    for k in range(1, 4):
        ctx.draw_frames(vids[k])
        got = ctx.camshift_track(n, calc_angles=True)
        for f in range(n):
            sw_, to = oracles[f].track(want[k][f])
            cs_check(got[f], sw_, to, stats, where=("ingest", f, k))
    cs_all_exact(stats, "track on drawn frames")
    rgba = ctx.camshift_backproject(n, kind="rgba8")
    pdf = ctx.camshift_backproject(n, kind="f64")
    for f in range(n):
        wr, wp = bp_cases.expected(bp_cases.model_of(want[0][f], rects[f]), want[3][f])
        same(rgba[f], wr, f"back-projection rgba8 {f}")
        assert np.array_equal(pdf[f].view(np.uint64), wp.view(np.uint64)), f


def test_two_draws_into_the_same_buffer_each_get_their_own_detections(cascade):
    """The bind form writes the context's own frame buffer, whose pointer does not change between calls, and the detect sequence of a
    small batch is replayed from a hipGraph keyed on (frames pointer, count, flags).  The replay runs on the context's stream behind the
    draw, so it must see the NEW pixels: alternate two different contents, detect after each draw, six rounds (the graph is captured on
    the second enqueue and replayed from then on) — every round returns the hits of the content drawn last."""
    (sw, sh), (dw, dh), n = (640, 480), (320, 240), 2
    c = Context()
    try:
        c.set_geometry(dw, dh, n)
        a = np.stack([synth.face_frame(sw, sh, [(200, 120, 192)]), synth.face_frame(sw, sh, [(60, 40, 150), (330, 200, 220)])])
        b = np.stack([synth.face_frame(sw, sh, [(300, 200, 240)]), ic.smooth(sw, sh, 3)])
        wa = np.stack([ic.expected(a[f], None, dw, dh) for f in range(n)])
        wb = np.stack([ic.expected(b[f], None, dw, dh) for f in range(n)])
        ha = hb = None
        for rnd in range(6):
            src, want = (a, wa) if rnd % 2 == 0 else (b, wb)
            c.draw_frames(src)
            hits, _ = hits_of(c, cascade, want)
            if rnd == 0:
                ha = hits.copy()
            if rnd == 1:
                hb = hits.copy()
        assert len(ha) > 0 and len(hb) > 0 and (len(ha) != len(hb) or not np.array_equal(ha["sum"], hb["sum"]))  # the contents do differ
        assert c.graph_launches >= 4, c.graph_launches  # rounds 1 .. 5 were replays (round 1 captures and launches)
    finally:
        c.close()


def test_draw_and_enqueue_only_track_keep_their_order():
    """draw -> enqueue-only track -> draw -> enqueue-only track -> collect twice: the second draw overwrites the buffer the first track
    step reads, and is ordered behind it on the context's stream — both steps return the oracle's objects for THEIR frames"""
    (sw, sh), (dw, dh), n = (640, 480), (320, 240), 2
    c = Context()
    try:
        c.set_geometry(dw, dh, n)
        c.camshift_reserve(n)
        vids = [np.stack([synth.blob_frame(sw, sh, 300 + 40 * f + 6 * k, 220 + 4 * k, 90, 50, (4, 3, 5), (200, 60, 40), seed=60 + 5 * f + k) for f in range(n)])
                for k in range(3)]
        want = [np.stack([ic.expected(v[f], None, dw, dh) for f in range(n)]) for v in vids]
        rects = [(105 + 20 * f, 85, 90, 50) for f in range(n)]
        c.draw_frames(vids[0])
        c.camshift_init(rects)
        oracles = []
        for f in range(n):
            o = ho.Camshift(True)
            o.init_tracker(want[0][f], rects[f])
            oracles.append(o)
        for k in (1, 2):
            c.draw_frames(vids[k])
            c.camshift_track(n, calc_angles=True, fetch=False)
        stats = []
        for k in (1, 2):
            got = c.camshift_track_collect(n)
            for f in range(n):
                sw_, to = oracles[f].track(want[k][f])
                cs_check(got[f], sw_, to, stats, where=("order", f, k))
        cs_all_exact(stats, "draw / enqueue-only track order")
    finally:
        c.close()


# ---- the reference's recorded canvases, end to end -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ic.golden()["cases"], ids=lambda c: c["name"])
def test_golden_cases_end_to_end(ctx, case, cascade):
    """every video frame of a recorded case is drawn on the device and read by the facetrackr sequence on the device (detect ->
    floor the best face -> initTracker -> track, facetrackr.js:97-108, 185-217).  The CRC-32 of every device-drawn canvas (device form,
    read back whole) is the one the unmodified reference's drawImage left, the bind form holds the same frame (see bound_equals), the VJ
    frame's best face equals the recorded
    tracking object exactly and every CS frame's object matches under the criteria of tests/test_gpu_camshift.py."""
    vw, vh, w, h = case["vw"], case["vh"], case["w"], case["h"]
    ctx.set_geometry(w, h, 1)
    ctx.camshift_reserve(1)
    stats, tracking = [], False
    for k, call in enumerate(case["calls"]):
        video = ic.golden_video(case, k)
        want = ic.expected(video, None, w, h)
        # the canvas as the DEVICE drew it, all four channels of every pixel: its CRC-32 is the one the reference's own drawImage left
        got, _ = draw_device(ctx, video[None], w, h)
        assert ic.crc(got[0]) == call["canvas_crc"], (case["name"], k)
        same(got[0], want, f"{case['name']} frame {k}")
        ctx.draw_frames(video[None])
        if call["detection"] == "WB":  # the full loop's whitebalance phase: the canvas only
            bound_equals(ctx, want[None], f"{case['name']} frame {k}")
            continue
        if call["detection"] == "VJ":
            assert not tracking
            bound_equals(ctx, want[None], f"{case['name']} frame {k}")
            hits, counts = hits_of(ctx, cascade, want[None])
            best = ctx.best_faces(hits, counts, 1)[0]
            if "confidence" in call:  # (the full loop announces its VJ frame by a status event only: its rect is not observable)
                for key in ("x", "y", "width", "height", "confidence"):
                    assert best[key] == call[key], (case["name"], k, key, best, call)
            assert best["confidence"] > -10
            ctx.camshift_init([[math.floor(best["x"]), math.floor(best["y"]), math.floor(best["width"]), math.floor(best["height"])]])
            tracking = True
            continue
        assert tracking
        got = ctx.camshift_track(1, calc_angles=True)[0]
        assert call["detection"] == "CS"
        for key in ("x", "y"):
            assert abs(float(got[key]) - call[key]) <= 1, (case["name"], k, key)
        for key in ("width", "height"):
            assert float(got[key]) == call[key] and call[key] > 0, (case["name"], k, key)
        d = abs(float(got["angle"]) - call["angle"])
        assert min(d, abs(d - math.pi)) <= ANGLE_TOL, (case["name"], k)
        stats.append(all(float(got[key]) == call[key] for key in ("x", "y", "width", "height")))
    assert tracking and len(stats) >= 3 and sum(stats) == len(stats), (case["name"], stats)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------

def test_error_statuses_leave_the_context_usable(cascade):
    (sw, sh), (dw, dh), n = (64, 48), (40, 30), 2
    src = ic.frames_of("noise", sw, sh, n, seed=9)
    want = np.stack([ic.expected(src[f], None, dw, dh) for f in range(n)])
    c = Context()
    dsrc = DeviceArray(src)
    ddst = DeviceArray(np.zeros(4 * n * dw * dh * 4, dtype=np.uint8))
    L, h = c._lib, c._h
    fb = dw * dh * 4

    def dev(ptr=None, n_=n, w=sw, h_=sh, pitch=0, stride=0, rect=None, dst=ddst.ptr, dstride=0):
        r = Context._cs_rect(rect)
        return L.ht_draw_frames_device(h, dsrc.ptr if ptr is None else ptr, n_, w, h_, pitch, stride, r.ctypes.data if r is not None else None, dst, dstride)

    def host(ptr=src.ctypes.data, n_=n, w=sw, h_=sh, stride=0, rect=None):
        r = Context._cs_rect(rect)
        return L.ht_draw_frames(h, ptr, n_, w, h_, stride, r.ctypes.data if r is not None else None)

    try:
        assert dev() == HT_ERR_STATE and host() == HT_ERR_STATE  # no geometry yet
        assert b"ht_set_geometry" in L.ht_last_error(h)
        c.set_geometry(dw, dh, n)
        c.draw_frames(src)
        bound_equals(c, want, "before the failing calls")
        bad = [
            ("NULL source", lambda: dev(ptr=0)), ("NULL host source", lambda: host(ptr=None)),
            ("misaligned source", lambda: dev(ptr=dsrc.ptr + 2)), ("misaligned destination", lambda: dev(dst=ddst.ptr + 1)),
            ("pitch not a multiple of 4", lambda: dev(pitch=sw * 4 + 2)), ("pitch smaller than a row", lambda: dev(pitch=sw * 4 - 4)),
            ("source stride not a multiple of 4", lambda: dev(stride=sw * sh * 4 + 2)), ("source stride too small", lambda: dev(stride=sw * sh * 4 - 4)),
            ("host source stride too small", lambda: host(stride=sw * sh * 4 - 1)),
            ("destination stride too small", lambda: dev(dstride=fb - 4)), ("destination stride not a multiple of 4", lambda: dev(dstride=fb + 2)),
            ("n = 0", lambda: dev(n_=0)), ("n < 0", lambda: host(n_=-1)),
            ("n above the batch capacity, bind form", lambda: dev(n_=n + 1, dst=None)), ("n above the batch capacity, host form", lambda: host(n_=n + 1)),
            ("zero width", lambda: dev(w=0)), ("negative height", lambda: host(h_=-3)),
            ("rect beyond the right edge", lambda: dev(rect=(10, 0, sw - 9, sh))), ("rect beyond the bottom edge", lambda: host(rect=(0, 1, sw, sh))),
            ("rect with a negative origin", lambda: dev(rect=(-1, 0, 8, 8))), ("empty rect", lambda: host(rect=(0, 0, 0, 5))),
            ("destination inside the source", lambda: dev(dst=dsrc.ptr + 4 * sw)),
            ("source inside the destination", lambda: dev(ptr=ddst.ptr + fb, dst=ddst.ptr, dstride=2 * fb)),
        ]
        for what, call in bad:
            assert call() == HT_ERR_INVALID, what
            assert len(L.ht_last_error(h)) > 10, what
            assert L.ht_frames_bound(h) == n, what  # binding untouched
            assert dev() == 0, what  # ... and the next call on the same context succeeds
            same(c.device_download(ddst.ptr, n * fb).reshape(n, dh, dw, 4), want, f"draw after: {what}")
        # (a source inside the context's OWN frame buffer is refused by the same interval test as the two overlaps above; the library
        # hands that buffer's address to nobody, so no caller — this test included — can name a pointer into it)
        bound_equals(c, want, "after the failing calls")  # frames and every stage still work
        assert dev() == 0  # and a successful call on the same context
        c.synchronize()
        got = d2h(ddst.ptr, n * fb).reshape(n, dh, dw, 4)
        same(got, want, "device form after the failing calls")
        assert L.ht_frames_bound(h) == n
    finally:
        c.close()
        dsrc.free()
        ddst.free()


def test_every_refusal_of_the_draw_calls_is_the_recorded_one():
    """tests/draw_refusal_cases.py's table — every refusal of the six canvas-draw entry points, the adjacent double faults that pin each
    call's check order, ht_set_geometry not yet called — replayed on the built library: status and ht_last_error text equal
    tests/golden/draw_call_refusals.json, which was recorded before the calls' host path was written once.  No kernel runs."""
    import draw_refusal_cases as drc

    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "draw_call_refusals.json")))
    got = drc.replay()
    assert got["canvas"] == golden["canvas"]
    assert sorted(got["cases"]) == sorted(golden["cases"]) and len(golden["cases"]) >= 180
    for key, want in golden["cases"].items():
        assert got["cases"][key] == want, (key, got["cases"][key], want)
    assert all(st in (HT_ERR_INVALID, HT_ERR_STATE) and len(text) > 10 for st, text in golden["cases"].values())


# ---- Node ----------------------------------------------------------------------------------------------------------------------------------

def test_node_facade_draws_on_the_device(tmp_path):
    """tests/js/ingest_gpu.js: the addon's drawFrames / drawFramesDevice and ccv.DeviceBatch's uploadSource / draw / drawBound followed by
    detectStep / trackStep, against expectations computed here (the oracle on `expected`)"""
    from headtrackr_amd import build

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    (sw, sh), (dw, dh), n, steps = (640, 480), (320, 240), 2, 4
    vids = [np.stack([synth.face_frame(sw, sh, [(200 + 30 * f + 3 * k, 120 + 2 * k, 192)]) for f in range(n)]) for k in range(steps)]
    want = [np.stack([ic.expected(v[f], None, dw, dh) for f in range(n)]) for v in vids]
    rect = (40, 30, 560, 420)
    want_rect = np.stack([ic.expected(vids[0][f], rect, dw, dh) for f in range(n)])
    from headtrackr_amd.cascade import load_cascade

    blob = load_cascade().blob
    best = ho.best_faces(want[0], blob, 1)
    rects = [[int(math.floor(best[k][f])) for k in ("x", "y", "width", "height")] for f in range(n)]
    tracks = []
    oracles = []
    for f in range(n):
        o = ho.Camshift(True)
        o.init_tracker(want[0][f], rects[f])
        oracles.append(o)
    for k in range(1, steps):
        tracks.append([dict(oracles[f].track(want[k][f])[1], sw=oracles[f].search_window()) for f in range(n)])
    for k, v in enumerate(vids):
        v.tofile(tmp_path / f"video{k}.raw")
    job = dict(sw=sw, sh=sh, w=dw, h=dh, n=n, steps=steps, dir=str(tmp_path), rect=list(rect),
               gray_crc=[ic.crc(ho.grayscale_rgba(want[0][f])[..., 0]) for f in range(n)],
               best=[{k: float(best[k][f]) for k in ("x", "y", "width", "height", "confidence")} for f in range(n)],
               best_rect=[{k: float(b[k]) for k in ("x", "y", "width", "height", "confidence")} for b in ho.best_faces(want_rect, blob, 1)],
               rects=rects, tracks=tracks, wb=[ho.whitebalance(want[0][f]) for f in range(n)], wb_rect=[ho.whitebalance(want_rect[f]) for f in range(n)])
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "ingest_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ingest_gpu: ok" in r.stdout, r.stdout[-2000:]

"""The device back-projection (ht_camshift_backproject / _device; camshift.js:172-196, 314-353) against the reference's recorded bytes
and against tests/bp_cases.py's binary64 restatement of the reference formulas (itself pinned to those bytes by
tests/test_backproject_cpu.py).  Every operation is an integer operation or one correctly rounded binary64 operation, so there is no
tolerance anywhere: every comparison is equality of every byte of every pixel."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bp_cases
import cs_cases
from conftest import ROOT
from headtrackr_amd import synth
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray, _rt
from test_gpu_camshift import SCHEDULES

pytestmark = pytest.mark.gpu

KINDS = ("rgba8", "f64")
EXTRA_SIZES = [(97, 81), (131, 99), (333, 217), (511, 97), (40, 30), (23, 23)]  # tests/test_gpu_sizes.py


def same(got, want, what):
    """byte equality of whole arrays (float64 compared as bit patterns), with the first difference in the message"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    a, b = got.view(np.uint8).reshape(-1), want.view(np.uint8).reshape(-1)
    if not np.array_equal(a, b):
        bad = np.flatnonzero(a != b)
        i = int(bad[0]) // got.dtype.itemsize
        raise AssertionError(f"{what}: {len(bad)} bytes differ; first at element {i}: got {got.reshape(-1)[i]!r}, want {want.reshape(-1)[i]!r}")


def both_kinds(ctx, n, first, want, what):
    """want: [(rgba, pdf)] per frame"""
    same(ctx.camshift_backproject(n, first=first, kind="rgba8"), np.stack([w[0] for w in want]), f"{what} rgba8")
    same(ctx.camshift_backproject(n, first=first, kind="f64"), np.stack([w[1] for w in want]), f"{what} f64")


def d2h(ptr, nbytes):
    out = np.empty(nbytes, dtype=np.uint8)
    assert _rt().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


# ---- the reference's own bytes ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=list(SCHEDULES))
def ctx(request):
    """the four track schedules of tests/test_gpu_camshift.py: the back-projection must not depend on which track path ran before it"""
    c = Context(options=SCHEDULES[request.param])
    yield c
    c.close()


@pytest.mark.parametrize("case", bp_cases.golden_cases(), ids=lambda c: c["name"])
def test_golden_cases_give_the_reference_recorded_bytes(ctx, case):
    """init, replay the case's track() calls (the stream has real tracker state), back-project the last tracked frame: the CRC-32 of
    the RGBA8 bytes is the reference's `backprojection_crc`, the binary64 output at `pdf_samples` the recorded values, and both whole
    outputs the expectation"""
    w, h = case["w"], case["h"]
    frames = bp_cases.golden_frames(case["name"])
    ctx.set_geometry(w, h, 1)
    ctx.camshift_reserve(1)
    ctx.upload(frames[0][None])
    ctx.camshift_init([case["rect"]])
    for call in case["calls"]:
        ctx.upload(frames[call["frame"]][None])
        ctx.camshift_track(1, calc_angles=case["calcAngles"])
    rgba = ctx.camshift_backproject(1, kind="rgba8")
    pdf = ctx.camshift_backproject(1, kind="f64")
    assert rgba.shape == (1, h, w, 4) and rgba.dtype == np.uint8 and pdf.shape == (1, h, w) and pdf.dtype == np.float64
    assert bp_cases.crc(rgba[0]) == case["backprojection_crc"]
    for x, y, v in case["pdf_samples"]:
        assert pdf[0, y, x] == v, (case["name"], x, y, pdf[0, y, x], v)
    want_rgba, want_pdf = bp_cases.golden_expected(case["name"])
    same(rgba[0], want_rgba, case["name"] + " rgba8")
    same(pdf[0], want_pdf, case["name"] + " f64")


# ---- sizes and content ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", cs_cases.HIST_SIZES + EXTRA_SIZES, ids=lambda v: str(v))
def test_sizes_families_and_stream_ranges(w, h):
    """Pixel counts on both sides of the chunking and of the 4-pixel quantum (an odd W*H puts the second frame of a packed batch on a
    4-byte boundary, on the input and on the output side), flat / noise / run-structured content, model rects that cross every border,
    three streams per call at first > 0 inside a larger reservation, and a reservation that grows between two calls (the old streams'
    models move to the new state block; streams behind them are initialised afterwards)."""
    border = cs_cases.init_border_rects()
    n = 3
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(5)
        for fi, family in enumerate(cs_cases.HIST_FAMILIES):
            a = np.stack([cs_cases.hist_frame(family, w, h, 10 * fi + s) for s in range(n)])       # models come from these ...
            b = np.stack([cs_cases.hist_frame(family, w, h, 10 * fi + s + 4) for s in range(n)])   # ... and these are projected (flat: same colours)
            rects = [border[(3 * fi) % len(border)], border[(3 * fi + 1) % len(border)], (w // 4, h // 4, max(w // 2, 1), max(h // 2, 1))]
            models = [bp_cases.model_of(a[s], rects[s]) for s in range(n)]
            first = 2
            c.upload(a)
            c.camshift_init(rects, first=first)
            both_kinds(c, n, first, [bp_cases.expected(models[s], a[s]) for s in range(n)], f"{w}x{h} {family} own frames")
            c.upload(b)
            both_kinds(c, n, first, [bp_cases.expected(models[s], b[s]) for s in range(n)], f"{w}x{h} {family} other frames")
            if fi == 0:
                # never initialised streams [0, 2) + stream 2: all-zero models give all-zero weights (defined behaviour)
                zero = np.zeros(4096, dtype=np.int64)
                both_kinds(c, n, 0, [bp_cases.expected(zero, b[0]), bp_cases.expected(zero, b[1]), bp_cases.expected(models[0], b[2])],
                           f"{w}x{h} {family} uninitialised streams")
                c.camshift_reserve(12)  # grows: streams 2..4 keep their models
                both_kinds(c, n, first, [bp_cases.expected(models[s], b[s]) for s in range(n)], f"{w}x{h} {family} after the reservation grew")
                c.upload(a)
                c.camshift_init(rects, first=9)
                c.upload(b)
                both_kinds(c, n, 9, [bp_cases.expected(models[s], b[s]) for s in range(n)], f"{w}x{h} {family} new streams 9..11")
                # one frame of the batch through one stream of the range
                same(c.camshift_backproject(1, first=10, kind="rgba8")[0], bp_cases.expected(models[1], b[0])[0], f"{w}x{h} n = 1")
    finally:
        c.close()


# ---- the benchmark's shapes -------------------------------------------------------------------------------------------------------------

def test_c5_shape_eight_1080p_feeds():
    w, h, n = 1920, 1080, 8
    uniq = synth.stream_feed_frames(n + 1, w, h, 0)
    rects = [(700 + 3 * k, 300 + k, 360, 360) for k in range(n)]
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.upload(uniq[:n])
        c.camshift_init(rects)
        c.upload(uniq[1:])
        c.camshift_track(n, calc_angles=True)
        want = [bp_cases.expected(bp_cases.model_of(uniq[s], rects[s]), uniq[s + 1]) for s in range(n)]
        assert all(len(np.unique(wr[..., 0])) >= 2 for wr, _ in want)  # the feeds are a face on a flat background: few values, not one
        both_kinds(c, n, 0, want, "8 x 1080p")
    finally:
        c.close()


def c3_streams(nuniq=16, steps=4):
    """[(frames of every step, init rect)] of nuniq distinct 320x240 trackers (tests/cs_cases.py stream_seq)"""
    seqs = [cs_cases.stream_seq("bp", s, steps) for s in range(nuniq)]
    return [(s.frames, s.rect) for s in seqs]


def test_c3_shape_256_streams():
    w, h, n = 320, 240, 256
    uniq = c3_streams()
    frames0 = np.stack([uniq[s % len(uniq)][0][0] for s in range(n)])
    frames1 = np.stack([uniq[s % len(uniq)][0][1] for s in range(n)])
    rects = [uniq[s % len(uniq)][1] for s in range(n)]
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.upload(frames0)
        c.camshift_init(rects)
        c.upload(frames1)
        c.camshift_track(n, calc_angles=True)
        wu = [bp_cases.expected(bp_cases.model_of(uniq[s][0][0], uniq[s][1]), uniq[s][0][1]) for s in range(len(uniq))]
        both_kinds(c, n, 0, [wu[s % len(uniq)] for s in range(n)], "256 x 320x240")
    finally:
        c.close()


# ---- device output ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,n", [(320, 240, 5), (65, 63, 3)], ids=["320x240", "odd-65x63"])
@pytest.mark.parametrize("kind", KINDS)
def test_device_form_writes_the_frames_and_nothing_else(w, h, n, kind):
    """the _device form into a sentinel-filled buffer with a stride larger than a frame, at an offset that is a multiple of the element
    size only: the frames equal the host form's, every gap, the bytes in front of the first and behind the last frame keep the sentinel"""
    elem = 8 if kind == "f64" else 4
    fb, lead = w * h * elem, 3 * elem
    stride, tail = fb + 5 * elem, 4096
    frames = np.stack([cs_cases.hist_frame("blocks", w, h, 40 + s) for s in range(n)])
    rects = [(w // 4, h // 4, w // 2, h // 2)] * n
    c = Context()
    buf = DeviceArray(np.full(lead + n * stride + tail, 0xA5, dtype=np.uint8))
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n + 2)
        c.upload(frames)
        c.camshift_init(rects, first=2)
        want = c.camshift_backproject(n, first=2, kind=kind)
        same(want, np.stack([bp_cases.expected(bp_cases.model_of(frames[s], rects[s]), frames[s])[0 if kind == "rgba8" else 1] for s in range(n)]), "host form")
        c.camshift_backproject_device(buf.ptr + lead, n, first=2, kind=kind, stride=stride)
        c.synchronize()
        got = d2h(buf.ptr, buf.nbytes)
        assert (got[:lead] == 0xA5).all()
        for s in range(n):
            o = lead + s * stride
            same(got[o:o + fb], want[s].view(np.uint8).reshape(-1), f"device frame {s}")
            assert (got[o + fb:o + stride] == 0xA5).all(), f"gap behind frame {s}"
        assert (got[lead + n * stride:] == 0xA5).all()
        # packed (stride 0)
        c.camshift_backproject_device(buf.ptr, n, first=2, kind=kind)
        c.synchronize()
        same(d2h(buf.ptr, n * fb), want.view(np.uint8).reshape(-1), "device form, packed")
    finally:
        c.close()
        buf.free()


# ---- non-interference -------------------------------------------------------------------------------------------------------------------

def _track_run(options, w, h, step_frames, rects, interleave, keep_hist_stream):
    """init on step 0, then one enqueue-only track step per later entry of step_frames with up to two outstanding; with `interleave`,
    back-projection calls of both kinds (host and device form) sit between the steps — also while two track steps are outstanding, and
    once more after the last step on other frames.  Returns (track objects per step, stats, debug histogram of one stream)."""
    n = len(rects)
    c = Context(options=options)
    dev = [DeviceArray(f) for f in step_frames]
    scratch = DeviceArray(np.zeros(n * w * h * 8, dtype=np.uint8)) if interleave else None
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)
        if interleave:
            c.camshift_backproject(n, kind="rgba8")
        c.camshift_stats(n, reset=True)
        out, pend, bps = [], 0, 0
        for i in range(1, len(dev)):
            c.bind_device(dev[i].ptr, n)
            c.camshift_track(n, calc_angles=True, fetch=False)
            pend += 1
            if interleave:
                if pend == 2:  # two enqueue-only track steps outstanding in the ring
                    kind = KINDS[bps % 2]
                    got = c.camshift_backproject(n, kind=kind)
                    assert got.shape[0] == n
                    c.camshift_backproject_device(scratch.ptr, n, kind=KINDS[(bps + 1) % 2])
                    bps += 1
                elif i % 2:
                    c.camshift_backproject_device(scratch.ptr, n, kind="f64")
            if pend == 2:
                out.append(c.camshift_track_collect(n).copy())
                pend -= 1
        while pend:
            out.append(c.camshift_track_collect(n).copy())
            pend -= 1
        if interleave:
            assert bps >= 2
            c.bind_device(dev[0].ptr, n)  # other frames than the last track call's
            c.camshift_backproject(n, kind="f64")
            c.camshift_backproject(max(n // 2, 1), first=0, kind="rgba8")
        stats = c.camshift_stats(n, reset=False)
        hist = c.camshift_debug_hist(keep_hist_stream)
        return out, stats, hist
    finally:
        c.close()
        for d in dev:
            d.free()
        if scratch:
            scratch.free()


def _assert_same_runs(plain, mixed, last_frame_of_stream, what):
    (oa, sa, ha), (ob, sb, hb) = plain, mixed
    assert len(oa) == len(ob) > 0
    for k, (a, b) in enumerate(zip(oa, ob)):
        assert a.tobytes() == b.tobytes(), f"{what}: track objects of step {k + 1} differ"
        assert (a["width"] > 0).all(), f"{what}: a tracker lost its target (the sequence must exercise real tracking)"
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]), f"{what}: camshift_stats differ"
    assert np.array_equal(ha[0], hb[0]), f"{what}: model histogram"
    assert np.array_equal(ha[1], hb[1]), f"{what}: debug histogram differs between the runs"
    assert np.array_equal(hb[1], cs_cases.frame_histogram(last_frame_of_stream)), f"{what}: debug histogram is not the last TRACK call's"


def test_back_projection_leaves_the_cluster_track_path_alone():
    """C5 style: 8 x 1080p feeds, cluster mean-shift (LUT + exchange slots in d_cs_lut / d_cs_parts, results in the pinned ring)"""
    w, h, n, steps = 1920, 1080, 8, 6
    uniq = synth.stream_feed_frames(steps + n, w, h, 0)
    step_frames = [np.stack([uniq[k + f] for f in range(n)]) for k in range(steps)]
    rects = [(700 + 3 * f, 300 + f, 360, 360) for f in range(n)]
    plain = _track_run(None, w, h, step_frames, rects, False, 3)
    mixed = _track_run(None, w, h, step_frames, rects, True, 3)
    _assert_same_runs(plain, mixed, step_frames[-1][3], "cluster path")


def test_back_projection_leaves_the_fused_track_path_alone():
    """C3 style: 256 x 320x240 streams, the single-launch kernel; cs_keep_hist=1 makes it write the histogram ht_camshift_debug_hist reads"""
    w, h, n, steps = 320, 240, 256, 5
    uniq = c3_streams(16, steps - 1)
    step_frames = [np.stack([uniq[s % 16][0][k] for s in range(n)]) for k in range(steps)]
    rects = [uniq[s % 16][1] for s in range(n)]
    plain = _track_run("cs_keep_hist=1", w, h, step_frames, rects, False, 37)
    mixed = _track_run("cs_keep_hist=1", w, h, step_frames, rects, True, 37)
    _assert_same_runs(plain, mixed, step_frames[-1][37], "fused path")


# ---- errors -----------------------------------------------------------------------------------------------------------------------------

def test_bad_calls_are_status_codes_and_the_context_survives():
    INVALID, STATE = -1, -6
    w, h, n = 64, 48, 2
    frames = np.stack([cs_cases.hist_frame("noise", w, h, 70 + s) for s in range(n)])
    rects = [(10, 10, 30, 20)] * n
    c = Context()
    buf = DeviceArray(np.zeros(n * w * h * 8 + 64, dtype=np.uint8))
    host = np.zeros(n * w * h * 8, dtype=np.uint8)
    L, H = c._lib, c._h

    def st(fn, *a):
        return getattr(L, fn)(H, *a)

    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        # nothing bound
        assert st("ht_camshift_backproject", 0, 1, 0, host.ctypes.data, 0) == STATE
        assert st("ht_camshift_backproject_device", 0, 1, 0, buf.ptr, 0) == STATE
        c.upload(frames)
        c.camshift_init(rects)
        for fn, out in (("ht_camshift_backproject", host.ctypes.data), ("ht_camshift_backproject_device", buf.ptr)):
            assert st(fn, 0, n, 0, None, 0) == INVALID                       # NULL output
            assert getattr(L, fn)(None, 0, n, 0, out, 0) == INVALID          # NULL context
            assert st(fn, 0, n, 2, out, 0) == INVALID                        # unknown kind
            assert st(fn, 0, n, -1, out, 0) == INVALID
            assert st(fn, 0, n + 1, 0, out, 0) == STATE                      # more than the bound frames
            assert st(fn, 0, 0, 0, out, 0) == STATE
            assert st(fn, 1, n, 0, out, 0) == INVALID                        # stream range not reserved
            assert st(fn, -1, n, 0, out, 0) == INVALID
            assert st(fn, 0, n, 0, out, w * h * 4 - 4) == INVALID            # stride shorter than a frame
            assert st(fn, 0, n, 1, out, w * h * 8 - 8) == INVALID
        assert st("ht_camshift_backproject_device", 0, n, 0, buf.ptr, w * h * 4 + 2) == INVALID  # stride not a multiple of the element size
        assert st("ht_camshift_backproject_device", 0, n, 1, buf.ptr, w * h * 8 + 4) == INVALID
        assert st("ht_camshift_backproject_device", 0, n, 0, buf.ptr + 2, 0) == INVALID          # pointer likewise
        assert st("ht_camshift_backproject_device", 0, n, 1, buf.ptr + 4, 0) == INVALID
        with pytest.raises(HtError) as e:
            c.camshift_backproject(n, kind=2)
        assert e.value.status == INVALID and "kind" in str(e.value)
        # the host form takes any stride >= a frame (it is applied by the copy)
        padded = np.full((n, w * h * 4 + 6), 0x5A, dtype=np.uint8)
        assert st("ht_camshift_backproject", 0, n, 0, padded.ctypes.data, padded.shape[1]) == 0
        want = [bp_cases.expected(bp_cases.model_of(frames[s], rects[s]), frames[s]) for s in range(n)]
        for s in range(n):
            same(padded[s, :w * h * 4], want[s][0].reshape(-1), "host form with a padded stride")
            assert (padded[s, w * h * 4:] == 0x5A).all()
        # and the context still works
        both_kinds(c, n, 0, want, "after the refused calls")
        assert (c.camshift_track(n)["width"] >= 0).all()
    finally:
        c.close()
        buf.free()


# ---- the Node host ----------------------------------------------------------------------------------------------------------------------

def test_node_facade_takes_the_device_route(tmp_path):
    """tests/js/backproject_gpu.js: DeviceBatch.backProjection for two frame sets x both kinds equals raw files written here from the
    expectation; camshift.Tracker.getBackProjectionImg() through the real addon gives the reference's CRC for the six 320x240 / 720p
    golden cases and went through camshiftBackProject (the script wraps the addon's function and counts)"""
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr_hip.node")):
        pytest.skip("node or the addon is missing")
    w, h, n = 320, 240, 4
    uniq = c3_streams(n, 2)
    rects = [uniq[s][1] for s in range(n)]
    sets = [np.stack([uniq[s][0][k] for s in range(n)]) for k in range(3)]
    job = {"w": w, "h": h, "n": n, "rects": [int(v) for r in rects for v in r], "sets": [], "expect": [], "golden": []}
    for k, fr in enumerate(sets):
        p = tmp_path / f"set{k}.raw"
        fr.tofile(p)
        job["sets"].append(str(p))
    for k in (1, 2):
        want = [bp_cases.expected(bp_cases.model_of(sets[0][s], rects[s]), sets[k][s]) for s in range(n)]
        pr, pf = tmp_path / f"want{k}.rgba8", tmp_path / f"want{k}.f64"
        np.stack([x[0] for x in want]).tofile(pr)
        np.stack([x[1] for x in want]).tofile(pf)
        job["expect"].append({"set": k, "rgba8": str(pr), "f64": str(pf)})
    for case in bp_cases.golden_cases():
        if case["w"] * case["h"] > 1280 * 720:
            continue
        files = []
        for i, f in enumerate(bp_cases.golden_frames(case["name"])):
            p = tmp_path / f"{case['name']}_{i}.raw"
            f.tofile(p)
            files.append(str(p))
        job["golden"].append({"name": case["name"], "w": case["w"], "h": case["h"], "rect": case["rect"], "calcAngles": case["calcAngles"],
                              "frames": files, "calls": [c["frame"] for c in case["calls"]], "crc": case["backprojection_crc"]})
    assert len(job["golden"]) == 6
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "backproject_gpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["batch_checks"] == 4 and out["golden_checks"] == 6
    assert out["device_calls"] == 6 + 4 + 1, out  # one per getBackProjectionImg, one per DeviceBatch.backProjection (+ the set = -1 call)

"""The back-projection over (stream, frame) pairs (ht_camshift_backproject_pairs / _device) against tests/bp_cases.py's binary64
restatement of the reference (pinned to the reference's recorded bytes by tests/test_bp_pairs_cpu.py and tests/test_backproject_cpu.py),
against the reference's recorded CRCs of tests/golden/multitrack_bp.json, and against ht_camshift_backproject on replicated frames.
Integer operations and single correctly rounded binary64 operations only: every comparison is equality of every byte."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bp_cases
import cs_cases
import pair_cases as pc
from conftest import ROOT, load_golden
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from test_gpu_backproject import d2h, same

pytestmark = pytest.mark.gpu

KINDS = ("rgba8", "f64")
GROUP = {"rgba8": 4, "f64": 2}  # pairs that share one pass over a frame (LUTs of a k_bpp_project workgroup)
KIND_ID = {"rgba8": 0, "f64": 1}
INVALID, STATE = -1, -6
# pixel counts 4096, 4095 (one chunk, with and without a tail), 16384, 16385 (one and two chunks) and an odd W * H (output i on a 4-byte boundary)
SIZES = [(64, 64), (65, 63), (128, 128), (145, 113), (23, 23)]


def sel(want, kind):
    return want[0] if kind == "rgba8" else want[1]


def golden_sequences():
    return {s.name: s for s in (pc.feed_scene(0), pc.same_colour(320, 240))}


@functools.lru_cache(maxsize=None)
def seq_models(name):
    s = golden_sequences()[name]
    return [bp_cases.model_of(s.frames[0], s.rects[j]) for j in range(s.ntrackers)]


@functools.lru_cache(maxsize=None)
def seq_expected(name, j, k):
    """(rgba, pdf) of frame k of the sequence through tracker j's model"""
    return bp_cases.expected(seq_models(name)[j], golden_sequences()[name].frames[k])


# ---- pixel-count and group boundaries ---------------------------------------------------------------------------------------------------

def boundary_layout(kind, seed):
    """pairs per frame 1, G, G + 1, 2 G + 1 on bound frames 4, 0, 5, 2 of six (1 and 3 are named by no pair), streams scattered inside a
    reservation of 40, pair order shuffled: [(stream, frame, rect index)]"""
    g = GROUP[kind]
    per_frame = {4: 1, 0: g, 5: g + 1, 2: 2 * g + 1}
    flat = [(f, r % 3) for f, cnt in per_frame.items() for r in range(cnt)]
    streams = pc.scattered_streams(len(flat), 40, seed)
    order = pc.shuffled(len(flat), seed + 1)
    return [(streams[i], flat[i][0], flat[i][1]) for i in order]


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_pixel_count_and_group_boundaries(w, h):
    nb = 6
    rects = [(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)), (0, 0, max(w // 3, 1), h), (w // 2, h // 3, w // 2, max(h // 2, 1))]
    c, c2 = Context(), Context()
    try:
        c.set_geometry(w, h, nb)
        c.camshift_reserve(40)
        for fi, family in enumerate(cs_cases.HIST_FAMILIES):
            a = np.stack([cs_cases.hist_frame(family, w, h, 10 * fi + s) for s in range(nb)])           # models come from these ...
            b = np.stack([cs_cases.hist_frame(family, w, h, 10 * fi + (s + 3) % nb) for s in range(nb)])  # ... and these are projected
            models, wants = {}, {}
            for kind in KINDS:
                lay = boundary_layout(kind, 9400 + 10 * fi + KIND_ID[kind])
                pairs = [(s, f) for s, f, _r in lay]
                assert sorted(set(f for _s, f in pairs)) == [0, 2, 4, 5] and pairs != [(pairs[0][0] + i, i) for i in range(len(pairs))]
                c.upload(a)
                c.camshift_init_pairs(pairs, [rects[r] for _s, _f, r in lay])
                c.upload(b)
                got = c.camshift_backproject_pairs(pairs, kind=kind)
                want = []
                for _s, f, r in lay:
                    if (f, r) not in models:
                        models[(f, r)] = bp_cases.model_of(a[f], rects[r])
                        wants[(f, r)] = bp_cases.expected(models[(f, r)], b[f])
                    want.append(sel(wants[(f, r)], kind))
                same(got, np.stack(want), f"{w}x{h} {family} {kind}")
                # the batch call on the frames replicated per pair
                n = len(lay)
                c2.set_geometry(w, h, n)
                c2.camshift_reserve(n)
                c2.upload(np.stack([a[f] for _s, f, _r in lay]))
                c2.camshift_init([rects[r] for _s, _f, r in lay])
                c2.upload(np.stack([b[f] for _s, f, _r in lay]))
                same(got, c2.camshift_backproject(n, kind=kind), f"{w}x{h} {family} {kind} against replicated frames")
    finally:
        c.close()
        c2.close()


# ---- the reference's recorded values ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", load_golden("multitrack_bp.json")["cases"], ids=lambda c: c["name"])
def test_golden_sequences_after_every_call(case):
    """the trackers of one canvas track (ht_camshift_track_pairs) and are back-projected after every call, in ONE pair call per kind: the
    CRC-32 of every tracker's RGBA8 output and its binary64 output at the recorded points are the reference's"""
    s = golden_sequences()[case["name"]]
    m = s.ntrackers
    streams = pc.scattered_streams(m, 7, 9600)
    pairs = [(streams[j], 0) for j in range(m)]
    c = Context()
    try:
        c.set_geometry(s.w, s.h, 1)
        c.camshift_reserve(7)
        c.upload(s.frames[0][None])
        c.camshift_init_pairs(pairs, s.rects)
        for k in range(1, s.ncalls + 1):
            c.upload(s.frames[k][None])
            got = c.camshift_track_pairs(pairs)
            assert (got["width"] > 0).all()
            rgba = c.camshift_backproject_pairs(pairs, kind="rgba8")
            pdf = c.camshift_backproject_pairs(pairs, kind="f64")
            assert rgba.shape == (m, s.h, s.w, 4) and rgba.dtype == np.uint8 and pdf.shape == (m, s.h, s.w) and pdf.dtype == np.float64
            for j in range(m):
                rec = case["trackers"][j][k - 1]
                assert rec["frame"] == k
                assert bp_cases.crc(rgba[j]) == rec["crc"], (case["name"], j, k)
                for x, y, v in rec["pdf"]:
                    assert pdf[j, y, x] == v, (case["name"], j, k, x, y, pdf[j, y, x], v)
                same(rgba[j], seq_expected(case["name"], j, k)[0], f"{case['name']} tracker {j} call {k} rgba8")
                same(pdf[j], seq_expected(case["name"], j, k)[1], f"{case['name']} tracker {j} call {k} f64")
    finally:
        c.close()


# ---- identity pairs ---------------------------------------------------------------------------------------------------------------------

def test_identity_pairs_with_and_without_the_pair_kernels():
    """pairs (first + i, i) are the batch call; cs_pairs_force=1 sends them through k_bpp_*: same bytes, and the timers tell the route"""
    w, h, n, first = 145, 113, 5, 2
    a = np.stack([cs_cases.hist_frame("blocks", w, h, 50 + s) for s in range(n)])
    b = np.stack([cs_cases.hist_frame("blocks", w, h, 53 + s) for s in range(n)])
    rects = [(w // 4 + s, h // 4, w // 2, h // 2) for s in range(n)]
    pairs = [(first + i, i) for i in range(n)]
    want = [bp_cases.expected(bp_cases.model_of(a[s], rects[s]), b[s]) for s in range(n)]
    outs = {}
    for opt in (None, "cs_pairs_force=1"):
        c = Context(options=opt)
        try:
            c.set_geometry(w, h, n)
            c.camshift_reserve(n + first)
            c.upload(a)
            c.camshift_init(rects, first=first)
            c.upload(b)
            c.profile(True)
            c.kernel_times(reset=True)
            for kind in KINDS:
                outs[(opt, kind)] = c.camshift_backproject_pairs(pairs, kind=kind)
                same(outs[(opt, kind)], np.stack([sel(x, kind) for x in want]), f"identity pairs, {opt}, {kind}")
                same(outs[(opt, kind)], c.camshift_backproject(n, first=first, kind=kind), f"identity pairs against the batch call, {opt}, {kind}")
            t = c.kernel_times()
            assert ("bpp_project" in t) == (opt is not None), (opt, sorted(t))
        finally:
            c.close()
    for kind in KINDS:
        same(outs[(None, kind)], outs[("cs_pairs_force=1", kind)], f"forced against forwarded, {kind}")


# ---- device output ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(145, 113), (65, 63)], ids=["145x113", "odd-65x63"])
@pytest.mark.parametrize("kind", KINDS)
def test_device_form_writes_the_frames_and_nothing_else(w, h, kind):
    """the _device form into a sentinel-filled buffer with a stride larger than a frame, at an offset that is a multiple of the element
    size only: the outputs equal the host form's; every gap and the bytes in front of the first and behind the last output keep the sentinel"""
    elem = 8 if kind == "f64" else 4
    fb, lead = w * h * elem, 3 * elem
    stride, tail = fb + 5 * elem, 4096
    nb = 3
    frames = np.stack([cs_cases.hist_frame("blocks", w, h, 40 + s) for s in range(nb)])
    pairs = [(6, 2), (1, 0), (4, 2), (0, 2), (3, 0), (7, 2), (5, 2), (2, 2)]  # frame 2 six times (two groups of either kind), frame 1 unused
    n = len(pairs)
    rects = [(w // 4 + i, h // 4, w // 2, h // 2) for i in range(n)]
    c = Context()
    buf = DeviceArray(np.full(lead + n * stride + tail, 0xA5, dtype=np.uint8))
    try:
        c.set_geometry(w, h, nb)
        c.camshift_reserve(9)
        c.upload(frames)
        c.camshift_init_pairs(pairs, rects)
        want = c.camshift_backproject_pairs(pairs, kind=kind)
        same(want, np.stack([sel(bp_cases.expected(bp_cases.model_of(frames[f], rects[i]), frames[f]), kind) for i, (_s, f) in enumerate(pairs)]), "host form")
        c.camshift_backproject_pairs_device(buf.ptr + lead, pairs, kind=kind, stride=stride)
        c.synchronize()
        got = d2h(buf.ptr, buf.nbytes)
        assert (got[:lead] == 0xA5).all()
        for i in range(n):
            o = lead + i * stride
            same(got[o:o + fb], want[i].view(np.uint8).reshape(-1), f"device output {i}")
            assert (got[o + fb:o + stride] == 0xA5).all(), f"gap behind output {i}"
        assert (got[lead + n * stride:] == 0xA5).all()
        c.camshift_backproject_pairs_device(buf.ptr, pairs, kind=kind)  # packed (stride 0)
        c.synchronize()
        same(d2h(buf.ptr, n * fb), want.view(np.uint8).reshape(-1), "device form, packed")
    finally:
        c.close()
        buf.free()


# ---- neighbouring calls -----------------------------------------------------------------------------------------------------------------

def _neighbour_run(interleave):
    """feed 0's three trackers as pairs on frame 0 and feed 1's first tracker as a batch stream on frame 1; enqueue-only pair and batch track
    steps, two pair steps and a batch step outstanding at a time.  With `interleave`, back-projection pair calls (both forms and kinds) sit
    between the two enqueue-only pair steps: behind the first, and behind the batch step that follows it.  Returns (track objects, stats, debug histograms, checked outputs)."""
    f0, f1 = pc.feed_scene(0), pc.feed_scene(1)
    pairs = [(5, 0), (0, 0), (3, 0)]
    bp_pairs = [(3, 0), (8, 1), (5, 0), (0, 0)]
    dev = [DeviceArray(np.stack([f0.frames[k], f1.frames[k]])) for k in range(pc.FEED_CALLS + 1)]
    scratch = DeviceArray(np.zeros(len(bp_pairs) * 320 * 240 * 8, dtype=np.uint8))
    c = Context()
    try:
        c.set_geometry(320, 240, 2)
        c.camshift_reserve(12)
        c.bind_device(dev[0].ptr, 2)
        c.camshift_init_pairs(pairs, f0.rects)
        c.camshift_init([f0.rects[0], f1.rects[0]], first=7)  # stream 8 = feed 1's tracker 0 on frame 1
        c.camshift_stats(12, reset=True)
        objs, checked = [], 0
        models = {3: bp_cases.model_of(f0.frames[0], f0.rects[2]), 5: bp_cases.model_of(f0.frames[0], f0.rects[0]),
                  0: bp_cases.model_of(f0.frames[0], f0.rects[1]), 8: bp_cases.model_of(f1.frames[0], f1.rects[0])}
        for k in (1, 3):
            c.bind_device(dev[k].ptr, 2)
            c.camshift_track_pairs(pairs, fetch=False)
            if interleave:
                c.camshift_backproject_pairs_device(scratch.ptr, bp_pairs, kind="f64")
                got = c.camshift_backproject_pairs(bp_pairs, kind="rgba8")  # waits: frames dev[k] are still bound
                for i, (s, f) in enumerate(bp_pairs):
                    same(got[i], bp_cases.expected(models[s], (f0, f1)[f].frames[k])[0], f"behind a pair step, call {k}, pair {i}")
                    checked += 1
                pdf = d2h(scratch.ptr, scratch.nbytes).view(np.float64).reshape(len(bp_pairs), 240, 320)
                for i, (s, f) in enumerate(bp_pairs):
                    same(pdf[i], bp_cases.expected(models[s], (f0, f1)[f].frames[k])[1], f"device form behind a pair step, call {k}, pair {i}")
            c.bind_device(dev[k + 1].ptr, 2)
            c.camshift_track(2, first=7, fetch=False)
            if interleave:  # behind a batch step and in front of a pair step, a pair step and a batch step outstanding
                c.camshift_backproject_pairs_device(scratch.ptr, bp_pairs, kind="rgba8")
            c.camshift_track_pairs(pairs, fetch=False)
            objs.append(c.camshift_track_collect(3).copy())
            objs.append(c.camshift_track_collect(2).copy())
            objs.append(c.camshift_track_collect(3).copy())
            if interleave:
                c.synchronize()
                rg = d2h(scratch.ptr, len(bp_pairs) * 320 * 240 * 4).reshape(len(bp_pairs), 240, 320, 4)
                for i, (s, f) in enumerate(bp_pairs):
                    same(rg[i], bp_cases.expected(models[s], (f0, f1)[f].frames[k + 1])[0], f"between a batch and a pair step, call {k + 1}, pair {i}")
                    checked += 1
        stats = c.camshift_stats(12, reset=False)
        hists = [c.camshift_debug_hist(s) for s in (5, 0, 3)]
        return objs, stats, hists, checked
    finally:
        c.synchronize()
        c.close()
        scratch.free()
        for d in dev:
            d.free()


def test_the_call_leaves_neighbouring_track_steps_alone():
    plain, mixed = _neighbour_run(False), _neighbour_run(True)
    assert mixed[3] == 16 and len(plain[0]) == len(mixed[0]) == 6
    for k, (a, b) in enumerate(zip(plain[0], mixed[0])):
        assert a.tobytes() == b.tobytes(), f"track objects of collect {k} differ"
        assert (a["width"] > 0).all()
    assert np.array_equal(plain[1][0], mixed[1][0]) and np.array_equal(plain[1][1], mixed[1][1]), "camshift_stats differ"
    last = pc.feed_scene(0).frames[4]
    for (ma, ca), (mb, cb) in zip(plain[2], mixed[2]):
        assert np.array_equal(ma, mb) and np.array_equal(ca, cb), "debug histograms differ"
        assert np.array_equal(cb, cs_cases.frame_histogram(last)), "debug histogram is not the last pair TRACK call's"


# ---- errors -----------------------------------------------------------------------------------------------------------------------------

def test_bad_calls_are_status_codes_and_write_nothing():
    w, h, nb = 64, 48, 2
    frames = np.stack([cs_cases.hist_frame("noise", w, h, 70 + s) for s in range(nb)])
    good = [(4, 1), (1, 0), (2, 1)]
    rects = [(10, 10, 30, 20), (5, 8, 20, 30), (20, 4, 40, 40)]
    n = len(good)
    c = Context()
    buf = DeviceArray(np.full(8 * w * h * 8 + 64, 0xA5, dtype=np.uint8))
    host = np.full(8 * w * h * 8, 0x5A, dtype=np.uint8)
    L, H = c._lib, c._h

    def arr(p):
        return np.array(p, dtype=np.int32).reshape(-1, 2)

    def st(fn, p, n_, kind, out, stride):
        a = arr(p) if p is not None else None  # alive until the call returns
        return getattr(L, fn)(H, a.ctypes.data if a is not None else None, n_, kind, out, stride)

    def untouched():
        c.synchronize()
        assert (host == 0x5A).all(), "a refused call wrote to the host output"
        assert (d2h(buf.ptr, buf.nbytes) == 0xA5).all(), "a refused call wrote to the device output"

    try:
        c.set_geometry(w, h, nb)
        c.camshift_reserve(6)
        for fn, out in (("ht_camshift_backproject_pairs", host.ctypes.data), ("ht_camshift_backproject_pairs_device", buf.ptr)):
            assert st(fn, good, n, 0, out, 0) == STATE  # nothing bound
        c.upload(frames)
        c.camshift_init_pairs(good, rects)
        bad = [("unreserved stream", [(4, 1), (6, 0), (2, 1)]), ("negative stream", [(-1, 0), (1, 0), (2, 1)]), ("unbound frame", [(4, 1), (1, 2), (2, 1)]),
               ("negative frame", [(4, 1), (1, -1), (2, 1)]), ("a stream named twice", [(4, 1), (1, 0), (4, 0)]),
               ("more pairs than streams", [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0), (0, 1)])]
        want = [bp_cases.expected(bp_cases.model_of(frames[f], rects[i]), frames[f]) for i, (_s, f) in enumerate(good)]
        for fn, out in (("ht_camshift_backproject_pairs", host.ctypes.data), ("ht_camshift_backproject_pairs_device", buf.ptr)):
            for what, p in bad:
                assert st(fn, p, len(p), 0, out, 0) == INVALID, (fn, what)
                assert st(fn, p, len(p), 1, out, 0) == INVALID, (fn, what)
            assert st(fn, good, 0, 0, out, 0) == INVALID                       # n = 0
            assert st(fn, good, -2, 0, out, 0) == INVALID
            assert st(fn, None, n, 0, out, 0) == INVALID                       # NULL pairs
            assert st(fn, good, n, 0, None, 0) == INVALID                      # NULL output
            assert getattr(L, fn)(None, arr(good).ctypes.data, n, 0, out, 0) == INVALID
            assert st(fn, good, n, 2, out, 0) == INVALID                       # unknown kind
            assert st(fn, good, n, -1, out, 0) == INVALID
            assert st(fn, good, n, 0, out, w * h * 4 - 4) == INVALID           # stride smaller than a frame
            assert st(fn, good, n, 1, out, w * h * 8 - 8) == INVALID
            untouched()
        fn = "ht_camshift_backproject_pairs_device"
        assert st(fn, good, n, 0, buf.ptr + 2, 0) == INVALID                   # misaligned device pointer
        assert st(fn, good, n, 1, buf.ptr + 4, 0) == INVALID
        assert st(fn, good, n, 0, buf.ptr, w * h * 4 + 2) == INVALID           # stride not a multiple of the element size
        assert st(fn, good, n, 1, buf.ptr, w * h * 8 + 4) == INVALID
        untouched()
        with pytest.raises(HtError) as e:
            c.camshift_backproject_pairs(good, kind=2)
        assert e.value.status == INVALID and "kind" in str(e.value)
        with pytest.raises(HtError) as e:
            c.camshift_backproject_pairs([(4, 1), (4, 0)])
        assert e.value.status == INVALID and "twice" in str(e.value)
        # the host form takes any stride >= a frame (applied by the copy)
        padded = np.full((n, w * h * 4 + 6), 0x5A, dtype=np.uint8)
        assert st("ht_camshift_backproject_pairs", good, n, 0, padded.ctypes.data, padded.shape[1]) == 0
        for i in range(n):
            same(padded[i, :w * h * 4], want[i][0].reshape(-1), "host form with a padded stride")
            assert (padded[i, w * h * 4:] == 0x5A).all()
        # a valid call afterwards is exact, and the trackers still track
        for kind in KINDS:
            same(c.camshift_backproject_pairs(good, kind=kind), np.stack([sel(x, kind) for x in want]), f"after the refused calls, {kind}")
        assert (c.camshift_track_pairs(good)["width"] >= 0).all()
    finally:
        c.close()
        buf.free()


# ---- 1080p ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_two_trackers_on_one_1080p_frame(kind):
    s = pc.large_1080p()
    pairs = [(1, 0), (0, 0)]
    c = Context()
    try:
        c.set_geometry(s.w, s.h, 1)
        c.camshift_reserve(2)
        c.upload(s.frames[0][None])
        c.camshift_init_pairs(pairs, s.rects)
        c.upload(s.frames[1][None])
        got = c.camshift_backproject_pairs(pairs, kind=kind)
        for j in range(2):
            want = sel(bp_cases.expected(bp_cases.model_of(s.frames[0], s.rects[j]), s.frames[1]), kind)
            assert len(np.unique(want)) >= 2
            same(got[j], want, f"1080p tracker {j} {kind}")
    finally:
        c.close()


# ---- the Node host ----------------------------------------------------------------------------------------------------------------------

def test_multitracker_back_projections_from_node(tmp_path):
    """tests/js/bp_pairs_gpu.js: camshift.MultiTracker on the real addon, getBackProjectionImgs() after every track() of both golden
    sequences against the reference's recorded CRCs, getPdf(i) at the recorded points, one device call per getBackProjectionImgs()"""
    node = shutil.which("node")
    if node is None or not os.path.exists(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr_hip.node")):
        pytest.skip("node or the addon is missing")
    golden = load_golden("multitrack_bp.json")
    job = {"cases": []}
    for case in golden["cases"]:
        s = golden_sequences()[case["name"]]
        files = []
        for k, f in enumerate(s.frames):
            p = tmp_path / f"{case['name']}_{k}.raw"
            f.tofile(p)
            files.append(str(p))
        job["cases"].append({"name": case["name"], "w": s.w, "h": s.h, "rects": case["rects"], "frames": files, "trackers": case["trackers"]})
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "bp_pairs_gpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    ncalls = sum(len(c["trackers"][0]) for c in golden["cases"])
    ntr = sum(len(c["trackers"]) * len(c["trackers"][0]) for c in golden["cases"])
    assert out["crc_checks"] == ntr and out["pdf_checks"] == ntr
    assert out["imgs_calls"] == ncalls and out["device_calls"] == ncalls + ntr, out  # one per getBackProjectionImgs(), one per getPdf(i)

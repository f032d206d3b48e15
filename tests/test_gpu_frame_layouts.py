"""Frames where a host leaves them: ht_bind_frames_device and ht_camshift_track_sequence at every layout of tests/frame_layouts.py (bases that
are 4- but not 16-byte aligned, strides beyond W * H * 4), and the host entry points at frame strides beyond a frame.  Every frame-reading
kernel computes frames + index * frame_stride; this module is where that product is anything but index * W * H * 4 and where a 16-byte load
starts off a 16-byte boundary.  DESIGN.md ("Frame-reading kernels") lists which test reaches which kernel.

Every comparison is against the CPU oracle on the TRUE frames: exact for detect, planes, white balance, histograms and back-projection,
the project's +-1 px / +-0.5 deg of tests/test_gpu_camshift.py for track objects — whose bytes must also be those of the same context on the
packed, 16-byte-aligned control layout.  The gaps between the frames hold seeded noise; tests/test_frame_layouts_cpu.py proves from the oracle
alone that a reader which ignores the stride, or rounds a base down to 16 bytes, changes every one of these results."""
import ctypes as C
import functools

import numpy as np
import pytest

import bp_cases
import cs_cases as cc
import frame_layouts as fl
import ingest_cases as ic
from headtrackr_amd import native
from headtrackr_amd.api import HT_INPUT_GRAY_IN_R, Context, HtError
from headtrackr_amd.native import HIT_DTYPE, HT_DETECT_WHITEBALANCE
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_backproject import same
from test_gpu_camshift import SCHEDULES, check

pytestmark = pytest.mark.gpu

HT_ERR_INVALID = -1
N = fl.NFRAMES
NAMES = list(fl.LAYOUTS)
DETECT_FLAGS = [0, HT_INPUT_GRAY_IN_R, HT_DETECT_WHITEBALANCE, HT_INPUT_GRAY_IN_R | HT_DETECT_WHITEBALANCE]


class Placed:
    """a batch laid out on the device: the host image, its device copy and the pointer / stride a host would bind"""

    def __init__(self, frames, name, w, h, salt=0):
        self.frames, self.w, self.h = frames, w, h
        self.lead, self.stride = fl.layout(name, w, h)
        self.image = fl.lay_out(frames, self.lead, self.stride, fl.layout_seed(name, w, h, salt))
        self.dev = DeviceArray(self.image)
        self.ptr = self.dev.ptr + self.lead

    def bind(self, c, n=N):
        c.bind_device(self.ptr, n, self.stride)

    def assert_untouched(self, c, what):
        """frames are read-only: the whole image, gaps included, is what was uploaded"""
        got = c.device_download(self.dev.ptr, len(self.image))
        assert np.array_equal(got, self.image), (what, np.flatnonzero(got != self.image)[:8])

    def free(self):
        self.dev.free()


# ---- the oracle, once per input --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_detect(w, h, gray_in_r):
    from headtrackr_amd.cascade import load_cascade

    blob = load_cascade().blob
    return [ho.detect_raw(f, blob, gray_in_r=gray_in_r) for f in fl.detect_frames(w, h)]


@functools.lru_cache(maxsize=None)
def oracle_planes(w, h, gray_in_r):
    return [fl.gray_plane(f, gray_in_r) for f in fl.detect_frames(w, h)]


@functools.lru_cache(maxsize=None)
def oracle_wb(w, h):
    return np.array([ho.whitebalance(f) for f in fl.detect_frames(w, h)])


def assert_detect(c, w, h, flags, frames_idx, what):
    """the batch collected from `c` == the oracle for detect_frames(w, h)[frames_idx]: raw hits field for field with the bits of `sum`,
    counts[] per frame (the check of tests/test_gpu_sizes.py), the level-0 plane of every frame, and the fused white balance"""
    hits, counts = c.detect_collect()
    gray_in_r = bool(flags & HT_INPUT_GRAY_IN_R)
    want = [oracle_detect(w, h, gray_in_r)[f] for f in frames_idx]
    assert len(counts) == len(frames_idx) and [int(v) for v in counts] == [len(x) for x in want], (what, counts)
    k = 0
    for i, ref in enumerate(want):
        g = hits[k : k + len(ref)]
        assert np.all(g["frame"] == i), (what, i)
        for name in ("scale", "q", "x", "y"):
            assert np.array_equal(g[name].astype(np.int64), ref[name].astype(np.int64)), (what, i, name)
        assert np.array_equal(g["sum"].view(np.uint64), ref["sum"].view(np.uint64)), (what, i)
        k += len(ref)
    assert k == len(hits), what
    for i, f in enumerate(frames_idx):
        same(c.pyramid_readback(i, 0), oracle_planes(w, h, gray_in_r)[f], f"{what}: level-0 plane of frame {i}")
    if flags & HT_DETECT_WHITEBALANCE:
        assert np.array_equal(c.detect_whitebalance(), oracle_wb(w, h)[list(frames_idx)]), what
    return len(hits)


# ---- detect ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", fl.DETECT_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", NAMES)
def test_detect_on_bound_layout(name, w, h):
    """k_gray_linear (96x80, all four instantiations) / k_gray_rows (97x81) and k_channel_sums read the frames where the binding says"""
    p = Placed(fl.detect_frames(w, h), name, w, h)
    c = Context()
    try:
        c.set_geometry(w, h, N)
        p.bind(c)
        total = 0
        for flags in DETECT_FLAGS:
            c.detect_enqueue(flags)
            total += assert_detect(c, w, h, flags, range(N), (name, w, h, flags))
            assert np.array_equal(c.whitebalance(), oracle_wb(w, h)), (name, w, h, flags)  # k_channel_sums
        assert total > 0
        p.assert_untouched(c, (name, w, h))
    finally:
        c.close()
        p.free()


@pytest.mark.parametrize("name", NAMES)
def test_detect_graph_key_holds_the_stride(name):
    """one buffer, ONE pointer, two frames, two strides: S sees frames 1 and 2, 2 S sees frames 1 and 3.  The two bindings differ in
    nothing but the stride, so a replayed graph that was captured for the other one shows the other pair's hits, planes and white balance.
    Three enqueues per key: plain, captured + replayed, replayed — graph_launches grows by 2 per key."""
    w, h = fl.DETECT_SIZES[0]
    p = Placed(fl.detect_frames(w, h), name, w, h)
    flags = HT_DETECT_WHITEBALANCE
    c = Context()  # its own stream, no profiling: what the graph path asks for
    try:
        c.set_geometry(w, h, 2)
        ptr = p.ptr + p.stride
        seen = {1: [1, 2], 2: [1, 3]}
        assert oracle_detect(w, h, False)[2].tobytes() != oracle_detect(w, h, False)[3].tobytes()
        grown = {1: 0, 2: 0}
        for rnd in range(3):
            for mult in (1, 2):
                c.bind_device(ptr, 2, mult * p.stride)
                before = c.graph_launches
                c.detect_enqueue(flags)
                grown[mult] += c.graph_launches - before
                assert_detect(c, w, h, flags, seen[mult], (name, "stride x", mult, "round", rnd))
        assert grown[1] >= 2 and grown[2] >= 2, grown
        p.assert_untouched(c, name)
    finally:
        c.close()
        p.free()


# ---- camshift --------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=list(SCHEDULES))
def cs_ctx(request):
    """(schedule, context, {size: control run}) — the four schedules of tests/test_gpu_camshift.py, full-frame histograms kept"""
    c = Context(options=SCHEDULES[request.param] + ",cs_keep_hist=1")
    yield request.param, c, {}
    c.close()


@functools.lru_cache(maxsize=None)
def cs_expected(w, h):
    """[stream][call] -> (search window, track object) from the oracle"""
    return [[(sw, to) for (_b, sw, to) in s.oracle_calls()] for s in fl.cs_streams(w, h)]


@functools.lru_cache(maxsize=None)
def cs_frame_hist(w, h, k, s):
    return cc.frame_histogram(fl.cs_streams(w, h)[s].frames[k])


@functools.lru_cache(maxsize=None)
def cs_model(w, h, s, rect):
    return cc.model_histogram(fl.cs_streams(w, h)[s].frames[0], rect)


def run_camshift(c, sched, name, w, h):
    """init (both initTracker kernels) and three track calls from bindings of layout `name`, then the same three calls through
    ht_camshift_track_sequence; returns the raw bytes of the track objects of both routes"""
    seqs = fl.cs_streams(w, h)
    placed = [Placed(fl.cs_batch(w, h, k), name, w, h, salt=k) for k in range(fl.CS_STEPS + 1)]
    try:
        c.set_geometry(w, h, N)
        c.camshift_reserve(N)
        placed[0].bind(c)
        for kind in ("short", "tall"):  # k_cs_init, k_cs_init_rows
            rects = fl.cs_init_rects(w, h, kind)
            c.camshift_init(rects)
            for s, rect in enumerate(rects):
                model = c.camshift_debug_hist(s, current=False)[0].astype(np.int64)
                assert np.array_equal(model, cs_model(w, h, s, tuple(rect))), (name, sched, kind, s, rect)
        stats, raw = [], {}
        c.camshift_init([s.rect for s in seqs])
        single = b""
        for k in range(1, fl.CS_STEPS + 1):
            placed[k].bind(c)
            got = c.camshift_track(N, calc_angles=True)
            for s in range(N):
                sw, to = cs_expected(w, h)[s][k - 1]
                check(got[s], sw, to, stats, where=("layouts", name, sched, f"{w}x{h}", s, k), tally=("layouts",))
                cur = c.camshift_debug_hist(s, current=True)[1].astype(np.int64)
                assert np.array_equal(cur, cs_frame_hist(w, h, k, s)), (name, sched, w, h, s, k, np.flatnonzero(cur != cs_frame_hist(w, h, k, s))[:8])
            single += got.tobytes()
        raw["track"] = single
        placed[0].bind(c)
        c.camshift_init([s.rect for s in seqs])  # the same initial state again
        got = c.camshift_track_sequence([placed[k].ptr for k in range(1, fl.CS_STEPS + 1)], N, calc_angles=True, frame_stride=placed[0].stride, fetch="all")
        assert got.shape == (fl.CS_STEPS, N)
        for k in range(1, fl.CS_STEPS + 1):
            for s in range(N):
                sw, to = cs_expected(w, h)[s][k - 1]
                check(got[k - 1, s], sw, to, stats, where=("layouts-sequence", name, sched, f"{w}x{h}", s, k), tally=("layouts",))
        raw["sequence"] = got.tobytes()
        assert len(stats) == 2 * fl.CS_STEPS * N
        for k, p in enumerate(placed):
            p.assert_untouched(c, (name, sched, w, h, k))
        return raw
    finally:
        c.synchronize()
        for p in placed:
            p.free()


@pytest.mark.parametrize("w,h", fl.CS_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", NAMES)
def test_camshift_on_bound_layout(cs_ctx, name, w, h):
    """k_cs_init / k_cs_init_rows, k_cs_hist, k_cs_meanshift, k_cs_meanshift_cluster and both forms of the fused kernel (rows2d at 320x240,
    linear at 201x157), single calls and sequences: every call within the project's tolerance of the oracle, and the bytes of every track
    object those of the same context on the packed, aligned control"""
    sched, c, control = cs_ctx
    if (w, h) not in control:
        control[w, h] = run_camshift(c, sched, fl.CONTROL, w, h)
    got = control[w, h] if name == fl.CONTROL else run_camshift(c, sched, name, w, h)
    assert got["track"] == control[w, h]["track"], (name, sched, w, h)
    assert got["sequence"] == control[w, h]["sequence"], (name, sched, w, h)


# ---- pairs and back-projection -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", fl.CS_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", NAMES)
def test_pairs_and_backprojection_on_bound_layout(name, w, h):
    """k_csp_init / k_csp_hist / k_csp_meanshift with frames out of order and repeated, k_bp_project and k_bpp_project in both kinds"""
    seqs = fl.cs_streams(w, h)
    placed = [Placed(fl.cs_batch(w, h, k), name, w, h, salt=k) for k in range(fl.CS_STEPS + 1)]
    c = Context()
    try:
        c.set_geometry(w, h, N)
        c.camshift_reserve(N)
        placed[0].bind(c)
        c.camshift_init_pairs(fl.PAIRS, [seqs[f].rect for _s, f in fl.PAIRS])  # tracker `stream` follows the blob of frame slot f
        stats = []
        for k in range(1, fl.CS_STEPS + 1):
            placed[k].bind(c)
            got = c.camshift_track_pairs(fl.PAIRS, calc_angles=True)
            for i, (_s, f) in enumerate(fl.PAIRS):
                sw, to = cs_expected(w, h)[f][k - 1]
                check(got[i], sw, to, stats, where=("layouts-pairs", name, f"{w}x{h}", i, k), tally=("layouts",))
        assert len(stats) == fl.CS_STEPS * len(fl.PAIRS)
        # back-projection of call 2's frames: batch form through every stream's own model, pair form through the models the pairs left
        placed[0].bind(c)
        c.camshift_init([s.rect for s in seqs])
        placed[2].bind(c)
        batch = fl.cs_batch(w, h, 2)
        models = [cs_model(w, h, s, seqs[s].rect) for s in range(N)]
        want = [bp_cases.expected(models[s], batch[s]) for s in range(N)]
        want_pairs = [bp_cases.expected(models[s], batch[f]) for s, f in fl.PAIRS]
        for kind, sel in (("rgba8", 0), ("f64", 1)):
            same(c.camshift_backproject(N, kind=kind), np.stack([x[sel] for x in want]), f"{name} {w}x{h} backproject {kind}")
            same(c.camshift_backproject_pairs(fl.PAIRS, kind=kind), np.stack([x[sel] for x in want_pairs]), f"{name} {w}x{h} backproject_pairs {kind}")
        for k, p in enumerate(placed):
            p.assert_untouched(c, (name, w, h, k))
    finally:
        c.close()
        for p in placed:
            p.free()


# ---- host frames, frame_stride bytes apart -----------------------------------------------------------------------------------------------------

def host_strides(name, w, h):
    """fb + 4 and fb + 13 (a host stride need not be a multiple of 4), and the layout's own"""
    fb = fl.fb_of(w, h)
    return sorted({fb + 4, fb + 13, fl.layout(name, w, h)[1]})


def host_image(name, w, h, stride, frames=None):
    lead = fl.layout(name, w, h)[0]
    img = fl.lay_out(fl.detect_frames(w, h) if frames is None else frames, lead, stride, fl.layout_seed(name, w, h, stride))
    return img, lead


@pytest.mark.parametrize("w,h", fl.DETECT_SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", NAMES)
def test_host_uploads_at_a_frame_stride(name, w, h):
    """ht_upload_frames, ht_upload_frames_async + ht_swap_frames (from ht_host_alloc memory) and ht_detect_batch"""
    L = native.lib()
    c = Context()
    try:
        c.set_geometry(w, h, N)
        for stride in host_strides(name, w, h):
            img, lead = host_image(name, w, h, stride)
            keep = img.copy()
            c.upload_ptr(img.ctypes.data + lead, N, stride)
            c.detect_enqueue(HT_DETECT_WHITEBALANCE)
            assert_detect(c, w, h, HT_DETECT_WHITEBALANCE, range(N), (name, "upload_ptr", stride))
            assert np.array_equal(c.whitebalance(), oracle_wb(w, h))
            # ht_detect_batch
            hits = np.zeros(1 << 12, dtype=HIT_DTYPE)
            counts, total = np.zeros(N, dtype=np.uint32), C.c_uint32(0)
            st = L.ht_detect_batch(c._h, img.ctypes.data + lead, N, w, h, stride, HT_INPUT_GRAY_IN_R, hits.ctypes.data, len(hits), counts.ctypes.data, C.byref(total))
            assert st == 0, L.ht_last_error(c._h)
            want = oracle_detect(w, h, True)
            assert [int(v) for v in counts] == [len(x) for x in want] and total.value == sum(len(x) for x in want)
            k = 0
            for i, ref in enumerate(want):
                g = hits[k : k + len(ref)]
                assert np.all(g["frame"] == i) and np.array_equal(g["sum"].view(np.uint64), ref["sum"].view(np.uint64)), (name, stride, i)
                for f in ("scale", "q", "x", "y"):
                    assert np.array_equal(g[f].astype(np.int64), ref[f].astype(np.int64)), (name, stride, i, f)
                k += len(ref)
            for i in range(N):
                same(c.pyramid_readback(i, 0), oracle_planes(w, h, True)[i], f"{name} detect_batch stride {stride} frame {i}")
            # the pinned route
            pinned = C.c_void_p()
            assert L.ht_host_alloc(len(img), C.byref(pinned)) == 0
            try:
                C.memmove(pinned.value, img.ctypes.data, len(img))
                c.upload_async_ptr(pinned.value + lead, N, stride)
                c.swap_frames()
                c.detect_enqueue(0)
                assert_detect(c, w, h, 0, range(N), (name, "upload_async_ptr", stride))
                c.synchronize()
                back = np.ctypeslib.as_array(C.cast(pinned, C.POINTER(C.c_uint8)), shape=(len(img),))
                assert np.array_equal(back, keep)
            finally:
                L.ht_host_free(pinned)
            assert np.array_equal(img, keep), (name, stride)
    finally:
        c.close()


@pytest.mark.parametrize("name", NAMES)
def test_host_draw_and_grayscale_at_a_frame_stride(name):
    """ht_draw_frames with source frames further apart than a frame, against the ingest oracle; ht_grayscale_batch (k_gray_inplace) in
    place at a stride: the frames are ccv.grayscale's, alpha and every gap byte stay"""
    L = native.lib()
    (sw, sh), (dw, dh) = (64, 48), (40, 30)
    src = ic.frames_of("noise", sw, sh, N, seed=21)
    want = np.stack([ic.expected(src[f], None, dw, dh) for f in range(N)])
    rect = (3, 5, sw - 7, sh - 9)
    want_rect = np.stack([ic.expected(src[f], rect, dw, dh) for f in range(N)])
    c = Context()
    try:
        c.set_geometry(dw, dh, N)
        for stride in host_strides(name, sw, sh):
            img, lead = host_image(name, sw, sh, stride, frames=src)
            keep = img.copy()
            for r, wnt in ((None, want), (rect, want_rect)):
                rr = Context._cs_rect(r)
                st = L.ht_draw_frames(c._h, img.ctypes.data + lead, N, sw, sh, stride, rr.ctypes.data if rr is not None else None)
                assert st == 0, L.ht_last_error(c._h)
                assert L.ht_frames_bound(c._h) == N
                c.nframes = N
                c.detect_enqueue(HT_INPUT_GRAY_IN_R)
                c.detect_collect()
                for f in range(N):
                    same(c.pyramid_readback(f, 0), wnt[f][..., 0], f"{name} draw stride {stride} rect {r}: R of frame {f}")
                c.detect_enqueue(0)
                c.detect_collect()
                for f in range(N):
                    same(c.pyramid_readback(f, 0), ho.grayscale_rgba(wnt[f])[..., 0], f"{name} draw stride {stride} rect {r}: gray of frame {f}")
                assert np.array_equal(c.whitebalance(), np.array([ho.whitebalance(x) for x in wnt]))
            assert np.array_equal(img, keep)
        for w, h in fl.DETECT_SIZES:
            frames = fl.detect_frames(w, h).copy()
            frames[..., 3] = ic.noise(w, h * N, 77 + w).reshape(N, h, w, 4)[..., 3]  # an alpha worth keeping
            wantg = np.stack([ho.grayscale_rgba(f) for f in frames])
            assert np.array_equal(wantg[..., 3], frames[..., 3])
            for stride in host_strides(name, w, h):
                img, lead = host_image(name, w, h, stride, frames=frames)
                expect = img.copy()
                for f in range(N):
                    expect[lead + f * stride : lead + f * stride + fl.fb_of(w, h)] = wantg[f].reshape(-1)
                st = L.ht_grayscale_batch(c._h, img.ctypes.data + lead, N, w, h, stride)
                assert st == 0, L.ht_last_error(c._h)
                got = fl.read_at(img, fl.true_offsets(lead, stride, N), w, h)
                same(got, wantg, f"{name} grayscale_batch {w}x{h} stride {stride}")
                assert np.array_equal(got[..., 3], frames[..., 3])
                assert np.array_equal(img, expect), (name, w, h, stride, "a gap byte changed")
    finally:
        c.close()


# ---- argument edges ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_bad_strides_and_pointers_are_refused_and_leave_the_binding(name):
    """stride fb - 4, stride fb + 2 and pointer + 2: HT_ERR_INVALID from ht_bind_frames_device and ht_camshift_track_sequence; the
    binding made before them is still the one the next detect reads"""
    w, h = fl.DETECT_SIZES[0]
    fb = fl.fb_of(w, h)
    p = Placed(fl.detect_frames(w, h), name, w, h)
    other = DeviceArray(np.zeros(N * fb + 64, dtype=np.uint8))
    c = Context()
    try:
        c.set_geometry(w, h, N)
        c.camshift_reserve(N)
        p.bind(c)
        for ptr, stride in ((other.ptr, fb - 4), (other.ptr, fb + 2), (other.ptr + 2, fb), (other.ptr + 2, fb + 4)):
            with pytest.raises(HtError) as e:
                c.bind_device(ptr, N, stride)
            assert e.value.status == HT_ERR_INVALID, (ptr - other.ptr, stride - fb)
            with pytest.raises(HtError) as e:
                c.camshift_track_sequence([ptr], N, frame_stride=stride)
            assert e.value.status == HT_ERR_INVALID, (ptr - other.ptr, stride - fb)
            assert c._lib.ht_frames_bound(c._h) == N
        with pytest.raises(HtError) as e:  # every pointer of the list is checked, not the first alone
            c.camshift_track_sequence([other.ptr, other.ptr + 2], N, frame_stride=fb + 4)
        assert e.value.status == HT_ERR_INVALID
        c.detect_enqueue(HT_DETECT_WHITEBALANCE)
        assert_detect(c, w, h, HT_DETECT_WHITEBALANCE, range(N), (name, "after the refused calls"))
        assert np.array_equal(c.whitebalance(), oracle_wb(w, h))
        p.assert_untouched(c, name)
    finally:
        c.close()
        p.free()
        other.free()


def test_every_refusal_of_the_frame_and_detect_step_calls_is_the_recorded_one():
    """tests/frame_refusal_cases.py's script — every refusal of the frame calls (upload, async upload, swap, bind, the allocation calls,
    ht_device_free under another context's binding) and of the detect-step calls (enqueue, the three collect forms, the batch call, both
    whitebalance calls), the adjacent double faults that pin each call's check order, ht_set_geometry not yet called — replayed on the
    built library: status, ht_last_error text and ht_frames_bound() afterwards equal tests/golden/frame_call_refusals.json, which was
    recorded before the calls moved out of csrc/ht_context.hip."""
    import json
    import os

    import frame_refusal_cases as frc
    from conftest import GOLDEN

    golden = json.load(open(os.path.join(GOLDEN, "frame_call_refusals.json")))
    got = frc.replay()
    assert got["canvas"] == golden["canvas"]
    assert list(got["cases"]) == list(golden["cases"]) and len(golden["cases"]) >= 100  # the script's order is part of the record
    for key, want in golden["cases"].items():
        assert got["cases"][key] == want, (key, got["cases"][key], want)
    refused = [v for v in golden["cases"].values() if v[0] != 0]
    assert len(refused) >= 95 and all(st in (HT_ERR_INVALID, -6) for st, _, _ in refused)
    assert len({text for _, text, _ in refused}) >= 15  # the messages of all the calls, not one repeated

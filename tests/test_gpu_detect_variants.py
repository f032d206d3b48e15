"""The HIP detect path at intervals other than 5 and with cascades whose window is not 24x24 (ht_create takes interval 1..12 and windows
4x4 .. 64x64; ccv.detect_objects takes both as arguments): pyramid planes, raw hits, stage counters, rects, host and device grouping
against the CPU oracle, and against vectors recorded from the unmodified reference (tests/golden/detect_variants.json).  The tables are
tests/detect_variant_cases.py; tests/test_detect_variants_cpu.py shows without a device that every case plans, finds something and that the
oracle equals the recorded vectors.  Every comparison is equality of bytes: indices, plane bytes, binary64 values."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import detect_variant_cases as dv
import group_cases as gc
from conftest import load_golden
from headtrackr_amd import native, synth
from headtrackr_amd.api import HT_INPUT_RGBA, HT_SCAN_NO_SPLIT, HT_SCAN_SIMPLE, Context
from headtrackr_amd.cascade import load_cascade
from headtrackr_amd.native import HT_SCAN_GENERIC, HT_SCAN_STATS
from oracle import ht_oracle as ho

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("detect_variants.json")
DETECT = load_golden("detect.json")
FLAGS = [0, HT_SCAN_NO_SPLIT, HT_SCAN_SIMPLE, HT_SCAN_GENERIC, HT_SCAN_GENERIC | HT_SCAN_NO_SPLIT]
FLAG_IDS = ["gen+deep", "gen-nosplit", "simple", "generic+deep", "generic-nosplit"]
RECT_FIELDS = ("x", "y", "width", "height", "confidence", "neighbors")

_CTX = {}


@pytest.fixture(scope="module")
def ctx_for():
    """one context per (window or None for the built-in cascade, interval, options), closed when the module is done"""
    def get(window, interval, options=None):
        key = (window, interval, options)
        if key not in _CTX:
            _CTX[key] = Context(cascade=dv.window_cascade(*window) if window else None, interval=interval, options=options, hit_capacity=1 << 16)
        return _CTX[key]

    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def detect(c, frames, flags=HT_INPUT_RGBA, level_dims=None):
    """one batch through a geometry set here (never through Context.detect_raw, which keeps a batch size of its own)"""
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    c.set_geometry(w, h, n, level_dims)
    c.upload(frames)
    c.detect_enqueue(flags)
    return c.detect_collect()


def assert_hits_equal(got, per, what=None):
    """got: the library's batch hits; per: the oracle's per-frame hits in the reference's order"""
    ref = dv.as_batch_hits(per)
    assert len(got) == len(ref), (what, len(got), len(ref))
    for k in ("frame", "scale", "q", "y", "x"):
        assert np.array_equal(got[k].astype(np.int64), ref[k].astype(np.int64)), (what, k)
    assert np.array_equal(got["sum"].view(np.uint64), ref["sum"].view(np.uint64)), (what, "confidence bits")


@functools.lru_cache(maxsize=None)
def oracle_planes(w, h, interval, cw=24, ch=24):
    """ho.pyramid of each frame of the N / S / F triple, computed once"""
    out = []
    for f in dv.triple(w, h):
        levels, arena = ho.pyramid(f, interval, cw, ch)
        arena.setflags(write=False)
        out.append((levels, arena))
    return out


def check_planes(c, w, h, interval, cw=24, ch=24):
    """every present plane of every frame of the triple, and the level count"""
    detect(c, dv.triple(w, h))
    compared = 0
    for f, (levels, arena) in enumerate(oracle_planes(w, h, interval, cw, ch)):
        assert c.num_levels == len(levels)
        for i, (lw, lh, off) in enumerate(levels):
            for s in range(4):
                assert c.plane(i, s).present == (off[s] >= 0), (i, s)
                if off[s] < 0:
                    continue
                got = c.pyramid_readback(f, i, s)
                want = ho.plane(levels, arena, i, s)
                assert got.shape == want.shape and np.array_equal(got, want), f"frame {f} level {i} slot {s}"
                compared += 1
    nxt = interval + 1
    assert compared == 3 * (len(levels) + 3 * (len(levels) - 2 * nxt))


def oracle_rects(per, interval, cw=24, ch=24):
    return [ho.hits_to_rects(h, interval, cw, ch) for h in per]


def check_rects_and_grouping(c, frames, per, interval, blob, cw=24, ch=24):
    """ht_hits_to_rects and ht_group_rects against ho.hits_to_rects / ho.group, then the device route (detect_best_enqueue /
    detect_best_collect / detect_grouped) against ho.detect_objects and facetrackr's selection"""
    hits, counts = detect(c, frames)
    assert_hits_equal(hits, per)
    assert [int(v) for v in counts] == [len(h) for h in per]
    want = oracle_rects(per, interval, cw, ch)
    rects = c.hits_to_rects(hits)
    assert rects.tobytes() == np.concatenate(want).tobytes()
    k = 0
    for f, wr in enumerate(want):
        for mn in (1, 2):
            assert c.group_rects(rects[k:k + len(wr)], mn).tobytes() == ho.group(wr, mn).tobytes(), (f, mn)
        k += len(wr)
    for mn in (1, 2):
        c.detect_enqueue(HT_INPUT_RGBA)
        c.detect_best_enqueue(mn, 0)
        best, total = c.detect_best_collect()
        best = best.copy()
        assert total == len(hits)
        for f in range(len(frames)):
            wg = ho.detect_objects(frames[f], blob, interval, mn, cw=cw, ch=ch, cap=1 << 20)
            assert wg.tobytes() == ho.group(want[f], mn).tobytes()
            got = c.detect_grouped(f)
            assert len(got) == len(wg) and got.tobytes() == wg.tobytes(), (f, mn)
            assert best[f].tobytes() == gc.select_best(wg).tobytes(), (f, mn)


# ---- planes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", dv.SIZES)
@pytest.mark.parametrize("interval", dv.INTERVALS)
def test_pyramid_planes_at_other_intervals(ctx_for, interval, w, h):
    """interval 1: many short generations (next = 2, the offset slots from level 4); interval 12: twelve non-2:1 jobs in generation 1"""
    check_planes(ctx_for(None, interval), w, h, interval)


@pytest.mark.parametrize("opts", dv.TAIL_OPTIONS)
@pytest.mark.parametrize("w,h", dv.TAIL_SIZES)
@pytest.mark.parametrize("interval", dv.TAIL_INTERVALS)
def test_pyramid_planes_at_other_intervals_with_every_generation_kernel(ctx_for, interval, w, h, opts):
    """k_resample, k_resample_bands and the three tail forms forced on the generation structures of intervals 1 and 12"""
    check_planes(ctx_for(None, interval, opts), w, h, interval)


# ---- raw hits, built-in cascade -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("interval", dv.INTERVALS)
def test_builtin_hits_and_stage_counters_at_other_intervals(ctx_for, cascade, interval, mode):
    """every scan schedule: raw hits in the reference's order, stage counters, window count"""
    frames = dv.hit_batch(interval)
    per, sp = dv.builtin_expected(interval)
    c = ctx_for(None, interval)
    hits, counts = detect(c, frames, mode | HT_SCAN_STATS)
    assert_hits_equal(hits, per, mode)
    assert [int(v) for v in counts] == [len(h) for h in per]
    assert np.array_equal(c.stage_counts().astype(np.int64), sp)
    assert c.windows_per_frame * len(frames) == sp[0]
    hits2, _ = detect(c, frames, mode)  # the same without the counters
    assert hits2.tobytes() == hits.tobytes()


@pytest.mark.parametrize("interval", [2, 8])
def test_early_scan_at_other_intervals(ctx_for, interval):
    """the early split is planned from the generation of each scale's last plane: three back-to-back batches"""
    frames = dv.hit_batch(interval)
    c = ctx_for(None, interval, "early_scan=1")
    c.set_geometry(160, 120, len(frames))
    c.upload(frames)
    for _ in range(3):
        c.detect_enqueue(HT_INPUT_RGBA)
        hits, _ = c.detect_collect()
        assert_hits_equal(hits, dv.builtin_expected(interval)[0])


@pytest.mark.parametrize("deep_v", [4, 2])
@pytest.mark.parametrize("interval", [2, 8])
def test_exact_tie_fallback_at_other_intervals(ctx_for, interval, deep_v):
    hits, _ = detect(ctx_for(None, interval, f"force_exact=1,deep_v={deep_v}"), dv.hit_batch(interval))
    assert_hits_equal(hits, dv.builtin_expected(interval)[0])


@pytest.mark.parametrize("interval", [2, 8])
def test_queue_overflow_at_other_intervals(interval):
    c = Context(interval=interval, queue_capacity=8)
    try:
        hits, _ = detect(c, dv.hit_batch(interval))
        assert_hits_equal(hits, dv.builtin_expected(interval)[0])
    finally:
        c.close()


@pytest.mark.parametrize("interval", [2, 8])
def test_graph_replay_on_a_bound_buffer_at_other_intervals(interval):
    """four enqueue / collect rounds on one bound device buffer: the second captures the launch sequence, the later ones replay it"""
    L = native.lib()
    frames = np.ascontiguousarray(dv.hit_batch(interval))
    per = dv.builtin_expected(interval)[0]
    c = Context(interval=interval)
    try:
        p = C.c_void_p()
        assert L.ht_device_alloc(c._h, frames.nbytes, C.byref(p)) == 0
        assert L.ht_device_upload(c._h, p, frames.ctypes.data, frames.nbytes) == 0
        c.set_geometry(160, 120, len(frames))
        c.bind_device(p.value, len(frames))
        for rnd in range(4):
            c.detect_enqueue(HT_INPUT_RGBA)
            hits, _ = c.detect_collect()
            assert_hits_equal(hits, per, rnd)
        assert c.graph_launches == 3  # 1st plain, 2nd captured + launched, 3rd / 4th replayed
    finally:
        c.close()


# ---- rects and grouping, built-in cascade -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interval", dv.INTERVALS)
def test_rects_and_grouping_at_other_intervals(ctx_for, cascade, interval):
    """scale_x is built by repeated multiplication with the context's own 2^(1 / (interval + 1)) (ccv.js:724)"""
    per = dv.builtin_expected(interval)[0]
    assert len({int(s) for h in per for s in h["scale"]}) >= 2
    check_rects_and_grouping(ctx_for(None, interval), dv.hit_batch(interval), per, interval, cascade.blob)


# ---- other windows: every launch lands in k_scan_simple --------------------------------------------------------------------------------

WINDOW_PARAMS = [(cw, ch, iv, w, h) for (w, h) in reversed(dv.WINDOW_SIZES) for (cw, ch, iv) in reversed(dv.WINDOW_CASES)]  # narrowest first


@pytest.mark.parametrize("cw,ch,interval,w,h", WINDOW_PARAMS)
def test_window_planes(ctx_for, cw, ch, interval, w, h):
    """upto, the level count and the sizes follow the window (ccv.js:112-113)"""
    check_planes(ctx_for((cw, ch), interval), w, h, interval, cw, ch)


@pytest.mark.parametrize("cw,ch,interval,w,h", WINDOW_PARAMS)
def test_window_hits_and_stage_counters_under_every_flag(ctx_for, cw, ch, interval, w, h):
    """raw hits and stage counters equal the oracle's; the scan flags change nothing (a scale with qw <= 0 — 64x64 on 97x81 — is skipped,
    a frame may have no hit at all, and neither is an error)"""
    frames = dv.triple(w, h)
    per, sp = dv.window_expected(cw, ch, interval, w, h)
    c = ctx_for((cw, ch), interval)
    first = None
    for mode in FLAGS:
        hits, counts = detect(c, frames, mode | HT_SCAN_STATS)
        assert_hits_equal(hits, per, mode)
        assert [int(v) for v in counts] == [len(x) for x in per]
        assert np.array_equal(c.stage_counts().astype(np.int64), sp), mode
        assert c.windows_per_frame * len(frames) == sp[0]
        plain, _ = detect(c, frames, mode)
        first = hits.tobytes() if first is None else first
        assert hits.tobytes() == first and plain.tobytes() == first, mode


@pytest.mark.parametrize("cw,ch,interval,w,h", WINDOW_PARAMS)
def test_window_rects_and_grouping(ctx_for, cw, ch, interval, w, h):
    """rect sizes are cw x ch times the level's scale (ccv.js:710-711), on the host and in the device grouping"""
    per = dv.window_expected(cw, ch, interval, w, h)[0]
    check_rects_and_grouping(ctx_for((cw, ch), interval), dv.triple(w, h), per, interval, dv.window_cascade(cw, ch).blob, cw, ch)


# ---- vectors recorded from the reference -----------------------------------------------------------------------------------------------

def check_recorded_case(case, casc, interval, level_dims, grouped=True):
    w, h = case["w"], case["h"]
    frame = synth.make(case["gen"], w, h)
    assert zlib.crc32(frame.tobytes()) == case["input_crc"]
    c = Context(cascade=casc, interval=interval, hit_capacity=1 << 16)
    try:
        hits, _ = detect(c, frame[None], level_dims=level_dims)
        nlevels = case.get("nlevels", c.num_levels)
        assert c.num_levels == nlevels
        order = dv.creation_order(nlevels, interval + 1)
        assert len(order) == len(case["pyramid"])
        assert zlib.crc32(c.pyramid_readback(0, 0, 0).tobytes()) == case["gray_crc"]
        for (i, s), g in zip(order, case["pyramid"]):
            p = c.pyramid_readback(0, i, s)
            assert (p.shape[1], p.shape[0]) == (g["w"], g["h"]), f"level {i} size"
            assert zlib.crc32(p.tobytes()) == g["crc"], f"pyramid level {i} slot {s}"
        rects = c.hits_to_rects(hits)
        assert len(rects) == len(case["raw"]) > 0
        for r, g in zip(rects, case["raw"]):
            for k in ("x", "y", "width", "height", "confidence"):
                assert r[k] == g[k], (k, r, g)
        assert_hits_equal(hits, [ho.detect_raw(frame, casc.blob, interval=interval, cap=1 << 20)])
        if grouped:
            got = c.group_rects(rects, case["min_neighbors"])
            assert len(got) == len(case["grouped"])
            for r, g in zip(got, case["grouped"]):
                for k in RECT_FIELDS:
                    assert r[k] == g[k], (k, r, g)
    finally:
        c.close()


@pytest.mark.parametrize("dims", ["recorded_level_dims", "own_level_dims"])
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_recorded_case(case, dims):
    """plane CRCs in creation order, raw rects and grouped rects of the reference itself — once with the reference's level sizes handed to
    ht_set_geometry, once with the library's own (level_dims = None): its std::pow sizes must be the reference's"""
    casc = load_cascade() if case["cascade"] is None else dv.cascade_from_json(GOLDEN["cascades"][case["cascade"]])
    check_recorded_case(case, casc, case["interval"], dv.recorded_level_dims(case) if dims == "recorded_level_dims" else None)


def test_recorded_interval3_case_at_plane_and_raw_hit_level(cascade):
    """face_interval3_160x120 of tests/golden/detect.json (tests/test_gpu_group.py compares it after grouping only)"""
    case = next(c for c in DETECT["cases"] if c["name"] == "face_interval3_160x120")
    check_recorded_case(case, cascade, 3, None)

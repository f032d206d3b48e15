"""The device grouping (ht_group.hip: ht_detect_best_enqueue / _collect / _collect_requeue, ht_detect_grouped,
ht_detect_best_records_device, ht_group_hits) against the reference's recorded vectors, the CPU oracle and the host route.  Everything is
compared byte for byte: grouped rects, best faces, the 64-byte records.  The regimes of the per-frame kernel all run here: one wavefront,
a full 1024-thread workgroup (synthetic and behind a real scan), the same template at 128 / 256 / 512 threads (group_cap), frames over
the default cap finished on the host, and batches of more than 1024 frames through the bucket kernel's frame loop."""
import ctypes as C
import functools
import json
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import group_cases as gc
from conftest import ROOT, load_golden
from headtrackr_amd import distributed as hd
from headtrackr_amd import native, synth
from headtrackr_amd.api import Context, HtError
from headtrackr_amd.native import HT_DETECT_WHITEBALANCE, HT_SCAN_STATS
from oracle import ht_oracle as ho

pytestmark = pytest.mark.gpu

DETECT = load_golden("detect.json")
FIELDS = ("x", "y", "width", "height", "confidence", "neighbors")
NODE = shutil.which("node")


def _interval(case):
    return 3 if "interval3" in case["name"] else 5


@functools.lru_cache(maxsize=None)
def _frame(name):
    case = next(c for c in DETECT["cases"] if c["name"] == name)
    f = synth.make(case["gen"], case["w"], case["h"])
    assert zlib.crc32(f.tobytes()) == case["input_crc"]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _oracle_grouped(name, cascade_blob, min_neighbors):
    case = next(c for c in DETECT["cases"] if c["name"] == name)
    g = ho.detect_objects(_frame(name), cascade_blob, _interval(case), min_neighbors)
    g.setflags(write=False)
    return g


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx3():
    c = Context(interval=3)
    yield c
    c.close()


def _device_route(c, frames, min_neighbors, flags=0, frame_base=0):
    frames = np.ascontiguousarray(frames)
    n, h, w, _ = frames.shape
    c.set_geometry(w, h, n)
    c.upload(frames)
    c.detect_enqueue(flags)
    c.detect_best_enqueue(min_neighbors, frame_base)
    best, total = c.detect_best_collect()
    return best.copy(), total


def _assert_rects(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (what, got, want)


@pytest.mark.parametrize("case", DETECT["cases"], ids=lambda c: c["name"])
def test_golden_case_through_the_device_route(ctx, ctx3, cascade, case):
    """every recorded case: grouped rects and best face equal the reference's recorded `grouped` and the oracle's, byte for byte"""
    c = ctx3 if _interval(case) == 3 else ctx
    mn = case["min_neighbors"]
    best, total = _device_route(c, _frame(case["name"])[None], mn)
    assert total == len(case["raw"])
    grouped = c.detect_grouped(0)
    assert len(grouped) == len(case["grouped"])
    for r, g in zip(grouped, case["grouped"]):
        for k in FIELDS:
            assert r[k] == g[k], (k, r, g)
    want = _oracle_grouped(case["name"], cascade.blob, mn)
    _assert_rects(grouped, want, case["name"])
    assert best[0].tobytes() == gc.select_best(want).tobytes()
    if _interval(case) == 5:  # (the oracle's best_faces is the interval-5 pipeline)
        assert best[0].tobytes() == ho.best_faces(_frame(case["name"])[None], cascade.blob, mn)[0].tobytes()


def test_golden_frames_as_one_shuffled_batch_with_empty_frames_between(ctx, cascade):
    """two_faces, mixed5, mixed2 of the recorded cases in one detect batch, out of order, empty frames between them — and the same three
    plus faces_1280x720 (another geometry: its raw hits come from a batch of its own) as ONE shuffled hit list through ht_group_hits"""
    names = {1: "two_faces_320x240", 3: "mixed5_320x240", 4: "mixed2_320x240"}
    frames = np.stack([_frame(names[f]) if f in names else _frame("noise_320x240") for f in range(6)])
    best, total = _device_route(ctx, frames, 1, frame_base=40)
    lists = [ctx.detect_grouped(f).copy() for f in range(6)]
    for f in range(6):
        if f in names:
            want = _oracle_grouped(names[f], cascade.blob, 1)
            case = next(c for c in DETECT["cases"] if c["name"] == names[f])
            assert [tuple(r[k] for k in FIELDS) for r in lists[f]] == [tuple(g[k] for k in FIELDS) for g in case["grouped"]]
            _assert_rects(lists[f], want, names[f])
            assert best[f].tobytes() == gc.select_best(want).tobytes()
        else:
            assert len(lists[f]) == 0 and best[f]["confidence"] == -10000.0 and best[f]["neighbors"] == 0
    # the hit lists of four recorded frames (two geometries), renumbered into a batch of 9 frames and shuffled
    slots = {1: "two_faces_320x240", 2: "faces_1280x720", 5: "mixed2_320x240", 7: "mixed5_320x240"}
    parts = []
    for f, name in slots.items():
        hits, _ = ctx.detect_raw(_frame(name)[None])
        hits = hits.copy()
        hits["frame"] = f
        parts.append(hits)
    allhits = np.concatenate(parts)
    allhits = allhits[np.random.default_rng(5).permutation(len(allhits))]
    best, grouped, ng = ctx.group_hits(allhits, 9, 1)
    k = 0
    for f in range(9):
        want = _oracle_grouped(slots[f], cascade.blob, 1) if f in slots else np.zeros(0, dtype=ho.RECT_DTYPE)
        _assert_rects(grouped[k:k + int(ng[f])], want, f)
        assert best[f].tobytes() == gc.select_best(want).tobytes()
        k += int(ng[f])


_CTX_BY_OPTIONS = {}


@pytest.fixture(scope="module")
def ctx_for():
    def get(options):
        if options not in _CTX_BY_OPTIONS:
            _CTX_BY_OPTIONS[options] = Context(options=options)
        return _CTX_BY_OPTIONS[options]

    yield get
    for c in _CTX_BY_OPTIONS.values():
        c.close()
    _CTX_BY_OPTIONS.clear()


def _over_cap_frames(c):
    return int(c.kernel_times(reset=True).get("grp_over_cap_frames", {"launches": 0})["launches"])


@pytest.mark.parametrize("name,mn", gc.case_ids(), ids=lambda v: str(v))
def test_synthetic_case_through_group_hits(ctx_for, name, mn):
    """every case of tests/group_cases.py: every byte of best, grouped and ngrouped equals the oracle's"""
    case = gc.cases()[name]
    c = ctx_for(case["options"])
    _over_cap_frames(c)
    best, grouped, ng = c.group_hits(case["hits"], case["nframes"], mn)
    wbest, wgrouped, wng = gc.expected(name, mn)
    assert np.array_equal(ng, wng), (ng, wng)
    assert grouped.tobytes() == wgrouped.tobytes()
    assert best.tobytes() == wbest.tobytes()
    # the status words: exactly the frames with more hits than the context's cap are finished on the host
    assert _over_cap_frames(c) == gc.over_cap_frames(name)


def test_every_cap_route_returns_the_same_bytes(ctx, ctx_for):
    """one hit list (frames of 64 .. 513 hits) on a default context and under group_cap=128, 256, 512 and 300 (k_grp_frames<1024> launched
    with 128, 256, 512 and 256 threads): the frames above each cap go to the host, every route returns the oracle's bytes"""
    case = gc.cases()["caps_128"]
    want = gc.expected("caps_128", 1)
    over = []
    for options in (None, "group_cap=128", "group_cap=256", "group_cap=512", "group_cap=300"):
        c = ctx if options is None else ctx_for(options)
        _over_cap_frames(c)
        best, grouped, ng = c.group_hits(case["hits"], case["nframes"], 1)
        assert np.array_equal(ng, want[2]) and grouped.tobytes() == want[1].tobytes() and best.tobytes() == want[0].tobytes(), options
        over.append(_over_cap_frames(c))
        assert over[-1] == gc.over_cap_frames("caps_128", options)
    # frames with MORE hits than the cap, of 64, 65, 128, 129, 256, 257, 512, 513: a frame of exactly `cap` hits is a full workgroup
    assert over == [0, 5, 3, 1, 3]


def test_a_batch_of_2500_frames_returns_the_last_frames_list(ctx):
    """k_grp_bucket's frame loop runs three passes: the bucket starts carry over, and the last frame's list is the oracle's"""
    for name in ("frames_2500", "last_of_2500_only"):
        case = gc.cases()[name]
        best, grouped, ng = ctx.group_hits(case["hits"], case["nframes"], 1)
        wbest, wgrouped, wng = gc.expected(name, 1)
        assert len(ng) == 2500 and wng[2499] > 0 and ng[2499] == wng[2499]
        assert grouped[len(grouped) - int(ng[2499]):].tobytes() == wgrouped[len(wgrouped) - int(wng[2499]):].tobytes()
        assert best[2499].tobytes() == wbest[2499].tobytes() and best[2499]["neighbors"] > 0
        assert np.array_equal(ng, wng) and grouped.tobytes() == wgrouped.tobytes() and best.tobytes() == wbest.tobytes()


def test_overflow_frame_is_flagged_only_under_the_lowered_cap(ctx, ctx_for):
    """the same hit list on a default context (cap 1024) is grouped on the device; under group_cap=64 the 65-hit frame's status word is
    set, the 64-hit frame next to it is not, and both routes return the same bytes"""
    case = gc.cases()["overflow"]
    _over_cap_frames(ctx)
    a = ctx.group_hits(case["hits"], case["nframes"], 1)
    assert _over_cap_frames(ctx) == 0
    low = ctx_for("group_cap=64")
    _over_cap_frames(low)
    b = low.group_hits(case["hits"], case["nframes"], 1)
    assert _over_cap_frames(low) == 1
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_hits_with_a_frame_or_scale_out_of_range_are_reported_not_used(ctx):
    hits = gc.cases()["one_frame"]["hits"].copy()
    want = gc.expected("one_frame", 1)
    for field, value in (("frame", 1), ("frame", 0xFFFFFFFF), ("scale", native.HT_MAX_LEVELS), ("scale", 255)):
        bad = hits.copy()
        bad[field][5] = value
        with pytest.raises(HtError) as e:
            ctx.group_hits(bad, 1, 1)
        assert e.value.status == -1, (field, value)
    best, grouped, ng = ctx.group_hits(hits, 1, 1)  # and the context is as good as before
    assert best.tobytes() == want[0].tobytes() and grouped.tobytes() == want[1].tobytes()
    with pytest.raises(HtError):
        ctx.group_hits(hits, 0, 1)


# ---- behind a real scan that crowds a frame: the hits arrive in the scan's atomic order, hundreds to one frame ----------------------------


def _assert_raw_equals_the_oracle(c, batch, blob):
    """detect_raw per frame: keys and confidence bits (the scan's hit append at this density)"""
    hits, counts = c.detect_raw(gc.scan_frames(batch))
    want = gc.scan_raw(batch, blob)
    assert [int(n) for n in counts] == [len(r) for r in want]
    k = 0
    for f, r in enumerate(want):
        got = hits[k:k + len(r)]
        k += len(r)
        assert (got["frame"] == f).all()
        for fld in ("scale", "q", "y", "x"):
            assert np.array_equal(got[fld].astype(np.int64), r[fld].astype(np.int64)), (f, fld)
        assert np.array_equal(got["sum"].view(np.uint64), r["sum"].view(np.uint64)), f


def _assert_scan_batch(c, batch, blob, mn, over_cap, requeue=False):
    """detect_enqueue, detect_best_enqueue(mn, 7), detect_best_collect, detect_grouped(f) on a scan batch: best faces, total, every grouped
    list and the device's record buffer equal the oracle's; `over_cap`: the frames finished on the host"""
    frames = gc.scan_frames(batch)
    wbest, wlists = gc.scan_expected(batch, blob, mn)
    wtotal = sum(len(r) for r in gc.scan_raw(batch, blob))
    n, h, w, _ = frames.shape
    c.set_geometry(w, h, n)
    c.upload(frames)
    _over_cap_frames(c)
    c.detect_enqueue()
    c.detect_best_enqueue(mn, 7)
    if requeue:  # (the batch the requeue started owns the lists and the records until it is collected: best faces and total only)
        best, total = c.detect_best_collect_requeue()
        assert total == wtotal and best.tobytes() == wbest.tobytes()
        assert _over_cap_frames(c) == over_cap
    best, total = c.detect_best_collect()
    best = best.copy()
    assert total == wtotal
    for f in range(n):
        _assert_rects(c.detect_grouped(f), wlists[f], (batch, mn, f))
    assert best.tobytes() == wbest.tobytes()
    ptr, nrec = c.detect_best_records_ptr()
    assert nrec == n
    assert c.device_download(ptr, n * 64).tobytes() == hd.pack_best_records(wbest, 7).tobytes()
    assert _over_cap_frames(c) == over_cap


def test_real_scan_fills_a_workgroup(ctx, ctx_for, cascade):
    """640x480, frames 0 and 3 tiled with faces (755 raw hits each, 88 grouped rects), one face on frame 1, noise on frame 2: raw hits,
    grouped lists, best faces and records equal the oracle's on a default context; under group_cap=512 the two tiled frames are finished
    on the host and the bytes are the same; a requeue round returns them twice"""
    blob = cascade.blob
    raw = gc.scan_raw("full_640x480", blob)
    assert 512 < len(raw[0]) <= 1024 and len(raw[0]) == len(raw[3]) and len(raw[2]) == 0
    _assert_raw_equals_the_oracle(ctx, "full_640x480", blob)
    # the two contexts in turn: each replays its captured detect sequence after the other one has allocated its geometry and run a batch
    # (LABLOG 2026-10-20: the replayed memset node of the counters once left a garbage hit count exactly here)
    for mn in (1, 2):
        _assert_scan_batch(ctx, "full_640x480", blob, mn, 0)
        _assert_scan_batch(ctx_for("group_cap=512"), "full_640x480", blob, mn, 2)
    _assert_scan_batch(ctx, "full_640x480", blob, 1, 0, requeue=True)
    _assert_scan_batch(ctx_for("group_cap=512"), "full_640x480", blob, 1, 2, requeue=True)


def test_real_scan_over_the_default_cap(ctx, cascade):
    """960x540, frame 0 tiled with faces (1473 raw hits > 1024), one face on frame 1: frame 0 is flagged, finished by the collect call on
    the host and its completed record written back to the device; detect_grouped(0) is the host's list, detect_grouped(1) the device's.
    The second batch replays the context's captured detect sequence behind a collect call that finished a frame on the host."""
    blob = cascade.blob
    raw = gc.scan_raw("over_960x540", blob)
    assert len(raw[0]) > 1024 and 0 < len(raw[1]) <= 64
    _assert_raw_equals_the_oracle(ctx, "over_960x540", blob)
    for mn in (1, 2):
        _assert_scan_batch(ctx, "over_960x540", blob, mn, 1)
    wbest, wlists = gc.scan_expected("over_960x540", blob, 1)
    assert len(wlists[0]) == 153 and wbest[0]["neighbors"] > 0  # the record compared above is a face's, not the flagged frame's placeholder


def test_hit_capacity_is_a_limit_not_a_fault(cascade):
    """hit_capacity=100: a scan that finds 129 hits is reported by detect_best_collect with HT_ERR_CAPACITY and the next batch on the
    context is exact; group_hits takes exactly hit_capacity hits and refuses one more"""
    import init_best_cases as ib

    blob = cascade.blob
    tiled = ib.frames()[ib.TILED]
    assert ib.raw_counts(blob)[ib.TILED] == 129
    one = synth.face_frame(ib.W, ib.H, [(100, 60, 96)])
    wone = ho.detect_objects(one, blob, 5, 1)
    assert 0 < len(ho.detect_raw(one, blob)) < 100 and len(wone) == 1
    c = Context(hit_capacity=100)
    try:
        c.set_geometry(ib.W, ib.H, 1)
        c.upload(tiled[None])
        c.detect_enqueue()
        c.detect_best_enqueue(1, 0)
        with pytest.raises(HtError) as e:
            c.detect_best_collect()
        assert e.value.status == native.HT_ERR_CAPACITY == -4
        best, total = _device_route(c, one[None], 1)
        assert total == len(ho.detect_raw(one, blob)) and best[0].tobytes() == gc.select_best(wone).tobytes()
        _assert_rects(c.detect_grouped(0), wone, "after the capacity error")
        rng = np.random.default_rng(100)
        hits = np.concatenate([gc.clustered(rng, 0, 70), gc.clustered(rng, 1, 31)])
        hits = hits[rng.permutation(len(hits))]
        full = hits[:100]
        want = gc.oracle_result(full, 2, 1)
        best, grouped, ng = c.group_hits(full, 2, 1)
        assert np.array_equal(ng, want[2]) and grouped.tobytes() == want[1].tobytes() and best.tobytes() == want[0].tobytes()
        with pytest.raises(HtError) as e:
            c.group_hits(hits, 2, 1)
        assert len(hits) == 101 and e.value.status == -1
        best, grouped, ng = c.group_hits(full, 2, 1)  # and the context is as good as before
        assert grouped.tobytes() == want[1].tobytes() and best.tobytes() == want[0].tobytes()
    finally:
        c.close()


@functools.lru_cache(maxsize=None)
def _c2_frames():
    f = np.ascontiguousarray(synth.mixed_batch(64, 320, 240, seed0=1234))
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def c2_host_route():
    c = Context()
    try:
        c.set_geometry(320, 240, 64)
        c.upload(_c2_frames())
        c.detect_enqueue()
        best, total = c.detect_collect_best(1)
        return best.copy(), total
    finally:
        c.close()


def test_c2_shape_batch_equals_the_host_route(c2_host_route):
    """64 x 320x240 frames of the benchmark's generator: device route == ht_detect_collect_best for every frame and total_hits; the
    requeue form over three consecutive batches == three host-route batches (the frames stay bound: the same answer three times)"""
    want, wtotal = c2_host_route
    c = Context()
    try:
        best, total = _device_route(c, _c2_frames(), 1)
        assert total == wtotal and total > 100 and best.tobytes() == want.tobytes()
        c.detect_enqueue()
        c.detect_best_enqueue(1, 0)
        for _ in range(3):
            got, n = c.detect_best_collect_requeue()
            assert n == wtotal and got.tobytes() == want.tobytes()
        got, n = c.detect_best_collect()  # the batch the last requeue started
        assert n == wtotal and got.tobytes() == want.tobytes()
        with pytest.raises(HtError) as e:
            c.detect_best_collect()
        assert e.value.status == -6
        c.detect_enqueue()
        with pytest.raises(HtError) as e:  # a batch in flight that no best-enqueue followed
            c.detect_best_collect()
        assert e.value.status == -6
        hits, counts = c.detect_collect()  # ... is still collectable the plain way
        assert len(hits) == wtotal
        with pytest.raises(HtError) as e:
            c.detect_best_enqueue(1, 0)  # nothing in flight
        assert e.value.status == -6
    finally:
        c.close()


def test_record_buffer_equals_pack_best_records_and_is_gathered(c2_host_route):
    """the device buffer behind ht_detect_best_records_device == pack_best_records(host best, frame_base), byte for byte, before and after
    ht_allgather_records on one rank through RCCL (force_rccl=1)"""
    want, _ = c2_host_route
    c = Context(options="force_rccl=1")
    try:
        with pytest.raises(HtError) as e:
            c.detect_best_records_ptr()  # no device-grouped batch yet
        assert e.value.status == -6
        _device_route(c, _c2_frames(), 1, frame_base=1000)
        ptr, n = c.detect_best_records_ptr()
        assert n == 64 and ptr
        rec = hd.pack_best_records(want, 1000)
        assert (rec[:, 4] == -10000.0).any() and (rec[:, 5] > 0).any()
        assert c.device_download(ptr, n * 64).tobytes() == rec.tobytes()
        handles, bufs = (C.c_void_p * 1)(c._h), (C.c_void_p * 1)(ptr)
        assert native.lib().ht_allgather_records(handles, 1, bufs, n * 64) == 0
        assert c.device_download(ptr, n * 64).tobytes() == rec.tobytes()
    finally:
        c.close()


def test_neighbours_are_undisturbed(cascade):
    """a device-grouped detect between enqueue-only track steps leaves the track objects and ht_camshift_stats as they are without it;
    ht_detect_whitebalance and ht_stage_counts report the batch collected last, as after ht_detect_collect"""
    w, h, n = 320, 240, 4
    frames = [np.ascontiguousarray(np.stack([synth.face_frame(w, h, [(100 + 3 * k + s, 60 + k, 96)]) for s in range(n)])) for k in range(3)]
    rects = [[100 + s, 60, 96, 96] for s in range(n)]

    def run(with_detect):
        c = Context()
        try:
            c.set_geometry(w, h, n)
            c.camshift_reserve(n)
            c.upload(frames[0])
            c.camshift_init(rects)
            out, extra = [], None
            for k in (1, 2):
                c.upload(frames[k])
                c.camshift_track(n, fetch=False)
                if with_detect and k == 1:
                    c.detect_enqueue(HT_DETECT_WHITEBALANCE | HT_SCAN_STATS)
                    c.detect_best_enqueue(1, 0)
                    best, total = c.detect_best_collect()
                    extra = (best.copy(), total, c.detect_whitebalance().copy(), c.stage_counts().copy())
                out.append(c.camshift_track_collect(n).copy())
            px, calls = c.camshift_stats(n)
            return out, np.asarray(px).copy(), np.asarray(calls).copy(), extra
        finally:
            c.close()

    a, apx, acalls, _ = run(False)
    b, bpx, bcalls, extra = run(True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(apx, bpx) and np.array_equal(acalls, bcalls)
    best, total, wb, stages = extra
    ref = Context()
    try:
        ref.set_geometry(w, h, n)
        ref.upload(frames[1])
        ref.detect_enqueue(HT_DETECT_WHITEBALANCE | HT_SCAN_STATS)
        wbest, wtotal = ref.detect_collect_best(1)
        assert total == wtotal and best.tobytes() == wbest.tobytes() and total > 0
        assert np.array_equal(wb, ref.detect_whitebalance()) and np.array_equal(stages, ref.stage_counts()) and stages[0] > 0
    finally:
        ref.close()


@pytest.mark.parametrize("n", [4, 1])
def test_device_grouped_collect_carries_the_whitebalance_sums(cascade, n):
    """ht_detect_best_collect and its requeue form with HT_DETECT_WHITEBALANCE: the head they share with ht_detect_collect (one pinned copy,
    the batch's channel sums behind it, one wait) gives them the whitebalance values and best records that ht_detect_collect +
    ht_detect_whitebalance + ht_best_faces give for the same frames — and the oracle's values.  A requeued batch reports its OWN flag."""
    w, h = 320, 240
    frames = np.ascontiguousarray(np.stack([synth.face_frame(w, h, [(100 + 7 * s, 60 + s, 96)], gray=90 + 20 * s) for s in range(n)]))
    want_wb = np.array([ho.whitebalance(f) for f in frames])
    assert len(set(want_wb)) == n
    host, dev = Context(), Context()
    try:
        host.set_geometry(w, h, n)
        host.upload(frames)
        host.detect_enqueue(HT_DETECT_WHITEBALANCE)
        hits, counts = host.detect_collect()
        assert np.array_equal(host.detect_whitebalance(), want_wb)
        want_best = host.best_faces(hits, counts, 1)
        assert len(hits) > 0 and (want_best["neighbors"] > 0).any()

        dev.set_geometry(w, h, n)
        dev.upload(frames)
        dev.detect_enqueue(HT_DETECT_WHITEBALANCE)
        dev.detect_best_enqueue(1, 0)
        best, total = dev.detect_best_collect()
        assert total == len(hits) and best.tobytes() == want_best.tobytes()
        assert np.array_equal(dev.detect_whitebalance(), want_wb)
        dev.detect_enqueue(HT_DETECT_WHITEBALANCE)
        dev.detect_best_enqueue(1, 0)
        best, total = dev.detect_best_collect_requeue(next_flags=0)  # collects a batch WITH the sums, starts one without
        assert total == len(hits) and best.tobytes() == want_best.tobytes()
        assert np.array_equal(dev.detect_whitebalance(), want_wb)  # the collected batch's, although the one in flight has none
        best, total = dev.detect_best_collect_requeue(next_flags=HT_DETECT_WHITEBALANCE)  # ... and the other way round
        assert total == len(hits) and best.tobytes() == want_best.tobytes()
        with pytest.raises(HtError) as e:
            dev.detect_whitebalance()
        assert e.value.status == -6
        best, total = dev.detect_best_collect()
        assert total == len(hits) and best.tobytes() == want_best.tobytes()
        assert np.array_equal(dev.detect_whitebalance(), want_wb)
    finally:
        host.close()
        dev.close()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_device_grouping_from_node(tmp_path, cascade):
    """tests/js/group_gpu.js on the product addon: new ccv.DeviceBatch(.., {grouping: 'device'}) against the default route, the oracle's best
    faces and the reference's recorded grouped rects (detectBest, detect, whitebalance, the C5 loop's step functions), then the raw addon
    calls — detectBestRecords, groupHits — and the call-sequence errors"""
    from headtrackr_amd import build

    build.build_all()
    job = gc.js_job(tmp_path, cascade.blob, DETECT)
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "group_gpu.js"), str(jf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] >= 20 and out["grouped_rects"] == 8 and out["initialised"] == 2 and out["state_errors"] == 4 and out["hits"] == 59

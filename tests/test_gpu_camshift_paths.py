"""The camshift code paths that tests/test_gpu_camshift.py reaches only by accident, each pushed into its state on purpose and judged by
the CPU oracle through the C ABI:

  A  stream ranges [first, first + n) with first > 0 and reservations larger than the batch — the kernels index tracker state by
     first + s, and frames, chunk histograms, the cluster LUT, the exchange slots, the result slot and the ring's flag words by s;
  B  the LDS search-region cache of the mean-shift kernels: windows that leave it in the middle of a call, its capacity and margin
     boundaries (option cs_region), margins clamped by the frame, the two ways the single-launch kernel fills it, the two capacities;
  C  the two initTracker kernels at rect sizes next to their lane / row quanta;
  D  the chunk histograms at pixel counts next to the chunking quanta;
  E  the schedule a call takes with DEFAULT options (parts A - D force one): both sides of every threshold of the decision table of
     headtrackr_amd/csrc/ht_cs_schedule.h, told apart by the profiling timers the call leaves behind.

Inputs, and the CPU proof that they reach these states and that the reference is unambiguous on them: tests/cs_cases.py,
tests/test_cs_cases_cpu.py.  Every track() call is checked with check() and, in parts A - D, is in an assert_all_exact(): the oracle's integers, no tie
class.  The module's calls are in the tally of camshift_parity.json (tests/test_gpu_camshift.py writes it), with sub-totals "paths" and
"paths/<schedule>"."""
import numpy as np
import pytest

import cs_cases as cc
import cs_schedule
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray, multiprocessor_count
from test_gpu_camshift import SCHEDULES, assert_all_exact, check

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6


@pytest.fixture(scope="module", params=list(SCHEDULES))
def ctx(request):
    """(schedule name, context) — the four camshift schedules of tests/test_gpu_camshift.py"""
    c = Context(options=SCHEDULES[request.param])
    yield request.param, c
    c.close()


@pytest.fixture(scope="module")
def plain_ctx():
    c = Context()
    yield c
    c.close()


def _tally(sched):
    return ("paths", f"paths/{sched}")


def _expected(seq):
    """[(search window, track object)] of the sequence's calls from the oracle, computed once"""
    if not hasattr(seq, "_expected"):
        seq._expected = [(sw, to) for (_before, sw, to) in seq.oracle_calls()]
    return seq._expected


def _track_single(c, sched, seq, stats, tag=""):
    """one tracker on stream 0, one upload + track() per call; returns the raw bytes of the track objects"""
    c.set_geometry(seq.w, seq.h, 1)
    c.camshift_reserve(1)
    c.upload(seq.frames[0][None])
    c.camshift_init([seq.rect])
    raw = b""
    for k, (sw, to) in enumerate(_expected(seq), 1):
        c.upload(seq.frames[k][None])
        got = c.camshift_track(1, calc_angles=True)
        check(got[0], sw, to, stats, where=(seq.name + tag, sched, k), tally=_tally(sched))
        raw += got.tobytes()
    assert len(stats) >= seq.ncalls
    return raw


def _init_ranges(c, layout, bind=None):
    """reserve the layout, initialise each range with a call of its own from its own frames and rects; returns (ranges, streams)"""
    res, ranges = cc.LAYOUTS[layout]
    seqs = cc.layout_streams(layout)
    c.set_geometry(320, 240, max(n for _f, n in ranges))
    c.camshift_reserve(res)
    for first, n in ranges:
        if bind:
            bind(first, n, 0)
        else:
            c.upload(cc.range_batch(seqs, first, n, 0))
        c.camshift_init([seqs[first + s].rect for s in range(n)], first=first)
    return ranges, seqs


def _check_range(got, seqs, first, n, k, stats, sched, what):
    for s in range(n):
        sw, to = _expected(seqs[first + s])[k - 1]
        check(got[s], sw, to, stats, where=(what, sched, first + s, k), tally=_tally(sched))


# ---- A: stream ranges and reservations ----------------------------------------------------------------------------------------------------

# (range, call) in the order they are issued: the ranges advance interleaved and at different paces; range 1 never gets its 4th call
RANGE_ORDER = [(0, 1), (1, 1), (0, 2), (2, 1), (1, 2), (2, 2), (2, 3), (0, 3), (1, 3), (0, 4), (2, 4)]


@pytest.mark.parametrize("layout", list(cc.LAYOUTS))
def test_disjoint_stream_ranges_track_their_own_streams(ctx, layout):
    """R reserved streams, three disjoint ranges initialised and tracked by separate calls (stream first + s <-> frame slot s), every
    stream against its own oracle: a wrong s / first + s shows up as another stream's model, window or result.  Then the per-stream
    counters: calls == the track calls the stream's range received, 0 for the streams never touched; a reset clears its range only."""
    sched, c = ctx
    ranges, seqs = _init_ranges(c, layout)
    res = cc.LAYOUTS[layout][0]
    c.camshift_stats(res, first=0, reset=True)
    stats = []
    for ri, k in RANGE_ORDER:
        first, n = ranges[ri]
        c.upload(cc.range_batch(seqs, first, n, k))
        got = c.camshift_track(n, calc_angles=True, first=first)
        _check_range(got, seqs, first, n, k, stats, sched, layout)
    assert len(stats) == sum(ranges[ri][1] for ri, _k in RANGE_ORDER)
    assert_all_exact(stats, f"{layout}, {sched}")
    want = np.zeros(res, dtype=np.uint64)
    for ri, _k in RANGE_ORDER:
        first, n = ranges[ri]
        want[first : first + n] += 1
    px, calls = c.camshift_stats(res, first=0, reset=False)
    assert np.array_equal(calls, want), (calls, want)
    assert np.array_equal(px > 0, want > 0)
    first, n = ranges[1]
    px1, calls1 = c.camshift_stats(n, first=first, reset=True)  # read and clear the middle range only
    assert np.array_equal(calls1, want[first : first + n]) and np.array_equal(px1, px[first : first + n])
    want[first : first + n] = 0
    px2, calls2 = c.camshift_stats(res, first=0, reset=False)
    assert np.array_equal(calls2, want) and np.array_equal(px2[want > 0], px[want > 0]) and not px2[want == 0].any()


def test_track_sequence_on_stream_ranges(ctx):
    """the same through ht_camshift_track_sequence(first, ...) on device-resident frames, every call's objects fetched: the fused
    schedules walk a stream's calls inside one launch, the other two launch per call"""
    sched, c = ctx
    layout = "r24"
    _res, ranges = cc.LAYOUTS[layout]
    seqs = cc.layout_streams(layout)
    dev = {(first, k): DeviceArray(cc.range_batch(seqs, first, n, k)) for first, n in ranges for k in range(cc.RANGE_STEPS + 1)}
    try:
        _init_ranges(c, layout, bind=lambda first, n, k: c.bind_device(dev[first, k].ptr, n))
        stats = []
        for ri, ks in [(0, (1, 2)), (1, (1, 2, 3, 4)), (2, (1, 2)), (0, (3, 4)), (2, (3,)), (2, (4,))]:
            first, n = ranges[ri]
            got = c.camshift_track_sequence([dev[first, k].ptr for k in ks], n, calc_angles=True, first=first, fetch="all")
            assert got.shape == (len(ks), n)
            for i, k in enumerate(ks):
                _check_range(got[i], seqs, first, n, k, stats, sched, "sequence")
        assert len(stats) == cc.RANGE_STEPS * sum(n for _f, n in ranges)
        assert_all_exact(stats, f"track_sequence with first > 0, {sched}")
    finally:
        c.synchronize()
        for d in dev.values():
            d.free()


@pytest.mark.parametrize("flags", [1, 0], ids=["cs_flags=1", "cs_flags=0"])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_enqueue_only_calls_on_a_stream_range(sched, flags):
    """enqueue-only track() calls (results in the pinned ring, completion by per-stream flag words written by the kernel or — cs_flags=0 —
    by an event) on ranges with first > 0, two calls outstanding at a time"""
    layout = "r24"
    _res, ranges = cc.LAYOUTS[layout]
    seqs = cc.layout_streams(layout)
    c = Context(options=SCHEDULES[sched] + f",cs_flags={flags}")
    dev = {(first, k): DeviceArray(cc.range_batch(seqs, first, n, k)) for first, n in ranges for k in range(cc.RANGE_STEPS + 1)}
    try:
        _init_ranges(c, layout, bind=lambda first, n, k: c.bind_device(dev[first, k].ptr, n))
        stats = []
        for ri, ks in [(2, (1, 2)), (1, (1, 2)), (2, (3, 4)), (1, (3, 4))]:
            first, n = ranges[ri]
            assert first > 0
            for k in ks:
                c.bind_device(dev[first, k].ptr, n)
                c.camshift_track(n, calc_angles=True, first=first, fetch=False)
            for k in ks:
                _check_range(c.camshift_track_collect(n), seqs, first, n, k, stats, sched, f"enqueue-only cs_flags={flags}")
        assert len(stats) == cc.RANGE_STEPS * (ranges[1][1] + ranges[2][1])
        assert_all_exact(stats, f"enqueue-only with first > 0, {sched}, cs_flags={flags}")
    finally:
        c.synchronize()
        c.close()
        for d in dev.values():
            d.free()


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_debug_histograms_of_a_stream_range(sched):
    """ht_camshift_debug_hist(stream) after a track() call on [first, first + n), first > 0: the full-frame histogram of stream first + s
    is that of slot s's frame, the model that of the stream's own rect; a stream outside the last call's range is HT_ERR_STATE, not
    another stream's bins"""
    layout = "r24"
    c = Context(options=SCHEDULES[sched] + ",cs_keep_hist=1")
    try:
        ranges, seqs = _init_ranges(c, layout)
        stats = []
        for first, n in (ranges[1], ranges[2]):
            c.upload(cc.range_batch(seqs, first, n, 1))
            _check_range(c.camshift_track(n, calc_angles=True, first=first), seqs, first, n, 1, stats, sched, "debug-hist")
        assert_all_exact(stats, f"debug-hist, {sched}")
        first, n = ranges[2]  # the last call's range
        for s in range(n):
            seq = seqs[first + s]
            model, cur = c.camshift_debug_hist(first + s)
            assert np.array_equal(cur.astype(np.int64), cc.frame_histogram(seq.frames[1])), (first, s)
            assert np.array_equal(model.astype(np.int64), cc.model_histogram(seq.frames[0], seq.rect)), (first, s)
            assert int(cur.sum()) == 320 * 240 and int(model.sum()) == seq.rect[2] * seq.rect[3]
        for stream in (0, ranges[1][0], first - 1, 12):  # tracked earlier, just below the range, never initialised
            model, _ = c.camshift_debug_hist(stream, current=False)
            if stream in seqs:
                assert np.array_equal(model.astype(np.int64), cc.model_histogram(seqs[stream].frames[0], seqs[stream].rect)), stream
            else:
                assert not model.any()
            with pytest.raises(HtError) as e:
                c.camshift_debug_hist(stream)
            assert e.value.status == HT_ERR_STATE, stream
        with pytest.raises(HtError) as e:
            c.camshift_debug_hist(cc.LAYOUTS[layout][0])
        assert e.value.status == HT_ERR_INVALID
    finally:
        c.close()


@pytest.mark.parametrize("seq", cc.growing(), ids=lambda s: s.name)
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_reservation_grows_between_calls(sched, seq):
    """ht_camshift_reserve keeps existing trackers when it grows: reserve(1), two calls, reserve(40), two more — the oracle's sequence.
    At 1920x1080 the same frame size runs under two chunkings (127 chunk histograms with 1 stream reserved, 8 with 40)."""
    c = Context(options=SCHEDULES[sched])
    try:
        c.set_geometry(seq.w, seq.h, 1)
        c.camshift_reserve(1)
        c.upload(seq.frames[0][None])
        c.camshift_init([seq.rect])
        stats = []
        for k, (sw, to) in enumerate(_expected(seq), 1):
            if k == 3:
                c.camshift_reserve(40)
            c.upload(seq.frames[k][None])
            check(c.camshift_track(1, calc_angles=True)[0], sw, to, stats, where=(seq.name, sched, k), tally=_tally(sched))
        assert len(stats) == 4
        assert_all_exact(stats, f"{seq.name}, {sched}")
    finally:
        c.close()


# ---- B: the LDS region cache ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq", cc.region_sequences(), ids=lambda s: s.name)
def test_region_cache_sequences(ctx, seq):
    """jumping targets (moment passes from LDS first, from memory once the window has left the region), margins clamped by borders and
    corners, every column phase of the stash path, frame widths on both sides of the two cache fills, windows between and above the
    two capacities: all == the oracle, on every schedule"""
    sched, c = ctx
    stats = []
    _track_single(c, sched, seq, stats)
    assert len(stats) == seq.ncalls
    assert_all_exact(stats, f"{seq.name}, {sched}")


def _sweep(sched, jobs):
    """jobs: [(sequence, cs_region value)]; one context per value; returns {sequence name: {value: raw track objects}}"""
    raws = {}
    for v in sorted({v for _s, v in jobs}):
        c = Context(options=SCHEDULES[sched] + f",cs_region={v}")
        try:
            for s, sv in jobs:
                if sv == v:
                    stats = []
                    raws.setdefault(s.name, {})[v] = _track_single(c, sched, s, stats, tag=f" cs_region={v}")
                    assert_all_exact(stats, f"{s.name}, {sched}, cs_region={v}")
        finally:
            c.close()
    return raws


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_region_capacity_sweep(sched):
    """option cs_region on the capacity boundary of the first window (A - 1: no region, A and A + 1: margin 0), on the exact pixel
    counts that admit margins 1, 3, 8, 15 and 16, off, and at the two built-in capacities: every value == the oracle, and all values
    return the same bytes (cached and uncached passes instantiate one reduction)"""
    seqs = cc.jumping() + cc.static()
    raws = _sweep(sched, [(s, v) for s in seqs for v in cc.region_sweep_values(s.w, s.h, s.rect)])
    for s in seqs:
        assert len(raws[s.name]) == 11
        differ = [v for v, raw in raws[s.name].items() if raw != raws[s.name][0]]
        assert not differ, (s.name, sched, differ)


@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_region_with_zero_margin_reads_its_outermost_columns(sched):
    """capacity == area of the first window: the first call's region is the window itself, so its passes read the cache's first and
    last column and row — the partial 16-byte groups of the stash path at all sixteen column phases, the last lane of the copy pass;
    compared with the oracle and with the bytes of the same sequence without a cache"""
    jobs = cc.zero_margin()
    raws = _sweep(sched, jobs + [(s, 0) for s, _v in jobs])
    for s, v in jobs:  # and bit for bit what the uncached passes return: a wrong bin in a background column moves the sums by very little
        assert raws[s.name][v] == raws[s.name][0], (s.name, sched, v)


# ---- C: initTracker kernels -------------------------------------------------------------------------------------------------------------------

INIT_RESERVED = 80


def _init_and_compare(c, batch, first):
    _name, _kernel, rects = batch
    n = len(rects)
    frames = np.stack([cc.init_frame(slot) for slot in range(n)])
    c.set_geometry(cc.INIT_W, cc.INIT_H, 64)
    c.camshift_reserve(INIT_RESERVED)
    behind = c.camshift_debug_hist(first + n, current=False)[0].copy()
    c.upload(frames)
    c.camshift_init(rects, first=first)
    for s, rect in enumerate(rects):
        model = c.camshift_debug_hist(first + s, current=False)[0].astype(np.int64)
        want = cc.model_histogram(frames[s], rect)
        assert int(model.sum()) == rect[2] * rect[3], (s, rect, int(model.sum()))
        assert np.array_equal(model, want), (s, rect, np.flatnonzero(model != want)[:8])
    assert np.array_equal(c.camshift_debug_hist(first + n, current=False)[0], behind)


@pytest.mark.parametrize("first", [0, 7])
@pytest.mark.parametrize("batch", [b for b in cc.init_batches() if len(b[2]) > 1], ids=lambda b: b[0])
def test_init_kernels_model_histograms(plain_ctx, batch, first):
    """model histograms of a batch bin for bin vs the oracle's initTracker, sum == width * height, for batches that dispatch the
    one-workgroup-per-stream kernel and the row-split kernel, into streams [first, first + n); the stream behind the range keeps its model"""
    _init_and_compare(plain_ctx, batch, first)


@pytest.mark.parametrize("batch", [b for b in cc.init_batches() if len(b[2]) == 1], ids=lambda b: b[0])
def test_init_kernels_rect_sizes(plain_ctx, batch):
    """one stream, rect widths next to 64 / 128 columns and heights next to 16 / 128 / 256 rows"""
    w, h = batch[2][0][2:]
    _init_and_compare(plain_ctx, batch, (w + h) % 9)


# ---- D: chunk-histogram edges -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", ["chunked", "fused"])
def test_chunk_histogram_edges(sched):
    """full-frame histogram of every stream vs np.bincount at pixel counts on and next to the chunking quanta (4096-px chunk granule,
    one chunk per 16 384 px), 1 or 3 streams tracked out of 1 / 32 / 40 reserved, distinct frames per slot (with an odd pixel count
    slots 1 and 2 start 4- but not 16-byte aligned); noise, flat and run-length frames"""
    c = Context(options=SCHEDULES[sched] + ",cs_keep_hist=1")
    try:
        for n, reserved in cc.HIST_TRACKED_RESERVED:
            c.camshift_reserve(reserved)
            for w, h in cc.HIST_SIZES:
                c.set_geometry(w, h, 3)
                for family in cc.HIST_FAMILIES:
                    frames = np.stack([cc.hist_frame(family, w, h, slot) for slot in range(n)])
                    c.upload(frames)
                    c.camshift_init([(1, 1, 8, 8)] * n)
                    c.camshift_track(n, calc_angles=True)
                    for s in range(n):
                        cur = c.camshift_debug_hist(s)[1].astype(np.int64)
                        want = cc.frame_histogram(frames[s])
                        assert int(cur.sum()) == w * h, (w, h, family, n, reserved, s, int(cur.sum()))
                        assert np.array_equal(cur, want), (w, h, family, n, reserved, s, np.flatnonzero(cur != want)[:8])
    finally:
        c.close()


# ---- E: the default decision table ----------------------------------------------------------------------------------------------------------

CS_TIMERS = ("cs_track", "cs_track_512", "cs_hist", "cs_lut", "cs_meanshift", "cs_fused_launches_1024", "cs_fused_launches_512")
# (streams, W, H, the case on the other side of the threshold this one guards): 10 240 / 9 216 pixels around cs_cluster_min_px, 64 / 65
# streams around the cluster form's stream limit (and, with 256 CUs, its 4 workgroups per stream), 191 / 192 around cs_fused_min, 192 / 257
# around one workgroup per CU
DEFAULT_CASES = {"n1-128x80": (1, 128, 80, "n1-96x96"), "n1-96x96": (1, 96, 96, "n1-128x80"), "n64-128x80": (64, 128, 80, "n65-128x80"),
                 "n65-128x80": (65, 128, 80, "n64-128x80"), "n191-64x64": (191, 64, 64, "n192-64x64"), "n192-64x64": (192, 64, 64, "n191-64x64"),
                 "n257-64x64": (257, 64, 64, "n192-64x64")}
ON_256_CUS = {"n1-128x80": "CLUSTER", "n1-96x96": "PER_STREAM", "n64-128x80": "CLUSTER", "n65-128x80": "PER_STREAM", "n191-64x64": "PER_STREAM",
              "n192-64x64": "FUSED_1024", "n257-64x64": "FUSED_512"}


def _default_plan(name, cus):
    n, w, h, _other = DEFAULT_CASES[name]
    return cs_schedule.track_plan(n, w, h, num_cus=cus)


def _expected_timers(plan, calls):
    want = {t: calls for t in plan["timers"]}
    if plan["form"].startswith("FUSED"):
        want["cs_fused_launches_" + plan["form"][6:]] = calls
    return want


def _default_batches(w, h, n, steps):
    seqs = cc.default_path_streams(w, h)
    per = [seqs[s % len(seqs)] for s in range(n)]
    return per, [np.stack([q.frames[k] for q in per]) for k in range(steps + 1)]


def test_default_table_on_256_compute_units():
    """the table the cases below are computed from, at the CU count of the device this library is written for (no device needed)"""
    assert {name: _default_plan(name, 256)["form"] for name in DEFAULT_CASES} == ON_256_CUS


@pytest.mark.parametrize("name", list(DEFAULT_CASES))
def test_default_options_take_the_schedule_of_the_table(name):
    """default options, profiling on: one init + two track() calls, every track object against the oracle, then the timers the two calls
    left behind say which kernels ran: the form the decision table gives for this device's CU count, and nothing of another form.  The
    process's other contexts are idle, so no other context is busy on the fused path."""
    n, w, h, other = DEFAULT_CASES[name]
    cus = multiprocessor_count()
    plan = _default_plan(name, cus)
    if plan["form"] == _default_plan(other, cus)["form"]:
        pytest.skip(f"with {cus} compute units {name} and {other} take the same schedule ({plan['form']}): no threshold between them")
    per, batches = _default_batches(w, h, n, 2)
    c = Context()
    try:
        c.profile(True)
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.upload(batches[0])
        c.camshift_init([q.rect for q in per])
        c.synchronize()
        c.kernel_times(reset=True)
        stats = []
        for k in (1, 2):
            c.upload(batches[k])
            got = c.camshift_track(n, calc_angles=True)
            for s, q in enumerate(per):
                sw, to = _expected(q)[k - 1]
                check(got[s], sw, to, stats, where=(name, "default", s, k), tally=_tally("default"))
        assert len(stats) == 2 * n
        c.synchronize()
        times = c.kernel_times()
        got_timers = {t: times[t]["launches"] for t in CS_TIMERS if t in times}
        assert got_timers == _expected_timers(plan, 2), (name, cus, plan["form"], got_timers)
    finally:
        c.close()


@pytest.mark.parametrize("fetch", ["all", "last"])
def test_fused_track_sequence_equals_single_calls(fetch):
    """ht_camshift_track_sequence on the fused path with default options (192 streams, 3 calls in ONE launch whose workgroups walk their
    stream's calls) returns the bytes of three single track() calls from the same initial state, for every call's objects and for the
    last call's only; the single calls are checked against the oracle"""
    n, w, h, steps = 192, 64, 64, 3
    form = cs_schedule.track_plan(n, w, h, num_cus=multiprocessor_count())["form"]
    per, batches = _default_batches(w, h, n, steps)
    dev = [DeviceArray(b) for b in batches]
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        rects = [q.rect for q in per]
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)
        single, stats = [], []
        for k in range(1, steps + 1):
            c.bind_device(dev[k].ptr, n)
            got = c.camshift_track(n, calc_angles=True)
            for s, q in enumerate(per):
                sw, to = _expected(q)[k - 1]
                check(got[s], sw, to, stats, where=("sequence-default", s, k), tally=_tally("default"))
            single.append(got.tobytes())
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)  # the same initial state again
        c.kernel_times(reset=True)
        got = c.camshift_track_sequence([d.ptr for d in dev[1:]], n, calc_angles=True, fetch=fetch)
        assert got.tobytes() == (b"".join(single) if fetch == "all" else single[-1])
        times = c.kernel_times()
        assert times["cs_fused_launches_" + form[6:]]["launches"] == 1 and form.startswith("FUSED"), (form, times)
    finally:
        c.synchronize()
        c.close()
        for d in dev:
            d.free()

"""A tracker per grouped face on the device (ht_camshift_init_faces / _result, ht_cs_faces.hip) against the rule restated in Python
(tests/init_faces_cases.py, on the CPU oracle's grouped lists) and against the host route it replaces: collect, ht_detect_grouped, the
rule on the host, ht_camshift_init_pairs.  Records are demanded equal, models and the following track steps byte for byte (both routes
launch the same init kernels on the same rects).  No tolerance anywhere: the rule is integer and binary64 comparisons.

The search windows the association reads are known on the host without a read-back of their own: zeros since ht_camshift_reserve, the
rect after an initTracker (camshift.js:209), sw_* of the last track result after a track step."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import frame_layouts as fl
import init_faces_cases as fc
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray

pytestmark = pytest.mark.gpu

NODE = shutil.which("node")
LAYOUT = "lead12_rowpad"
N, S = fc.NFRAMES, 24


class Bound:
    """the batch on the device at LAYOUT: the pointer and stride a host would bind"""

    def __init__(self, frames, salt):
        self.lead, self.stride = fl.layout(LAYOUT, fc.W, fc.H)
        self.dev = DeviceArray(fl.lay_out(frames, self.lead, self.stride, fl.layout_seed(LAYOUT, fc.W, fc.H, salt)))

    def bind(self, c, n=N):
        c.bind_device(self.dev.ptr + self.lead, n, self.stride)


@pytest.fixture(scope="module")
def bound():
    b = Bound(fc.frames(), 3)
    yield b
    b.dev.free()


@pytest.fixture(scope="module")
def lists(cascade):
    return fc.lists_of(cascade.blob)


def make_ctx(bound, options=None, streams=S):
    c = Context(options=options)
    c.set_geometry(fc.W, fc.H, N)
    c.camshift_reserve(streams)
    bound.bind(c)
    return c


def group(c):
    c.detect_enqueue(0)
    c.detect_best_enqueue(1)


def records(c, n):
    return [(int(r["code"]), int(r["face"]), (int(r["x"]), int(r["y"]), int(r["width"]), int(r["height"])), int(r["dropped"])) for r in c.camshift_init_faces_result(n)]


def models(c, streams=S):
    return np.stack([c.camshift_debug_hist(s, current=False)[0] for s in range(streams)])


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, got, want)


class Pair:
    """the context under test and its twin, which takes the host route; the search window of every stream, followed on the host"""

    def __init__(self, bound, options=None, streams=S):
        self.c, self.twin = make_ctx(bound, options, streams), make_ctx(bound, None, streams)
        self.win = {s: fc.ZERO for s in range(streams)}
        self.streams = streams

    def close(self):
        self.c.close()
        self.twin.close()

    def init(self, pairs, rects):
        for x in (self.c, self.twin):
            x.camshift_init_pairs(pairs, rects)
        for (s, _f), r in zip(pairs, rects):
            self.win[s] = tuple(r)

    def track(self, pairs, steps, what):
        """`steps` track steps of both contexts, equal in every bit; the windows they leave"""
        for k in range(steps):
            got, want = self.c.camshift_track_pairs(pairs), self.twin.camshift_track_pairs(pairs)
            assert_same(got, want, (what, "track step", k))
        for (s, _f), t in zip(pairs, got):
            self.win[s] = tuple(int(t[k]) for k in ("sw_x", "sw_y", "sw_width", "sw_height"))

    def host_route(self, pairs, recs):
        """what a host does today with the records' rects: initTracker of the slots that got a face"""
        sel = [i for i, r in enumerate(recs) if r[0] == fc.FACE]
        if sel:
            self.twin.camshift_init_pairs([pairs[i] for i in sel], [recs[i][2] for i in sel])
        for i in sel:
            self.win[pairs[i][0]] = recs[i][2]
        return sel

    def windows(self, pairs):
        return [self.win[s] for s, _f in pairs]

    def same_models(self, what):
        assert_same(models(self.c, self.streams), models(self.twin, self.streams), what)


def pair_list(k):
    """shuffled streams; the slots of different frames interleaved"""
    order = [(7 * i + 3) % S for i in range(S)]  # every stream once
    if k == 1:
        frames = list(range(N))
    elif k == 3:
        frames = [f for _round in range(3) for f in (fc.FRAME_B, 0, fc.TILED, 1, 4, fc.FRAME_A, 2, 3)]
    else:  # sixteen slots on the tiled frame, four each on two_faces and B, dealt in turn
        frames = [fc.TILED, fc.TWO_FACES, fc.TILED, fc.FRAME_B, fc.TILED, fc.TILED] * 4
        assert frames.count(fc.TILED) == 16
    return [(order[i], f) for i, f in enumerate(frames)]


@pytest.mark.parametrize("k", [1, 3, 16])
def test_records_models_and_track_steps_against_restatement_and_host_route(bound, lists, k):
    """both thresholds, associate 0 and 1: records equal the restatement; the models of the slots with a face are the host route's bits,
    every other stream keeps every byte; the next three track steps are equal in every bit.  Each call starts from the windows the one
    before left: never initialised, an initTracker's rect, a track step's window."""
    pairs = pair_list(k)
    n = len(pairs)
    p = Pair(bound)
    try:
        # two of three streams start on a rect of their own; the others have never been initialised: not live
        pre = [(s, f) for s, f in pairs if s % 3]
        p.init(pre, [(5 + 11 * s, 8 + 7 * s, 40 + 2 * s, 30 + s) for s, _f in pre])
        seen = set()
        for threshold, associate in ((5.0, True), (-10.0, False), (-10.0, True), (5.0, False)):
            group(p.c)
            want = fc.resolve(lists, pairs, p.windows(pairs), threshold, associate)
            p.c.camshift_init_faces(pairs, threshold, associate)
            got = records(p.c, n)                   # before the collect
            assert got == records(p.c, n)           # may be called repeatedly
            assert got == want, (k, threshold, associate, got, want)
            p.c.detect_best_collect()
            sel = p.host_route(pairs, got)
            p.same_models((k, threshold, associate, "models"))
            seen |= {r[0] for r in got}
            live = [pairs[i] for i in range(n) if p.win[pairs[i][0]][2] > 0 and p.win[pairs[i][0]][3] > 0]
            p.track(live, 3, (k, threshold, associate))
            assert sel
        assert seen == {fc.FACE, fc.UNTOUCHED}
        if k == 3:
            assert got[pairs.index((pairs[2][0], fc.TILED))][3] == sum(f[4] > 5.0 for f in lists[fc.TILED]) - 3 > 0  # dropped
    finally:
        p.close()


@pytest.mark.parametrize("scenario", sorted(fc.SCENARIOS))
def test_a_tracker_keeps_its_slot_across_a_redetection(bound, lists, scenario):
    """initTracker on frame A's faces in the scenario's slot order, two track steps, detection on the batch, init_faces(associate) on frame
    B: the slot -> face map is the restatement's on the device's own windows and not the rank order; without associate it is the rank
    order.  A stream never initialised is not live: it takes the first face no tracker matched."""
    slots = fc.SCENARIOS[scenario]
    k = len(slots)
    p = Pair(bound, streams=4)
    try:
        on_a = [(j, fc.FRAME_A) for j, s in enumerate(slots) if s is not None]
        p.init(on_a, [fc.floor_rect(lists[fc.FRAME_A][s[1]]) for s in slots if s is not None])
        p.track(on_a, 2, scenario)
        on_b = [(j, fc.FRAME_B) for j in range(k)]
        wins = p.windows(on_b)
        assert [w == fc.ZERO for w in wins] == [s is None for s in slots]
        group(p.c)
        p.c.camshift_init_faces(on_b, -10.0, associate=True)
        got = records(p.c, k)
        assert got == fc.resolve(lists, on_b, wins, -10.0, True)
        B = lists[fc.FRAME_B]
        rank = sorted(range(len(B)), key=lambda i: (-B[i][4], i))
        assert [r[1] for r in got] != rank[:k] and sorted(r[1] for r in got) == sorted(rank[:k])
        if scenario == "permuted":  # every tracker is on the face it was on: the nearest one
            for j, s in enumerate(slots):
                a = lists[fc.FRAME_A][s[1]]
                assert got[j][1] == min(range(4), key=lambda i: abs(B[i][0] - a[0]) + abs(B[i][1] - a[1]))
        else:
            assert got[2][1] == [i for i in rank[:k] if i != got[0][1]][0]  # the never-initialised slot, not live slot 1, takes the first face left
        p.host_route(on_b, got)
        p.same_models((scenario, "associate"))
        p.c.camshift_init_faces(on_b, -10.0, associate=False)
        got = records(p.c, k)
        assert [r[1] for r in got] == rank[:k] and got == fc.resolve(lists, on_b, p.windows(on_b), -10.0, False)
        p.c.detect_best_collect()
        p.host_route(on_b, got)
        p.same_models((scenario, "rank order"))
        p.track(on_b, 1, scenario)
    finally:
        p.close()


def test_a_list_longer_than_a_wavefront(bound, cascade):
    """min_neighbors 0: the tiled frame's list is its 129 raw detections — the selection's lanes stride over more than one face each, and
    equal confidences are ranked by list index"""
    lists0 = fc.lists_of(cascade.blob, 0)
    assert len(lists0[fc.TILED]) == 129 and len({f[4] for f in lists0[fc.TILED]}) < 129
    pairs = pair_list(16)
    p = Pair(bound)
    try:
        for threshold, associate in ((-10.0, False), (5.0, True)):
            p.c.detect_enqueue(0)
            p.c.detect_best_enqueue(0)
            want = fc.resolve(lists0, pairs, p.windows(pairs), threshold, associate)
            p.c.camshift_init_faces(pairs, threshold, associate)
            got = records(p.c, len(pairs))
            assert got == want, (threshold, associate, got, want)
            assert max(r[1] for r in got) >= 64 and got[0][3] == sum(f[4] > threshold for f in lists0[fc.TILED]) - min(16, sum(f[4] > threshold for f in lists0[fc.TILED]))
            p.c.detect_best_collect()
            assert [fc.face_tuple(x) for x in p.c.detect_grouped(fc.TILED)] == lists0[fc.TILED]
            p.host_route(pairs, got)
            p.same_models((threshold, associate))
    finally:
        p.close()


def test_untouched_slots_keep_every_byte(bound, lists):
    pairs = pair_list(3)
    p = Pair(bound)
    try:
        p.init(pairs, [(5 + 11 * s, 8 + 7 * s, 40 + 2 * s, 30 + s) for s, _f in pairs])
        p.track(pairs, 1, "before")
        before = models(p.c)
        group(p.c)
        p.c.camshift_init_faces(pairs, 1e9, associate=True)  # above every face
        got = records(p.c, len(pairs))
        assert got == [(fc.UNTOUCHED, -1, fc.ZERO, 0)] * len(pairs)
        p.c.detect_best_collect()
        assert_same(models(p.c), before, "models")
        p.track(pairs, 2, "untouched: window and track object")  # the twin was never called
    finally:
        p.close()


def test_deferred_under_the_lowest_cap_then_resolved_after_the_collect(bound, lists):
    """group_cap=64: the tiled frame (129 raw hits) is not final while the batch is in flight — its slots are deferred and keep every byte;
    after the collect the same pairs resolve to the restatement (the collect completes the frame's list on the device)"""
    pairs = [(4, fc.TILED), (0, fc.TWO_FACES), (2, fc.TILED), (1, fc.TWO_FACES), (3, fc.TILED)]
    p = Pair(bound, "group_cap=64", streams=6)
    try:
        p.init(pairs[:4], [(5 + 11 * s, 8 + 7 * s, 40 + 2 * s, 30 + s) for s, _f in pairs[:4]])
        before = models(p.c, 6)
        group(p.c)
        p.c.camshift_init_faces(pairs, -10.0, associate=True)
        got = records(p.c, 5)
        want = fc.resolve(lists, pairs, p.windows(pairs), -10.0, True, deferred_frames=(fc.TILED,))
        assert got == want and [r[0] for r in got] == [fc.DEFERRED, fc.FACE, fc.DEFERRED, fc.FACE, fc.DEFERRED]
        for s in (4, 2, 3):
            assert_same(models(p.c, 6)[s], before[s], ("deferred stream", s))
        p.host_route(pairs, got)
        p.same_models("deferred: models")
        # search window and track object of the deferred, previously initialised streams too: a track step against the twin, which the call
        # never reached, while the batch is still in flight (stream 3 was never initialised: nothing to track)
        p.track([pr for pr in pairs if pr[0] != 3], 1, "deferred: window and track object")
        p.c.detect_best_collect()
        g = p.c.detect_grouped(fc.TILED)
        assert [fc.face_tuple(x) for x in g] == lists[fc.TILED]
        tiled = [pr for pr in pairs if pr[1] == fc.TILED]
        p.c.camshift_init_faces(tiled, -10.0, associate=True)
        got = records(p.c, 3)
        assert got == fc.resolve(lists, tiled, p.windows(tiled), -10.0, True) and [r[0] for r in got] == [fc.FACE] * 3 and got[0][3] == 12
        p.host_route(tiled, got)
        p.same_models("after the collect: models")
        p.track(pairs, 1, "after the collect")
    finally:
        p.close()


def test_before_and_after_the_collect_give_the_same(bound, lists):
    pairs = pair_list(3)
    a, b = make_ctx(bound), make_ctx(bound)
    try:
        group(a)
        a.camshift_init_faces(pairs, -10.0, associate=True)   # between ht_detect_best_enqueue and the collect
        a.detect_best_collect()
        group(b)
        b.detect_best_collect()
        for f in range(N):  # the lists both read are the oracle's
            assert [fc.face_tuple(x) for x in b.detect_grouped(f)] == lists[f], f
        b.camshift_init_faces(pairs, -10.0, associate=True)   # after it
        ra, rb = records(a, len(pairs)), records(b, len(pairs))
        assert ra == rb == fc.resolve(lists, pairs, [fc.ZERO] * len(pairs), -10.0, True)
        assert_same(models(a), models(b), "models")
    finally:
        a.close()
        b.close()


def test_row_form_gives_the_same_bits(bound, lists):
    """cs_pairs_cluster=1: < 64 pairs take k_csp_zero_models + k_csp_init_rows, planned for the frame height"""
    pairs = pair_list(16)
    c, r = make_ctx(bound), make_ctx(bound, "cs_pairs_cluster=1")
    try:
        outs = []
        for x in (c, r):
            x.profile(True)
            x.kernel_times(reset=True)
            group(x)
            x.camshift_init_faces(pairs, 5.0, associate=False)
            outs.append((records(x, len(pairs)), models(x), x.kernel_times(reset=True)))
            x.profile(False)
            x.detect_best_collect()
        (rec_c, m_c, t_c), (rec_r, m_r, t_r) = outs
        assert rec_c == rec_r == fc.resolve(lists, pairs, [fc.ZERO] * len(pairs), 5.0, False)
        assert {fc.FACE, fc.UNTOUCHED} == {x[0] for x in rec_c}
        assert_same(m_r, m_c, "row form against the one-workgroup form")
        assert t_r["csp_init_rows"]["launches"] >= 1 and "csp_init" not in t_r and t_r["csf_resolve"]["launches"] == 1
        assert t_c["csp_init"]["launches"] >= 1 and "csp_init_rows" not in t_c and t_c["csf_resolve"]["launches"] == 1
    finally:
        c.close()
        r.close()


def _refused(fn, status, *needles):
    with pytest.raises(HtError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))
    for needle in needles:
        assert needle in str(e.value), (needle, str(e.value))


def test_refusals_change_nothing(bound, lists):
    pairs = pair_list(3)
    p = Pair(bound)
    try:
        c = p.c
        p.init(pairs, [(5 + 11 * s, 8 + 7 * s, 40 + 2 * s, 30 + s) for s, _f in pairs])
        before = models(c)
        ok = pairs[1:4]  # on frames 0, the tiled one and 1
        _refused(lambda: c.camshift_init_faces(ok), native.HT_ERR_STATE, "no device-grouped batch")
        _refused(lambda: c.camshift_init_faces_result(3), native.HT_ERR_STATE)
        bound.bind(c, N - 1)  # a grouped batch of seven frames ...
        group(c)
        bound.bind(c, N)      # ... and eight bound frames: frame 7 is bound, and outside the batch
        bad = [
            ([(s, fc.TILED) for s in range(17)], ("frame %d" % fc.TILED, "16 slots")),   # 17 slots on one frame
            ([(0, 0), (1, N - 1)], ("pair 1", "frame %d" % (N - 1), "outside")),          # a frame outside the batch
            # the rules of ht_camshift_init_pairs, in csp_plan's words: they name the stream or the frame
            ([(0, 0), (1, 1), (0, 2)], ("stream 0", "twice")),                            # a duplicate stream
            ([(0, 0), (S, 0)], ("stream %d" % S, "not reserved")), ([(0, N)], ("frame %d" % N, "not bound")),
            ([], ()), ([(s % S, 0) for s in range(S + 1)], ()),
        ]
        for prs, needles in bad:
            _refused(lambda: c.camshift_init_faces(prs, -10.0, True), native.HT_ERR_INVALID, *needles)
        _refused(lambda: c.camshift_init_faces(ok, float("nan")), native.HT_ERR_INVALID, "NaN")
        L = native.lib()
        pa = Context._pairs(ok)
        for flags in (2, 3, 0x80000000):  # unknown flag bits
            assert L.ht_camshift_init_faces(c._h, pa.ctypes.data, 3, -10.0, flags) == native.HT_ERR_INVALID
        _refused(lambda: c.camshift_init_faces_result(3), native.HT_ERR_STATE)   # still no accepted call
        assert_same(models(c), before, "after the refusals")
        p.track(pairs, 1, "after the refusals")  # windows and track objects too: the twin saw none of this
        before = models(c)
        c.camshift_init_faces(ok, 1e9)           # accepted: every slot untouched
        assert [r[0] for r in records(c, 3)] == [fc.UNTOUCHED] * 3
        _refused(lambda: c.camshift_init_faces_result(2), native.HT_ERR_STATE)   # n differs
        assert [r[0] for r in records(c, 3)] == [fc.UNTOUCHED] * 3               # ... and the result is still there
        c.camshift_reserve(S + 4)
        _refused(lambda: c.camshift_init_faces_result(3), native.HT_ERR_STATE)   # the trackers have been replaced
        assert_same(models(c), before, "after the reservation grew")
        c.detect_best_collect()
    finally:
        p.close()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_device_batch_route_from_node(tmp_path, cascade):
    """tests/js/init_faces_gpu.js on the product addon: ccv.DeviceBatch.initFaces / initFacesResult against the Python expectations of a
    rank-order call and an associate call, a track step enqueued behind each; then the raw addon calls and their refusals"""
    from conftest import ROOT
    from headtrackr_amd import build

    build.build_all()
    job = fc.js_job(tmp_path, cascade.blob)
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "init_faces_gpu.js"), str(jf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] == 13 and out["refusals"] == 6

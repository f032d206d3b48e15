"""initTracker from the device's best-face records (ht_camshift_init_best / ht_camshift_init_best_result, ht_cs_best.hip) against the
host hand-off it replaces: detect_best_collect, Math.floor on the host, ht_camshift_init_pairs.  Everything compared with the host
hand-off is demanded byte for byte (both routes launch the same kernels on the same rects); models are also compared bin for bin with
the CPU oracle's initTracker, track objects with the oracle within the project's tolerance and counted exact.

The frames are bound at one layout of tests/frame_layouts.py (base + 12, padded stride): the record-driven init reads them through the
same addressing as every other frame-reading kernel."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import frame_layouts as fl
import init_best_cases as ib
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_camshift import assert_all_exact, check

pytestmark = pytest.mark.gpu

NODE = shutil.which("node")

LAYOUT = "lead12_rowpad"
N, S, PAIRS = ib.NFRAMES, ib.STREAMS, ib.PAIRS
# where every stream stands before the call under test: rects that are no frame's best face
PRE = [(10 + 7 * s, 20 + 5 * s, 40 + 3 * s, 30 + 2 * s) for s, _f in PAIRS]
# per pair; pair 1 meets the noise frame (always a fallback): its rect hangs over the canvas' left and bottom edges
FALLBACK = [ib.centre_half() if i != 1 else (-5, 200, 60, 60) for i in range(len(PAIRS))]


class Bound:
    """a batch on the device at LAYOUT: the pointer and stride a host would bind"""

    def __init__(self, frames, salt):
        self.lead, self.stride = fl.layout(LAYOUT, ib.W, ib.H)
        assert self.lead == 12 and self.stride > fl.fb_of(ib.W, ib.H)
        self.dev = DeviceArray(fl.lay_out(frames, self.lead, self.stride, fl.layout_seed(LAYOUT, ib.W, ib.H, salt)))

    def bind(self, c, n=N):
        c.bind_device(self.dev.ptr + self.lead, n, self.stride)


@pytest.fixture(scope="module")
def moved():
    """the frames of the track calls: the batch moved by 3 rows and 5 columns"""
    f = np.ascontiguousarray(np.roll(ib.frames(), (3, 5), axis=(1, 2)))
    f.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def bound(moved):
    b = (Bound(ib.frames(), 1), Bound(moved, 2))
    yield b
    for x in b:
        x.dev.free()


def make_ctx(bound, options=None):
    c = Context(options=options)
    c.set_geometry(ib.W, ib.H, N)
    c.camshift_reserve(S)
    bound[0].bind(c)
    return c


@pytest.fixture(scope="module")
def ctxs(bound):
    """the context under test and its twin, which takes the host hand-off"""
    c, twin = make_ctx(bound), make_ctx(bound)
    yield c, twin
    c.close()
    twin.close()


def pre_init(c, bound):
    bound[0].bind(c)
    c.camshift_init_pairs(PAIRS, PRE)


def group(c):
    c.detect_enqueue(0)
    c.detect_best_enqueue(1)


def models(c):
    return np.stack([c.camshift_debug_hist(s, current=False)[0] for s in range(S)])


def host_handoff(twin, codes, rects):
    """what the host does today: initTracker of the pairs that were decided face or fallback, with the host's rects"""
    sel = [i for i, code in enumerate(codes) if code in (ib.FACE, ib.FALLBACK)]
    if sel:
        twin.camshift_init_pairs([PAIRS[i] for i in sel], [rects[i] for i in sel])
    return sel


def result(c, n=len(PAIRS)):
    codes, rects = c.camshift_init_best_result(n)
    return [int(v) for v in codes], [tuple(int(r[k]) for k in ("x", "y", "width", "height")) for r in rects]


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (what, got, want)


@pytest.mark.parametrize("with_fallback", [False, True], ids=["no_fallback", "fallback"])
@pytest.mark.parametrize("threshold", ib.THRESHOLDS)
def test_both_thresholds_with_and_without_fallback(ctxs, bound, moved, cascade, threshold, with_fallback):
    """codes, rects, models and the following track step equal the host hand-off's; streams that are not initialised keep every byte"""
    c, twin = ctxs
    fb = FALLBACK if with_fallback else None
    pre_init(c, bound)
    pre_init(twin, bound)
    group(c)
    c.camshift_init_best(PAIRS, threshold, fb)
    codes, rects = result(c)                      # before the collect
    assert (codes, rects) == result(c)            # may be called repeatedly
    best, _total = c.detect_best_collect()
    assert best.tobytes() == ib.best(cascade.blob).tobytes(), ("best faces", best)
    # the host's floor of the collected faces, and the oracle's
    want = [ib.decide(best[f], threshold, None if fb is None else fb[i]) for i, (_s, f) in enumerate(PAIRS)]
    assert codes == [w[0] for w in want] and rects == [w[1] for w in want], (codes, rects, want)
    assert (codes, rects) == ib.expected(cascade.blob, PAIRS, threshold, fb)
    assert codes[PAIRS.index((2, ib.TILED))] == ib.FACE  # 129 raw hits are below the default cap: final at once
    assert ib.FACE in codes and (ib.FALLBACK if with_fallback else ib.UNTOUCHED) in codes
    sel = host_handoff(twin, codes, rects)
    m, mt = models(c), models(twin)
    assert_same(m, mt, "models against the host hand-off")
    oracles = {}
    for i in sel:  # bin for bin the oracle's initTracker on the floored rect
        s, f = PAIRS[i]
        oracles[i] = ho.cs_init(ib.frames()[f], *rects[i])
        assert np.array_equal(m[s], np.frombuffer(oracles[i].s.model, dtype=np.int32).astype(np.uint32)), (i, s, f, rects[i])
    for b, x in ((bound[1], c), (bound[1], twin)):
        b.bind(x)
    got, got_twin = c.camshift_track_pairs(PAIRS), twin.camshift_track_pairs(PAIRS)
    assert_same(got, got_twin, "track step against the host hand-off")  # the untouched streams' search windows and models included
    stats = []
    for i in sel:
        sw, to = oracles[i].track(moved[PAIRS[i][1]])
        if PAIRS[i][1] == ib.TILED and codes[i] == ib.FACE:
            # the window on the tiled frame's face comes out square (width == height): the orientation of an isotropic distribution is
            # atan2 of rounding noise, not a quantity to compare with the oracle.  Every integer-valued output is demanded exactly.
            assert float(got[i]["width"]) == float(got[i]["height"]) == to["width"] == to["height"]
            assert [int(got[i][k]) for k in ("sw_x", "sw_y", "sw_width", "sw_height")] == [int(v) for v in sw]
            assert (float(got[i]["x"]), float(got[i]["y"])) == (to["x"], to["y"])
            continue
        check(got[i], sw, to, stats, where=("init_best", threshold, with_fallback, i))
    assert_all_exact(stats, "init_best")


def test_deferred_frame_under_the_lowest_cap(bound, cascade):
    """group_cap=64: the tiled frame's record is not final before the collect — its pair is deferred and its stream keeps every byte; after
    the collect the same call initialises it with the oracle's rect"""
    c, twin = make_ctx(bound, "group_cap=64"), make_ctx(bound)
    try:
        pre_init(c, bound)
        pre_init(twin, bound)
        group(c)
        c.camshift_init_best(PAIRS, -10.0, None)
        codes, rects = result(c)
        i_t = PAIRS.index((2, ib.TILED))
        want = ib.expected(cascade.blob, PAIRS, -10.0, None, deferred_frames=(ib.TILED,))
        assert (codes, rects) == want and codes[i_t] == ib.DEFERRED and codes.count(ib.DEFERRED) == 1
        host_handoff(twin, codes, rects)
        assert_same(models(c), models(twin), "deferred: models")  # the deferred stream still has its PRE model
        bound[1].bind(c), bound[1].bind(twin)
        assert_same(c.camshift_track_pairs(PAIRS), twin.camshift_track_pairs(PAIRS), "deferred: track step")
        bound[0].bind(c), bound[0].bind(twin)
        best, _total = c.detect_best_collect()
        assert best.tobytes() == ib.best(cascade.blob).tobytes(), ("best faces", best)
        c.camshift_init_best([PAIRS[i_t]], -10.0, None)  # the deferred pair only: its record is complete now
        codes2, rects2 = result(c, 1)
        assert codes2 == [ib.FACE] and rects2 == [ib.floor_rect(ib.best(cascade.blob)[ib.TILED])]
        twin.camshift_init_pairs([PAIRS[i_t]], rects2)
        assert_same(models(c), models(twin), "after the collect: models")
    finally:
        c.close()
        twin.close()


def test_row_form_gives_the_same_models(ctxs, bound, cascade):
    """cs_pairs_cluster=1: < 64 pairs take k_csp_zero_models + k_csp_init_rows, planned for the frame height; same bits"""
    c, _twin = ctxs
    r = make_ctx(bound, "cs_pairs_cluster=1")
    try:
        outs = []
        for x in (c, r):
            pre_init(x, bound)
            x.profile(True)
            x.kernel_times(reset=True)
            group(x)
            x.camshift_init_best(PAIRS, 5.0, FALLBACK)
            outs.append((result(x), models(x), x.kernel_times(reset=True)))
            x.profile(False)
            x.detect_best_collect()
        (res_c, m_c, t_c), (res_r, m_r, t_r) = outs
        assert res_c == res_r == ib.expected(cascade.blob, PAIRS, 5.0, FALLBACK)
        assert_same(m_r, m_c, "row form against the one-workgroup form")
        assert t_r["csp_init_rows"]["launches"] >= 1 and "csp_init" not in t_r and t_r["csb_resolve"]["launches"] >= 1
        assert t_c["csp_init"]["launches"] >= 1 and "csp_init_rows" not in t_c and t_c["csb_resolve"]["launches"] >= 1
    finally:
        r.close()


def test_row_form_leaves_untouched_streams_alone(bound, cascade):
    """the guard of k_csp_zero_models and k_csp_init_rows: without a fallback the noise frame's stream keeps its model under the row form"""
    r, twin = make_ctx(bound, "cs_pairs_cluster=1"), make_ctx(bound, "cs_pairs_cluster=1")
    try:
        pre_init(r, bound)
        pre_init(twin, bound)
        group(r)
        r.camshift_init_best(PAIRS, 5.0, None)
        codes, rects = result(r)
        assert codes.count(ib.UNTOUCHED) == 2  # the noise frame and c1_face (3.924 <= 5.0)
        r.detect_best_collect()
        host_handoff(twin, codes, rects)
        assert_same(models(r), models(twin), "row form: models")
        bound[1].bind(r), bound[1].bind(twin)
        assert_same(r.camshift_track_pairs(PAIRS), twin.camshift_track_pairs(PAIRS), "row form: track step")
    finally:
        r.close()
        twin.close()


@pytest.mark.parametrize("requeue", [False, True], ids=["collect", "collect_requeue"])
def test_track_steps_enqueued_behind_the_init_without_draining(ctxs, bound, requeue):
    """init_best -> two enqueue-only track steps -> collect of the best faces -> the two track results == the drained host sequence.  With
    collect_requeue a later grouping overwrites the records: the earlier init has already read them."""
    c, twin = ctxs
    pre_init(c, bound)
    pre_init(twin, bound)
    group(c)
    c.camshift_init_best(PAIRS, -10.0, FALLBACK)
    c.camshift_track_pairs(PAIRS, fetch=False)
    c.camshift_track_pairs(PAIRS, fetch=False)
    best, _t = c.detect_best_collect_requeue() if requeue else c.detect_best_collect()
    got = [c.camshift_track_collect(len(PAIRS)).copy() for _ in range(2)]
    codes, rects = result(c)
    # the host sequence, drained at every step
    group(twin)
    best_t, _t = twin.detect_best_collect()
    assert_same(best, best_t, "best faces")
    want = [ib.decide(best_t[f], -10.0, FALLBACK[i]) for i, (_s, f) in enumerate(PAIRS)]
    assert codes == [w[0] for w in want] and rects == [w[1] for w in want]
    host_handoff(twin, codes, rects)
    want_tracks = [twin.camshift_track_pairs(PAIRS).copy() for _ in range(2)]
    for k in range(2):
        assert_same(got[k], want_tracks[k], f"track step {k}")
    assert_same(models(c), models(twin), "models")
    if requeue:  # the batch in flight now: the same call reads ITS records (the same frames: the same decision), then it is collected
        c.camshift_init_best(PAIRS, -10.0, FALLBACK)
        assert result(c) == (codes, rects)
        best2, _t = c.detect_best_collect()
        assert_same(best2, best, "requeued batch")


def _refused(fn, status):
    with pytest.raises(HtError) as e:
        fn()
    assert e.value.status == status, (e.value.status, str(e.value))


def test_refusals_change_nothing(bound):
    c = make_ctx(bound)
    try:
        pre_init(c, bound)
        before = models(c)
        ok = PAIRS[:3]
        _refused(lambda: c.camshift_init_best(ok), native.HT_ERR_STATE)          # no device-grouped batch
        _refused(lambda: c.camshift_init_best_result(3), native.HT_ERR_STATE)    # no call to report on
        bound[0].bind(c, N - 1)  # a grouped batch of five frames ...
        group(c)
        bound[0].bind(c, N)      # ... and six bound frames: frame 5 is bound, and outside the batch
        bad = [
            [(0, N - 1)],                                   # frame >= grouped frames
            [(0, N)],                                       # frame not bound
            [(0, 0), (1, 1), (0, 2)],                       # duplicate stream
            [(S, 0)], [(-1, 0)],                            # unreserved stream
            [(s, 0) for s in range(S + 1)],                 # n > reserved
            [],                                             # n == 0
        ]
        for pairs in bad:
            _refused(lambda: c.camshift_init_best(pairs, -10.0), native.HT_ERR_INVALID)
            assert_same(models(c), before, ("refused", pairs))
        _refused(lambda: c.camshift_init_best(ok, float("nan")), native.HT_ERR_INVALID)
        _refused(lambda: c.camshift_init_best_result(3), native.HT_ERR_STATE)    # still no accepted call
        assert_same(models(c), before, "refused: NaN")
        with pytest.raises(ValueError):
            c.camshift_init_best(ok, -10.0, FALLBACK[:2])
        c.camshift_init_best(ok, 1e9, None)  # accepted: every pair untouched
        assert result(c, 3)[0] == [ib.UNTOUCHED] * 3
        assert_same(models(c), before, "threshold above every face")
        _refused(lambda: c.camshift_init_best_result(2), native.HT_ERR_STATE)    # n differs
        assert result(c, 3)[0] == [ib.UNTOUCHED] * 3                             # ... and the result is still there
        c.camshift_reserve(S + 4)
        _refused(lambda: c.camshift_init_best_result(3), native.HT_ERR_STATE)    # the trackers have been replaced
        assert_same(models(c), before, "after the reservation grew")
        c.detect_best_collect()
    finally:
        c.close()


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_device_handoff_from_node(tmp_path, cascade):
    """tests/js/init_best_gpu.js on the product addon: new ccv.DeviceBatch(.., {grouping: 'device', handoff: 'device'}) against the default
    (detectStep, enqueue -> track -> finish -> collect with and without {feeds}, a mini C5 loop), then the raw addon calls and their
    call-sequence errors"""
    import group_cases as gc
    from conftest import ROOT, load_golden
    from headtrackr_amd import build

    build.build_all()
    job = gc.js_job(tmp_path, cascade.blob, load_golden("detect.json"))
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "init_best_gpu.js"), str(jf)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] >= 11 and out["range_errors"] == 7 and out["state_errors"] == 4
    assert out["fallbacks"] == 1 and out["initialised"] == 2 and out["loop_tracks"] == 33

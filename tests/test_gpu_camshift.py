"""Parity of the HIP camshift path with the CPU oracle and the reference-JS golden vectors, through the C ABI.

Tolerance = BASELINE.json north_star: (x, y, width, height) within +-1 px, angle within +-0.5 deg.  width / height / search-window
size are multiples of 4 (`<< 2`, camshift.js:240-241) resp. floor(1.1 * that), so +-1 px means EQUAL for them; the moment sums are
binary64 on both sides but accumulated in a different (fixed) order, so x / y may in principle differ by one truncation step
(camshift.js:295-296) — the assertions allow exactly that one pixel and nothing else, every call that is not bit-for-bit the oracle's
is listed with (test, stream, call), and the module writes exact/total to gpurun_out/camshift_parity.json (also printed with -s)."""
import atexit
import json
import math
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
from cs_cases import ANGLE_TOL
from headtrackr_amd import synth
from headtrackr_amd.api import Context
from oracle import ht_oracle as ho

pytestmark = pytest.mark.gpu
CAMSHIFT = load_golden("camshift.json")

PARITY = {"exact": 0, "total": 0, "angle_max_abs_diff_rad": 0.0, "not_exact": []}


def _write_parity():
    if PARITY["total"]:
        out = os.path.join(ROOT, "gpurun_out")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "camshift_parity.json"), "w") as f:
            json.dump(PARITY, f, indent=1)
        print(f"camshift parity: {PARITY['exact']}/{PARITY['total']} track() calls bit-exact in (x, y, width, height, search window); "
              f"max |angle difference| {PARITY['angle_max_abs_diff_rad']:.3e} rad; not exact: {PARITY['not_exact'][:8]}")


atexit.register(_write_parity)


SCHEDULES = {"chunked": "cs_fused_min=1000000,cs_cluster=0", "fused": "cs_fused_min=1,cs_fused_nt=1024", "fused512": "cs_fused_min=1,cs_fused_nt=512",
             "cluster": "cs_fused_min=1000000,cs_cluster_min_px=1"}


@pytest.fixture(scope="module", params=list(SCHEDULES))
def ctx(request):
    """every test of this module runs on the camshift schedules: chunk histograms + one mean-shift workgroup per stream (few small
    streams), the single-launch kernel that is chosen for >= 192 streams (forced here with option cs_fused_min=1) in its 1024-thread
    form (one stream owns a CU) and its 512-thread form (two workgroups per CU), and chunk histograms + LUT + a cluster of workgroups per
    stream (<= 64 streams of frames from 10 000 pixels on, the default of cs_cluster_min_px; forced here for every size with
    cs_cluster_min_px=1)"""
    c = Context(options=SCHEDULES[request.param])
    yield c
    c.close()


def check(got, want_sw, want, stats, where=None, tally=()):
    """one track() call against the oracle / golden vector: sizes exact, positions +-1 px, angle +-0.5 deg; `stats` collects whether
    the call was bit-exact in every integer-valued output.  `tally`: keys of PARITY under which sub-totals are kept as well, each with
    its own largest angle difference"""
    sw = [int(got["sw_x"]), int(got["sw_y"]), int(got["sw_width"]), int(got["sw_height"])]
    exact = sw == list(want_sw)
    for a, b in zip(sw[:2], want_sw[:2]):
        assert abs(a - b) <= 1, (where, sw, want_sw)
    assert sw[2:] == list(want_sw[2:]), (where, sw, want_sw)  # floor(1.1 * size), size a multiple of 4: +-1 px means equal
    for k in ("x", "y"):
        assert abs(float(got[k]) - want[k]) <= 1, (where, k, got, want)
        exact = exact and float(got[k]) == want[k]
    for k in ("width", "height"):
        assert float(got[k]) == want[k], (where, k, got, want)  # multiples of 4 (`<< 2`, camshift.js:240-241): +-1 px means equal
    wa = want["angle"]
    if wa is None or (isinstance(wa, float) and math.isnan(wa)):
        assert math.isnan(float(got["angle"]))
    else:
        d = abs(float(got["angle"]) - wa)
        d = min(d, abs(d - math.pi))  # the angle is defined modulo pi
        assert d <= ANGLE_TOL, (where, got, want)
        PARITY["angle_max_abs_diff_rad"] = max(PARITY["angle_max_abs_diff_rad"], d)
    PARITY["total"] += 1
    PARITY["exact"] += int(exact)
    for key in tally:
        t = PARITY.setdefault(key, {"exact": 0, "total": 0, "angle_max_abs_diff_rad": 0.0})
        t["total"] += 1
        t["exact"] += int(exact)
        if not (wa is None or (isinstance(wa, float) and math.isnan(wa))):
            t["angle_max_abs_diff_rad"] = max(t["angle_max_abs_diff_rad"], d)
    if not exact:
        PARITY["not_exact"].append({"where": str(where), "got": [float(got[k]) for k in ("x", "y", "width", "height")] + sw,
                                    "want": [want[k] for k in ("x", "y", "width", "height")] + list(want_sw)})
    stats.append(exact)


def assert_all_exact(stats, what):
    """The reduction tree is fixed, so the result is deterministic: on these inputs every call reproduces the oracle bit for bit
    (measured: a row-major restatement of the oracle's column-major sums differs in 0 of 15 360 calls of the C3 shape)."""
    bad = len(stats) - sum(stats)
    assert bad == 0, f"{what}: {bad} of {len(stats)} track() calls within tolerance but not exact: {PARITY['not_exact'][-bad:][:5]}"


@pytest.mark.parametrize("case", CAMSHIFT["cases"], ids=lambda c: c["name"])
def test_golden_sequences(ctx, case):
    w, h = case["w"], case["h"]
    frames = [synth.make(g, w, h) for g in case["gen"]]
    ctx.set_geometry(w, h, 1)
    ctx.camshift_reserve(1)
    ctx.upload(frames[0][None])
    ctx.camshift_init([case["rect"]])
    stats = []
    for call in case["calls"]:
        ctx.upload(frames[call["frame"]][None])
        got = ctx.camshift_track(1, calc_angles=case["calcAngles"])[0]
        check(got, call["sw"], call, stats, where=(case["name"], 0, len(stats)))
    assert_all_exact(stats, case["name"])


def test_batch_of_streams_vs_oracle(ctx):
    """64 independent trackers in one batch (different targets, sizes, colours), 8 frames each, vs the oracle"""
    w, h, n, steps = 320, 240, 64, 8
    rng = synth.lcg_stream(99, 16 * n).astype(np.int64) >> 12
    specs = []
    for s in range(n):
        r = rng[16 * s : 16 * s + 16]
        cx, cy = 60 + int(r[0] % 200), 50 + int(r[1] % 140)
        a, b = 14 + int(r[2] % 30), 10 + int(r[3] % 20)
        rot = [(1, 0, 1), (4, 3, 5), (3, 4, 5), (12, 5, 13), (0, 1, 1)][int(r[4] % 5)]
        color = [(200, 60, 40), (40, 200, 80), (40, 80, 230), (220, 200, 30)][int(r[5] % 4)]
        specs.append((cx, cy, a, b, rot, color, [int(v % 7) - 3 for v in r[6:6 + 2 * 4]]))
    seqs = []
    for s, (cx, cy, a, b, rot, color, walk) in enumerate(specs):
        fr = []
        x, y = cx, cy
        for k in range(steps):
            fr.append(synth.blob_frame(w, h, x, y, a, b, rot, color, seed=1000 + 31 * s + k))
            x += walk[(2 * k) % len(walk)]
            y += walk[(2 * k + 1) % len(walk)]
        seqs.append(fr)
    rects = [(cx - a, cy - b, 2 * a, 2 * b) for (cx, cy, a, b, *_rest) in specs]
    ctx.set_geometry(w, h, n)
    ctx.camshift_reserve(n)
    ctx.upload(np.stack([seqs[s][0] for s in range(n)]))
    ctx.camshift_init(rects)
    oracles = []
    for s in range(n):
        o = ho.Camshift(True)
        o.init_tracker(seqs[s][0], rects[s])
        oracles.append(o)
    stats = []
    for k in range(1, steps):
        ctx.upload(np.stack([seqs[s][k] for s in range(n)]))
        got = ctx.camshift_track(n, calc_angles=True)
        for s in range(n):
            sw, to = oracles[s].track(seqs[s][k])
            check(got[s], sw, to, stats, where=("batch64", s, k))
    assert_all_exact(stats, "64 streams x 7 calls")


@pytest.mark.parametrize("w,h,n", [(1920, 1080, 1), (641, 363, 3), (61, 45, 2)], ids=["1080p-1stream", "odd-641x363", "tiny-61x45"])
@pytest.mark.parametrize("fused", list(SCHEDULES))
def test_frame_sizes_and_chunking(w, h, n, fused):
    """The histogram pass cuts a frame into chunk histograms (127 for one 1080p stream, 1 for a tiny frame) and handles
    pixel counts that are not multiples of 4; the mean-shift kernel adds the chunks.  Same answers as the oracle."""
    steps = 4
    a, b = max(3, w // 5), max(2, h // 9)  # elongated: a well-conditioned orientation
    seqs, rects = [], []
    for s in range(n):
        cx, cy = w // 2 + 3 * s, h // 2 - 2 * s
        seqs.append([synth.blob_frame(w, h, cx + k, cy + k // 2, a, b, (4, 3, 5), (200, 60, 40), seed=77 + 13 * s + k) for k in range(steps)])
        rects.append((cx - a, cy - b, 2 * a, 2 * b))
    c = Context(options=SCHEDULES[fused])
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.upload(np.stack([seqs[s][0] for s in range(n)]))
        c.camshift_init(rects)
        oracles = []
        for s in range(n):
            o = ho.Camshift(True)
            o.init_tracker(seqs[s][0], rects[s])
            oracles.append(o)
        stats = []
        for k in range(1, steps):
            c.upload(np.stack([seqs[s][k] for s in range(n)]))
            got = c.camshift_track(n, calc_angles=True)
            for s in range(n):
                sw, to = oracles[s].track(seqs[s][k])
                check(got[s], sw, to, stats, where=(f"{w}x{h}", s, k))
        assert_all_exact(stats, f"{w}x{h}")
    finally:
        c.close()


def test_detect_then_track_like_facetrackr(ctx, golden_facetrackr):
    """facetrackr's VJ -> CS hand-over (facetrackr.js:97-108,185-217) driven from Python: detect, floor the best rect,
    initTracker on the COLOUR frame, then track — against the reference-JS state-machine vector"""
    case = next(c for c in golden_facetrackr["cases"] if c["name"] == "ft_nowb_moving")
    w, h = case["w"], case["h"]
    frames = [synth.make(g, w, h) for g in case["gen"]]
    calls = case["calls"]
    rects = ctx.detect_objects(frames[0][None], min_neighbors=1)[0]
    best = rects[int(np.argmax(rects["confidence"]))]  # strict '>' keeps the first maximum (facetrackr.js:161-165)
    assert calls[0]["detection"] == "VJ"
    for k in ("x", "y", "width", "height", "confidence"):
        assert best[k] == calls[0][k]
    ctx.camshift_reserve(1)
    ctx.upload(frames[0][None])
    ctx.camshift_init([[math.floor(best["x"]), math.floor(best["y"]), math.floor(best["width"]), math.floor(best["height"])]])
    stats = []
    for i in range(1, len(frames)):
        ctx.upload(frames[i][None])
        got = ctx.camshift_track(1, calc_angles=True)[0]
        assert calls[i]["detection"] == "CS"
        for k in ("x", "y"):
            assert abs(float(got[k]) - calls[i][k]) <= 1
        for k in ("width", "height"):
            assert float(got[k]) == calls[i][k]
        stats.append(all(float(got[k]) == calls[i][k] for k in ("x", "y", "width", "height")))
    assert sum(stats) == len(stats)


def _feeds_1080p(nfeeds, steps):
    w, h = 1920, 1080
    feeds, rects = [], []
    for s in range(nfeeds):
        cx, cy, a, b = 500 + 150 * s, 400 + 40 * s, 180, 120
        feeds.append([synth.blob_frame(w, h, cx + 2 * k, cy + k, a, b, (4, 3, 5), (200, 60, 40), seed=300 + 17 * s + k) for k in range(steps)])
        rects.append((cx - a, cy - b, 2 * a, 2 * b))
    return feeds, rects


def test_six_contexts_track_1080p_feeds_concurrently():
    """Six contexts (own HIP streams), each tracking one 1920x1080 feed with the CLUSTER mean-shift (32 workgroups per stream that
    spin on each other at every moment pass).  Every context's whole call sequence is enqueued before any result is fetched, so the
    six streams have cluster grids pending at the same time (6 x 32 x up to 11 barriers each): cluster launches are serialised per
    device, the spin is bounded, nothing hangs and every call == the oracle."""
    from hipmem import DeviceArray

    nctx, steps = 6, 5
    w, h = 1920, 1080
    feeds, rects = _feeds_1080p(nctx, steps)
    ctxs = [Context() for _ in range(nctx)]
    dev = [[DeviceArray(f) for f in feeds[i]] for i in range(nctx)]
    try:
        for i, c in enumerate(ctxs):
            c.set_geometry(w, h, 1)
            c.camshift_reserve(1)
            c.bind_device(dev[i][0].ptr, 1)
            c.camshift_init([rects[i]])
        for rounds in range(2):  # twice: the second round starts from the first round's tracker state
            for i, c in enumerate(ctxs):
                c.camshift_track_sequence([d.ptr for d in dev[i][1:]], 1, calc_angles=True, fetch="none", keep_all=True)
        stats = []
        for i, c in enumerate(ctxs):
            got = c.camshift_sequence_collect(1, steps - 1, fetch="all")  # the second round's results
            o = ho.Camshift(True)
            o.init_tracker(feeds[i][0], rects[i])
            for rounds in range(2):
                for k in range(1, steps):
                    sw, to = o.track(feeds[i][k])
                    if rounds == 1:
                        check(got[k - 1, 0], sw, to, stats, where=("6ctx", i, k))
        assert len(stats) == nctx * (steps - 1)
        assert_all_exact(stats, "6 contexts x 1080p")
    finally:
        for c in ctxs:
            c.close()
        for row in dev:
            for d in row:
                d.free()


def test_cluster_barrier_timeout_is_a_status_code():
    """The cluster barrier is a bounded spin: with a budget of one cycle every workgroup that arrives early gives up at once; the
    call must come back with HT_ERR_STATE (never hang), and the context must work again afterwards."""
    from headtrackr_amd.api import HtError

    w, h = 1920, 1080
    feeds, rects = _feeds_1080p(1, 3)
    c = Context(options="cs_barrier_budget=1")
    good = Context()
    try:
        for cx in (c, good):
            cx.set_geometry(w, h, 1)
            cx.camshift_reserve(1)
            cx.upload(feeds[0][0][None])
            cx.camshift_init([rects[0]])
            cx.upload(feeds[0][1][None])
        with pytest.raises(HtError) as e:
            c.camshift_track(1, calc_angles=True)
        assert e.value.status == -6 and "barrier" in str(e.value)
        want = good.camshift_track(1, calc_angles=True)[0]
        o = ho.Camshift(True)
        o.init_tracker(feeds[0][0], rects[0])
        sw, to = o.track(feeds[0][1])
        check(want, sw, to, [], where=("timeout-good", 0, 0))
    finally:
        c.close()
        good.close()


def test_order_sensitive_call_lands_on_one_of_the_two_sides(ctx):
    """A case the randomised soak of round 6 found (tools/gpu_soak.py, seed 1790745752; kept as tests/golden/camshift_tie_case.npz): in the third
    mean-shift iteration of call 4 only ONE column of the 4-pixel-wide search window has non-zero weights, so xc = M10 / M00 is exactly 3 in real
    arithmetic and `toint32(xc - 2)` is decided by the rounding noise of the binary64 sums — the reference's column-major loop gets 3.0000000000000004
    (window moves right), the SAME loop with even and odd rows added apart gets the other side (tests/test_oracle_golden.py checks that on the CPU).
    No parallel reduction can promise the reference's side of such a tie; every schedule must still return one of the two results, and calls 1 - 3,
    which are not ties, exactly."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "camshift_tie_case.npz"))
    frames, rect = z["frames"][0], tuple(int(v) for v in z["rects"][0])
    h, w = frames.shape[1], frames.shape[2]
    o = ho.Camshift(True)
    o.init_tracker(frames[0], rect)
    ctx.set_geometry(w, h, 1)
    ctx.camshift_reserve(1)
    ctx.upload(frames[0][None])
    ctx.camshift_init([rect])
    stats = []
    for k in range(1, 5):
        sw, to = o.track(frames[k])
        ctx.upload(frames[k][None])
        got = ctx.camshift_track(1, calc_angles=True)[0]
        if k < 4:
            check(got, sw, to, stats, where=("tie-case", 0, k))
        else:
            assert [float(to[f]) for f in ("x", "y", "width", "height")] == [37.0, 23.0, 0.0, 12.0] and [int(v) for v in sw] == [35, 15, 0, 13]  # the reference's side
            g = [float(got[f]) for f in ("x", "y", "width", "height")] + [int(got[f]) for f in ("sw_x", "sw_y", "sw_width", "sw_height")]
            assert g in ([37.0, 23.0, 0.0, 12.0, 35, 15, 0, 13], [36.0, 23.0, 0.0, 8.0, 34, 15, 0, 8]), g
    assert_all_exact(stats, "tie case, calls 1 - 3")

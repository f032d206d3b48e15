"""Parity at the BENCHMARK shapes (BASELINE.json configs C2 / C3 / C4) — every frame / stream against the CPU oracle, not a
sample — plus the hooks added for them: histogram read-back, the camshift call sequence, the white-balance sums fused into
the gray pass, and the context's behaviour when a geometry cannot be allocated.  Everything goes through the C ABI."""
import math

import numpy as np
import pytest

from headtrackr_amd import synth
from headtrackr_amd.api import Context, HtError
from headtrackr_amd.native import HT_DETECT_WHITEBALANCE, HT_SCAN_STATS
from oracle import ht_oracle as ho
from test_gpu_camshift import assert_all_exact as cs_all_exact, check as cs_check
from test_gpu_detect import assert_hits_equal, oracle_hits

pytestmark = pytest.mark.gpu


def test_c2_batch_every_frame_vs_oracle(cascade):
    """C2 (256 x 320x240, the bench's own frames): raw hits of EVERY frame == the oracle's, bit for bit, and the best face
    per frame (grouping + facetrackr's selection, the bench's timed step) == the oracle's."""
    w, h, n = 320, 240, 256
    frames = synth.mixed_batch(n, w, h, seed0=1234)
    c = Context()
    try:
        hits, counts = c.detect_raw(frames)
        ref = np.concatenate([oracle_hits(frames[i], cascade, i) for i in range(n)])
        assert_hits_equal(hits, ref)
        assert np.array_equal(counts, np.bincount(ref["frame"], minlength=n))
        best = c.best_faces(hits, counts, 1)
        want = ho.best_faces(frames, cascade.blob, 1)
        for k in ("x", "y", "width", "height", "confidence", "neighbors"):
            assert np.array_equal(best[k], want[k]), k
        assert int((best["neighbors"] > 0).sum()) > n // 3 * 0.9
        c.detect_enqueue(0)  # the one-call form the batch bench uses
        best2, nhits = c.detect_collect_best(1)
        assert nhits == len(hits) and best2.tobytes() == best.tobytes()
    finally:
        c.close()


def test_c4_batch_shape_every_frame_vs_oracle(cascade):
    """C4 per-GPU shape: 128 x 1280x720 built from the first 12 of the bench's 128 distinct frames (tile count, XCD ordering, survivor
    queue at 129 M windows): every frame's hits and the per-stage window counts == the oracle's."""
    w, h, n, uniq = 1280, 720, 128, 12
    base = synth.mixed_batch(uniq, w, h, seed0=1234)
    frames = base[np.arange(n) % uniq]
    stage_ref = np.zeros(cascade.count + 1, dtype=np.int64)
    per_unique = []
    for u in range(uniq):
        sp = np.zeros(cascade.count + 1, dtype=np.int64)
        hits_u = ho.detect_raw(base[u], cascade.blob, stage_pass=sp)
        per_unique.append(hits_u)
        stage_ref += sp * len([i for i in range(n) if i % uniq == u])
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.upload(frames)
        c.detect_enqueue(HT_SCAN_STATS)
        hits, counts = c.detect_collect(cap=1 << 17)
        assert c.windows_per_frame == 1007428
        got_stage = c.stage_counts().astype(np.int64)
        assert np.array_equal(got_stage, stage_ref), (got_stage, stage_ref)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert len(hits) == starts[-1] and len(hits) > 100
        for i in range(n):
            got = hits[starts[i] : starts[i + 1]]
            r = per_unique[i % uniq]
            assert len(got) == len(r), f"frame {i}"
            assert np.all(got["frame"] == i)
            for k in ("scale", "q", "x", "y"):
                assert np.array_equal(got[k].astype(np.int64), r[k].astype(np.int64)), (i, k)
            assert np.array_equal(got["sum"].view(np.uint64), r["sum"].view(np.uint64)), f"frame {i}: confidence bits"
    finally:
        c.close()


@pytest.mark.parametrize("rank", list(range(8)))
def test_c4_bench_frames_all_128_distinct_vs_oracle(cascade, rank):
    """The frames bench.py TIMES at C4: all 128 distinct 1280x720 frames of a rank's batch (seed 1234 + 1000 * rank) for EVERY rank
    of the 8-GPU run of BASELINE.json configs[3] — rank r > 0 times frames no other test has seen —, in one batch like the bench:
    every frame's raw hits (indices + binary64 confidence bits), the per-stage window counts and the best face per frame == the
    oracle's."""
    w, h, n = 1280, 720, 128
    frames = synth.mixed_batch(n, w, h, seed0=1234 + 1000 * rank)
    stage_ref = np.zeros(cascade.count + 1, dtype=np.int64)
    ref = []
    for i in range(n):
        sp = np.zeros(cascade.count + 1, dtype=np.int64)
        ref.append(ho.detect_raw(frames[i], cascade.blob, stage_pass=sp))
        stage_ref += sp
    c = Context()
    try:
        c.set_geometry(w, h, n)
        c.upload(frames)
        c.detect_enqueue(HT_SCAN_STATS)
        hits, counts = c.detect_collect(cap=1 << 17)
        assert np.array_equal(c.stage_counts().astype(np.int64), stage_ref)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert len(hits) == starts[-1] == sum(len(r) for r in ref) and len(hits) > 300
        for i in range(n):
            got, r = hits[starts[i] : starts[i + 1]], ref[i]
            assert len(got) == len(r), f"frame {i}"
            assert np.all(got["frame"] == i)
            for k in ("scale", "q", "x", "y"):
                assert np.array_equal(got[k].astype(np.int64), r[k].astype(np.int64)), (i, k)
            assert np.array_equal(got["sum"].view(np.uint64), r["sum"].view(np.uint64)), f"frame {i}: confidence bits"
        c.detect_enqueue(0)  # the bench's timed call
        best, nhits = c.detect_collect_best(1)
        assert nhits == len(hits)
        want = np.zeros(n, dtype=ho.RECT_DTYPE)
        for i in range(n):
            g = ho.group(ho.hits_to_rects(ref[i]), 1)
            want[i]["confidence"] = -10000.0
            for k in range(len(g)):
                if k == 0 or g[k]["confidence"] > want[i]["confidence"]:
                    want[i] = g[k]
        for k in ("x", "y", "width", "height", "confidence", "neighbors"):
            assert np.array_equal(best[k], want[k]), k
    finally:
        c.close()


def test_c4_strong_shape_1024_frames_on_one_gpu(cascade):
    """The `c4_strong` sub-record of the bench line: all 1024 x 1280x720 frames of BASELINE.json configs[3] in ONE batch on one GPU
    (15 x the tile count, survivor queue and hit volume of the 128-frame shape; 1.03 G windows): every frame's raw hits — indices and
    binary64 confidence bits — and the per-stage window counts == the oracle's.  Frames are the first 12 of the bench's distinct frames, tiled."""
    from hipmem import DeviceArray

    w, h, n, uniq = 1280, 720, 1024, 12
    base = synth.mixed_batch(uniq, w, h, seed0=1234)
    per_unique, stage_unique = [], []
    for u in range(uniq):
        sp = np.zeros(cascade.count + 1, dtype=np.int64)
        per_unique.append(ho.detect_raw(base[u], cascade.blob, stage_pass=sp))
        stage_unique.append(sp)
    reps = np.bincount(np.arange(n) % uniq, minlength=uniq)
    stage_ref = sum(int(reps[u]) * stage_unique[u] for u in range(uniq))
    c = Context()  # first: ht_create selects the device
    dev = DeviceArray.tiled(base, n)
    try:
        c.set_geometry(w, h, n)
        c.bind_device(dev.ptr, n)
        c.detect_enqueue(HT_SCAN_STATS)
        hits, counts = c.detect_collect(cap=1 << 20)
        assert len(counts) == n and c.windows_per_frame * n == stage_ref[0] == 1007428 * 1024
        assert np.array_equal(c.stage_counts().astype(np.int64), stage_ref)
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        assert len(hits) == starts[-1] == sum(int(reps[u]) * len(per_unique[u]) for u in range(uniq))
        for i in range(n):
            got, r = hits[starts[i] : starts[i + 1]], per_unique[i % uniq]
            assert len(got) == len(r), f"frame {i}"
            assert np.all(got["frame"] == i)
            for k in ("scale", "q", "x", "y"):
                assert np.array_equal(got[k].astype(np.int64), r[k].astype(np.int64)), (i, k)
            assert np.array_equal(got["sum"].view(np.uint64), r["sum"].view(np.uint64)), f"frame {i}: confidence bits"
        # the bench's timed step at this shape: one call, best face per frame, next batch re-enqueued inside it
        c.detect_enqueue(0)
        best, nhits = c.detect_collect_best_requeue(1)
        best = best.copy()
        best2, nhits2 = c.detect_collect_best(1)
        assert nhits == nhits2 == len(hits) and best.tobytes() == best2.tobytes()
        want = ho.best_faces(base, cascade.blob, 1)
        for i in range(n):
            assert best[i].tobytes() == want[i % uniq].tobytes(), i
    finally:
        c.close()
        dev.free()


def _c3_streams(n, w, h, nv):
    """the bench's C3 input: one vote-image face per stream, moved by a seeded <= 3 px walk over nv frame versions"""
    walk = synth.lcg_stream(4242, 2 * nv * n).astype(np.int64) >> 20
    vers = np.empty((nv, n, h, w, 4), dtype=np.uint8)
    for f in range(n):
        s0 = 48 + (f * 7) % 80
        x, y = 20 + (f * 13) % (w - s0 - 40), 16 + (f * 29) % (h - s0 - 32)
        for v in range(nv):
            vers[v, f] = synth.face_frame(w, h, [(x, y, s0)])
            x += int(walk[2 * (f * nv + v)] % 7) - 3
            y += int(walk[2 * (f * nv + v) + 1] % 7) - 3
    return vers


def test_c3_shape_256_streams_60_calls_vs_oracle(cascade):
    """C3: 256 streams, detect once, initTracker on the floored best face (facetrackr.js:97-108), then 60 track() calls in ONE
    ht_camshift_track_sequence: every call of every stream within +-1 px / +-0.5 deg of the oracle (sizes equal) and — the
    reduction tree being fixed — all 15 360 calls bit-exact; exact/total goes to gpurun_out/camshift_parity.json."""
    from hipmem import DeviceArray

    w, h, n, nv, calls = 320, 240, 256, 4, 60
    vers = _c3_streams(n, w, h, nv)
    c = Context()  # first: ht_create selects the device
    dev = [DeviceArray(vers[v]) for v in range(nv)]
    try:
        c.set_geometry(w, h, n)
        c.bind_device(dev[0].ptr, n)
        c.camshift_reserve(n)
        c.detect_enqueue(0)
        hits, counts = c.detect_collect(cap=1 << 17)
        best = c.best_faces(hits, counts, 1)
        assert int((best["neighbors"] > 0).sum()) >= 0.9 * n
        rects = [(math.floor(best["x"][f]), math.floor(best["y"][f]), math.floor(best["width"][f]), math.floor(best["height"][f]))
                 if best["neighbors"][f] > 0 else (w // 4, h // 4, w // 2, h // 2) for f in range(n)]
        c.camshift_init(rects)
        got = c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True, fetch="all")
        assert got.shape == (calls, n)
        stats = []
        for f in range(n):
            o = ho.Camshift(True)
            o.init_tracker(vers[0, f], rects[f])
            for k in range(calls):
                sw, to = o.track(vers[(k + 1) % nv, f])
                cs_check(got[k, f], sw, to, stats, where=("c3", f, k))
        assert len(stats) == n * calls
        cs_all_exact(stats, "C3 shape, 256 streams x 60 calls")
        # the sequence call == the same calls issued one by one
        c.camshift_init(rects)
        for k in range(3):
            c.bind_device(dev[(k + 1) % nv].ptr, n)
            one = c.camshift_track(n, calc_angles=True)
            assert one.tobytes() == got[k].tobytes(), k
        # enqueue only + ht_camshift_sequence_collect == fetched in the same call (all calls, and the last one)
        c.bind_device(dev[0].ptr, n)  # initTracker reads the bound frames
        c.camshift_init(rects)
        assert c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True, fetch="none", keep_all=True) is None
        assert c.camshift_sequence_collect(n, calls, fetch="all").tobytes() == got.tobytes()
        c.camshift_init(rects)
        c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True, fetch="none")
        assert c.camshift_sequence_collect(n, calls).tobytes() == got[calls - 1].tobytes()
        px, ncalls = c.camshift_stats(n, reset=True)
        assert np.all(ncalls == calls) and np.all(px > 0)  # initTracker resets the counters: the last enqueue-only sequence
        # more calls than one launch carries (64): the second launch continues where the first stopped
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)
        longer = c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls + 6)], n, calc_angles=True, fetch="all")
        assert longer[:calls].tobytes() == got.tobytes()
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)
        c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True)
        for k in range(calls, calls + 6):
            c.bind_device(dev[(k + 1) % nv].ptr, n)
            assert c.camshift_track(n, calc_angles=True).tobytes() == longer[k].tobytes(), k
    finally:
        c.close()
        for d in dev:
            d.free()


def test_fused_track_kernel_forms_return_the_same_bits(cascade):
    """k_cs_track_fused exists in a 1024-thread form (one stream owns a CU) and a 512-thread form (two workgroups per CU, chosen when a
    launch has more streams than the device has CUs or when another context of the device that tracks on this path has work in
    flight at launch time: the launches then share the CUs).  The small form's wavefronts play the sixteen of the large one, so
    every track object is identical to the last bit of the angle — forced forms on the C3 shape, then the automatic choice with a
    context on its own and with two contexts' sequences in flight at the same time."""
    from hipmem import DeviceArray

    w, h, n, nv, calls = 320, 240, 256, 4, 12
    vers = _c3_streams(n, w, h, nv)
    rects = [(w // 4 + (f % 7), h // 4 + (f % 5), w // 3, h // 3) for f in range(n)]
    ctxs = [Context(options="cs_fused_nt=1024"), Context(options="cs_fused_nt=512"), Context(), Context()]
    dev = [DeviceArray(vers[v]) for v in range(nv)]
    try:
        outs = []
        for c in ctxs:
            c.set_geometry(w, h, n)
            c.bind_device(dev[0].ptr, n)
            c.camshift_reserve(n)
            c.camshift_init(rects)
        for c in ctxs[:3]:  # the third one chooses by itself (every call here is collected before the next context starts)
            outs.append(c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True, fetch="all"))
        # two contexts on the automatic rule with their sequences in flight at the same time
        for c in ctxs[2:]:
            c.bind_device(dev[0].ptr, n)
            c.camshift_init(rects)
        for c in ctxs[2:]:
            assert c.camshift_track_sequence([dev[(k + 1) % nv].ptr for k in range(calls)], n, calc_angles=True, fetch="none", keep_all=True) is None
        for c in ctxs[2:]:
            outs.append(c.camshift_sequence_collect(n, calls, fetch="all"))
        # and one call at a time
        c = ctxs[1]
        c.bind_device(dev[0].ptr, n)
        c.camshift_init(rects)
        for k in range(3):
            c.bind_device(dev[(k + 1) % nv].ptr, n)
            assert c.camshift_track(n, calc_angles=True).tobytes() == outs[0][k].tobytes(), k
        for i, o in enumerate(outs[1:]):
            assert o.tobytes() == outs[0].tobytes(), i + 1
        moved = sum(int(outs[0][calls - 1][f]["sw_x"]) != rects[f][0] for f in range(n))
        assert moved > n // 2  # the trackers did something
    finally:
        for c in ctxs:
            c.close()
        for d in dev:
            d.free()


@pytest.mark.parametrize("fused", [0, 1024, 512, "cluster"], ids=["chunked", "fused", "fused512", "cluster"])
def test_camshift_histograms_bin_for_bin(fused):
    """camshift.Histogram (camshift.js:49-72): the model histogram of initTracker and the full-frame histogram of track(),
    read back from the device, equal the oracle's in every one of the 4096 bins — incl. a rect reaching outside the frame
    (transparent black -> bin 0), an odd pixel count, and a frame cut into many chunk histograms; on every schedule (the
    single-launch kernel keeps its histogram in LDS and only writes it out with option cs_keep_hist)."""
    if fused == "cluster":  # chunk histograms -> LUT kernel -> cluster mean-shift, forced for every frame size
        opts = "cs_fused_min=1000000,cs_cluster_min_px=1,cs_keep_hist=1"
    else:
        opts = f"cs_fused_min={1 if fused else 1000000},cs_keep_hist=1" + (f",cs_fused_nt={fused}" if fused else "")
    for (w, h, rect) in [(320, 240, (100, 60, 90, 80)), (321, 243, (-10, -5, 60, 70)), (1280, 720, (1200, 650, 200, 200))]:
        a = synth.blob_frame(w, h, w // 2, h // 2, w // 6, h // 8, (4, 3, 5), (200, 60, 40), seed=5)
        b = synth.blob_frame(w, h, w // 2 + 3, h // 2 + 2, w // 6, h // 8, (4, 3, 5), (200, 60, 40), seed=6)
        c = Context(options=opts)
        try:
            c.set_geometry(w, h, 1)
            c.camshift_reserve(1)
            c.upload(a[None])
            c.camshift_init([rect])
            c.upload(b[None])
            c.camshift_track(1, calc_angles=True)
            model, cur = c.camshift_debug_hist(0)
            o = ho.cs_init(a, *rect)
            want_model, want_cur = ho.cs_histograms(o, b)
            assert np.array_equal(model.astype(np.int64), want_model), (w, h)
            assert np.array_equal(cur.astype(np.int64), want_cur), (w, h)
            assert int(model.sum()) == rect[2] * rect[3] and int(cur.sum()) == w * h
        finally:
            c.close()


@pytest.mark.parametrize("w,h", [(320, 240), (201, 157), (1280, 720)])
def test_whitebalance_fused_into_gray_pass(w, h, cascade):
    """HT_DETECT_WHITEBALANCE: getWhitebalance's channel sums ride along with the gray pass (or, for widths that are not
    multiples of 4, a separate pass): same value as the stand-alone entry point and the oracle, detect results unchanged."""
    frames = synth.mixed_batch(5, w, h, seed0=77)
    c = Context()
    try:
        plain, _ = c.detect_raw(frames)
        c.detect_enqueue(HT_DETECT_WHITEBALANCE)
        hits, _ = c.detect_collect()
        assert hits.tobytes() == plain.tobytes()
        wb = c.detect_whitebalance()
        want = np.array([ho.whitebalance(f) for f in frames])
        assert np.array_equal(wb, want)
        assert np.array_equal(c.whitebalance(), want)
        c.detect_enqueue(0)
        c.detect_collect()
        with pytest.raises(HtError):
            c.detect_whitebalance()
    finally:
        c.close()


def test_failed_geometry_leaves_a_clean_context(cascade):
    """A geometry that cannot be allocated (arena far beyond the device) must fail with HT_ERR_NOMEM and leave the context
    without a half-built geometry: the natural 'try a big batch, fall back to a smaller one' then works."""
    frames = synth.mixed_batch(3, 320, 240, seed0=1234)
    c = Context()
    try:
        want, _ = c.detect_raw(frames)
        with pytest.raises(HtError) as e:
            c.set_geometry(1920, 1080, 200000)  # ~2.6 TB of pyramid
        assert e.value.status == -3
        with pytest.raises(HtError):
            c.detect_enqueue(0)  # nothing bound any more
        c._max_batch = 0
        got, _ = c.detect_raw(frames)  # smaller batch: re-plans from scratch
        assert got.tobytes() == want.tobytes()
        with pytest.raises(HtError) as e:
            c.set_geometry(320, 240, 3, level_dims=np.full(2 * c.num_levels, 999999, dtype=np.int32))
        assert e.value.status == -1
        half = np.array(ho.pyramid_layout(320, 240), dtype=np.int32)
        half[6] = (161, 120)  # wider than half of level 0: the scan's windows would leave level 0 (ht_check_level_dims)
        with pytest.raises(HtError) as e:
            c.set_geometry(320, 240, 3, level_dims=half)
        assert e.value.status == -1 and "level 6 (161x120) is larger than half of level 0 (320x240)" in str(e.value)
        c.upload(frames)  # bad level_dims are rejected BEFORE the current geometry is torn down
        c.detect_enqueue(0)
        got, _ = c.detect_collect()
        assert got.tobytes() == want.tobytes()
    finally:
        c.close()


def test_collect_reports_the_enqueued_batch(cascade):
    """enqueue(A: 4 frames) -> swap in B (2 frames) -> collect: counts[] has A's 4 entries and A's hits"""
    A = np.ascontiguousarray(synth.mixed_batch(4, 320, 240, seed0=1234))
    B = np.ascontiguousarray(synth.mixed_batch(2, 320, 240, seed0=4321))
    c = Context()
    try:
        c.set_geometry(320, 240, 4)
        want, want_counts = c.detect_raw(A)
        c.upload(A)
        c.upload_async_ptr(B.ctypes.data, 2)
        c.detect_enqueue(0)
        c.swap_frames()
        got, counts = c.detect_collect()
        assert got.tobytes() == want.tobytes() and np.array_equal(counts, want_counts)
    finally:
        c.close()


def test_allgather_best_faces_over_rccl(cascade):
    """The single-process exchange step (ht_allgather_best_faces): one context per visible GPU, frames block-sharded, every
    rank's best-face rects all-gathered over RCCL and checked to be identical on every GPU.  With one GPU the call still goes
    through dlopen(librccl) + ncclCommInitAll + ncclAllGather (option force_rccl)."""
    from headtrackr_amd import api, distributed as hd

    ndev = api.device_count()
    assert ndev >= 1
    n = 6 * ndev + (1 if ndev > 1 else 0)
    frames = synth.mixed_batch(n, 320, 240, seed0=1234)
    per = -(-n // ndev)
    ctxs, bests = [], []
    try:
        for r in range(ndev):
            a, b = hd.shard_range(n, r, ndev)
            c = Context(device=r, options="force_rccl=1")
            ctxs.append(c)
            hits, counts = c.detect_raw(frames[a:b])
            best = np.zeros(per, dtype=api.RECT_DTYPE)
            best[: b - a] = c.best_faces(hits, counts, 1)
            bests.append(best)
        g = api.allgather_best_faces(ctxs, bests)
        assert g.shape == (ndev, per)
        want = ho.best_faces(frames, cascade.blob, 1)
        for r in range(ndev):
            a, b = hd.shard_range(n, r, ndev)
            assert g[r, : b - a].tobytes() == want[a:b].tobytes()
            assert g[r].tobytes() == bests[r].tobytes()
        assert int((g["neighbors"] > 0).sum()) >= 2
    finally:
        for c in ctxs:
            c.close()


def test_whitebalance_survives_requeue_and_swap(cascade):
    """ht_detect_collect_best_requeue enqueues the NEXT batch inside the collect call; ht_detect_whitebalance must still report the
    batch that was collected — also when other frames were swapped in meanwhile and whether or not the next batch carries the flag."""
    A = np.ascontiguousarray(synth.mixed_batch(4, 320, 240, seed0=1234))
    B = np.ascontiguousarray(synth.mixed_batch(3, 320, 240, seed0=4321))
    wa, wb = np.array([ho.whitebalance(f) for f in A]), np.array([ho.whitebalance(f) for f in B])
    c = Context()
    try:
        c.set_geometry(320, 240, 4)
        c.upload(A)
        c.detect_enqueue(HT_DETECT_WHITEBALANCE)
        c.upload_async_ptr(B.ctypes.data, 3)
        c.swap_frames()  # B is bound now; the batch in flight is A
        best_a, _ = c.detect_collect_best_requeue(1, next_flags=HT_DETECT_WHITEBALANCE)  # collects A, enqueues B (with the flag)
        assert len(best_a) == 4
        assert np.array_equal(c.detect_whitebalance(), wa)  # A's values, not B's; no wait for B
        best_b, _ = c.detect_collect_best_requeue(1, next_flags=0)  # collects B, enqueues B again WITHOUT the flag
        assert len(best_b) == 3
        assert np.array_equal(c.detect_whitebalance(), wb)  # still available although the batch in flight has no sums
        assert np.array_equal(c.whitebalance(), wb)  # the stand-alone call does not disturb the batch in flight ...
        c.detect_collect_best(1)
        with pytest.raises(HtError):  # ... and the batch collected last carried no flag
            c.detect_whitebalance()
        c.detect_enqueue(HT_DETECT_WHITEBALANCE)
        assert np.array_equal(c.whitebalance(), wb)  # stand-alone sums while a flagged batch is in flight: separate regions
        c.detect_collect()
        assert np.array_equal(c.detect_whitebalance(), wb)
    finally:
        c.close()


def test_python_wrapper_sizes_buffers_by_the_enqueued_batch(cascade):
    """enqueue 4 frames, swap in 2, collect: the library reports on the 4 enqueued frames — the wrapper's buffers must hold them
    (it used to size them by the 2 frames bound at collect time: heap overflow)."""
    A = np.ascontiguousarray(synth.mixed_batch(4, 320, 240, seed0=1234))
    B = np.ascontiguousarray(synth.mixed_batch(2, 320, 240, seed0=4321))
    c = Context()
    try:
        c.set_geometry(320, 240, 4)
        want, want_counts = c.detect_raw(A)
        want_best = c.best_faces(want, want_counts, 1)
        for mode in ("collect", "best", "requeue"):
            c.upload(A)
            c.upload_async_ptr(B.ctypes.data, 2)
            c.detect_enqueue(0)
            c.swap_frames()
            assert c.nframes == 2
            if mode == "collect":
                got, counts = c.detect_collect()
                assert got.tobytes() == want.tobytes() and np.array_equal(counts, want_counts)
            elif mode == "best":
                best, nh = c.detect_collect_best(1)
                assert len(best) == 4 and best.tobytes() == want_best.tobytes() and nh == len(want)
            else:
                best, nh = c.detect_collect_best_requeue(1)
                assert len(best) == 4 and best.tobytes() == want_best.tobytes()
                nxt, _ = c.detect_collect_best(1)  # the re-enqueued batch covers the 2 frames bound at that time
                assert len(nxt) == 2
    finally:
        c.close()


def test_sequence_collect_requires_the_pending_sequence(cascade):
    """ht_camshift_sequence_collect only returns the sequence that was enqueued with out == NULL, in the layout it was enqueued with"""
    from hipmem import DeviceArray

    w, h, n = 320, 240, 4
    fr = np.stack([synth.face_frame(w, h, [(100 + 2 * i, 60, 96)]) for i in range(n)])
    c = Context()
    dev = DeviceArray(fr)
    try:
        c.set_geometry(w, h, n)
        c.bind_device(dev.ptr, n)
        c.camshift_reserve(n)
        c.camshift_init([(100 + 2 * i, 60, 90, 90) for i in range(n)])
        with pytest.raises(HtError):
            c.camshift_sequence_collect(n, 3)  # nothing pending
        got = c.camshift_track_sequence([dev.ptr] * 3, n, fetch="all")
        with pytest.raises(HtError):
            c.camshift_sequence_collect(n, 3, fetch="all")  # that sequence was fetched by the call itself
        c.camshift_init([(100 + 2 * i, 60, 90, 90) for i in range(n)])
        c.camshift_track_sequence([dev.ptr] * 3, n, fetch="none", keep_all=True)
        for bad in [(n - 1, 3, "all"), (n, 2, "all"), (n, 3, "last")]:
            with pytest.raises(HtError):
                c.camshift_sequence_collect(bad[0], bad[1], fetch=bad[2])
        assert c.camshift_sequence_collect(n, 3, fetch="all").tobytes() == got.tobytes()
        with pytest.raises(HtError):
            c.camshift_sequence_collect(n, 3, fetch="all")  # collected: no longer pending
    finally:
        c.close()
        dev.free()

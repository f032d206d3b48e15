"""Detect, pyramid, grouping, white balance, camshift and the list draw at the 16384-pixel limits of ht_set_geometry, against the oracle.

The geometries and frames are tests/limit_cases.py's: 16384 x 64, 16383 x 97, 65 x 16384 and 4099 x 2051 (with 16384 x 32 and 33 x 16384 for the
pyramid alone), the smallest frames on which the packed layouts are at their ends — tile records X0 | Y0 << 16, resample records bx / pass0
in 16 bits, queue entries x | y << 16 and two strides per word, ht_hit's 16-bit x and y, k_scan_simple's flat window index.
tests/test_limit_cases_cpu.py shows from the oracle alone that the inputs reach those ends: hits within 8 windows of the last window column
(x = 4087 of 4090) and of the first, planes 1 .. 3 pixels across and up to 1824 long, variant canvases on which nothing is drawn.

Every comparison is equality with the oracle, except camshift, which uses tests/test_gpu_camshift.py's check / assert_all_exact unchanged.

The 16384 x 16384 canvas itself is not run here: its arena is 1.5 GB per frame, the frames another 1 GB each, and the oracle needs about a
minute for it.  Its plan is pinned on the host (tests/test_limit_cases_cpu.py: the planner harness with its invariants, under ASan + UBSan)."""
import numpy as np
import pytest

import bp_cases
import draw_list_cases as dl
import limit_cases as lc
import yuv_cases as yc
from headtrackr_amd import distributed as hd
from headtrackr_amd.api import HT_INPUT_RGBA, HT_SCAN_NO_SPLIT, HT_SCAN_SIMPLE, Context
from headtrackr_amd.native import HT_DETECT_WHITEBALANCE, HT_SCAN_GENERIC, HT_SCAN_STATS
from oracle import ht_oracle as ho
from test_gpu_backproject import same
from test_gpu_camshift import SCHEDULES, assert_all_exact, check
from test_gpu_detect import assert_hits_equal
from test_gpu_draw_list import Resident
from test_gpu_ingest import bound_equals
from test_gpu_pyramid_ties import check_pyramid as check_pyramid_dims

pytestmark = pytest.mark.gpu

_CTX = {}


@pytest.fixture(scope="module")
def ctx_for():
    """one context per (options, queue capacity), closed when the module is done"""
    def get(options=None, queue_capacity=0):
        key = (options, queue_capacity)
        if key not in _CTX:
            _CTX[key] = Context(options=options, queue_capacity=queue_capacity)
        return _CTX[key]

    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------

def first_difference(got, want):
    y, x = (int(a[0]) for a in np.nonzero(got != want))
    return f"{int((got != want).sum())} bytes differ, first at x={x} y={y}: got {got[y, x]}, oracle {want[y, x]}"


def check_pyramid(c, name):
    """every (level, slot) plane of every frame against ho.pyramid / ho.plane, as tests/test_gpu_detect.py's _check_pyramid"""
    frames = lc.pyramid_frames(name)
    w, h = lc.SIZES[name]
    c.set_geometry(w, h, len(frames))
    c.upload(frames)
    c.detect_enqueue(HT_INPUT_RGBA)
    c.detect_collect()
    compared = 0
    for f, (levels, arena) in enumerate(lc.oracle_pyramid(name)):
        assert c.num_levels == len(levels)
        for i, (lw, lh, off) in enumerate(levels):
            for s in range(4):
                assert bool(c.plane(i, s).present) == (off[s] >= 0), (i, s)
                if off[s] < 0:
                    continue
                got = c.pyramid_readback(f, i, s)
                want = ho.plane(levels, arena, i, s)
                assert got.shape == want.shape, f"frame {f} level {i} slot {s}: {got.shape[::-1]} for {lw}x{lh}"
                assert np.array_equal(got, want), f"frame {f} level {i} slot {s} ({lw}x{lh}): {first_difference(got, want)}"
                compared += 1
    assert compared == 3 * 120


RS_OPTIONS = ["rs_bands=0", "rs_bands=0,rs_nofast=1", "rs_bands=1,rs_notail=1", "rs_bands=0,rs_rpt=2"]


@pytest.mark.parametrize("name", list(lc.SIZES))
def test_pyramid_planes_under_the_shipped_options(ctx_for, name):
    """all 120 canvases of an N, an S and an F frame on every limit geometry"""
    check_pyramid(ctx_for(), name)


@pytest.mark.parametrize("opts", RS_OPTIONS)
@pytest.mark.parametrize("name", list(lc.STRIPS) + list(lc.THIN))
def test_pyramid_planes_of_the_strips_under_each_generation_kernel(ctx_for, name, opts):
    """k_resample in place of k_resample_bands, binary64 everywhere, every generation through the kernel (no tail), two passes per tile: on the
    strips the HBM-tap path runs on full 64-column tiles and the undrawn variant canvases span a dozen to two dozen tile columns"""
    check_pyramid(ctx_for(opts), name)


@pytest.mark.parametrize("opts", ["rs_bands=1", "rs_bands=0"])
@pytest.mark.parametrize("name", lc.COPIES)
def test_a_level_of_the_frames_own_size_reaches_the_last_tile_column_and_pass(ctx_for, name, opts):
    """level_dims gives level 2 the frame's own size, so the resample tile records reach bx = 255 (wide) and pass0 = 1023 (tall) — at ccv's own
    sizes the largest destination is 14596 pixels, bx <= 228 and pass0 <= 912 — and level 8 halves the test's own bytes from there.  Against
    tests/pyramid_cases.py's numpy restatement, which takes the level sizes as an argument"""
    check_pyramid_dims(ctx_for(opts), f"limit_{name}_copy", lc.copy_case(name), own_dims=False)


# ---- raw hits -----------------------------------------------------------------------------------------------------------------------------

def check_hits(c, name, flags=0):
    frames = lc.face_frames(name)
    ref, counts, sp = lc.oracle_detect(name)
    hits, got_counts = c.detect_raw(frames, flags=flags | HT_SCAN_STATS)
    assert_hits_equal(hits, ref)
    assert [int(v) for v in got_counts] == counts
    assert np.array_equal(c.stage_counts().astype(np.int64), sp)
    assert c.windows_per_frame * len(frames) == sp[0]


@pytest.mark.parametrize("mode", [0, HT_SCAN_NO_SPLIT, HT_SCAN_SIMPLE, HT_SCAN_GENERIC, HT_SCAN_GENERIC | HT_SCAN_NO_SPLIT],
                         ids=["gen+deep", "gen-nosplit", "simple", "generic+deep", "generic-nosplit"])
@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_raw_hits_in_every_scan_schedule(ctx_for, name, mode):
    """two face frames (flat and smooth background, faces at both ends of the long axis): raw hits in the reference's order with the binary64
    sums, per-frame counts and the stage survival counters equal the oracle's"""
    check_hits(ctx_for(), name, mode)


@pytest.mark.parametrize("fp_sparse", [0, 1])
def test_sparse_stage_schedules_on_the_wide_frame(ctx_for, fp_sparse):
    check_hits(ctx_for(f"fp_sparse={fp_sparse}"), "wide")


def test_queue_overflow_far_from_the_origin(ctx_for):
    """a survivor queue of 8 entries on 16384 x 64: the tile kernel finishes the overflow itself, thousands of window columns from the origin"""
    check_hits(ctx_for(queue_capacity=8), "wide")


# ---- grouping -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_device_grouping_equals_the_host_route_and_the_oracle(ctx_for, name):
    """ht_detect_best_enqueue -> best records and ht_detect_grouped against ht_detect_collect + ht_hits_to_rects + ht_group_rects /
    ht_best_faces, byte for byte, and both against the oracle's grouped rects (x up to 16345 on the wide frames)"""
    c = ctx_for()
    frames = lc.face_frames(name)
    n = len(frames)
    want = lc.oracle_grouped(name)
    hits, counts = c.detect_raw(frames)
    host_best = c.best_faces(hits, counts, 1)
    host_lists, k = [], 0
    for cnt in counts:
        host_lists.append(c.group_rects(c.hits_to_rects(hits[k:k + int(cnt)]), 1))
        k += int(cnt)
    c.detect_enqueue()
    c.detect_best_enqueue(1, 0)
    best, total = c.detect_best_collect()
    best = best.copy()
    assert total == len(hits)
    for f in range(n):
        dev = c.detect_grouped(f)
        assert len(dev) == len(want[f]) > 0
        assert dev.tobytes() == host_lists[f].tobytes() == want[f].tobytes(), (name, f, dev, want[f])
        assert best[f].tobytes() == host_best[f].tobytes() == lc.select_best(want[f])[0].tobytes(), (name, f)
    ptr, nrec = c.detect_best_records_ptr()
    assert nrec == n and c.device_download(ptr, n * 64).tobytes() == hd.pack_best_records(host_best, 0).tobytes()


# ---- white balance ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_whitebalance_equals_the_channel_sums(ctx_for, name):
    """ht_whitebalance_batch and the sums fused into the gray pass (HT_DETECT_WHITEBALANCE) on an N, an S and an F frame: the channel sums
    divided as whitebalance.js divides them, in numpy"""
    c = ctx_for()
    frames = lc.pyramid_frames(name)
    want = [lc.whitebalance(f) for f in frames]
    assert len(set(want)) == len(frames)
    w, h = lc.GEOMETRIES[name]
    c.set_geometry(w, h, len(frames))
    c.upload(frames)
    assert [float(v) for v in c.whitebalance()] == want
    c.detect_enqueue(HT_DETECT_WHITEBALANCE)
    c.detect_collect()
    assert [float(v) for v in c.detect_whitebalance()] == want


# ---- camshift and back-projection -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(lc.CS_BLOBS))
def test_camshift_and_backprojection_at_the_far_edge(name, sched):
    """the shape of test_frame_sizes_and_chunking — two streams, 4 frames, every schedule — with the blob within 200 pixels of the far edge of
    16384 x 64 (x near 16250) and of 65 x 16384 (y near 16250); then getBackProjectionImg / getPdf of the last step"""
    w, h = lc.GEOMETRIES[name]
    seqs, rects = lc.cs_case(name)
    calls, models = lc.cs_oracle(name)
    n = lc.CS_STREAMS
    c = Context(options=SCHEDULES[sched])
    try:
        c.set_geometry(w, h, n)
        c.camshift_reserve(n)
        c.upload(np.stack([seqs[s][0] for s in range(n)]))
        c.camshift_init(rects)
        stats = []
        for k in range(1, lc.CS_STEPS):
            c.upload(np.stack([seqs[s][k] for s in range(n)]))
            got = c.camshift_track(n, calc_angles=True)
            for s in range(n):
                sw, to = calls[k - 1][s]
                check(got[s], sw, to, stats, where=(f"limit-{name}", s, k))
        assert_all_exact(stats, f"{w}x{h}")
        want = [bp_cases.expected(models[s], seqs[s][-1]) for s in range(n)]
        assert all(wr[..., 0].any() for wr, _ in want)
        same(c.camshift_backproject(n, kind="rgba8"), np.stack([wr for wr, _ in want]), f"{name}: getBackProjectionImg")
        same(c.camshift_backproject(n, kind="f64"), np.stack([wp for _, wp in want]), f"{name}: getPdf")
    finally:
        c.close()


# ---- draw onto a limit canvas ---------------------------------------------------------------------------------------------------------------

def test_draw_list_onto_the_wide_canvas():
    """one draw_list, bound form: a 333 x 217 NV12 source and a 23 x 23 RGBA source onto 16384 x 64 — 256 destination tile columns, upscales of
    49 and 712 times — read back through the stages that consume the bound frames"""
    w, h = lc.GEOMETRIES["wide"]
    srcs = [dl.Source(yc.NV12, 333, 217, seed=21, matrix=1, pad0=3, pad1=2), dl.Source(dl.RGBA, 23, 23, seed=22, pad0=4)]
    res = Resident(srcs)
    c = Context()
    try:
        c.set_geometry(w, h, len(srcs))
        c.draw_list([res.entry(k) for k in range(len(srcs))])
        want = np.stack([s.expected(None, w, h) for s in srcs])
        assert want.shape == (2, h, w, 4) and want[0, :, -64:].any() and want[1, :, -64:].any()
        bound_equals(c, want, "16384 x 64 canvas")
    finally:
        c.close()
        res.free()

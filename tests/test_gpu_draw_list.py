"""ht_draw_list_device (one launch draws a list of per-feed sources: separate allocations, sizes, formats, matrices and rects) against
tests/draw_list_cases.py: every entry's expectation is ingest_cases.expected / yuv_cases.expected, which the CPU suite pins to the
oracle's resampler and to the declared conversion.  Both are exact sequences of operations, so there is no tolerance: every comparison is
equality of every byte.  Without the feature every test here fails at its first call: the library has no ht_draw_list_device."""
import numpy as np
import pytest

import draw_list_cases as dl
import ingest_cases as ic
import yuv_cases as yc
from headtrackr_amd.api import Context, HtError
from hipmem import DeviceArray
from oracle import ht_oracle as ho
from test_gpu_ingest import bound_equals, d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_INVALID = -1
GUARD_BYTES = 64


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


class Resident:
    """sources in device memory, every plane in an allocation of its own"""

    def __init__(self, sources):
        self.sources = sources
        self.arrays = [[DeviceArray(b) for b in s.plane_buffers()] for s in sources]

    def entry(self, k, rect=None):
        return self.sources[k].entry([a.ptr for a in self.arrays[k]], rect)

    def free(self):
        for planes in self.arrays:
            for a in planes:
                a.free()


def expected_buffer(wants, dw, dh, dstride):
    """the whole destination: 0xA5 everywhere but in the frames, 64 guard bytes behind the last"""
    fb = dw * dh * 4
    buf = np.full(len(wants) * dstride + GUARD_BYTES, dl.GUARD, dtype=np.uint8)
    for i, w in enumerate(wants):
        buf[i * dstride:i * dstride + fb] = w.reshape(-1)
    return buf


def guarded(n, dw, dh, dstride):
    return DeviceArray(np.full(n * dstride + GUARD_BYTES, dl.GUARD, dtype=np.uint8))


def test_mixed_list_every_destination_byte(ctx):
    """seven entries on 97 x 81 (partial tiles in both directions), neighbours in different branches: RGBA, NV12, I420 (2 x 2: the single
    chroma column), NV12 odd x odd, RGBA one pixel wide, I420 under a rect with an odd origin, NV12 under a rect.  Every entry has its own
    allocations, size, pitch padding (0x5A) and matrix; the destination is strided and every byte of it is compared, the padding between
    the frames and the guard behind the last included."""
    dw, dh = 97, 81
    ctx.set_geometry(dw, dh, 2)  # the form into a caller's buffer is not limited by the batch capacity
    pairs = dl.mixed_sources()
    assert [s.fmt for s, _ in pairs] == [dl.RGBA, yc.NV12, yc.I420, yc.NV12, dl.RGBA, yc.I420, yc.NV12]
    res = Resident([s for s, _ in pairs])
    dstride = dw * dh * 4 + 52
    ddst = guarded(len(pairs), dw, dh, dstride)
    try:
        ctx.draw_list([res.entry(k, rect) for k, (_, rect) in enumerate(pairs)], dst=ddst.ptr, dst_stride=dstride)
        ctx.synchronize()
        got = d2h(ddst.ptr, ddst.nbytes)
    finally:
        res.free()
        ddst.free()
    wants = [s.expected(rect, dw, dh) for s, rect in pairs]
    fb = dw * dh * 4
    for i, w in enumerate(wants):  # per entry first: a failure names the entry
        same(got[i * dstride:i * dstride + fb].reshape(dh, dw, 4), w, f"entry {i} ({dl.FORMAT_NAMES[pairs[i][0].fmt]} {pairs[i][0].w}x{pairs[i][0].h} rect {pairs[i][1]})")
    same(got, expected_buffer(wants, dw, dh, dstride), "the whole destination")


def test_shared_sources_under_several_rects(ctx):
    """one 333 x 217 NV12 allocation in four entries under four rects and one RGBA allocation in two: equal pointers in different entries"""
    dw, dh = 97, 81
    ctx.set_geometry(dw, dh, 2)
    nv = dl.Source(yc.NV12, 333, 217, seed=21, matrix=1, pad0=3, pad1=2)
    rg = dl.Source(dl.RGBA, 333, 217, seed=22, pad0=4)
    rects = ic.rects_for(333, 217)
    plan = [(0, rects[0]), (1, None), (0, rects[5]), (0, rects[3]), (1, rects[9]), (0, rects[8])]  # rects[8]: one pixel wide; [5], [9]: odd origins
    res = Resident([nv, rg])
    fb = dw * dh * 4
    ddst = guarded(len(plan), dw, dh, fb)
    try:
        ctx.draw_list([res.entry(k, rect) for k, rect in plan], dst=ddst.ptr)
        ctx.synchronize()
        got = d2h(ddst.ptr, ddst.nbytes)
    finally:
        res.free()
        ddst.free()
    wants = [res.sources[k].expected(rect, dw, dh) for k, rect in plan]
    for i, w in enumerate(wants):
        same(got[i * fb:(i + 1) * fb].reshape(dh, dw, 4), w, f"entry {i} rect {plan[i][1]}")
    same(got, expected_buffer(wants, dw, dh, fb), "the whole destination")


def test_bind_form_feeds_the_pipeline():
    """dst NULL on 40 x 30, n = 3: the bound frames are the expectation (read through the pyramid, bound_equals), ht_frames_bound() == 3 and
    ht_whitebalance_batch on them gives the oracle's values on the expected canvases"""
    dw, dh, n = 40, 30, 3
    c = Context()
    srcs = dl.cycling_sources()
    res = Resident(srcs)
    try:
        c.set_geometry(dw, dh, n)
        plan = dl.cycling_list(9)[4:4 + n]
        c.draw_list([res.entry(k, rect) for k, rect in plan])
        want = np.stack([srcs[k].expected(rect, dw, dh) for k, rect in plan])
        assert c._lib.ht_frames_bound(c._h) == 3
        assert [float(v) for v in c.whitebalance()] == [ho.whitebalance(w) for w in want]
        bound_equals(c, want, "bound form")
    finally:
        c.close()
        res.free()


def test_two_calls_back_to_back_without_a_synchronise(ctx):
    """two calls with different lists into two destinations, nothing in between, then one ht_synchronize: the second call's table must not
    disturb the first call's, which is still queued"""
    dw, dh = 97, 81
    ctx.set_geometry(dw, dh, 2)
    srcs = dl.cycling_sources() + [dl.Source(yc.NV12, 1, 5, seed=51, matrix=1, content="raw"), dl.Source(dl.RGBA, 2, 2, seed=52)]
    res = Resident(srcs)
    rects = ic.rects_for(23, 23)
    lists = [[(0, None), (1, rects[4]), (6, None), (2, rects[5])], [(5, rects[11]), (7, None), (3, None), (4, rects[1]), (1, None)]]
    fb = dw * dh * 4
    dsts = [guarded(len(lst), dw, dh, fb) for lst in lists]
    try:
        for lst, d in zip(lists, dsts):
            ctx.draw_list([res.entry(k, rect) for k, rect in lst], dst=d.ptr)
        ctx.synchronize()
        got = [d2h(d.ptr, d.nbytes) for d in dsts]
    finally:
        res.free()
        for d in dsts:
            d.free()
    for j, lst in enumerate(lists):
        same(got[j], expected_buffer([srcs[k].expected(rect, dw, dh) for k, rect in lst], dw, dh, fb), f"call {j}")


@pytest.mark.parametrize("n", [1, 40])
def test_short_and_long_lists(ctx, n):
    """n = 1 and n = 40 on 40 x 30 from 23 x 23 sources, cycling the formats: 40 entries are more than any table passed in the kernel
    arguments could hold (the library has one route, the staged table, at every n)"""
    dw, dh = 40, 30
    ctx.set_geometry(dw, dh, 2)
    srcs = dl.cycling_sources()
    res = Resident(srcs)
    plan = dl.cycling_list(n)
    fb = dw * dh * 4
    ddst = guarded(n, dw, dh, fb)
    try:
        ctx.draw_list([res.entry(k, rect) for k, rect in plan], dst=ddst.ptr)
        ctx.synchronize()
        got = d2h(ddst.ptr, ddst.nbytes)
    finally:
        res.free()
        ddst.free()
    wants = [srcs[k].expected(rect, dw, dh) for k, rect in plan]
    for i, w in enumerate(wants):
        same(got[i * fb:(i + 1) * fb].reshape(dh, dw, 4), w, f"entry {i} of {n}")
    same(got, expected_buffer(wants, dw, dh, fb), "the whole destination")


def test_refusals_name_the_entry_and_write_nothing():
    """overlap with the destination, an odd NV12 chroma base, a rect outside its source at entry 5 of 7, n above max_batch in the bind
    form: HT_ERR_INVALID, the entry's index in ht_last_error, the destination still all 0xA5 and the binding as it was"""
    dw, dh = 40, 30
    pairs = dl.mixed_sources()
    res = Resident([s for s, _ in pairs])
    fb = dw * dh * 4
    ddst = guarded(len(pairs), dw, dh, fb)
    c = Context()
    try:
        c.set_geometry(dw, dh, 3)
        c.upload(np.stack([ic.noise(dw, dh, 60 + k) for k in range(2)]))
        good = [res.entry(k, rect) for k, (_, rect) in enumerate(pairs)]

        def refused(entries, index, dst=ddst.ptr):
            with pytest.raises(HtError) as e:
                c.draw_list(entries, dst=dst)
            assert e.value.status == HT_ERR_INVALID, str(e.value)
            assert f"entry {index}:" in str(e.value), (index, str(e.value))
            c.synchronize()
            assert (d2h(ddst.ptr, ddst.nbytes) == dl.GUARD).all(), index
            assert c._lib.ht_frames_bound(c._h) == 2, index

        bad = [dict(e) for e in good]
        bad[3]["p1"] = ddst.ptr + 2 * fb + 16                      # entry 3's chroma plane lies inside destination frame 2
        refused(bad, 3)
        bad = [dict(e) for e in good]
        bad[6]["p0"] = ddst.ptr + len(pairs) * fb - 1               # entry 6's Y plane begins at the destination's last byte
        refused(bad, 6)
        bad = [dict(e) for e in good]
        bad[1]["p1"] += 1                                           # odd NV12 chroma base
        refused(bad, 1)
        bad = [dict(e) for e in good]
        bad[5]["rect"] = (10, 0, pairs[5][0].w - 9, pairs[5][0].h)  # one column beyond the right edge, at entry 5 of 7
        refused(bad, 5)
        refused(good[:4], 3, dst=None)                              # four entries, max_batch 3: entry 3 is the first without a frame
        c.draw_list(good, dst=ddst.ptr)                             # ... and the same context draws the good list afterwards
        c.synchronize()
        same(d2h(ddst.ptr, ddst.nbytes), expected_buffer([s.expected(rect, dw, dh) for s, rect in pairs], dw, dh, fb), "after the refusals")
    finally:
        c.close()
        res.free()
        ddst.free()


def test_node_facade_draws_a_list_on_the_device(tmp_path):
    """tests/js/draw_list_gpu.js on the real addon: a ccv.DeviceBatch with mixed opts.sources (NV12 odd x odd, RGBA under a rect, I420 under a
    rect with an odd origin); drawList into a frame set and drawListBound, each followed by whitebalance and detectStep, equal the same steps
    on the numpy canvases uploaded directly"""
    import json
    import os
    import shutil
    import subprocess

    from conftest import ROOT
    from headtrackr_amd import build

    if shutil.which("node") is None or build.build_addon() is None:
        pytest.skip("node or the N-API headers are missing on this machine")
    dw, dh = 160, 120
    srcs = [dl.Source(yc.NV12, 333, 217, seed=71, matrix=1, content="smooth"), dl.Source(dl.RGBA, 320, 240, seed=72, content="smooth"),
            dl.Source(yc.I420, 23, 23, seed=73, matrix=2)]
    rects = [None, (21, 13, 280, 190), (1, 1, 21, 21)]
    job = dict(w=dw, h=dh, dir=str(tmp_path), feeds=[])
    for k, (s, rect) in enumerate(zip(srcs, rects)):
        s.packed().tofile(tmp_path / f"feed{k}.raw")
        want = s.expected(rect, dw, dh)
        want.tofile(tmp_path / f"want{k}.raw")
        job["feeds"].append(dict(file=f"feed{k}.raw", want=f"want{k}.raw", width=s.w, height=s.h, format=dl.FORMAT_NAMES[s.fmt], matrix=yc.MATRIX_NAMES[s.matrix],
                                 rect=list(rect) if rect else None, wb=ho.whitebalance(want)))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run(["node", os.path.join(ROOT, "tests", "js", "draw_list_gpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "draw_list_gpu: ok" in r.stdout, r.stdout[-2000:]

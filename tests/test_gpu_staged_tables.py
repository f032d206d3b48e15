"""The staged tables under the list calls (HtStagedTable, ht_internal.h) on the two paths no other test reaches: more calls in flight than
the table has pinned slots (the ring is reused), and a list longer than the table's first capacity of 64 entries (the table, the slots and
the records are reallocated behind a call that is still queued).  For ht_camshift_crop_pairs_device, ht_camshift_align_pairs_device and
ht_draw_list_device; the camshift pair table has tests/test_gpu_camshift_pairs.py and tests/test_gpu_cs_pairs_cluster.py, which make many
pair calls per context.

The inputs are the existing ones — crop_cases' 97 x 81 canvas and pairs scene, draw_list_cases' cycling sources — and everything expected
comes from those modules' oracle-backed helpers, never from the library.  Every comparison is equality: the whole strided buffer with its
guard bytes, and the records bit for bit."""
import functools

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_list_cases as dl
from headtrackr_amd import native
from headtrackr_amd.api import Context, HtError
from test_gpu_align import objects_agree
from test_gpu_align import record_tuples as align_tuples
from test_gpu_crop import CROP_LIST, canvas_source, expected_buffer, guarded, oracle_step, start_pairs
from test_gpu_crop import record_tuples as crop_tuples
from test_gpu_draw_list import Resident
from test_gpu_draw_list import expected_buffer as canvas_buffer
from test_gpu_ingest import d2h, same

pytestmark = pytest.mark.gpu

HT_ERR_STATE = -6
W, H = cr.CANVAS
SLOTS = 4          # HT_STAGE_SLOTS (ht_stage_plan.h)
FIRST_CAPACITY = 64  # entries a list table holds after its first call


class Family:
    """one of the two face-patch families: its calls on a Context and its expectation, memoised per distinct (stream, frame) of a list"""

    def __init__(self, name, objs, sources):
        self.name, self.objs, self.sources = name, objs, sources
        self.crop = name == "crop"
        self.rec_dtype = native.CROP_RECORD_DTYPE if self.crop else native.ALIGN_RECORD_DTYPE
        self.tuples = crop_tuples if self.crop else align_tuples
        self.entry = functools.lru_cache(maxsize=None)(self._entry)

    def call(self, c, out, pairs, P, Q, margin, flags, stride):
        fn = c.camshift_crop_pairs_device if self.crop else c.camshift_align_pairs_device
        fn(out.ptr, pairs, P, Q, margin=margin / 256, square=bool(flags), stride=stride)

    def result(self, c, n):
        return (c.camshift_crop_result if self.crop else c.camshift_align_result)(n)

    def records_ptr(self, c):
        return (c.camshift_crop_records_ptr if self.crop else c.camshift_align_records_ptr)()

    def _entry(self, s, f, P, Q, margin, flags):
        """(patch, record) of entry (stream s, bound frame f)"""
        if self.crop:
            o = cr.obj_of(self.objs[s]) if s in self.objs else (0.0, 0.0, 0.0, 0.0)
            return cr.patch(self.sources[f], o, W, H, None, margin, flags, P, Q), cr.record(s, o, W, H, W, H, None, margin, flags, P, Q)
        o = al.obj_of(self.objs[s]) if s in self.objs else al.NO_OBJECT
        return al.patch(self.sources[f], o, W, H, None, margin, flags, P, Q), al.record(s, o, W, H, W, H, None, margin, flags)

    def expected(self, pairs, P, Q, margin, flags, stride):
        """(the whole strided output with its guard, the records) of one call"""
        got = [self.entry(s, f, P, Q, margin, flags) for s, f in pairs]
        return expected_buffer([p for p, _r in got], stride), [r for _p, r in got]


@pytest.fixture(scope="module")
def scene():
    """the oracle's step-1 objects of the pairs scene and the two bound canvases as sources; `fresh()` makes a context that has tracked
    that step and has never made a crop or an align call"""
    a, b = cr.pairs_scene()
    want = oracle_step(1)
    sources = [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
    made = []

    def fresh():
        c = Context()
        made.append(c)
        c.set_geometry(W, H, 2)
        c.upload(np.stack([a.frames[0], b.frames[0]]))
        pairs = start_pairs(c)
        c.upload(np.stack([a.frames[1], b.frames[1]]))
        objects_agree(c.camshift_track_pairs(pairs), [want[s] for s, _f in pairs], "pairs scene, step 1")
        return c

    yield {name: Family(name, want, sources) for name in ("crop", "align")}, fresh
    for c in made:
        c.close()


def rotated(lst, k):
    return lst[k % len(lst):] + lst[:k % len(lst)]


@pytest.mark.parametrize("name", ["crop", "align"])
def test_six_calls_in_flight_reuse_the_ring_of_four_slots(scene, name):
    """six pairs calls back to back with no synchronise in between, each with another rotation of the crop list, another config and a
    buffer of its own, 1 x 1 patches (short kernels: a slot written before its copy had left it would be caught): every output whole, and
    the records of the last call"""
    families, fresh = scene
    fam, c = families[name], fresh()
    calls = SLOTS + 2
    stride = 4 + 12
    lists = [rotated(CROP_LIST, k) for k in range(calls)]
    assert len({tuple(lst) for lst in lists}) == calls
    outs = [guarded(len(lst), stride) for lst in lists]
    try:
        for k, (lst, out) in enumerate(zip(lists, outs)):
            fam.call(c, out, lst, 1, 1, *cr.CONFIGS[k], stride)
        rec = fam.result(c, len(lists[-1]))  # waits for the last call only
        c.synchronize()
        got = [d2h(o.ptr, o.nbytes) for o in outs]
    finally:
        for o in outs:
            o.free()
    for k, lst in enumerate(lists):
        want, want_rec = fam.expected(lst, 1, 1, *cr.CONFIGS[k], stride)
        same(got[k], want, f"{name} call {k} of {calls}")
    assert fam.tuples(rec) == want_rec, (fam.tuples(rec), want_rec)


@pytest.mark.parametrize("size", [(1, 1), (70, 19)])
@pytest.mark.parametrize("name", ["crop", "align"])
def test_a_list_beyond_the_first_capacity_grows_the_table_and_the_records(scene, name, size):
    """a fresh context refuses result and records-device with HT_ERR_STATE; then 3 entries, 65 entries (the first capacity is 64: table,
    slots and records are reallocated) and 3 entries again, nothing synchronised by the test in between: every call's whole output, its
    records from the pinned twin and the last call's from the device"""
    families, fresh = scene
    fam, c = families[name], fresh()
    P, Q = size
    for refused in (lambda: fam.result(c, 3), lambda: fam.records_ptr(c)):
        with pytest.raises(HtError) as e:
            refused()
        assert e.value.status == HT_ERR_STATE, str(e.value)
    stride = P * Q * 4 + 52
    long_list = [CROP_LIST[i % len(CROP_LIST)] for i in range(FIRST_CAPACITY + 1)]
    lists = [CROP_LIST[:3], long_list, CROP_LIST[3:]]
    outs = [guarded(len(lst), stride) for lst in lists]
    recs = []
    try:
        for k, (lst, out) in enumerate(zip(lists, outs)):
            fam.call(c, out, lst, P, Q, *cr.CONFIGS[k + 1], stride)
            recs.append(fam.result(c, len(lst)))
        ptr, cnt = fam.records_ptr(c)
        c.synchronize()
        got = [d2h(o.ptr, o.nbytes) for o in outs]
        dev = np.frombuffer(d2h(ptr, cnt * fam.rec_dtype.itemsize).tobytes(), dtype=fam.rec_dtype)
    finally:
        for o in outs:
            o.free()
    for k, lst in enumerate(lists):
        want, want_rec = fam.expected(lst, P, Q, *cr.CONFIGS[k + 1], stride)
        same(got[k], want, f"{name} {P}x{Q} call {k}: {len(lst)} entries")
        assert fam.tuples(recs[k]) == want_rec, (k, len(lst))
    assert cnt == 3 and fam.tuples(dev) == want_rec


# ---- the draw list ------------------------------------------------------------------------------------------------------------------------

DW, DH = 40, 30  # the smallest canvas of tests/test_gpu_draw_list.py


@pytest.fixture(scope="module")
def feeds():
    """draw_list_cases' cycling sources in device memory, and the expectation of an entry, memoised"""
    srcs = dl.cycling_sources()
    res = Resident(srcs)
    want = functools.lru_cache(maxsize=None)(lambda k, rect: srcs[k].expected(rect, DW, DH))
    yield res, want
    res.free()


def draw_and_compare(c, res, want, lists):
    fb = DW * DH * 4
    dsts = [guarded(len(lst), fb) for lst in lists]
    try:
        for lst, d in zip(lists, dsts):
            c.draw_list([res.entry(k, rect) for k, rect in lst], dst=d.ptr)
        c.synchronize()
        got = [d2h(d.ptr, d.nbytes) for d in dsts]
    finally:
        for d in dsts:
            d.free()
    for j, lst in enumerate(lists):
        same(got[j], canvas_buffer([want(k, rect) for k, rect in lst], DW, DH, fb), f"call {j}: {len(lst)} entries")


def test_six_draw_lists_in_flight_reuse_the_ring_of_four_slots(feeds):
    """six calls with six rotations of a seven-entry list into six destinations, one synchronise at the end"""
    res, want = feeds
    base = dl.cycling_list(7)
    lists = [rotated(base, k) for k in range(SLOTS + 2)]
    assert len({tuple(lst) for lst in lists}) == SLOTS + 2
    c = Context()
    try:
        c.set_geometry(DW, DH, 2)
        draw_and_compare(c, res, want, lists)
    finally:
        c.close()


def test_a_draw_list_beyond_the_first_capacity_grows_the_table(feeds):
    """a fresh context: 3 entries, 65 entries (the first capacity is 64) and 3 entries again, one synchronise at the end"""
    res, want = feeds
    base = dl.cycling_list(7)
    lists = [base[:3], [base[i % 7] for i in range(FIRST_CAPACITY + 1)], base[4:]]
    c = Context()
    try:
        c.set_geometry(DW, DH, 2)
        draw_and_compare(c, res, want, lists)
    finally:
        c.close()

"""The prefiltered face crops on the device — ht_camshift_crop_pairs_filtered_device / ht_camshift_crop_sources_filtered_device /
ht_camshift_align_pairs_filtered_device / ht_camshift_align_sources_filtered_device — against tests/filter_cases.py.  The track objects are
the ORACLE's, the fine patch is the Python restatement of the unfiltered crop / align rule (tests/crop_cases.py, tests/align_cases.py) at
Nx * P x Ny * Q, the output its integer block mean, the tensor the restated f of that: nothing expected comes from the code under test, and
every comparison is equality of every byte, padding and the 64-byte guard included.  The structural tests compare the filtered calls with
the EXISTING kernels on the same tracker state.  Without the feature every test fails at its first filtered call."""
import ctypes as C
import functools

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_list_cases as dl
import filter_cases as fc
import patch_tensor_cases as pt
from headtrackr_amd import api, native
from headtrackr_amd.api import Context, HtError, PatchFormat
from test_gpu_align import objects_agree
from test_gpu_crop import CROP_LIST, ResidentFeeds, canvas_source, expected_buffer, guarded, oracle_step, start_pairs
from test_gpu_ingest import d2h, same
from test_gpu_patch_tensor import KINDS, NO_BOX, fmt_of, pairs_ctx  # noqa: F401  (pairs_ctx: the module-scoped fixture, one instance for this module)

pytestmark = pytest.mark.gpu

HT_ERR_INVALID, HT_ERR_STATE = -1, -6
W, H = cr.CANVAS
TENSOR_FORMATS = ((("f32", "chw", "rgb"), "imagenet"), (("f16", "hwc", "bgr"), "signed"), (("bf16", "chw", "gray"), "unit"))
FEED_STREAMS = [4, 0, 6, 2, 8, 1, 5]


def filtered_pairs(kind, c, ptr, pairs, P, Q, mf, margin, flags, fmt=None, stride=0):
    fn = c.camshift_crop_pairs_filtered_device if kind == "crop" else c.camshift_align_pairs_filtered_device
    fn(ptr, pairs, P, Q, max_factor=mf, fmt=fmt, margin=margin / 256, square=bool(flags), stride=stride)


def filtered_sources(kind, c, ptr, streams, entries, P, Q, mf, margin, flags, fmt=None, stride=0):
    fn = c.camshift_crop_sources_filtered_device if kind == "crop" else c.camshift_align_sources_filtered_device
    fn(ptr, streams, entries, P, Q, max_factor=mf, fmt=fmt, margin=margin / 256, square=bool(flags), stride=stride)


def exported_factors(kind, rec, P, Q, mf):
    """the library's own factor functions on the call's records"""
    return [tuple(int(v) for v in row) for row in (api.crop_filter_factors if kind == "crop" else api.align_filter_factors)(rec, P, Q, mf)]


class Restated:
    """the restatement's filtered patches, each fine patch computed once (max_factor 8 and 3 share most of them)"""

    def __init__(self):
        self.fine = functools.lru_cache(maxsize=None)(self._fine)
        self.sources = {}

    def _fine(self, kind, key, obj, mapping, margin, flags, Pf, Qf):
        return (cr.patch if kind == "crop" else al.patch)(self.sources[key], obj, W, H, mapping, margin, flags, Pf, Qf)

    def patch(self, kind, key, source, obj, mapping, margin, flags, P, Q, mf):
        """(patch, (Nx, Ny)); key names the source"""
        self.sources[key] = source
        if kind == "crop":
            code, rect = cr.rule(obj, W, H, source.w, source.h, mapping, margin, flags)
            nx, ny = fc.crop_factors(code, rect, P, Q, mf)
        else:
            nx, ny = fc.align_factors(al.plan(obj, W, H, source.w, source.h, mapping, margin, flags), P, Q, mf)
        if (nx, ny) == (0, 0):
            return np.zeros((Q, P, 4), dtype=np.uint8), (0, 0)
        return fc.block_mean(self.fine(kind, key, obj, mapping, margin, flags, nx * P, ny * Q), nx, ny), (nx, ny)


@pytest.fixture(scope="module")
def restated():
    return Restated()


@pytest.fixture(scope="module")
def feeds_ctx():
    """one context that has drawn, initialised and tracked crop_cases.feeds(); every sources-form test reads it"""
    feeds, objs = cr.feeds(), cr.feed_objects()
    n = len(feeds)
    res = ResidentFeeds()
    c = Context()
    c.set_geometry(W, H, n)
    c.draw_list(res.entries())
    c.camshift_reserve(9)
    pairs = [(FEED_STREAMS[i], i) for i in range(n)]
    c.camshift_init_pairs(pairs, [cr.canvas_rect_of(i) for i in range(n)])
    tracked = c.camshift_track_pairs(pairs)
    objects_agree(tracked, objs, "feeds")
    yield c, res, objs, tracked
    c.close()
    res.free()


def pairs_objects(kind, objs):
    return [KINDS[kind].obj(objs.get(s)) for s, _f in CROP_LIST]


# ---- 1: the pairs form ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", fc.SIZES)
@pytest.mark.parametrize("kind", ["crop", "align"])
def test_pairs_form_every_byte_and_every_record(pairs_ctx, restated, kind, size):
    """the 97 x 81 pairs scene and CROP_LIST (FACE entries, both EMPTY kinds, one stream twice) -> 70 x 19, 1 x 1, 112 x 112, 16 x 7 and 3 x 4; every
    margin, square on and off; max_factor 8, 3 and 2 (either tile of the kernels); a strided output (a patch + 52 bytes).  Expected: the block mean of the restated fine
    patch; the records are the UNFILTERED call's restated records; the exported factor functions give the restated factors"""
    c, objs, sources = pairs_ctx
    k = KINDS[kind]
    P, Q = size
    n, pb = len(CROP_LIST), P * Q * 4
    stride = pb + 52
    obj = pairs_objects(kind, objs)
    seen = set()
    for (margin, flags) in cr.CONFIGS:
        want_rec = [k.record(s, o, W, H, None, margin, flags, P, Q) for o, (s, _f) in zip(obj, CROP_LIST)]
        for mf in fc.MAX_FACTORS:
            both = [restated.patch(kind, ("pairs", f), sources[f], o, None, margin, flags, P, Q, mf) for o, (_s, f) in zip(obj, CROP_LIST)]
            patches, factors = [p for p, _ in both], [f for _, f in both]
            out = guarded(n, stride)
            try:
                filtered_pairs(kind, c, out.ptr, CROP_LIST, P, Q, mf, margin, flags, stride=stride)
                rec = k.result(c, n)
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            where = f"{kind} margin {margin} flags {flags} max_factor {mf} -> {P}x{Q}"
            for i, p in enumerate(patches):  # per entry first: a failure names the entry
                same(got[i * stride:i * stride + pb].reshape(Q, P, 4), p, f"entry {i} {CROP_LIST[i]} factors {factors[i]} {where}")
            same(got, expected_buffer(patches, stride), f"the whole output, {where}")
            assert k.tuples(rec) == want_rec, where
            assert exported_factors(kind, rec, P, Q, mf) == factors, where
            assert [f == (0, 0) for f in factors] == [False, True, False, False, True, False]
            seen |= set(factors)
    assert (0, 0) in seen and len(seen) >= 2
    assert (kind, P, Q) != ("crop", 112, 112) or seen == {(0, 0), (1, 1)}  # the canvas is smaller than the patch: the unfiltered bytes
    assert (P, Q) != (1, 1) or (8, 8) in seen and (3, 3) in seen  # limited by max_factor either way


# ---- 2: the sources form -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_sources_form_from_a_mixed_list(feeds_ctx, restated, kind):
    """crop_cases.feeds() — padded RGBA 333 x 217, NV12 under an odd-origin rect, I420 23 x 23 upscaled, the 1 x 5 strips, every matrix —:
    every size, every margin, square on and off; max_factor 8, and 3 and 2 (either side of the tile threshold) at 16 x 7.  The YUV taps are converted before they are blended and
    averaged; the strips have no tap pair"""
    c, res, objs, tracked = feeds_ctx
    k = KINDS[kind]
    feeds = cr.feeds()
    n = len(feeds)
    obj = [k.obj(to, float(g["angle"])) for to, g in zip(objs, tracked)]
    seen = set()
    for (P, Q, margin, flags, mf) in [(P, Q, m, fl, 8) for (P, Q) in fc.SIZES for (m, fl) in cr.CONFIGS] + [(16, 7, m, fl, mf) for (m, fl) in cr.CONFIGS for mf in (3, 2)]:
        pb = P * Q * 4
        both = [restated.patch(kind, ("feed", i), src, o, m, margin, flags, P, Q, mf) for i, ((src, m), o) in enumerate(zip(feeds, obj))]
        patches, factors = [p for p, _ in both], [f for _, f in both]
        want_rec = [k.record(st, o, src.w, src.h, m, margin, flags, P, Q) for (src, m), o, st in zip(feeds, obj, FEED_STREAMS)]
        out = guarded(n, pb)
        try:
            filtered_sources(kind, c, out.ptr, FEED_STREAMS, res.entries(), P, Q, mf, margin, flags)
            rec = k.result(c, n)
            c.synchronize()
            got = d2h(out.ptr, out.nbytes)
        finally:
            out.free()
        where = f"{kind} margin {margin} flags {flags} max_factor {mf} -> {P}x{Q}"
        for i, p in enumerate(patches):
            same(got[i * pb:(i + 1) * pb].reshape(Q, P, 4), p, f"feed {i} ({dl.FORMAT_NAMES[feeds[i][0].fmt]} {feeds[i][0].w}x{feeds[i][0].h}) factors {factors[i]} {where}")
        same(got, expected_buffer(patches, pb), f"the whole output, {where}")
        assert k.tuples(rec) == want_rec, where
        assert exported_factors(kind, rec, P, Q, mf) == factors, where
        seen |= {(feeds[i][0].fmt, f) for i, f in enumerate(factors)}
    # every format was averaged over a real block, and some entry of every format kept factor 1 on an axis
    for fmt in {s.fmt for s, _ in feeds}:
        assert any(f[0] * f[1] > 1 for g, f in seen if g == fmt), (fmt, seen)


# ---- 3: max_factor 1, and boxes that are not downscaled, are the unfiltered call ----------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_max_factor_1_is_the_unfiltered_call_byte_for_byte(pairs_ctx, feeds_ctx, kind):
    """both on the device, on the same tracker state: the same patches, the same records — pairs and sources form, RGBA8 and f16 CHW"""
    k = KINDS[kind]
    c, _objs, _sources = pairs_ctx
    fmt = PatchFormat.mean_std(pt.IMAGENET_MEAN, pt.IMAGENET_STD)
    n = len(CROP_LIST)
    for (P, Q, margin, flags) in ((70, 19, 1024, cr.SQUARE), (16, 7, 256, 0), (1, 1, 64, 0)):
        for f in (None, fmt):
            nbytes = P * Q * 4 if f is None else f.default_stride(P, Q)
            a, b = guarded(n, nbytes), guarded(n, nbytes)
            try:
                if f is None:
                    k.rgba_pairs(c, a.ptr, CROP_LIST, P, Q, margin, flags)
                else:
                    k.tensor_pairs(c, a.ptr, CROP_LIST, P, Q, f, margin, flags)
                ra = k.result(c, n).tobytes()
                filtered_pairs(kind, c, b.ptr, CROP_LIST, P, Q, 1, margin, flags, fmt=f)
                rb = k.result(c, n).tobytes()
                c.synchronize()
                ga, gb = d2h(a.ptr, a.nbytes), d2h(b.ptr, b.nbytes)
            finally:
                a.free()
                b.free()
            assert ga.any() and ra == rb
            same(gb, ga, f"{kind} pairs {P}x{Q} margin {margin} flags {flags} {'rgba' if f is None else 'f16'}")
    c, res, _o, _t = feeds_ctx
    n = len(cr.feeds())
    for (P, Q, margin, flags) in ((16, 7, 1024, cr.SQUARE), (70, 19, 256, 0)):
        a, b = guarded(n, P * Q * 4), guarded(n, P * Q * 4)
        try:
            k.rgba_sources(c, a.ptr, FEED_STREAMS, res.entries(), P, Q, margin, flags)
            ra = k.result(c, n).tobytes()
            filtered_sources(kind, c, b.ptr, FEED_STREAMS, res.entries(), P, Q, 1, margin, flags)
            rb = k.result(c, n).tobytes()
            c.synchronize()
            ga, gb = d2h(a.ptr, a.nbytes), d2h(b.ptr, b.nbytes)
        finally:
            a.free()
            b.free()
        assert ra == rb
        same(gb, ga, f"{kind} sources {P}x{Q} margin {margin} flags {flags}")


# ---- 4: against the existing kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_filtered_patch_is_the_block_mean_of_the_existing_kernels_fine_patch(pairs_ctx, feeds_ctx, kind):
    """single-entry lists: the EXISTING call at Nx * P x Ny * Q (<= 1024), downloaded, and its block mean computed on the host, equals the
    filtered call's patch.  The factors are the exported functions' on the call's own record.  Every FACE entry of the pairs list and
    every feed (RGBA, NV12, I420, the strips)"""
    k = KINDS[kind]
    seen = set()

    def one(c, call_filtered, call_plain, P, Q, mf, where):
        out = guarded(1, P * Q * 4)
        try:
            call_filtered(out.ptr, P, Q, mf)
            rec = k.result(c, 1)
            c.synchronize()
            got = d2h(out.ptr, P * Q * 4).reshape(Q, P, 4)
        finally:
            out.free()
        (nx, ny), = exported_factors(kind, rec, P, Q, mf)
        if (nx, ny) == (0, 0):
            assert not got.any(), where
            return
        assert nx * P <= 1024 and ny * Q <= 1024
        fine = guarded(1, nx * P * ny * Q * 4)
        try:
            call_plain(fine.ptr, nx * P, ny * Q)
            c.synchronize()
            f = d2h(fine.ptr, nx * P * ny * Q * 4).reshape(ny * Q, nx * P, 4)
        finally:
            fine.free()
        same(got, fc.block_mean(f, nx, ny), f"{where} factors {(nx, ny)}")
        seen.add((nx, ny))

    c, _objs, _sources = pairs_ctx
    for pair in [(5, 0), (0, 0), (2, 1), (cr.NEVER_TRACKED, 1)]:
        for (P, Q, margin, flags, mf) in ((16, 7, 256, 0, 8), (16, 7, 1024, cr.SQUARE, 8), (70, 19, 1024, 0, 3), (1, 1, 1024, 0, 8)):
            one(c, lambda ptr, p, q, m: filtered_pairs(kind, c, ptr, [pair], p, q, m, margin, flags), lambda ptr, p, q: k.rgba_pairs(c, ptr, [pair], p, q, margin, flags),
                P, Q, mf, f"{kind} pair {pair} margin {margin} flags {flags} max_factor {mf} -> {P}x{Q}")
    c, res, _o, _t = feeds_ctx
    for i in range(len(cr.feeds())):
        st, en = [FEED_STREAMS[i]], [res.entry(i)]
        for (P, Q, margin, flags, mf) in ((16, 7, 1024, cr.SQUARE, 8), (70, 19, 256, 0, 8)):
            one(c, lambda ptr, p, q, m: filtered_sources(kind, c, ptr, st, en, p, q, m, margin, flags), lambda ptr, p, q: k.rgba_sources(c, ptr, st, en, p, q, margin, flags),
                P, Q, mf, f"{kind} feed {i} margin {margin} flags {flags} -> {P}x{Q}")
    assert len(seen) >= 4 and any(nx != ny for nx, ny in seen) and (8, 8) in seen


# ---- 5: the tensor form ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["crop", "align"])
def test_tensor_form_is_f_of_the_filtered_rgba_bytes(pairs_ctx, restated, kind):
    """f32 CHW RGB, f16 HWC BGR and bf16 CHW gray of the pairs list at 16 x 7 (margin 4, square) and 70 x 19: f, in numpy, of the filtered RGBA
    bytes of the same call sequence — which are the restatement's —; gray is taken from the filtered R, G, B; empty entries are bias[c]"""
    c, objs, sources = pairs_ctx
    k = KINDS[kind]
    n = len(CROP_LIST)
    obj = pairs_objects(kind, objs)
    for (P, Q, margin, flags, mf) in ((16, 7, 1024, cr.SQUARE, 8), (70, 19, 256, 0, 3)):
        rgba = guarded(n, P * Q * 4)
        try:
            filtered_pairs(kind, c, rgba.ptr, CROP_LIST, P, Q, mf, margin, flags)
            rgba_rec = k.result(c, n).tobytes()
            c.synchronize()
            patches = d2h(rgba.ptr, n * P * Q * 4).reshape(n, Q, P, 4)
        finally:
            rgba.free()
        want_patches = [restated.patch(kind, ("pairs", f), sources[f], o, None, margin, flags, P, Q, mf)[0] for o, (_s, f) in zip(obj, CROP_LIST)]
        same(patches, np.stack(want_patches), f"{kind} filtered RGBA {P}x{Q}")
        for fmt, name in TENSOR_FORMATS:
            pair = pt.pair_for(name, fmt[2])
            pb, stride = pt.patch_bytes(P, Q, fmt[0], fmt[2]), pt.default_stride(P, Q, fmt[0], fmt[2]) + 8
            out = guarded(n, stride)
            try:
                filtered_pairs(kind, c, out.ptr, CROP_LIST, P, Q, mf, margin, flags, fmt=fmt_of(fmt, pair), stride=stride)
                rec = k.result(c, n).tobytes()
                c.synchronize()
                got = d2h(out.ptr, out.nbytes)
            finally:
                out.free()
            want = [pt.f(p, fmt, pair) for p in patches]
            same(got, expected_buffer(want, stride), f"{kind} {fmt} {P}x{Q}")
            assert rec == rgba_rec
            for i in (1, 4):  # the two EMPTY entries: bias[c] in the dtype, everywhere
                same(got[i * stride:i * stride + pb], pt.f(np.zeros((Q, P, 4), dtype=np.uint8), fmt, pair), f"empty entry {i} {fmt}")


# ---- 6: a filtered call leaves everything else as it is ----------------------------------------------------------------------------------------

def test_filtered_calls_leave_the_trackers_and_the_unfiltered_calls_of_the_same_step_as_they_are():
    """a twin context without filtered calls returns the same track objects, histograms and statistics on the following step — the oracle's —,
    and the crop call and the align call of the same step, issued among the filtered calls, give the bytes and records they give alone;
    crop_result / align_result report on a filtered call issued last"""
    a, b = cr.pairs_scene()
    res = ResidentFeeds()
    ctxs = [Context(), Context()]
    n = len(CROP_LIST)
    pb = 70 * 19 * 4
    fmt = PatchFormat.mean_std(pt.IMAGENET_MEAN, pt.IMAGENET_STD)
    outs = [guarded(n + 1, 112 * 112 * 6), guarded(n, pb), guarded(n, pb), guarded(n, pb), guarded(n, pb)]
    try:
        results, rgba = [], []
        for with_filter, c, crop_out, align_out in zip((True, False), ctxs, outs[1:3], outs[3:5]):
            c.set_geometry(W, H, 2)
            c.upload(np.stack([a.frames[0], b.frames[0]]))
            pairs = start_pairs(c)
            c.camshift_stats(cr.RESERVED, reset=True)
            c.upload(np.stack([a.frames[1], b.frames[1]]))
            c.camshift_track_pairs(pairs, fetch=False)
            if with_filter:
                c.camshift_align_pairs_filtered_device(outs[0].ptr, CROP_LIST, 16, 7, 8, fmt, margin=4.0, square=True)
                c.camshift_crop_pairs_filtered_device(outs[0].ptr, CROP_LIST, 1, 1, 8)
            c.camshift_crop_pairs_device(crop_out.ptr, CROP_LIST, 70, 19)
            crop_rec = c.camshift_crop_result(n).tobytes()
            if with_filter:
                c.camshift_crop_sources_filtered_device(outs[0].ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 16, 7, 8, dict(dtype="f32", layout="hwc", channels="bgr"))
                assert len(c.camshift_crop_result(7)) == 7
            c.camshift_align_pairs_device(align_out.ptr, CROP_LIST, 70, 19)
            align_rec = c.camshift_align_result(n).tobytes()
            if with_filter:
                c.camshift_align_sources_filtered_device(outs[0].ptr, [5, 0, 2, cr.NEVER_TRACKED, 3, 5, 0], res.entries(), 7, 3, 3)
                assert len(c.camshift_align_result(7)) == 7
                with pytest.raises(HtError):
                    c.camshift_align_result(n)  # n differs: the filtered call IS the last align call
                c.camshift_crop_pairs_filtered_device(outs[0].ptr, CROP_LIST[:2], 1, 1, 2, fmt)
                assert [int(v) for v in c.camshift_crop_result(2)["code"]] == [cr.FACE, cr.EMPTY]
            first = c.camshift_track_collect(3)
            c.synchronize()
            rgba.append((crop_rec, align_rec, d2h(crop_out.ptr, crop_out.nbytes).tobytes(), d2h(align_out.ptr, align_out.nbytes).tobytes()))
            c.upload(np.stack([a.frames[2], b.frames[2]]))
            second = c.camshift_track_pairs(pairs)
            tracked = {s for s, _f in pairs}
            hists = [c.camshift_debug_hist(s, current=s in tracked) for s in range(cr.RESERVED)]
            results.append((first.tobytes(), second.tobytes(), [(m.tobytes(), h.tobytes()) for m, h in hists], [v.tobytes() for v in c.camshift_stats(cr.RESERVED, reset=False)]))
        objects_agree(np.frombuffer(results[0][1], dtype=native.CS_TRACKOBJ_DTYPE), [oracle_step(2)[s] for s, _f in pairs], "step 2 behind the filtered calls")
        assert results[0] == results[1]
        assert rgba[0] == rgba[1]
        objs = oracle_step(1)
        srcs = [canvas_source(a.frames[1]), canvas_source(b.frames[1])]
        want = [cr.patch(srcs[f], cr.obj_of(objs[s]) if s in objs else NO_BOX, W, H, None, 256, 0, 70, 19) for s, f in CROP_LIST]
        same(np.frombuffer(rgba[0][2], dtype=np.uint8), expected_buffer(want, pb), "the crop call among the filtered calls")
    finally:
        for c in ctxs:
            c.close()
        res.free()
        for o in outs:
            o.free()


# ---- 7: refusals change nothing ------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing(pairs_ctx, restated):
    """max_factor 0, 9 and -1; a bad format; and the sibling calls' refusals (params, list, entries, output, stride, overlap): the status, the
    words, the guarded output still all 0xA5 and the previous call's records unchanged; the next valid call is exact"""
    c, objs, sources = pairs_ctx
    L, h = c._lib, c._h
    P, Q = 7, 3
    n = len(CROP_LIST)
    res = ResidentFeeds()
    out = guarded(8, P * Q * 4)
    fill = guarded(8, P * Q * 12)
    try:
        entries = res.entries()
        srcs = c._draw_sources(entries)
        streams7 = np.array([5, 0, 2, 4, 3, 5, 0], dtype=np.int32)
        pairs6 = c._pairs(CROP_LIST)
        good = pt.pack_format(1, 0, 0, 0, *pt.PAIRS["signed"])
        z3, one3 = (0.0,) * 3, (1.0,) * 3
        bad_formats = [pt.pack_format(3, 0, 0, 0, one3, z3), pt.pack_format(0, 2, 0, 0, one3, z3), pt.pack_format(0, 0, 3, 0, one3, z3), pt.pack_format(0, 0, 0, 1, one3, z3),
                       pt.pack_format(1, 0, 0, 0, (1.0, float("nan"), 1.0), z3), pt.pack_format(1, 0, 2, 0, (1.0, 1.0, 0.0), z3)]
        for kind in ("crop", "align"):
            k = KINDS[kind]
            k.rgba_pairs(c, out.ptr, CROP_LIST, P, Q, 256, 0)
            before = k.result(c, n).tobytes()
            c.synchronize()
            prm_t = native.CROP_PARAMS if k.crop else native.ALIGN_PARAMS
            fn_pairs = L.ht_camshift_crop_pairs_filtered_device if k.crop else L.ht_camshift_align_pairs_filtered_device
            fn_sources = L.ht_camshift_crop_sources_filtered_device if k.crop else L.ht_camshift_align_sources_filtered_device

            def refused(call, status, index=None, text=None):
                with pytest.raises(HtError) as e:
                    call()
                assert e.value.status == status, str(e.value)
                if index is not None:
                    assert f"entry {index}:" in str(e.value), (index, str(e.value))
                if text is not None:
                    assert text in str(e.value), (text, str(e.value))
                c.synchronize()
                assert (d2h(fill.ptr, fill.nbytes) == dl.GUARD).all(), str(e.value)
                assert k.result(c, n).tobytes() == before, str(e.value)

            def pairs_call(mf=8, fmt=None, ptr=fill.ptr, stride=0, prm=(P, Q, 256, 0), plist=pairs6, cnt=None):
                p = prm_t(*prm) if prm is not None else None
                f = native.PATCH_FORMAT.from_buffer_copy(fmt) if fmt is not None else None
                return lambda: c._check(fn_pairs(h, plist.ctypes.data if plist is not None else None, len(pairs6) if cnt is None else cnt, C.byref(p) if p is not None else None, mf,
                                                 C.byref(f) if f is not None else None, ptr, stride))

            def sources_call(mf=8, fmt=None, ptr=fill.ptr, stride=0, prm=(P, Q, 256, 0), arr=srcs, st=streams7, cnt=7):
                p = prm_t(*prm) if prm is not None else None
                f = native.PATCH_FORMAT.from_buffer_copy(fmt) if fmt is not None else None
                return lambda: c._check(fn_sources(h, st.ctypes.data if st is not None else None, arr, cnt, C.byref(p) if p is not None else None, mf,
                                                   C.byref(f) if f is not None else None, ptr, stride))

            for call in (pairs_call, sources_call):
                for mf in (0, 9, -1):
                    refused(call(mf=mf), HT_ERR_INVALID, text="max_factor")
                    refused(call(mf=mf, fmt=good), HT_ERR_INVALID, text="max_factor")
                for bf in bad_formats:
                    refused(call(fmt=bf), HT_ERR_INVALID, text="format")
                # the sibling calls' refusals
                refused(call(prm=None), HT_ERR_INVALID, text="NULL params")
                refused(call(prm=(0, Q, 256, 0)), HT_ERR_INVALID, text="1..1024")
                refused(call(prm=(P, 1025, 256, 0)), HT_ERR_INVALID, text="1..1024")
                refused(call(prm=(P, Q, 63, 0)), HT_ERR_INVALID, text="margin_q8")
                refused(call(prm=(P, Q, 1025, 0)), HT_ERR_INVALID, text="margin_q8")
                refused(call(prm=(P, Q, 256, 2)), HT_ERR_INVALID, text="unknown flag")
                refused(call(prm=(P, Q, 256, 0x80000000)), HT_ERR_INVALID, text="unknown flag")
                refused(call(cnt=0), HT_ERR_INVALID)
                refused(call(cnt=65536), HT_ERR_INVALID)
                refused(call(ptr=fill.ptr + 2), HT_ERR_INVALID)       # misaligned
                refused(call(ptr=None), HT_ERR_INVALID)               # no output
                refused(call(stride=P * Q * 4 - 4), HT_ERR_INVALID)   # shorter than a patch
                refused(call(stride=P * Q * 4 + 2), HT_ERR_INVALID)   # no multiple of 4
                refused(call(fmt=good, stride=126), HT_ERR_INVALID)   # the tensor's stride rule: a patch's 126 bytes are no multiple of 4
            refused(pairs_call(plist=None), HT_ERR_INVALID)
            bad = pairs6.copy()
            bad[3] = (cr.RESERVED, 0)
            refused(pairs_call(plist=bad), HT_ERR_INVALID, 3, "not reserved")
            bad = pairs6.copy()
            bad[2] = (0, 2)
            refused(pairs_call(plist=bad), HT_ERR_INVALID, 2, "not bound")
            refused(sources_call(st=None), HT_ERR_INVALID, text="NULL streams")
            bad = streams7.copy()
            bad[5] = -1
            refused(sources_call(st=bad), HT_ERR_INVALID, 5, "not reserved")
            e = [dict(x) for x in entries]
            e[4]["format"] = 7
            refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 4)
            e = [dict(x) for x in entries]
            e[2]["p1"] = fill.ptr + 7 * P * Q * 4 - 1                # entry 2's U plane begins on the RGBA range's last byte
            refused(sources_call(arr=c._draw_sources(e)), HT_ERR_INVALID, 2, "overlap")
            e[2]["p1"] = fill.ptr + 893                              # ... and on the last byte of the TENSOR's range (7 patches, 128 apart)
            refused(sources_call(arr=c._draw_sources(e), fmt=good), HT_ERR_INVALID, 2, "overlap")
            # the next valid call is exact
            obj = pairs_objects(kind, objs)
            want = [restated.patch(kind, ("pairs", f), sources[f], o, None, 1024, cr.SQUARE, P, Q, 8)[0] for o, (_s, f) in zip(obj, CROP_LIST)]
            ok = guarded(n, P * Q * 4)
            try:
                filtered_pairs(kind, c, ok.ptr, CROP_LIST, P, Q, 8, 1024, cr.SQUARE)
                c.synchronize()
                same(d2h(ok.ptr, ok.nbytes), expected_buffer(want, P * Q * 4), f"{kind}: the call behind the refusals")
            finally:
                ok.free()
        # a context without geometry or streams: HT_ERR_STATE, as the siblings
        c2 = Context()
        try:
            with pytest.raises(HtError) as e:
                c2.camshift_crop_pairs_filtered_device(fill.ptr, CROP_LIST, P, Q)
            assert e.value.status == HT_ERR_STATE
            c2.set_geometry(W, H, 2)
            with pytest.raises(HtError) as e:
                c2.camshift_align_sources_filtered_device(fill.ptr, [0], entries[:1], P, Q)
            assert e.value.status == HT_ERR_STATE
        finally:
            c2.close()
    finally:
        res.free()
        out.free()
        fill.free()

"""CPU-side checks of the prefiltered face crops (ht_camshift_crop_*_filtered_device / ht_camshift_align_*_filtered_device): the rule in
headtrackr_amd/csrc/ht_filter_plan.h — the lines k_cut_mean and k_upright_mean compile for the device — against the Python restatement of
tests/filter_cases.py, plain and under AddressSanitizer + UBSan, as a program of its own; the restatement's own properties (factor 1 is
the unfiltered patch, exact ratios are the integer box mean of the source, a checkerboard comes out flat); the scenes the GPU tests
filter, proved from the oracle alone to cover what those tests claim; the entry points at every layer; the kernels' budget and their
place in the library's code objects.  No compute calls (no GPU here).  Without the feature every test but the restatement's own fails."""
import ctypes as C
import importlib.util
import inspect
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import draw_list_cases as dl
import filter_cases as fc
import patch_tensor_cases as pt
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
EXPORTS = ("ht_camshift_crop_pairs_filtered_device", "ht_camshift_crop_sources_filtered_device", "ht_camshift_align_pairs_filtered_device",
           "ht_camshift_align_sources_filtered_device", "ht_camshift_crop_filter_factors", "ht_camshift_align_filter_factors")
N_RANDOM = 100000
W, H = cr.CANVAS


# ---- the rule header ------------------------------------------------------------------------------------------------------------------------

def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("filter_plan") / ("filter_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "filter_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, False)


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, True)


@pytest.fixture(scope="module")
def cases():
    """the edge table and the seeded random records, with the restatement's answer for each: computed once"""
    cs = fc.edge_cases() + fc.random_cases(N_RANDOM)
    return cs, np.array([fc.want_of(c) for c in cs], dtype=np.int64)


def test_edge_table_covers_what_it_claims():
    """from the restatement alone: w and h at exact multiples of P and Q and one either side (the factor steps there); every factor 1..8 and
    every max_factor; sums at the rounding half for even and odd n, where the mean steps; the L1 norm at 2^49 with a fine width of 8192;
    empty records"""
    cs = fc.edge_cases()
    crop = {c: fc.want_of(c) for c in cs if c[0] == 0 and c[8] == 1}
    for (P, k) in ((112, 3), (70, 8), (16, 5)):
        at, above, below = [next(v for c, v in crop.items() if c[1] == k * P + d and c[5] == P and c[7] == 8) for d in (0, 1, -1)]
        assert (below[0], at[0], above[0]) == (k, k, min(8, k + 1))
    assert {v[0] for v in crop.values()} == set(range(1, 9)) == {v[1] for v in crop.values()} and {c[7] for c in cs} == set(range(1, 9))
    assert any(c[1] > 8 * c[5] and v[0] == c[7] for c, v in crop.items())  # limited by max_factor
    align = {c: fc.want_of(c) for c in cs if c[0] == 1 and c[8] == 1}
    assert {v[0] for v in align.values()} == set(range(1, 9)) == {v[1] for v in align.values()}
    bound = [(c, v) for c, v in align.items() if abs(c[1]) + abs(c[2]) == 1 << 49 and c[5] == 1024 and c[7] == 8]
    assert bound and all(v[0] == 8 and abs(v[3]) > 1 << 46 for c, v in bound)  # P' = 8192: a term of nearly half the vector
    assert any(c[1] < 0 for c, _ in bound) and any(c[1] > 0 for c, _ in bound)
    assert all(fc.want_of(c)[:2] == (0, 0) for c in cs if c[8] == 0) and sum(c[8] == 0 for c in cs) >= 16
    rounding = [c for c in cs if c[5:8] == (1, 1, 1) and c[:3] == (0, 1, 1)]
    assert {c[10] for c in rounding} == {a * b for a in range(1, 9) for b in range(1, 9)}
    for n in (2, 9, 64, 35):  # even and odd n: the sum one below the half rounds down, from the half on up
        q, down, up = 127, (n - 1) >> 1, (n + 1) >> 1  # the largest remainder that rounds down, the smallest that rounds up
        assert any(c[10] == n and c[9] == q * n + down for c in rounding) and any(c[10] == n and c[9] == q * n + up for c in rounding)
        assert fc.mean(q * n + down, n) == q and fc.mean(q * n + up, n) == q + 1
    assert fc.mean(2 * 127 + 1, 2) == 128 and fc.mean(9 * 127 + 4, 9) == 127 and fc.mean(9 * 127 + 5, 9) == 128  # a tie (even n only) rounds up
    assert fc.mean(255 * 64, 64) == 255 and fc.mean(0, 64) == 0


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rule_header_equals_the_restatement(harness, harness_san, cases, tmp_path, which):
    """every case of the edge table and 100 000 seeded random records: the factors (through the record functions), the rounded mean and the
    fine patch's first and last column term of the header equal the restatement's"""
    cs, want = cases
    assert len(cs) >= N_RANDOM + 1000
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(fc.pack_cases(cs))
    r = subprocess.run([harness if which == "plain" else harness_san, src, dst], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.int64).reshape(-1, 5)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(cs[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    rnd = want[-N_RANDOM:]
    assert 0.05 * N_RANDOM < int((rnd[:, 0] == 0).sum()) < 0.25 * N_RANDOM  # empty records among the random ones
    for f in range(1, 9):
        assert int((rnd[:, 0] == f).sum()) > 0.01 * N_RANDOM, f  # the random records are no monoculture


# ---- properties of the restatement ------------------------------------------------------------------------------------------------------------

def _boxed(w, h, margin=256):
    """a track object on the 97 x 81 canvas (the canvas is the source) whose crop rect is exactly w x h around (48, 40); w, h even"""
    obj = (48.0, 40.0, float(w), float(h))
    code, rect = cr.rule(obj, W, H, W, H, None, margin, 0)
    assert code == cr.FACE and rect == (48 - w // 2, 40 - h // 2, w, h)
    return obj, rect


def _box_mean(view, rect, nx, ny):
    """the exact integer box mean of a source block, pixel by pixel in Python integers"""
    l, t, w, h = rect
    out = np.zeros((h // ny, w // nx, 4), dtype=np.uint8)
    for y in range(h // ny):
        for x in range(w // nx):
            for ch in range(4):
                total = sum(int(view[t + ny * y + b, l + nx * x + a, ch]) for a in range(nx) for b in range(ny))
                out[y, x, ch] = (total + ((nx * ny) >> 1)) // (nx * ny)
    return out


def test_factor_1_is_the_unfiltered_patch():
    """at max_factor 1, and for any box that is not downscaled, the restatement is the unfiltered restatement, crop and align"""
    src = dl.Source(dl.RGBA, W, H, seed=5)
    for obj5 in ((48.0, 40.0, 30.0, 22.0, 0.9), (20.3, 60.1, 9.0, 14.0, 2.2)):
        for (P, Q, margin, flags) in ((7, 3, 256, 0), (16, 7, 1024, cr.SQUARE), (70, 19, 64, 0)):
            for mf in (1, 8):
                got, f = fc.crop_patch(src, obj5[:4], W, H, None, margin, flags, P, Q, mf)
                if mf == 1 or f == (1, 1):
                    assert f == (1, 1) and np.array_equal(got, cr.patch(src, obj5[:4], W, H, None, margin, flags, P, Q))
                got, f = fc.align_patch(src, obj5, W, H, None, margin, flags, P, Q, mf)
                if mf == 1 or f == (1, 1):
                    assert f == (1, 1) and np.array_equal(got, al.patch(src, obj5, W, H, None, margin, flags, P, Q))
    assert fc.crop_patch(src, (48.0, 40.0, 6.0, 2.0), W, H, None, 256, 0, 70, 19, 8)[1] == (1, 1)  # upscaled: not filtered


def test_exact_ratios_are_the_integer_box_mean_of_the_source():
    """where w == Nx P and h == Ny Q the fine patch is the source block itself, so the output is the exact integer box mean of the source:
    RGBA, and NV12 / I420 through the declared conversion (the mean is taken of the converted pixels)"""
    for src in (dl.Source(dl.RGBA, W, H, seed=11), dl.Source(yc.NV12, W, H, seed=12, matrix=1), dl.Source(yc.I420, W, H, seed=13, matrix=2)):
        for (w, h, P, Q) in ((20, 12, 10, 4), (16, 16, 2, 2), (48, 6, 6, 6), (8, 64, 8, 8)):
            obj, rect = _boxed(w, h)
            got, (nx, ny) = fc.crop_patch(src, obj, W, H, None, 256, 0, P, Q, 8)
            assert (nx, ny) == (w // P, h // Q) and nx * ny > 1
            assert np.array_equal(cr.patch(src, obj, W, H, None, 256, 0, nx * P, ny * Q), src.rgba[rect[1]:rect[1] + h, rect[0]:rect[0] + w])  # the fine patch IS the block
            assert np.array_equal(got, _box_mean(src.rgba, rect, nx, ny)), (src.fmt, w, h, P, Q)
        # cut by max_factor the fine patch is a resampling again, and the output no box mean of the source
        obj, rect = _boxed(48, 6)
        got, f = fc.crop_patch(src, obj, W, H, None, 256, 0, 6, 6, 3)
        assert f == (3, 1) and not np.array_equal(got, fc.crop_patch(src, obj, W, H, None, 256, 0, 6, 6, 8)[0])


def test_a_checkerboard_comes_out_flat():
    """the failure the feature removes.  A 1-pixel checkerboard cut at 2 : 1 is a flat 127 or 128 patch (each 2 x 2 block holds two white and
    two black pixels).  At 3 : 1 the UNFILTERED restatement samples one source pixel per patch pixel (the tap weight is 0: 3 i + 1 is a
    pixel centre) and gives pure black or white, a full-contrast alias of a source whose mean is gray; the filtered patch stays within 15
    of the mean (5 of 9 or 4 of 9 pixels white).  (At exactly 2 : 1 the unfiltered sample centre falls between four pixels and the bilinear
    blend is gray too: the alias needs a ratio whose centres land on pixels.)"""
    src = dl.Source(dl.RGBA, W, H, seed=1)
    src.rgba = fc.checkerboard(W, H)
    obj, _rect = _boxed(40, 24)
    got, f = fc.crop_patch(src, obj, W, H, None, 256, 0, 20, 12, 8)
    assert f == (2, 2) and set(np.unique(got[..., :3]).tolist()) <= {127, 128} and (got[..., 3] == 255).all()
    obj, _rect = _boxed(60, 36)
    plain = cr.patch(src, obj, W, H, None, 256, 0, 20, 12)
    assert set(np.unique(plain[..., :3]).tolist()) == {0, 255}
    got, f = fc.crop_patch(src, obj, W, H, None, 256, 0, 20, 12, 8)
    assert f == (3, 3) and set(np.unique(got[..., :3]).tolist()) == {113, 142}
    got, f = fc.align_patch(src, (48.0, 40.0, 40.0, 24.0, np.pi / 2), W, H, None, 256, 0, 20, 12, 8)  # upright: the crop's factors
    assert f == (2, 2) and set(np.unique(got[..., :3]).tolist()) <= {127, 128}


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------

def _scene_entries():
    """[(obj5 or None, source size, mapping)] of the GPU tests' lists: the pairs scene's trackers after step 1 and its two EMPTY streams on
    the canvas, the feeds' objects in their own sources"""
    a, b = cr.pairs_scene()
    seqs = (a, b)
    out = [(al.obj_of(seqs[q].oracle_calls(j)[0][2]), W, H, None) for (_s, _f, q, j) in cr.pairs_trackers()]
    out += [(None, W, H, None), (None, W, H, None)]  # a stream never tracked, a stream never initialised: the state's zeros
    out += [(al.obj_of(to), src.w, src.h, m) for (src, m), to in zip(cr.feeds(), cr.feed_objects())]
    return out


@pytest.mark.parametrize("kind", ["crop", "align"])
def test_scenes_cover_every_factor_and_what_the_gpu_tests_claim(kind):
    """from the oracle's real track objects alone (tests/test_crop_cpu.py and tests/test_align_cpu.py prove them insensitive to the
    summation order): over crop_cases.pairs_scene() and crop_cases.feeds() under crop_cases.CONFIGS and filter_cases.SIZES every factor 1..8
    occurs on each axis; entries with Nx != Ny, entries limited by max_factor (the need exceeds 8), entries at (1, 1) and empty entries
    exist.  With the four sizes of the issue alone the crop entries miss factor 6 on both axes and the align entries Nx == 7: 3 x 4 was
    added, the condition was not relaxed.  At the wrap (the strip feeds' angle, 0 or pi) both admissible steps give the same factors"""
    entries = _scene_entries()
    seen, limited = set(), False
    for (P, Q) in fc.SIZES:
        for (m, fl) in cr.CONFIGS:
            for obj, SW, SH, mapping in entries:
                if kind == "crop":
                    code, rect = cr.rule(obj[:4] if obj else (0.0, 0.0, 0.0, 0.0), W, H, SW, SH, mapping, m, fl)
                    seen.add(fc.crop_factors(code, rect, P, Q, 8))
                    limited |= code == cr.FACE and (rect[2] > 8 * P or rect[3] > 8 * Q)
                else:
                    pl = al.plan(obj if obj else al.NO_OBJECT, W, H, SW, SH, mapping, m, fl)
                    seen.add(fc.align_factors(pl, P, Q, 8))
                    limited |= pl[0] == al.FACE and (abs(pl[4]) + abs(pl[5]) > 8 * P * 65536 or abs(pl[6]) + abs(pl[7]) > 8 * Q * 65536)
                    if obj and al.at_wrap(obj[4]):
                        both = {fc.align_factors(al.plan((*obj[:4], a), W, H, SW, SH, mapping, m, fl), P, Q, 8) for a in (0.0, np.pi)}
                        assert len(both) == 1
    assert (0, 0) in seen and (1, 1) in seen and limited
    faces = seen - {(0, 0)}
    assert {f[0] for f in faces} == set(range(1, 9)) == {f[1] for f in faces}, sorted(faces)
    assert any(nx != ny for nx, ny in faces)
    if kind == "crop":
        assert {(3, 8), (5, 8), (1, 4), (2, 3)} <= faces
    # the issue's four sizes alone do not hold the condition: that is why there is a fifth
    four = set()
    for (P, Q) in fc.SIZES[:4]:
        for (m, fl) in cr.CONFIGS:
            for obj, SW, SH, mapping in entries:
                if obj and kind == "crop":
                    four.add(fc.crop_factors(*cr.rule(obj[:4], W, H, SW, SH, mapping, m, fl), P, Q, 8))
                elif obj:
                    four.add(fc.align_factors(al.plan(obj, W, H, SW, SH, mapping, m, fl), P, Q, 8))
    assert fc.SIZES[:4] == [(70, 19), (1, 1), (112, 112), (16, 7)] and {f[0] for f in four} != set(range(1, 9))


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_at_every_layer_and_fail_loudly_without_a_device():
    """fails without the feature: the header, the library, native.py, the API, torch_patches and INTEGRATION.md all name the six exports; the
    C ABI answers all-zero arguments with a status; the factor functions need no context, refuse NULL and out-of-range arguments and give
    0, 0 for an empty record; without a device a Context cannot be made, so no filtered call can silently do nothing"""
    from headtrackr_amd import api, torch_patches
    from headtrackr_amd.api import Context, HtError

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "#define HT_ABI_VERSION 2" in header and "a prefilter for strong downscales, per-entry" not in header  # the "Not part of this" lists point here now
    assert L.ht_camshift_crop_pairs_filtered_device(None, None, 0, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_crop_sources_filtered_device(None, None, None, 0, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_pairs_filtered_device(None, None, 0, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_sources_filtered_device(None, None, None, 0, None, 0, None, None, 0) == native.HT_ERR_INVALID
    nx, ny = C.c_int32(-7), C.c_int32(-7)
    crop, align = native.CROP_RECORD(), native.ALIGN_RECORD()
    for fn, rec in ((L.ht_camshift_crop_filter_factors, crop), (L.ht_camshift_align_filter_factors, align)):
        assert fn(None, 0, 0, 0, None, None) == native.HT_ERR_INVALID
        assert fn(None, 112, 112, 8, C.byref(nx), C.byref(ny)) == native.HT_ERR_INVALID
        assert fn(C.byref(rec), 112, 112, 8, None, C.byref(ny)) == native.HT_ERR_INVALID and fn(C.byref(rec), 112, 112, 8, C.byref(nx), None) == native.HT_ERR_INVALID
        for (P, Q, mf) in ((0, 112, 8), (112, 1025, 8), (112, 112, 0), (112, 112, 9), (112, 112, -1)):
            assert fn(C.byref(rec), P, Q, mf, C.byref(nx), C.byref(ny)) == native.HT_ERR_INVALID, (P, Q, mf)
        assert (nx.value, ny.value) == (-7, -7)  # a refusal writes nothing
        assert fn(C.byref(rec), 112, 112, 8, C.byref(nx), C.byref(ny)) == 0 and (nx.value, ny.value) == (0, 0)  # an empty record
        nx.value = ny.value = -7
    # the wrappers over record arrays against the restatement
    rec = np.zeros(4, dtype=native.CROP_RECORD_DTYPE)
    rec["code"], rec["width"], rec["height"] = [1, 0, 1, 1], [792, 500, 112, 113], [594, 500, 1, 2000]
    assert api.crop_filter_factors(rec, 112, 112, 8).tolist() == [list(fc.crop_factors(int(r["code"]), (0, 0, int(r["width"]), int(r["height"])), 112, 112, 8)) for r in rec]
    assert api.crop_filter_factors(rec, 112, 112, 8).tolist() == [[8, 6], [0, 0], [1, 1], [2, 8]] and api.crop_filter_factors(rec, 112, 112, 3).tolist()[0] == [3, 3]
    arec = np.zeros(2, dtype=native.ALIGN_RECORD_DTYPE)
    arec["code"], arec["ux"], arec["uy"], arec["vx"], arec["vy"] = 1, [300 * 65536, -5], [-(36 * 65536 + 1), 0], [7, 0], [-112 * 65536, 1 << 48]
    want = [list(fc.align_factors((1, 0, 0, 0, int(r["ux"]), int(r["uy"]), int(r["vx"]), int(r["vy"])), 112, 112, 8)) for r in arec]
    assert api.align_filter_factors(arec, 112, 112, 8).tolist() == want == [[4, 2], [1, 8]]  # one Q16 unit beyond 3 P and beyond 1 Q: the next factor
    with pytest.raises(HtError):
        api.crop_filter_factors(rec, 112, 112, 9)
    for m in ("camshift_crop_pairs_filtered_device", "camshift_crop_sources_filtered_device", "camshift_align_pairs_filtered_device", "camshift_align_sources_filtered_device"):
        sig = inspect.signature(getattr(Context, m))
        assert sig.parameters["max_factor"].default == 8 and sig.parameters["fmt"].default is None and sig.parameters["stride"].default == 0, m
    for m in ("crop_pairs_into", "crop_sources_into", "align_pairs_into", "align_sources_into"):
        assert inspect.signature(getattr(torch_patches, m)).parameters["prefilter"].default is None, m
    if L.ht_device_count() == 0:
        with pytest.raises(HtError) as e:
            Context()
        assert "no CPU fallback" in str(e.value) or "no HIP device" in str(e.value)


def test_torch_patches_prefilter_takes_the_filtered_route_and_none_todays():
    """on a recording stand-in for the Context: prefilter=None issues exactly the _tensor call it issues today, prefilter=N the _filtered
    call with max_factor N and the same pointer, size, format and stride"""
    import torch

    from headtrackr_amd import torch_patches as tp
    from headtrackr_amd.api import PatchFormat

    calls = []

    class Rec:
        device = 0

        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))

    fmt = PatchFormat("f16", "chw", "rgb")
    x = torch.zeros((2, 3, 7, 6), dtype=torch.float16)
    orig, tp._on_device = tp._on_device, lambda what, ctx, tensor: None  # a CPU tensor stands in: nothing is written
    try:
        tp.crop_pairs_into(Rec(), x, [(0, 0), (1, 0)], fmt)
        tp.crop_pairs_into(Rec(), x, [(0, 0), (1, 0)], fmt, margin=2.0, prefilter=5)
        tp.align_sources_into(Rec(), x, [0, 1], [{}, {}], fmt, square=True, prefilter=8)
        tp.align_sources_into(Rec(), x, [0, 1], [{}, {}], fmt, square=True)
    finally:
        tp._on_device = orig
    stride = x.stride(0) * 2
    assert calls[0] == ("camshift_crop_pairs_tensor_device", (x.data_ptr(), [(0, 0), (1, 0)], 6, 7, fmt), dict(margin=1.0, square=False, stride=stride))
    assert calls[1] == ("camshift_crop_pairs_filtered_device", (x.data_ptr(), [(0, 0), (1, 0)], 6, 7), dict(max_factor=5, fmt=fmt, margin=2.0, square=False, stride=stride))
    assert calls[2] == ("camshift_align_sources_filtered_device", (x.data_ptr(), [0, 1], [{}, {}], 6, 7), dict(max_factor=8, fmt=fmt, margin=1.0, square=True, stride=stride))
    assert calls[3] == ("camshift_align_sources_tensor_device", (x.data_ptr(), [0, 1], [{}, {}], 6, 7, fmt), dict(margin=1.0, square=True, stride=stride))
    assert len(calls) == 4


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ops(txt):
    return [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]


def test_filter_kernels_fit_their_budget_and_live_with_the_draw_kernels():
    """code-object metadata and disassembly of k_cut_mean<DT, RPT> and k_upright_mean<DT, RPT> (DT -1: RGBA8; 0, 1, 2: the tensor dtypes; RPT 4:
    the 64 x 16 tile of max_factor 1 and 2, RPT 1: the 64 x 4 tile beyond): no spills, no scratch, the fine taps' 15 / 13 KB and the fine
    terms' 10 / 8.5 KB of LDS (within 64 KB), 256 threads, <= 128 VGPRs (the small tile <= 64), one barrier, no scratch, flat or buffer access;
    the crop kernels blend in binary64 with nothing contracted behind the barrier.  They live in
    the code object of k_draw_list; the pyramid, scan and camshift code objects are byte-identical to profiles/traffic.json's build; the
    unfiltered kernels' names stay the only ones with `crop` / `align` in them; the pixel bodies are the siblings' text"""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr, dz = _tool("kernel_resources"), _tool("disasm")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    names = [f"{base}<{dt}, {rpt}>" for base in ("k_cut_mean", "k_upright_mean") for dt in (-1, 0, 1, 2) for rpt in (1, 4)]
    for name in names:
        r = res[name]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        rpt = int(name[-2])
        assert r["vgpr_count"] <= (128 if rpt == 4 else 64) and r["group_segment_fixed_size"] <= 64 * 1024, (name, r)
        assert r["group_segment_fixed_size"] == 8 * (64 + 4 * rpt) * (24 if "cut" in name else 16), (name, r)  # taps of 24 bytes, terms of 2 x 8
        assert "crop" not in name and "align" not in name and not name.startswith(("k_cut_tensor", "k_upright_tensor"))
        for marker in fingerprint.UNITS.values():
            assert marker.decode() not in name
    assert sorted(k for k in res if "_mean<" in k) == sorted(names)
    for mangled in ("k_cut_meanILin1ELi1E", "k_cut_meanILin1ELi4E", "k_upright_meanILin1ELi1E", "k_upright_meanILi1ELi4E"):
        ops = _ops(dz.disasm(mangled))
        assert ops, mangled
        assert not any(o.startswith(("scratch_", "flat_", "buffer_")) for o in ops) and sum(o == "s_barrier" for o in ops) == 1
        head, body = ops[:ops.index("s_barrier")], ops[ops.index("s_barrier"):]
        assert any(o.startswith("s_load_dword") for o in head) and not any(o.startswith("global_load") for o in head)  # descriptor and state: scalar loads only
        if "cut" in mangled:
            rpt = 1 if mangled.endswith("Li1E") else 4
            assert sum(o.startswith("v_rndne_f64") for o in body) == 3 * 4 * rpt  # one rounding per channel of a thread's samples, in each of the three bodies
            assert not any(o.startswith(("v_fma_f64", "v_mad_f", "v_mac_f", "v_div_")) for o in body)
            assert sum(o.startswith("v_div_fixup_f64") for o in head) == 4  # the record's two ratios and the fine patch's two
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_cut_mean" in o]
    assert len(home) == 1 and b"k_upright_mean" in home[0] and b"k_draw_list" in home[0] and b"k_crop_list" in home[0]
    family = ("ht_crop.hip", "ht_align.hip", "ht_patch.hip", "ht_filter.hip", "ht_face_calls.hip", "ht_list_parts.inc")
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_filter_plan.h", "ht_ingest_bodies.inc") + family}
    whole = "".join(text[f] for f in family)
    assert text["ht_ingest.hip"].index('#include "ht_patch.hip"') < text["ht_ingest.hip"].index('#include "ht_filter.hip"')
    # the pixel bodies are the siblings' text: the mean kernels include no body themselves, they take the ONE scaffold (with their loops over
    # the fine slices in front of each body) and the ONE al_pixels dispatch, behind the ONE cut head and the ONE upright head
    assert text["ht_filter.hip"].count('#include "ht_ingest_bodies.inc"') == 0 and text["ht_filter.hip"].count("#define LP_PART 4  // LP_SCAFFOLD") == 1
    assert text["ht_filter.hip"].count("#define LP_EACH_PASS") == 1 and text["ht_filter.hip"].count("AL_PIXELS_ANY(") == 1 and whole.count("al_pixels<") == 3
    assert text["ht_filter.hip"].count("#define LP_PART 1  // LP_CUT_HEAD") == 1 and text["ht_filter.hip"].count("#define LP_PART 2  // LP_UPRIGHT_HEAD") == 1
    assert whole.count("ht_crop_rule(") == 1 and whole.count("ht_align_rule(") == 1 and "ig_channel(" not in whole
    assert text["ht_list_parts.inc"].count('#include "ht_ingest_bodies.inc"') == 3 and whole.count('#include "ht_ingest_bodies.inc"') == 3 + 2
    assert text["ht_ingest_bodies.inc"].count("        IG_STORE(o, x, Y0 + ") == 2
    plan = text["ht_filter_plan.h"]
    assert "hip/" not in plan and "__global__" not in plan and "double" not in plan and "float" not in plan  # integers only
    assert "2^61" in plan  # the new bound of the align term is stated


# ---- the N-API shim against the recording stub ------------------------------------------------------------------------------------------------

NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_max_factor_and_the_format_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with the existing stubs and tests/js/filter_stub.cc: the successful calls of tests/js/filter_addon.js reach the
    C ABI with the pairs / streams, the params, maxFactor, a NULL format for null / undefined or the format's enums and the bits of its six
    floats, the output offset and the stride as given; the range check uses the RGBA patch's bytes without a format and the TENSOR's with
    one; a maxFactor outside 1..8 is a RangeError and every malformed argument throws before the C ABI is reached, through the shim's one
    argument reader (its call sites are still four); the factor functions hand records, sizes and maxFactor on and return an Int32Array;
    a refusal of the library comes back as an Error"""
    addon = str(tmp_path / "addon_filter.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), *[os.path.join(ROOT, "tests", "js", f) for f in
                                                                                                        ("abi_stub.cc", "crop_stub.cc", "align_stub.cc", "patch_stub.cc", "filter_stub.cc")], "-o", addon])
    log = str(tmp_path / "filter.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "filter_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_FILTER_STUB_LOG=log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kinds"] == ["function"] * 6
    calls = [json.loads(ln) for ln in open(log)]
    bits = lambda *v: [struct.unpack("<I", struct.pack("<f", x))[0] for x in v]
    F16 = dict(format=[1, 0, 0, 0], coef=bits(1 / 255, 2 / 255, 0.5, -1.0, 0.0, -0.0))
    for k, kind in enumerate(("crop", "align")):
        c = calls[4 * k:4 * k + 4]
        assert c[0] == dict(fn=f"{kind}_pairs", ctx=True, n=4, out=1, pairs=[[5, 0], [0, 0], [2, 1], [2, 1]], params=[7, 3, 256, 0], max_factor=8, format=None, stride=0)
        assert c[1] == dict(fn=f"{kind}_pairs", ctx=True, n=2, out=1, pairs=[[5, 0], [0, 0]], params=[7, 3, 1024, 1], max_factor=1, stride=132, **F16)
        assert c[2] == dict(fn=f"{kind}_sources", ctx=True, n=2, out=-50000, streams=[3, 3], sizes=[[7, 5, 16], [23, 23, 0]], params=[7, 3, 256, 0], max_factor=3, format=None, stride=0)
        assert c[3] == dict(fn=f"{kind}_sources", ctx=True, n=2, out=12 - 51001, streams=[1, 7], sizes=[[23, 23, 0], [7, 5, 16]], params=[7, 3, 1024, 1], max_factor=5, stride=0, **F16)
    rest = calls[8:]
    assert len(rest) == 12 and [(c["n"], c["format"] is None) for c in rest] == [(4, True), (4, False), (3, True)] * 4  # per function: the two calls that exactly fit, the one the stub refuses
    # the stub's factor functions answer (width + out_width, height + max_factor) and (ux >> 16) + out_width, (vy >> 16) + max_factor: every argument arrived
    assert out["cropFactors"] == [30 + 112, 40 + 8, 0, 0] and out["cropFactorsKind"] == "Int32Array" and out["alignFactors"] == [7 + 112, -3 + 3, 0, 0]
    thrown = dict(out["thrown"])
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    names = {"cropPairs": "ht_camshift_crop_pairs_filtered_device", "cropSources": "ht_camshift_crop_sources_filtered_device", "alignPairs": "ht_camshift_align_pairs_filtered_device",
             "alignSources": "ht_camshift_align_sources_filtered_device"}
    kinds = {"too few arguments": "TypeError", "no maxFactor": "TypeError", "maxFactor a string": "TypeError", "maxFactor 0": "RangeError", "maxFactor 9": "RangeError",
             "maxFactor -1": "RangeError", "format a number": "TypeError", "format without dtype": "TypeError", "scale a plain array": "TypeError", "width 0": "RangeError",
             "height 1025": "RangeError", "params of three": "TypeError", "RGBA output four bytes too small": "RangeError", "f16 output two bytes too small": "RangeError",
             "f16 output where only RGBA fits": "RangeError", "output offset beyond": "RangeError", "out null": "TypeError"}
    factor_kinds = {"cropFilterFactors: too few arguments": "TypeError", "cropFilterFactors: records a plain array": "TypeError", "cropFilterFactors: records of five": "TypeError",
                    "cropFilterFactors: maxFactor 9": "RangeError", "cropFilterFactors: width 0": "RangeError", "alignFilterFactors: terms missing": "TypeError",
                    "alignFilterFactors: terms of five": "TypeError", "alignFilterFactors: height 1025": "RangeError"}
    assert set(thrown) == {f"{n}: {w}" for n in names for w in list(kinds) + ["the library refuses"]} | set(factor_kinds)
    for n, sym in names.items():
        for what, kind in kinds.items():
            assert thrown[f"{n}: {what}"].startswith(kind + ": "), (n, what, thrown[f"{n}: {what}"])
        for mf in ("0", "9", "-1"):
            assert "maxFactor is 1..8" in thrown[f"{n}: maxFactor {mf}"]
        assert f"{sym}: status -1" in thrown[f"{n}: the library refuses"]
    for what, kind in factor_kinds.items():
        assert thrown[what].startswith(kind + ": "), (what, thrown[what])
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert {"cropPairsFilteredDevice", "cropSourcesFilteredDevice", "alignPairsFilteredDevice", "alignSourcesFilteredDevice", "cropFilterFactors", "alignFilterFactors"} <= set(
        re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    assert napi.count("get_crop_out(a, ") == 1 and napi.count("get_patch_format(a.env, ") == 1 and napi.count("get_filter_args(a, ") == 1  # the one reader and range check: no second one, and ONE place that calls them


# ---- the JavaScript facade on the mock addon ----------------------------------------------------------------------------------------------------

JS_PREFILTERS = [8, 3, 1]
JS_TENSOR = dict(dtype="f16", layout="chw", channels="rgb", scale=list(pt.PAIRS["imagenet"][0]), bias=list(pt.PAIRS["imagenet"][1]))


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_opts_prefilter_gives_the_rules_bytes_and_changes_nothing_without_it(tmp_path):
    """tests/js/filter_cpu.js on tests/js/mock_addon_filter.js: cropPairs / alignPairs on the pairs scene and cropFeeds / alignFeeds on the
    mixed feeds, 7 x 3 at margin 4, square: without opts.prefilter the facade issues exactly the call it issues today and the result is what
    it always was (the restated RGBA patches' CRC-32, no `factors`), before and after the filtered calls; with opts.prefilter 8, 3 and 1 it
    issues ONE filtered call, `patches` are the restated block means, `factors` the restated factors and the records the unfiltered call's;
    together with opts.tensor the elements are the restated f of the filtered patches; malformed opts.prefilter throw"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    import zlib

    from test_align_cpu import _frame_source
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    P, Q = 7, 3
    cfg = dict(width=P, height=Q, margin=4.0, square=True)
    a, b = cr.pairs_scene()
    seqs, trackers = (a, b), cr.pairs_trackers()
    np.stack([a.frames[0], b.frames[0]]).tofile(tmp_path / "init.raw")
    np.stack([a.frames[1], b.frames[1]]).tofile(tmp_path / "step.raw")
    init_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)] + [cr.NEVER_TRACKED, 1]
    rects = [v for (_s, _f, q, j) in trackers for v in seqs[q].rects[j]] + list(b.rects[0])
    plist = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]
    objs = {s: seqs[q].oracle_calls(j)[0][2] for (s, _f, q, j) in trackers}
    frame_src = [_frame_source(seqs[q].frames[1]) for q in (0, 1)]
    job = dict(w=W, h=H, configs=[cfg], tensors=[JS_TENSOR], prefilters=JS_PREFILTERS,
               pairs=dict(init=str(tmp_path / "init.raw"), step=str(tmp_path / "step.raw"), trackers=cr.RESERVED, init_pairs=init_pairs, rects=[int(v) for v in rects],
                          track_pairs=[v for (s, f, _q, _j) in trackers for v in (s, f)], align_pairs=[v for p in plist for v in p]))
    feeds, fobjs = cr.feeds(), cr.feed_objects()
    streams = [4, 0, 6, 2, 8, 1, 5]
    flist = []
    for k, (src, m) in enumerate(feeds):
        fn = tmp_path / f"feed{k}.raw"
        src.packed().tofile(fn)
        flist.append(dict(file=str(fn), width=src.w, height=src.h, format=dl.FORMAT_NAMES[src.fmt], matrix=yc.MATRIX_NAMES[src.matrix], rect=list(m) if m else None,
                          init=list(cr.canvas_rect_of(k))))
    job["feeds"] = dict(list=flist, streams=streams, trackers=9)
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "filter_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["refusals"] == 2 * 6 + 1 + 2

    def expect(kind, entries, mf):
        """[(patch, factors)] of the restatement; mf None: the unfiltered call"""
        res = []
        for src, to, mapping in entries:
            obj = (cr.obj_of(to) if to else (0.0, 0.0, 0.0, 0.0)) if kind == "crop" else (al.obj_of(to) if to else al.NO_OBJECT)
            if mf is None:
                res.append(((cr.patch if kind == "crop" else al.patch)(src, obj, W, H, mapping, 1024, 1, P, Q), None))
            else:
                res.append((fc.crop_patch if kind == "crop" else fc.align_patch)(src, obj, W, H, mapping, 1024, 1, P, Q, mf))
        return res

    forms = {"pairs": ("Pairs", [(frame_src[f], objs.get(s), None) for (s, f) in plist]), "feeds": ("Sources", [(src, to, m) for (src, m), to in zip(feeds, fobjs)])}
    seen = set()
    for form, (Form, entries) in forms.items():
        n = len(entries)
        for kind in ("crop", "align"):
            got = out[form][kind]
            assert len(got) == 3 + len(JS_PREFILTERS)
            plain_crc = zlib.crc32(np.stack([p for p, _ in expect(kind, entries, None)]).tobytes())
            for g in (got[0], got[-1]):  # without opts.prefilter: the call and the result of today
                assert (g["kind"], g["length"], g["crc"], g["tensor"], g["factors"]) == ("Uint8Array", n * P * Q * 4, plain_crc, None, None), (form, kind, g)
                assert g["called"] == [f"{kind}{Form}Device"], (form, kind, g["called"])
            for g, mf in zip(got[1:1 + len(JS_PREFILTERS)], JS_PREFILTERS):
                want = expect(kind, entries, mf)
                assert g["called"] == [f"{kind}{Form}FilteredDevice"], (form, kind, mf, g["called"])
                assert g["factors"] == [v for _, f in want for v in f], (form, kind, mf, g["factors"])
                assert (g["kind"], g["length"], g["crc"]) == ("Uint8Array", n * P * Q * 4, zlib.crc32(np.stack([p for p, _ in want]).tobytes())), (form, kind, mf)
                assert g["records"] == got[0]["records"] and g["extra"] == got[0]["extra"] and g["n"] == n and g["size"] == [P, Q] and g["tensor"] is None
                assert mf != 1 or g["crc"] == plain_crc  # factor 1: the unfiltered bytes
                seen |= {f for _, f in want}
            g, want = got[1 + len(JS_PREFILTERS)], expect(kind, entries, JS_PREFILTERS[0])  # prefilter and tensor together: still ONE call
            tensor = np.concatenate([pt.f(p, ("f16", "chw", "rgb"), pt.PAIRS["imagenet"]) for p, _ in want])
            assert g["called"] == [f"{kind}{Form}FilteredDevice"] and g["kind"] == "Uint16Array" and g["length"] == n * 3 * P * Q and g["crc"] == zlib.crc32(tensor.tobytes()), (form, kind)
            assert g["factors"] == [v for _, f in want for v in f] and g["tensor"] == dict(dtype="f16", layout="chw", channels="rgb", shape=[n, 3, Q, P])
    assert (0, 0) in seen and (1, 1) in seen and (8, 8) in seen and (3, 3) in seen and any(nx != ny for nx, ny in seen), sorted(seen)
    facade = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("A.cropPairsFilteredDevice(", "A.cropSourcesFilteredDevice(", "A.alignPairsFilteredDevice(", "A.alignSourcesFilteredDevice(", "A.cropFilterFactors(", "A.alignFilterFactors("):
        assert facade.count(m) == 1, m

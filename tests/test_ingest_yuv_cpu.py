"""CPU-side checks of the YUV ingest (ht_draw_frames_yuv / ht_draw_frames_yuv_device): the declared conversion in
headtrackr_amd/csrc/ht_yuv_plan.h equals its numpy restatement (tests/yuv_cases.py) over all 2^24 triples and stays within 1 of the exact
ITU matrices, the call plan handles odd sizes and refuses malformed descriptions (plain and under AddressSanitizer + UBSan, as a program
of its own), the test inputs are sufficient for what the GPU tests claim, the new entry points exist at every layer, the new kernels fit
their budget and leave the three fingerprinted code objects alone, and the JavaScript facade's host logic works on the mock addon.  No
compute calls on the library (no GPU here)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import ingest_cases as ic
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import build, native

NODE = shutil.which("node")
CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NEW_SYMBOLS = ("ht_draw_frames_yuv", "ht_draw_frames_yuv_device")
NEW_ADDON = ("drawFramesYuv", "drawFramesYuvDevice")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the header against the numpy restatement ---------------------------------------------------------------------------------------------

def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("yuv_plan") / ("yuv_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "yuv_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, False)


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, True)


@pytest.fixture(scope="module")
def all_triples_crc():
    """CRC-32 of the numpy restatement over all 2^24 triples (Y slowest, V fastest, 4 bytes R G B A per pixel), per matrix; and the
    largest distance to the exact matrix, and the fraction of triples that clamp — computed in slabs of one Y value"""
    u, v = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    crc, dist, clamped = {}, {}, {}
    for m in range(4):
        c, worst, nclamp = 0, 0, 0
        for y in range(256):
            yy = np.full_like(u, y)
            px = yc.convert(yy, u, v, m)
            c = zlib.crc32(px.tobytes(), c)
            ex = yc.exact_rgb(yy, u, v, m)
            worst = max(worst, max(int(np.abs(px[..., k].astype(np.int32) - ex[k]).max()) for k in range(3)))
            nclamp += int(round(yc.clamped_fraction(yy, u, v, m) * u.size))
        crc[m], dist[m], clamped[m] = c & 0xFFFFFFFF, worst, nclamp / float(1 << 24)
    return crc, dist, clamped


def _run_crc(exe):
    r = subprocess.run([exe, "crc"], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.split("\n")
    assert lines[4] == "out-of-range 0 0"
    return {int(ln.split()[0]): int(ln.split()[1]) for ln in lines[:4]}


def test_header_conversion_equals_the_numpy_restatement_over_all_triples(harness, all_triples_crc):
    assert _run_crc(harness) == all_triples_crc[0]


def test_header_conversion_under_sanitizers(harness_san, all_triples_crc):
    assert _run_crc(harness_san) == all_triples_crc[0]


def test_tables_are_within_one_of_the_exact_matrices_and_most_triples_clamp(all_triples_crc):
    """the "1" re-derived: over all 2^24 triples no channel of the integer formula is further than 1 from the exact ITU matrix (binary64,
    rounded, clamped) — and it is not 0: the tables are 8-bit fixed point.  Most uniformly random triples clamp on some channel (about
    84 % for the limited-range matrices, about 76 % for the full-range ones).  What the raw_noise cases need is >= 50 % per case: the
    smallest case that is asked for a fraction has 57 pixels in 29 chroma samples, whose fraction has a standard deviation under
    sqrt(0.25 / 29) = 9 %, so a population of >= 60 % is demanded here; the cases themselves are checked one by one below."""
    _, dist, clamped = all_triples_crc
    assert dist == {0: 1, 1: 1, 2: 1, 3: 1}
    for m in range(4):
        assert clamped[m] >= 0.60, (m, clamped[m])


def test_restatement_spot_values():
    """a few values by hand: black, white and the primaries' neighbourhood, limited and full range"""
    assert yc.convert(16, 128, 128, 0).tolist() == [0, 0, 0, 255] and yc.convert(235, 128, 128, 0).tolist() == [255, 255, 255, 255]
    assert yc.convert(0, 128, 128, 2).tolist() == [0, 0, 0, 255] and yc.convert(255, 128, 128, 3).tolist() == [255, 255, 255, 255]
    assert yc.convert(81, 90, 240, 0).tolist() == [255, 0, 0, 255]   # BT.601 red: (81 - 16) 298 + 409 112 + 128 = 65306 >> 8 = 255
    # BT.709, all zero: C = -16 298 = -4768; R = (-4768 - 459 128 + 128) >> 8 < 0; G = (-4768 + 55 128 + 136 128 + 128) >> 8 = 19808 >> 8 = 77; B < 0
    assert yc.convert(0, 0, 0, 1).tolist() == [0, 77, 0, 255]
    assert (-1 >> 8, np.int32(-1) >> 8) == (-1, -1)                  # >> is arithmetic in both restatements


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------

PLAN_OK = [
    # w h fmt mat y_pitch c_pitch stride n -> fields
    ((97, 81, 0, 0, 0, 0, 0, 1), dict(cw=49, ch=41, c_row=98, y_pitch=97, c_pitch=98, stride=0, y_extent=97 * 81, c_extent=98 * 41, packed_frame=97 * 81 + 2 * 49 * 41)),
    ((97, 81, 1, 3, 0, 0, 0, 1), dict(cw=49, ch=41, c_row=49, y_pitch=97, c_pitch=49, stride=0, y_extent=97 * 81, c_extent=49 * 41, packed_frame=97 * 81 + 2 * 49 * 41)),
    ((1, 1, 0, 0, 0, 0, 0, 1), dict(cw=1, ch=1, c_row=2, y_extent=1, c_extent=2, packed_frame=3)),
    ((2, 2, 1, 0, 0, 0, 0, 1), dict(cw=1, ch=1, c_row=1, y_extent=4, c_extent=1, packed_frame=6)),
    ((1, 57, 0, 1, 0, 0, 0, 1), dict(cw=1, ch=29, y_extent=57, c_extent=58, packed_frame=57 + 58)),
    ((61, 1, 1, 2, 0, 0, 0, 1), dict(cw=31, ch=1, y_extent=61, c_extent=31, packed_frame=61 + 62)),
    ((1920, 1080, 0, 1, 0, 0, 3110400, 8), dict(cw=960, ch=540, y_extent=7 * 3110400 + 1920 * 1080, c_extent=7 * 3110400 + 1920 * 540, packed_frame=3110400)),
    # pitches: the extent ends with the last ROW, not with a whole pitch
    ((97, 81, 0, 0, 110, 104, 0, 1), dict(y_pitch=110, c_pitch=104, y_extent=110 * 80 + 97, c_extent=104 * 40 + 98)),
    ((97, 81, 1, 0, 110, 55, 20000, 3), dict(y_pitch=110, c_pitch=55, stride=20000, y_extent=2 * 20000 + 110 * 80 + 97, c_extent=2 * 20000 + 55 * 40 + 49)),
    ((97, 81, 0, 0, 0, 0, 12345, 1), dict(stride=0)),  # one frame: the stride is never added, so it is not looked at
    ((16384, 16384, 1, 0, 0, 0, 0, 1), dict(cw=8192, ch=8192, packed_frame=16384 * 16384 * 3 // 2)),
]
PLAN_BAD = [
    ((97, 81, 0, 0, 0, 0, 0, 0), 1), ((97, 81, 0, 0, 0, 0, 0, -2), 1),                                 # count
    ((0, 81, 0, 0, 0, 0, 0, 1), 2), ((97, -1, 0, 0, 0, 0, 0, 1), 2), ((16385, 8, 0, 0, 0, 0, 0, 1), 2), ((8, 16385, 1, 0, 0, 0, 0, 1), 2),  # size
    ((97, 81, 2, 0, 0, 0, 0, 1), 3), ((97, 81, -1, 0, 0, 0, 0, 1), 3),                                 # format
    ((97, 81, 0, 4, 0, 0, 0, 1), 4), ((97, 81, 1, -1, 0, 0, 0, 1), 4),                                 # matrix
    ((97, 81, 0, 0, 96, 0, 0, 1), 5), ((97, 81, 0, 0, 1 << 33, 0, 0, 1), 5),                           # Y pitch
    ((97, 81, 0, 0, 0, 97, 0, 1), 6), ((97, 81, 0, 0, 0, 99, 0, 1), 6), ((97, 81, 1, 0, 0, 48, 0, 1), 6), ((97, 81, 1, 0, 0, 1 << 33, 0, 1), 6),  # chroma pitch (NV12: < 98, odd)
    ((97, 81, 0, 0, 0, 0, 0, 2), 7), ((97, 81, 0, 0, 0, 0, 97 * 81 - 1, 2), 7), ((97, 81, 0, 0, 0, 0, 97 * 81 + 2, 2), 7),  # stride: none, < a Y plane, odd (NV12)
    ((2, 4, 1, 0, 0, 64, 16, 2), 7), ((97, 81, 1, 0, 0, 0, 1 << 33, 2), 7),                             # stride < a chroma plane at its pitch; absurd
]


def _run_plan(exe, tmp_path, cases):
    path = str(tmp_path / "plan_cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(v) for v in c) for c in cases) + "\n")
    r = subprocess.run([exe, "plan", path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_of_odd_sizes_and_refusal_of_malformed_descriptions(harness, harness_san, tmp_path, which):
    exe = harness if which == "plain" else harness_san
    got = _run_plan(exe, tmp_path, [c for c, _ in PLAN_OK] + [c for c, _ in PLAN_BAD])
    for (case, want), g in zip(PLAN_OK, got):
        assert g["status"] == 0, (case, g)
        w, h = case[0], case[1]
        assert (g["cw"], g["ch"]) == yc.chroma_dims(w, h) and g["packed_frame"] == yc.frame_bytes(w, h), (case, g)
        for k, v in want.items():
            assert g[k] == v, (case, k, g[k], v)
    seen = set()
    for (case, status), g in zip(PLAN_BAD, got[len(PLAN_OK):]):
        assert g["status"] == status and set(g) == {"status", "message"} and len(g["message"]) > 10, (case, g)
        seen.add(status)
    assert seen == set(range(1, 8))  # every refusal the plan knows


# ---- input sufficiency: conditions, not measurements ------------------------------------------------------------------------------------------

def gpu_ratio_cases():
    return [r for r in ic.RATIOS if r[0][0] * r[0][1] <= 400 * 400] + [((1920, 1080), (320, 240))]


def test_from_rgb_content_is_in_gamut_and_raw_noise_is_not():
    """every from_rgb case the GPU tests use has >= 90 % of its converted pixels unclamped (so the matrix, not the clamp, decides their
    bytes); every raw_noise case has >= 50 % clamped on some channel; the extremes grid holds all 216 triples at the size that can"""
    for (sw, sh), _ in gpu_ratio_cases():
        for fmt in (yc.NV12, yc.I420):
            for matrix in (0, 1):
                for kind in ("smooth", "noise"):
                    if sw * sh < 64:
                        continue  # (a handful of pixels: a fraction says nothing; the GPU test still draws them)
                    p = yc.from_rgb_frames(kind, sw, sh, 1, fmt, matrix, seed=sw + 7 * sh)[0]
                    y, u, v = yc.split(p, fmt)
                    iy, ix = np.arange(sh)[:, None] >> 1, np.arange(sw)[None, :] >> 1
                    frac = yc.clamped_fraction(y, u[iy, ix], v[iy, ix], matrix)
                    assert frac <= 0.10, ((sw, sh), fmt, matrix, kind, frac)
    for (w, h) in ((97, 81), (1, 57), (61, 1)):
        for fmt in (yc.NV12, yc.I420):
            for matrix in range(4):
                y, u, v = yc.split(yc.raw_noise(w, h, fmt, 5 + w), fmt)
                iy, ix = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
                assert yc.clamped_fraction(y, u[iy, ix], v[iy, ix], matrix) >= 0.50, ((w, h), fmt, matrix)
    want = {(a, b, c) for a in yc.EXTREME_VALUES for b in yc.EXTREME_VALUES for c in yc.EXTREME_VALUES}
    for fmt in (yc.NV12, yc.I420):
        assert yc.triples_of(yc.extremes(97, 81, fmt), 97, 81, fmt) == want


def test_to_rgba_sites_chroma_by_the_frame_and_formats_agree():
    """pixel (x, y) takes chroma sample (x >> 1, y >> 1); NV12 and I420 of the same samples give the same frame; pack / unpack round-trip"""
    w, h = 7, 5
    nv = yc.raw_noise(w, h, yc.NV12, 3)
    y, u, v = yc.split(nv, yc.NV12)
    i4 = yc.join(y, u, v, yc.I420)
    a, b = yc.to_rgba(nv, w, h, yc.NV12, 1), yc.to_rgba(i4, w, h, yc.I420, 1)
    assert np.array_equal(a, b)
    for (px, py) in ((0, 0), (1, 1), (2, 0), (6, 4), (5, 3)):
        assert a[py, px].tolist() == yc.convert(y[py, px], u[py >> 1, px >> 1], v[py >> 1, px >> 1], 1).tolist()
    for fmt, planes in ((yc.NV12, nv), (yc.I420, i4)):
        buf = yc.pack(planes)
        assert len(buf) == yc.frame_bytes(w, h)
        for p, q in zip(planes, yc.unpack(buf, w, h, fmt)):
            assert np.array_equal(p, q)


def test_rect_cases_cross_and_share_chroma_samples_and_outside_starts_at_the_next_sample():
    """Every rect of the GPU rect cases with an odd origin (and at least two columns: a 1-pixel-wide rect has ONE tap column, so there
    is no pair of taps to speak of) has a destination pixel whose two column taps fall into different chroma samples and one whose taps
    share a sample, from the numpy twin of rs_tap; the same for rows of rects with an odd top.  And outside_filled replaces exactly what
    the draw of the rect must not read: the converted frame inside the rect is unchanged, every Y pixel outside the rect and every
    chroma sample outside chroma_span differs somewhere — while the straddling samples, which belong to both sides, are kept."""
    nodd = 0
    for (sw, sh), (dw, dh) in yc.RECT_CASES:
        base = yc.from_rgb_frames("smooth", sw, sh, 1, yc.NV12, 0, seed=20)[0]
        for k, rect in enumerate(ic.rects_for(sw, sh)):
            x, y, w, h = rect
            for origin, extent, d in ((x, w, dw), (y, h, dh)):
                if origin & 1 and extent >= 2:
                    a, b = yc.taps(d, extent, origin)
                    assert ((a >> 1) != (b >> 1)).any(), (rect, origin)
                    assert ((a >> 1) == (b >> 1)).any(), (rect, origin)
                    nodd += 1
            filled = yc.outside_filled(base, sw, sh, yc.NV12, rect, 30 + k)
            ra, rb = yc.to_rgba(base, sw, sh, yc.NV12, 0), yc.to_rgba(filled, sw, sh, yc.NV12, 0)
            assert np.array_equal(ra[y:y + h, x:x + w], rb[y:y + h, x:x + w]), rect
            cx0, cx1, cy0, cy1 = yc.chroma_span(rect)
            assert (cx0, cy0) == (x // 2, y // 2) and cx1 == (x + w - 1) // 2 and cy1 == (y + h - 1) // 2
            yo, uo, vo = yc.split(base, yc.NV12)
            yf, uf, vf = yc.split(filled, yc.NV12)
            assert np.array_equal(uo[cy0:cy1 + 1, cx0:cx1 + 1], uf[cy0:cy1 + 1, cx0:cx1 + 1]) and np.array_equal(vo[cy0:cy1 + 1, cx0:cx1 + 1], vf[cy0:cy1 + 1, cx0:cx1 + 1])
            mask = np.ones((sh, sw), dtype=bool)
            mask[y:y + h, x:x + w] = False
            if mask.any():
                assert (yo[mask] != yf[mask]).mean() > 0.9, rect
            cmask = np.ones(uo.shape, dtype=bool)
            cmask[cy0:cy1 + 1, cx0:cx1 + 1] = False
            if cmask.any():
                assert ((uo[cmask] != uf[cmask]) | (vo[cmask] != vf[cmask])).mean() > 0.9, rect
    assert nodd >= 8


# ---- every layer has the entry points -------------------------------------------------------------------------------------------------------

def test_new_entry_points_exist_at_every_layer():
    """fails without the feature: the library, the header, native.py, the API, the addon and INTEGRATION.md all name the two exports"""
    import ctypes as C

    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), f"libheadtrackr_hip.so does not export {name}"
        assert name in native.SYMBOLS
        assert f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "typedef struct ht_yuv_frames" in header
    # the ctypes struct mirrors the C one: three pointers, three size_t, four int32
    assert C.sizeof(native.YUV_FRAMES) == 64 and native.YUV_FRAMES.width.offset == 48 and native.YUV_FRAMES.matrix.offset == 60
    assert (native.HT_YUV_NV12, native.HT_YUV_I420) == (yc.NV12, yc.I420) and [native.YUV_MATRICES[k] for k in yc.MATRIX_NAMES] == [0, 1, 2, 3]
    assert L.ht_draw_frames_yuv_device(None, None, 0, None, None, 0) < 0  # all-zero arguments: a status, never a crash
    assert L.ht_draw_frames_yuv(None, None, 0, 0, 0, 0, 0, 0, None) < 0
    assert L.ht_abi_version() == 2
    assert callable(Context.draw_frames_yuv) and callable(Context.draw_frames_yuv_device)
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    exported = set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    assert set(NEW_ADDON) <= exported
    addon = build.build_addon()
    if addon is None or NODE is None:
        pytest.skip("node or its N-API headers are missing on this machine: the addon is not built")
    js = "const A = require(%r); console.log(JSON.stringify(%s.map(function (k) { return typeof A[k]; }).concat([A.YUV_NV12, A.YUV_I420])));" % (addon, json.dumps(list(NEW_ADDON)))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function"] * len(NEW_ADDON) + [0, 1]


def test_new_kernels_fit_their_budget_and_live_in_the_fourth_code_object():
    """code-object metadata and disassembly: k_draw_yuv<NV12> and <I420> have no spills and no scratch, stay within 64 VGPRs (8
    wavefronts per SIMD, like k_draw_frames) and the tile's 1.9 KB of LDS; no binary64 product is contracted, 16 round-half-even
    conversions (4 rows x 4 channels) and 4 dword stores each; the unit is a file of its own, included by ht_ingest.hip, whose kernels
    carry none of the fingerprint's markers and live in the one code object besides the three recorded ones — which are byte-identical
    to profiles/traffic.json's build; ig_channel's text exists once."""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr, dz = _tool("kernel_resources"), _tool("disasm")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    mine = sorted(k for k in res if k.startswith("k_draw_yuv"))
    assert mine == ["k_draw_yuv<0>", "k_draw_yuv<1>"], mine
    for name, mangled in zip(mine, ("k_draw_yuvILi0", "k_draw_yuvILi1")):
        r = res[name]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 4096, (name, r)
        txt = dz.disasm(mangled)
        assert txt, name
        ops = [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]
        assert not any(o.startswith("v_fma") or o.startswith("scratch_") for o in ops), name
        assert sum(o.startswith("v_rndne_f64") for o in ops) == 16 and sum(o.startswith("global_store_dword") for o in ops) == 4, name
        assert sum(o == "s_barrier" for o in ops) == 1, name
        for marker in fingerprint.UNITS.values():
            assert marker.decode() not in name and marker.decode() not in mangled
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    assert build.HIP_SOURCES == ["ht_context.hip", "ht_pyramid.hip", "ht_scan.hip", "ht_camshift.hip", "ht_backproject.hip", "ht_allgather.hip"]
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_draw_yuv" in o]
    assert len(home) == 1 and b"k_draw_frames" in home[0]
    for marker in fingerprint.UNITS.values():
        assert marker not in home[0], marker
    ingest, yuv = open(os.path.join(CSRC, "ht_ingest.hip")).read(), open(os.path.join(CSRC, "ht_ingest_yuv.hip")).read()
    assert '#include "ht_ingest_yuv.hip"' in ingest and '#include "ht_yuv_plan.h"' in yuv
    assert ingest.count("uint32_t ig_channel(") == 1 and "ig_channel(" in yuv and "uint32_t ig_channel(" not in yuv and "__dmul_rn" not in yuv
    plan = open(os.path.join(CSRC, "ht_yuv_plan.h")).read()
    assert "hip/" not in plan and "__global__" not in plan


# ---- the JavaScript layer on the mock addon ---------------------------------------------------------------------------------------------------

def js_cases():
    """(planes, w, h, fmt, matrix, rect | None, dw, dh): both formats, every matrix, odd sizes (an odd x odd NV12 frame is placed one byte
    into its device buffer), a rect with an odd origin"""
    out = []
    for k, (w, h, dw, dh, rect) in enumerate([(97, 81, 97, 81, None), (97, 81, 40, 30, None), (64, 48, 40, 30, None), (23, 23, 40, 30, (5, 3, 11, 13)),
                                             (1, 57, 40, 30, None), (61, 1, 40, 30, None), (2, 2, 3, 3, None), (96, 81, 40, 30, (3, 5, 89, 72))]):
        for fmt in (yc.NV12, yc.I420):
            matrix = (k + fmt) % 4
            planes = yc.raw_noise(w, h, fmt, 40 + k) if k % 2 else yc.from_rgb_frames("smooth", w, h, 1, fmt, matrix, seed=40 + k)[0]
            out.append((planes, w, h, fmt, matrix, rect, dw, dh))
    return out


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_draws_yuv_sources_through_the_yuv_entry_point(tmp_path):
    """tests/js/ingest_yuv_cpu.js on tests/js/mock_addon_yuv.js: ccv.drawFrames on NV12 / I420 video-like objects and ccv.DeviceBatch with
    sourceFormat give the canvases of the numpy / oracle expectation; an RGBA video and an RGBA batch still log the RGBA entry point"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from oracle import ht_oracle as ho
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    cases, job = js_cases(), {"cases": []}
    for k, (planes, w, h, fmt, matrix, rect, dw, dh) in enumerate(cases):
        fn = tmp_path / f"s{k}.yuv"
        yc.pack(planes).tofile(fn)
        job["cases"].append(dict(file=str(fn), w=w, h=h, format=fmt, matrix=matrix, dw=dw, dh=dh, rect=list(rect) if rect else None))
    # the batch: 333 x 217 NV12 (odd x odd: frames one byte into the buffer and one byte further apart), 2 frames
    bw, bh, bdw, bdh, bn = 333, 217, 160, 120, 2
    frames = yc.from_rgb_frames("smooth", bw, bh, bn, yc.NV12, 1, seed=9)
    np.concatenate([yc.pack(p) for p in frames]).tofile(tmp_path / "batch.yuv")
    want = [yc.expected(p, bw, bh, yc.NV12, 1, None, bdw, bdh) for p in frames]
    for f, wnt in enumerate(want):
        wnt.tofile(tmp_path / f"batch_expect{f}.raw")
    assert ho.whitebalance(want[0]) != ho.whitebalance(want[1])
    job["batch"] = dict(file=str(tmp_path / "batch.yuv"), n=bn, w=bw, h=bh, format=yc.NV12, matrix=1, dw=bdw, dh=bdh, expect=[str(tmp_path / f"batch_expect{f}.raw") for f in range(bn)])
    rgba = ic.noise(64, 48, 3)
    rgba.tofile(tmp_path / "rgba.raw")
    job["rgba"] = dict(file=str(tmp_path / "rgba.raw"), w=64, h=48, dw=40, dh=30)
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "ingest_yuv_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["canvas_crc"] == [ic.crc(yc.expected(p, w, h, fmt, m, rect, dw, dh)) for p, w, h, fmt, m, rect, dw, dh in cases]
    assert out["rgba_crc"] == ic.crc(ic.expected(rgba, None, 40, 30))
    assert out["device_checks"] == len(cases) and out["batch_checks"] == 4 and out["rgba_checks"] == 2 and out["refusals"] == 5

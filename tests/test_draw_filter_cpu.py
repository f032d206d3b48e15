"""CPU-side checks of the prefiltered draw list (ht_draw_list_filtered_device / ht_draw_filter_factors): the host plan in
headtrackr_amd/csrc/ht_draw_filter_plan.h against the Python restatement of tests/draw_filter_cases.py, plain and under AddressSanitizer +
UBSan, as a program of its own; the consequences the rule states (factor 1 is the unfiltered draw, exact ratios are the integer box mean of
the source, a checkerboard's alias goes away); the scenes the GPU tests draw, proved to cover what those tests claim; the kernels' budget
and their neighbours' unchanged resources; the entry points at every layer; the addon shim on a recording stub and the JavaScript facade on
a mock addon.  No compute calls (no GPU here).  Without the feature every test but the restatement's own fails."""
import ctypes as C
import importlib.util
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import draw_filter_cases as dfc
import draw_list_cases as dl
import ingest_cases as ic
import yuv_cases as yc
from conftest import GOLDEN, ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
EXPORTS = ("ht_draw_list_filtered_device", "ht_draw_filter_factors")
N_RANDOM = 20000
LDS_BOUND = 8 * (64 + 16) * 24  # the fine taps of a 64 x 16 tile at factor 8, 24 bytes each


# ---- the plan header ------------------------------------------------------------------------------------------------------------------------

def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("draw_filter_plan") / ("draw_filter_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "draw_filter_plan_harness.cc"), "-o", exe])
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
    """the edge table and the seeded random entries, with the restatement's answer for each: computed once"""
    cs = dfc.edge_cases() + dfc.random_cases(N_RANDOM)
    return cs, np.array([dfc.want_of(c) for c in cs], dtype=np.int64)


def test_edge_table_covers_what_it_claims():
    """from the restatement alone: sizes 1 and 16384, canvases 1 and beyond 1024, the factor's step at exact multiples of the canvas and one
    either side, every factor and every max_factor, max_factor 0 and 9, every refusal of the plan at entry 0 and at entry 5"""
    cs = dfc.edge_cases()
    want = {c: dfc.want_of(c) for c in cs}
    ok = {c: v for c, v in want.items() if v[0] == dfc.OK}
    assert {1, 16384} <= {c[8] for c in ok} and {1, 16384} <= {c[9] for c in ok} and {1, 1024, 1025, 16384} <= {c[5] for c in ok} and 2049 in {c[6] for c in ok}
    assert {v[2] for v in ok.values()} == set(range(1, 9)) == {v[3] for v in ok.values()} and {c[7] for c in ok} == set(range(1, 9))
    for (W, k) in ((70, 3), (40, 8), (3, 5)):
        below, at, above = [next(v for c, v in ok.items() if c[10] == dl.RGBA and c[8] == k * W + d and c[5] == W and c[7] == 8) for d in (-1, 0, 1)]
        assert (below[2], at[2], above[2]) == (k, k, min(8, k + 1))
        assert at[4] == dfc.bits(1.0) and below[4] != dfc.bits(1.0)  # at an exact multiple the fine ratio is exactly 1
    assert any(c[8] > 8 * c[5] and v[2] == 8 for c, v in ok.items()) and any(c[8] > c[7] * c[5] and v[2] == c[7] < 8 for c, v in ok.items())  # limited by max_factor
    assert any(v[6:10] == (3, 5, 210, 210) for v in ok.values())  # the factors follow the RECT
    refused = {v[0] for v in want.values()} - {dfc.OK}
    assert refused == set(range(dfc.BAD_CANVAS, dfc.BAD_RECT + 1)) | {dfc.BAD_FACTOR}
    assert {c[7] for c, v in want.items() if v[0] == dfc.BAD_FACTOR} >= {0, 9, -1}
    assert all(v[1] == -1 for v in want.values() if v[0] in (dfc.BAD_FACTOR, dfc.BAD_CANVAS, dfc.OK))
    for st in range(dfc.BAD_FORMAT, dfc.BAD_RECT + 1):
        assert {v[1] for v in want.values() if v[0] == st} == {0, 5}, st  # named at entry 0 of 1 and at entry 5 of 6


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_header_equals_the_restatement(harness, harness_san, cases, tmp_path, which):
    """every case of the edge table and 20 000 seeded random entries: status, offending entry, factors, the bits of the two fine ratios, the
    rect, the effective pitches and the chroma width of the header equal the restatement's"""
    cs, want = cases
    assert len(cs) >= N_RANDOM + 1000
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(dfc.pack_cases(cs))
    r = subprocess.run([harness if which == "plain" else harness_san, src, dst], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.int64).reshape(-1, 13)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(cs[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    rnd = want[-N_RANDOM:]
    assert 0.05 * N_RANDOM < int((rnd[:, 0] != 0).sum()) < 0.25 * N_RANDOM  # refusals among the random ones, of several kinds
    assert len(set(rnd[rnd[:, 0] != 0][:, 0].tolist())) >= 7
    for f in range(1, 9):
        assert int((rnd[:, 2] == f).sum()) > 0.01 * N_RANDOM and int((rnd[:, 3] == f).sum()) > 0.01 * N_RANDOM, f  # no monoculture


# ---- consequences of the rule -----------------------------------------------------------------------------------------------------------------

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


def test_factor_1_is_the_unfiltered_draw():
    """max_factor 1, a source not larger than the canvas and an upscale give the unfiltered expectation, for all three formats"""
    W, H = 40, 30
    for src in (dl.Source(dl.RGBA, 117, 95, seed=5), dl.Source(yc.NV12, 117, 95, seed=6, matrix=1), dl.Source(yc.I420, 23, 23, seed=7, matrix=2),
                dl.Source(dl.RGBA, 40, 30, seed=8)):
        for rect in (None, (3, 5, 20, 17)):
            got, f = dfc.expected(src, rect, W, H, 1)
            assert f == (1, 1) and np.array_equal(got, src.expected(rect, W, H))
            got, f = dfc.expected(src, rect, W, H, 8)
            small = rect is not None or (src.w <= W and src.h <= H)
            assert (f == (1, 1)) == small
            assert not small or np.array_equal(got, src.expected(rect, W, H))
            assert small or not np.array_equal(got, src.expected(rect, W, H))


def test_exact_ratios_are_the_integer_box_mean_of_the_source():
    """where sw == Nx W and sh == Ny H the fine frame is the source block itself (every tap weight 0), so the output is the exact integer box
    mean of the source: RGBA, and NV12 / I420 through the declared conversion (the mean is taken of the converted pixels)"""
    for src in (dl.Source(dl.RGBA, 64, 48, seed=11), dl.Source(yc.NV12, 64, 48, seed=12, matrix=1), dl.Source(yc.I420, 64, 48, seed=13, matrix=2)):
        for (rect, W, H) in (((0, 0, 64, 48), 8, 6), ((3, 5, 20, 12), 10, 4), ((1, 1, 48, 6), 6, 6), ((7, 0, 8, 48), 8, 6), ((0, 0, 14, 35), 2, 5)):
            got, (nx, ny) = dfc.expected(src, rect, W, H, 8)
            assert (nx, ny) == (rect[2] // W, rect[3] // H) and nx * ny > 1
            assert np.array_equal(src.expected(rect, nx * W, ny * H), src.rgba[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]])  # the fine frame IS the block
            assert np.array_equal(got, _box_mean(src.rgba, rect, nx, ny)), (src.fmt, rect, W, H)
        # limited by max_factor the fine frame is a resampling again, and the output no box mean of the source
        got, f = dfc.expected(src, (1, 1, 48, 6), 6, 6, 3)
        assert f == (3, 1) and not np.array_equal(got, dfc.expected(src, (1, 1, 48, 6), 6, 6, 8)[0])
    # the .5 ties of an exact 2 : 1 draw round UP in the mean (the unfiltered draw rounds them to even)
    t = ic.ties(80, 60, 3)
    got, f = dfc.expected_rgba(t, None, 40, 30, 8)
    plain = ic.expected(t, None, 40, 30)
    assert f == (2, 2) and np.array_equal(got, _box_mean(t, (0, 0, 80, 60), 2, 2)) and (got >= plain).all() and (got > plain).any()


def test_a_checkerboard_alias_goes_away():
    """the failure the feature removes, on the test's own input: a 1-pixel checkerboard drawn 120 x 90 -> 40 x 30 (3 : 1) is bytes {0, 255} in
    the unfiltered rule, a full-contrast alias of a source whose mean is gray, and stays inside [113, 142] filtered; at 5 : 1 inside
    [122, 133]; noise loses two thirds of its standard deviation"""
    board = dfc.checkerboard(120, 90)
    plain = ic.expected(board, None, 40, 30)
    assert set(np.unique(plain[..., :3]).tolist()) == {0, 255}
    got, f = dfc.expected_rgba(board, None, 40, 30, 8)
    assert f == (3, 3) and 113 <= int(got[..., :3].min()) and int(got[..., :3].max()) <= 142 and (got[..., 3] == 255).all()
    board = dfc.checkerboard(200, 150)
    assert set(np.unique(ic.expected(board, None, 40, 30)[..., :3]).tolist()) == {0, 255}
    got, f = dfc.expected_rgba(board, None, 40, 30, 8)
    assert f == (5, 5) and 122 <= int(got[..., :3].min()) and int(got[..., :3].max()) <= 133
    noise = ic.noise(240, 135, 3)
    got, f = dfc.expected_rgba(noise, None, 40, 30, 8)
    assert f == (6, 5) and ic.expected(noise, None, 40, 30).std() > 35 and got.std() < 15


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------

def test_scenes_cover_what_the_gpu_tests_claim():
    """from the scenes alone: every Nx and every Ny in 1..8, the corners (1, 8) and (8, 1), entries limited by max_factor, all three formats and
    all four matrices for YUV, odd YUV sizes, pitches beyond a row on every plane, rects 1 and 2 pixels wide, and entries whose last rect
    column is the `a` tap of a fine column (the bodies then read the tap pair one pixel to the left); the canvases and list lengths the
    issue names; no source wider than 8 x 70 or taller than 8 x 30"""
    seen, limited, fmts, mats, odd, widths, last_col = set(), 0, set(), set(), 0, set(), 0
    pads = set()
    for name in dfc.SCENES:
        (W, H), srcs, plan = dfc.scene(name)
        assert (name == "long" and len(plan) == 70) or 3 <= len(plan) <= 12, name
        assert name == "small" or {k for k, _ in plan} == set(range(len(srcs))), name  # every source is drawn ("small" takes three of "long"'s)
        assert all(s.w <= 560 and s.h <= 240 for s in srcs)  # 8 x the widest and 8 x the tallest canvas
        for k, rect in plan:
            s = srcs[k]
            sx, sy, sw, sh = rect if rect else (0, 0, s.w, s.h)
            nx, ny = dfc.factors(sw, sh, W, H, 8)
            seen.add((nx, ny))
            limited += sw > 8 * W or sh > 8 * H
            fmts.add(s.fmt)
            widths.add(sw)
            if s.fmt != dl.RGBA:
                mats.add((s.fmt, s.matrix))
                odd += s.w % 2 == 1 and s.h % 2 == 1
                pads.add((s.fmt, s.pad0 > 0, s.pad1 > 0))
            else:
                pads.add((s.fmt, s.pad0 > 0))
            a, _b = yc.taps(nx * W, sw, sx)
            last_col += sw >= 2 and bool((a == sx + sw - 1).any())
    assert {(70, 19), (40, 30), (3, 4), (1, 1)} == {dfc.scene(n)[0] for n in dfc.SCENES}
    assert {f[0] for f in seen} == set(range(1, 9)) == {f[1] for f in seen}, sorted(seen)
    assert {(1, 8), (8, 1), (1, 1), (8, 8)} <= seen and limited >= 3
    assert fmts == {dl.RGBA, yc.NV12, yc.I420} and {m for _, m in mats} == {0, 1, 2, 3} and odd >= 4
    assert {f for f, _ in mats} == {yc.NV12, yc.I420}
    assert {(dl.RGBA, True), (yc.NV12, True, True), (yc.I420, True, True)} <= pads
    assert {1, 2} <= widths and last_col >= 10
    # at max_factor 3 and 2 the limited entries multiply, and at 1 every entry is the unfiltered draw
    for mf in (3, 2, 1):
        f = {dfc.factors(*dfc.size_of((srcs[k].w, srcs[k].h), rect), *dfc.scene(n)[0], mf) for n in dfc.SCENES for srcs, plan in [dfc.scene(n)[1:]] for k, rect in plan}
        assert max(v for p in f for v in p) == mf and (1, 1) in f
    # the twin-context lists have ONE factor pair each and are no exact ratio
    for (nx, ny), (W, H) in (((2, 2), (40, 30)), ((3, 5), (40, 30)), ((8, 8), (70, 19))):
        for s in dfc.uniform_list(nx, ny, W, H):
            assert dfc.factors(s.w, s.h, W, H, 8) == (nx, ny) and (s.w != nx * W or s.h != ny * H)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ops(txt):
    return [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]


def test_mean_kernels_fit_their_budget_and_leave_their_neighbours_alone():
    """code-object metadata and disassembly of k_draw_list_mean_tile<RPT> (RPT 1: the 64 x 4 tile every call takes; RPT 4: the 64 x 16 tile behind
    the context option draw_filter_rows = 16, kept for the measurement): no spills, no scratch, the fine taps' 15 / 13 KB of LDS (the bound DESIGN.md §2.3.8 states), 256 threads, <= 128 VGPRs (the
    small tile <= 64), one barrier, no flat or buffer access, the descriptor and the factors by scalar loads, the binary64 blend with
    nothing contracted, one rounding per channel of a thread's samples in each of the three bodies, no division on the device (the fine
    ratios come from the host).  Every OTHER kernel of that code object has the registers, LDS, scratch and spills it had before the
    feature (tests/golden/draw_filter_neighbours.json, recorded from the parent's build); the pyramid, scan and camshift code objects are
    byte-identical to profiles/traffic.json's build; the pixel bodies are the shared text"""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr, dz = _tool("kernel_resources"), _tool("disasm")
    raw = kr.kernel_resources()
    res = {kr.short(k): v for k, v in raw.items() if "vgpr_count" in v}
    names = ["k_draw_list_mean_tile<1>", "k_draw_list_mean_tile<4>"]
    assert sorted(k for k in res if "k_draw_list_mean_tile" in k) == names
    for name in names:
        r, rpt = res[name], int(name[-2])
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= (128 if rpt == 4 else 64) and r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["group_segment_fixed_size"] == 8 * (64 + 4 * rpt) * 24 <= LDS_BOUND, (name, r)
        for marker in fingerprint.UNITS.values():
            assert marker.decode() not in name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "2.3.8" in design and "15 360" in design[design.index("2.3.8"):] and "13 056" in design[design.index("2.3.8"):]
    for mangled, rpt in (("k_draw_list_mean_tileILi1E", 1), ("k_draw_list_mean_tileILi4E", 4)):
        ops = _ops(dz.disasm(mangled))
        assert ops, mangled
        assert not any(o.startswith(("scratch_", "flat_", "buffer_")) for o in ops) and sum(o == "s_barrier" for o in ops) == 1
        head, body = ops[:ops.index("s_barrier")], ops[ops.index("s_barrier"):]
        assert any(o.startswith("s_load_dword") for o in head) and not any(o.startswith("global_load") for o in head)  # the descriptor: scalar loads only
        assert sum(o.startswith("v_rndne_f64") for o in body) == 3 * 4 * rpt
        assert not any(o.startswith(("v_fma_f64", "v_mad_f", "v_mac_f", "v_div_")) for o in ops)
        assert any(o == "global_load_dwordx2" for o in body) and any(o == "global_load_ushort" for o in body) and any(o == "global_store_dword" for o in body)
    # the neighbours: the same code object, the same resources as on the parent
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_draw_list_mean_tile" in o]
    assert len(home) == 1 and b"k_draw_listE" in home[0] and b"k_cut_mean" in home[0] and b"k_draw_frames" in home[0]
    before = json.load(open(os.path.join(GOLDEN, "draw_filter_neighbours.json")))
    here = {kr.short(k): v for k, v in raw.items() if "vgpr_count" in v and k.encode() in home[0] and "k_draw_list_mean_tile" not in k}
    assert sorted(here) == sorted(before) and len(before) >= 40
    for k, v in before.items():
        assert here[k] == v, (k, here[k], v)
    assert here["k_draw_frames"]["vgpr_count"] <= 64 and here["k_draw_list"]["vgpr_count"] <= 64
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_draw_filter.hip", "ht_draw_filter_plan.h", "ht_draw_list.hip")}
    ingest = text["ht_ingest.hip"]  # the draw family's host path (ht_draw_calls.hip) is included last, behind this file's kernel and launcher
    assert ingest.rstrip().endswith('#include "ht_draw_calls.hip"')
    assert ingest.index('#include "ht_filter.hip"') < ingest.index('#include "ht_draw_filter.hip"') < ingest.index('#include "ht_draw_calls.hip"')
    # no second restatement of the blend or of the conversion: the kernel takes the ONE scaffold with its loops in front of each body
    f = text["ht_draw_filter.hip"]
    assert f.count("#define LP_PART 4  // LP_SCAFFOLD") == 1 and f.count("#define LP_EACH_PASS") == 1 and f.count('#include "ht_ingest_bodies.inc"') == 0
    assert "ig_channel(" not in f and "ht_yuv_to_rgba(" not in f and "__dmul_rn" not in f and f.count("ht_filter_pixel") == 1 and "fm_finish<RPT>(" in f
    plan = text["ht_draw_filter_plan.h"]
    assert "hip/" not in plan and "__global__" not in plan and "__device__" not in plan and "ht_draw_list_plan_entry(" in plan and "ht_filter_factor(" in plan
    assert "static_assert(sizeof(HtDrawDesc) == 104" in open(os.path.join(CSRC, "ht_draw_list_plan.h")).read()


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_at_every_layer_and_fail_loudly_without_a_device():
    """fails without the feature: the header, the library, native.py, the API, the addon, the facade and INTEGRATION.md all name the two
    exports; the C ABI answers all-zero arguments with a status; the factor function needs no context, refuses NULL and out-of-range
    arguments without writing, and equals the restatement; without a device a Context cannot be made, so no filtered draw can silently
    do nothing"""
    from headtrackr_amd import api
    from headtrackr_amd.api import Context, HtError

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "#define HT_ABI_VERSION 2" in header
    assert L.ht_draw_list_filtered_device(None, None, 0, 0, None, 0) == native.HT_ERR_INVALID
    src = (native.DRAW_SOURCE * 1)()
    assert L.ht_draw_list_filtered_device(None, src, 1, 8, None, 0) == native.HT_ERR_INVALID  # no context: a status, never a crash
    nx, ny = C.c_int32(-7), C.c_int32(-7)
    fn = L.ht_draw_filter_factors
    assert fn(1920, 1080, 320, 240, 8, None, C.byref(ny)) == native.HT_ERR_INVALID and fn(1920, 1080, 320, 240, 8, C.byref(nx), None) == native.HT_ERR_INVALID
    for args in ((0, 1080, 320, 240, 8), (1920, 16385, 320, 240, 8), (1920, 1080, 0, 240, 8), (1920, 1080, 320, -1, 8), (1920, 1080, 320, 240, 0), (1920, 1080, 320, 240, 9), (-1, -1, -1, -1, -1)):
        assert fn(*args, C.byref(nx), C.byref(ny)) == native.HT_ERR_INVALID, args
    assert (nx.value, ny.value) == (-7, -7)  # a refusal writes nothing
    assert fn(1920, 1080, 320, 240, 8, C.byref(nx), C.byref(ny)) == 0 and (nx.value, ny.value) == (6, 5)
    assert fn(16384, 16384, 1, 4096, 8, C.byref(nx), C.byref(ny)) == 0 and (nx.value, ny.value) == (8, 4)  # a canvas beyond 1024 is the geometry's to refuse, not the rule's
    sizes = [(1920, 1080), (1280, 720), (320, 240), (1, 1), (321, 241), (16384, 3)]
    for mf in range(1, 9):
        assert api.draw_filter_factors(sizes, 320, 240, mf).tolist() == [list(dfc.factors(w, h, 320, 240, mf)) for w, h in sizes]
    entries = [dict(width=1920, height=1080, rect=None), dict(width=1920, height=1080, rect=(420, 0, 1080, 1080)), dict(width=64, height=48)]
    assert api.draw_filter_factors(entries, 320, 240, 8).tolist() == [[6, 5], [4, 5], [1, 1]] and api.draw_filter_factors([], 320, 240).shape == (0, 2)
    for bad in (dict(max_factor=9), dict(max_factor=0)):
        with pytest.raises(HtError) as e:
            api.draw_filter_factors(sizes, 320, 240, **bad)
        assert "entry 0" in str(e.value)
    sig = inspect.signature(Context.draw_list)
    assert list(sig.parameters)[1:] == ["entries", "dst", "dst_stride", "prefilter"] and sig.parameters["prefilter"].default is None
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert {"drawListDevice", "drawListFilteredDevice", "drawFilterFactors"} <= set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    # ONE reader and ONE range check for both forms: the two addon functions are one-liners over draw_list_call, which reads the entries once
    assert napi.count("get_draw_entry(env, e, &srcs[i])") == 2 and napi.count("return draw_list_call(env, info, ") == 2 and napi.count("napi_value draw_list_call(") == 1
    assert napi.count("ht_draw_list_filtered_device(L.ctx, ") == 1 and napi.count("ht_draw_list_device(L.ctx, ") == 1
    facade = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    assert facade.count("A.drawListFilteredDevice(") == 2 and facade.count("A.drawListDevice(") == 2 and facade.count("A.drawFilterFactors(") == 1
    for f in ("README.md", "LABLOG.md", os.path.join("profiles", "README.md")):
        assert "ht_draw_list_filtered_device" in open(os.path.join(ROOT, f)).read() or "draw_filter" in open(os.path.join(ROOT, f)).read(), f
    if L.ht_device_count() == 0:
        with pytest.raises(HtError) as e:
            Context()
        assert "no CPU fallback" in str(e.value) or "no HIP device" in str(e.value)


def test_draw_list_prefilter_takes_the_filtered_call_and_none_todays():
    """on a recording stand-in for the library: prefilter=None issues exactly the ht_draw_list_device call it issues today, prefilter=N
    ht_draw_list_filtered_device with max_factor N and the same array, count, destination and stride"""
    from headtrackr_amd.api import Context

    calls = []

    class Lib:
        def __getattr__(self, name):
            return lambda *a: calls.append((name, a)) or 0

    c = Context.__new__(Context)
    c._lib, c._h, c.nframes = Lib(), 1234, 0
    e = [dict(format="nv12", width=23, height=23, p0=4096, p1=8192, matrix="bt709", rect=(1, 1, 21, 21)), dict(format="rgba", width=7, height=5, p0=12288)]
    c.draw_list(e, dst=65536, dst_stride=5000)
    c.draw_list(e, dst=65536, dst_stride=5000, prefilter=5)
    assert c.nframes == 0
    c.draw_list(e, prefilter=8)
    assert c.nframes == 2
    c.nframes = 0
    c.draw_list(e)
    assert c.nframes == 2
    assert [n for n, _ in calls] == ["ht_draw_list_device", "ht_draw_list_filtered_device", "ht_draw_list_filtered_device", "ht_draw_list_device"]
    assert calls[0][1][0] == 1234 and calls[0][1][2:] == (2, 65536, 5000) and calls[1][1][2:] == (2, 5, 65536, 5000) and calls[2][1][2:] == (2, 8, None, 0) and calls[3][1][2:] == (2, None, 0)
    for _, a in calls:
        arr = a[1]
        assert (arr[0].width, arr[0].format, arr[0].matrix, arr[0].rect.x, arr[0].rect.width, arr[1].format, arr[1].p0) == (23, 0, 1, 1, 21, 16, 12288)


# ---- the N-API shim against the recording stubs ----------------------------------------------------------------------------------------------

NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_max_factor_and_entries_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with tests/js/abi_stub.cc, draw_list_stub.cc and draw_filter_stub.cc: the successful calls of
    tests/js/draw_filter_addon.js reach ht_draw_list_filtered_device with maxFactor, the plane layout of a packed frame, offsets, rects, the
    destination offset and stride — what drawListDevice hands to ITS function for the same entries; a maxFactor outside 1..8 is a
    RangeError and every malformed call throws before the C ABI is reached; drawFilterFactors hands sizes, canvas and maxFactor on and
    returns an Int32Array; a refusal of the library comes back as an Error"""
    addon = str(tmp_path / "addon_df.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), *[os.path.join(ROOT, "tests", "js", f) for f in
                                                                                                        ("abi_stub.cc", "draw_list_stub.cc", "draw_filter_stub.cc")], "-o", addon])
    log, plain_log = str(tmp_path / "df.log"), str(tmp_path / "dl.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "draw_filter_addon.js"), addon], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HT_DF_STUB_LOG=log, HT_DL_STUB_LOG=plain_log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["kinds"] == ["function"] * 3
    calls = [json.loads(ln) for ln in open(log)]
    fb = 40 * 30 * 4
    whole = [0, 0, 0, 0]
    E_RGBA = dict(p0=0, p1=None, p2=None, pitch=[0, 0], size=[7, 5], format=16, matrix=0, rect=whole)
    E_NV12 = dict(p1=23 * 23, p2=None, pitch=[0, 0], size=[23, 23], format=0, matrix=1, rect=[1, 1, 21, 21])
    E_I420 = dict(p1=97 * 81, p2=97 * 81 + 49 * 41, pitch=[0, 0], size=[97, 81], format=1, matrix=3, rect=whole)
    E_TAIL = dict(p0=100000 - 6, p1=4, p2=5, pitch=[0, 0], size=[2, 2], format=1, matrix=0, rect=whole)
    assert (calls[0]["n"], calls[0]["max_factor"], calls[0]["dst_stride"], calls[0]["ctx"]) == (4, 8, 0, True)
    assert calls[0]["entries"] == [E_RGBA, dict(E_NV12, p0=1001), dict(E_I420, p0=4000), E_TAIL]
    dst0 = calls[0]["dst"]
    assert (calls[1]["n"], calls[1]["max_factor"], calls[1]["dst_stride"], calls[1]["dst"]) == (2, 3, fb + 48, dst0 + 4 - 1001)
    assert calls[1]["entries"] == [dict(E_NV12, p0=0), dict(E_RGBA, p0=-1001)]
    assert (calls[2]["n"], calls[2]["max_factor"], calls[2]["dst"]) == (1, 1, None) and calls[2]["entries"] == [dict(E_I420, p0=0)]
    assert len(calls) == 4 and calls[3]["n"] == 3  # the one the stub refuses; nothing malformed reached the C ABI
    plain = [json.loads(ln) for ln in open(plain_log)]
    assert len(plain) == 1 and plain[0]["n"] == 2 and plain[0]["dst"] == dst0 and plain[0]["entries"] == [E_RGBA, dict(E_NV12, p0=1001)]
    # the stub's factor function answers (width + canvas width, height + 10 maxFactor + canvas height): every argument arrived
    assert out["factors"] == [1920 + 320, 1080 + 80 + 240, 7 + 320, 5 + 80 + 240] and out["factorsKind"] == "Int32Array" and out["noFactors"] == []
    thrown = dict(out["thrown"])
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    kinds = {"too few arguments": "TypeError", "the plain arguments": "TypeError", "no context": "TypeError", "entries no array": "TypeError", "no entries": "RangeError",
             "maxFactor a string": "TypeError", "maxFactor 0": "RangeError", "maxFactor 9": "RangeError", "maxFactor -1": "RangeError", "entry no object": "TypeError",
             "entry without dev": "TypeError", "width a string": "TypeError", "rect a plain array": "TypeError", "frame beyond its buffer": "RangeError",
             "RGBA frame beyond its buffer": "RangeError", "destination too small": "RangeError", "destination offset beyond": "RangeError",
             "destination stride beyond": "RangeError", "dst a context": "TypeError", "stride a string": "TypeError", "the library refuses": "Error",
             "drawFilterFactors: too few arguments": "TypeError", "drawFilterFactors: sizes a plain array": "TypeError", "drawFilterFactors: sizes of three": "TypeError",
             "drawFilterFactors: maxFactor 9": "RangeError", "drawFilterFactors: maxFactor 0": "RangeError", "drawFilterFactors: canvas width 0": "RangeError",
             "drawFilterFactors: the library refuses": "RangeError"}
    assert set(thrown) == set(kinds)
    for what, kind in kinds.items():
        assert thrown[what].startswith(kind + ": "), (what, thrown[what])
    for mf in ("0", "9", "-1"):
        assert "maxFactor is 1..8" in thrown[f"maxFactor {mf}"]
    assert "ht_draw_list_filtered_device" in thrown["the library refuses"] and "status -1" in thrown["the library refuses"]


# ---- the JavaScript facade on the mock addon ----------------------------------------------------------------------------------------------------

JS_PREFILTERS = [8, 3, 1]


def js_feeds():
    """(source, rect) on a 20 x 15 canvas: all three formats, an odd x odd NV12 frame, an odd-origin rect, an upscale, a one-pixel-wide source"""
    return [(dl.Source(dl.RGBA, 160, 120, seed=81, content="smooth"), None), (dl.Source(yc.NV12, 91, 67, seed=82, matrix=1), None),
            (dl.Source(yc.I420, 97, 81, seed=83, matrix=2, content="raw"), (1, 1, 95, 79)), (dl.Source(yc.NV12, 96, 81, seed=84, matrix=3), (5, 3, 2, 2)),
            (dl.Source(dl.RGBA, 1, 5, seed=85), None), (dl.Source(yc.I420, 60, 45, seed=86, content="raw"), None)]


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_opts_prefilter_gives_the_rules_bytes_and_changes_nothing_without_it(tmp_path):
    """tests/js/draw_filter_cpu.js on tests/js/mock_addon_draw_filter.js: ccv.DeviceBatch with mixed opts.sources at depth 1 and 2.  Without
    opts.prefilter (absent, {}, null, undefined) drawList / drawListBound issue exactly the drawListDevice call they issue today and the
    canvases are the unfiltered expectation, before and after the filtered calls; with opts.prefilter 8, 3 and 1 they issue ONE
    drawListFilteredDevice call and nothing else, into the frame set asked for, the canvases are the restated block means, the bound
    frames feed the step functions, and drawFilterFactors gives the restated factors; malformed opts throw, and an addon without the
    function gives the rebuild-it error for opts.prefilter only"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    dw, dh = 20, 15
    feeds, job = js_feeds(), {"w": dw, "h": dh, "prefilters": JS_PREFILTERS, "feeds": []}
    for k, (s, rect) in enumerate(feeds):
        fn = tmp_path / f"feed{k}.raw"
        s.packed().tofile(fn)
        job["feeds"].append(dict(file=str(fn), width=s.w, height=s.h, format=dl.FORMAT_NAMES[s.fmt], matrix=yc.MATRIX_NAMES[s.matrix], rect=list(rect) if rect else None))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "draw_filter_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["refusals"] == 2 * 9
    plain = [ic.crc(s.expected(rect, dw, dh)) for s, rect in feeds]
    assert len(out["plain"]) == 2 * 4
    for g in out["plain"]:
        waited = ["drawListDeviceWaited"] if g["depth"] > 1 else []
        assert g["list"] == plain and g["bound"] == plain and g["listCalled"] == ["drawListDevice"] + waited and g["boundCalled"] == ["drawListDevice"], g
    assert len(out["filtered"]) == 2 * len(JS_PREFILTERS)
    seen = set()
    for g in out["filtered"]:
        want = [dfc.expected(s, rect, dw, dh, g["prefilter"]) for s, rect in feeds]
        crcs = [ic.crc(w) for w, _ in want]
        waited = ["drawListFilteredDeviceWaited"] if g["depth"] > 1 else []
        assert g["list"] == crcs and g["bound"] == crcs and g["untouched"] and g["stepped"], g
        assert g["listCalled"] == ["drawListFilteredDevice"] + waited and g["boundCalled"] == ["drawListFilteredDevice"] and g["factorsCalled"] == ["drawFilterFactors"], g
        assert g["factors"] == [v for _, f in want for v in f], g
        assert g["prefilter"] != 1 or crcs == plain  # factor 1: the unfiltered bytes
        seen |= {f for _, f in want}
    assert {(8, 8), (5, 5), (1, 1), (3, 3)} <= seen and any(nx != ny for nx, ny in seen), sorted(seen)
    assert [ic.crc(dfc.expected(s, rect, dw, dh, 8)[0]) for s, rect in feeds] != plain

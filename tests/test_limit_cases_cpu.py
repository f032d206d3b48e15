"""The inputs of tests/test_gpu_limits.py suffice — shown from the oracle alone, without a device: the hit lists are non-empty and reach
both ends of the long axis, the pyramids hold the strip planes and the undrawn variant canvases, the blobs sit at the far edge and stay
tracked, and the host-only planner (ASan + UBSan harness, `plan` mode with its check_plan invariants) accepts every limit geometry, the
16384 x 16384 canvas that no GPU test runs and the 16384 x 1 row included."""
import json
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

import limit_cases as lc
import pyramid_cases as pc
from oracle import ht_oracle as ho

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
EDGE = 8  # "at the end": within 8 windows of the last / first window column or row


def per_frame(name):
    hits, counts, _ = lc.oracle_detect(name)
    out, k = [], 0
    for n in counts:
        out.append(hits[k:k + n])
        k += n
    return out


@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_the_face_frames_have_hits_at_both_ends(name):
    """(a) every F frame has oracle hits; (b) on the strips F0 has a hit within 8 windows of the LAST window column (row, for tall) of a
    scale <= 2 — where x | y << 16 and the 16-bit hit fields are at their largest; (c) and one within 8 of the first, in the same list"""
    w, h = lc.GEOMETRIES[name]
    f0, f1 = per_frame(name)
    assert len(f0) > 0 and len(f1) > 0
    axis = "y" if h > w else "x"
    if name in lc.STRIPS:
        far = [(int(s), int(v)) for s, v in zip(f0["scale"], f0[axis]) if s <= 2 and v >= lc.windows(name, int(s))[axis == "y"] - EDGE]
        assert far, (name, sorted(zip(f0["scale"].tolist(), f0[axis].tolist())))
        assert max(v for _, v in far) > 2048  # beyond the widest frame of the other tests, in window units
    assert ((f0["x"] <= EDGE) | (f0["y"] <= EDGE)).any()
    # the mirrored frame reaches the far end too, so the far end is hit on frame 1 of the batch (one arena_stride in) as well
    assert any(v >= lc.windows(name, int(s))[axis == "y"] - EDGE for s, v in zip(f1["scale"], f1[axis]))
    _, _, sp = lc.oracle_detect(name)
    assert sp[0] > 0 and sp[8] > len(f0) + len(f1)  # survivors deep into the cascade that are no hits: the queue and the deep kernels have work


def test_the_wide_frame_is_the_recorded_one():
    """the figures the wide case was chosen by: 21 hits on F0, the largest x per scale 0 .. 3 against the last window column"""
    f0 = per_frame("wide")[0]
    assert len(f0) == 21
    assert [int(f0["x"][f0["scale"] == s].max()) for s in range(4)] == [4087, 3641, 3243, 2889]
    assert [lc.windows("wide", s)[0] for s in range(4)] == [4090, 3643, 3244, 2890]
    grouped = lc.oracle_grouped("wide")[0]
    assert len(grouped) >= 3 and grouped["x"].max() > 16300 and grouped["x"].min() < 16


@pytest.mark.parametrize("name", list(lc.GEOMETRIES))
def test_grouped_lists_are_non_empty_on_both_frames(name):
    for g in lc.oracle_grouped(name):
        assert len(g) >= 2 and lc.select_best(g)[0]["neighbors"] > 0


def strip_planes(name, along, least):
    """[(level, slot, w, h, slot-0 size across)] of the planes at most 3 pixels across and at least `least` along"""
    levels, _ = lc.oracle_pyramid(name)[0]
    out = []
    for i, (lw, lh, off) in enumerate(levels):
        across, length = (lh, lw) if along == "x" else (lw, lh)
        for s in range(4):
            if off[s] >= 0 and 1 <= across <= 3 and length >= least:
                out.append((i, s, lw, lh, across))
    return out


@pytest.mark.parametrize("name,along,least", [("thin", "x", 1024), ("thin_tall", "y", 1024), ("wide", "x", 512), ("tall", "y", 512)])
def test_the_pyramid_has_strip_planes_and_undrawn_variant_canvases(name, along, least):
    """(d) planes <= 3 pixels across and >= 1024 along, and among them a variant slot whose level is <= 2 across: the slots that draw D.h - 2
    (D.w - 2) rows (columns) draw nothing there, and the canvas, 16 and more 64-column tiles long, must come back all zero.  1024 is reached
    on the 32- and 33-pixel strips; on 16384 x 64 and 65 x 16384 no plane 3 across can be longer than 3 * 256 + 255 pixels (the longest is 912),
    and there the same is asked from 512 on."""
    planes = strip_planes(name, along, least)
    assert planes, name
    assert (max(max(lw, lh) for _, _, lw, lh, _ in planes) >= 1024) == (name in lc.THIN)
    undrawn = [(i, s) for (i, s, lw, lh, across) in planes if across <= 2 and s in ((2, 3) if along == "x" else (1, 3))]
    assert undrawn, planes
    for levels, arena in lc.oracle_pyramid(name):
        for i, s in undrawn:
            p = ho.plane(levels, arena, i, s)
            assert p.size >= least and not p.any(), (i, s)
        i, s = undrawn[0]
        assert ho.plane(levels, arena, i, 0).any()  # ... while slot 0 of the same level is drawn


def test_level_sizes_follow_ccvs_rule_written_out():
    for name, (w, h) in lc.SIZES.items():
        assert [tuple(d) for d in pc.ccv_dims(w, h, 5)] == lc.level_dims(name), name
        assert [(lw, lh) for lw, lh, _ in lc.oracle_pyramid(name)[0][0]] == lc.level_dims(name), name


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(e) the limit geometries, 16384 x 16384 and 16384 x 1 through the planner harness: built as tests/test_geometry_plan_cpu.py builds it, a stand-alone program"""
    d = tmp_path_factory.mktemp("limit_plan")
    exe = str(d / "geometry_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "geometry_plan_harness.cc"), "-o", exe])
    path = str(d / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join([lc.plan_line(name) for name in lc.PLAN_GEOMETRIES] + [lc.plan_line(n + "_copy", dims=lc.copy_case(n)["dims"]) for n in lc.COPIES]) + "\n")
    r = subprocess.run([exe, "plan", path], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = {o["name"]: o for o in (json.loads(line) for line in r.stdout.splitlines())}
    assert list(out) == list(lc.PLAN_GEOMETRIES) + [n + "_copy" for n in lc.COPIES]
    return out


def test_the_planner_accepts_every_limit_geometry(plans):
    """status 0 and every check_plan invariant (the harness exits non-zero on the first that fails); the level sizes are the oracle's, for
    16384 x 16384 ccv's rule written out in Python (its pyramid is 2.5 GB per frame and is not built anywhere)"""
    for name, (w, h) in lc.PLAN_GEOMETRIES.items():
        p = plans[name]
        assert p["status"] == 0 and p["why"] == "", (name, p["why"])
        if name in lc.SIZES:
            assert p["levels"] == [list(d) for d in lc.level_dims(name)], name
        assert p["levels"] == [list(d) for d in pc.ccv_dims(w, h, 5)], name
        assert p["levels"] == [list(d) for d in ho.pyramid_layout(w, h)], name
    assert plans["full"]["windows_per_frame"] == 322849560 and plans["full"]["arena_stride"] == 1544648448
    assert plans["row"]["windows_per_frame"] == 0 and plans["row"]["tiles_per_frame"] == 0


def test_the_plans_reach_the_ends_of_the_16_bit_fields(plans):
    """bx (uint16_t) reaches 228 on the 16384-wide frames at ccv's own sizes (the widest resample destination is level 1, 14596 pixels) and
    255 when level_dims gives a level the frame's own width (wide_copy); pass0 (uint16_t) likewise 900 and more on the 16384-tall frames
    and 1000 and more on tall_copy; the scan tiles' packed origins
    X0 | Y0 << 16 reach the last half-steps of scale 0 (2 qw = 8180); frame 1 of the area geometry lies beyond 2^25 bytes"""
    for name in ("wide", "wide_odd", "thin", "full"):
        assert plans[name]["max_bx"] == 228 == (lc.level_dims("wide")[1][0] - 1) // 64, name
    for n in lc.COPIES:
        assert plans[n + "_copy"]["status"] == 0 and plans[n + "_copy"]["levels"] == [list(d) for d in lc.copy_case(n)["dims"]]
    assert plans["wide_copy"]["max_bx"] == 255 and plans["tall_copy"]["max_pass0"] >= 1000
    for name in ("tall", "thin_tall", "full"):
        assert 900 <= plans[name]["max_pass0"] <= (lc.level_dims("tall")[1][1] - 1) // 16, name
    assert plans["wide"]["max_tile_x0"] > 8000 and plans["tall"]["max_tile_y0"] > 8000
    assert plans["full"]["max_tile_x0"] > 8000 and plans["full"]["max_tile_y0"] > 8000
    assert plans["area"]["arena_stride"] > 1 << 25 and 4099 * 2051 > 1 << 23
    for name in lc.GEOMETRIES:
        assert plans[name]["windows_per_frame"] == sum(4 * qw * qh for qw, qh in (lc.windows(name, s) for s in range(27)) if qw > 0 and qh > 0)


@pytest.mark.parametrize("name", list(lc.CS_BLOBS))
def test_the_blobs_sit_at_the_far_edge_and_stay_tracked(name):
    """(f) within 200 pixels of the far edge; the oracle's track object keeps its size class and its box (x +- width / 2, y +- height / 2, as
    the reference turns it into the next search window) stays inside the frame at every step"""
    w, h = lc.GEOMETRIES[name]
    cx, cy, a, b = lc.CS_BLOBS[name]
    assert (w - cx <= 200 and w == lc.LIMIT) or (h - cy <= 200 and h == lc.LIMIT)
    calls, models = lc.cs_oracle(name)
    assert len(calls) == lc.CS_STEPS - 1 and all(m.sum() > 0 for m in models)
    for step in calls:
        for sw, to in step:
            assert to["width"] >= 16 and to["height"] >= 32, to
            assert 0 <= to["x"] - to["width"] / 2 and to["x"] + to["width"] / 2 <= w and 0 <= to["y"] - to["height"] / 2 and to["y"] + to["height"] / 2 <= h, to
            assert max(w - to["x"], 0) <= 200 or max(h - to["y"], 0) <= 200
            assert not np.isnan(to["angle"])

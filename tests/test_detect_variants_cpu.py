"""Guards the tables of tests/detect_variant_cases.py without a device, and pins the CPU oracle to the reference at intervals other than 5
and windows other than 24x24 (tests/golden/detect_variants.json, recorded by tests/golden/make_detect_variants_golden.py from the unmodified
reference JS): level sizes, plane CRCs, raw rects and grouped rects, bit for bit.  tests/test_gpu_detect_variants.py then compares the HIP
path with this oracle and with the same vectors."""
import json
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
from conftest import ROOT, load_golden

import detect_variant_cases as dv
from headtrackr_amd import synth
from headtrackr_amd.cascade import load_cascade
from oracle import ht_oracle as ho

GOLDEN = load_golden("detect_variants.json")
CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NODE = shutil.which("node")
PLAN_DEFAULTS = "4 0 0 0 32768 0 1 0 0 0 0 0"  # rs_rpt .. queue_capacity_cfg, nlevel_dims = 0 (tests/host/geometry_plan_harness.cc)


def _geometries():
    """every (w, h, interval, cw, ch) a GPU test of tests/test_gpu_detect_variants.py sets"""
    g = [(w, h, iv, 24, 24) for iv in dv.INTERVALS for (w, h) in dv.SIZES]
    g += [(w, h, iv, cw, ch) for (cw, ch, iv) in dv.WINDOW_CASES for (w, h) in dv.WINDOW_SIZES]
    for c in dv.GOLDEN_CASES + [dict(w=160, h=120, interval=3, cascade=None)]:
        cw, ch = (24, 24) if not c["cascade"] else (int(v) for v in c["cascade"].split("x"))
        g.append((c["w"], c["h"], c["interval"], cw, ch))
    return sorted(set(g))


def _option_plans():
    """the planner inputs behind the option strings of the GPU tests (TAIL_OPTIONS on intervals 1 and 12; early_scan, batch 6, on 2 and 8):
    W H max_batch interval rs_rpt rs_nofast rs_nosort rs_notail rs_tailcap forced tail_table forced early_scan aux_stream queue_cfg 0"""
    lines = []
    for iv in dv.TAIL_INTERVALS:
        for (w, h) in dv.TAIL_SIZES:
            lines.append(f"{w} {h} 3 {iv} 4 0 0 1 32768 0 1 0 0 0 0 0")      # rs_notail=1
            lines.append(f"{w} {h} 3 {iv} 4 1 0 0 32768 0 1 0 0 0 0 0")      # rs_nofast=1
            for table in (0, 1, 2):
                lines.append(f"{w} {h} 3 {iv} 4 0 0 0 1000 1 {table} 1 0 0 0 0")  # rs_tailtable, rs_tailcap=1000
    for iv in (2, 8):
        lines.append(f"160 120 6 {iv} 4 0 0 0 32768 0 1 0 1 1 0 0")          # early_scan=1 on a context with its second stream
        lines.append(f"160 120 6 {iv} 4 0 0 0 32768 0 1 0 0 0 8 0")          # queue_capacity=8
    return lines


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """the host geometry planner (headtrackr_amd/csrc/ht_geometry_plan.h in its sanitised harness) on every geometry, batch 3"""
    d = tmp_path_factory.mktemp("variant_plans")
    exe = str(d / "geometry_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "geometry_plan_harness.cc"), "-o", exe])
    path = str(d / "cases.txt")
    geos = _geometries()
    with open(path, "w") as f:
        for (w, h, iv, cw, ch) in geos:
            f.write(f"g_{w}x{h}_i{iv}_{cw}x{ch} {w} {h} 3 {iv} {PLAN_DEFAULTS} {cw} {ch}\n")
        for k, line in enumerate(_option_plans()):
            f.write(f"opt{k} {line}\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, "plan", path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(geos) + len(_option_plans()) and all(o["status"] == 0 for o in out)
    return dict(zip(geos, out))


def test_tables_are_the_ones_the_issue_names():
    assert dv.INTERVALS == [1, 2, 3, 8, 12] and 5 not in dv.INTERVALS
    assert dv.SIZES == [(160, 120), (97, 81), (201, 157)]
    assert dv.WINDOWS == [(20, 20), (24, 20), (20, 24), (32, 32), (64, 64), (8, 8)] and (24, 24) not in dv.WINDOWS
    assert max(max(s) for s in dv.SIZES) <= 201


def test_every_geometry_plans_within_the_level_limit_and_equals_the_oracles_layout(plans):
    """level count and sizes: ho.pyramid_layout == the host planner, which also passes its own invariants (tiles cover every canvas and every
    scale's half-steps once) under the sanitizers; the planner's window count is the oracle's stage-0 count"""
    seen_empty, seen_no_scale = 0, 0
    for (w, h, iv, cw, ch), p in plans.items():
        layout = ho.pyramid_layout(w, h, iv, cw, ch)
        assert p["status"] == 0, p
        assert len(layout) == p["nlevels"] <= dv.MAX_LEVELS, (w, h, iv, cw, ch)
        assert [list(x) for x in layout] == p["levels"], (w, h, iv, cw, ch)
        assert p["nlevels"] <= 255  # ht_hit.scale is 8 bits
        seen_empty += any(a == 0 or b == 0 for a, b in layout)
        nxt = iv + 1
        qs = [(layout[i + 2 * nxt][0] - cw // 4, layout[i + 2 * nxt][1] - ch // 4) for i in range(len(layout) - 2 * nxt)]
        seen_no_scale += any(qw <= 0 or qh <= 0 for qw, qh in qs)
        assert p["windows_per_frame"] == sum(4 * qw * qh for qw, qh in qs if qw > 0 and qh > 0) > 0
    assert seen_empty >= 2 and seen_no_scale >= 10  # levels that collapse to nothing, scales without a window (64x64 on 97x81 among them)
    assert any(qw <= 0 for qw, _ in [(ho.pyramid_layout(97, 81, 5, 64, 64)[i + 12][0] - 16, 0) for i in range(35)])
    for (w, h, iv, cw, ch), p in plans.items():
        if (w, h) in dv.WINDOW_SIZES and (cw, ch, iv) in dv.WINDOW_CASES:
            assert p["windows_per_frame"] * 3 == dv.window_expected(cw, ch, iv, w, h)[1][0]
    for iv in dv.INTERVALS:
        assert plans[(160, 120, iv, 24, 24)]["windows_per_frame"] * 6 == dv.builtin_expected(iv)[1][0]


def test_level_limit_is_what_keeps_large_windows_away_from_interval_12():
    """upto + 2 (interval + 1) levels: 85 for 24x24 at interval 12, 103 for 64x64 — refused, which is why no window case runs there"""
    assert len(ho.pyramid_layout(160, 120, 12)) == 85
    with pytest.raises(ValueError):
        ho.pyramid_layout(160, 120, 12, 64, 64)


def test_builder_at_24x24_is_the_custom_cascade_tests_builder():
    import test_gpu_custom_cascade as old

    for mode, seed in (("ties", 1), ("asym", 3), ("binary", 4)):
        a = old.make_cascade(seed, 6, [3, 4, 6, 9, 70, 130], mode, thr_pass=old.THR_PASS[mode])
        b = dv.make_cascade(seed, 24, 24, 6, [3, 4, 6, 9, 70, 130], mode, thr_pass=old.THR_PASS[mode], corner=False)
        assert a.blob == b.blob


@pytest.mark.parametrize("cw,ch", dv.WINDOWS)
def test_window_cascades_stay_inside_their_window_and_reach_its_far_corner(cw, ch):
    c = dv.window_cascade(cw, ch)
    assert (c.width, c.height) == (cw, ch)
    corners = {0: False, 1: False, 2: False}
    for f in c.features:
        for pol in "pn":
            for q in range(8):
                z = int(f[pol + "z"][q])
                if z < 0:
                    continue
                assert q < f["size"] and 0 <= f[pol + "x"][q] < (cw >> z) and 0 <= f[pol + "y"][q] < (ch >> z)
                if f[pol + "x"][q] == (cw >> z) - 1 and f[pol + "y"][q] == (ch >> z) - 1:
                    corners[z] = True
        assert f["pz"][0] >= 0 and f["nz"][0] >= 0
    assert all(corners.values())
    f = c.features[1]  # the corner feature sits in stage 0: every window evaluates it
    assert int(c.stages[0]["count"]) > 1 and (f["px"][0], f["py"][0], f["pz"][0]) == (cw - 1, ch - 1, 0) and (f["nx"][1], f["ny"][1], f["nz"][1]) == (0, ch - 1, 0)
    assert {dv.WINDOW_CASCADE[w][1] for w in dv.WINDOWS} == {"ties", "asym", "binary"}


def test_json_shape_round_trips_through_both_packers(tmp_path):
    """cascade_from_json(cascade_to_json(c)) gives c's bytes; so does headtrackr_amd/js/cascade_pack.js where node is installed"""
    for name, obj in GOLDEN["cascades"].items():
        c = dv.golden_cascade(name)
        assert obj == dv.cascade_to_json(c), name  # the committed cascade is the builder's
        assert dv.cascade_from_json(obj).blob == c.blob, name
        if NODE:
            jf, bf = tmp_path / (name + ".json"), tmp_path / (name + ".bin")
            jf.write_text(json.dumps(obj))
            script = "const fs=require('fs');const p=require(process.argv[1]);fs.writeFileSync(process.argv[3],p.packCascade(JSON.parse(fs.readFileSync(process.argv[2],'utf8'))));"
            subprocess.check_call([NODE, "-e", script, os.path.join(ROOT, "headtrackr_amd", "js", "cascade_pack.js"), str(jf), str(bf)])
            assert bf.read_bytes() == c.blob, name


@pytest.mark.parametrize("interval", dv.INTERVALS)
def test_builtin_hit_cases_find_something_and_reject_something(interval):
    per, sp = dv.builtin_expected(interval)
    assert sum(len(h) for h in per) > 0 and 0 < sp[-1] < sp[0]
    assert sum(1 for h in per if len(h)) >= 2 and any(len(h) == 0 for h in per)
    assert len({int(s) for h in per for s in h["scale"]}) >= 2  # hits on more than one scale: sx[] matters


@pytest.mark.parametrize("cw,ch,interval", dv.WINDOW_CASES)
@pytest.mark.parametrize("w,h", dv.WINDOW_SIZES)
def test_window_hit_cases_find_something_and_three_stages_reject(cw, ch, interval, w, h):
    per, sp = dv.window_expected(cw, ch, interval, w, h)
    assert sum(len(x) for x in per) > 0 and 0 < sp[-1] < sp[0]
    assert int((np.diff(sp) < 0).sum()) >= 3, list(sp)


def _case_cascade(case):
    if case["cascade"] is None:
        return load_cascade()
    return dv.cascade_from_json(GOLDEN["cascades"][case["cascade"]])


def test_golden_file_holds_the_cases_of_the_table():
    assert [(c["name"], c["w"], c["h"], c["interval"], c["cascade"], c["gen"]) for c in GOLDEN["cases"]] == \
           [(c["name"], c["w"], c["h"], c["interval"], c["cascade"], c["gen"]) for c in dv.GOLDEN_CASES]
    assert sorted(GOLDEN["cascades"]) == ["20x20", "32x32"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "detect_variants.json")) < 128 << 10


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_oracle_equals_the_recorded_reference(case):
    """as tests/test_oracle_golden.py check_detect_case: level sizes, plane CRCs in creation order, raw rects, grouped rects.  The level
    sizes outside interval 5 come from the C library's pow() in the oracle and from V8's Math.pow in the reference: they agree for every
    recorded (interval, size), so include/headtrackr_hip.h's promise holds here too."""
    w, h, interval = case["w"], case["h"], case["interval"]
    casc = _case_cascade(case)
    cw, ch = casc.width, casc.height
    frame = synth.make(case["gen"], w, h)
    assert zlib.crc32(frame.tobytes()) == case["input_crc"], "synthetic input drifted from the golden input"
    gray = ho.grayscale_rgba(frame)
    assert zlib.crc32(gray[..., 0].tobytes()) == case["gray_crc"]
    assert [list(x) for x in ho.pyramid_layout(w, h, interval, cw, ch)] == dv.recorded_level_dims(case)
    levels, arena = ho.pyramid(frame, interval=interval, cw=cw, ch=ch)
    assert len(levels) == case["nlevels"]
    order = dv.creation_order(len(levels), interval + 1)
    assert len(order) == len(case["pyramid"])
    for (i, s), g in zip(order, case["pyramid"]):
        p = ho.plane(levels, arena, i, s)
        assert (p.shape[1], p.shape[0]) == (g["w"], g["h"]), f"level {i} size"
        assert zlib.crc32(p.tobytes()) == g["crc"], f"level {i} slot {s} bytes"
    hits = ho.detect_raw(frame, casc.blob, interval=interval, cap=1 << 20)
    rects = ho.hits_to_rects(hits, interval, cw, ch)
    assert len(rects) == len(case["raw"]) > 0
    for r, g in zip(rects, case["raw"]):
        for k in ("x", "y", "width", "height", "confidence"):
            assert r[k] == g[k], (k, r, g)
    grouped = ho.group(rects, case["min_neighbors"])
    assert len(grouped) == len(case["grouped"])
    for r, g in zip(grouped, case["grouped"]):
        for k in ("x", "y", "width", "height", "confidence", "neighbors"):
            assert r[k] == g[k], (k, r, g)
    assert grouped.tobytes() == ho.detect_objects(frame, casc.blob, interval, case["min_neighbors"], cw=cw, ch=ch, cap=1 << 20).tobytes()

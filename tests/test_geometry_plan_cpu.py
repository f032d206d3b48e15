"""The geometry plan of ht_set_geometry (headtrackr_amd/csrc/ht_geometry_plan.h: level sizes and arena offsets, resample jobs and tile records
in launch order, the tail kernel's tables, scan scales and tile records, early-scan split, queue capacity) without a device: the header is
compiled with AddressSanitizer + UBSan into a host-only harness (tests/host/geometry_plan_harness.cc) and run as a program.

The expected tables (tests/golden/geometry_plan.json) were recorded from the library as it was BEFORE the planner became a unit of its own —
its set_geometry_impl and ht_scan_plan_tiles compiled for the host, with the device allocations and copies replaced by stubs that kept the
uploaded bytes — so they say what the kernels have been given all along, not what the new planner thinks."""
import json
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import ROOT

from oracle import ht_oracle as ho

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "geometry_plan.json")))["cases"]
KEYS = ["W", "H", "max_batch", "interval", "rs_rpt", "rs_nofast", "rs_nosort", "rs_notail", "rs_tailcap", "rs_tailcap_forced", "tail_table",
        "tail_table_forced", "early_scan", "aux_stream", "queue_capacity_cfg"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("geometry_plan") / "geometry_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "geometry_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def plans(harness, tmp_path_factory):
    """every recorded case planned once: {name: the harness's JSON line}.  The harness also checks the plan invariants the kernels rely on
    (check_plan: tiles cover each canvas / each scale's half-steps exactly once, extents and bands hold their taps, prefix sums, contiguous
    tail tap ranges) and exits non-zero on the first that does not hold — or on the first sanitizer report."""
    path = str(tmp_path_factory.mktemp("geometry_cases") / "cases.txt")
    with open(path, "w") as f:
        for c in GOLDEN:
            i = c["inputs"]
            f.write(" ".join([c["name"]] + [str(i[k]) for k in KEYS] + [str(len(i["level_dims"]))] + [str(v) for wh in i["level_dims"] for v in wh]) + "\n")
    r = subprocess.run([harness, "plan", path], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["name"] for o in out] == [c["name"] for c in GOLDEN]
    return {o["name"]: o for o in out}


def test_the_recorded_cases_reach_every_branch_of_the_planner():
    """the fixture itself: both sides of the small-batch tail cap (48 / 49) and of the tail-table choice (128 / 129), all three tail forms, a
    geometry without a tail and without a scale, an early split, explicit level sizes with empty levels, another interval"""
    e = {c["name"]: c["expect"] for c in GOLDEN}
    assert len(e) == 25
    assert (e["320x240_b48"]["tail_first_gen"], e["320x240_b49"]["tail_first_gen"]) == (5, 4)
    assert (e["320x240_b128"]["tail_table"], e["320x240_b129"]["tail_table"]) == (1, 0)
    assert {x["tail_table"] for x in e.values()} == {0, 1, 2}
    assert e["1920x1080_b8"]["tail_first_gen"] == 0 and e["320x240_b256_notail"]["tail_first_gen"] == 0
    assert e["24x24_b4"]["tiles_per_frame"] == 0 and e["48x48_b4"]["tiles_per_frame"] > 0
    assert e["320x240_b256_early_scan_aux"]["early_gen"] == 2 and e["320x240_b256_queue_cfg"]["queue_capacity"] == 100000
    assert any(wh == [0, 0] for wh in [c for c in GOLDEN if c["name"].endswith("level_dims_zero")][0]["inputs"]["level_dims"])
    assert e["320x240_b256_interval3"]["nlevels"] == 26
    for a, b in (("nofast", "crc_gen_tiles"), ("nosort", "crc_gen_tiles"), ("rpt1", "gen_blocks"), ("rpt2", "gen_blocks"), ("tailcap4000", "crc_tail_jobs")):
        assert e["320x240_b256_" + a][b] != e["320x240_b256"][b], a
    # (rs_rpt = 3 plans what 4 does here: no ratio of this pyramid lets a tile's source rows fit the LDS window with four passes)
    assert e["320x240_b256_rpt3"]["crc_gen_tiles"] == e["320x240_b256"]["crc_gen_tiles"]


@pytest.mark.parametrize("name", [c["name"] for c in GOLDEN])
def test_plan_tables_and_scalars_equal_the_recorded_ones(plans, name):
    want = [c for c in GOLDEN if c["name"] == name][0]["expect"]
    got = plans[name]
    assert want["status"] == 0
    for key, value in want.items():
        assert got[key] == value, (name, key, got[key], value)


def test_level_sizes_equal_the_oracles_pyramid(plans):
    """ccv.js:110-147 through the oracle's own pyramid (not this library's arithmetic), for every recorded case that leaves the sizes to ccv"""
    seen = {}
    for c in GOLDEN:
        i = c["inputs"]
        if not i["level_dims"]:
            seen.setdefault((i["W"], i["H"], i["interval"]), c["name"])
    assert len(seen) == 8
    for (w, h, interval), name in seen.items():
        levels, _arena = ho.pyramid(np.zeros((h, w, 4), dtype=np.uint8), interval=interval)
        assert [[lw, lh] for lw, lh, _off in levels] == plans[name]["levels"], name


def test_host_tap_equals_the_declared_formula_in_python_floats(harness, tmp_path):
    """ht_host_tap against the same binary64 operations written out in Python (whose float is binary64 and never fused): the ratios of the
    pyramid (2^(k/6)-derived size quotients, exact 2.0), s = 1, the clamps at both ends, source-rect origins 0 and 1"""
    import math

    rng = np.random.default_rng(20261017)
    tuples = []
    for s, d in ((320, 285), (240, 213), (320, 160), (160, 80), (159, 78), (1080, 962), (641, 571), (1, 1), (1, 7), (7, 1), (2, 5)):
        r = s / d
        for i in sorted({0, 1, d // 2, max(d - 2, 0), d - 1, d, d + 2} | {int(v) for v in rng.integers(0, d, 12)}):
            tuples.append((i, r, s, int(rng.integers(0, 2))))
    for i in range(40):
        tuples.append((i, 2.0, 80, 1))
    for _ in range(120):
        s = int(rng.integers(1, 2000))
        tuples.append((int(rng.integers(0, 2200)), float(rng.uniform(0.3, 3.0)), s, int(rng.integers(0, 2))))
    assert len(tuples) >= 300
    path = str(tmp_path / "taps.txt")
    with open(path, "w") as f:
        for i, r, s, o in tuples:
            f.write("%d %s %d %d\n" % (i, float(r).hex(), s, o))
    res = subprocess.run([harness, "taps", path], capture_output=True, text=True, timeout=120, env=ENV)
    assert res.returncode == 0 and not res.stderr, res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == len(tuples)
    for (i, r, s, o), line in zip(tuples, lines):
        f = (float(i) + 0.5) * r
        f = f + (-0.5)
        f = 0.0 if f < 0.0 else f
        fmax = float(s - 1)
        f = fmax if f > fmax else f
        af = math.floor(f)
        t = f - af
        want = (o + int(af), o + min(int(af) + 1, s - 1), t, 1.0 - t)
        a, b, th, uh = line.split()
        assert (int(a), int(b), float.fromhex(th), float.fromhex(uh)) == want, (i, r, s, o)


def test_the_plan_is_computed_in_one_place():
    """source layout: the host tap, the resample tile-record loop and the scan tiling are defined once under csrc/, in the host-only header; the
    context only calls the planner and uploads (no sort, no tap arithmetic of its own), and the header pulls in no HIP"""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".inc", ".cc"))}
    for marker in (r"\bHtTap ht_host_tap\(", r"t\.bx = \(uint16_t\)x, t\.pass0 = ", r"std::stable_sort", r"strip_magic = \(\(1u << 24\)"):
        assert [f for f, t in texts.items() if re.search(marker, t)] == ["ht_geometry_plan.h"], marker
    ctx = texts["ht_context.hip"]
    assert "std::stable_sort" not in ctx and "ht_host_tap(" not in ctx and "ht_plan_geometry(" in ctx
    assert "ht_scan_plan_tiles" not in "".join(texts.values())
    assert len(re.findall(r"constexpr int TXH = HT_SCAN_TXH;", texts["ht_scan.hip"])) == 1 and not re.search(r"constexpr int TXH = \d", texts["ht_scan.hip"])
    for f in ("ht_geometry_plan.h", "ht_plan_types.h"):
        assert "#include <hip" not in texts[f] and '#include "ht_internal.h"' not in texts[f], f
    assert '#include "ht_plan_types.h"' in texts["ht_internal.h"] and "struct HtResampleJob" not in texts["ht_internal.h"]


# ---- level_dims: what ht_set_geometry refuses, and the geometries of tests/test_gpu_pyramid_ties.py ----------------------------------------

def run_dims(harness, tmp_path, cases):
    """cases: [(name, W, H, interval, dims)] through ht_check_level_dims: {name: (status, why)}"""
    path = str(tmp_path / "dims.txt")
    with open(path, "w") as f:
        for name, w, h, interval, dims in cases:
            f.write(" ".join([name, str(w), str(h), str(interval), str(len(dims))] + [str(v) for wh in dims for v in wh]) + "\n")
    r = subprocess.run([harness, "dims", path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["name"] for o in out] == [c[0] for c in cases]
    return {o["name"]: (o["status"], o["why"]) for o in out}


def test_level_dims_the_scan_cannot_take_are_refused(harness, tmp_path):
    """Scale i reads one window on levels i, i + next, i + 2 next at 4, 2 and 1 times its coordinates, unclamped (HT_WIN_SETUP in
    ht_scan.hip): a level i + next larger than floor(size / 2) of level i would put the last windows past the end of level i.  Such
    level_dims are refused on the host, with a message naming the two levels; ccv's own sizes, smaller ones and empty levels pass."""
    import pyramid_cases as pc

    ok = pc.ccv_dims(320, 240, 5)
    cases = [("ccv", 320, 240, 5, ok), ("ccv_i2", 169, 125, 2, pc.ccv_dims(169, 125, 2))]

    def with_level(i, wh):
        d = list(ok)
        d[i] = wh
        return d

    smaller = with_level(6, (100, 70))  # less than half of level 0, and the levels above it halved in turn
    for i in range(12, 39, 6):
        smaller[i] = (smaller[i - 6][0] // 2, smaller[i - 6][1] // 2)
    cases += [("wider_half", 320, 240, 5, with_level(6, (161, 120))), ("taller_half", 320, 240, 5, with_level(6, (160, 121))),
              ("quarter", 320, 240, 5, with_level(12, (81, 60))),                 # more than half of level 6, a quarter of level 0
              ("odd_parent", 320, 240, 5, with_level(7, (143, 106))),             # level 1 is 285 x 213: floor(285 / 2) = 142
              ("last_level", 320, 240, 5, with_level(38, (ok[32][0] // 2 + 1, ok[38][1]))),
              ("smaller_is_fine", 320, 240, 5, smaller),
              ("zeros_are_fine", 320, 240, 5, [(320, 240)] + [(0, 0)] * 38),
              ("level0_is_the_frame", 320, 240, 5, with_level(0, (319, 240))), ("negative", 320, 240, 5, with_level(3, (-1, 5))),
              ("beyond_the_frame", 320, 240, 5, with_level(1, (321, 10)))]
    for (w, h) in pc.UNUSUAL_SIZES:
        for k, dims in enumerate(pc.unusual_dims(w, h)):
            cases.append((f"unusual_{w}_{k}", w, h, 5, dims))
    for name, args in pc.COPY_CASES.items():
        cases.append((name, args[0], args[1], 5, pc.copy_level_case(*args)["dims"]))
    got = run_dims(harness, tmp_path, cases)
    for name in ("ccv", "ccv_i2", "smaller_is_fine", "zeros_are_fine", "unusual_333_0", "unusual_333_1", "unusual_641_0", "unusual_641_1", "odd_169x125", "even_164x124"):
        assert got[name] == (0, ""), (name, got[name])
    for name, a, b in (("wider_half", 6, 0), ("taller_half", 6, 0), ("quarter", 12, 6), ("odd_parent", 7, 1), ("last_level", 38, 32)):
        st, why = got[name]
        assert st == -1 and f"level {a} (" in why and f"larger than half of level {b} (" in why, (name, got[name])
    for name in ("level0_is_the_frame", "negative", "beyond_the_frame"):
        assert got[name] == (-1, "ht_set_geometry: bad level_dims"), (name, got[name])


def test_recorded_reference_level_sizes_are_accepted(harness, tmp_path):
    """the level sizes recorded from the reference itself (tests/golden/detect_variants.json) obey the rule with equality"""
    import detect_variant_cases as dv
    from conftest import load_golden

    cases = [(c["name"], c["w"], c["h"], c["interval"], dv.recorded_level_dims(c)) for c in load_golden("detect_variants.json")["cases"]]
    assert len(cases) >= 8
    got = run_dims(harness, tmp_path, cases)
    assert all(v == (0, "") for v in got.values()), got
    for _, _, _, interval, dims in cases:
        assert all(tuple(dims[i + interval + 1]) == (dims[i][0] // 2, dims[i][1] // 2) for i in range(len(dims) - interval - 1))


def test_set_geometry_checks_level_dims_before_it_tears_anything_down():
    ctx = open(os.path.join(CSRC, "ht_context.hip")).read()
    body = ctx[ctx.index('extern "C" ht_status ht_set_geometry('):]
    assert 0 < body.index("ht_check_level_dims(") < body.index("free_geometry(c)")
    assert len(re.findall(r"\bht_check_level_dims\(", "".join(open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".inc", ".cc"))))) == 2  # defined once, called once


def test_the_pyramid_tie_geometries_plan(harness, tmp_path):
    """the geometries of tests/test_gpu_pyramid_ties.py through the planner and the harness's invariants (tiles cover each canvas once, extents
    and bands hold their taps): the unusual level sizes, the ratio-1 copies, and a tail that starts at generation 1 in all three forms"""
    import pyramid_cases as pc

    lines = []
    w, h, interval = pc.TAIL_CASE[:3]
    for table in (0, 1, 2):
        lines.append(f"tail{table} {w} {h} 3 {interval} 4 0 0 0 {pc.TAIL_CAP} 1 {table} 1 0 0 0 0")
    with_dims = [(f"unusual_{w}_{k}", w, h, dims) for (w, h) in pc.UNUSUAL_SIZES for k, dims in enumerate(pc.unusual_dims(w, h))]
    with_dims += [(name, a[0], a[1], pc.copy_level_case(*a)["dims"]) for name, a in pc.COPY_CASES.items()]
    for name, w, h, dims in with_dims:
        for rpt in (4, 2):
            lines.append(f"{name}_rpt{rpt} {w} {h} 3 5 {rpt} 0 0 0 32768 0 1 0 0 0 0 {len(dims)} " + " ".join(f"{a} {b}" for a, b in dims))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([harness, "plan", path], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = {o["name"]: o for o in (json.loads(line) for line in r.stdout.splitlines())}
    assert len(out) == len(lines) and all(o["status"] == 0 for o in out.values())
    for table in (0, 1, 2):
        assert out[f"tail{table}"]["tail_first_gen"] == 1 and out[f"tail{table}"]["tail_table"] == table
        assert out[f"tail{table}"]["levels"] == [list(d) for d in pc.ccv_dims(pc.TAIL_CASE[0], pc.TAIL_CASE[1], 5)]
    for name, w, h, dims in with_dims:
        assert out[name + "_rpt4"]["levels"] == [list(d) for d in dims] and out[name + "_rpt4"]["windows_per_frame"] > 0

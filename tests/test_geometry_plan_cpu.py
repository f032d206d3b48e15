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

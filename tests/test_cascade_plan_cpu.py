"""The cascade plan of ht_create (headtrackr_amd/csrc/ht_cascade_plan.h: the blob's checks, the integer-decision test, the tile, fp, coordinate,
patch and packed feature tables, the hand-off stage) without a device: the header is compiled with AddressSanitizer + UBSan into a host-only
harness (tests/host/cascade_plan_harness.cc) and run as a program on the blobs of tests/cascade_cases.py.

The expected results (tests/golden/cascade_plan.json) were recorded from the library as it was BEFORE the planner became a unit of its own —
its ht_create run on the CPU, with the device allocations and copies replaced by stubs that kept the uploaded bytes — so they say what the
kernels have been given all along, not what the new planner thinks."""
import json
import os
import re
import subprocess
import zlib

import pytest
from conftest import ROOT

import cascade_cases as cc

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "cascade_plan.json")))["cases"]
EXPECT = {c["name"]: c["expect"] for c in GOLDEN}
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
MESSAGES = ("cascade blob: bad magic", "cascade blob: unsupported version", "cascade blob: unsupported stage count or window size", "cascade blob: truncated",
            "cascade blob: inconsistent stage table", "cascade blob: feature without a valid first point", "cascade blob: feature point outside the window")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """every case planned once: {name: the harness's JSON line}.  The harness also checks what the kernels rely on (check_plan: every
    offset decodes back to the blob's point, slot fill, counts, LDS bounds, integer alphas, stage tiling, the packed tail) and exits non-zero
    on the first that does not hold — or on the first sanitizer report."""
    exe = str(tmp_path_factory.mktemp("cascade_plan") / "cascade_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "cascade_plan_harness.cc"), "-o", exe])
    r = subprocess.run([exe, cc.manifest(str(tmp_path_factory.mktemp("cascade_blobs")))], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert [o["name"] for o in out] == [c["name"] for c in GOLDEN]
    return {o["name"]: o for o in out}


def test_the_cases_are_the_recorded_ones():
    """the blobs are rebuilt from headtrackr_amd/data/cascade.bin on every run: same names, same order, same bytes, same inputs as recorded"""
    now = [(n, len(b), zlib.crc32(b), int(builtin), split) for n, b, builtin, split in cc.accepted()] + [(n, len(b), zlib.crc32(b), 0, 0) for n, b in cc.rejected()]
    assert now == [(c["name"], c["blob_len"], c["blob_crc"], c["builtin"], c["split"]) for c in GOLDEN]
    assert [c["expect"]["status"] for c in GOLDEN] == [0] * len(cc.accepted()) + [-1] * len(cc.rejected())


def test_the_recorded_cases_reach_every_branch_of_the_planner():
    """from the record alone (what the library did before the planner existed): both values of decimal_alphas, the fp table present and absent,
    the packed tail present and absent for each of its reasons, every reject message, hand-off stages on both sides of 8"""
    e = EXPECT
    base = e["builtin_split0"]
    assert (base["decimal_alphas"], base["n_fp"], base["split_stage"], base["packed_first"], base["n_packed"]) == (1, 2015, 8, 147, 1868)
    # option split: clamped to the 8 generated stages for the built-in cascade, to the stage count otherwise; default 8 / 4
    assert [e["builtin_split%d" % s]["split_stage"] for s in (1, 4, 8, 12, 63)] == [1, 4, 8, 8, 8]
    assert [e["same_bytes_not_builtin_split%d" % s]["split_stage"] for s in (0, 8, 12, 63)] == [4, 8, 12, 16]
    for name in ("builtin_split1", "builtin_split4", "same_bytes_not_builtin_split12"):  # the tail follows the hand-off stage, the other tables do not
        assert e[name]["n_packed"] == 2015 - e[name]["packed_first"] and e[name]["crc_packed"] != base["crc_packed"]
        assert all(e[name][k] == base[k] for k in ("crc_stages", "crc_deep", "crc_tile", "crc_fp", "crc_patch"))
    # integer decisions off: an alpha that is no multiple of 1e-8 / only the rounding-error bound; both take fp and the packed tail with them
    for name in ("undecimal", "huge_alphas"):
        assert (e[name]["decimal_alphas"], e[name]["n_fp"], e[name]["n_packed"]) == (0, 0, 0)
    # fp absent for its own reasons while the tail is packed: alpha[0] != -alpha[1], six points in front of the hand-off stage
    for name in ("asymmetric", "six_points_below_split"):
        assert (e[name]["decimal_alphas"], e[name]["n_fp"]) == (1, 0) and e[name]["n_packed"] > 0
    # the packed tail absent while fp exists: 2.0e9 <= |alpha * 1e8| < 2^31, a window that is not 24x24, no stage behind the hand-off, no
    # feature behind it, more than 64 KB
    for name in ("alpha_21", "window_20x20", "window_64x64", "window_24x20", "single_stage", "same_bytes_not_builtin_split63", "empty_last_stage_split16", "long_tail"):
        assert e[name]["decimal_alphas"] == 1 and e[name]["n_fp"] == e[name]["nfeat"] and (e[name]["n_packed"], e[name]["packed_first"]) == (0, 0), name
    assert e["long_tail"]["nfeat"] - 28 > 2048 and e["long_tail_split15"]["n_packed"] == 2579 - 1451
    assert (e["empty_last_stage_split16"]["split_stage"], e["empty_last_stage_split16"]["nstages"]) == (16, 17)
    # ... and six points behind it (the tile tables take them: both are without fp)
    for name in ("six_points_behind_split", "six_points_at_split12"):
        assert (e[name]["decimal_alphas"], e[name]["n_fp"], e[name]["n_packed"]) == (1, 0, 0)
    assert e["six_points_at_split12"]["split_stage"] == 12
    # points that are not in the leading slots are compacted: other tables than the built-in cascade's, the same shape
    hole, split4 = e["hole"], e["builtin_split4"]
    assert all(hole[k] != split4[k] for k in ("crc_deep", "crc_tile", "crc_fp", "crc_patch", "crc_packed")) and all(hole[k] == split4[k] for k in ("n_fp", "n_packed", "crc_stages"))
    assert {(x["cw"], x["ch"]) for x in e.values() if x["status"] == 0} == {(24, 24), (20, 20), (64, 64), (24, 20)}
    rejected = [x["message"] for x in e.values() if x["status"] != 0]
    assert all(x["status"] == -1 for x in e.values() if x["status"] != 0)  # HT_ERR_INVALID
    assert set(rejected) == set(MESSAGES) and all(rejected.count(m) >= 2 for m in MESSAGES)


@pytest.mark.parametrize("name", [c["name"] for c in GOLDEN])
def test_plan_tables_and_scalars_equal_the_recorded_ones(plans, name):
    got = plans[name]
    for key, value in EXPECT[name].items():
        assert got[key] == value, (name, key, got[key], value)


def test_which_reason_switched_the_integer_decisions_off(plans):
    """the harness's count of alphas and thresholds that are no multiple of 1e-8: two in `undecimal`, none in `huge_alphas` — there only the
    bound on the sequential sum's rounding error fails"""
    assert {n: p["inexact"] for n, p in plans.items() if p["status"] == 0 and (p["inexact"] or not p["decimal_alphas"])} == {"undecimal": 2, "huge_alphas": 0}


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def test_the_cascade_is_planned_in_one_place():
    """source layout: the two offset formulas, the point compaction and alpha * 1e8 are written once under csrc/, in headers without HIP;
    the context only calls the planner and uploads, ht_scan.hip keeps kernels and launches"""
    texts = {f: _code(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".inc", ".cc"))}

    def files_with(pattern):
        return [f for f, t in texts.items() if re.search(pattern, t)]

    def scan_count(word):
        return len(re.findall(r"\b%s\b" % word, texts["ht_scan.hip"]))

    assert files_with(r"#define HT_O[012]\(") == ["ht_cascade_types.h"] and len(re.findall(r"#define HT_O[012]\(", texts["ht_cascade_types.h"])) == 3
    for marker in (r"HT_O0\(x, y\) : ", r"\bHT_PATCH1 \+ y \* ", r"\* 1e8", r"\bllround\b", r"cascade blob: "):
        assert files_with(marker) in (["ht_cascade_plan.h"], []), marker
    plan = texts["ht_cascade_plan.h"]
    assert len(re.findall(r"\* 1e8", plan)) == 1 and len(re.findall(r"HT_PATCH1 \+", plan)) == 1 and len(re.findall(r"HT_O0\(", plan)) == 1
    assert not files_with(r"\bnearbyint\b|\bas_decimal8\b|\bht_scan_tile_tables\b|\bht_scan_pack_deep\b") and scan_count("tile_ok") == 2
    for f in ("ht_cascade_plan.h", "ht_cascade_types.h"):
        assert "#include <hip" not in texts[f] and '#include "ht_internal.h"' not in texts[f], f
    assert '#include "ht_cascade_types.h"' in texts["ht_internal.h"] and "struct HtBlobFeature" not in texts["ht_internal.h"]
    ctx, scan = texts["ht_context.hip"], texts["ht_scan.hip"]
    assert "ht_plan_cascade(" in ctx and "ht_plan_cascade_split(" in ctx and not re.search(r"\bf\.size\b|HT_MAXPTS|\bpz\b", ctx)
    assert "HtBlobFeature" not in scan and "hipMalloc" not in scan and "hipMemcpy(" not in scan
    for short, full in (("PITCH0", "HT_SCAN_PITCH0"), ("P12_BASE", "HT_SCAN_P12_BASE"), ("G_PITCH", "HT_SCAN_G_PITCH"), ("DEEP_LDS_TABLE_BYTES", "HT_DEEP_LDS_TABLE_BYTES")):
        assert re.search(r"constexpr \w+ %s = %s;" % (short, full), scan) and not re.search(r"constexpr \w+ %s = \d" % short, scan), short
    assert re.search(r"constexpr int PATCH1 = HT_PATCH1, PATCH2 = HT_PATCH2, PATCH_BYTES = HT_PATCH_BYTES;", scan)

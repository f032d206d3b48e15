"""The host-side schedule of the camshift calls (headtrackr_amd/csrc/ht_cs_schedule.h: which of the three schedules a track() call takes,
grids, blocks and dynamic LDS of its launches, the chunk plan of the histogram pass, the cluster size, initTracker's row split, the sizes
ht_camshift_reserve allocates) without a device: the header is compiled with AddressSanitizer + UBSan into a host-only harness
(tests/host/cs_schedule_harness.cc) and run as a program.

The expected values (tests/golden/cs_schedule.json) were derived from the expressions of launch_track, fused_threads, hist_chunks,
ht_camshift_init_batch and ht_camshift_reserve as they stood before the header existed; tests/cs_schedule.py restates them in Python for
the GPU tests, and is held against the header here on every case."""
import json
import os
import re
import subprocess

import pytest
from conftest import ROOT

import cs_cases as cc
import cs_schedule as sched
from headtrackr_amd import build

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "cs_schedule.json")))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
OPTS = ("num_cus", "cs_fused_min", "cs_cluster", "cs_cluster_min_px", "cs_iters", "cs_region", "cs_fused_nt", "other_busy")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cs_schedule") / "cs_schedule_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "cs_schedule_harness.cc"), "-o", exe])
    return exe


def _run(harness, tmp_path, lines):
    """one JSON object per case line; the harness exits non-zero on the first invariant that does not hold or the first sanitizer report"""
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([harness, path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _track_line(case):
    o = dict(GOLDEN["defaults"], **{k: case[k] for k in OPTS if k in case})
    return "track %d %d %d %d " % (case["n"], case.get("reserved", case["n"]), case["w"], case["h"]) + " ".join(str(o[k]) for k in OPTS)


def test_defaults_of_the_table_are_the_librarys():
    """the golden rows assume the option defaults of ht_ctx; a changed default must come with a changed table"""
    text = open(os.path.join(CSRC, "ht_internal.h")).read()
    for pattern in (r"int cs_fused_min_streams = 192;", r"bool cs_cluster = true;", r"uint32_t cs_cluster_min_px = 10000;", r"int dbg_cs_iters = 10;",
                    r"int cs_region_cap = 40960;", r"int cs_fused_nt = 0;", r"int num_cus = 256;"):
        assert re.search(pattern, text), pattern
    assert GOLDEN["defaults"] == sched.DEFAULTS


def test_chunk_plan(harness, tmp_path):
    """the recorded (max_chunks, chunk_px, nchunks), and on them and on the pixel counts of the GPU suite's histogram-edge frames, under every
    reservation: chunk_px a multiple of 4 * HIST_NT, the chunks cover the frame, the last one is not empty, nchunks <= max_chunks (asserted
    in the harness and again here)"""
    rows = GOLDEN["chunks"]
    px = sorted(set(GOLDEN["chunk_invariant_pixel_counts"]) | {w * h for w, h in cc.HIST_SIZES} | {r["w"] * r["h"] for r in rows})
    assert {4095, 4096, 4097, 16384, 16385, 32768, 32769} <= set(px)
    more = [(p, n) for p in px for n in GOLDEN["chunk_invariant_reservations"]]
    out = _run(harness, tmp_path, ["chunks %d %d" % (r["w"] * r["h"], r["reserved"]) for r in rows] + ["chunks %d %d" % pn for pn in more])
    for r, got in zip(rows, out):
        assert got == {k: r[k] for k in ("max_chunks", "chunk_px", "nchunks")}, (r, got)
    for (npix, n), got in zip([(r["w"] * r["h"], r["reserved"]) for r in rows] + more, out):
        assert (got["max_chunks"], got["chunk_px"], got["nchunks"]) == sched.chunk_plan(npix, n), (npix, n, got)
        assert got["chunk_px"] % (4 * sched.HIST_NT) == 0
        assert got["nchunks"] * got["chunk_px"] >= npix > (got["nchunks"] - 1) * got["chunk_px"]
        assert got["nchunks"] <= got["max_chunks"]


def test_track_forms(harness, tmp_path):
    """the decision table: both sides of the pixel, stream-count and cluster-size thresholds of the cluster form, of the fused threshold and of
    the 1024 / 512 choice; the options that switch a form off; a forced form wins over everything"""
    cases = GOLDEN["forms"]
    assert len(cases) == 15
    out = _run(harness, tmp_path, [_track_line(c) for c in cases])
    for c, got in zip(cases, out):
        want = c["expect"]
        launch = got["fused"] if got["form"].startswith("FUSED") else got["meanshift"]
        flat = dict(form=got["form"], G=got["G"], region_cap=got["region_cap"], grid=launch["grid"][0], block=launch["block"], lds=launch["lds"])
        for k, v in want.items():
            assert flat[k] == v, (c["name"], k, flat[k], v)
        # the Python restatement the GPU tests use says the same, timers included
        py = sched.track_plan(c["n"], c["w"], c["h"], c.get("reserved"), **{k: c[k] for k in OPTS if k in c})
        timers = [got[k]["timer"] for k in ("fused", "hist", "lut", "meanshift") if got[k]["block"]]
        assert (py["form"], py["G"], py["grid"], py["block"], py["lds"], py["region_cap"], py["timers"]) == (
            flat["form"], flat["G"], flat["grid"], flat["block"], flat["lds"], flat["region_cap"], timers), (c["name"], py, got)
        if not got["form"].startswith("FUSED"):
            assert (got["chunk_px"], got["nchunks"]) == (py["chunk_px"], py["nchunks"])
            assert got["hist"] == {"grid": [got["nchunks"], c["n"]], "block": 1024, "lds": 0, "timer": "cs_hist"}
        if got["form"] == "CLUSTER":
            assert got["lut"] == {"grid": [64, c["n"]], "block": 512, "lds": 0, "timer": "cs_lut"}
    by = {c["name"]: g["form"] for c, g in zip(cases, out)}
    assert by["n191"] != by["n192"] and by["n256"] != by["n257"] and by["n64_128x80"] != by["n65_128x80"] and by["n1_128x80"] != by["n1_96x96"]


def test_the_chunk_plan_of_a_track_call_is_the_reservations(harness, tmp_path):
    """d_cs_hist is sized for hist_max_chunks(reserved streams) chunk histograms per stream: a call of fewer streams must plan with the same
    bound, not with its own n (1 stream of 40 reserved at 1920x1080: 8 chunks, not 127)"""
    c = {"n": 1, "reserved": 40, "w": 1920, "h": 1080}
    (got,) = _run(harness, tmp_path, [_track_line(c)])
    assert (got["nchunks"], got["chunk_px"]) == sched.chunk_plan(1920 * 1080, 40)[:0:-1] == (8, 262144)
    assert sched.chunk_plan(1920 * 1080, 1)[2] == 127


def test_init_plan(harness, tmp_path):
    rows = GOLDEN["init"]
    out = _run(harness, tmp_path, ["init %d %d 256" % (r["n"], r["tallest"]) for r in rows])
    for r, got in zip(rows, out):
        assert got == {"G": r["G"], "rows": r["rows"]}, (r, got)
        assert sched.init_plan(r["n"], r["tallest"]) == (r["G"], r["rows"])


def test_reserve_sizes(harness, tmp_path):
    """bytes of every buffer of a reservation; the cluster form's LUTs and exchange slots stop growing at 64 streams"""
    rows = GOLDEN["reserve"]
    assert [r["nstreams"] for r in rows] == [1, 64, 65, 300]
    out = _run(harness, tmp_path, ["reserve %d" % r["nstreams"] for r in rows])
    for r, got in zip(rows, out):
        assert got == {k: v for k, v in r.items() if k != "nstreams"}, (r, got)
    assert out[1]["lut"] == out[2]["lut"] == out[3]["lut"] == 64 * 4096 * 8 and out[1]["parts"] == out[3]["parts"]
    assert out[2]["states"] > out[1]["states"] and out[2]["hist"] > out[1]["hist"]


def test_the_schedule_is_decided_in_one_place():
    """source layout: each host decision and each host sequence of the camshift calls has one definition under csrc/"""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip", ".inc", ".cc"))}
    everything = "".join(texts.values())
    hdr = texts["ht_cs_schedule.h"]
    assert "#include <hip" not in hdr and '#include "ht_internal.h"' not in hdr
    assert '#include "ht_cs_schedule.h"' in texts["ht_internal.h"] and "struct alignas(16) HtCsState" not in texts["ht_internal.h"]

    def only_in(pattern, name, count=1):
        found = {f: len(re.findall(pattern, t)) for f, t in texts.items() if re.search(pattern, t)}
        assert found == {name: count}, (pattern, found)

    only_in(r"\bvoid hist_chunks\(", "ht_cs_schedule.h")
    only_in(r"\buint32_t hist_max_chunks\(", "ht_cs_schedule.h")
    only_in(r"\bHtCsTrackPlan ht_cs_plan_track\(", "ht_cs_schedule.h")
    only_in(r"constexpr int (?:HIST_MAXCHUNKS|HIST_TARGET_WGS|FUSED_NT|FUSED_NT_SMALL|CS_REGION_CAP|CS_REGION_CAP_SMALL|HIST_NT|CS_NT) =", "ht_cs_schedule.h", 8)
    # one fill of the fused kernel's argument block, one launch site per instantiation
    only_in(r"\bCsFusedArgs ka;", "ht_camshift.hip")
    only_in(r"\bka\.flist\.p\[", "ht_camshift.hip")
    sites = re.findall(r"hipLaunchKernelGGL\(\(k_cs_track_fused<(true|false), (FUSED_NT|FUSED_NT_SMALL)>\)", everything)
    assert sorted(sites) == [("false", "FUSED_NT"), ("false", "FUSED_NT_SMALL"), ("true", "FUSED_NT"), ("true", "FUSED_NT_SMALL")], sites
    # one grow helper; no scratch buffer of the camshift units is allocated by hand
    assert "bp_grow" not in everything
    only_in(r"\bht_status ht_grow_device\(", "ht_internal.h")
    assert not re.search(r"hipMalloc\([^;]*d_(?:cs_seq_out|csp_hist|bp_\w+)", everything)
    assert len(re.findall(r"\bht_grow_device\(c, &c->d_", everything)) == 6
    # one read-back sequence, one chunk-summing loop
    only_in(r"hipMemcpyAsync\(c->h_cs_err, c->d_cs_err,", "ht_camshift.hip")
    only_in(r"v \+= part\[", "ht_camshift.hip")
    # the all-gather is a unit of its own, without device code and without the camshift unit's flag
    cam = texts["ht_camshift.hip"]
    assert "rccl" not in cam.lower() and "ncclAllGather" not in cam and "dlopen" not in cam
    assert "ncclAllGather" in texts["ht_allgather.hip"] and "__global__" not in texts["ht_allgather.hip"]
    assert "ht_allgather.hip" in build.HIP_SOURCES and list(build.EXTRA_FLAGS) == ["ht_camshift.hip"]
    # the context frees no camshift buffer itself
    ctx = texts["ht_context.hip"]
    assert not re.search(r"hip(?:Host)?Free\(\s*c->[dh]_cs", ctx) and not re.search(r"sl\.h_(?:out|flag)", ctx) and "ht_camshift_free(c);" in ctx
    only_in(r"\bvoid ht_camshift_free\(ht_ctx \*c\) \{", "ht_camshift.hip")

"""CPU side of the cluster schedule of the (stream, frame) pair calls (option cs_pairs_cluster=1): the decision table of
ht_cs_plan_track_pairs / ht_cs_plan_init_pairs on both sides of every threshold (a stand-alone harness compiled from ht_cs_schedule.h
alone with AddressSanitizer + UBSan), the option at every layer, the new kernels in the fourth code object within the budgets of the
kernels whose text they share, one definition of every shared helper, and the JavaScript layer on the oracle-backed mock addon.  No
compute calls (no GPU here).  The inputs of the GPU tests (tests/test_gpu_cs_pairs_cluster.py) all come from tests/pair_cases.py /
tests/cs_cases.py, which tests/test_pairs_cpu.py and tests/test_cs_cases_cpu.py prove insensitive to the summation order."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

import pair_cases as pc
from conftest import ROOT, load_golden
from headtrackr_amd import build

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NODE = shutil.which("node")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
CLUSTER_KERNELS = {"k_csp_lut": "k_cs_lut", "k_csp_meanshift_cluster": "k_cs_meanshift_cluster", "k_csp_init_rows": "k_cs_init_rows"}
DEFAULTS = dict(nd=1, w=1920, h=1080, num_cus=256, opt=1, cs_cluster=1, min_px=10000, iters=10, region=40960)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cs_pairs_schedule") / "cs_pairs_schedule_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "cs_pairs_schedule_harness.cc"), "-o", exe])
    return exe


def _run(harness, tmp_path, lines):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([harness, path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return out


def _track(n, **kw):
    o = dict(DEFAULTS, **kw)
    return "track %d %d %d %d %d %d %d %d %d %d" % (n, o["nd"], o["w"], o["h"], o["num_cus"], o["opt"], o["cs_cluster"], o["min_px"], o["iters"], o["region"])


def test_track_pairs_decision_table(harness, tmp_path):
    """the cluster form iff cs_pairs_cluster, cs_cluster, n <= 64, G = min(32, num_cus / n) >= 4, npix >= cs_cluster_min_px and iterations
    > 0 — each condition on both sides of its threshold; otherwise today's one-workgroup form with today's numbers"""
    cases = [  # (line, form, G)
        (_track(2), "CLUSTER", 32), (_track(2, opt=0), "PER_PAIR", 32),
        (_track(2, cs_cluster=0), "PER_PAIR", 32), (_track(2, opt=0, cs_cluster=0), "PER_PAIR", 32),
        (_track(64, nd=16, w=160, h=120), "CLUSTER", 4), (_track(65, nd=17, w=160, h=120), "PER_PAIR", 3),
        (_track(64, nd=16, w=160, h=120, num_cus=255), "PER_PAIR", 3), (_track(64, nd=16, w=160, h=120, num_cus=256), "CLUSTER", 4),
        (_track(2, w=100, h=100), "CLUSTER", 32), (_track(2, w=101, h=99), "PER_PAIR", 32),  # 10 000 / 9 999 pixels
        (_track(2, w=96, h=80), "PER_PAIR", 32),
        (_track(1), "CLUSTER", 32), (_track(8, nd=8), "CLUSTER", 32), (_track(18, nd=6, w=320, h=240), "CLUSTER", 14),
        (_track(2, iters=0), "PER_PAIR", 32), (_track(200, nd=50, w=160, h=120), "PER_PAIR", 1),
    ]
    assert 101 * 99 == 9999
    out = _run(harness, tmp_path, [c[0] for c in cases])
    for (line, form, G), got in zip(cases, out):
        n, nd = (int(v) for v in line.split()[1:3])
        assert (got["form"], got["G"]) == (form, G), (line, got)
        assert got["hist"]["timer"] == "csp_hist" and got["hist"]["grid"][1] == nd and got["hist"]["block"] == 1024
        if form == "CLUSTER":
            assert got["lut"] == {"grid": [64, n], "block": 512, "lds": 0, "timer": "csp_lut"}
            assert got["meanshift"] == {"grid": [n * G, 1], "block": 512, "lds": 0, "timer": "csp_meanshift_cluster"}
            assert n * G <= int(line.split()[5]) and got["region_cap"] == 0
        else:
            assert got["lut"]["block"] == 0
            assert got["meanshift"] == {"grid": [n, 1], "block": 512, "lds": 81920, "timer": "csp_meanshift"} and got["region_cap"] == 40960


def test_chunk_plan_follows_the_distinct_frames_not_the_pairs(harness, tmp_path):
    """8 pairs on one 1080p frame: that frame's 127 chunks; 8 pairs on 8 frames: 32 each — whatever the form"""
    import cs_schedule as sched

    lines = [_track(8, nd=1), _track(8, nd=8), _track(8, nd=1, opt=0), _track(8, nd=8, opt=0), _track(18, nd=6, w=320, h=240), _track(3, nd=2, w=641, h=363)]
    out = _run(harness, tmp_path, lines)
    assert [o["nchunks"] for o in out[:4]] == [127, 32, 127, 32]
    for line, o in zip(lines, out):
        nd, w, h = (int(v) for v in line.split()[2:5])
        assert (o["chunk_px"], o["nchunks"]) == sched.chunk_plan(w * h, nd)[1:], line
        assert o["hist"]["grid"] == [o["nchunks"], nd]


def test_init_pairs_decision_table(harness, tmp_path):
    """the row form iff the option is set and the batch rule holds: fewer than 64 pairs and G = min(32, 2 num_cus / n, ceil(tallest / 16))
    >= 2 — n 63 / 64, heights 16 / 17"""
    cases = [("init 1 63 129 256", True, 8), ("init 1 64 129 256", False, 1), ("init 1 27 16 256", False, 1), ("init 1 27 17 256", True, 2),
             ("init 0 27 129 256", False, 1), ("init 0 63 129 256", False, 1), ("init 1 1 360 256", True, 23), ("init 1 2 1080 256", True, 32),
             ("init 1 27 129 256", True, 9), ("init 1 1 0 256", False, 1)]
    out = _run(harness, tmp_path, [c[0] for c in cases])
    for (line, rows, G), got in zip(cases, out):
        assert (got["rows"], got["G"]) == (rows, G), (line, got)


def test_the_96x80_scene_keeps_its_objects_and_is_insensitive_to_the_summation_order():
    """the one input of tests/test_gpu_cs_pairs_cluster.py that tests/pair_cases.all_multi_sequences() does not hold — small_scene(0) at
    96 x 80, the geometry below cs_cluster_min_px — through the two checks of tests/test_pairs_cpu.py"""
    import cs_cases as cc

    s = pc.small_scene(0, 96, 80)
    assert s.w * s.h == 7680 and s.ntrackers == 4 and s.ncalls == 2
    ref = s.oracle_calls()
    for calls in ref:
        for (_b, sw, to) in calls:
            assert to["width"] > 0 and to["height"] > 0 and sw[2] > 0 and sw[3] > 0, (to, sw)
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            alt = s.oracle_calls()
        assert all(cc.same_call(a, b) for ca, cb in zip(ref, alt) for a, b in zip(ca, cb)), flag
    assert ref == s.oracle_calls()


# ---- the option at every layer ------------------------------------------------------------------------------------------------------------

def test_cs_pairs_cluster_is_an_option_of_the_product_library():
    src = open(os.path.join(CSRC, "ht_context.hip")).read()
    parser = src[src.index("static bool apply_options"):src.index('extern "C" ht_status ht_create')]
    product, _sep, knobs = parser.partition("#ifdef HT_DEBUG_KNOBS")
    assert 'key == "cs_pairs_cluster"' in product and "cs_pairs_cluster" not in knobs
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    assert "cs_pairs_cluster=1" in header[header.index("const char *options;"):header.index("} ht_config;")]
    assert re.search(r"bool cs_pairs_cluster = false;", open(os.path.join(CSRC, "ht_internal.h")).read())  # opt-in
    build.build_lib()
    assert b"cs_pairs_cluster" in open(build.LIB, "rb").read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pairSchedule" in doc and "cs_pairs_cluster=1" in doc
    js = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("opts.pairSchedule", "this.pairSchedule", "'cs_pairs_cluster=1'", "headtrackr.camshift, 'pairSchedule'"):
        assert m in js, m
    # no new C-ABI export and no new addon function for it
    from headtrackr_amd import native

    assert not [s for s in native.SYMBOLS if "cluster" in s]
    assert "pairSchedule" not in open(os.path.join(CSRC, "ht_napi.cc")).read()


def test_launches_come_from_the_plan():
    """csp_launch_track and ht_camshift_init_pairs launch what ht_cs_plan_track_pairs / ht_cs_plan_init_pairs say; the pair launch goes
    through the cluster gate the batch launch goes through, and its read-back fetches the error word"""
    pairs = open(os.path.join(CSRC, "ht_cs_pairs.hip")).read()
    cam = open(os.path.join(CSRC, "ht_camshift.hip")).read()
    internal = open(os.path.join(CSRC, "ht_internal.h")).read()
    assert "ht_cs_plan_track_pairs(in)" in pairs and "ht_cs_plan_init_pairs(c->cs_pairs_cluster, n, max_rh, c->num_cus)" in pairs
    assert "num_cus /" not in pairs and "CL_MAXG" not in pairs.split("// ---- host side")[1]  # no decision of its own
    for fn in ("ht_cs_cluster_gate_begin", "ht_cs_cluster_gate_end"):
        assert re.search(r"ht_status %s\(ht_ctx \*\w+\);" % fn, internal), fn
        assert len(re.findall(r"\b%s\(c\)" % fn, pairs)) == 1 and len(re.findall(r"= %s\(c\)" % fn, cam)) == 1, fn
    assert cam.count("std::mutex> lk(gate.mu") == 4  # forget, fused_threads, begin, end: launch_track holds no lock of its own
    assert "ht_cs_read_back(c, \"ht_camshift_track_pairs\"" in pairs
    launch = pairs[pairs.index("hipLaunchKernelGGL(k_csp_meanshift_cluster"):]
    launch = launch[:launch.index(";")]
    for arg in ("c->d_cs_lut", "c->d_cs_parts", "c->d_cs_err", "c->h_cs_err_direct", "c->cs_barrier_budget", "static_cast<uint32_t *>(nullptr)"):
        assert arg in launch, arg


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------

def test_cluster_pair_kernels_live_in_the_fourth_code_object_and_do_not_spill():
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    assert recorded["camshift"].startswith("2739de9c")
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    new = list(CLUSTER_KERNELS) + ["k_csp_zero_models"]
    mine = [o for o in objs if b"k_csp_meanshift_cluster" in o]
    assert len(mine) == 1 and b"k_bp_project" in mine[0] and all(k.encode() in mine[0] for k in new)
    for o in objs:
        if o is not mine[0]:
            assert not any(k.encode() in o for k in new)
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0], marker
        for k in new:
            assert marker.decode() not in k
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in new:
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
    for mine_k, theirs in CLUSTER_KERNELS.items():  # the same workgroups and LDS as the kernels whose text they are
        assert res[mine_k]["max_flat_workgroup_size"] == res[theirs]["max_flat_workgroup_size"], mine_k
        assert res[mine_k]["group_segment_fixed_size"] == res[theirs]["group_segment_fixed_size"], mine_k
    assert res["k_csp_zero_models"]["max_flat_workgroup_size"] == 1024 and res["k_csp_zero_models"]["group_segment_fixed_size"] == 0
    assert "ht_backproject.hip" not in build.EXTRA_FLAGS


def test_cluster_helpers_and_kernel_texts_have_one_definition():
    """cluster_moments, ClusterSync and CL_UNWRITTEN are defined once, in ht_cs_device.h; k_cs_lut / k_cs_meanshift_cluster /
    k_cs_init_rows and their pair forms are ONE __global__ text each in ht_cs_kernels.inc, which ht_camshift.hip includes part by part
    (the order its code object has) and ht_cs_pairs.hip whole"""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc", ".hip", ".cc"))}
    hdr = texts["ht_cs_device.h"]
    for sig in ("Mom cluster_moments(", "struct ClusterSync {", "constexpr unsigned long long CL_UNWRITTEN ="):
        assert hdr.count(sig) == 1, sig
        assert sum(t.count(sig) for t in texts.values()) == 1, sig
    kern = re.compile(r"__global__[^;{]*?\b(k_csp?_(?:lut|meanshift_cluster|init_rows)|CS_K\((?:lut|meanshift_cluster|init_rows)\))\s*\(")
    found = {f: kern.findall(t) for f, t in texts.items()}
    assert sorted(found.pop("ht_cs_kernels.inc")) == ["CS_K(init_rows)", "CS_K(lut)", "CS_K(meanshift_cluster)"]
    assert not any(found.values()), found
    cam = texts["ht_camshift.hip"]
    parts = [int(m) for m in re.findall(r"#define CS_KERNELS_PART (\d)", cam)]
    assert parts == [1, 3, 2, 4]  # k_cs_init, k_cs_init_rows, k_cs_hist + k_cs_meanshift, [k_cs_track_fused], k_cs_lut + k_cs_meanshift_cluster
    assert cam.index("#define CS_KERNELS_PART 2") < cam.index("void k_cs_track_fused(") < cam.index("#define CS_KERNELS_PART 4")
    assert "CS_KERNELS_PART" not in texts["ht_cs_pairs.hip"] and texts["ht_cs_pairs.hip"].count('#include "ht_cs_kernels.inc"') == 1
    # the spin stays bounded and fence-free, and nothing but the one 8-byte store / load pair carries an entry
    cm = hdr[hdr.index("Mom cluster_moments("):]
    assert "sync.budget" in cm and "*sync.s_timeout = 1" in cm and "atomicOr(sync.err, 1u)" in cm and "sync.err_host" in cm
    assert "fence" not in cm and cm.count("__hip_atomic_store(&slot_parts") == 1 and cm.count("__hip_atomic_load(&slot_parts") == 2


# ---- the JavaScript layer on the mock -----------------------------------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_js_pair_schedule_on_the_cpu_mock(tmp_path, cascade):
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    job = pc.js_job(tmp_path, cascade.blob, load_golden("multitrack.json"))
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "pairs_cluster_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["option_checks"] == 2 + 1 + 3 and out["job_contexts"] == 3 and out["setter_refused"] is True
    assert out["created"] == [None] * 3 + ["cs_pairs_cluster=1"] * 6
    # what the MultiTracker, batch and loop runs return today (tests/test_pairs_cpu.py)
    loop_cs = sum(1 for recs in job["loop"]["expect"] for e in recs if e["mode"] == "CS")
    assert out["calls_total"] == out["calls_exact"] == 6 * 4 + loop_cs + (3 + 2) * 4
    assert out["loop_lost"] == 2 and out["loop_mixed_steps"] >= 1 and out["multi_done"] == 2
    assert out["pair_calls"][0] >= 4 and out["pair_calls"][1] >= 4 + 8

"""CPU side of the back-projection over (stream, frame) pairs (ht_camshift_backproject_pairs): the expectation the GPU tests compare with
reproduces a recording of several reference camshift.Tracker instances on one canvas, the group plan holds its invariants under
AddressSanitizer + UBSan, the entry points exist at every layer, the new kernels live in the fourth code object within their budgets, and
the JavaScript layer runs on the oracle-backed mock addon.  No compute calls (no GPU here)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

import bp_cases
import pair_cases as pc
from conftest import ROOT, load_golden
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NODE = shutil.which("node")
NEW_KERNELS = ("k_bpp_lut", "k_bpp_project<0>", "k_bpp_project<1>")
NEW_SYMBOLS = ("ht_camshift_backproject_pairs", "ht_camshift_backproject_pairs_device")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sequences():
    return [pc.feed_scene(0), pc.same_colour(320, 240)]


# ---- the expectation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ci", [0, 1], ids=["feed0", "same-colour"])
def test_expectation_reproduces_the_reference_recorded_back_projections(ci):
    """tests/golden/multitrack_bp.json: per tracker and track() call the CRC-32 of the reference's getBackProjectionImg().data and its
    getPdf() at a few points.  bp_cases.expected(model of the tracker's rect on frame 0, frame k) gives every recorded value bit for bit:
    the back-projection depends on the model and the frame alone, which is what the GPU tests' expectation assumes."""
    case, s = load_golden("multitrack_bp.json")["cases"][ci], _sequences()[ci]
    assert (case["name"], case["w"], case["h"]) == (s.name, s.w, s.h) and case["rects"] == [list(map(int, r)) for r in s.rects]
    assert load_golden("multitrack.json")["cases"][ci]["name"] == case["name"]  # the two sequences of multitrack.json
    assert len(case["trackers"]) == s.ntrackers
    for j, calls in enumerate(case["trackers"]):
        model = bp_cases.model_of(s.frames[0], s.rects[j])
        assert [c["frame"] for c in calls] == list(range(1, s.ncalls + 1))
        for call in calls:
            rgba, pdf = bp_cases.expected(model, s.frames[call["frame"]])
            assert bp_cases.crc(rgba) == call["crc"], (case["name"], j, call["frame"])
            assert len(call["pdf"]) >= 8
            for x, y, v in call["pdf"]:
                assert pdf[y, x] == v, (case["name"], j, call["frame"], x, y, pdf[y, x], v)
            assert any(v > 0 for _x, _y, v in call["pdf"]) and any(v == 0 for _x, _y, v in call["pdf"])


# ---- the group plan -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bp_pairs_plan") / "bp_pairs_plan_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "bp_pairs_plan_harness.cc"), "-o", exe])
    return exe


def _plan_cases(G):
    """frame lists: pairs-per-frame counts 1, G, G + 1, 2 G + 1 — one frame alone, the four together in blocks, interleaved round-robin and
    shuffled —, with frame numbers that leave bound frames unused"""
    counts = [1, G, G + 1, 2 * G + 1]
    frames = [7, 0, 5, 2]  # frames 1, 3, 4, 6 are named by no pair
    cases = [[f] * c for f, c in zip(frames, counts)]
    blocks = [f for f, c in zip(frames, counts) for _ in range(c)]
    cases.append(blocks)
    left, rr = dict(zip(frames, counts)), []
    while any(left.values()):
        for f in frames:
            if left[f]:
                rr.append(f)
                left[f] -= 1
    cases.append(rr)
    for seed in (9801, 9802):
        cases.append([blocks[i] for i in pc.shuffled(len(blocks), seed)])
    return cases


@pytest.mark.parametrize("G", [2, 4])
def test_group_plan_invariants_under_sanitizers(harness, tmp_path, G):
    cases = _plan_cases(G)
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("\n".join(" ".join(map(str, [G] + c)) for c in cases) + "\n")
    r = subprocess.run([harness, path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(cases)
    for frames, got in zip(cases, out):
        groups = got["groups"]
        # every pair in exactly one group
        assert sorted(i for g in groups for i in g["pairs"]) == list(range(len(frames)))
        distinct = list(dict.fromkeys(frames))
        for g in groups:
            assert 1 <= g["count"] == len(g["pairs"]) <= G
            assert all(frames[i] == g["frame"] for i in g["pairs"]) and g["slot"] == distinct.index(g["frame"])
            assert g["pairs"] == sorted(g["pairs"])
        # the frame order holds: groups in the order of their first pairs, a frame's pairs in call order through its groups, and only the
        # last group of a frame may be short
        assert [g["pairs"][0] for g in groups] == sorted(g["pairs"][0] for g in groups)
        for f in distinct:
            mine = [g for g in groups if g["frame"] == f]
            assert [i for g in mine for i in g["pairs"]] == [i for i, x in enumerate(frames) if x == f]
            assert all(g["count"] == G for g in mine[:-1])
            assert len(mine) == -(-frames.count(f) // G)


def test_group_plan_refuses_what_the_kernels_cannot_hold(harness, tmp_path):
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.write("0 1 1 2\n5 1 1 2\n4\n")
    r = subprocess.run([harness, path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
    assert [json.loads(line) for line in r.stdout.splitlines()] == [{"groups": []}] * 3


def test_group_plan_is_written_once_without_hip():
    text = open(os.path.join(CSRC, "ht_bp_pairs_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    unit = open(os.path.join(CSRC, "ht_bp_pairs.hip")).read()
    assert '#include "ht_bp_pairs_plan.h"' in unit and "ht_bpp_plan(" in unit and "struct HtBppGroup" not in unit
    assert "csp_plan(" in unit and "csp_upload(" in unit and "k_csp_hist" in unit and "ht_cs_hist_plan(" in unit
    assert "hipStreamSynchronize" not in unit.split("bpp_enqueue")[1].split("}  // namespace")[0]  # the tables never wait for the stream


# ---- the entry points at every layer ------------------------------------------------------------------------------------------------------

def test_new_symbols_exist_at_every_layer():
    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    exported = set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    for name, js in zip(NEW_SYMBOLS, ("camshiftBackProjectPairs", "camshiftBackProjectPairsDevice")):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS
        row = re.search(r"^\| `%s` \|.*\| ([^|]*) \|$" % name, doc, flags=re.M)
        assert row and js in row.group(1), name
        assert js in exported
        assert getattr(L, name)(None, None, 0, 0, None, 0) == -1  # all-zero arguments: a status, never a crash
    assert L.ht_abi_version() == 2
    from headtrackr_amd.api import Context

    assert callable(Context.camshift_backproject_pairs) and callable(Context.camshift_backproject_pairs_device)
    js = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("this.backProjectionPairs", "this.getBackProjectionImgs", "this.getBackProjectionImg = function (i)", "this.getPdf = function (i)"):
        assert m in js, m
    assert os.path.exists(os.path.join(ROOT, "tools", "gpu_bp_pairs.py"))


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_addon_exports_the_calls_and_refuses_malformed_arguments():
    build.build_lib()
    addon = build.build_addon()
    js = ("const A = require(%r); const r = [typeof A.camshiftBackProjectPairs, typeof A.camshiftBackProjectPairsDevice];"
          "for (const f of [A.camshiftBackProjectPairs, A.camshiftBackProjectPairsDevice]) for (const args of [[], [1], [{}, new Int32Array(2)], [null, 3, 4, 5, 6, 7]])"
          "{ try { f.apply(null, args); r.push('no throw'); } catch (e) { r.push(e instanceof TypeError ? 'TypeError' : String(e)); } }"
          "console.log(JSON.stringify(r));" % addon)
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function", "function"] + ["TypeError"] * 8


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------

def test_kernels_live_in_the_fourth_code_object_within_their_budgets():
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_bpp_project" in o]
    assert len(mine) == 1 and b"k_bpp_lut" in mine[0] and b"k_csp_hist" in mine[0] and b"k_bp_project" in mine[0]
    for marker in list(fingerprint.UNITS.values()) + [b"k_bp_project", b"k_bp_lut", b"k_cs_hist"]:
        for k in NEW_KERNELS:
            assert marker.decode() not in k, (marker, k)
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0], marker
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in NEW_KERNELS:
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (k, r)
    for k in ("k_bpp_project<0>", "k_bpp_project<1>"):
        assert res[k]["vgpr_count"] <= 64 and res[k]["group_segment_fixed_size"] == 64 * 1024 and res[k]["max_flat_workgroup_size"] == 1024, (k, res[k])
    assert res["k_bpp_lut"]["max_flat_workgroup_size"] == 512
    csrc = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_backproject.hip", "ht_bp_pairs.hip")}
    inc = re.findall(r'^\s*#\s*include\s+"([^"]+)"', csrc["ht_backproject.hip"], flags=re.M)
    assert inc[-2:] == ["ht_cs_pairs.hip", "ht_bp_pairs.hip"] and "ht_bp_pairs.hip" not in build.HIP_SOURCES
    # the histogram kernel is launched, not copied; the bin and the load-laundering macro are the shared ones
    assert len(re.findall(r"__global__", csrc["ht_bp_pairs.hip"])) == 2 and "cs_bin(" in csrc["ht_bp_pairs.hip"] and "CS_BATCH_LOADED(" in csrc["ht_bp_pairs.hip"]


def test_project_kernel_reads_the_frame_in_batches_behind_one_barrier():
    """on the code object: the four LUT loads ride in front of the first batch of four 16-byte pixel loads (8 loads before the first
    `s_waitcnt vmcnt`), later batches hold 4; one s_barrier, no atomics, no scratch"""
    build.build_lib()
    dz = _tool("disasm")
    for form in ("k_bpp_projectILi0", "k_bpp_projectILi1"):
        txt = dz.disasm(form)
        assert txt, form
        runs, run = [], 0
        for ln in txt.splitlines()[1:]:
            op = (ln.split() or [""])[0]
            if op == "global_load_dwordx4":
                run += 1
            elif op == "s_waitcnt" and "vmcnt" in ln:
                runs.append(run)
                run = 0
        runs.append(run)
        runs.sort(reverse=True)
        assert runs[0] >= 8 and runs[1] >= 4, (form, runs[:4])
        assert "global_atomic" not in txt and "ds_add" not in txt and "scratch_" not in txt
        assert sum(1 for ln in txt.splitlines() if (ln.split() or [""])[0] == "s_barrier") == 1


# ---- the JavaScript layer on the mock -----------------------------------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_js_layer_on_the_cpu_mock(tmp_path):
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    golden = load_golden("multitrack_bp.json")
    job = {"cases": []}
    for case, s in zip(golden["cases"], _sequences()):
        files = []
        for k, f in enumerate(s.frames):
            p = tmp_path / f"{case['name']}_{k}.raw"
            f.tofile(p)
            files.append(str(p))
        job["cases"].append({"name": case["name"], "w": s.w, "h": s.h, "rects": case["rects"], "frames": files, "trackers": case["trackers"]})
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "bp_pairs_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    ncalls = sum(len(c["trackers"][0]) for c in golden["cases"])                          # track() calls: 4 + 4
    ntr = sum(len(c["trackers"]) * len(c["trackers"][0]) for c in golden["cases"])        # (3 + 2) x 4
    assert out["imgs_calls"] == 2 * ncalls and out["crc_checks"] == out["pdf_checks"] == out["single_checks"] == 2 * ntr
    # entry point present: one call per getBackProjectionImgs(), getPdf(i) and getBackProjectionImg(i); absent: none
    assert out["device_calls_present"] == ncalls + 2 * ntr and out["device_calls_absent"] == 0
    assert out["batch_checks"] == 3 + 2 + 5 + 1 and out["missing_checks"] == 1

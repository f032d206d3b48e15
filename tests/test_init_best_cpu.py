"""The record-driven initTracker (ht_camshift_init_best) without a GPU: the inputs of tests/init_best_cases.py provably reach the states
they are named after (from the CPU oracle alone), and the decision function the resolve kernel compiles (csrc/ht_cs_best_plan.h) gives, in
a stand-alone program under AddressSanitizer + UBSan, what facetrackr.js:97-107 gives — `confidence > threshold`, Math.floor."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import init_best_cases as ib
from conftest import ROOT

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
OVER_CAP = 1  # HT_GRP_ST_OVER_CAP


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------

def test_inputs_reach_the_states_they_are_named_after(cascade):
    counts = ib.raw_counts(cascade.blob)
    best = ib.best(cascade.blob)
    assert len(ib.frames()) == ib.NFRAMES == 6
    assert all(n <= 21 for n in counts[: ib.TILED]) and counts[ib.NOISE] == 0
    assert counts[ib.TILED] == 129 and 64 < counts[ib.TILED] < 1024  # above group_cap=64, the lowest cap, below the default one
    want = {"two_faces_320x240": 8.488, "mixed2_320x240": 6.785, "mixed5_320x240": 10.828, "c1_face_320x240": 3.924}
    for f, name in enumerate(ib.GOLDEN_FRAMES):
        if name in want:
            assert best[f]["neighbors"] > 0 and round(float(best[f]["confidence"]), 3) == want[name], (name, best[f])
    assert best[ib.NOISE]["neighbors"] == 0 and best[ib.NOISE]["confidence"] == -10000.0
    assert round(float(best[ib.TILED]["confidence"]), 3) == 6.283 and best[ib.TILED]["neighbors"] == 8
    # the two thresholds split the frames differently, and each leaves faces on both sides
    faces = {t: [f for f in range(ib.NFRAMES) if ib.decide(best[f], t)[0] == ib.FACE] for t in ib.THRESHOLDS}
    assert faces[-10.0] == [0, 2, 3, 4, 5] and faces[5.0] == [0, 2, 4, 5]
    # every best rect is at least 32 rows tall (the row form of initTracker has G >= 2), inside the canvas, and not integral
    for f in faces[-10.0]:
        x, y, w, h = ib.floor_rect(best[f])
        assert h >= 32 and 0 <= x and 0 <= y and x + w <= ib.W and y + h <= ib.H
        assert any(float(best[f][k]) != int(best[f][k]) for k in ("x", "y", "width", "height"))
    # the pair list: every stream once, frame 0 three times, every frame named
    assert sorted(s for s, _f in ib.PAIRS) == list(range(ib.STREAMS)) and sorted({f for _s, f in ib.PAIRS}) == list(range(ib.NFRAMES))
    assert [f for _s, f in ib.PAIRS].count(0) == 3


# ---- the decision function under the sanitizers -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("init_best") / "init_best_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "init_best_harness.cc"), "-o", exe])
    return exe


def _case(rec, thr, status=0, nhits=10, bad=0, cap=1 << 20, collected=0, fb=None):
    """(packed input, expected code, expected rect).  rec: x, y, width, height, confidence, neighbors"""
    rec8 = [float(v) for v in rec] + [0.0, 1.0]
    blob = struct.pack("<8dd4I2i4i", *rec8, float(thr), status, nhits, bad, cap, collected, int(fb is not None), *(fb or (0, 0, 0, 0)))
    assert len(blob) == 112
    deferred = nhits > cap or bad != 0 or (not collected and (status & OVER_CAP) != 0)
    r = dict(zip(("x", "y", "width", "height", "confidence", "neighbors"), rec))
    code, rect = ib.decide(r, thr, fb, deferred)
    return blob, code, rect


def _cases(cascade):
    best = ib.best(cascade.blob)
    fb = (-3, 7, 160, 120)
    out = []
    for r in best:  # the oracle's records at both thresholds, with and without a fallback
        rec = [float(r[k]) for k in ("x", "y", "width", "height", "confidence", "neighbors")]
        for thr in ib.THRESHOLDS:
            out += [_case(rec, thr), _case(rec, thr, fb=fb)]
        out.append(_case(rec, float(r["confidence"])))          # tie: confidence == min_confidence is not a face
        out.append(_case(rec, float(r["confidence"]), fb=fb))
        out.append(_case(rec, np.nextafter(float(r["confidence"]), -np.inf)))  # one ulp below: a face (when it has neighbours)
    face = [23.35, 31.88, 42.66, 42.66, 8.5, 9.0]
    out.append(_case(face[:5] + [0.0], -10.0))                   # neighbours 0: no face whatever the confidence
    out.append(_case(face[:5] + [0.0], -10.0, fb=fb))
    none = [0.0, 0.0, 0.0, 0.0, -10000.0, 0.0]                   # facetrackr.js:233-241
    out += [_case(none, -10.0), _case(none, -10.0, fb=fb), _case(none, -20000.0), _case(none[:5] + [1.0], -20000.0)]
    for collected in (0, 1):                                     # over-cap status with and without the "collected" flag
        out += [_case(face, -10.0, status=OVER_CAP, collected=collected), _case(face, -10.0, status=OVER_CAP, collected=collected, fb=fb),
                _case(none, -10.0, status=OVER_CAP, collected=collected, fb=fb), _case(face, -10.0, status=2, collected=collected)]
        out += [_case(face, -10.0, nhits=11, cap=10, collected=collected, fb=fb), _case(face, -10.0, nhits=10, cap=10, collected=collected),
                _case(face, -10.0, bad=1, collected=collected, fb=fb)]  # batch overflow, exactly full, a bad hit
    for xy in ([-0.5, -1.0, 0.999, 1.0], [-0.0, 0.0, 1e-300, -1e-300], [-7.25, 7.75, 2147483646.5, -2147483647.5]):  # floor(-0.5) = -1
        out.append(_case(xy + [1.0, 1.0], 0.0))
    huge = [[1e300, -1e300, float("inf"), float("-inf")], [2147483647.0, 2147483648.0, -2147483648.0, -2147483649.0],
            [float("nan"), 2147483647.5, -2147483648.5, 4294967296.0]]   # saturation, NaN -> 0
    for xy in huge:
        out.append(_case(xy + [1.0, 1.0], 0.0))
    out += [_case(face[:4] + [float("nan"), 3.0], -10.0, fb=fb), _case(face[:4] + [float("inf"), 3.0], 1e308), _case(face[:5] + [float("nan")], -10.0),
            _case(face, float("inf")), _case(face, float("-inf"))]
    return out


def test_decision_function_under_the_sanitizers(harness, cascade, tmp_path):
    cases = _cases(cascade)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(b"".join(c[0] for c in cases))
    r = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and r.stdout.strip() == f"cases {len(cases)}", (r.returncode, r.stdout, r.stderr[-3000:])
    got = np.fromfile(fout, dtype=np.int32).reshape(-1, 5)
    assert len(got) == len(cases)
    for k, (_blob, code, rect) in enumerate(cases):
        assert (int(got[k, 0]), tuple(int(v) for v in got[k, 1:])) == (code, rect), (k, got[k], code, rect)
    codes = [c[1] for c in cases]
    assert {ib.UNTOUCHED, ib.FACE, ib.FALLBACK, ib.DEFERRED} == set(codes)  # every outcome occurs
    assert (-1, -1, 0, 1) in [c[2] for c in cases] and (2147483647, -2147483648, 2147483647, -2147483648) in [c[2] for c in cases]


# ---- the build, the N-API shim and the JavaScript layer -------------------------------------------------------------------------------------

NEW_EXPORTS = ("ht_camshift_init_best", "ht_camshift_init_best_result")
JS_CALLS = ("camshiftInitBest", "camshiftInitBestResult")
NODE = shutil.which("node")
HAVE_NODE = NODE is not None and os.path.exists("/usr/include/node/node_api.h")


def test_library_and_python_layer_bind_the_new_entry_points():
    from headtrackr_amd import build, native
    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name) and name in native.SYMBOLS
    assert L.ht_camshift_init_best(None, None, 0, 0.0, None) == -1 and L.ht_camshift_init_best_result(None, 0, None, None) == -1
    assert callable(Context.camshift_init_best) and callable(Context.camshift_init_best_result)
    assert (native.HT_CSB_UNTOUCHED, native.HT_CSB_FACE, native.HT_CSB_FALLBACK, native.HT_CSB_DEFERRED) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    assert "HT_CSB_UNTOUCHED = 0, HT_CSB_FACE = 1, HT_CSB_FALLBACK = 2, HT_CSB_DEFERRED = 3" in hdr


def test_resolve_kernel_lives_in_the_fourth_code_object_and_the_pair_kernels_keep_their_budgets():
    """the new unit is part of the back-projection unit's code object; the guard costs the init kernels no register budget: no spills, no
    scratch, k_csp_init within the 128 VGPRs of a 1024-thread workgroup"""
    import importlib.util

    from headtrackr_amd import build
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_csb_resolve" in o]
    assert len(mine) == 1 and b"k_bp_project" in mine[0] and b"k_csp_init" in mine[0]
    assert "ht_cs_best.hip" not in build.HIP_SOURCES
    assert '#include "ht_cs_best.hip"' in open(os.path.join(CSRC, "ht_cs_pairs.hip")).read()  # ... which ht_backproject.hip includes
    assert "CS_INIT_SKIP" not in open(os.path.join(CSRC, "ht_camshift.hip")).read()  # the batch unit leaves the hook empty
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in ("k_csb_resolve", "k_csp_init", "k_csp_init_rows", "k_csp_zero_models"):
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
    assert res["k_csp_init"]["vgpr_count"] <= 128 and res["k_csb_resolve"]["group_segment_fixed_size"] == 0


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_exports_the_new_calls_and_refuses_malformed_arguments():
    """tests/js/addon_args.js picks the new functions up by itself: too few or wrong arguments end in an exception, never silently"""
    from headtrackr_amd import build

    addon = build.build_addon()
    assert addon is not None
    js = "const A = require(%r); console.log(JSON.stringify(%r.map(function (k) { return typeof A[k]; })));" % (addon, list(JS_CALLS))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function"] * len(JS_CALLS)
    js = ("const A = require(%r); const out = []; [[], [{}], [{}, new Int32Array(2)]].forEach(function (a) { try { A.camshiftInitBest.apply(null, a); out.push('silent'); }"
          " catch (e) { out.push(e instanceof TypeError ? 'TypeError' : 'Error'); } }); try { A.camshiftInitBestResult({}); out.push('silent'); } catch (e)"
          " { out.push(e instanceof TypeError ? 'TypeError' : 'Error'); } console.log(JSON.stringify(out));" % addon)
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["TypeError"] * 4  # too few arguments: a TypeError
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "addon_args.js")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert not set(out["silent"]) & set(JS_CALLS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_still_loads_against_a_c_abi_without_the_new_symbols(tmp_path):
    """tests/js/abi_stub.cc defines neither export: the shim calls them directly, so the addon linked against the stub loads and
    reproduces its recorded transcript"""
    import addon_stub

    got = addon_stub.run(addon_stub.NAPI_SRC, tmp_path)
    assert got["transcript"] == json.load(open(addon_stub.GOLDEN))
    src = open(addon_stub.NAPI_SRC).read()
    for sym in NEW_EXPORTS:
        assert ("&" + sym) not in src and sym + "(" in src
    assert not any(sym in open(os.path.join(ROOT, "tests", "js", "abi_stub.cc")).read() for sym in NEW_EXPORTS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_js_device_handoff_on_the_cpu_mock(tmp_path, cascade):
    """new ccv.DeviceBatch(.., {grouping: 'device', handoff: 'device'}) on the oracle-backed mock: detectStep, enqueue -> track -> finish ->
    collect with and without {feeds}, and a mini C5 loop return what the default hand-off returns; the RangeErrors, the missing-function
    Error, and no tracker initialised from the host under 'device'"""
    import group_cases as gc
    from conftest import load_golden
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    job = gc.js_job(tmp_path, cascade.blob, load_golden("detect.json"))
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "init_best_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] >= 11 and out["range_errors"] == 7 and out["missing_checks"] == 3
    assert out["fallbacks"] == 1 and out["initialised"] == 2 and out["loop_tracks"] == 33
    assert not set(out["host_calls"]) & set(JS_CALLS)
    assert out["host_calls"]["camshiftInitBound"] == 1 and out["host_calls"]["camshiftInitPairs"] == 1
    assert out["device_calls"]["camshiftInitBest"] == 2 and "camshiftInitPairs" not in out["device_calls"] and "camshiftInitBound" not in out["device_calls"]

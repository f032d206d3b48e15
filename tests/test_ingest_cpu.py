"""CPU-side checks of the device drawImage (ht_draw_frames / ht_draw_frames_device): the expectation the GPU tests compare with is the
declared resampler's and the reference's own, the new entry points exist at every layer, the new kernel leaves the three
fingerprinted code objects alone, its kernel fits its budget, and the JavaScript facade's host logic (fallback included) works on the
mock addon.  No compute calls on the library (no GPU here)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ingest_cases as ic
from conftest import ROOT
from headtrackr_amd import build, native
from oracle import ht_oracle as ho

NODE = shutil.which("node")
CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NEW_SYMBOLS = ("ht_draw_frames", "ht_draw_frames_device", "ht_device_download")
NEW_ADDON = ("drawFrames", "drawFramesDevice", "deviceDownload")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cpu_cases():
    """(source frame, rect | None, dw, dh): every small ratio family with noise, the 2:1 ties, and every rect of the rect list"""
    out = []
    for (sw, sh), (dw, dh) in ic.CPU_RATIOS:
        out.append((ic.noise(sw, sh, 3 * sw + sh), None, dw, dh))
        if (sw, sh) == (2 * dw, 2 * dh):
            out.append((ic.ties(sw, sh, 11), None, dw, dh))
    for (sw, sh), (dw, dh) in (((333, 217), (97, 81)), ((23, 23), (40, 30))):
        for k, rect in enumerate(ic.rects_for(sw, sh)):
            out.append((ic.outside_filled(ic.smooth(sw, sh, 20 + k), rect, 30 + k), rect, dw, dh))
    return out


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_expectation_equals_the_declared_resampler_and_the_facade_falls_back(tmp_path):
    """`expected` == oracle/canvas_shim.js's resample == headtrackr_amd/js/canvas.js's drawImage, byte for byte (CRC-32 of all four
    channels), over the case list; ccv.drawFrames returns the same bytes through its fallback (an addon without the calls: the plain
    tests/js/mock_addon.js) and through the device route (tests/js/mock_addon_ingest.js); ccv.DeviceBatch's source buffer and draw calls
    drive the addon as documented."""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    cases, job = cpu_cases(), {"cases": []}
    for k, (src, rect, dw, dh) in enumerate(cases):
        fn = tmp_path / f"s{k}.raw"
        src.tofile(fn)
        job["cases"].append(dict(file=str(fn), sw=src.shape[1], sh=src.shape[0], dw=dw, dh=dh, rect=list(rect) if rect else None))
    job["batch_case"] = next(k for k, c in enumerate(job["cases"]) if (c["sw"], c["sh"], c["dw"], c["dh"]) == (333, 217, 160, 120))
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "ingest_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    want = [ic.crc(ic.expected(src, rect, dw, dh)) for src, rect, dw, dh in cases]
    assert out["shim_crc"] == want
    assert out["canvas_crc"] == want
    assert out["fallback_checks"] == len(cases) and out["device_checks"] == len(cases) and out["batch_checks"] == 4
    assert len(cases) >= 30


def test_ties_are_ties_of_both_parities():
    """the constructed 2:1 content: every block sums to 4 q + 2, so its mean is q + 0.5 exactly; round-half-even gives q for even q and
    q + 1 for odd q, floor(v + 0.5) would give q + 1 everywhere — and both parities occur, so the difference shows"""
    f = ic.ties(194, 162, 11).astype(np.int64)
    s = f[0::2, 0::2] + f[0::2, 1::2] + f[1::2, 0::2] + f[1::2, 1::2]
    assert (s % 4 == 2).all()
    q = (s - 2) // 4
    want = ic.expected(f.astype(np.uint8), None, 97, 81)
    assert np.array_equal(want, q + (q & 1))
    assert not np.array_equal(want, q + 1) and 0.3 < (q & 1).mean() < 0.7


def test_expectation_reproduces_the_reference_recorded_canvases_and_tracking():
    """tests/golden/ingest.json was recorded from the UNMODIFIED reference drawing videos larger than its canvas (main.js:170): every
    canvas CRC-32 is reproduced by `expected`, and the oracle run on those canvases reproduces the reference's tracking objects — the
    VJ frame's best face exactly, every CS frame within the criteria the camshift tests apply to golden cases (sizes equal, position
    +-1 px; here bit-exact)"""
    import math

    from cs_cases import ANGLE_TOL
    from headtrackr_amd.cascade import load_cascade

    blob = load_cascade().blob
    g = ic.golden()
    assert {(c["vw"], c["vh"], c["w"], c["h"]) for c in g["cases"]} >= {(640, 480, 320, 240), (1280, 720, 320, 240), (1920, 1080, 320, 240), (333, 217, 160, 120)}
    assert any(c["kind"] == "mainjs" for c in g["cases"])
    for case in g["cases"]:
        cs, seen_vj, ncs = None, False, 0
        for k, call in enumerate(case["calls"]):
            canvas = ic.expected(ic.golden_video(case, k), None, case["w"], case["h"])
            assert ic.crc(canvas) == call["canvas_crc"], (case["name"], k)
            if call["detection"] == "WB":
                assert not seen_vj
            elif call["detection"] == "VJ":
                best = ho.best_faces(canvas[None], blob, 1)[0]
                assert best["confidence"] > -10
                if "confidence" in call:
                    for key in ("x", "y", "width", "height", "confidence"):
                        assert best[key] == call[key], (case["name"], k, key)
                cs = ho.Camshift(True)
                cs.init_tracker(canvas, [math.floor(best[key]) for key in ("x", "y", "width", "height")])
                seen_vj = True
            else:
                assert call["detection"] == "CS" and cs is not None and call["width"] > 0 and call["height"] > 0
                _, to = cs.track(canvas)
                for key in ("x", "y", "width", "height"):
                    assert to[key] == call[key], (case["name"], k, key, to, call)
                d = abs(to["angle"] - call["angle"])
                assert min(d, abs(d - math.pi)) <= ANGLE_TOL
                ncs += 1
        assert seen_vj and ncs >= 3, case["name"]


def test_new_entry_points_exist_at_every_layer():
    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ingest: the loop's video -> canvas copy (main.js:170, 312)" in header
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), f"libheadtrackr_hip.so does not export {name}"
        assert name in native.SYMBOLS
        assert f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "main.js:170" in doc[:doc.index("## 1.")]
    assert L.ht_draw_frames_device(None, None, 0, 0, 0, 0, 0, None, None, 0) < 0  # all-zero arguments: a status, never a crash
    assert L.ht_draw_frames(None, None, 0, 0, 0, 0, None) < 0
    assert L.ht_abi_version() == 2
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    exported = set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    assert set(NEW_ADDON) <= exported
    addon = build.build_addon()
    if addon is None or NODE is None:
        pytest.skip("node or its N-API headers are missing on this machine: the addon is not built")
    js = "const A = require(%r); console.log(JSON.stringify(%s.map(function (k) { return typeof A[k]; })));" % (addon, json.dumps(list(NEW_ADDON)))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function"] * len(NEW_ADDON)


def test_recorded_code_objects_are_unchanged_and_the_draw_kernel_lives_outside_them():
    """profiles/traffic.json's hardware counters belong to the machine code of the pyramid, scan and camshift units.  The draw kernel
    shares the pyramid's tap helper through a header (ht_resample_tap.h) — the pyramid's code object must not have changed by a byte —
    and is compiled (ht_ingest.hip, included by ht_backproject.hip) into the ONE other code object of the library, whose kernel names
    carry none of the fingerprint's markers."""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    assert os.path.exists(os.path.join(CSRC, "ht_ingest.hip"))
    assert '#include "ht_ingest.hip"' in open(os.path.join(CSRC, "ht_backproject.hip")).read()
    for marker in fingerprint.UNITS.values():
        assert marker.decode() not in "ht_ingest.hip k_draw_frames"
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_draw_frames" in o]
    assert len(mine) == 1
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0], marker
        assert sum(1 for o in objs if marker in o) == 1, marker
    # the tap helper exists once, in the shared header
    assert "rs_tap(int i" in open(os.path.join(CSRC, "ht_resample_tap.h")).read()
    for unit in ("ht_pyramid.hip", "ht_ingest.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert '#include "ht_resample_tap.h"' in text and "RsTap rs_tap(int i" not in text, unit


def test_draw_kernel_fits_its_budget_and_is_not_contracted():
    """code-object metadata and disassembly: no spills, no scratch, <= 64 VGPRs (8 wavefronts per SIMD), under 4 KB of LDS (the
    tile's 80 taps of 24 bytes, no pixel staging); every binary64 product and sum is an instruction of its own (a contracted v_fma_f64 would round
    differently from the declared sequence), the rounding is v_rndne_f64 (round half to even), tap pairs are read as 8-byte loads and
    a pixel is stored as one dword"""
    build.build_lib()
    kr, dz = _tool("kernel_resources"), _tool("disasm")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    r = res["k_draw_frames"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 4096, r
    txt = dz.disasm("k_draw_frames")
    assert txt
    ops = [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]
    assert not any(o.startswith("v_fma") or o.startswith("scratch_") for o in ops)
    assert sum(o.startswith("v_rndne_f64") for o in ops) == 16  # 4 rows x 4 channels
    assert sum(o == "global_load_dwordx2" for o in ops) == 8 and sum(o.startswith("global_store_dword") for o in ops) == 4
    assert sum(o == "s_barrier" for o in ops) == 1

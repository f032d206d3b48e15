"""CPU-side checks of the device back-projection (ht_camshift_backproject): the expectation the GPU tests compare with is the
reference's own, the new entry points exist at every layer, the new translation unit leaves the three fingerprinted code objects alone,
and its kernels fit their budgets.  No compute calls (no GPU here)."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

import bp_cases
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NEW_KERNELS = ("k_bp_lut", "k_bp_project<0>", "k_bp_project<1>")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", bp_cases.golden_cases(), ids=lambda c: c["name"])
def test_expectation_reproduces_the_reference_recorded_bytes(case):
    """guards the GPU tests' inputs: numpy's restatement gives the CRC-32 of the reference's getBackProjectionImg().data and its
    getPdf() samples, bit for bit, for every golden case (model rect partly outside the frame and the all-zero image included)"""
    rgba, pdf = bp_cases.golden_expected(case["name"])
    assert bp_cases.crc(rgba) == case["backprojection_crc"]
    for x, y, v in case["pdf_samples"]:
        assert pdf[y, x] == v, (case["name"], x, y, pdf[y, x], v)  # getPdf()[x][y]
    assert (rgba[..., 3] == 255).all() and (rgba[..., 0] == rgba[..., 1]).all() and (rgba[..., 0] == rgba[..., 2]).all()


def test_library_and_addon_export_the_new_entry_points():
    build.build_lib()
    L = native.lib()
    for name in ("ht_camshift_backproject", "ht_camshift_backproject_device"):
        assert hasattr(L, name), f"libheadtrackr_hip.so does not export {name}"
        assert name in native.SYMBOLS
        f = getattr(L, name)
        assert f(None, 0, 0, 0, None, 0) < 0  # all-zero arguments: a status, never a crash
    assert (native.HT_BP_RGBA8, native.HT_BP_F64) == (0, 1)
    addon = build.build_addon()
    if addon is None:
        pytest.skip("no N-API headers on this machine: the addon is not built")
    js = ("const A = require(%r); console.log(JSON.stringify([typeof A.camshiftBackProject, typeof A.camshiftBackProjectDevice, A.BP_RGBA8, A.BP_F64]));"
          % addon)
    r = subprocess.run(["node", "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function", "function", 0, 1]


def test_recorded_code_objects_are_unchanged_and_the_new_unit_is_its_own():
    """profiles/traffic.json's hardware counters belong to the machine code of the pyramid, scan and camshift units: adding the
    back-projection must not touch it.  The new kernels live in a fourth gfx950 code object and their names carry none of the
    substrings the fingerprint finds a unit by (or that object would silently replace a recorded unit)."""
    from benchlib import fingerprint

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    kr = _tool("kernel_resources")
    names = [kr.short(k) for k, v in kr.kernel_resources().items() if "vgpr_count" in v]
    for k in NEW_KERNELS:
        assert k in names, (k, names)
        for marker in fingerprint.UNITS.values():
            assert marker.decode() not in k
    # one code object per translation unit with device code (ht_context.hip and ht_allgather.hip have none): the three recorded ones and
    # ONE more, which holds the new kernels and none of the markers
    objs = _gfx950_code_objects(build.LIB)
    with_device_code = [s for s in build.HIP_SOURCES if "__global__" in open(os.path.join(CSRC, s)).read()]
    assert len(objs) == len(with_device_code) == 4, (len(objs), with_device_code)
    assert sorted(set(build.HIP_SOURCES) - set(with_device_code)) == ["ht_allgather.hip", "ht_context.hip"]
    mine = [o for o in objs if b"k_bp_project" in o]
    assert len(mine) == 1 and b"k_bp_lut" in mine[0]
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0], marker
        assert sum(1 for o in objs if marker in o) == 1, marker


def _gfx950_code_objects(lib):
    """the gfx950 entries of the library's clang offload bundles (header: magic, entry count, then offset / size / triple per entry),
    read the way benchlib/fingerprint.py reads them"""
    import struct

    from benchlib.fingerprint import MAGIC

    data, out = open(lib, "rb").read(), []
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        p = pos + len(MAGIC) + 8
        for _ in range(min(n, 16)):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen]
            p += 24 + tlen
            if b"gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 1)
    return out


def test_bin_function_is_the_camshift_units_text():
    """tests/test_oracle_golden.py proves the four-instruction cs_bin against the reference formula exhaustively.  There is exactly ONE
    definition — in ht_cs_device.h, which this unit and ht_camshift.hip include — so the proof covers every kernel that bins a pixel: no
    file of csrc/ defines cs_bin or a load-laundering macro of its own"""
    sig = "__device__ __forceinline__ uint32_t cs_bin(uint32_t px) {"
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc", ".hip", ".cc"))}
    assert sum(t.count(sig) for t in texts.values()) == 1 and texts["ht_cs_device.h"].count(sig) == 1
    m = re.search(re.escape(sig) + r"\n(.*?)\n\}\n", texts["ht_cs_device.h"], flags=re.S)
    assert m and "0x00f0f0f0u" in m.group(1)
    for f, t in texts.items():
        defs = re.findall(r"\bcs_bin\s*\([^;{)]*\)\s*\{", t)  # any definition, whatever its qualifiers
        macros = re.findall(r"#\s*define\s+(\w*_BATCH_LOADED)\b", t)
        if f == "ht_cs_device.h":
            assert len(defs) == 1 and macros == ["CS_BATCH_LOADED"], (defs, macros)
        else:
            assert not defs and not macros, (f, defs, macros)
    assert "CS_BATCH_LOADED(" in texts["ht_backproject.hip"] and "cs_bin(" in texts["ht_backproject.hip"]  # and the unit uses them


def test_new_kernels_fit_their_budgets():
    """code-object metadata: no spills, no scratch, static LDS within the 64 KB a workgroup gets by default; the streaming kernel keeps 8
    wavefronts per SIMD (<= 64 VGPRs) so that two 1024-thread workgroups fit a CU"""
    build.build_lib()
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in NEW_KERNELS:
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (k, r)
    assert res["k_bp_project<0>"]["group_segment_fixed_size"] == 16384 and res["k_bp_project<1>"]["group_segment_fixed_size"] == 32768
    assert res["k_bp_project<0>"]["vgpr_count"] <= 64 and res["k_bp_project<1>"]["vgpr_count"] <= 64


def test_pixel_loads_are_batched_before_the_first_wait():
    """the streaming kernel issues its 16-byte pixel loads as a batch (4 per thread) in front of the first `s_waitcnt vmcnt`: the
    LUT's own load(s) ride in front of the first batch.  Checked on the code object, like the camshift kernels in tests/test_abi.py."""
    build.build_lib()
    dz = _tool("disasm")
    for form, lut_loads in (("k_bp_projectILi0", 1), ("k_bp_projectILi1", 2)):
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
        assert runs[0] >= 4 + lut_loads and runs[1] >= 4, (form, runs[:4])
        assert "global_atomic" not in txt and "ds_add" not in txt and "scratch_" not in txt
        assert sum(1 for ln in txt.splitlines() if (ln.split() or [""])[0] == "s_barrier") == 1

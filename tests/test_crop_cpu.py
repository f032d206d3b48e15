"""CPU-side checks of the face crops (ht_camshift_crop_pairs_device / ht_camshift_crop_sources_device): the rule in
headtrackr_amd/csrc/ht_crop_plan.h — the lines k_crop_list compiles for the device — against the Python restatement of tests/crop_cases.py,
plain and under AddressSanitizer + UBSan, as a program of its own; the scenes the GPU tests track, proved from the oracle alone to be
insensitive to the summation order and to cover what those tests claim; the entry points at every layer; the kernel's budget and its
place in the library's code objects; the N-API shim against a recording stub; the JavaScript facade on the mock addon.  No compute
calls (no GPU here)."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crop_cases as cr
import cs_cases as cc
import draw_list_cases as dl
import ingest_cases as ic
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
NODE = shutil.which("node")
EXPORTS = ("ht_camshift_crop_pairs_device", "ht_camshift_crop_sources_device", "ht_camshift_crop_result", "ht_camshift_crop_records_device")
N_RANDOM = 100000


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("crop_plan") / ("crop_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "crop_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, False)


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, True)


@pytest.fixture(scope="module")
def cases():
    """the edge table and the seeded random objects, with the restatement's answer for each: computed once"""
    cs = cr.edge_cases() + cr.random_cases(N_RANDOM)
    return cs, np.array([cr.want_of(c) for c in cs], dtype=np.int64)


def test_edge_table_covers_what_it_claims():
    """from the restatement alone: both codes; NaN, infinities and negatives; 0 x 0; 65536 / 65537 and 2^20 / 2^20 + 1 on both sides; crops
    that touch each edge of the source; one-pixel-wide and one-pixel-high results; the three margins; square on and off changing a rect"""
    cs = cr.edge_cases()
    objs = {c[:4] for c in cs}
    assert any(o[0] != o[0] for o in objs) and any(o[2] != o[2] for o in objs) and any(o[0] == float("inf") for o in objs) and any(o[0] == float("-inf") for o in objs)
    assert any(o[2] < 0 for o in objs) and (48, 40, 0, 0) in objs and (0, 0, 0, 0) in objs
    by = {c: cr.want_of(c) for c in cs}
    pairs97 = [c for c in cs if c[4:12] == (97, 81, 97, 81, 0, 0, 97, 81) and c[12] == 256 and c[13] == 0]
    code = {c[:4]: by[c][0] for c in pairs97}
    assert code[(48, 40, 65536, 10)] == cr.FACE and code[(48, 40, 65537, 10)] == cr.EMPTY and code[(48, 40, 10, 65536.999)] == cr.FACE and code[(48, 40, 10, 65537)] == cr.EMPTY
    huge = {c[:4]: by[c][0] for c in cs if c[4] == 1 << 21 and c[8] == 0 and c[12] == 256 and c[13] == 0}  # a canvas that holds a centre at 2^20: only the bound refuses the next one
    assert huge[(2 ** 20, 40, 10, 10)] == cr.FACE == huge[(2 ** 20 + 0.5, 40, 10, 10)] == huge[(48, 2 ** 20, 10, 10)] and huge[(2 ** 20 + 1, 40, 10, 10)] == cr.EMPTY == huge[(48, 2 ** 20 + 1, 10, 10)]
    neg = {c[:4]: by[c][0] for c in cs if c[4] == 1 << 21 and c[8] == 16000 and c[12] == 256 and c[13] == 0}  # source pixels to the left of the mapping rect
    assert neg[(-2 ** 20, 40, 10, 10)] == cr.FACE == neg[(48, -2 ** 20, 10, 10)] and neg[(-2 ** 20 - 0.5, 40, 10, 10)] == cr.EMPTY == neg[(-2 ** 20 - 1, 40, 10, 10)] == neg[(48, -2 ** 20 - 1, 10, 10)]
    seen = set()
    for c in cs:
        seen |= cr.classify([(by[c][0], by[c][1:], c[6], c[7])], 8, 8)
    assert seen >= {"empty", "left", "top", "right", "bottom", "one-wide", "one-high", "up", "down"}
    assert {c[12] for c in cs} >= {64, 256, 1024} and {c[13] for c in cs} == {0, cr.SQUARE}
    assert any(by[c] != by[c[:13] + (cr.SQUARE,)] for c in cs if c[13] == 0)
    assert {(c[4:8], c[8:12]) for c in cs} >= {((97, 81, 511, 97), (7, 1, 500, 95)), ((97, 81, 333, 217), (3, 5, 326, 208)), ((97, 81, 333, 217), (0, 0, 0, 0))}


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rule_header_equals_the_restatement(harness, harness_san, cases, tmp_path, which):
    """every case of the edge table and 100 000 seeded random objects: code and rect of ht_crop_rule equal the restatement's"""
    cs, want = cases
    assert len(cs) >= N_RANDOM + 1000
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(cr.pack_cases(cs))
    r = subprocess.run([harness if which == "plain" else harness_san, src, dst], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.int32).reshape(-1, 5)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, [(cs[i], got[i].tolist(), want[i].tolist()) for i in bad[:5]]
    faces = int((want[:, 0] == cr.FACE).sum())
    assert 0.3 * len(cs) < faces < 0.9 * len(cs)  # the random objects are no monoculture


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------

def _pairs_objects():
    a, b = cr.pairs_scene()
    return [[[to for (_b, _sw, to) in calls] for calls in s.oracle_calls()] for s in (a, b)]


def test_scenes_are_insensitive_to_the_summation_order_and_cover_the_gpu_tests_claims():
    """the method of tests/test_pairs_cpu.py on the crop scenes: the oracle under the three order variants returns the same track objects,
    so the GPU tests may expect the oracle's; no object is lost; the two steps of the pairs scene differ; the crops of the scenes touch all
    four sides, hold one-pixel-wide rects, upscales and downscales; every matrix and format occurs; two entries share an allocation"""
    ref_p, ref_f = _pairs_objects(), cr.feed_objects()
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            cr.feed_objects.cache_clear()
            alt_p, alt_f = _pairs_objects(), cr.feed_objects()
        cr.feed_objects.cache_clear()
        assert [[[cr.obj_of(t) for t in tr] for tr in s] for s in alt_p] == [[[cr.obj_of(t) for t in tr] for tr in s] for s in ref_p], flag
        assert [cr.obj_of(t) for t in alt_f] == [cr.obj_of(t) for t in ref_f], flag
    W, H = cr.CANVAS
    for s in ref_p:
        for tr in s:
            assert all(t["width"] > 0 and t["height"] > 0 for t in tr)
            assert cr.obj_of(tr[0]) != cr.obj_of(tr[1])
    seen = set()
    for (P, Q) in cr.SIZES:
        for (m, fl) in cr.CONFIGS:
            seen |= cr.classify([(*cr.rule(cr.obj_of(tr[0]), W, H, W, H, None, m, fl), W, H) for s in ref_p for tr in s], P, Q)
    assert seen >= {"left", "top", "right", "bottom", "up", "down"}
    feeds = cr.feeds()
    seen = set()
    for (m, fl) in cr.CONFIGS:
        seen |= cr.classify([(*cr.rule(cr.obj_of(to), W, H, src.w, src.h, mp, m, fl), src.w, src.h) for (src, mp), to in zip(feeds, ref_f)], 70, 19)
    assert seen >= {"left", "top", "right", "bottom", "one-wide", "one-high", "up", "down"}
    assert {s.matrix for s, _ in feeds if s.fmt != dl.RGBA} == {0, 1, 2, 3} and {s.fmt for s, _ in feeds} == {dl.RGBA, yc.NV12, yc.I420}
    assert feeds[3][0].planes is feeds[1][0].planes and feeds[1][1][0] % 2 == 1 and feeds[1][1][1] % 2 == 1  # a shared allocation; an odd-origin mapping rect
    # a wide margin reaches beyond the mapping rect of entry 3, into source pixels that were never drawn
    code, (l, t, w, h) = cr.rule(cr.obj_of(ref_f[3]), W, H, 333, 217, feeds[3][1], 1024, 0)
    assert code == cr.FACE and (l < feeds[3][1][0] or t < feeds[3][1][1])
    # on the upscaled 23 x 23 feeds the tightest boxes are 2-3 source pixels
    assert cr.rule(cr.obj_of(ref_f[2]), W, H, 23, 23, None, 64, 0)[1][2] <= 3


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_at_every_layer_and_refuse_malformed_calls_without_a_device():
    """fails without the feature: the header, the library, native.py, the API, the addon's table and INTEGRATION.md all name the four
    exports; ht_crop_record is 40 bytes in C and in its ctypes and numpy mirrors; the C ABI answers all-zero arguments with a status"""
    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "typedef struct ht_crop_params" in header and "typedef struct ht_crop_record" in header and "#define HT_ABI_VERSION 2" in header
    assert "enum { HT_CROP_EMPTY = 0, HT_CROP_FACE = 1 };" in header and "enum { HT_CROP_SQUARE = 1 };" in header
    assert C.sizeof(native.CROP_RECORD) == native.CROP_RECORD_DTYPE.itemsize == 40 and C.sizeof(native.CROP_PARAMS) == 16
    assert native.CROP_RECORD.rect.offset == 8 and native.CROP_RECORD.rx.offset == 24 and native.CROP_RECORD.ry.offset == 32
    assert [native.CROP_RECORD_DTYPE.fields[k][1] for k in ("code", "stream", "x", "width", "rx", "ry")] == [0, 4, 8, 16, 24, 32]
    assert (native.HT_CROP_EMPTY, native.HT_CROP_FACE, native.HT_CROP_SQUARE) == (cr.EMPTY, cr.FACE, cr.SQUARE) == (0, 1, 1)
    assert L.ht_camshift_crop_pairs_device(None, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_crop_sources_device(None, None, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_crop_result(None, 0, None) == native.HT_ERR_INVALID
    assert L.ht_camshift_crop_records_device(None, None, None) == native.HT_ERR_INVALID
    prm, src = native.CROP_PARAMS(7, 3, 256, 0), (native.DRAW_SOURCE * 1)()
    assert L.ht_camshift_crop_sources_device(None, None, src, 1, C.byref(prm), None, 0) == native.HT_ERR_INVALID  # no context: a status, never a crash
    assert L.ht_abi_version() == 2
    for m in ("camshift_crop_pairs_device", "camshift_crop_sources_device", "camshift_crop_result"):
        assert callable(getattr(Context, m)), m
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert {"cropPairsDevice", "cropSourcesDevice", "cropResult"} <= set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    assert '{"CROP_SQUARE", HT_CROP_SQUARE}' in napi
    facade = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("this.cropPairs = ", "this.cropFeeds = ", "this.cropResult = "):
        assert m in facade, m


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _ops(txt):
    return [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]


def test_crop_kernel_fits_its_budget_and_shares_the_text_of_the_draw_kernels():
    """code-object metadata and disassembly of k_crop_list (the fused form: there is no resolve kernel): no spills, no scratch, <= 64 VGPRs
    like its siblings, the tile's 1.9 KB of LDS, one barrier, plane reads as global (not flat) loads, the descriptor and the track object
    as scalar loads.  The binary64 division of the two ratios expands to v_fma_f64, so a blanket ban on fused operations does not apply;
    instead the pixel bodies behind the barrier hold exactly k_draw_list's binary64 products, sums and roundings (nothing contracted) and no
    fused operation at all, and the two divisions are in front of it.  The kernel lives in the one code object besides the three recorded
    ones, which are byte-identical to profiles/traffic.json's build; the rule is host AND device text"""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr, dz = _tool("kernel_resources"), _tool("disasm")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    r = res["k_crop_list"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 4096, r
    assert not [k for k in res if "crop" in k and k != "k_crop_list"]  # the fused form shipped: no resolve kernel in front
    ops, ref = _ops(dz.disasm("k_crop_list")), _ops(dz.disasm("k_draw_list"))
    assert ops and ref
    assert not any(o.startswith(("scratch_", "flat_", "buffer_")) for o in ops)
    assert sum(o == "s_barrier" for o in ops) == 1 and sum(o == "s_barrier" for o in ref) == 1
    head, body, ref_body = ops[:ops.index("s_barrier")], ops[ops.index("s_barrier"):], ref[ref.index("s_barrier"):]
    for name in ("v_mul_f64", "v_add_f64"):
        assert sum(o.startswith(name) for o in body) == sum(o.startswith(name) for o in ref_body) > 0, name
    assert sum(o.startswith("v_rndne_f64") for o in body) == 3 * 4 * 4  # one rounding per channel of the 4 pixels of a thread, in each of the three bodies
    assert not any(o.startswith(("v_fma", "v_mad_f", "v_mac_f", "v_div_")) for o in body)  # (v_mad_u64_u32 / v_mad_i64_i32 are address arithmetic)
    assert sum(o.startswith("v_div_fixup_f64") for o in head) == 2  # rx and ry: one correctly rounded division each
    assert any(o.startswith("s_load_dword") for o in head) and not any(o.startswith("global_load") for o in head)  # descriptor and state: scalar loads only
    for name in ("global_load_dwordx2", "global_load_ushort", "global_load_ubyte", "global_load_dword"):
        assert sum(o == name for o in body) == sum(o == name for o in ref_body) > 0, name
    for marker in fingerprint.UNITS.values():
        assert marker.decode() not in "k_crop_list"
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_crop_list" in o]
    assert len(home) == 1 and b"k_draw_list" in home[0] and b"k_draw_frames" in home[0]
    family = ("ht_crop.hip", "ht_align.hip", "ht_patch.hip", "ht_filter.hip", "ht_face_calls.hip", "ht_list_parts.inc")  # the face-patch calls' kernels, their one host path and the text the kernels share
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_crop_plan.h", "ht_ingest_bodies.inc") + family}
    whole = "".join(text[f] for f in family)
    assert '#include "ht_crop.hip"' in text["ht_ingest.hip"] and text["ht_ingest.hip"].index('#include "ht_filter.hip"') < text["ht_ingest.hip"].index('#include "ht_face_calls.hip"')
    # the pixel bodies are ht_ingest_bodies.inc's text: the ONE format scaffold includes its three bodies, and the only other includes are the
    # taps of the two kernels with the draw list's tile
    assert text["ht_list_parts.inc"].count('#include "ht_ingest_bodies.inc"') == 3 and whole.count('#include "ht_ingest_bodies.inc"') == 3 + 2
    assert text["ht_crop.hip"].count('#include "ht_ingest_bodies.inc"') == 1 and whole.count("#define LP_PART 4  // LP_SCAFFOLD") == 3
    assert "ig_channel(" not in whole and whole.count("rs_tap(") == text["ht_filter.hip"].count("rs_tap(") == 2  # the fine patch's taps, as before
    assert whole.count("ht_crop_rule(") == 1 and "ht_crop_rule(" in text["ht_list_parts.inc"]  # the cut head, written once
    assert whole.count("#define LP_PART 1  // LP_CUT_HEAD") == 3
    # an entry's rules are asked of the draw list's plan, not restated: once, in the family's one host path
    assert whole.count("ht_draw_list_plan_entry(") == 1 and "ht_draw_list_plan_entry(" in text["ht_face_calls.hip"]
    assert "hip/" not in text["ht_crop_plan.h"] and "__global__" not in text["ht_crop_plan.h"] and "ht_csb_floor_i32(" in text["ht_crop_plan.h"]
    assert "double" not in text["ht_crop_plan.h"].split("HT_CROP_FN int32_t ht_crop_rule(")[1].split(") {", 1)[1]  # integer-only behind the four floors


# ---- the N-API shim against the recording stub --------------------------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_arguments_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with tests/js/abi_stub.cc and tests/js/crop_stub.cc: the successful calls of tests/js/crop_addon.js reach the C
    ABI with the pairs, the streams, the entries' plane layout, the params, the output offset and stride; cropResult unpacks the 40-byte
    records; every malformed call throws before the C ABI is reached, and a refusal of the library comes back as an Error"""
    addon = str(tmp_path / "addon_crop.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), os.path.join(ROOT, "tests", "js", "abi_stub.cc"),
                           os.path.join(ROOT, "tests", "js", "crop_stub.cc"), "-o", addon])
    log = str(tmp_path / "crop.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "crop_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_CROP_STUB_LOG=log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["consts"] == [0, 1, 1, "function", "function", "function"]
    calls = [json.loads(ln) for ln in open(log)]
    pb = 7 * 3 * 4
    whole = [0, 0, 0, 0]
    E_RGBA = dict(p1=None, p2=None, size=[7, 5], format=16, matrix=0, rect=whole)
    E_NV12 = dict(p1=23 * 23, p2=None, size=[23, 23], format=0, matrix=1, rect=[1, 1, 21, 21])
    E_I420 = dict(p1=97 * 81, p2=97 * 81 + 49 * 41, size=[97, 81], format=1, matrix=3, rect=whole)
    assert calls[0] == dict(fn="pairs", ctx=True, n=4, out=1, pairs=[[5, 0], [0, 0], [2, 1], [2, 1]], params=[7, 3, 256, 0], stride=0)
    assert calls[1] == dict(fn="pairs", ctx=True, n=2, out=1, pairs=[[5, 0], [0, 0]], params=[7, 3, 1024, 1], stride=pb + 16)
    assert calls[2] == dict(fn="sources", ctx=True, n=2, streams=[3, 3], entries=[dict(E_RGBA, p0=50000), dict(E_NV12, p0=51001)], params=[7, 3, 256, 0], stride=0)
    # the output 12 bytes into the buffer: the planes are logged relative to it
    assert calls[3] == dict(fn="sources", ctx=True, n=4, streams=[1, 0, 7, 7], params=[7, 3, 1024, 1], stride=pb + 4,
                            entries=[dict(E_I420, p0=54000 - 12), dict(E_NV12, p0=51001 - 12), dict(E_RGBA, p0=50000 - 12), dict(E_RGBA, p0=50000 - 12)])
    res = out["result"]
    assert res["kinds"] == ["Int32Array", "Float64Array"]
    assert res["records"] == [v for i in range(4) for v in (i & 1, 10 + i, i, 2 * i, 3 * i + 1, 4 * i + 1)]
    assert res["ratios"] == [v for i in range(4) for v in (i + 0.25, 1.0 / (i + 3))]
    thrown = dict(out["thrown"])
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    refused = {k: thrown.pop(k) for k in list(thrown) if k.endswith("the library refuses")}
    assert len(calls) == 6 and calls[4]["n"] == 3 and calls[5]["n"] == 3  # the only two further calls that reach the C ABI: the stub refuses n == 3
    assert "ht_camshift_crop_pairs_device: status -1" in refused["pairs: the library refuses"] and "ht_camshift_crop_sources_device: status -1" in refused["sources: the library refuses"]
    assert "ht_camshift_crop_result: status -6" in refused["result: the library refuses"]
    kinds = {"pairs: too few arguments": "TypeError", "pairs: no context": "TypeError", "pairs: a plain array": "TypeError", "pairs: odd length": "TypeError",
             "pairs: none": "TypeError", "pairs: 65536": "RangeError", "pairs: params of three": "TypeError", "pairs: params of five": "TypeError",
             "pairs: params a Float64Array": "TypeError", "pairs: width 0": "RangeError", "pairs: height 1025": "RangeError", "pairs: out null": "TypeError",
             "pairs: out a context": "TypeError", "pairs: stride a string": "TypeError", "pairs: negative offset": "TypeError", "pairs: output too small": "RangeError",
             "pairs: output offset beyond": "RangeError", "pairs: output stride beyond": "RangeError",
             "sources: too few arguments": "TypeError", "sources: streams a plain array": "TypeError", "sources: entries no array": "TypeError",
             "sources: no entries": "RangeError", "sources: one stream for two entries": "RangeError", "sources: entry no object": "TypeError",
             "sources: entry without dev": "TypeError", "sources: frame beyond its buffer": "RangeError", "sources: rect a plain array": "TypeError",
             "sources: width 1025": "RangeError", "sources: output too small": "RangeError", "sources: out null": "TypeError",
             "result: too few arguments": "TypeError", "result: n 0": "TypeError", "result: n a string": "TypeError"}
    assert set(thrown) == set(kinds)
    for what, kind in kinds.items():
        assert thrown[what].startswith(kind + ": "), (what, thrown[what])


# ---- the JavaScript facade on the mock addon ----------------------------------------------------------------------------------------------------

JS_CONFIGS = [dict(width=70, height=19, margin=1.0, square=False), dict(width=1, height=1, margin=0.25, square=True), dict(width=24, height=24, margin=4.0, square=True),
              dict(width=24, height=24, margin=4.0, square=False)]


def _expect(entries, cfg):
    """entries: [(source, track object or None, mapping, stream)] -> (crcs, records, ratios) of one crop call"""
    W, H = cr.CANVAS
    m, fl, P, Q = int(round(cfg["margin"] * 256)), int(cfg["square"]), cfg["width"], cfg["height"]
    crcs, recs, ratios = [], [], []
    for src, to, mapping, stream in entries:
        obj = cr.obj_of(to) if to else (0.0, 0.0, 0.0, 0.0)
        crcs.append(ic.crc(cr.patch(src, obj, W, H, mapping, m, fl, P, Q)))
        code, rect = cr.rule(obj, W, H, src.w, src.h, mapping, m, fl)
        recs += [code, stream, *rect]
        ratios += [rect[2] / P, rect[3] / Q] if code == cr.FACE else [0.0, 0.0]
    return crcs, recs, ratios


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_crops_pairs_and_feeds_through_the_crop_entry_points(tmp_path):
    """tests/js/crop_cpu.js on tests/js/mock_addon_crop.js: cropPairs behind an enqueue-only track step and cropFeeds on mixed
    opts.sources give the patches (CRC-32), records and ratios of the numpy / oracle expectation, through the crop entry points alone;
    malformed calls throw"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    W, H = cr.CANVAS
    a, b = cr.pairs_scene()
    seqs, trackers = (a, b), cr.pairs_trackers()
    np.stack([a.frames[0], b.frames[0]]).tofile(tmp_path / "init.raw")
    np.stack([a.frames[1], b.frames[1]]).tofile(tmp_path / "step.raw")
    init_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)] + [cr.NEVER_TRACKED, 1]
    rects = [v for (_s, _f, q, j) in trackers for v in seqs[q].rects[j]] + list(b.rects[0])
    track_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)]
    crop_list = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]  # a stream that was never tracked, one never initialised, one twice
    objs = {s: seqs[q].oracle_calls(j)[0][2] for (s, _f, q, j) in trackers}
    frame_src = []
    for q in (0, 1):
        s = dl.Source(dl.RGBA, W, H, seed=1)
        s.rgba = seqs[q].frames[1]
        frame_src.append(s)
    job = dict(w=W, h=H, configs=JS_CONFIGS,
               pairs=dict(init=str(tmp_path / "init.raw"), step=str(tmp_path / "step.raw"), trackers=cr.RESERVED, init_pairs=init_pairs, rects=[int(v) for v in rects],
                          track_pairs=track_pairs, crop_pairs=[v for p in crop_list for v in p]))
    feeds, fobjs = cr.feeds(), cr.feed_objects()
    streams = [4, 0, 6, 2, 8, 1, 5]
    flist = []
    for k, (src, m) in enumerate(feeds):
        fn = tmp_path / f"feed{k}.raw"
        src.packed().tofile(fn)
        flist.append(dict(file=str(fn), width=src.w, height=src.h, format=dl.FORMAT_NAMES[src.fmt], matrix=yc.MATRIX_NAMES[src.matrix], rect=list(m) if m else None,
                          init=list(cr.canvas_rect_of(k))))
    job["feeds"] = dict(list=flist, streams=streams, trackers=9)
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "crop_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert len(out["pairs"]) == len(out["feeds"]) == len(JS_CONFIGS)
    for cfg, gp, gf in zip(JS_CONFIGS, out["pairs"], out["feeds"]):
        crcs, recs, ratios = _expect([(frame_src[f], objs.get(s), None, s) for (s, f) in crop_list], cfg)
        assert (gp["crc"], gp["records"], gp["ratios"]) == (crcs, recs, ratios), (cfg, gp)
        assert gp["n"] == len(crop_list) and gp["size"] == [cfg["width"], cfg["height"]] and gp["bytes"] == len(crop_list) * cfg["width"] * cfg["height"] * 4
        crcs, recs, ratios = _expect([(src, to, m, st) for (src, m), to, st in zip(feeds, fobjs, streams)], cfg)
        assert (gf["crc"], gf["records"], gf["ratios"]) == (crcs, recs, ratios), (cfg, gf)
    # the enqueue-only track step was collected AFTER the crops and is the oracle's
    got = np.array(out["track"]).reshape(-1, 9)
    for row, (s, _f, _q, _j) in zip(got, trackers):
        assert tuple(row[:4]) == cr.obj_of(objs[s])
    assert out["refusals"] == 14 + 5

"""CPU-side checks of ht_draw_list_device (one launch draws a list of per-feed sources): the host-only plan in
headtrackr_amd/csrc/ht_draw_list_plan.h against a Python restatement — descriptors, ratios bit for bit, plane extents, every refusal with
the entry's index — plain and under AddressSanitizer + UBSan, as a program of its own; the entry point at every layer; the malformed calls
the C ABI refuses without a device; the kernel's budget and its place in the library's code objects.  No compute calls (no GPU here)."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import pytest

import draw_list_cases as dl
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
W, H = 97, 81
(OK, BAD_COUNT, BAD_CANVAS, BAD_FORMAT, BAD_SIZE, BAD_MATRIX, BAD_PITCH0, BAD_PITCH1, NULL_PLANE, MISALIGNED, BAD_RECT) = range(11)


def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("draw_list_plan") / ("draw_list_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "draw_list_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, False)


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, True)


def entry(fmt, w, h, p=(0x10000, 0x90000, 0xA0000), pitch=(0, 0), matrix=0, rect=(0, 0, 0, 0), count=1):
    return dict(fmt=fmt, w=w, h=h, p=p, pitch=pitch, matrix=matrix, rect=rect, count=count)


def call_text(entries, n=None, w=W, h=H, null=False, dst=None):
    total = sum(e["count"] for e in entries)
    lines = [f"call {w} {h} {total if n is None else n}"]
    for e in entries:
        lines.append("entry %d %d %d %d %d %d %d %d %d %d %d %d %d %d" % (e["count"], *e["p"], *e["pitch"], e["w"], e["h"], e["fmt"], e["matrix"], *e["rect"]))
    if null:
        lines.append("null")
    if dst:
        lines.append("dst %d %d" % dst)
    return "\n".join(lines + ["end"]) + "\n"


def run(exe, tmp_path, calls):
    path = str(tmp_path / "calls.txt")
    with open(path, "w") as f:
        f.write("".join(calls))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(calls)
    return out


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def want_desc(e, w=W, h=H):
    """the Python restatement of one descriptor and of its extents"""
    fmt, sw, sh = e["fmt"], e["w"], e["h"]
    rect = e["rect"] if (e["rect"][2] or e["rect"][3]) else (0, 0, sw, sh)
    if fmt == dl.RGBA:
        pitch0 = e["pitch"][0] or 4 * sw
        d = dict(p=[e["p"][0], 0, 0], pitch=[pitch0, 0], cw=0, kc=[0] * 6)
        ext = [[e["p"][0], (sh - 1) * pitch0 + 4 * sw], [0, 0], [0, 0]]
    else:
        cw, ch = yc.chroma_dims(sw, sh)
        crow = 2 * cw if fmt == yc.NV12 else cw
        pitch0, pitch1 = e["pitch"][0] or sw, e["pitch"][1] or crow
        d = dict(p=[e["p"][0], e["p"][1], e["p"][1] if fmt == yc.NV12 else e["p"][2]], pitch=[pitch0, pitch1], cw=cw, kc=list(yc.TABLE[e["matrix"]]))
        cext = (ch - 1) * pitch1 + crow
        ext = [[e["p"][0], (sh - 1) * pitch0 + sw], [e["p"][1], cext], [e["p"][2], cext] if fmt == yc.I420 else [0, 0]]
    d.update(rect=list(rect), format=fmt, rx=bits(rect[2] / w), ry=bits(rect[3] / h))  # Python's / is one binary64 division
    return d, ext


MIXED = [
    entry(dl.RGBA, 333, 217, pitch=(1344, 0), matrix=9),                         # the matrix of an RGBA entry is not looked at
    entry(yc.NV12, 333, 217, pitch=(346, 340), matrix=1),
    entry(yc.I420, 2, 2, pitch=(5, 6), matrix=2),
    entry(yc.NV12, 23, 23, matrix=3, p=(0x10001, 0x90002, 0)),                   # odd x odd; the Y plane needs no alignment
    entry(dl.RGBA, 1, 5, pitch=(12, 0), p=(0x20004, 0, 0)),
    entry(yc.I420, 333, 217, rect=(3, 5, 326, 208), p=(0x10003, 0x90001, 0xA0007)),  # I420 planes need no alignment
    entry(yc.NV12, 23, 23, rect=(1, 1, 21, 21), matrix=2),
    entry(yc.I420, 16384, 16384, pitch=(1 << 20, 1 << 19), rect=(16383, 16383, 1, 1)),
    entry(dl.RGBA, 7, 3, rect=(0, 0, 0, 0)), entry(dl.RGBA, 7, 3, rect=(5, 9, 0, 0)),  # width == height == 0: the whole source, x / y not looked at
]
BAD_ENTRIES = [
    (entry(2, 8, 8), BAD_FORMAT), (entry(-1, 8, 8), BAD_FORMAT), (entry(15, 8, 8), BAD_FORMAT), (entry(17, 8, 8), BAD_FORMAT),
    (entry(dl.RGBA, 0, 8), BAD_SIZE), (entry(dl.RGBA, 8, 16385), BAD_SIZE), (entry(yc.NV12, -3, 8), BAD_SIZE), (entry(yc.I420, 16385, 8), BAD_SIZE),
    (entry(yc.NV12, 8, 8, matrix=4), BAD_MATRIX), (entry(yc.I420, 8, 8, matrix=-1), BAD_MATRIX),
    (entry(dl.RGBA, 8, 8, pitch=(28, 0)), BAD_PITCH0), (entry(dl.RGBA, 8, 8, pitch=(34, 0)), BAD_PITCH0), (entry(dl.RGBA, 8, 8, pitch=((1 << 32) + 4, 0)), BAD_PITCH0),
    (entry(yc.NV12, 9, 8, pitch=(8, 0)), BAD_PITCH0),
    (entry(yc.NV12, 9, 8, pitch=(0, 8)), BAD_PITCH1), (entry(yc.NV12, 9, 8, pitch=(0, 11)), BAD_PITCH1), (entry(yc.I420, 9, 8, pitch=(0, 4)), BAD_PITCH1),
    (entry(dl.RGBA, 8, 8, p=(0, 0, 0)), NULL_PLANE), (entry(yc.NV12, 8, 8, p=(0x100, 0, 0)), NULL_PLANE), (entry(yc.NV12, 8, 8, p=(0, 0x100, 0)), NULL_PLANE),
    (entry(yc.I420, 8, 8, p=(0x100, 0x200, 0)), NULL_PLANE),
    (entry(dl.RGBA, 8, 8, p=(0x102, 0, 0)), MISALIGNED), (entry(yc.NV12, 8, 8, p=(0x100, 0x201, 0)), MISALIGNED),
    (entry(dl.RGBA, 8, 8, rect=(1, 0, 8, 8)), BAD_RECT), (entry(yc.NV12, 8, 8, rect=(0, 1, 8, 8)), BAD_RECT), (entry(yc.I420, 8, 8, rect=(-1, 0, 4, 4)), BAD_RECT),
    (entry(dl.RGBA, 8, 8, rect=(0, 0, 0, 5)), BAD_RECT), (entry(dl.RGBA, 8, 8, rect=(0, 0, 5, -1)), BAD_RECT), (entry(yc.NV12, 8, 8, rect=(8, 0, 1, 1)), BAD_RECT),
]


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_plan_descriptors_extents_and_every_refusal(harness, harness_san, tmp_path, which):
    exe = harness if which == "plain" else harness_san
    assert {e["fmt"] for e in MIXED} == {dl.RGBA, yc.NV12, yc.I420}
    good = entry(yc.NV12, 23, 23)
    calls = [call_text(MIXED)]
    # overlap probes on the mixed list: [address, bytes] -> the first entry with a plane inside, or -1
    nv = MIXED[1]
    y_end, c_end = nv["p"][0] + 216 * 346 + 333, nv["p"][1] + 108 * 340 + 334
    probes = [((0x8000, 0x8000), -1), ((0x8000, 0x8001), 0), ((y_end, 64), 0),  # (entry 0's RGBA plane at the same base is longer)
              ((c_end, 1 << 20), 2), ((c_end - 1, 1), 1), ((0xA0000, 1), 2), ((0xA0007 + 108 * 167 + 167, 4), 7), ((0x90000 + (16383 << 19) + 8191, 1), 7), ((1 << 40, 1 << 20), -1)]
    calls += [call_text(MIXED, dst=p) for p, _ in probes]
    # every refusal at entry 5 of 7, and at entry 0 of 1
    for e, _ in BAD_ENTRIES:
        calls.append(call_text([dict(good, count=5), e, good]))
        calls.append(call_text([e]))
    # the count: none, negative, above 65535, no list; 65535 itself is drawn; a canvas without a size
    calls += [call_text([], n=0), call_text([], n=-1), call_text([], n=65536), call_text([good], n=1, null=True), call_text([dict(good, count=65535)]),
              call_text([good], w=0), call_text([good], h=-1)]
    out = run(exe, tmp_path, calls)
    g = out[0]
    assert g["status"] == OK and g["bad"] == -1 and len(g["desc"]) == len(MIXED)
    for i, e in enumerate(MIXED):
        d, ext = want_desc(e)
        assert g["desc"][i] == d, (i, g["desc"][i], d)
        assert g["ext"][i] == ext, (i, g["ext"][i], ext)
    for (p, want), g in zip(probes, out[1:1 + len(probes)]):
        assert g["status"] == OK and g["overlap"] == want, (p, g.get("overlap"), want)
    k = 1 + len(probes)
    seen = set()
    for e, status in BAD_ENTRIES:
        for g, index in ((out[k], 5), (out[k + 1], 0)):
            assert g["status"] == status and g["bad"] == index and set(g) == {"status", "message", "bad"} and len(g["message"]) > 8, (e, g)
        seen.add(status)
        k += 2
    assert seen == set(range(BAD_FORMAT, BAD_RECT + 1))  # every per-entry refusal the plan knows
    for g in out[k:k + 4]:
        assert g["status"] == BAD_COUNT and g["bad"] == -1, g
    g = out[k + 4]
    assert g["status"] == OK and len(g["desc"]) == 2 and g["desc"][0] == g["desc"][1] == want_desc(good)[0]
    assert [g["status"] for g in out[k + 5:]] == [BAD_CANVAS, BAD_CANVAS]


def test_restated_extents_are_those_of_the_test_sources():
    """the extents of the restatement above are the sizes of the buffers the GPU tests allocate (a plane ends with its last row)"""
    for s, _ in dl.mixed_sources():
        p0, p1 = s.pitches()
        _, ext = want_desc(entry(s.fmt, s.w, s.h, pitch=(p0, p1), matrix=s.matrix))
        assert [b for _, b in ext if b] == dl.extent_of(s) == [len(b) for b in s.plane_buffers()]


def test_entry_point_exists_at_every_layer_and_refuses_malformed_calls_without_a_device():
    """fails without the feature: the library, the header, native.py, the API, the addon and INTEGRATION.md all name the export; the C ABI
    answers all-zero arguments with a status; the YUV entry points go on refusing the RGBA format number"""
    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    name = "ht_draw_list_device"
    assert re.search(r"\b%s\s*\(" % name, header) and "typedef struct ht_draw_source" in header and "#define HT_ABI_VERSION 2" in header
    assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):]
    # the ctypes struct mirrors the C one: three pointers, two size_t, four int32, the rect
    assert C.sizeof(native.DRAW_SOURCE) == 72 and native.DRAW_SOURCE.width.offset == 40 and native.DRAW_SOURCE.rect.offset == 56
    assert native.HT_DRAW_RGBA == dl.RGBA == 16 and native.DRAW_FORMATS == {"nv12": 0, "i420": 1, "rgba": 16}
    assert L.ht_draw_list_device(None, None, 0, None, 0) == native.HT_ERR_INVALID
    src = (native.DRAW_SOURCE * 1)()
    assert L.ht_draw_list_device(None, src, 1, None, 0) == native.HT_ERR_INVALID  # no context: a status, never a crash
    assert L.ht_abi_version() == 2 and callable(Context.draw_list)
    assert yc.NV12 in (0, 1) and yc.I420 in (0, 1) and native.HT_DRAW_RGBA not in (0, 1)  # outside the range tests/test_ingest_yuv_cpu.py pins as valid
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert "drawListDevice" in set(re.findall(r'\{"(\w+)",\s*\w+\}', napi)) and '{"DRAW_RGBA", HT_DRAW_RGBA}' in napi


def test_list_kernel_fits_its_budget_and_shares_the_text_of_the_draw_kernels():
    """code-object metadata and disassembly of k_draw_list: no spills, no scratch, <= 64 VGPRs (8 wavefronts per SIMD like the single-source
    kernels), the tile's 1.9 KB of LDS, one barrier, no contracted binary64 product, plane reads as global (not flat) loads and the
    descriptor as scalar loads; it lives in the one code object besides the three recorded ones, which are byte-identical to
    profiles/traffic.json's build; the tile's text exists once, in ht_ingest_bodies.inc, and every draw kernel compiles it"""
    import importlib.util

    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    def tool(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    build.build_lib()
    kr, dz = tool("kernel_resources"), tool("disasm")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    r = res["k_draw_list"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 4096, r
    txt = dz.disasm("k_draw_list")
    assert txt
    ops = [(ln.split() or [""])[0] for ln in txt.splitlines()[1:]]
    assert not any(o.startswith(("v_fma", "scratch_", "flat_")) for o in ops)
    assert sum(o == "s_barrier" for o in ops) == 1 and any(o.startswith("s_load_dword") for o in ops)
    assert any(o == "global_load_dwordx2" for o in ops) and any(o == "global_load_ushort" for o in ops)
    for marker in fingerprint.UNITS.values():
        assert marker.decode() not in "k_draw_list"
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_draw_list" in o]
    assert len(home) == 1 and b"k_draw_frames" in home[0] and b"k_draw_yuv" in home[0]
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_ingest_yuv.hip", "ht_draw_list.hip", "ht_draw_calls.hip", "ht_ingest_bodies.inc", "ht_draw_list_plan.h")}
    assert '#include "ht_draw_list.hip"' in text["ht_ingest.hip"]
    assert [text[f].count('#include "ht_ingest_bodies.inc"') for f in ("ht_ingest.hip", "ht_ingest_yuv.hip", "ht_draw_list.hip", "ht_draw_calls.hip")] == [2, 2, 4, 0]  # (the calls' host path holds no kernel)
    assert text["ht_ingest_bodies.inc"].count("ig_channel(") == 2 and text["ht_ingest_bodies.inc"].count("rs_tap(") == 2  # one per pixel body; column and row taps
    for f in ("ht_ingest.hip", "ht_ingest_yuv.hip", "ht_draw_list.hip", "ht_draw_calls.hip"):
        assert "rs_tap(" not in text[f], f
    assert "hip/" not in text["ht_draw_list_plan.h"] and "__global__" not in text["ht_draw_list_plan.h"] and "ht_yuv_plan(" in text["ht_draw_list_plan.h"]


# ---- the JavaScript layer on the mock addon ---------------------------------------------------------------------------------------------------

NODE = __import__("shutil").which("node")


def js_feeds():
    """(source, rect): all three formats, an odd x odd NV12 frame (one byte into its buffer), odd-origin rects, a one-pixel-wide source"""
    return [(dl.Source(dl.RGBA, 64, 48, seed=81, content="smooth"), (3, 5, 50, 40)), (dl.Source(yc.NV12, 23, 23, seed=82, matrix=1), None),
            (dl.Source(yc.I420, 97, 81, seed=83, matrix=2, content="raw"), (1, 1, 95, 79)), (dl.Source(yc.NV12, 96, 81, seed=84, matrix=3), (5, 3, 2, 2)),
            (dl.Source(dl.RGBA, 1, 5, seed=85), None), (dl.Source(yc.I420, 2, 2, seed=86, content="raw"), None)]


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_draws_mixed_feeds_through_the_list_entry_point(tmp_path):
    """tests/js/draw_list_cpu.js on tests/js/mock_addon_draw_list.js: ccv.DeviceBatch with mixed opts.sources — drawList into a frame set and
    drawListBound give the numpy / oracle canvases, through drawListDevice alone; malformed opts.sources and rects throw; an RGBA
    opts.source batch still logs the old entry point"""
    import ingest_cases as ic

    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    dw, dh = 40, 30
    feeds, job = js_feeds(), {"w": dw, "h": dh, "feeds": []}
    for k, (s, rect) in enumerate(feeds):
        fn = tmp_path / f"feed{k}.raw"
        s.packed().tofile(fn)
        job["feeds"].append(dict(file=str(fn), width=s.w, height=s.h, format=dl.FORMAT_NAMES[s.fmt], matrix=yc.MATRIX_NAMES[s.matrix], rect=list(rect) if rect else None))
    rgba = ic.noise(64, 48, 3)
    rgba.tofile(tmp_path / "rgba.raw")
    job["rgba"] = dict(file=str(tmp_path / "rgba.raw"), w=64, h=48)
    (tmp_path / "job.json").write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "draw_list_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    want = [ic.crc(s.expected(rect, dw, dh)) for s, rect in feeds]
    assert out["list_crc"] == want and out["bound_crc"] == want
    assert out["list_checks"] == 6 and out["rgba_checks"] == 1 and out["refusals"] == 2 * 9 + 9 + 1


# ---- the N-API shim itself, linked against the recording C-ABI stub ---------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_entries_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with tests/js/abi_stub.cc and tests/js/draw_list_stub.cc (a recording ht_draw_list_device): the successful calls
    of tests/js/draw_list_addon.js reach the C ABI with the plane layout of a packed frame (p1 = p0 + w h; I420: p2 = p1 + cw ch; NULL
    where the format has no plane), offsets, rects, the destination offset and stride; every malformed call throws before the C ABI is
    reached, and a refusal of the library comes back with its message"""
    addon = str(tmp_path / "addon_dl.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), os.path.join(ROOT, "tests", "js", "abi_stub.cc"),
                           os.path.join(ROOT, "tests", "js", "draw_list_stub.cc"), "-o", addon])
    log = str(tmp_path / "dl.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "draw_list_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_DL_STUB_LOG=log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["consts"] == [16, 0, 1, "function"]
    calls = [json.loads(ln) for ln in open(log)]
    fb = 40 * 30 * 4
    whole = [0, 0, 0, 0]
    E_RGBA = dict(p0=0, p1=None, p2=None, pitch=[0, 0], size=[7, 5], format=16, matrix=0, rect=whole)
    E_NV12 = dict(p1=23 * 23, p2=None, pitch=[0, 0], size=[23, 23], format=0, matrix=1, rect=[1, 1, 21, 21])
    E_I420 = dict(p1=97 * 81, p2=97 * 81 + 49 * 41, pitch=[0, 0], size=[97, 81], format=1, matrix=3, rect=whole)
    E_TAIL = dict(p0=100000 - 6, p1=4, p2=5, pitch=[0, 0], size=[2, 2], format=1, matrix=0, rect=whole)
    assert calls[0]["n"] == 4 and calls[0]["dst_stride"] == 0 and calls[0]["ctx"] is True
    assert calls[0]["entries"] == [E_RGBA, dict(E_NV12, p0=1001), dict(E_I420, p0=4000), E_TAIL]
    dst0 = calls[0]["dst"]  # the destination buffer relative to the source buffer: the second call's is 4 bytes further, from another entry 0
    assert calls[1]["n"] == 2 and calls[1]["dst_stride"] == fb + 48 and calls[1]["dst"] == dst0 + 4 - 1001
    assert calls[1]["entries"] == [dict(E_NV12, p0=0), dict(E_RGBA, p0=-1001)]
    assert calls[2]["n"] == 1 and calls[2]["dst"] is None and calls[2]["entries"] == [dict(E_I420, p0=0)]
    thrown = dict(out["thrown"])
    assert thrown.pop("an empty rect is not the whole source") is None  # (the stub accepts it: what matters is the rect that arrived, below)
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    # the two calls that DO reach the C ABI: the stub refuses n == 3, and the empty rect arrives as a rect the library refuses (width -1)
    assert len(calls) == 5 and calls[3]["n"] == 3 and "status -1" in thrown["the library refuses"] and "ht_draw_list_device" in thrown["the library refuses"]
    assert calls[4]["n"] == 2 and calls[4]["entries"][0]["rect"] == [0, 0, -1, 0] and calls[4]["entries"][1]["rect"] == whole
    del thrown["the library refuses"]
    kinds = {"too few arguments": "TypeError", "no context": "TypeError", "entries no array": "TypeError", "no entries": "RangeError", "65536 entries": "RangeError",
             "entry no object": "TypeError", "entry without dev": "TypeError", "entry.dev a context": "TypeError", "width a string": "TypeError", "no format": "TypeError",
             "negative offset": "TypeError", "rect of three": "TypeError", "rect a plain array": "TypeError", "frame beyond its buffer": "RangeError",
             "RGBA frame beyond its buffer": "RangeError", "zero width": "RangeError", "destination too small": "RangeError", "destination offset beyond": "RangeError",
             "destination stride beyond": "RangeError", "dst a context": "TypeError", "stride a string": "TypeError"}
    assert set(thrown) == set(kinds)
    for what, kind in kinds.items():
        assert thrown[what].startswith(kind + ": "), (what, thrown[what])

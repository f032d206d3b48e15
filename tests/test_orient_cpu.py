"""The oriented ingest (rotated and mirrored feeds: orientation 0..7 in bits 8..10 of a source's format) without a device: the rule against
numpy, the plan header (csrc/ht_orient_plan.h) in a stand-alone program, plain and under AddressSanitizer + UBSan, the module's code object
(libheadtrackr_hip_orient.hsaco: its notes, its registers, its place outside the library), the text of its blend against ig_channel's, and
the orientation helpers of the Python layer.  On the parent commit there is no header, no module and no helper: every test here fails."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import draw_list_cases as dl
import orient_cases as oc
import yuv422_cases as y4
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import api, build

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
OK = 0
L_BAD_FORMAT, L_BAD_SIZE, L_BAD_MATRIX, L_BAD_PITCH0, L_BAD_PITCH1, L_NULL_PLANE, L_MISALIGNED, L_BAD_RECT = range(3, 11)
BIG = 16384


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", oc.MAPPING_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mapping_formula_is_rot90_then_fliplr(size):
    """O(x, y) = S(u, v) by the header's table equals np.rot90(S, -rot) then np.fliplr, for all eight k, on a frame whose every pixel is
    its own index"""
    w, h = size
    stored = np.arange(w * h, dtype=np.int64).reshape(h, w)
    for k in oc.ORIENTATIONS:
        want = oc.orient(stored, k)
        ow, oh = oc.oriented_size(k, w, h)
        assert want.shape == (oh, ow)
        y, x = np.mgrid[0:oh, 0:ow]
        u, v = oc.mapping(k, w, h, x, y)
        assert u.min() >= 0 and u.max() < w and v.min() >= 0 and v.max() < h
        assert np.array_equal(stored[v, u], want), k


def _exif_by_numpy(n, img):
    """the upright image of a stored image with EXIF orientation n, from the tag's definition (row 0 / column 0 of the STORED image is the
    visual top | bottom / left | right side for 1..4, and the visual left | right / top | bottom for 5..8), in numpy's flips and transposes"""
    return {1: img, 2: np.fliplr(img), 3: np.flipud(np.fliplr(img)), 4: np.flipud(img), 5: np.swapaxes(img, 0, 1), 6: np.fliplr(np.swapaxes(img, 0, 1)),
            7: np.flipud(np.fliplr(np.swapaxes(img, 0, 1))), 8: np.flipud(np.swapaxes(img, 0, 1))}[n]


def test_exif_and_rotation_helpers_against_numpy():
    img = np.arange(5 * 7 * 4, dtype=np.uint8).reshape(5, 7, 4)
    table = {}
    for n in range(1, 9):
        k = api.orientation_from_exif(n)
        assert np.array_equal(oc.orient(img, k), _exif_by_numpy(n, img)), n
        table[n] = k
    assert table == oc.EXIF and sorted(table.values()) == list(range(8))
    for deg in (-270, -180, -90, 0, 90, 180, 270, 360, 450):
        for mirror in (False, True):
            k = api.orientation_from_rotation(deg, mirror)
            want = np.rot90(img, -(deg // 90))  # rot90 turns counter-clockwise: `deg` clockwise is -deg / 90 of its turns
            assert np.array_equal(oc.orient(img, k), np.fliplr(want) if mirror else want), (deg, mirror)
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            api.orientation_from_exif(bad)
    for bad in (45, 91, 0.5):
        with pytest.raises(ValueError):
            api.orientation_from_rotation(bad)
    assert [api.orientation_bits(k) for k in range(8)] == [k << 8 for k in range(8)]
    for bad in (-1, 8, 1.5, 256):
        with pytest.raises(ValueError):
            api.orientation_bits(bad)


# ---- the plan header -----------------------------------------------------------------------------------------------------------------------

def _build(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("orient_plan") / ("orient_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "orient_plan_harness.cc"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    """the stand-alone program, plain and with AddressSanitizer + UBSan linked in (run directly)"""
    return _build(tmp_path_factory, request.param == "sanitized")


def _run(exe, mode, tmp_path, cases):
    path = str(tmp_path / (mode + ".txt"))
    with open(path, "w") as f:
        f.write("\n".join(" ".join(str(int(v)) for v in c) for c in cases) + "\n")
    r = subprocess.run([exe, mode, path], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(cases)
    return out


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


P0, P1, P2 = 0x10000, 0x50000, 0x90000


def entry(fmt, k, w, h, W, H, p0=P0, p1=P1, p2=P2, pitch0=0, pitch1=0, matrix=0, rect=(0, 0, 0, 0), raw=None):
    return (p0, p1, p2, pitch0, pitch1, w, h, oc.fmt_code(fmt, k) if raw is None else raw, matrix, *rect, W, H)


def want_entry(c):
    """numpy-free restatement of what ht_orient_plan_entry writes for a legal entry"""
    p0, p1, p2, pitch0, pitch1, w, h, code, matrix, rx, ry, rw, rh, W, H = c
    fmt, k = code & 0xff, code >> 8
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == dl.RGBA:
        p, pitch, cwd, kc = [p0, 0, 0], [pitch0 or 4 * w, 0], 0, [0] * 6
        base, nbytes = [p0, 0, 0], [pitch[0] * (h - 1) + 4 * w, 0, 0]
    elif fmt in (y4.YUYV, y4.UYVY):
        p, pitch, cwd, kc = [p0, 0, 0], [pitch0 or 4 * cw, 0], cw, list(yc.TABLE[matrix])
        base, nbytes = [p0, 0, 0], [pitch[0] * (h - 1) + 4 * cw, 0, 0]
    else:
        nv12 = fmt == yc.NV12
        crow = 2 * cw if nv12 else cw
        p, pitch, cwd, kc = [p0, p1, p1 if nv12 else p2], [pitch0 or w, pitch1 or crow], cw, list(yc.TABLE[matrix])
        cbytes = pitch[1] * (ch - 1) + crow
        base, nbytes = [p0, p1, 0 if nv12 else p2], [pitch[0] * (h - 1) + w, cbytes, 0 if nv12 else cbytes]
    ow, oh = oc.oriented_size(k, w, h)
    rect = [rx, ry, rw, rh] if rw or rh else [0, 0, ow, oh]
    return dict(status=0, p=p, pitch=pitch, stored=[0, 0, w, h], cw=cwd, format=fmt, ratio_bits=[_bits(rect[2] / W), _bits(rect[3] / H)], kc=kc, orient=k, frame=0, rect=rect,
                base=base, bytes=nbytes, size=[ow, oh], present=k != 0)


def test_descriptors_sizes_and_extents_for_every_format_and_orientation(harness, tmp_path):
    """every format x k on 37 x 23 (whole, and under a rect of O that touches O's far corner), pitched, with a matrix; the stored frame in
    the descriptor, the rect and the ratios O's, the extents the stored planes'; 16384 x 1 under rot 1.  `plain`: at k = 0 the descriptor
    is ht_draw_list_plan_entry's own."""
    cases = []
    for fmt in oc.FORMATS:
        for k in oc.ORIENTATIONS:
            ow, oh = oc.oriented_size(k, 37, 23)
            pitch0 = {dl.RGBA: 4 * 37 + 8, y4.YUYV: 4 * 19 + 4, y4.UYVY: 4 * 19 + 12}.get(fmt, 37 + 3)
            pitch1 = 0 if fmt in (dl.RGBA, y4.YUYV, y4.UYVY) else (2 * 19 + 2 if fmt == yc.NV12 else 19 + 5)
            cases.append(entry(fmt, k, 37, 23, 97, 81, matrix=k % 4))
            cases.append(entry(fmt, k, 37, 23, 97, 81, pitch0=pitch0, pitch1=pitch1, matrix=(k + 1) % 4, rect=(1, 3, ow - 1, oh - 3)))
    cases.append(entry(dl.RGBA, 1, BIG, 1, 320, 240))                                   # 16384 x 1 under rot 1: O is 1 x 16384
    cases.append(entry(yc.NV12, 1, BIG, 1, 320, 240, rect=(0, BIG - 1, 1, 1)))          # ... and its last row, a column of S
    cases.append(entry(y4.YUYV, 7, 1, BIG, 320, 240, rect=(BIG - 1, 0, 1, 1)))
    got = _run(harness, "entry", tmp_path, cases)
    for c, g in zip(cases, got):
        plain = g.pop("plain")
        assert g == want_entry(c), (c, g)
        if c[7] >> 8 == 0:
            assert plain is True, c   # k = 0 written through the bits IS the draw list's descriptor
    assert got[-3]["size"] == [1, BIG] and got[-3]["rect"] == [0, 0, 1, BIG] and got[-3]["ratio_bits"] == [_bits(1 / 320), _bits(BIG / 240)]


def test_k0_through_the_bits_is_the_draw_lists_own_descriptor(harness, tmp_path):
    """orientation 0 on every format, whole and under rects: ht_orient_as_plain(plan) == ht_draw_list_plan_entry(entry), descriptor and
    extents compared as bytes"""
    cases = [entry(fmt, 0, 333, 217, 97, 81, matrix=2, rect=r) for fmt in oc.FORMATS for r in ((0, 0, 0, 0), (3, 5, 326, 208), (332, 216, 1, 1))]
    got = _run(harness, "entry", tmp_path, cases)
    assert all(g["status"] == 0 and g["plain"] is True and g["orient"] == 0 and g["present"] is False for g in got), got


def test_rect_refusals_both_ways(harness, tmp_path):
    """37 x 23 under rot 1 is 23 x 37: a rect inside O but outside S is legal, one inside S but outside O is BAD_RECT; the same under flip
    alone follows S's shape"""
    in_o_not_s, in_s_not_o = (0, 0, 23, 37), (0, 0, 37, 23)
    legal = [entry(fmt, k, 37, 23, 97, 81, rect=in_o_not_s) for fmt in oc.FORMATS for k in (1, 3, 5, 7)] + [entry(fmt, k, 37, 23, 97, 81, rect=in_s_not_o) for fmt in oc.FORMATS for k in (0, 2, 4, 6)]
    bad = [entry(fmt, k, 37, 23, 97, 81, rect=in_s_not_o) for fmt in oc.FORMATS for k in (1, 3, 5, 7)] + [entry(fmt, k, 37, 23, 97, 81, rect=in_o_not_s) for fmt in oc.FORMATS for k in (0, 2, 4, 6)]
    bad += [entry(dl.RGBA, 1, 37, 23, 97, 81, rect=r) for r in ((-1, 0, 4, 4), (0, 0, 24, 1), (22, 36, 2, 1), (0, 0, 0, 5), (0, 0, 5, -1), (23, 0, 1, 1))]
    got = _run(harness, "entry", tmp_path, legal + bad)
    assert all(g["status"] == OK for g in got[:len(legal)]), got[:len(legal)]
    assert [g for g in got[len(legal):]] == [{"status": L_BAD_RECT}] * len(bad)


def test_bad_bits_and_refused_formats_stay_refused(harness, tmp_path):
    """any bit from 11 up, or the sign, is no format whatever the low bits say; the formats tests/yuv422_cases.py lists as refused stay
    refused under every k; the other statuses still come from the stored frame's plan"""
    bad = [(entry(dl.RGBA, 0, 37, 23, 97, 81, raw=raw), L_BAD_FORMAT) for raw in (dl.RGBA | 1 << 11, yc.NV12 | 1 << 11, 4 | 5 << 8 | 1 << 12, 1 << 30, dl.RGBA | 1 << 16, -(1 << 31) | dl.RGBA)]
    bad += [(entry(f & 0xff, k, 37, 23, 97, 81, raw=(f & 0xff) | k << 8 if f >= 0 else f), L_BAD_FORMAT) for f in y4.REFUSED_FORMATS for k in oc.ORIENTATIONS]
    bad += [(entry(yc.NV12, 3, 37, 23, 97, 81, p1=P1 + 1), L_MISALIGNED), (entry(y4.YUYV, 5, 37, 23, 97, 81, p0=P0 + 2), L_MISALIGNED), (entry(dl.RGBA, 6, 37, 23, 97, 81, p0=0), L_NULL_PLANE),
            (entry(yc.I420, 1, 37, 23, 97, 81, p2=0), L_NULL_PLANE), (entry(dl.RGBA, 1, 37, 23, 97, 81, pitch0=4 * 37 - 4), L_BAD_PITCH0), (entry(yc.NV12, 2, 37, 23, 97, 81, pitch1=37), L_BAD_PITCH1),
            (entry(yc.I420, 7, 0, 23, 97, 81), L_BAD_SIZE), (entry(dl.RGBA, 1, BIG + 1, 1, 97, 81), L_BAD_SIZE), (entry(yc.NV12, 4, 37, 23, 97, 81, matrix=4), L_BAD_MATRIX)]
    got = _run(harness, "entry", tmp_path, [c for c, _ in bad])
    for (c, want), g in zip(bad, got):
        assert g == {"status": want}, (c, g)


def test_map_in_the_header_is_the_numpy_permutation(harness, tmp_path):
    """ht_orient_map itself, every pixel of 1 x 1, 1 x 5, 2 x 2, 23 x 23 and 37 x 22 under all eight k"""
    cases = [(k, w, h) for (w, h) in oc.MAPPING_SIZES[:5] for k in oc.ORIENTATIONS]
    got = _run(harness, "map", tmp_path, cases)
    for (k, w, h), g in zip(cases, got):
        stored = np.arange(w * h).reshape(h, w)
        ow, oh = oc.oriented_size(k, w, h)
        assert g["size"] == [ow, oh]
        uv = np.array(g["uv"]).reshape(oh, ow, 2)
        assert np.array_equal(stored[uv[..., 1], uv[..., 0]], oc.orient(stored, k)), (k, w, h)


def test_orient_first_job_and_the_upright_entry(harness, tmp_path):
    """what the calls that orient first are given: the 1 : 1 job (the whole of O, both ratios exactly 1.0, the stored planes untouched) and
    the RGBA entry of O the oriented entry becomes (packed pitch, O's size, the rect kept)"""
    cases = [entry(yc.NV12, 1, 333, 217, 97, 81, matrix=1, pitch0=340, rect=(3, 5, 200, 300)), entry(y4.UYVY, 6, 333, 217, 97, 81, matrix=3), entry(dl.RGBA, 7, 37, 23, 97, 81, rect=(1, 1, 22, 36))]
    got = _run(harness, "whole", tmp_path, cases)
    for c, g in zip(cases, got):
        w, h, k = c[5], c[6], c[7] >> 8
        ow, oh = oc.oriented_size(k, w, h)
        want = want_entry(c)
        assert g["rect"] == [0, 0, ow, oh] and g["ratio_bits"] == [_bits(1.0)] * 2 and g["orient"] == k and g["frame"] == 0
        assert all(g[key] == want[key] for key in ("p", "pitch", "stored", "cw", "format", "kc"))
        assert g["upright"] == dict(p=[0x7000, 0, 0], pitch=[4 * ow, 0], size=[ow, oh], format=dl.RGBA, matrix=0, rect=list(c[9:13]))


# ---- the module's code object ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def module_notes():
    build.build_lib()
    assert os.path.exists(build.ORIENT_MODULE) and build.ORIENT_MODULE == os.path.join(os.path.dirname(build.LIB), "libheadtrackr_hip_orient.hsaco")
    return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", build.ORIENT_MODULE], capture_output=True, text=True, check=True).stdout


def _kernels(notes):
    out, cur = {}, None
    for ln in notes.splitlines():
        m = re.match(r"\s*(-?)\s*\.(\w+):\s*(.*)$", ln)
        if not m:
            continue
        dash, key, val = m.group(1), m.group(2), m.group(3).strip().strip("'")
        if dash and key == "agpr_count":
            cur = {}
        if cur is None:
            continue
        if key == "name" and val.startswith(("_Z", "k_")):
            out[val] = cur
        elif re.fullmatch(r"-?\d+", val):
            cur[key] = int(val)
    return out


def test_module_is_a_plain_gfx950_code_object_with_its_kernels(module_notes):
    """a build produces the .hsaco next to the library: a bare ELF (no offload bundle around it) whose notes name gfx950 and
    k_draw_list_oriented; no spills, no scratch, LDS far inside 64 KB, 256 threads, at most 64 VGPRs (8 wavefronts per SIMD, what the draw
    kernels it stands beside are held to); no kernel name carries a marker of benchlib.fingerprint.UNITS"""
    from benchlib import fingerprint

    data = open(build.ORIENT_MODULE, "rb").read()
    assert data[:4] == b"\x7fELF" and b"__CLANG_OFFLOAD_BUNDLE__" not in data
    assert "amdgcn-amd-amdhsa--gfx950" in module_notes
    ks = _kernels(module_notes)
    assert set(ks) == {"k_draw_list_oriented", "k_draw_list_oriented_turn"}, sorted(ks)
    for name, r in ks.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["max_flat_workgroup_size"] == 256 and r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 8 * 1024, (name, r)
        assert not any(marker.decode() in name for marker in fingerprint.UNITS.values())
    assert ks["k_draw_list_oriented"]["group_segment_fixed_size"] == 24 * (64 + 16)
    assert ks["k_draw_list_oriented_turn"]["group_segment_fixed_size"] == 24 * (32 + 32) + 4 * 32 * 33
    assert not any(marker in data for marker in fingerprint.UNITS.values())


def test_module_source_is_outside_the_library():
    """ht_orient_kernels.hip is not one of the library's translation units, is included by none of them, and holds the only __global__ of
    the oriented draw; the library's host code names the module's file and its two kernels"""
    assert build.ORIENT_SOURCE == "ht_orient_kernels.hip" and build.ORIENT_SOURCE not in build.HIP_SOURCES
    for f in (f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".cc"))):
        text = open(os.path.join(CSRC, f)).read()
        if f != build.ORIENT_SOURCE:
            assert '#include "ht_orient_kernels.hip"' not in text and "__global__ __launch_bounds__(OR_NT)" not in text, f
    host = open(os.path.join(CSRC, "ht_draw_list.hip")).read()
    assert '"/libheadtrackr_hip_orient.hsaco"' in host and '"k_draw_list_oriented"' in host and '"k_draw_list_oriented_turn"' in host and "getenv" not in host
    assert "-ffp-contract=off" in build.HIP_FLAGS and build.ORIENT_FLAGS == ["--cuda-device-only", "--no-gpu-bundle-output"]


def _function_body(text, name):
    """the parameter list and body of `uint32_t <name>(`, from its opening parenthesis to the closing brace of the function"""
    at = text.index("uint32_t " + name + "(")
    end = text.index("\n}\n", at)
    return text[at + len("uint32_t " + name):end]


def test_blend_body_is_ig_channels_text():
    """the module cannot include ig_channel (ht_ingest.hip is the library's), so it restates it as or_channel: the two functions are equal
    as text once the name is put back — parameters, every operation, the rounding, the comments"""
    mine = _function_body(open(os.path.join(CSRC, "ht_orient_kernels.hip")).read(), "or_channel")
    theirs = _function_body(open(os.path.join(CSRC, "ht_ingest.hip")).read(), "ig_channel")
    assert mine == theirs and "__dmul_rn" in mine and "__builtin_rint" in mine
    # ... and the definitions the CPU suite counts across csrc/ stay single: the shared headers are included, not restated
    text = open(os.path.join(CSRC, "ht_orient_kernels.hip")).read()
    assert "uint32_t ig_channel(" not in text and "RsTap rs_tap(" not in text and "ht_yuv_to_rgba(int32_t" not in text
    for header in ("ht_resample_tap.h", "ht_yuv_plan.h", "ht_orient_plan.h"):
        assert f'#include "{header}"' in text


def test_python_layer_packs_the_orientation_into_the_format():
    """_draw_sources and draw_frames_yuv_device write format | k << 8; k outside 0..7 raises before anything reaches the library"""
    c = api.Context.__new__(api.Context)  # no device: only the marshalling is exercised
    for name, code in (("rgba", 16), ("nv12", 0), ("i420", 1), ("yuyv", 4), ("uyvy", 5)):
        for k in range(8):
            arr = c._draw_sources([dict(format=name, width=4, height=2, p0=4096, orientation=k)])
            assert arr[0].format == code | k << 8
        assert c._draw_sources([dict(format=name, width=4, height=2, p0=4096)])[0].format == code
    for bad in (-1, 8, 2.5):
        with pytest.raises(ValueError):
            c._draw_sources([dict(format="nv12", width=4, height=2, p0=4096, orientation=bad)])
        with pytest.raises(ValueError):
            c.draw_frames_yuv_device(4096, 8192, None, 1, 4, 2, orientation=bad)
        with pytest.raises(ValueError):
            c.draw_frames_yuv((np.zeros((1, 2, 4), np.uint8), np.zeros((1, 1, 2, 2), np.uint8)), orientation=bad)

"""CPU-side checks of the model-input tensors (ht_camshift_crop_*_tensor_device / ht_camshift_align_*_tensor_device): the rule in
headtrackr_amd/csrc/ht_patch_plan.h — the lines k_cut_tensor and k_upright_tensor compile for the device — against the Python restatement
of tests/patch_tensor_cases.py on every byte, every pair and every dtype, the gray byte on all 2^24 triples, the format check's refusals,
sizes and offsets, plain and under AddressSanitizer + UBSan as a program of its own; the pairs proved, from the restatement alone, to
exercise every rounding branch they claim (and a fused multiply-add to be visible); the entry points at every layer; the kernels' budget
from code-object metadata; torch_patches on CPU tensors.  No compute calls (no GPU here).  Without the feature every test fails at its
first import or call."""
import ctypes as C
import importlib.util
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import patch_tensor_cases as pt
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
EXPORTS = ("ht_camshift_crop_pairs_tensor_device", "ht_camshift_crop_sources_tensor_device", "ht_camshift_align_pairs_tensor_device",
           "ht_camshift_align_sources_tensor_device")
SIZES = [(1, 1), (7, 3), (70, 19), (1024, 1024)]


def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("patch_plan") / ("patch_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "patch_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    """the program plain and with AddressSanitizer + UBSan linked in: stand-alone executables, run directly"""
    return {"plain": _build_harness(tmp_path_factory, False), "sanitized": _build_harness(tmp_path_factory, True)}


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])


# ---- the pairs exercise what they claim: from the restatement alone ---------------------------------------------------------------------

def test_the_pairs_cover_every_rounding_branch_and_a_fused_multiply_add_would_show():
    """1 + 2^-8 has 8 exact bfloat16 ties (the power-of-two bytes) that round-half-up would round the other way; 1 + 2^-11 has 8 exact
    binary16 ties; 300 sends 37 bytes to +inf in binary16; 2^-20 gives 63 non-zero binary16 subnormals; the bounds and the signed zero
    are there; and for at least one pair a byte exists where ONE rounding of b * scale + bias (exact rational arithmetic) gives other
    binary32 bits than the rule's two"""
    b = np.arange(256, dtype=np.uint8)
    u = pt.bits(pt.value(b, *[p[0] for p in pt.PAIRS["bf16_ties"]]), "f32")
    ties = [int(x) for x in b[(u & 0xFFFF) == 0x8000]]
    assert ties == [1, 2, 4, 8, 16, 32, 64, 128]
    rne, half_up = pt.byte_table("bf16_ties", "bf16"), ((u.astype(np.uint64) + 0x8000) >> 16).astype(np.uint16)
    assert [int(x) for x in b[rne != half_up]] == [t for t in ties if not ((int(u[t]) >> 16) & 1)] and (rne != half_up).sum() >= 1
    u = pt.bits(pt.value(b, *[p[0] for p in pt.PAIRS["f16_ties"]]), "f32")
    assert [int(x) for x in b[(u & 0x1FFF) == 0x1000]] == [1, 2, 4, 8, 16, 32, 64, 128]
    h = pt.byte_table("f16_ties", "f16")
    assert all(int(h[t]) == int(np.float16(t).view(np.uint16)) for t in (1, 2, 4, 8, 16, 32, 64, 128))  # ties to even: down to the byte itself
    h = pt.byte_table("f16_overflow", "f16")
    assert int((h == 0x7C00).sum()) == 37 and int(h[218]) < 0x7C00 == int(h[219])
    h = pt.byte_table("f16_subnormal", "f16")
    assert int(((h > 0) & (h < 0x0400)).sum()) == 63 and int(h[64]) == 0x0400
    assert (pt.byte_table("zero", "f32") == 0).all() and (pt.byte_table("negative_zero_bias", "f32") == 0).all()  # +0 + -0 = +0
    assert int(pt.byte_table("inverted", "f32")[255]) == 0 and int(pt.byte_table("largest", "f32")[0]) == struct.unpack("<I", struct.pack("<f", -2.0 ** 64))[0]
    assert int(pt.byte_table("smallest", "f32")[1]) == (127 - 64) << 23 and int(pt.byte_table("largest", "f32")[255]) == struct.unpack("<I", struct.pack("<f", 254 * 2.0 ** 64))[0]
    for name in pt.PAIRS:  # the bounds' promise: no binary32 intermediate is subnormal, infinite or NaN
        for c in range(3):
            m = b.astype(np.float32) * np.float32(pt.PAIRS[name][0][c])
            for v in (m, pt.value(b, pt.PAIRS[name][0][c], pt.PAIRS[name][1][c])):
                a = np.abs(v[v != 0])
                assert np.isfinite(v).all() and (a >= 2.0 ** -126).all(), name
    differs = {name: pt.fma_differs(name, c) for name in ("signed", "imagenet") for c in range(1)}
    assert any(differs.values()), differs
    assert pt.round_to_f32(pt.Fraction(1, 3)) == pt.f32(1 / 3) and pt.round_to_f32(pt.Fraction(-16777217)) == -16777216.0


# ---- the header against the restatement -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_values_equal_the_restatement_on_every_byte_pair_and_dtype(harnesses, tmp_path, which):
    """every byte 0 .. 255 x every (scale, bias) of every pair and channel x f32, f16, bf16: ht_patch_value and ht_patch_element give the
    restatement's bits (the host text of binary16 is integer arithmetic: numpy's conversion is the reference)"""
    sb = [struct.unpack("<2f", k) for k in sorted({struct.pack("<2f", pt.PAIRS[n][0][c], pt.PAIRS[n][1][c]) for n in pt.PAIRS for c in range(3)})]  # by bits: -0.0 is a pair of its own
    assert len(sb) == 14
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(b"".join(struct.pack("<2f", *p) for p in sb))
    _run(harnesses[which], "--values", src, dst)
    got = np.fromfile(dst, dtype=np.uint32).reshape(len(sb), 256, 3)
    b = np.arange(256, dtype=np.uint8)
    for i, (s, bi) in enumerate(sb):
        v = pt.value(b, s, bi)
        for k, dt in enumerate(pt.DTYPES):
            want = pt.bits(v, dt).astype(np.uint32)
            assert (got[i, :, k] == want).all(), (s, bi, dt, [(int(x), hex(int(got[i, x, k])), hex(int(want[x]))) for x in b[got[i, :, k] != want][:4]])


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_header_gray_byte_equals_the_restatement_on_all_rgb_triples(harnesses, tmp_path, which):
    """all 2^24 (R, G, B): ht_gray.h's text (the one ht_pyramid.hip compiles) gives ccv.js:29's byte"""
    dst = str(tmp_path / "gray.bin")
    _run(harnesses[which], "--gray", dst)
    got = np.fromfile(dst, dtype=np.uint8)
    idx = np.arange(1 << 24, dtype=np.uint32)
    want = pt.gray((idx & 255).astype(np.uint8), ((idx >> 8) & 255).astype(np.uint8), ((idx >> 16) & 255).astype(np.uint8))
    assert got.shape == want.shape and (got == want).all()
    assert want[0xFFFFFF] == 255 and want[0] == 0 and len(np.unique(want)) == 256


def _format_cases():
    """(packed ht_patch_format, expected code): 0 = accepted; 1 dtype, 2 layout, 3 channels, 4 pad, 5 scale, 6 bias, 7 unused slot"""
    ok3, z3 = (1 / 255,) * 3, (0.0,) * 3
    cases = []
    for d in range(3):
        for l in range(2):
            cases.append((pt.pack_format(d, l, 0, 0, ok3, (-1.0,) * 3), 0))
            cases.append((pt.pack_format(d, l, 1, 0, ok3, z3), 0))
            cases.append((pt.pack_format(d, l, 2, 0, (0.5, 0.0, 0.0), (-0.0, 0.0, -0.0)), 0))
    for v in (2.0 ** -64, -(2.0 ** -64), 2.0 ** 64, -(2.0 ** 64), 0.0, -0.0):  # the bounds themselves, both signs
        cases.append((pt.pack_format(0, 0, 0, 0, (v, 1.0, 1.0), z3), 0))
        cases.append((pt.pack_format(0, 0, 0, 0, ok3, (0.0, 0.0, v)), 0))
    below = float(np.nextafter(np.float32(2.0 ** -64), np.float32(0)))
    above = float(np.nextafter(np.float32(2.0 ** 64), np.float32(np.inf)))
    for v in (float("nan"), float("inf"), float("-inf"), below, -below, above, -above, 1e-45, 2.0 ** -127, 3.0e38):
        for c in range(3):
            s = [1.0, 1.0, 1.0]
            s[c] = v
            cases.append((pt.pack_format(1, 0, 0, 0, s, z3), 5))
            cases.append((pt.pack_format(2, 1, 1, 0, ok3, tuple(v if k == c else 0.0 for k in range(3))), 6))
        cases.append((pt.pack_format(0, 0, 2, 0, (v, 0.0, 0.0), z3), 5))
    for slot in (1, 2):  # gray: slots 1 and 2 are unused
        for v in (1.0, 2.0 ** -80, float("nan")):
            cases.append((pt.pack_format(0, 0, 2, 0, tuple(v if k == slot else (1.0 if k == 0 else 0.0) for k in range(3)), z3), 7))
            cases.append((pt.pack_format(0, 0, 2, 0, (1.0, 0.0, 0.0), tuple(v if k == slot else 0.0 for k in range(3))), 7))
    for bad in (-1, 3, 255, 2 ** 31 - 1, -2 ** 31):
        cases.append((pt.pack_format(bad, 0, 0, 0, ok3, z3), 1))
        cases.append((pt.pack_format(0, bad if bad != -1 else 2, 0, 0, ok3, z3), 2))
        cases.append((pt.pack_format(0, 0, bad, 0, ok3, z3), 3))
        cases.append((pt.pack_format(0, 0, 0, bad, ok3, z3), 4))
    cases.append((pt.pack_format(0, -1, 0, 0, ok3, z3), 2))
    cases.append((pt.pack_format(0, 0, 0, 1, ok3, z3), 4))
    return cases


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_format_check_accepts_the_bounds_and_refuses_everything_beyond(harnesses, tmp_path, which):
    """NaN, both infinities, magnitudes just below 2^-64 (subnormals included) and just above 2^64, in scale and in bias, in every slot;
    non-zero unused slots of gray (a NaN among them); unknown dtype, layout and channels values; a non-zero pad — and the bounds
    themselves, both zeros and every valid enum combination accepted"""
    cases = _format_cases()
    src, dst = str(tmp_path / "fmt.bin"), str(tmp_path / "fmt.out")
    with open(src, "wb") as f:
        f.write(b"".join(c[0] for c in cases))
    _run(harnesses[which], "--formats", src, dst)
    got = np.fromfile(dst, dtype=np.int32).tolist()
    want = [c[1] for c in cases]
    assert got == want, [(i, g, w, pt.FORMAT_STRUCT.unpack(cases[i][0])) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    assert set(want) == set(range(8))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_patch_sizes_strides_and_plane_offsets(harnesses, tmp_path, which):
    """1 x 1, 7 x 3 (odd plane: a 16-bit plane starts 2-byte aligned), 70 x 19 and 1024 x 1024 at each dtype, layout and channel mode:
    a patch's bytes, the default stride (rounded up to 4) and the offsets of the first and last element of every channel"""
    qs = [(w, h, pt.DTYPE_CODE[d], pt.LAYOUT_CODE[l], pt.CHANNELS_CODE[ch], d, l, ch) for (w, h) in SIZES for (d, l, ch) in pt.FORMATS]
    src, dst = str(tmp_path / "sz.bin"), str(tmp_path / "sz.out")
    with open(src, "wb") as f:
        f.write(b"".join(struct.pack("<5i", *q[:5]) for q in qs))
    _run(harnesses[which], "--sizes", src, dst)
    got = np.fromfile(dst, dtype=np.uint64).reshape(len(qs), 8)
    odd_planes = 0
    for g, (w, h, _d, _l, _c, d, l, ch) in zip(got.tolist(), qs):
        C = pt.nchannels(ch)
        want = [pt.patch_bytes(w, h, d, ch), pt.default_stride(w, h, d, ch)]
        want += [pt.offset(w, h, d, l, ch, c, 0, 0) if c < C else 0 for c in range(3)] + [pt.offset(w, h, d, l, ch, c, w - 1, h - 1) if c < C else 0 for c in range(3)]
        assert g == want, (w, h, d, l, ch, g, want)
        assert want[0] == C * w * h * pt.ESIZE[d] and want[1] % 4 == 0 and 0 <= want[1] - want[0] < 4
        assert max(want[5:]) + pt.ESIZE[d] == want[0]  # the last element of the last channel ends the patch
        odd_planes += l == "chw" and C == 3 and want[3] % 4 == 2
    assert odd_planes >= 4  # 1 x 1 and 7 x 3 at f16 and bf16
    # the restatement's f() lays a patch out by those offsets
    rng = np.random.RandomState(5)
    patch = rng.randint(0, 256, (3, 7, 4)).astype(np.uint8)
    for fmt in pt.FORMATS:
        pair = pt.pair_for("imagenet", fmt[2])
        by = pt.f(patch, fmt, pair)
        assert by.size == pt.patch_bytes(7, 3, fmt[0], fmt[2])
        src_b = pt.source_bytes(patch, fmt[2])
        for (c, x, y) in ((0, 0, 0), (pt.nchannels(fmt[2]) - 1, 6, 2), (0, 3, 1)):
            e = pt.bits(pt.value(src_b[y:y + 1, x, c], pair[0][c], pair[1][c]), fmt[0])
            o = pt.offset(7, 3, *fmt, c, x, y)
            assert by[o:o + pt.ESIZE[fmt[0]]].tobytes() == e.tobytes(), (fmt, c, x, y)


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_at_every_layer_and_fail_loudly_without_a_device(tmp_path):
    """the header, the library, native.py, the API and INTEGRATION.md all name the four exports; ht_patch_format is 40 bytes with the same
    offsets in C and in ctypes; the enums are the issue's; the ABI version stays 2; every export answers a NULL context with a status"""
    from headtrackr_amd.api import Context, PatchFormat

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    for line in ("enum { HT_PATCH_F32 = 0, HT_PATCH_F16 = 1, HT_PATCH_BF16 = 2 };", "enum { HT_PATCH_CHW = 0, HT_PATCH_HWC = 1 };",
                 "enum { HT_PATCH_RGB = 0, HT_PATCH_BGR = 1, HT_PATCH_GRAY = 2 };", "typedef struct ht_patch_format", "#define HT_ABI_VERSION 2"):
        assert line in header, line
    prog = tmp_path / "offsets.c"
    fields = ("dtype", "layout", "channels", "pad", "scale", "bias")
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "headtrackr_hip.h"\nint main(void) { printf("%zu", sizeof(ht_patch_format));\n'
                    + "".join('printf(" %%zu", offsetof(ht_patch_format, %s));\n' % f for f in fields) + "return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(tmp_path / "offsets")])
    offsets = [0, 4, 8, 12, 16, 28]
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "offsets")], text=True).split()] == [40] + offsets
    assert C.sizeof(native.PATCH_FORMAT) == 40 == pt.FORMAT_STRUCT.size and [getattr(native.PATCH_FORMAT, f).offset for f in fields] == offsets
    assert (native.HT_PATCH_F32, native.HT_PATCH_F16, native.HT_PATCH_BF16, native.HT_PATCH_CHW, native.HT_PATCH_HWC) == (0, 1, 2, 0, 1)
    assert (native.HT_PATCH_RGB, native.HT_PATCH_BGR, native.HT_PATCH_GRAY) == (0, 1, 2)
    assert native.PATCH_DTYPES == pt.DTYPE_CODE and native.PATCH_LAYOUTS == pt.LAYOUT_CODE and native.PATCH_CHANNELS == pt.CHANNELS_CODE
    fmt, prm, src = PatchFormat("f16", "chw", "rgb").struct(), native.CROP_PARAMS(7, 3, 256, 0), (native.DRAW_SOURCE * 1)()
    aprm = native.ALIGN_PARAMS(7, 3, 256, 0)
    assert L.ht_camshift_crop_pairs_tensor_device(None, None, 0, None, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_crop_sources_tensor_device(None, None, src, 1, C.byref(prm), C.byref(fmt), None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_pairs_tensor_device(None, None, 0, C.byref(aprm), C.byref(fmt), None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_sources_tensor_device(None, None, None, 0, None, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_abi_version() == 2
    for m in ("camshift_crop_pairs_tensor_device", "camshift_crop_sources_tensor_device", "camshift_align_pairs_tensor_device", "camshift_align_sources_tensor_device"):
        assert callable(getattr(Context, m)), m
    # the format object: mean_std in binary64, then binary32; one value for all channels; refusals
    f = PatchFormat.mean_std(pt.IMAGENET_MEAN, pt.IMAGENET_STD)
    assert (f.scale, f.bias) == pt.PAIRS["imagenet"] and (f.dtype, f.layout, f.channels) == ("f16", "chw", "rgb")
    s = f.struct()
    assert bytes(s) == pt.pack_format(1, 0, 0, 0, *pt.PAIRS["imagenet"])
    g = PatchFormat.of(dict(dtype="bf16", layout="hwc", channels="gray", scale=0.5, bias=(-1.0,)))
    assert bytes(g.struct()) == pt.pack_format(2, 1, 2, 0, (0.5, 0.0, 0.0), (-1.0, 0.0, 0.0)) and g.shape(7, 3) == (3, 7, 1) and g.patch_bytes(7, 3) == 42 and g.default_stride(7, 3) == 44
    assert PatchFormat("f32", "chw", "bgr", scale=2 / 255, bias=-1).shape(7, 3) == (3, 3, 7)
    for bad in (dict(dtype="f64"), dict(layout="nchw"), dict(channels="rgba"), dict(scale=(1.0, 2.0)), dict(channels="gray", bias=(0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            PatchFormat(**bad)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tensor_kernels_have_no_spills_and_no_scratch_and_share_the_sampling_text():
    """code-object METADATA only: k_cut_tensor<dtype> and k_upright_tensor<dtype> — the crop's and the align call's kernels with the tensor
    output stage; tests/test_crop_cpu.py and tests/test_align_cpu.py reserve those two words for k_crop_list and k_align_list — exist for
    all three dtypes, have no spills and no scratch, at most the LDS and no more than 8 VGPRs above their RGBA siblings (the occupancy
    step), and live in the code object of k_crop_list; the sampling bodies are shared as text through the store hooks, and the gray byte is
    one text for ht_pyramid.hip and the rule header"""
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for fam, sibling in (("k_cut_tensor", "k_crop_list"), ("k_upright_tensor", "k_align_list")):
        names = sorted(k for k in res if k.startswith(fam))
        assert names == [f"{fam}<{d}>" for d in range(3)], names
        for k in names:
            r = res[k]
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
            assert r["group_segment_fixed_size"] == res[sibling]["group_segment_fixed_size"] and r["vgpr_count"] <= 64, (k, r)
    objs = _gfx950_code_objects(build.LIB)
    home = [o for o in objs if b"k_cut_tensor" in o]
    assert len(objs) == 4 and len(home) == 1 and b"k_crop_list" in home[0] and b"k_upright_tensor" in home[0] and b"k_align_list" in home[0]
    family = ("ht_crop.hip", "ht_align.hip", "ht_patch.hip", "ht_filter.hip", "ht_face_calls.hip", "ht_list_parts.inc")
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_patch_plan.h", "ht_ingest_bodies.inc", "ht_pyramid.hip", "ht_gray.h") + family}
    whole = "".join(text[f] for f in family)
    assert text["ht_ingest.hip"].index('#include "ht_align.hip"') < text["ht_ingest.hip"].index('#include "ht_patch.hip"')
    assert text["ht_ingest_bodies.inc"].count("        IG_STORE(o, x, Y0 + ") == 2 and "out[(size_t)(Y0" not in text["ht_ingest_bodies.inc"]
    # the tensor kernels compile the RGBA kernels' text: the cut head with the ONE crop rule, the ONE format scaffold around the pixel bodies
    # (this file's only other include of them is the taps), the upright head and the ONE al_pixels dispatch
    assert whole.count("ht_crop_rule(") == 1 and text["ht_list_parts.inc"].count('#include "ht_ingest_bodies.inc"') == 3 and text["ht_patch.hip"].count('#include "ht_ingest_bodies.inc"') == 1
    assert text["ht_patch.hip"].count("#define LP_PART 1  // LP_CUT_HEAD") == 1 and text["ht_patch.hip"].count("#define LP_PART 4  // LP_SCAFFOLD") == 1
    assert text["ht_patch.hip"].count("#define LP_PART 2  // LP_UPRIGHT_HEAD") == 1 and text["ht_patch.hip"].count("AL_PIXELS_ANY(") == 1
    assert whole.count("al_pixels<") == text["ht_align.hip"].count("al_pixels<") == 3 and whole.count("#define AL_PIXELS_ANY(") == 1
    assert "store(o, x, y);" in text["ht_align.hip"] and "ht_gray_of(px)" in text["ht_pyramid.hip"] and "__dmul_rn" not in text["ht_pyramid.hip"].split("k_gray_linear")[0].split("xcd_item")[1]
    # the checks are the crop calls' own: ONE check of a call, ONE check of a format, in the family's one host path
    assert whole.count("ht_patch_check_format(") == 1 and "ht_patch_check_format(" in text["ht_face_calls.hip"] and whole.count("ht_status face_check(") == 1
    assert "_check(" not in text["ht_patch.hip"] and "extern" not in text["ht_patch.hip"]
    plan = text["ht_patch_plan.h"]
    assert "hip/" not in plan and "__global__" not in plan and "<math" not in plan and "<cmath" not in plan


# ---- torch_patches on CPU tensors -------------------------------------------------------------------------------------------------------------

def test_torch_patches_shapes_dtypes_and_refusals_on_cpu_tensors():
    """empty_patches gives [n, C, H, W] or [n, H, W, C] of the format's dtype; the wrappers refuse a wrong dtype, a non-contiguous tensor,
    a wrong shape or count and a tensor that is not in device memory before the context is touched (the context here is an object that
    fails on any use)"""
    torch = pytest.importorskip("torch")
    from headtrackr_amd import torch_patches as tp
    from headtrackr_amd.api import PatchFormat

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the context was touched: {name}")

    ctx = Untouchable()
    want_dtype = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    for (d, l, ch) in pt.FORMATS:
        fmt = PatchFormat(d, l, ch)
        t = tp.empty_patches(5, 7, 3, fmt, "cpu")
        C = pt.nchannels(ch)
        assert tuple(t.shape) == ((5, C, 3, 7) if l == "chw" else (5, 3, 7, C)) and t.dtype == want_dtype[d] and t.is_contiguous()
        assert t[0].numel() * t.element_size() == pt.patch_bytes(7, 3, d, ch)
    with pytest.raises(ValueError):
        tp.empty_patches(0, 7, 3, PatchFormat(), "cpu")
    fmt = PatchFormat("f16", "chw", "rgb")
    pairs = [(0, 0)] * 4
    good = tp.empty_patches(4, 8, 6, fmt, "cpu")
    calls = [lambda t: tp.crop_pairs_into(ctx, t, pairs, fmt), lambda t: tp.align_pairs_into(ctx, t, pairs, fmt),
             lambda t: tp.crop_sources_into(ctx, t, [0] * 4, [{}] * 4, fmt), lambda t: tp.align_sources_into(ctx, t, [0] * 4, [{}] * 4, fmt)]
    for call in calls:
        with pytest.raises(TypeError):
            call(good.float())                                    # wrong dtype
        with pytest.raises(TypeError):
            call(good.numpy())                                    # no tensor
        with pytest.raises(ValueError):
            call(tp.empty_patches(4, 6, 3, fmt, "cpu").transpose(2, 3))  # [4, 3, 6, 3]: the right shape for 6 x 3 ... but not contiguous
        with pytest.raises(ValueError):
            call(good[:3])                                        # three patches for four entries
        with pytest.raises(ValueError):
            call(good.permute(0, 2, 3, 1).contiguous())           # HWC tensor for a CHW format
        with pytest.raises(ValueError):
            call(good[0])                                         # three dimensions
        with pytest.raises(ValueError, match="device memory"):
            call(good)                                            # everything right but where it lives
    odd = tp.empty_patches(4, 7, 3, fmt, "cpu")                   # 126 bytes a patch: patches 126 bytes apart are no multiple of 4
    with pytest.raises(ValueError, match="multiple of 4"):
        tp.crop_pairs_into(ctx, odd, pairs, fmt)


# ---- the N-API shim against the recording stub ------------------------------------------------------------------------------------------------

NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_the_format_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with the existing stubs and tests/js/patch_stub.cc: the successful calls of tests/js/patch_addon.js reach the
    C ABI with the pairs / streams, the params, the format's enums and the bits of its six floats, the output offset and the stride as
    given (0 stays 0: the library rounds the patch up); the range check uses the TENSOR's bytes (four f16 7 x 3 patches fit 510 bytes,
    not 508; four f32 patches do not fit what four RGBA patches fit); every malformed format throws a TypeError before the C ABI is
    reached, through the shim's one argument reader; a refusal of the library comes back as an Error"""
    addon = str(tmp_path / "addon_patch.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), *[os.path.join(ROOT, "tests", "js", f) for f in
                                                                                                        ("abi_stub.cc", "crop_stub.cc", "align_stub.cc", "patch_stub.cc")], "-o", addon])
    log = str(tmp_path / "patch.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "patch_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_PATCH_STUB_LOG=log))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["consts"] == [0, 1, 2, 0, 1, 0, 1, 2] and out["kinds"] == ["function"] * 4
    calls = [json.loads(ln) for ln in open(log)]
    bits = lambda *v: [struct.unpack("<I", struct.pack("<f", x))[0] for x in v]
    F16 = dict(format=[1, 0, 0, 0], coef=bits(1 / 255, 2 / 255, 0.5, -1.0, 0.0, -0.0))
    F32G = dict(format=[0, 1, 2, 0], coef=bits(1.0, 0.0, 0.0, 0.25, 0.0, 0.0))
    BF = dict(format=[2, 1, 1, 0], coef=bits(1.0, 1.0, 1.0, 0.0, 0.0, 0.0))
    assert F16["coef"][5] == 0x80000000  # the signed zero arrives as it was given
    for k, kind in enumerate(("crop", "align")):
        c = calls[4 * k:4 * k + 4]
        assert c[0] == dict(fn=f"{kind}_pairs", ctx=True, n=4, out=1, pairs=[[5, 0], [0, 0], [2, 1], [2, 1]], params=[7, 3, 256, 0], stride=0, **F16)
        assert c[1] == dict(fn=f"{kind}_pairs", ctx=True, n=2, out=1, pairs=[[5, 0], [0, 0]], params=[7, 3, 1024, 1], stride=100, **F32G)
        assert c[2] == dict(fn=f"{kind}_sources", ctx=True, n=2, out=-50000, streams=[3, 3], sizes=[[7, 5, 16], [23, 23, 0]], params=[7, 3, 256, 0], stride=0, **BF)
        assert c[3] == dict(fn=f"{kind}_sources", ctx=True, n=2, out=12 - 51001, streams=[1, 7], sizes=[[23, 23, 0], [7, 5, 16]], params=[7, 3, 1024, 1], stride=132, **F16)
    rest = calls[8:]
    assert len(rest) == 8 and [c["n"] for c in rest] == [4, 3] * 4  # per function: the call that exactly fits, and the one the stub refuses
    thrown = dict(out["thrown"])
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    names = {"cropPairs": "ht_camshift_crop_pairs_tensor_device", "cropSources": "ht_camshift_crop_sources_tensor_device", "alignPairs": "ht_camshift_align_pairs_tensor_device",
             "alignSources": "ht_camshift_align_sources_tensor_device"}
    kinds = {"too few arguments": "TypeError", "no format": "TypeError", "format null": "TypeError", "format without dtype": "TypeError", "dtype a string": "TypeError",
             "scale a plain array": "TypeError", "scale a Float64Array": "TypeError", "bias of two": "TypeError", "scale of four": "TypeError",
             "f16 output two bytes too small": "RangeError", "f32 output too small for what an RGBA list fits": "RangeError", "output offset beyond": "RangeError",
             "out null": "TypeError"}
    assert set(thrown) == {f"{n}: {w}" for n in names for w in list(kinds) + ["the library refuses"]}
    for n, sym in names.items():
        for what, kind in kinds.items():
            assert thrown[f"{n}: {what}"].startswith(kind + ": "), (n, what, thrown[f"{n}: {what}"])
        assert f"{sym}: status -1" in thrown[f"{n}: the library refuses"]
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert {"cropPairsTensorDevice", "cropSourcesTensorDevice", "alignPairsTensorDevice", "alignSourcesTensorDevice"} <= set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    assert napi.count("get_crop_out(a, ") == 1 and napi.count("get_patch_format(a.env, ") == 1 and "get_patch_format(env, " not in napi  # the one argument reader and range check, one format reader, each called in ONE place


# ---- the JavaScript facade on the mock addon ----------------------------------------------------------------------------------------------------

JS_TENSORS = [dict(dtype="f16", layout="chw", channels="rgb", scale=list(pt.PAIRS["imagenet"][0]), bias=list(pt.PAIRS["imagenet"][1])),
              dict(dtype="bf16", layout="hwc", channels="bgr", scale=pt.PAIRS["signed"][0][0], bias=-1),
              dict(dtype="f32", layout="chw", channels="gray", scale=[1 / 255], bias=[0])]
JS_PAIRS = [("imagenet", ("f16", "chw", "rgb")), ("signed", ("bf16", "hwc", "bgr")), ("unit", ("f32", "chw", "gray"))]


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_opts_tensor_gives_typed_arrays_of_the_rules_bits_and_changes_nothing_without_it(tmp_path):
    """tests/js/patch_cpu.js on tests/js/mock_addon_patch.js: cropPairs / alignPairs on the pairs scene and cropFeeds / alignFeeds on the
    mixed feeds, 7 x 3 (a 16-bit patch of 126 bytes: the padding behind it is not part of `patches`): without opts.tensor the result is
    the Uint8Array it always was (the restated RGBA patches' CRC-32), before and after the tensor calls; with it `patches` is a Uint16Array
    of raw bits or a Float32Array of n C w h elements whose bytes are the restated f of the restated patches, `tensor` names dtype,
    layout, channels and shape, and the records are the RGBA call's; malformed opts.tensor throw"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    import zlib

    import align_cases as al
    import crop_cases as cr
    import draw_list_cases as dl
    import yuv_cases as yc
    from test_align_cpu import _frame_source
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    W, H = cr.CANVAS
    P, Q = 7, 3
    cfg = dict(width=P, height=Q, margin=4.0, square=True)
    a, b = cr.pairs_scene()
    seqs, trackers = (a, b), cr.pairs_trackers()
    np.stack([a.frames[0], b.frames[0]]).tofile(tmp_path / "init.raw")
    np.stack([a.frames[1], b.frames[1]]).tofile(tmp_path / "step.raw")
    init_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)] + [cr.NEVER_TRACKED, 1]
    rects = [v for (_s, _f, q, j) in trackers for v in seqs[q].rects[j]] + list(b.rects[0])
    plist = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]
    objs = {s: seqs[q].oracle_calls(j)[0][2] for (s, _f, q, j) in trackers}
    frame_src = [_frame_source(seqs[q].frames[1]) for q in (0, 1)]
    job = dict(w=W, h=H, configs=[cfg], tensors=JS_TENSORS,
               pairs=dict(init=str(tmp_path / "init.raw"), step=str(tmp_path / "step.raw"), trackers=cr.RESERVED, init_pairs=init_pairs, rects=[int(v) for v in rects],
                          track_pairs=[v for (s, f, _q, _j) in trackers for v in (s, f)], align_pairs=[v for p in plist for v in p]))
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
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "patch_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["refusals"] == 2 * 7 + 1

    def patches_of(kind, entries):
        res = []
        for src, to, mapping in entries:
            if kind == "crop":
                res.append(cr.patch(src, cr.obj_of(to) if to else (0.0, 0.0, 0.0, 0.0), W, H, mapping, 1024, 1, P, Q))
            else:
                res.append(al.patch(src, al.obj_of(to) if to else al.NO_OBJECT, W, H, mapping, 1024, 1, P, Q))
        return res

    forms = {"pairs": [(frame_src[f], objs.get(s), None) for (s, f) in plist], "feeds": [(src, to, m) for (src, m), to in zip(feeds, fobjs)]}
    for form, entries in forms.items():
        n = len(entries)
        for kind in ("crop", "align"):
            got = out[form][kind]
            patches = patches_of(kind, entries)
            rgba_crc = zlib.crc32(np.stack(patches).tobytes())
            assert len(got) == 2 + len(JS_TENSORS)
            for g in (got[0], got[-1]):  # without opts.tensor: what it always was
                assert (g["kind"], g["length"], g["crc"], g["tensor"]) == ("Uint8Array", n * P * Q * 4, rgba_crc, None), (form, kind, g)
            assert any(p.any() for p in patches)
            for g, (name, fmt) in zip(got[1:-1], JS_PAIRS):
                C = pt.nchannels(fmt[2])
                want = np.concatenate([pt.f(p, fmt, pt.pair_for(name, fmt[2])) for p in patches])
                assert g["kind"] == ("Float32Array" if fmt[0] == "f32" else "Uint16Array") and g["length"] == n * C * P * Q, (form, kind, fmt, g["kind"], g["length"])
                assert g["crc"] == zlib.crc32(want.tobytes()), (form, kind, fmt)
                assert g["tensor"] == dict(dtype=fmt[0], layout=fmt[1], channels=fmt[2], shape=[n, C, Q, P] if fmt[1] == "chw" else [n, Q, P, C])
                assert g["records"] == got[0]["records"] and g["extra"] == got[0]["extra"] and g["n"] == n and g["size"] == [P, Q]
    facade = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("A.cropPairsTensorDevice(", "A.cropSourcesTensorDevice(", "A.alignPairsTensorDevice(", "A.alignSourcesTensorDevice("):
        assert facade.count(m) == 1, m

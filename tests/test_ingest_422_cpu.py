"""The packed 4:2:2 ingest (HT_YUV_YUYV = 4 / HT_YUV_UYVY = 5) without a device: the plans (csrc/ht_yuv_plan.h, csrc/ht_draw_list_plan.h) in a
stand-alone program, plain and under AddressSanitizer + UBSan; tests/yuv422_cases.py against itself and against yuv_cases; and the proof, from
the restatement alone, that the GPU case list reaches every path of the packed pixel body.  On the parent commit the plan refuses format 4,
so the first test fails there."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import yuv422_cases as y4
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# ht_yuv_plan / ht_draw_list_plan_entry statuses
OK, Y_BAD_COUNT, Y_BAD_SIZE, Y_BAD_FORMAT, Y_BAD_MATRIX, Y_BAD_Y_PITCH, Y_BAD_C_PITCH, Y_BAD_STRIDE = range(8)
L_BAD_FORMAT, L_BAD_SIZE, L_BAD_MATRIX, L_BAD_PITCH0, L_BAD_PITCH1, L_NULL_PLANE, L_MISALIGNED, L_BAD_RECT = range(3, 11)


def _build(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("yuv422_plan") / ("yuv422_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "yuv422_plan_harness.cc"),
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


def want_plan(w, h, pitch, stride, n):
    cw = (w + 1) // 2
    p = pitch or 4 * cw
    frame = p * (h - 1) + 4 * cw
    st = stride if n > 1 else 0
    return dict(status=0, cw=cw, ch=h, c_row=0, y_pitch=p, c_pitch=0, stride=st, y_extent=(n - 1) * st + frame, c_extent=0, packed_frame=4 * cw * h)


BIG = 16384
# (width, height, pitch, stride, n)
PLAN_OK = [(97, 81, 0, 0, 1), (96, 81, 0, 0, 1), (1, 1, 0, 0, 1), (2, 1, 0, 0, 1), (1, 5, 4, 0, 1), (2, 2, 4, 0, 1), (333, 217, 4 * 167 + 12, 0, 1), (97, 81, 0, 4 * 49 * 81, 3),
           (97, 81, 200, 200 * 80 + 196, 2), (97, 81, 200, 200 * 80 + 196 + 148, 3), (BIG, BIG, 0, 0, 1), (BIG - 1, BIG, 0, 4 * (BIG // 2) * BIG, 2)]
# (case: width height format matrix y_pitch c_pitch stride n), status
PLAN_BAD = [((97, 81, f, 0, 0, 0, 0, 1), Y_BAD_FORMAT) for f in y4.REFUSED_FORMATS] + [
    ((97, 81, 4, 0, 4 * 49 - 4, 0, 0, 1), Y_BAD_Y_PITCH), ((97, 81, 5, 0, 4 * 49 + 2, 0, 0, 1), Y_BAD_Y_PITCH), ((97, 81, 4, 0, 4 * 49 + 1, 0, 0, 1), Y_BAD_Y_PITCH),
    ((97, 81, 4, 0, 0, 0, 0, 2), Y_BAD_STRIDE), ((97, 81, 4, 0, 0, 0, 4 * 49 * 81 - 4, 2), Y_BAD_STRIDE), ((97, 81, 5, 0, 0, 0, 4 * 49 * 81 + 2, 2), Y_BAD_STRIDE),
    ((97, 81, 4, 0, 200, 0, 200 * 80 + 192, 2), Y_BAD_STRIDE),
    ((0, 81, 4, 0, 0, 0, 0, 1), Y_BAD_SIZE), ((97, 0, 5, 0, 0, 0, 0, 1), Y_BAD_SIZE), ((BIG + 1, 81, 4, 0, 0, 0, 0, 1), Y_BAD_SIZE), ((97, BIG + 1, 5, 0, 0, 0, 0, 1), Y_BAD_SIZE),
    ((97, 81, 4, 4, 0, 0, 0, 1), Y_BAD_MATRIX), ((97, 81, 5, -1, 0, 0, 0, 1), Y_BAD_MATRIX), ((97, 81, 4, 0, 0, 0, 0, 0), Y_BAD_COUNT),
]


def test_plan_takes_formats_4_and_5_and_refuses_the_rest(harness, tmp_path):
    """formats 4 and 5 are planned — extents, packed_frame and the macropixel count for odd and even widths, w = 1 and w = 2, pitches, n > 1 at
    a stride with a gap, 16384 x 16384 —; -1, 2, 3, 6, 7, 15 and 17 are refused as bad format; every malformed layout maps to its status.
    c_pitch is not looked at (a value that NV12 would refuse is given)."""
    ok = [(w, h, fmt, m, p, 7, st, n) for (w, h, p, st, n) in PLAN_OK for fmt, m in ((y4.YUYV, 0), (y4.UYVY, 3))]
    got = _run(harness, "plan", tmp_path, ok + [c for c, _ in PLAN_BAD])
    for c, g in zip(ok, got):
        assert g == want_plan(c[0], c[1], c[4], c[6], c[7]), (c, g)
    for (c, want), g in zip(PLAN_BAD, got[len(ok):]):
        assert g == {"status": want}, (c, g)
    assert want_plan(97, 81, 0, 0, 1)["packed_frame"] == y4.frame_bytes(97, 81) == 4 * 49 * 81


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


P0 = 0x10000


def entry(fmt, w, h, W, H, p0=P0, p1=0, p2=0, pitch0=0, pitch1=0, matrix=0, rect=(0, 0, 0, 0)):
    return (p0, p1, p2, pitch0, pitch1, w, h, fmt, matrix, *rect, W, H)


def test_draw_list_entry_of_a_packed_source(harness, tmp_path):
    """ht_draw_list_plan_entry: the descriptor (p0 alone, p1 = p2 = NULL whatever the entry says, pitch, macropixel count in cw, the matrix's
    coefficients, the ratios as one binary64 division each) and ONE extent; a 1 x 1 rect in the far corner of 16384 x 16384; the refusals"""
    ok = [entry(y4.YUYV, 97, 81, 64, 48), entry(y4.UYVY, 96, 81, 64, 48, p1=0x5001, p2=0x7003, pitch1=3, matrix=2), entry(y4.YUYV, 1, 5, 8, 8), entry(y4.UYVY, 2, 1, 8, 8),
          entry(y4.YUYV, 333, 217, 320, 240, p0=P0 + 4, pitch0=4 * 167 + 12, matrix=1, rect=(3, 5, 326, 208)), entry(y4.UYVY, BIG, BIG, 320, 240, matrix=3, rect=(BIG - 1, BIG - 1, 1, 1))]
    bad = [(entry(f, 97, 81, 64, 48), L_BAD_FORMAT) for f in y4.REFUSED_FORMATS] + [
        (entry(y4.YUYV, 97, 81, 64, 48, p0=P0 + 2), L_MISALIGNED), (entry(y4.UYVY, 97, 81, 64, 48, p0=P0 + 1), L_MISALIGNED), (entry(y4.YUYV, 97, 81, 64, 48, p0=0), L_NULL_PLANE),
        (entry(y4.YUYV, 97, 81, 64, 48, pitch0=4 * 49 - 4), L_BAD_PITCH0), (entry(y4.UYVY, 97, 81, 64, 48, pitch0=4 * 49 + 2), L_BAD_PITCH0),
        (entry(y4.YUYV, 0, 81, 64, 48), L_BAD_SIZE), (entry(y4.YUYV, 97, BIG + 1, 64, 48), L_BAD_SIZE), (entry(y4.UYVY, 97, 81, 64, 48, matrix=4), L_BAD_MATRIX),
        (entry(y4.YUYV, 97, 81, 64, 48, rect=(10, 0, 88, 81)), L_BAD_RECT), (entry(y4.UYVY, 97, 81, 64, 48, rect=(0, 1, 97, 81)), L_BAD_RECT),
        (entry(y4.YUYV, 97, 81, 64, 48, rect=(-1, 0, 8, 8)), L_BAD_RECT)]
    got = _run(harness, "entry", tmp_path, ok + [c for c, _ in bad])
    for c, g in zip(ok, got):
        p0, _p1, _p2, pitch0, _pitch1, w, h, fmt, matrix, rx, ry, rw, rh, W, H = c
        cw = (w + 1) // 2
        pitch = pitch0 or 4 * cw
        rect = [rx, ry, rw, rh] if rw or rh else [0, 0, w, h]
        assert g == dict(status=0, p=[p0, 0, 0], pitch=[pitch, 0], rect=rect, cw=cw, format=fmt, ratio_bits=[_bits(rect[2] / W), _bits(rect[3] / H)], kc=list(yc.TABLE[matrix]),
                         base=[p0, 0, 0], bytes=[pitch * (h - 1) + 4 * cw, 0, 0]), (c, g)
    for (c, want), g in zip(bad, got[len(ok):]):
        assert g == {"status": want}, (c, g)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------------

def test_pack_unpack_and_the_format_tables():
    assert (native.HT_YUV_YUYV, native.HT_YUV_UYVY) == (y4.YUYV, y4.UYVY) == (4, 5) and native.YUV_FORMATS["yuyv"] == 4 and native.YUV_FORMATS["uyvy"] == 5
    assert native.DRAW_LIST_FORMATS == dict(native.DRAW_FORMATS, yuyv=4, uyvy=5)
    for w, h in ((97, 81), (96, 5), (1, 3), (2, 2)):
        cw = y4.macropixels(w)
        rng = np.random.RandomState(w)
        y, u, v = rng.randint(0, 256, (h, w)).astype(np.uint8), rng.randint(0, 256, (h, cw)).astype(np.uint8), rng.randint(0, 256, (h, cw)).astype(np.uint8)
        for fmt in (y4.YUYV, y4.UYVY):
            fr = y4.pack(y, u, v, fmt)
            assert fr.shape == (h, 4 * cw) and fr.nbytes == y4.frame_bytes(w, h)
            for a, b in zip(y4.unpack(fr, w, h, fmt), (y, u, v)):
                assert np.array_equal(a, b)
        a, b = y4.pack(y, u, v, y4.YUYV).reshape(h, cw, 4), y4.pack(y, u, v, y4.UYVY).reshape(h, cw, 4)
        assert np.array_equal(a[..., [1, 0, 3, 2]], b)  # the same macropixels, bytes swapped in pairs
        assert np.array_equal(a[:, 0, 0], y[:, 0]) and np.array_equal(a[:, 0, 1], u[:, 0]) and np.array_equal(a[:, 0, 3], v[:, 0])
        if w & 1:  # the spare luma byte is never selected: any value gives the same picture
            other = y4.pack(y, u, v, y4.YUYV, spare=np.full(h, 9, dtype=np.uint8))
            assert not np.array_equal(other, y4.pack(y, u, v, y4.YUYV)) or h == 0
            assert np.array_equal(y4.to_rgba(other, w, h, y4.YUYV, 0), y4.to_rgba(y4.pack(y, u, v, y4.YUYV), w, h, y4.YUYV, 0))


@pytest.mark.parametrize("size", [(97, 81), (96, 80), (23, 23), (2, 2), (1, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_doubled_chroma_rows_are_the_i420_frame(size):
    """to_rgba(from_i420(p)) equals yuv_cases.to_rgba(p, I420) on odd and even sizes, all four matrices, both byte orders"""
    w, h = size
    p = yc.raw_noise(w, h, yc.I420, 11 + w)
    for matrix in range(4):
        want = yc.to_rgba(p, w, h, yc.I420, matrix)
        for fmt in (y4.YUYV, y4.UYVY):
            assert np.array_equal(y4.to_rgba(y4.from_i420(p, fmt), w, h, fmt, matrix), want)


def test_the_gpu_case_list_reaches_every_path_of_the_pixel_body():
    """counted from the restatement alone: column taps with a even / odd, b in the same / the next macropixel, taps on a rect's last column
    with that column even / odd, a case with one macropixel per row, a rect one pixel wide, canvases cut by the 64-column and the 16-row tile
    edge (the tile the packed draws take) and by the 4-row edge of the filtered draw's other tile; a noise frame that mostly clamps and a smooth frame that mostly does not (the bounds of tests/test_ingest_yuv_cpu.py)"""
    cnt = y4.sufficiency()
    for k, v in cnt.items():
        assert v > 0, (k, cnt)
    case = y4.CASES[0]
    assert y4.clamped_fraction(y4.raw_noise(case.w, case.h, y4.YUYV, 7), case.w, case.h, y4.YUYV, 0) >= 0.50
    smooth = y4.from_rgb_frames("smooth", case.w, case.h, 1, y4.UYVY, 1, seed=3)[0]
    assert y4.clamped_fraction(smooth, case.w, case.h, y4.UYVY, 1) <= 0.10
    assert {(c.w, c.h) for c in y4.CASES} >= {(97, 81), (23, 23), (333, 217), (2, 2), (1, 5), (2, 1)} and any(c.n == 3 and c.gap for c in y4.CASES)
    assert any(c.pitch_pad == 12 and c.base_off % 16 == 4 for c in y4.CASES)
    ex = y4.extremes(97, 81, y4.YUYV)
    yy, u, v = y4.unpack(ex, 97, 81, y4.YUYV)
    ix = np.arange(97) >> 1
    assert len(set(zip(yy.reshape(-1).tolist(), u[:, ix].reshape(-1).tolist(), v[:, ix].reshape(-1).tolist()))) == 216  # every triple of the six extreme values

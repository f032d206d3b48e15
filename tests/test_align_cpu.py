"""CPU-side checks of the angle-aligned face crops (ht_camshift_align_pairs_device / ht_camshift_align_sources_device): the quarter-wave
table and its generator; the rule in headtrackr_amd/csrc/ht_align_plan.h — the lines k_align_list compiles for the device — against the
Python restatement of tests/align_cases.py, range test and blend included, plain and under AddressSanitizer + UBSan, as a program of its
own; the restatement against the overlay's rotated box in binary64; the identity and quarter-turn properties; the scenes the GPU tests
track, proved from the oracle alone to cover what those tests claim; the entry points at every layer; the kernel's budget from
code-object metadata; the N-API shim against a recording stub; the JavaScript facade on the mock addon.  No compute calls (no GPU here)."""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import align_cases as al
import crop_cases as cr
import cs_cases as cc
import draw_list_cases as dl
import ingest_cases as ic
import yuv_cases as yc
from conftest import ROOT
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
EXPORTS = ("ht_camshift_align_pairs_device", "ht_camshift_align_sources_device", "ht_camshift_align_result", "ht_camshift_align_records_device")
N_RANDOM = 100000
NODE = shutil.which("node")
W, H = cr.CANVAS


# ---- the table ----------------------------------------------------------------------------------------------------------------------------

def _committed_table():
    text = open(os.path.join(CSRC, "ht_align_table.inc")).read()
    body = "\n".join(ln for ln in text.splitlines() if not ln.startswith("//"))
    return [int(v) for v in re.findall(r"-?\d+", body)]


def test_committed_table_is_the_formula_and_the_generator_reproduces_it(tmp_path):
    """ht_align_table.inc holds round(sin(k pi / 2048) 2^30) for k = 0 .. 1024 — the landmarks, the CRC-32 of the 1025 little-endian int32
    and every value of the restatement's own table (binary64 sin; the generator uses decimal arithmetic) —, is monotonic, and
    tools/gen_align_table.py writes the same bytes"""
    t = _committed_table()
    assert len(t) == 1025 and (t[0], t[1], t[512], t[1024]) == (0, 1647099, 759250125, 2 ** 30)
    assert zlib.crc32(struct.pack("<1025i", *t)) == al.TABLE_CRC == 3814055822
    assert t == al.table() and all(b > a for a, b in zip(t, t[1:]))
    out = tmp_path / "table.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_align_table.py"), str(out)])
    assert out.read_bytes() == open(os.path.join(CSRC, "ht_align_table.inc"), "rb").read()


# ---- the rule -----------------------------------------------------------------------------------------------------------------------------

def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("align_plan") / ("align_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "align_plan_harness.cc"), "-o", exe])
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
    """the edge table, the seeded random objects and the term subset, with the restatement's answer for each: computed once"""
    cs = al.edge_cases() + al.random_cases(N_RANDOM) + al.term_cases()
    want = []
    for c in cs:
        want += al.want_of(c)
    return cs, np.array(want, dtype=np.int64)


def test_edge_angles_cover_what_they_claim():
    """from the restatement alone: NaN, both infinities, +-1024 (a face) and the next binary64 / +-1024.5 (empty), 0, the quarter turns,
    a full turn, the smallest subnormal, and for several rounding boundaries the boundary and two neighbours on each side, among which
    a12 changes once, by exactly one step"""
    geo = (W, H, W, H, None, 256, 0)
    code = lambda a: al.plan((48, 40, 10, 10, a), *geo)[0]
    ang = al.edge_angles()
    assert any(a != a for a in ang) and float("inf") in ang and float("-inf") in ang and 5e-324 in ang
    assert code(1024.0) == code(-1024.0) == al.FACE and code(math.nextafter(1024.0, math.inf)) == code(1024.5) == code(-1024.5) == al.EMPTY
    assert code(float("nan")) == code(float("inf")) == code(float("-inf")) == al.EMPTY and code(5e-324) == al.FACE
    assert [al.a12_of(a) for a in (0.0, math.pi / 2, math.pi, -math.pi / 2, 2 * math.pi, 3 * math.pi / 2, 5e-324, -5e-324)] == [0, 1024, 2048, 3072, 0, 3072, 0, 0]
    b = al.boundary_angles()
    for k in range(0, len(b), 5):
        at, up, down, up2, down2 = b[k:k + 5]
        seq = [al.a12_of(x) for x in (down2, down, at, up, up2)]  # (the quotient that names the boundary is itself rounded: the step falls somewhere among the five)
        assert seq[4] == (seq[0] + 1) & 4095 and set(seq) == {seq[0], seq[4]} and seq == sorted(seq, key=lambda v: v != seq[0]), seq
    # the sine's four quadrants and the cosine's shift
    assert [al.sin_q30(a) for a in (0, 1024, 2048, 3072)] == [0, 2 ** 30, 0, -2 ** 30] and [al.cos_q30(a) for a in (0, 1024, 2048, 3072)] == [2 ** 30, 0, -2 ** 30, 0]
    assert all(abs(al.sin_q30(a) - math.sin(a * math.pi / 2048) * 2 ** 30) <= 0.5000001 for a in range(4096))


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_rule_header_equals_the_restatement(harness, harness_san, cases, tmp_path, which):
    """crop_cases.edge_cases()'s objects and geometries x the edge angles, 100 000 seeded random objects: every field of ht_align_rule's
    plan equals the restatement's; on the term subset (every edge geometry, 2 000 random cases, P and Q from {1, 19, 70, 112, 1024}) all
    P column terms and all Q row terms of both axes too"""
    cs, want = cases
    assert len(cs) >= N_RANDOM + 100000 and {c[15] for c in cs} >= set(al.TERM_SIZES) and {c[16] for c in cs} >= set(al.TERM_SIZES)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(al.pack_cases(cs))
    r = subprocess.run([harness if which == "plain" else harness_san, src, dst], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.int64)
    assert got.shape == want.shape
    if (got != want).any():
        pos = 0
        for c in cs:  # name the first case that differs
            n = 8 + (2 * c[15] + 2 * c[16] if c[15] > 0 else 0)
            assert (got[pos:pos + n] == want[pos:pos + n]).all(), (c, got[pos:pos + 8].tolist(), want[pos:pos + 8].tolist())
            pos += n
    nrec = len(cs) - len(al.term_cases())
    faces = int((want[:8 * nrec:8] == al.FACE).sum())
    assert 0.3 * nrec < faces < 0.9 * nrec  # no monoculture


@pytest.mark.parametrize("which", ["plain", "sanitized"])
def test_range_test_and_blend_of_the_header_equal_the_restatement(harness, harness_san, tmp_path, which):
    """step 8 as the kernel compiles it (ht_align_inside, ht_align_channel): 200 000 seeded samples around all four edges of seeded frames,
    with taps of extreme and random bytes: the inside flag and the blended dword equal Python integers'"""
    rng = np.random.RandomState(20265)
    n = 200000
    SW, SH = rng.randint(1, 16385, n), rng.randint(1, 16385, n)
    near = lambda size: np.where(rng.randint(2, size=n) == 0, -32768, size.astype(np.int64) * 65536 - 32768) + rng.randint(-3, 4, n) * np.where(rng.randint(2, size=n) == 0, 1, 4096)
    fx = np.where(rng.randint(3, size=n) == 0, near(SW), (rng.uniform(-0.6, 1.1, n) * SW * 65536).astype(np.int64))
    fy = np.where(rng.randint(3, size=n) == 0, near(SH), (rng.uniform(-0.6, 1.1, n) * SH * 65536).astype(np.int64))
    taps = rng.randint(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(np.uint32)
    taps[rng.randint(4, size=n) == 0] = 0xFFFFFFFF
    taps[::7, 1] = 0
    taps[::11, 2] = 0xFF00FF00
    rec = np.zeros(n, dtype=[("fx", "<i8"), ("fy", "<i8"), ("SW", "<i4"), ("SH", "<i4"), ("p", "<u4", 4)])
    rec["fx"], rec["fy"], rec["SW"], rec["SH"], rec["p"] = fx, fy, SW, SH, taps
    src, dst = str(tmp_path / "pix.bin"), str(tmp_path / "pix.out")
    rec.tofile(src)
    r = subprocess.run([harness if which == "plain" else harness_san, "--pixels", src, dst], capture_output=True, text=True, timeout=600, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    got = np.fromfile(dst, dtype=np.uint32).reshape(n, 2)
    inside = (fx >= -32768) & (fy >= -32768) & (fx < SW.astype(np.int64) * 65536 - 32768) & (fy < SH.astype(np.int64) * 65536 - 32768)
    tx, ty = (fx & 65535) >> 8, (fy & 65535) >> 8
    want = np.zeros(n, dtype=np.int64)
    for ch in range(4):
        p = [(taps[:, k].astype(np.int64) >> (8 * ch)) & 255 for k in range(4)]
        top, bot = p[0] * (256 - tx) + p[1] * tx, p[2] * (256 - tx) + p[3] * tx
        want |= ((top * (256 - ty) + bot * ty + 32768) >> 16) << (8 * ch)
    want = np.where(inside, want, 0)
    assert (got[:, 0] == inside).all() and (got[:, 1] == want).all()
    assert 0.2 * n < inside.sum() < 0.9 * n and ((got[:, 1] >> 24) == 255).any()


def test_the_rule_is_the_overlays_rotation():
    """From the restatement alone, in binary64.  For a corner pixel (i, j) of a P x Q patch let u = (2i + 1 - P) / 2P, v = (2j + 1 - Q) / 2Q;
    its sample position (fx + 32768, fy + 32768) / 65536 must lie within r pi / 4096 + 1 / 128 source pixels of the exact affine image of
    the point (u, v) of main.js's box: translate(cx, cy); rotate(angle - pi / 2); rect(-bw / 2, -bh / 2, bw, bh), the object floored as
    the rule's step 1 floors it, mapped through the mapping rect.

    The bound.  (a) The angle is rounded to the nearest of 4096 steps: it is off by at most half a step, pi / 4096 (the one rounding of
    angle * K is 2^-53 relative and disappears in the slack of (b)).  Turning a point at distance d from the centre by delta moves it by
    at most d delta on the canvas, and the mapping scales a canvas vector by at most s = max(mw / W, mh / H); d is at most the box's
    half-diagonal.  So r is the half-diagonal of the widened box on the canvas times s — for an isotropic mapping exactly the box's
    half-diagonal in source pixels, which is the r the pairs-form cases below are held to.  (For an anisotropic mapping the image is a
    parallelogram whose own half-diagonals can be SHORTER than the displacement of a corner, so the canvas half-diagonal times the larger
    scale is the r that makes the statement true.)  (b) Fixed point, per axis, in units of 2^-16 source pixel: Cx's floor 1; Ux's floor 1
    plus the table's rounding bw / 2^23 (<= 1 for bw <= 2^23), times s, plus UxS's floor 1, times |u| <= 1/2, plus the term's floor 1;
    the same for V: 1 + 2 (s + 1 / 2 + 1) = 2 s + 4.  With s <= 128: 260 units per axis, 368 units = 0.0056 < 1 / 128 in the plane.
    The cases are therefore the seeded random objects with s <= 128 and bw, bh <= 2^23 (most of them), and crop_cases' pairs geometry."""
    rng = np.random.RandomState(20264)
    checked = iso = 0
    cs = [c for c in al.random_cases(3000) if max((c[11] or c[7]) / c[5], (c[12] or c[8]) / c[6]) <= 128]
    cs += [(*o, a, W, H, W, H, 0, 0, W, H, m, fl, 0, 0) for o in ((48, 40, 10, 10), (47.25, 39.75, 18.7, 25.3), (5, 76, 30, 9), (96.9, 0.2, 3, 41))
           for a in (0.0, 0.3, math.pi / 2, 2.2, -1.1, 17.0) for (m, fl) in cr.CONFIGS]
    worst = 0.0
    for c in cs:
        obj, geo = c[:5], (c[5], c[6], c[7], c[8], c[9:13], c[13], c[14])
        pl = al.plan(obj, *geo)
        if pl[0] != al.FACE:
            continue
        w, h = cr.floor_i32(obj[2]), cr.floor_i32(obj[3])
        bw, bh = w * geo[5], h * geo[5]
        if geo[6] & al.SQUARE:
            bw = bh = max(bw, bh)
        if max(bw, bh) > 2 ** 23:
            continue
        mw, mh = (geo[4][2], geo[4][3]) if (geo[4][2] or geo[4][3]) else (geo[2], geo[3])
        s = max(mw / geo[0], mh / geo[1])
        r = math.hypot(bw / 512, bh / 512) * s
        P, Q = al.TERM_SIZES[rng.randint(5)], al.TERM_SIZES[rng.randint(5)]
        tu_x, tu_y, tv_x, tv_y = al.terms(P, pl[4]), al.terms(P, pl[5]), al.terms(Q, pl[6]), al.terms(Q, pl[7])
        for i in (0, P - 1):
            for j in (0, Q - 1):
                gx, gy = (pl[2] + tu_x[i] + tv_x[j]) / 65536, (pl[3] + tu_y[i] + tv_y[j]) / 65536
                ex, ey = al.overlay_point(obj, *geo, (2 * i + 1 - P) / (2 * P), (2 * j + 1 - Q) / (2 * Q))
                err = math.hypot(gx - ex, gy - ey)
                assert err <= r * math.pi / 4096 + 1 / 128, (c, P, Q, i, j, err, r)
                worst = max(worst, err - r * math.pi / 4096)
        checked += 1
        iso += mw == geo[0] and mh == geo[1]
    assert checked >= 2000 and iso >= 100, (checked, iso)


def _frame_source(frame):
    s = dl.Source(dl.RGBA, W, H, seed=1)
    s.rgba = frame
    return s


def test_identity_and_quarter_turn_on_the_pairs_scene():
    """from the restatement alone, on pairs_scene() frames (pairs form, margin 256): with angle = pi / 2, P = w, Q = h (multiples of 4, as
    camshift's << 2 makes them) every sample lies on a pixel centre of the block (cx - w / 2 .. , cy - h / 2 ..) with weights 0: the patch
    is the block itself, zeros where it leaves the frame.  At a12 = 2048 (angle = pi) and a12 = 0 the patch is the exact quarter turn of
    the h x w block: patch(i, j) = block pixel (cx + h / 2 - 1 - j, cy - w / 2 + i), and the other way round."""
    a, b = cr.pairs_scene()
    boxes = [(20, 16, 12, 8), (48, 40, 8, 28), (4, 78, 16, 12), (95, 3, 8, 8), (60, 30, 4, 4)]  # two of them leave the frame
    left_frame = 0
    for frame in (a.frames[1], b.frames[1]):
        src = _frame_source(frame)
        padded = np.zeros((H + 200, W + 200, 4), dtype=np.uint8)
        padded[100:100 + H, 100:100 + W] = frame
        for (cx, cy, w, h) in boxes:
            block = padded[100 + cy - h // 2:100 + cy + h // 2, 100 + cx - w // 2:100 + cx + w // 2]
            got = al.patch(src, (cx + 0.75, cy + 0.25, w + 0.5, h, math.pi / 2), W, H, None, 256, 0, w, h)
            assert got.shape == block.shape and (got == block).all(), (cx, cy, w, h)
            left_frame += bool((block[..., 3] == 0).any())
            pl = al.plan((cx, cy, w, h, math.pi / 2), W, H, W, H, None, 256, 0)
            fx, fy = al.sample_positions(pl, w, h)
            assert (fx == (cx - w // 2 + np.arange(w))[None, :] * 65536).all() and (fy == (cy - h // 2 + np.arange(h))[:, None] * 65536).all()
            # a quarter turn further (a12 = 2048): patch +x is the canvas's +y, patch +y is the canvas's -x; P = w, Q = h samples an h x w block
            blk = padded[100 + cy - w // 2:100 + cy + w // 2, 100 + cx - h // 2:100 + cx + h // 2]
            got = al.patch(src, (cx, cy, w, h, math.pi), W, H, None, 256, 0, w, h)
            assert al.a12_of(math.pi) == 2048 and (got == np.rot90(blk, 1)).all(), (cx, cy, w, h)
            got = al.patch(src, (cx, cy, w, h, 0.0), W, H, None, 256, 0, w, h)
            assert (got == np.rot90(blk, -1)).all(), (cx, cy, w, h)
    assert left_frame >= 2


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------------------------------

def test_the_gpu_tests_inputs_suffice():
    """from the oracle alone: the pairs list holds EMPTY entries; the oracle's angles quantise to a12 on both sides of 1024 (upright), and
    to exactly 2048 on the strip feeds; at margin 256 entries exist whose every pixel is inside the source, and at margin 1024 with square
    entries with pixels on both sides of step 8's test; every angle is further than 0.01 of a step from a rounding boundary, so that a
    last-bit difference in `angle` cannot move a12 — except through camshift's own wrap at the two strip feeds, where the reference
    itself has two steps (below)"""
    a, b = cr.pairs_scene()
    seqs = (a, b)
    step1 = {s: seqs[q].oracle_calls(j)[0][2] for (s, _f, q, j) in cr.pairs_trackers()}
    step2 = {s: seqs[q].oracle_calls(j)[1][2] for (s, _f, q, j) in cr.pairs_trackers()}
    feeds, fobjs = cr.feeds(), cr.feed_objects()
    angles = [to["angle"] for to in list(step1.values()) + list(step2.values()) + fobjs]
    assert all(al.boundary_distance(x) > 0.01 for x in angles), [al.boundary_distance(x) for x in angles]
    a12 = [al.a12_of(to["angle"]) for to in step1.values()]
    assert min(a12) < 1024 < max(a12), a12
    fa12 = [al.a12_of(to["angle"]) for to in fobjs]
    assert fa12 == [689, 1015, 1396, 976, 1347, 2048, 2048] and min(fa12) < 1024 < max(fa12)
    # the wrap of camshift.js:244 (angle < 0: + pi) is a discontinuity too.  The two strip feeds' blobs are horizontal to rounding: the
    # oracle under its own summation-order variants returns pi - 5e-14 (2048) or 2e-14 (0) there, so both steps are the reference's;
    # every other angle of the scenes is the same step under every order and nowhere near the wrap
    assert [al.at_wrap(x) for x in angles] == [False] * (len(angles) - 2) + [True, True] and all(1e-3 < x < math.pi - 1e-3 for x in angles[:-2])  # (a million times the last-bit residues)
    seen = [{v} for v in fa12]
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            cr.feed_objects.cache_clear()
            alt = cr.feed_objects()
        cr.feed_objects.cache_clear()
        assert [cr.obj_of(t) for t in alt] == [cr.obj_of(t) for t in fobjs], flag
        for k, t in enumerate(alt):
            seen[k].add(al.a12_of(t["angle"]))
    assert seen == [al.admissible_a12(to["angle"]) for to in fobjs] and seen[5] == seen[6] == {0, 2048}, seen
    crop_list = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]
    codes = [al.plan(al.obj_of(step1[s]) if s in step1 else al.NO_OBJECT, W, H, W, H, None, 256, 0)[0] for s, _f in crop_list]
    assert codes == [al.FACE, al.EMPTY, al.FACE, al.FACE, al.EMPTY, al.FACE]
    for P, Q in ((70, 19), (24, 24)):
        tight = [al.inside_mask(al.plan(al.obj_of(to), W, H, s.w, s.h, m, 256, 0), P, Q, s.w, s.h).mean() for (s, m), to in zip(feeds, fobjs)]
        wide = [al.inside_mask(al.plan(al.obj_of(to), W, H, s.w, s.h, m, 1024, al.SQUARE), P, Q, s.w, s.h).mean() for (s, m), to in zip(feeds, fobjs)]
        assert sum(t == 1.0 for t in tight) >= 5 and all(0.05 < v < 0.95 for v in wide), (tight, wide)
    wide = [al.inside_mask(al.plan(al.obj_of(to), W, H, W, H, None, 1024, al.SQUARE), 70, 19, W, H).mean() for to in step1.values()]
    assert sum(0.05 < v < 0.95 for v in wide) >= 2, wide  # the two blobs near the corners; the one in the middle stays inside


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------

def test_entry_points_exist_at_every_layer_and_refuse_malformed_calls_without_a_device(tmp_path):
    """fails without the feature: the header, the library, native.py, the API and INTEGRATION.md all name the four exports;
    ht_align_record is 64 bytes with the same field offsets in C (a program compiled against the header), in ctypes and in numpy; the ABI
    version stays 2; the C ABI answers all-zero arguments with a status"""
    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS and f"| `{name}` |" in doc[doc.index("## 6. Every export"):], name
    assert "typedef struct ht_align_params" in header and "typedef struct ht_align_record" in header and "#define HT_ABI_VERSION 2" in header
    assert "enum { HT_ALIGN_EMPTY = 0, HT_ALIGN_FACE = 1 };" in header and "enum { HT_ALIGN_SQUARE = 1 };" in header
    fields = ("code", "stream", "a12", "pad", "cx", "cy", "ux", "uy", "vx", "vy")
    offsets = [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    prog = tmp_path / "offsets.c"
    prog.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "headtrackr_hip.h"\nint main(void) { printf("%zu %zu", sizeof(ht_align_record), sizeof(ht_align_params));\n'
                    + "".join('printf(" %%zu", offsetof(ht_align_record, %s));\n' % f for f in fields) + "return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(tmp_path / "offsets")])
    assert [int(v) for v in subprocess.check_output([str(tmp_path / "offsets")], text=True).split()] == [64, 16] + offsets
    assert C.sizeof(native.ALIGN_RECORD) == native.ALIGN_RECORD_DTYPE.itemsize == 64 and C.sizeof(native.ALIGN_PARAMS) == 16
    assert [getattr(native.ALIGN_RECORD, f).offset for f in fields] == offsets == [native.ALIGN_RECORD_DTYPE.fields[f][1] for f in fields]
    assert (native.HT_ALIGN_EMPTY, native.HT_ALIGN_FACE, native.HT_ALIGN_SQUARE) == (al.EMPTY, al.FACE, al.SQUARE) == (0, 1, 1)
    assert L.ht_camshift_align_pairs_device(None, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_sources_device(None, None, None, 0, None, None, 0) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_result(None, 0, None) == native.HT_ERR_INVALID
    assert L.ht_camshift_align_records_device(None, None, None) == native.HT_ERR_INVALID
    prm, src = native.ALIGN_PARAMS(7, 3, 256, 0), (native.DRAW_SOURCE * 1)()
    assert L.ht_camshift_align_sources_device(None, None, src, 1, C.byref(prm), None, 0) == native.HT_ERR_INVALID  # no context: a status, never a crash
    assert L.ht_abi_version() == 2
    for m in ("camshift_align_pairs_device", "camshift_align_sources_device", "camshift_align_result", "camshift_align_records_ptr"):
        assert callable(getattr(Context, m)), m


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------

def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_align_kernel_fits_its_budget_and_lives_in_the_ingest_code_object():
    """code-object METADATA only: k_align_list (the fused form: no resolve kernel) has no spills, no scratch, <= 64 VGPRs like its
    siblings and <= 4096 B of LDS; no kernel but k_crop_list carries `crop` in its name; the library still holds four gfx950 code objects,
    the kernel lives in the one that holds k_draw_list and k_crop_list, and the three fingerprinted units are byte-identical to
    profiles/traffic.json's build; the rule header is host AND device text without HIP, integer-only behind its floors and the one
    multiplication"""
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    r = res["k_align_list"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] <= 4096, r
    assert [k for k in res if "crop" in k] == ["k_crop_list"] and [k for k in res if "align" in k] == ["k_align_list"]
    for marker in fingerprint.UNITS.values():
        assert marker.decode() not in "k_align_list"
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    home = [o for o in objs if b"k_align_list" in o]
    assert len(home) == 1 and b"k_draw_list" in home[0] and b"k_crop_list" in home[0]
    family = ("ht_crop.hip", "ht_align.hip", "ht_patch.hip", "ht_filter.hip", "ht_face_calls.hip", "ht_list_parts.inc")
    text = {f: open(os.path.join(CSRC, f)).read() for f in ("ht_ingest.hip", "ht_align_plan.h") + family}
    whole = "".join(text[f] for f in family)
    assert text["ht_ingest.hip"].index('#include "ht_crop.hip"') < text["ht_ingest.hip"].index('#include "ht_align.hip"')
    assert whole.count("ht_align_rule(") == 1 and "ht_align_rule(" in text["ht_list_parts.inc"] and whole.count("#define LP_PART 2  // LP_UPRIGHT_HEAD") == 3  # the upright head, once
    assert whole.count("ht_draw_list_plan_entry(") == 1 and "ht_draw_list_plan_entry(" in text["ht_face_calls.hip"]  # the draw list's plan is asked, not restated: once for both families
    assert "_reserve(" not in text["ht_align.hip"] and "extern" not in text["ht_align.hip"] and "hipMalloc" not in text["ht_align.hip"]  # no copy of the crop calls' host path
    plan = text["ht_align_plan.h"]
    assert "hip/" not in plan and "__global__" not in plan and "<math" not in plan and "<cmath" not in plan and plan.count("ht_csb_floor_i32(") == 5  # five floors
    body = plan.split("HT_ALIGN_FN int32_t ht_align_rule(")[1].split(") {", 1)[1].split("\n}\n", 1)[0]
    assert "double" not in body and body.count("ht_csb_floor_i32(") == 4 and "ht_align_a12(angle)" in body
    a12 = plan.split("HT_ALIGN_FN int32_t ht_align_a12(double angle) {")[1].split("\n}\n", 1)[0]
    assert a12.count("*") == 1 and a12.count("ht_csb_floor_i32(") == 1  # ONE binary64 multiplication


# ---- the N-API shim against the recording stub --------------------------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_shim_passes_arguments_to_the_c_abi_and_refuses_malformed_calls(tmp_path):
    """csrc/ht_napi.cc built with tests/js/abi_stub.cc, crop_stub.cc and align_stub.cc: the successful calls of tests/js/align_addon.js
    reach the C ABI with the pairs, the streams, the entries' plane layout, the params, the output offset and stride; alignResult unpacks
    the 64-byte records (the int64 terms exactly, as binary64); every malformed call throws before the C ABI is reached — through the
    shim's one argument reader and range check, so with the crop calls' kinds —, and a refusal of the library comes back as an Error"""
    addon = str(tmp_path / "addon_align.node")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", "/usr/include/node", "-I", os.path.join(ROOT, "include"), "-DNAPI_VERSION=7",
                           "-DNODE_GYP_MODULE_NAME=headtrackr_hip", os.path.join(CSRC, "ht_napi.cc"), os.path.join(ROOT, "tests", "js", "abi_stub.cc"),
                           os.path.join(ROOT, "tests", "js", "crop_stub.cc"), os.path.join(ROOT, "tests", "js", "align_stub.cc"), "-o", addon])
    log = str(tmp_path / "align.log")
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "align_addon.js"), addon], capture_output=True, text=True, timeout=120, env=dict(os.environ, HT_ALIGN_STUB_LOG=log))
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
    assert calls[3] == dict(fn="sources", ctx=True, n=4, streams=[1, 0, 7, 7], params=[7, 3, 1024, 1], stride=pb + 4,
                            entries=[dict(E_I420, p0=54000 - 12), dict(E_NV12, p0=51001 - 12), dict(E_RGBA, p0=50000 - 12), dict(E_RGBA, p0=50000 - 12)])
    res = out["result"]
    assert res["kinds"] == ["Int32Array", "Float64Array"]
    assert res["records"] == [v for i in range(4) for v in (i & 1, 10 + i, 100 * i, 0)]
    assert res["terms"] == [float((2 ** 40 + 7 * i + k) * (-1 if k & 1 else 1)) for i in range(4) for k in range(6)]
    thrown = dict(out["thrown"])
    assert all(v is not None for v in thrown.values()), [k for k, v in thrown.items() if v is None]
    refused = {k: thrown.pop(k) for k in list(thrown) if k.endswith("the library refuses")}
    assert len(calls) == 6 and calls[4]["n"] == 3 and calls[5]["n"] == 3  # the only two further calls that reach the C ABI: the stub refuses n == 3
    assert "ht_camshift_align_pairs_device: status -1" in refused["pairs: the library refuses"] and "ht_camshift_align_sources_device: status -1" in refused["sources: the library refuses"]
    assert "ht_camshift_align_result: status -6" in refused["result: the library refuses"]
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
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    assert {"alignPairsDevice", "alignSourcesDevice", "alignResult"} <= set(re.findall(r'\{"(\w+)",\s*\w+\}', napi)) and '{"ALIGN_SQUARE", HT_ALIGN_SQUARE}' in napi
    assert napi.count("get_crop_out(a, ") == 1 and napi.count("get_draw_entry(env, e, &srcs[i])") == 2  # the one argument reader and range check, read in ONE place for every launching call


# ---- the JavaScript facade on the mock addon ----------------------------------------------------------------------------------------------------

JS_CONFIGS = [dict(width=70, height=19, margin=1.0, square=False), dict(width=1, height=1, margin=0.25, square=True), dict(width=24, height=24, margin=4.0, square=True),
              dict(width=24, height=24, margin=4.0, square=False)]


def _expect(entries, cfg):
    """entries: [(source, track object or None, mapping, stream)] -> (crcs, records, terms) of one align call"""
    m, fl, P, Q = int(round(cfg["margin"] * 256)), int(cfg["square"]), cfg["width"], cfg["height"]
    crcs, recs, terms = [], [], []
    for src, to, mapping, stream in entries:
        obj = al.obj_of(to) if to else al.NO_OBJECT
        crcs.append(ic.crc(al.patch(src, obj, W, H, mapping, m, fl, P, Q)))
        r = al.record(stream, obj, W, H, src.w, src.h, mapping, m, fl)
        recs += list(r[:4])
        terms += [float(v) for v in r[4:]]
    return crcs, recs, terms


@pytest.mark.skipif(NODE is None, reason="node is not installed")
def test_facade_aligns_pairs_and_feeds_through_the_align_entry_points(tmp_path):
    """tests/js/align_cpu.js on tests/js/mock_addon_align.js: alignPairs behind an enqueue-only track step and alignFeeds on mixed
    opts.sources give the patches (CRC-32), records and terms of the restatement on the oracle's objects, through the align entry points
    alone; malformed calls throw; an addon without the calls gives the rebuild-it error"""
    if not os.path.exists("/usr/include/node/node_api.h"):
        pytest.skip("node_api.h is not installed: the oracle addon of the mock cannot be built")
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    a, b = cr.pairs_scene()
    seqs, trackers = (a, b), cr.pairs_trackers()
    np.stack([a.frames[0], b.frames[0]]).tofile(tmp_path / "init.raw")
    np.stack([a.frames[1], b.frames[1]]).tofile(tmp_path / "step.raw")
    init_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)] + [cr.NEVER_TRACKED, 1]
    rects = [v for (_s, _f, q, j) in trackers for v in seqs[q].rects[j]] + list(b.rects[0])
    track_pairs = [v for (s, f, _q, _j) in trackers for v in (s, f)]
    align_list = [(5, 0), (cr.NEVER_TRACKED, 1), (0, 0), (2, 1), (3, 0), (5, 0)]  # a stream that was never tracked, one never initialised, one twice
    objs = {s: seqs[q].oracle_calls(j)[0][2] for (s, _f, q, j) in trackers}
    frame_src = [_frame_source(seqs[q].frames[1]) for q in (0, 1)]
    job = dict(w=W, h=H, configs=JS_CONFIGS,
               pairs=dict(init=str(tmp_path / "init.raw"), step=str(tmp_path / "step.raw"), trackers=cr.RESERVED, init_pairs=init_pairs, rects=[int(v) for v in rects],
                          track_pairs=track_pairs, align_pairs=[v for p in align_list for v in p]))
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
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "align_cpu.js"), str(tmp_path / "job.json")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert len(out["pairs"]) == len(out["feeds"]) == len(JS_CONFIGS)
    for cfg, gp, gf in zip(JS_CONFIGS, out["pairs"], out["feeds"]):
        crcs, recs, terms = _expect([(frame_src[f], objs.get(s), None, s) for (s, f) in align_list], cfg)
        assert (gp["crc"], gp["records"], gp["terms"]) == (crcs, recs, terms), (cfg, gp)
        assert gp["n"] == len(align_list) and gp["size"] == [cfg["width"], cfg["height"]] and gp["bytes"] == len(align_list) * cfg["width"] * cfg["height"] * 4
        crcs, recs, terms = _expect([(src, to, m, st) for (src, m), to, st in zip(feeds, fobjs, streams)], cfg)
        assert (gf["crc"], gf["records"], gf["terms"]) == (crcs, recs, terms), (cfg, gf)
    # the enqueue-only track step was collected AFTER the align calls and is the oracle's
    got = np.array(out["track"]).reshape(-1, 9)
    for row, (s, _f, _q, _j) in zip(got, trackers):
        assert tuple(row[:4]) == cr.obj_of(objs[s])
    assert out["refusals"] == 14 + 5
    facade = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("this.alignPairs = ", "this.alignFeeds = ", "this.alignResult = "):
        assert m in facade, m

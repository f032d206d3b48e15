"""Inputs and expectations of the angle-aligned face crops (ht_camshift_align_pairs_device / ht_camshift_align_sources_device), shared by
tests/test_align_cpu.py and tests/test_gpu_align.py.  `plan`, `terms` and `patch` restate the rule in Python integers (written from the
rule's description, not from headtrackr_amd/csrc/ht_align_plan.h); sources, scenes and oracle track objects are crop_cases'; the expected
patch is the restatement on Source.rgba, the source's declared RGBA view.  Nothing here comes from the code under test."""
import functools
import math
import struct
import zlib

import numpy as np

import crop_cases as cr

EMPTY, FACE = 0, 1
SQUARE = 1
K = float.fromhex("0x1.45f306dc9c883p+10")  # the binary64 nearest to 8192 / (2 pi): half steps per radian
assert K == 1303.7972938088067 and abs(K - 8192 / (2 * math.pi)) < 1e-12
TABLE_CRC = 3814055822


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def table():
    """T[k] = round(sin(k pi / 2048) * 2^30), k = 0 .. 1024.  binary64 sin is within an ulp, far from every rounding boundary but for a
    handful of entries the CRC would expose: the CRC of the description pins the result."""
    t = [int(round(math.sin(k * math.pi / 2048) * 2 ** 30)) for k in range(1025)]
    assert zlib.crc32(struct.pack("<1025i", *t)) == TABLE_CRC and (t[0], t[1], t[512], t[1024]) == (0, 1647099, 759250125, 2 ** 30)
    return t


def sin_q30(a):
    q, r = a >> 10, a & 1023
    T = table()
    return (T[r], T[1024 - r], -T[r], -T[1024 - r])[q]


def cos_q30(a):
    return sin_q30((a + 1024) & 4095)


def a12_of(angle):
    """the angle rounded to the nearest of 4096 steps per turn (ONE binary64 multiplication, a floor, integers)"""
    t = cr.floor_i32(angle * K)
    return ((t + 1) >> 1) & 4095


def boundary_distance(angle):
    """how far angle * K is from the nearest point where a12 changes (an odd number of half steps), in STEPS"""
    h = angle * K
    return abs(h - (2 * math.floor(h / 2) + 1)) / 2


def plan(obj, W, H, SW, SH, mapping, margin_q8, flags):
    """obj = (x, y, width, height, angle) -> (code, a12, Cx, Cy, UxS, UyS, VxS, VyS); Python's // and >> round towards -inf"""
    mx, my, mw, mh = mapping if mapping is not None and (mapping[2] or mapping[3]) else (0, 0, SW, SH)
    cx, cy, w, h = (cr.floor_i32(v) for v in obj[:4])
    angle = obj[4]
    empty = (EMPTY, 0, 0, 0, 0, 0, 0, 0)
    if w <= 0 or h <= 0 or w > 65536 or h > 65536 or abs(cx) > 2 ** 20 or abs(cy) > 2 ** 20:
        return empty
    if angle != angle or math.isinf(angle) or abs(angle) > 1024:
        return empty
    a = a12_of(angle)
    S, C = sin_q30(a), cos_q30(a)
    bw, bh = w * margin_q8, h * margin_q8
    if flags & SQUARE:
        bw = bh = max(bw, bh)
    Ux, Uy, Vx, Vy = (bw * S) >> 22, (-bw * C) >> 22, (bh * C) >> 22, (bh * S) >> 22
    return (FACE, a, mx * 65536 + (cx * 65536 * mw) // W, my * 65536 + (cy * 65536 * mh) // H, (Ux * mw) // W, (Uy * mh) // H, (Vx * mw) // W, (Vy * mh) // H)


def terms(P, v):
    """the P column (or row) terms of one axis: floor((2 i + 1 - P) v / 2 P)"""
    return [((2 * i + 1 - P) * v) // (2 * P) for i in range(P)]


def sample_positions(pl, P, Q):
    """(fx [Q, P], fy [Q, P]) int64 of a FACE plan"""
    _c, _a, Cx, Cy, UxS, UyS, VxS, VyS = pl
    fx = Cx - 32768 + np.array(terms(P, UxS), dtype=np.int64)[None, :] + np.array(terms(Q, VxS), dtype=np.int64)[:, None]
    fy = Cy - 32768 + np.array(terms(P, UyS), dtype=np.int64)[None, :] + np.array(terms(Q, VyS), dtype=np.int64)[:, None]
    return fx, fy


def inside_mask(pl, P, Q, SW, SH):
    fx, fy = sample_positions(pl, P, Q)
    return (fx >= -32768) & (fy >= -32768) & (fx < SW * 65536 - 32768) & (fy < SH * 65536 - 32768)


def sample(rgba, pl, P, Q):
    """the patch uint8 [Q, P, 4] of a FACE plan on an RGBA view uint8 [SH, SW, 4]"""
    SH, SW = rgba.shape[:2]
    fx, fy = sample_positions(pl, P, Q)
    ok = (fx >= -32768) & (fy >= -32768) & (fx < SW * 65536 - 32768) & (fy < SH * 65536 - 32768)
    fx, fy = np.where(ok, fx, 0), np.where(ok, fy, 0)
    xi, yi, tx, ty = fx >> 16, fy >> 16, ((fx & 65535) >> 8)[..., None], ((fy & 65535) >> 8)[..., None]
    xa, xb, ya, yb = np.clip(xi, 0, SW - 1), np.clip(xi + 1, 0, SW - 1), np.clip(yi, 0, SH - 1), np.clip(yi + 1, 0, SH - 1)
    src = rgba.astype(np.int64)
    top = src[ya, xa] * (256 - tx) + src[ya, xb] * tx
    bot = src[yb, xa] * (256 - tx) + src[yb, xb] * tx
    out = (top * (256 - ty) + bot * ty + 32768) >> 16
    return np.where(ok[..., None], out, 0).astype(np.uint8)


def patch(source, obj, W, H, mapping, margin_q8, flags, P, Q):
    """the expected patch uint8 [Q, P, 4] of a dl.Source under the rule: zeros when empty"""
    pl = plan(obj, W, H, source.w, source.h, mapping, margin_q8, flags)
    return sample(source.rgba, pl, P, Q) if pl[0] == FACE else np.zeros((Q, P, 4), dtype=np.uint8)


def record(stream, obj, W, H, SW, SH, mapping, margin_q8, flags):
    """the 64-byte record of an entry as a tuple (code, stream, a12, pad, cx, cy, ux, uy, vx, vy)"""
    pl = plan(obj, W, H, SW, SH, mapping, margin_q8, flags)
    return (pl[0], stream, pl[1], 0, *pl[2:])


def obj_of(to):
    return (to["x"], to["y"], to["width"], to["height"], to["angle"])


# camshift.js:244 wraps a negative angle by + pi.  For a blob whose long axis is horizontal to rounding, atan2's first argument is a rounding
# residue of either sign: the reference's own angle is then 0 + or pi - a few 1e-14, depending on the summation order
# (tests/test_align_cpu.py shows both from the oracle's declared order variants, on the two strip feeds and nowhere else).  Such an angle
# has TWO admissible steps, 0 and 2048; every other angle has the one it rounds to.
WRAP_EPS = 1e-9


def at_wrap(angle):
    return abs(angle) < WRAP_EPS or abs(angle - math.pi) < WRAP_EPS


def admissible_a12(angle):
    """the steps the reference's angle may quantise to"""
    return {0, 2048} if at_wrap(angle) else {a12_of(angle)}


def obj_tracked(to, tracked_angle):
    """the oracle's track object as the expectation uses it: at the wrap the angle is 0 or pi, whichever of the two admissible steps the
    tracked angle rounds to; everywhere else the oracle's own"""
    a = to["angle"]
    if at_wrap(a):
        assert a12_of(tracked_angle) in (0, 2048), tracked_angle
        a = 0.0 if a12_of(tracked_angle) == 0 else math.pi
    return (to["x"], to["y"], to["width"], to["height"], a)


NO_OBJECT = (0.0, 0.0, 0.0, 0.0, 0.0)  # a stream that was never tracked: the state's zeros


# ---- the harness cases of the CPU test --------------------------------------------------------------------------------------------------------
# (x, y, width, height, angle, W, H, SW, SH, mx, my, mw, mh, margin_q8, flags, P, Q); P == 0: the record only

CASE = struct.Struct("<5d9iI2i")  # 88 bytes: tests/host/align_plan_harness.cc
assert CASE.size == 88


def pack_cases(cases):
    return b"".join(CASE.pack(*[float(v) for v in c[:5]], *[int(v) for v in c[5:17]]) for c in cases)


def want_of(case):
    """the int64 words the harness writes for a case: code, a12, the six terms; then, if P > 0, P column terms of x, P of y, Q row terms of x, Q of y"""
    pl = plan(case[:5], case[5], case[6], case[7], case[8], case[9:13], case[13], case[14])
    out = list(pl)
    P, Q = case[15], case[16]
    if P > 0:
        out += terms(P, pl[4]) + terms(P, pl[5]) + terms(Q, pl[6]) + terms(Q, pl[7])
    return out


def boundary_angles():
    """angles on a rounding boundary of a12 (an odd number of half steps) and their binary64 neighbours on both sides"""
    out = []
    for m in (1, 700, -300, 4096 * 3 + 17):
        b = (2 * m - 1) / K
        out += [b, math.nextafter(b, math.inf), math.nextafter(b, -math.inf), math.nextafter(math.nextafter(b, math.inf), math.inf),
                math.nextafter(math.nextafter(b, -math.inf), -math.inf)]
    return out


def edge_angles():
    nan, inf = float("nan"), float("inf")
    return [nan, inf, -inf, 1024.0, -1024.0, 1024.5, -1024.5, math.nextafter(1024.0, inf), 0.0, -0.0, math.pi / 2, math.pi, -math.pi / 2, 2 * math.pi, 5e-324, -5e-324,
            1.0, -1.0, 3 * math.pi / 2, 1023.99] + boundary_angles()


def edge_cases():
    """crop_cases.edge_cases()'s objects and geometries (every margin and flag) x the edge angles"""
    return [(*c[:4], a, *c[4:14], 0, 0) for c in cr.edge_cases() for a in edge_angles()]


def random_cases(n, seed=20262):
    """crop_cases.random_cases' objects and geometries with seeded angles: mostly within two turns, some far out, some beyond the bound"""
    rng = np.random.RandomState(seed)
    out = []
    for c in cr.random_cases(n):
        kind = rng.randint(16)
        a = float(rng.uniform(-2 * math.pi, 2 * math.pi)) if kind < 13 else float(rng.uniform(-1024, 1024)) if kind < 15 else float(rng.uniform(-1100, 1100))
        out.append((*c[:4], a, *c[4:14], 0, 0))
    return out


TERM_SIZES = (1, 19, 70, 112, 1024)


def term_cases(n_random=2000, seed=20263):
    """the subset whose column and row terms are compared too: every edge geometry with boxes small and huge at several angles, and
    n_random of the random cases; P and Q from TERM_SIZES"""
    rng = np.random.RandomState(seed)
    geoms = sorted({c[4:12] for c in cr.edge_cases()})
    out = []
    for g in geoms:
        for o in ((48, 40, 10, 10), (47.25, 39.75, 18.7, 25.3), (2 ** 20, -2 ** 20, 65536, 65536), (-5, -7, 1, 30), (300, 200, 64, 48)):
            for a in (0.0, math.pi / 2, 0.9, -2.5, 1024.0):
                for (m, fl) in ((64, 0), (256, SQUARE), (1024, SQUARE), (1023, 0)):
                    out.append((*o, a, *g, m, fl, TERM_SIZES[rng.randint(5)], TERM_SIZES[rng.randint(5)]))
    for c in random_cases(n_random, seed=seed + 1):
        out.append((*c[:15], TERM_SIZES[rng.randint(5)], TERM_SIZES[rng.randint(5)]))
    return out


# ---- the overlay's box, in binary64 -------------------------------------------------------------------------------------------------------------

def overlay_point(obj, W, H, SW, SH, mapping, margin_q8, flags, u, v):
    """the exact affine image, in source pixels (continuous: pixel k covers [k, k + 1)), of the point at fractions (u, v) in -1/2 .. 1/2 of
    main.js's box translate(cx, cy); rotate(angle - pi / 2); rect(-bw / 2, -bh / 2, bw, bh) — the object floored as the rule floors it,
    the angle exact"""
    mx, my, mw, mh = mapping if mapping is not None and (mapping[2] or mapping[3]) else (0, 0, SW, SH)
    cx, cy, w, h = (cr.floor_i32(t) for t in obj[:4])
    bw, bh = w * margin_q8 / 256, h * margin_q8 / 256
    if flags & SQUARE:
        bw = bh = max(bw, bh)
    rot = obj[4] - math.pi / 2  # canvas rotate(): x' = x cos - y sin, y' = x sin + y cos
    lx, ly = u * bw, v * bh
    px, py = cx + lx * math.cos(rot) - ly * math.sin(rot), cy + lx * math.sin(rot) + ly * math.cos(rot)
    return mx + px * mw / W, my + py * mh / H

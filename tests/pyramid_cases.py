"""The whole pyramid restated in numpy binary64, and frames built to sit on its rounding boundaries (tests/test_pyramid_cases_cpu.py,
tests/test_gpu_pyramid_ties.py).  A plain module, imported like tests/cs_cases.py.  Nothing here runs the library.

Restatement.  The declared resampler (oracle/canvas_shim.js, head of headtrackr_amd/csrc/ht_pyramid.hip) is centre-aligned bilinear in
binary64 with a round-half-to-even store; taps as ht_host_tap / rs_tap, jobs as ht_plan_jobs (headtrackr_amd/csrc/ht_geometry_plan.h).
Every arithmetic step below is a numpy operation of its own, so nothing is fused.  pyramid() takes the level sizes as an argument: what
ht_set_geometry(level_dims) is given, or ccv_dims() for ccv's own.

Boundary frames.  The kernels evaluate a pixel in binary32 and fall back to the binary64 sequence only when the estimate lies within
RS_EPS = 2^-13 of a boundary k + 0.5.  On noise 2.5e-4 of the pixels lie there.  place_job() chooses the four source bytes of every
other destination pixel of a job (their 2x2 footprints are disjoint for ratios >= 1) so that the DECLARED value lies at a chosen signed
distance d in [-2 RS_EPS, 2 RS_EPS] from a boundary, a share of them at d = 0 exactly.  plane_stats() says what a plane's values then
look like, and model32() is a binary32 estimate WITHOUT any fallback: the number of pixels it gets wrong is the number of pixels at which a
kernel with a broken fallback would show."""
import functools
import math
import os
import re
import zlib

import numpy as np

RS_EPS = 2.0 ** -13
TIE_CANDIDATES = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")


# ---- the declared resampler -----------------------------------------------------------------------------------------------------------

def taps(d, s):
    """(a, b, t, u) of destination samples 0 .. d-1 over s source samples, and whether the coordinate was clamped"""
    r = np.float64(s) / np.float64(d)
    f = (np.arange(d, dtype=np.float64) + 0.5) * r
    f = f + (-0.5)
    clamped = (f < 0.0) | (f > float(s - 1))
    f = np.where(f < 0.0, 0.0, f)
    f = np.where(f > float(s - 1), float(s - 1), f)
    af = np.floor(f)
    a = af.astype(np.int64)
    b = np.minimum(a + 1, s - 1)
    t = f - af
    u = 1.0 - t
    return a, b, t, u, clamped


def declared_values(src, sx, sy, sw, sh, dw, dh):
    """v of every pixel of one drawImage call: source rect (sx, sy, sw, sh) of plane src onto dw x dh; binary64, before the store"""
    ax, bx, tx, ux, _ = taps(dw, sw)
    ay, by, ty, uy, _ = taps(dh, sh)
    p = src.astype(np.float64)
    ra, rb = p[sy + ay], p[sy + by]
    top = ra[:, sx + ax] * ux
    top = top + ra[:, sx + bx] * tx
    bot = rb[:, sx + ax] * ux
    bot = bot + rb[:, sx + bx] * tx
    v = top * uy[:, None]
    v = v + bot * ty[:, None]
    return v


def ccv_dims(w, h, interval, cw=24, ch=24):
    """ccv.js:110-127: the level sizes ccv itself asks for"""
    nxt = interval + 1
    scale = 2.0 ** (1.0 / nxt)
    upto = int(math.floor(math.log(min(cw, ch)) / math.log(scale)))
    n = upto + 2 * nxt
    dims = [(w, h)]
    for i in range(1, n):
        if i <= interval:
            dims.append((int(math.floor(w / scale ** i)), int(math.floor(h / scale ** i))))
        else:
            dims.append((dims[i - nxt][0] // 2, dims[i - nxt][1] // 2))
    return dims


def num_levels(interval, cw=24, ch=24):
    return len(ccv_dims(1000, 1000, interval, cw, ch))


def halved_from(dims, interval):
    """dims[0 .. interval] as given, every level above by ccv's rule: floor(size / 2) of the level interval + 1 below it"""
    nxt = interval + 1
    out = [tuple(d) for d in dims[: nxt]]
    for i in range(nxt, num_levels(interval)):
        out.append((out[i - nxt][0] // 2, out[i - nxt][1] // 2))
    return out


def jobs_of(dims, interval):
    """ht_plan_jobs: (dst level, slot, src level, sx, sy, sw, sh, dw, dh) in level order"""
    nxt = interval + 1
    out = []
    for i in range(1, len(dims)):
        src = 0 if i <= interval else i - nxt
        (sw, sh), (dw, dh) = dims[src], dims[i]
        out.append((i, 0, src, 0, 0, sw, sh, dw, dh))
        if i >= 2 * nxt:
            out.append((i, 1, src, 1, 0, sw - 1, sh, dw - 2, dh))
            out.append((i, 2, src, 0, 1, sw, sh - 1, dw, dh - 2))
            out.append((i, 3, src, 1, 1, sw - 1, sh - 1, dw - 2, dh - 2))
    return out


def pyramid(gray, dims, interval):
    """gray: the level-0 plane (uint8 [h, w]); dims: [(w, h)] of every level.  Returns {(level, slot): (plane, v)}: plane = the canvas
    (uint8 [D.h, D.w], zero outside the drawn rect), v = the declared binary64 values of the drawn rect ([dh, dw], None where nothing is
    drawn and for level 0)."""
    assert gray.dtype == np.uint8 and gray.shape == (dims[0][1], dims[0][0])
    out = {(0, 0): (gray, None)}
    for (i, slot, src, sx, sy, sw, sh, dw, dh) in jobs_of(dims, interval):
        cw_, ch_ = dims[i]
        canvas = np.zeros((max(ch_, 0), max(cw_, 0)), dtype=np.uint8)
        v = None
        if cw_ > 0 and ch_ > 0 and sw > 0 and sh > 0 and dw > 0 and dh > 0:
            v = declared_values(out[(src, 0)][0], sx, sy, sw, sh, dw, dh)
            canvas[:dh, :dw] = np.rint(v).astype(np.uint8)
        out[(i, slot)] = (canvas, v)
    return out


# ---- what a plane's values look like --------------------------------------------------------------------------------------------------

def boundary_distance(v):
    """signed distance of v from the nearest boundary k + 0.5"""
    g = v - 0.5
    return g - np.rint(g)


def model32(src, sw, sh, dw, dh):
    """the binary32 estimate of the kernels' fast path as a MODEL (numpy float32, one rounding per operation, no FMA), without any
    fallback: (rounded bytes, estimates)"""
    ax, bx, tx, _, _ = taps(dw, sw)
    ay, by, ty, _, _ = taps(dh, sh)
    p = src.astype(np.float32)
    tx32, ty32 = tx.astype(np.float32), ty.astype(np.float32)
    ra, rb = p[ay], p[by]
    top = ra[:, ax] + tx32 * (ra[:, bx] - ra[:, ax])
    bot = rb[:, ax] + tx32 * (rb[:, bx] - rb[:, ax])
    v = top + ty32[:, None] * (bot - top)
    assert v.dtype == np.float32
    return np.rint(v).astype(np.uint8), v


def plane_stats(src, dw, dh):
    """figures of the job src -> dw x dh (whole source plane): counts of declared values by distance from a boundary, exact ties by the
    parity of k, and the no-fallback model's mismatches and largest error"""
    sh, sw = src.shape
    v = declared_values(src, 0, 0, sw, sh, dw, dh)
    d = boundary_distance(v)
    ad = np.abs(d)
    k = np.floor(v[d == 0.0]).astype(np.int64)
    m_bytes, m_v = model32(src, sw, sh, dw, dh)
    return dict(pixels=int(v.size), inner=int((ad < RS_EPS).sum()), outer=int(((ad >= RS_EPS) & (ad < 2 * RS_EPS)).sum()),
                below=int(((d < 0) & (ad < 2 * RS_EPS)).sum()), above=int(((d > 0) & (ad < 2 * RS_EPS)).sum()),
                ties=int(k.size), ties_even=int((k % 2 == 0).sum()), ties_odd=int((k % 2 == 1).sum()),
                model_wrong=int((m_bytes != np.rint(v).astype(np.uint8)).sum()), model_err=float(np.abs(m_v.astype(np.float64) - v).max()))


def describe_difference(got, want, v):
    """None when the planes are equal; else the first differing pixel, its declared value and its distance from the boundary"""
    if np.array_equal(got, want):
        return None
    diff = got != want
    y, x = (int(a[0]) for a in np.nonzero(diff))
    if v is not None and y < v.shape[0] and x < v.shape[1]:
        where = f"declared v = {float(v[y, x])!r}, {float(boundary_distance(v[y:y + 1, x:x + 1])[0, 0]):+.3e} from the boundary"
    else:
        where = "outside the drawn rect (must stay 0)"
    return f"{int(diff.sum())} bytes differ, first at x={x} y={y}: got {got[y, x]}, declared {want[y, x]}; {where}"


def near(st):
    return st["inner"] + st["outer"]


# ---- frames on the rounding boundaries ------------------------------------------------------------------------------------------------

def _model_at(p00, p01, p10, p11, tx, ty):
    """model32 for single pixels"""
    p00, p01, p10, p11, tx, ty = (np.asarray(a, dtype=np.float64).astype(np.float32) for a in (p00, p01, p10, p11, tx, ty))
    top = p00 + tx * (p01 - p00)
    bot = p10 + tx * (p11 - p10)
    return top + ty * (bot - top)


def _declared_at(p00, p01, p10, p11, tx, ux, ty, uy):
    top = p00 * ux
    top = top + p01 * tx
    bot = p10 * ux
    bot = bot + p11 * tx
    v = top * uy
    return v + bot * ty


def place_job(plane, dw, dh, rng, rows=None, max_points=1500, rounds=3, chunk=48):
    """Rewrites, in place, the 2x2 source footprints of every other destination pixel (in x and in y) of the job plane -> dw x dh so that
    the declared value lies at a drawn distance d from a boundary: d in [-2 RS_EPS, 2 RS_EPS] on either side, a quarter of them exactly 0.
    rows = (y0, y1): only destination rows in that range (several jobs share one plane by taking bands of it).  Returns the number placed.

    Search per pixel: p00, p01 are drawn; over all (p10, p11) in 0..255 the declared v = A + p10 B + p11 C is a 256 x 256 table, and the
    entry closest to some k + 0.5 + d is taken (k is left free: any boundary will do).  Pixels whose best entry misses by more than `tol` (or,
    for d = 0, is not an exact tie of the binary64 sequence) are redrawn."""
    sh, sw = plane.shape
    ax, bx, tx, ux, cx = taps(dw, sw)
    ay, by, ty, uy, cy = taps(dh, sh)
    stepx, stepy = (1 if sw >= 2 * dw else 2), (1 if sh >= 2 * dh else 2)  # from ratio 2 on, neighbours' footprints are disjoint too
    okx = [x for x in range(0, dw, stepx) if not cx[x] and bx[x] == ax[x] + 1 and 0.02 <= tx[x] <= 0.98]
    y0, y1 = rows if rows else (0, dh)
    oky = [y for y in range(y0 + (y0 & 1), y1, stepy) if not cy[y] and by[y] == ay[y] + 1 and 0.02 <= ty[y] <= 0.98]
    pts = np.array([(y, x) for y in oky for x in okx], dtype=np.int64).reshape(-1, 2)
    if len(pts) > max_points:
        pts = pts[np.sort(rng.choice(len(pts), max_points, replace=False))]
    n = len(pts)
    # distances: a share of exact ties; of the others most lie in the outer half of the band, since the ties count towards the inner half.
    # tx = ((2 i + 1) sw - dw) / (2 dw) mod 1 is a multiple of 1 / (2 dw), of 1 / dw when sw - dw is even; so every value is a multiple of
    # 1 / D, D = den_x den_y.  A tie exists only when D is even; when it is odd the "ties" of the plane are its closest approaches,
    # |d| = 1 / (2 D).  A drawn d can be met to half a step.
    den = (dw if (sw - dw) % 2 == 0 else 2 * dw) * (dh if (sh - dh) % 2 == 0 else 2 * dh)
    tie_share, p_outer = 0.25, 0.62
    dmin = 0.5 / den if den % 2 else 0.0
    want = np.where(rng.random(n) < p_outer, rng.uniform(RS_EPS, 2 * RS_EPS, n), rng.uniform(0.0, RS_EPS, n)) * rng.choice([-1.0, 1.0], n)
    want[rng.random(n) < tie_share] = 0.0
    tol = 2e-5 + 0.5 / den
    grid = np.arange(256, dtype=np.float64)
    placed = 0
    for tie in (True, False):
        todo = np.nonzero((want == 0.0) == tie)[0]
        for _ in range(rounds + (1 if tie else 0)):
            left = []
            for c0 in range(0, len(todo), chunk):
                idx = todo[c0:c0 + chunk]
                y, x = pts[idx, 0], pts[idx, 1]
                wtx, wux, wty, wuy = tx[x], ux[x], ty[y], uy[y]
                p00 = rng.integers(0, 256, len(idx)).astype(np.float64)
                p01 = rng.integers(0, 256, len(idx)).astype(np.float64)
                # ties: the whole table; other distances: every other p10 is enough for a miss below 2e-5
                g10 = grid if tie else grid[int(rng.integers(0, 2))::2]
                base = (p00 * wux + p01 * wtx) * wuy - 0.5 - want[idx]
                g = (base[:, None] + g10[None, :] * (wux * wty)[:, None])[:, :, None] + grid[None, None, :] * (wtx * wty)[:, None, None]
                np.subtract(g, np.rint(g), out=g)
                np.abs(g, out=g)
                flat = g.reshape(len(idx), -1)
                if tie:  # ties of the rational weights are many; which of them is a tie of the binary64 sequence is a matter of its roundings
                    # the first TIE_CANDIDATES table entries, in index order, that are ties of the rational weights (closest approaches when
                    # den is odd); rows with fewer repeat their best entry
                    rr, cc = np.nonzero(flat <= (0.75 if den % 2 else 0.25) / den)
                    rank = np.arange(len(rr)) - np.searchsorted(rr, rr)
                    cand = np.repeat(flat.argmin(axis=1)[:, None], TIE_CANDIDATES, axis=1)
                    keep = rank < TIE_CANDIDATES
                    cand[rr[keep], rank[keep]] = cc[keep]
                    c10, c11 = g10[cand // 256], grid[cand % 256]
                    col = [a[:, None] for a in (p00, p01, wtx, wux, wty, wuy)]
                    vc = _declared_at(col[0], col[1], c10, c11, *col[2:])
                    exact = np.abs(boundary_distance(vc)) <= dmin * (1 + 1e-6)
                    # of the exact ones, one that the binary32 model gets wrong if there is any: these are the pixels a fallback is for
                    wrong = np.rint(_model_at(col[0], col[1], c10, c11, col[2], col[4])) != np.rint(vc)
                    pick = (2 * exact + (exact & wrong)).argmax(axis=1)
                    p10, p11 = c10[np.arange(len(idx)), pick], c11[np.arange(len(idx)), pick]
                else:
                    best = flat.argmin(axis=1)
                    p10, p11 = g10[best // 256], grid[best % 256]
                d = boundary_distance(_declared_at(p00, p01, p10, p11, wtx, wux, wty, wuy))
                good = (np.abs(d) <= dmin * (1 + 1e-6)) if tie else (np.abs(d - want[idx]) <= tol) & (np.abs(d) < 2 * RS_EPS) & (d != 0.0)
                for j in np.nonzero(good)[0]:
                    plane[ay[y[j]], ax[x[j]]], plane[ay[y[j]], bx[x[j]]] = int(p00[j]), int(p01[j])
                    plane[by[y[j]], ax[x[j]]], plane[by[y[j]], bx[x[j]]] = int(p10[j]), int(p11[j])
                placed += int(good.sum())
                left.append(idx[~good])
            todo = np.concatenate(left) if left else todo[:0]
    return placed


def noise_plane(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def as_frames(planes):
    """gray planes as RGBA frames for HT_INPUT_GRAY_IN_R: byte 0 is the plane, G and B differ from it (a kernel that read them would
    show), A = 255"""
    p = np.stack(planes)
    f = np.empty(p.shape + (4,), dtype=np.uint8)
    f[..., 0] = p
    f[..., 1] = 255 - p
    f[..., 2] = p // 2
    f[..., 3] = 255
    return f


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


# ---- k_resample's LDS window ----------------------------------------------------------------------------------------------------------

def kernel_constants():
    """RS_ROWB, RS_TW (ht_pyramid.hip), HT_RS_SRC_ROWS, HT_RSB_ROWS (ht_plan_types.h): read from the sources, not restated"""
    text = open(os.path.join(CSRC, "ht_pyramid.hip")).read() + open(os.path.join(CSRC, "ht_plan_types.h")).read()
    return {k: int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("RS_ROWB", "RS_TW", "HT_RS_SRC_ROWS", "HT_RSB_ROWS")}


def column_tiles_in_lds(sw, dw):
    """per 64-column tile of the job sw -> dw: does its source span fit the RS_ROWB bytes of an LDS row (k_resample: sw16 * 16 <= RS_ROWB,
    with xa = a & ~15 of the tile's first column and b of its last)"""
    K = kernel_constants()
    a, b, _, _, _ = taps(dw, sw)
    fits = []
    for x0 in range(0, dw, K["RS_TW"]):
        x1 = min(x0 + K["RS_TW"], dw) - 1
        xa = int(a[x0]) & ~15
        fits.append(((int(b[x1]) - xa) // 16 + 1) * 16 <= K["RS_ROWB"])
    return fits


@functools.lru_cache(maxsize=None)
def lds_limit_widths(sw):
    """(below, above): the narrowest destination width at which EVERY column tile of sw -> dw still fits the LDS window, and the widest at
    which at least one FULL tile does not (then read straight from HBM while its neighbours may still fit)"""
    K = kernel_constants()
    below = min(dw for dw in range(sw // 4, sw // 2 + 1) if all(column_tiles_in_lds(sw, dw)))
    above = max(dw for dw in range(sw // 4, below) if dw > K["RS_TW"] and not all(column_tiles_in_lds(sw, dw)[: dw // K["RS_TW"]]))
    return below, above


# ---- the cases of tests/test_gpu_pyramid_ties.py (conditions asserted in tests/test_pyramid_cases_cpu.py) ------------------------------

def _points(dw, dh):
    """lattice points asked for: enough for 5 % of the plane to be placed with a margin, the generation budget in mind"""
    return max(250, int(0.11 * dw * dh))


@functools.lru_cache(maxsize=None)
def targeted_planes(w, h, targets_a, targets_b, seed):
    """the batch of every GPU test: [plane A aimed at targets_a, plane B aimed at targets_b, noise]; read-only"""
    out = []
    for k, targets in enumerate((targets_a, targets_b)):
        rng_seed = seed + k
        rng = np.random.default_rng(rng_seed)
        plane = rng.integers(0, 256, (h, w), dtype=np.uint8)
        nb = len(targets)
        for j, (dw, dh) in enumerate(targets):
            ay, by, _, _, _ = taps(dh, h)
            lo, hi = j * h // nb, (j + 1) * h // nb
            ys = [y for y in range(dh) if ay[y] >= lo and by[y] < hi]
            place_job(plane, dw, dh, rng, rows=(ys[0], ys[-1] + 1) if nb > 1 else None, max_points=_points(dw, dh))
        out.append(plane)
    out.append(noise_plane(w, h, seed + 2))
    for p in out:
        p.setflags(write=False)
    return out


def ccv_case(w, h, interval, levels_a, levels_b, seed):
    """boundary frames at ccv's own sizes: dict(w, h, interval, dims, planes, targets = [(plane index, level)])"""
    dims = ccv_dims(w, h, interval)
    planes = targeted_planes(w, h, tuple(dims[i] for i in levels_a), tuple(dims[i] for i in levels_b), seed)
    return dict(w=w, h=h, interval=interval, dims=dims, planes=planes, targets=[(0, i) for i in levels_a] + [(1, i) for i in levels_b])


# C.1: 201x157 at interval 5, levels 1, 3, 5; 169x125 (odd x odd) at interval 2.  At interval 2 only levels 1 .. 3 read level 0 (level 3 is
# its 2 + 1/dw halving, level 5 reads level 2, which no test controls at ccv's own sizes), so the frames aim at 1, 2 and 3 there.
CCV_CASES = {"201x157_i5": (201, 157, 5, (1,), (3, 5), 7106), "169x125_i2": (169, 125, 2, (1,), (2, 3), 7200)}
# C.3: a geometry whose whole pyramid fits the tail kernel (tail_first_gen = 1 with rs_tailcap = TAIL_CAP)
TAIL_CASE = (133, 101, 5, (1,), (3, 5), 7309)
TAIL_CAP = 1000000


def copy_level_case(w, h, seed, copy_level=2, interval=5):
    """C.2: level copy_level (first generation) takes the frame's own size — ratio 1, t = 0, a copy —, so level copy_level + interval + 1 is
    a second-generation job whose source bytes are the frame's: w x h -> w // 2 x h // 2, ratio 2 + 1/dw for odd sizes, exactly 2 (the
    integer box mean) for even ones.  Level interval + 1 is the same job from level 0 itself."""
    first = ccv_dims(w, h, interval)[: interval + 1]
    first[copy_level] = (w, h)
    dims = halved_from(first, interval)
    half = (w // 2, h // 2)
    assert dims[copy_level + interval + 1] == half
    if w % 2 or h % 2:
        planes = targeted_planes(w, h, (half,), (half,), seed)
        targets = [(0, interval + 1), (1, interval + 1)]
    else:  # the box mean has no fast path to mislead: the frames aim at two ordinary levels, and a quarter of the 2:1 plane are ties anyway
        planes = targeted_planes(w, h, (dims[1],), (dims[3],), seed)
        targets = [(0, 1), (1, 3)]
    return dict(w=w, h=h, interval=interval, dims=dims, planes=planes, targets=targets, half_levels=(interval + 1, copy_level + interval + 1))


COPY_CASES = {"odd_169x125": (169, 125, 7403), "even_164x124": (164, 124, 7500)}


def unusual_dims(w, h):
    """C.4: two sets of sizes for levels 1 .. 5 (interval 5) that ccv never asks for; the levels above follow ccv's halving.
    set 0: ratio 1, w-1 x h-1, ratio 1.5, just below and just above the LDS window's limit (lds_limit_widths; heights at the same ratio);
    set 1: ratios 3 and 7, 1x1, 0x0, and w-2 x h-1 (an exact 2:1 above it has an even / odd parent depending on the frame: levels 6 ..
    halve levels 0 .. in both sets, so 2:1 jobs with even and with odd parents are in every set)."""
    below, above = lds_limit_widths(w)
    first0 = [(w, h), (w, h), (w - 1, h - 1), (int(w / 1.5), int(h / 1.5)), (below, h * below // w), (above, h * above // w)]
    first1 = [(w, h), (w // 3, h // 3), (w // 7, h // 7), (1, 1), (0, 0), (w - 2, h - 1)]
    return [halved_from(first0, 5), halved_from(first1, 5)]


UNUSUAL_SIZES = [(333, 217), (641, 359)]


@functools.lru_cache(maxsize=None)
def unusual_case(w, h, which):
    """planes: one boundary plane aimed at the level just below the LDS limit (the fast path at its largest ratio) and two noise planes; the
    same three frames for both sets of sizes"""
    dims = unusual_dims(w, h)[which]
    planes = targeted_planes(w, h, (unusual_dims(w, h)[0][4],), (), 7600 + w)
    return dict(w=w, h=h, interval=5, dims=dims, planes=planes, targets=[(0, 4)] if which == 0 else [])

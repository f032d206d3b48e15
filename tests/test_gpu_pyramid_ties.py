"""Every byte of every (level, slot) plane of the pyramid against the numpy binary64 restatement of tests/pyramid_cases.py, on frames built
to sit on the rounding boundaries and at level sizes ccv never asks for.

The generation kernels (k_resample, k_resample_bands, the three tail forms) evaluate a pixel in binary32 and take the declared binary64
sequence only when the estimate lies within RS_EPS = 2^-13 of a boundary k + 0.5; exact 2:1 jobs take an integer box mean.  On the noise,
smooth and face frames of the other pyramid tests a handful of pixels per plane lie where that decision is made.  Here 6 - 11 % of a
targeted plane do, ties of both parities among them: tests/test_pyramid_cases_cpu.py asserts that from the restatement alone, and that a
binary32 estimate without fallback gets dozens of those pixels wrong.

Every batch is three frames (two boundary frames and noise, or one and two for the unusual ratios), HT_INPUT_GRAY_IN_R, so byte 0 of a
frame IS level 0; planes are read with pyramid_readback after detect_enqueue / detect_collect.  Levels past the targeted ones are whatever
the frames yield: their near-boundary pixels are counted and printed, nothing is asked of the count.

The tail: HT_TAIL_MAX_GENS = 8 and HT_TAIL_MAX_JOBS = 32 leave room for the whole pyramid of a small frame (interval 5: 7 generations of
at most 24 jobs), so with rs_tailcap = 10^6 the plan of 133x101 has tail_first_gen = 1 (tests/test_geometry_plan_cpu.py) and the tail
kernels read the test's own bytes."""
import functools

import numpy as np
import pytest

import pyramid_cases as pc
from headtrackr_amd.api import HT_INPUT_GRAY_IN_R, Context

pytestmark = pytest.mark.gpu

# every generation-kernel selection the suite forces elsewhere (tests/test_gpu_detect.py, tests/detect_variant_cases.py)
KERNELS = [None, "rs_bands=0", "rs_bands=0,rs_notail=1", "rs_bands=1,rs_notail=1", "rs_bands=0,rs_rpt=2", "rs_bands=0,rs_k=3", "rs_bands=1,rs_rpt=2", "rs_nofast=1"]
BOTH = ["rs_bands=1", "rs_bands=0"]

_CTX = {}


@pytest.fixture(scope="module")
def ctx_for():
    """one context per (interval, options), closed when the module is done"""
    def get(interval, options=None):
        key = (interval, options)
        if key not in _CTX:
            _CTX[key] = Context(interval=interval, options=options, hit_capacity=1 << 16)
        return _CTX[key]

    yield get
    for c in _CTX.values():
        c.close()
    _CTX.clear()


_REF = {}


def reference(key, case):
    """the restated pyramid of the case's three planes, computed once and read-only"""
    if key not in _REF:
        out = []
        for p in case["planes"]:
            ref = pc.pyramid(p, case["dims"], case["interval"])
            for plane, v in ref.values():
                plane.setflags(write=False)
                if v is not None:
                    v.setflags(write=False)
            out.append(ref)
        _REF[key] = out
    return _REF[key]


def check_pyramid(c, key, case, own_dims):
    """own_dims: the library computes ccv's sizes itself (level_dims = None)"""
    frames = pc.as_frames(case["planes"])
    w, h, dims = case["w"], case["h"], case["dims"]
    c.set_geometry(w, h, len(frames), None if own_dims else np.array(dims, dtype=np.int32))
    c.upload(frames)
    c.detect_enqueue(HT_INPUT_GRAY_IN_R)
    c.detect_collect()
    assert c.num_levels == len(dims)
    nxt = case["interval"] + 1
    compared = deep_near = 0
    for f, ref in enumerate(reference(key, case)):
        for i in range(len(dims)):
            for s in range(4):
                present = s == 0 or i >= 2 * nxt
                assert bool(c.plane(i, s).present) == present and ((i, s) in ref) == present, (i, s)
                if not present:
                    continue
                want, v = ref[(i, s)]
                got = c.pyramid_readback(f, i, s)
                assert got.shape == want.shape, f"frame {f} level {i} slot {s}: {got.shape[::-1]} for {dims[i]}"
                compared += 1
                if v is not None and i > 2 * nxt:
                    deep_near += int((np.abs(pc.boundary_distance(v)) < 2 * pc.RS_EPS).sum())
                bad = pc.describe_difference(got, want, v)
                assert bad is None, f"frame {f} level {i} slot {s} ({dims[i][0]}x{dims[i][1]}): {bad}"
    assert compared == 3 * (len(dims) + 3 * (len(dims) - 2 * nxt))
    print(f"{key}: {compared} planes equal; {deep_near} values within 2 RS_EPS of a boundary on the levels past {2 * nxt}")


# ---- 1. boundary frames at ccv's own sizes ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ccv_case(name):
    return pc.ccv_case(*pc.CCV_CASES[name])


@pytest.mark.parametrize("opts", KERNELS, ids=lambda o: o or "default")
@pytest.mark.parametrize("name", list(pc.CCV_CASES))
def test_boundary_frames_at_ccvs_own_sizes(ctx_for, name, opts):
    """201x157 at interval 5 (frames aimed at levels 1, 3 and 5) and 169x125 at interval 2 (levels 1, 2, 3: only those read level 0
    there), under every generation-kernel selection"""
    case = ccv_case(name)
    check_pyramid(ctx_for(case["interval"], opts), name, case, own_dims=True)


# ---- 2. second generation from the test's own bytes ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def copy_case(name):
    return pc.copy_level_case(*pc.COPY_CASES[name])


@pytest.mark.parametrize("opts", BOTH)
@pytest.mark.parametrize("name", list(pc.COPY_CASES))
def test_second_generation_from_the_tests_own_bytes(ctx_for, name, opts):
    """level 2 is given the frame's own size (ratio 1: a copy), so level 8 halves the test's bytes in generation 2: 169x125 -> 84x62 at
    ratios 2 + 1/dw, and 164x124 -> 82x62 through the integer box mean, where a quarter of all pixels are ties"""
    case = copy_case(name)
    check_pyramid(ctx_for(5, opts), name, case, own_dims=False)


# ---- 3. the tail kernels on boundary inputs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", [0, 1, 2])
def test_tail_kernels_on_boundary_frames(ctx_for, table):
    """the whole pyramid of 133x101 in the tail kernel (tail_first_gen = 1): its first generations read the boundary frames themselves"""
    case = pc.ccv_case(*pc.TAIL_CASE)
    check_pyramid(ctx_for(5, f"rs_tailtable={table},rs_tailcap={pc.TAIL_CAP}"), "tail", case, own_dims=True)


# ---- 4. ratios ccv never asks for ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", BOTH)
@pytest.mark.parametrize("which", [0, 1], ids=["near-1-and-lds-limit", "3-7-1x1-0x0"])
@pytest.mark.parametrize("w,h", pc.UNUSUAL_SIZES)
def test_ratios_ccv_never_asks_for(ctx_for, w, h, which, opts):
    """levels 1 .. 5 through level_dims — set 0: the frame's own size, w-1 x h-1, ratio 1.5, just below and just above the LDS window's
    limit; set 1: ratios 3 and 7 (HBM taps on several tiles with partial last ones), 1x1, 0x0, w-2 x h-1 — and ccv's halving above them,
    so exact 2:1 jobs with even and with odd parents follow.  One boundary frame aimed at the level just below the limit, two of noise."""
    case = pc.unusual_case(w, h, which)
    check_pyramid(ctx_for(5, opts), f"unusual_{w}x{h}_{which}", case, own_dims=False)

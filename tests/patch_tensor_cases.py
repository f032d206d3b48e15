"""The model-input tensors' rule (headtrackr_amd/csrc/ht_patch_plan.h) restated in Python, from its description: which bits an RGBA8 patch
becomes.  numpy binary32 `*` and `+` (two ufuncs: nothing to fuse), astype(np.float16) for binary16, the integer formula for bfloat16, gray
from a restated ccv.js:29.  Shared by tests/test_patch_tensor_cpu.py and tests/test_gpu_patch_tensor.py; nothing here touches the code
under test."""
import itertools
import struct
from fractions import Fraction

import numpy as np

DTYPES = ("f32", "f16", "bf16")
LAYOUTS = ("chw", "hwc")
CHANNELS = ("rgb", "bgr", "gray")
FORMATS = list(itertools.product(DTYPES, LAYOUTS, CHANNELS))  # all 18
DTYPE_CODE = {"f32": 0, "f16": 1, "bf16": 2}
LAYOUT_CODE = {"chw": 0, "hwc": 1}
CHANNELS_CODE = {"rgb": 0, "bgr": 1, "gray": 2}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def f32(x):
    return float(np.float32(x))


def mean_std(mean, std):
    """scale = 1 / (255 std), bias = -mean / std in binary64, then rounded to binary32"""
    return tuple(f32(1.0 / (255.0 * s)) for s in std), tuple(f32(-m / s) for m, s in zip(mean, std))


def _same(scale, bias):
    return (f32(scale),) * 3, (f32(bias),) * 3


# name -> (scale[3], bias[3]) as binary32 values
PAIRS = {
    "unit": _same(1 / 255, 0.0),
    "signed": _same(2 / 255, -1.0),
    "imagenet": mean_std(IMAGENET_MEAN, IMAGENET_STD),
    "inverted": _same(-1 / 255, 1.0),
    "bf16_ties": _same(1 + 2.0 ** -8, 0.0),
    "f16_ties": _same(1 + 2.0 ** -11, 0.0),
    "f16_overflow": _same(300.0, 0.0),
    "f16_subnormal": _same(2.0 ** -20, 0.0),
    "zero": _same(0.0, 0.0),
    "negative_zero_bias": _same(0.0, -0.0),
    "smallest": _same(2.0 ** -64, 0.0),
    "largest": _same(2.0 ** 64, -(2.0 ** 64)),
}
ROUNDING_PAIRS = ("bf16_ties", "f16_ties", "f16_overflow", "f16_subnormal")


def nchannels(channels):
    return 1 if channels == "gray" else 3


def pair_for(name, channels):
    """the pair's scale and bias with the slots of channels the mode does not have at 0"""
    scale, bias = PAIRS[name]
    C = nchannels(channels)
    return tuple(scale[:C]) + (0.0,) * (3 - C), tuple(bias[:C]) + (0.0,) * (3 - C)


def gray(r, g, b):
    """ccv.js:29 on byte arrays: binary64 products and sums, round half to even, clamp (Uint8ClampedArray)"""
    v = (r.astype(np.float64) * 0.3 + g.astype(np.float64) * 0.59) + b.astype(np.float64) * 0.11
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def value(b, scale, bias):
    """step 2: two binary32 operations"""
    m = b.astype(np.float32) * np.float32(scale)
    return (m + np.float32(bias)).astype(np.float32)


def bits(v, dtype):
    """step 3: the element bits of binary32 values, as uint32 (f32) or uint16"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == "f32":
        return v.view(np.uint32)
    if dtype == "f16":
        with np.errstate(over="ignore", under="ignore"):
            return v.astype(np.float16).view(np.uint16)
    u = v.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def byte_table(name, dtype, c=0):
    """the element bits of bytes 0 .. 255 under a pair, channel c"""
    scale, bias = PAIRS[name]
    return bits(value(np.arange(256, dtype=np.uint8), scale[c], bias[c]), dtype)


def source_bytes(patch, channels):
    """step 1: [H, W, C] source bytes of an RGBA8 patch [H, W, 4]"""
    if channels == "rgb":
        return patch[..., :3]
    if channels == "bgr":
        return patch[..., 2::-1]
    return gray(patch[..., 0], patch[..., 1], patch[..., 2])[..., None]


def f(patch, fmt, pair):
    """the tensor bytes (uint8, 1-D) of an RGBA8 patch [H, W, 4] under fmt = (dtype, layout, channels) and pair = (scale[3], bias[3])"""
    dtype, layout, channels = fmt
    scale, bias = pair
    b = source_bytes(np.ascontiguousarray(patch), channels)
    el = np.stack([bits(value(b[..., c], scale[c], bias[c]), dtype) for c in range(b.shape[-1])], axis=-1)  # [H, W, C]
    if layout == "chw":
        el = np.moveaxis(el, -1, 0)
    return np.ascontiguousarray(el).reshape(-1).view(np.uint8)


def patch_bytes(w, h, dtype, channels):
    return nchannels(channels) * w * h * ESIZE[dtype]


def default_stride(w, h, dtype, channels):
    return (patch_bytes(w, h, dtype, channels) + 3) & ~3


def offset(w, h, dtype, layout, channels, c, x, y):
    C = nchannels(channels)
    return ((c * w * h + y * w + x) if layout == "chw" else ((y * w + x) * C + c)) * ESIZE[dtype]


# ---- exact arithmetic: what ONE rounding (a fused multiply-add) would give ------------------------------------------------------------

def round_to_f32(q):
    """a Fraction rounded to the nearest binary32, ties to even (normal range)"""
    if q == 0:
        return 0.0
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    m = a / Fraction(2) ** (e - 23)
    n, rem = m.numerator // m.denominator, m - m.numerator // m.denominator
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return s * float(Fraction(n) * Fraction(2) ** (e - 23))


def fma_differs(name, c=0):
    """the bytes at which round(b * scale + bias) in one step differs from the rule's two roundings"""
    scale, bias = PAIRS[name]
    two = value(np.arange(256, dtype=np.uint8), scale[c], bias[c])
    return [b for b in range(256) if struct.pack("<f", round_to_f32(Fraction(b) * Fraction(scale[c]) + Fraction(bias[c]))) != struct.pack("<f", float(two[b]))]


FORMAT_STRUCT = struct.Struct("<4i6f")  # ht_patch_format, 40 bytes


def pack_format(dtype, layout, channels, pad, scale, bias):
    return FORMAT_STRUCT.pack(dtype, layout, channels, pad, *scale, *bias)

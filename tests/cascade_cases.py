"""Cascade blobs for the host-only cascade planner (tests/test_cascade_plan_cpu.py).  A plain module, imported like tests/cs_cases.py.
Every blob is the built-in cascade (headtrackr_amd/data/cascade.bin: 24x24, 16 stages, 2015 features of at most 5 points per polarity,
alpha[0] == -alpha[1], 6-digit decimals) after a named mutation; nothing here says what the planner must answer — that is
tests/golden/cascade_plan.json, recorded from the library before the planner became a unit of its own.

A case is (name, blob, builtin, split): `builtin` is what ht_scan_is_builtin_cascade answers for the blob (its FNV-1a check, restated in
is_builtin below) unless the case overrides it, `split` the option of that name (0: not given)."""
import functools
import struct

import numpy as np

from headtrackr_amd.cascade import load_cascade

BUILTIN = load_cascade()


def is_builtin(blob):
    return bytes(blob) == BUILTIN.blob


def pack(stages, feats, cw=24, ch=24, nstages=None, nfeat=None, magic=b"HTCB", version=1, maxpts=8):
    """header + rows; the header's counts are the rows' unless given"""
    head = struct.pack("<4sIIIIIII", magic, version, len(stages) if nstages is None else nstages, cw, ch, len(feats) if nfeat is None else nfeat, maxpts, 0)
    return head + stages.tobytes() + feats.tobytes()


def rows():
    """writable copies of the built-in stage and feature rows"""
    return BUILTIN.stages.copy(), BUILTIN.features.copy()


def _first_of(stage):
    return int(BUILTIN.stages["first"][stage])


def _set_points(f, pol, pts):
    """points [(x, y, z)] into slots 0.. of polarity 'p' / 'n' of feature row f; size grows to hold them"""
    for q, (x, y, z) in enumerate(pts):
        f[pol + "x"][q], f[pol + "y"][q], f[pol + "z"][q] = x, y, z
    f["size"] = max(int(f["size"]), len(pts))


# ---- accepted blobs -------------------------------------------------------------------------------------------------------------------

def undecimal():
    """feature 10: alpha[0] with 10 decimals (alpha[1] is not looked at behind it); feature 20: alpha[1] with 10 decimals"""
    st, ft = rows()
    ft["alpha"][10, 0] = float(ft["alpha"][10, 0]) - 1e-10
    ft["alpha"][20, 1] = float(ft["alpha"][20, 1]) + 1e-10
    return pack(st, ft)


def huge_alphas(stage=15):
    """every alpha of one stage +-(1e6 + k / 4): exact multiples of 1e-8 whose sum's rounding error may reach the 1e-8 grid"""
    st, ft = rows()
    a, n = _first_of(stage), int(st["count"][stage])
    v = 1.0e6 + 0.25 * np.arange(n)
    ft["alpha"][a:a + n, 0], ft["alpha"][a:a + n, 1] = -v, v
    return pack(st, ft)


def asymmetric():
    """the last feature: alpha[0] = -2.5 beside its alpha[1], both decimal"""
    st, ft = rows()
    ft["alpha"][-1, 0] = -2.5
    return pack(st, ft)


def alpha_21():
    """the last feature: -+21.0, i.e. 2.1e9 after scaling: inside 2^31, outside 2.0e9"""
    st, ft = rows()
    ft["alpha"][-1] = (-21.0, 21.0)
    return pack(st, ft)


SIX = [(1, 2, 0), (20, 3, 0), (5, 11, 1), (0, 5, 2), (23, 23, 0), (11, 0, 1)]


def six_points(feature):
    st, ft = rows()
    _set_points(ft[feature], "p", SIX)
    return pack(st, ft)


def hole():
    """behind stage 4 (in every table, the packed tail too): the first feature with three positive points loses the middle one — pz[1] = -1,
    pz[2] valid — and the first with three negative ones likewise"""
    st, ft = rows()
    a = _first_of(4)
    kp = a + int(np.argmax((ft["pz"][a:, :3] >= 0).all(1)))
    kn = a + int(np.argmax((ft["nz"][a:, :3] >= 0).all(1)))
    ft["pz"][kp, 1] = -1
    ft["nz"][kn, 1] = -1
    return pack(st, ft)


def window(cw, ch):
    """another window size: coordinates folded into each plane's range; beyond 24x24 one feature reaches the far corner of every plane"""
    st, ft = rows()
    for pol in "pn":
        z = np.maximum(ft[pol + "z"], 0)
        ft[pol + "x"] %= (cw >> z).astype(np.int8)
        ft[pol + "y"] %= (ch >> z).astype(np.int8)
    if cw > 24:
        _set_points(ft[5], "p", [(cw - 1, ch - 1, 0), (cw // 2 - 1, ch // 2 - 1, 1), (cw // 4 - 1, ch // 4 - 1, 2)])
        _set_points(ft[5], "n", [(cw // 4 - 1, 0, 2), (0, ch - 1, 0)])
    return pack(st, ft, cw=cw, ch=ch)


def single_stage():
    st, ft = rows()
    return pack(st[:1], ft[:int(st["count"][0])])


def long_tail():
    """the last stage once more: 17 stages, 2579 features, 2551 of them behind stage 4 (2048 records fill the deep kernel's 64 KB)"""
    st, ft = rows()
    last = st[-1:].copy()
    last["first"] = len(ft)
    return pack(np.concatenate([st, last]), np.concatenate([ft, ft[_first_of(15):]]))


def empty_last_stage():
    """a 17th stage without features"""
    st, ft = rows()
    last = st[-1:].copy()
    last["first"], last["count"] = len(ft), 0
    return pack(np.concatenate([st, last]), ft)


@functools.lru_cache(maxsize=None)
def accepted():
    """[(name, blob, builtin, split)]"""
    out = []

    def add(name, blob, split=0, builtin=None):
        out.append((name, blob, is_builtin(blob) if builtin is None else builtin, split))

    for split in (0, 1, 4, 8, 12, 63):
        add("builtin_split%d" % split, BUILTIN.blob, split)
    for split in (0, 8, 12, 63):
        add("same_bytes_not_builtin_split%d" % split, BUILTIN.blob, split, builtin=False)
    add("undecimal", undecimal())
    add("huge_alphas", huge_alphas())
    add("asymmetric", asymmetric())
    add("alpha_21", alpha_21())
    add("six_points_below_split", six_points(_first_of(2)))
    add("six_points_behind_split", six_points(_first_of(9) + 3))
    add("six_points_at_split12", six_points(_first_of(12)), 12)
    add("hole", hole())
    add("window_20x20", window(20, 20))
    add("window_64x64", window(64, 64))
    add("window_24x20", window(24, 20))
    add("single_stage", single_stage())
    add("long_tail", long_tail())
    add("long_tail_split15", long_tail(), 15)
    add("empty_last_stage_split16", empty_last_stage(), 16)
    assert len({n for n, *_ in out}) == len(out)
    return out


# ---- rejected blobs: (name, blob), grouped by the message they are named for --------------------------------------------------------

def _feat_mut(feature, **fields):
    st, ft = rows()
    for k, v in fields.items():
        key, _, slot = k.partition("_")
        if slot:
            ft[key][feature, int(slot)] = v
        else:
            ft[key][feature] = v
    return pack(st, ft)


def _stage_mut(stage, **fields):
    st, ft = rows()
    for k, v in fields.items():
        st[k][stage] = v
    return pack(st, ft)


@functools.lru_cache(maxsize=None)
def rejected():
    st, ft = rows()
    b = BUILTIN.blob
    return [
        ("bad_magic", b"HTCX" + b[4:]),
        ("header_only_31_bytes", b[:31]),
        ("bad_version", pack(st, ft, version=2)),
        ("bad_maxpts", pack(st, ft, maxpts=4)),
        ("zero_stages", pack(st, ft, nstages=0)),
        ("stages_64", pack(st, ft, nstages=64)),
        ("window_3", pack(st, ft, cw=3)),
        ("window_65", pack(st, ft, ch=65)),
        ("short_by_one", b[:-1]),
        ("long_by_one", b + b"\0"),
        ("stage_first_off_by_one", _stage_mut(1, first=5)),
        ("last_stage_overruns", _stage_mut(15, count=565)),
        ("size_0", _feat_mut(7, size=0)),
        ("size_9", _feat_mut(7, size=9)),
        ("first_positive_invalid", _feat_mut(7, pz_0=-1)),
        ("first_negative_invalid", _feat_mut(7, nz_0=-1)),
        ("x_24_on_plane_0", _feat_mut(7, pz_0=0, px_0=24, py_0=0)),
        ("y_12_on_plane_1", _feat_mut(7, nz_0=1, nx_0=0, ny_0=12)),
        ("x_6_on_plane_2", _feat_mut(7, pz_0=2, px_0=6, py_0=0)),
        ("plane_3", _feat_mut(7, pz_0=3, px_0=0, py_0=0)),
        ("negative_x", _feat_mut(7, nz_0=0, nx_0=-1, ny_0=0)),
    ]


def manifest(directory):
    """writes every blob into `directory` and returns the path of the case list both the harness and the recorder read: one
    'name blob-file builtin split' per line (rejected cases: builtin 0, split 0)"""
    import os

    lines = []
    for name, blob, builtin, split in list(accepted()) + [(n, b, False, 0) for n, b in rejected()]:
        path = os.path.join(directory, name + ".bin")
        with open(path, "wb") as f:
            f.write(blob)
        lines.append("%s %s %d %d\n" % (name, path, int(builtin), split))
    path = os.path.join(directory, "cases.txt")
    with open(path, "w") as f:
        f.writelines(lines)
    return path

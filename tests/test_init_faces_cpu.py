"""A tracker per grouped face (ht_camshift_init_faces) without a GPU: the batch and the scenarios of tests/init_faces_cases.py provably
reach every branch of the rule (from the CPU oracle alone); the rule and the host plan the library compiles (csrc/ht_cs_faces_plan.h) give,
in a stand-alone program built plain and under AddressSanitizer + UBSan, what the Python restatement gives, record for record; the resolve
kernel's resources; the constants of the Python layer."""
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import init_faces_cases as fc
from conftest import ROOT
from headtrackr_amd import native
from oracle import ht_oracle as ho

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
OVER_CAP = 1  # HT_GRP_ST_OVER_CAP
ASSOC = native.HT_CSF_ASSOCIATE
I32_MAX, I32_MIN = 2147483647, -2147483648


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------

def oracle_windows(cascade_blob, slots):
    """the search windows of a scenario's slots from the oracle's camshift: initTracker on frame A's face, two track steps on frame A"""
    lists, fr = fc.lists_of(cascade_blob), fc.frames()
    out = []
    for s in slots:
        if s is None:
            out.append(fc.ZERO)
            continue
        t = ho.cs_init(fr[fc.FRAME_A], *fc.floor_rect(lists[fc.FRAME_A][s[1]]))
        for _ in range(2):
            sw, _to = ho.cs_track(t, fr[fc.FRAME_A])
        out.append(tuple(int(v) for v in sw))
    return out


def test_batch_and_scenarios_reach_every_branch_of_the_rule(cascade):
    lists = fc.lists_of(cascade.blob)
    assert len(fc.frames()) == fc.NFRAMES == 8
    A, B = lists[fc.FRAME_A], lists[fc.FRAME_B]
    assert len(A) == len(B) == 4 and all(f[5] > 0 and f[4] > 5.0 for f in B)

    def nearest(face, pasted):  # which pasted face a grouped rect is
        return min(range(4), key=lambda i: abs(pasted[i][0] - face[0]) + abs(pasted[i][1] - face[1]))

    ida, idb = [nearest(f, fc.FACES_A) for f in A], [nearest(f, fc.FACES_B) for f in B]
    assert sorted(ida) == sorted(idb) == [0, 1, 2, 3] and ida != idb  # the same four faces, listed in another order
    rank_b = sorted(range(4), key=lambda i: (-B[i][4], i))

    # a matching that is not the identity permutation: every tracker finds the face it was on, whatever its rank
    wins = oracle_windows(cascade.blob, fc.SCENARIOS["permuted"])
    assert all(w[2] > 0 and w[3] > 0 for w in wins)
    got = fc.resolve_frame(B, wins, -10.0, True)
    slot_rank = [rank_b.index(r[1]) for r in got]
    assert sorted(slot_rank) == [0, 1, 2, 3] and slot_rank != [0, 1, 2, 3]
    for j, s in enumerate(fc.SCENARIOS["permuted"]):
        assert idb[got[j][1]] == ida[s[1]], (j, got[j])  # the slot is the identity
    assert [rank_b.index(r[1]) for r in fc.resolve_frame(B, wins, -10.0, False)] == [0, 1, 2, 3]

    # an overlap tie; a live unmatched slot next to a free slot; a live unmatched slot that is overwritten
    wins = oracle_windows(cascade.blob, fc.SCENARIOS["tie_free_overwrite"])
    assert wins[0] == wins[1] and wins[2] == fc.ZERO
    kept = [fc.floor_rect(B[i]) for i in rank_b[:3]]
    ov = [[fc.overlap(w, r) for r in kept] for w in wins]
    tied = [r for r in range(3) if ov[0][r] > 0]
    assert len(tied) == 1 and ov[0] == ov[1] and ov[2] == [0, 0, 0]  # the tie: slots 0 and 1 against one face, nothing else overlaps
    got = fc.resolve_frame(B, wins, -10.0, True)
    assert [r[0] for r in got] == [fc.FACE] * 3 and all(r[3] == 1 for r in got)
    rest = [rank_b[r] for r in range(3) if r != tied[0]]
    assert got[0][1] == rank_b[tied[0]]          # the lowest slot position wins the tie
    assert got[2][1] == rest[0]                  # the first remaining face takes the free slot, not the live slot in front of it
    assert got[1][1] == rest[1]                  # no free slot is left: the unmatched live slot is overwritten

    # dropped > 0 at k = 3 on the tiled frame; a threshold that splits a frame's faces; a frame without faces
    T = lists[fc.TILED]
    assert len(T) == 15
    got = fc.resolve_frame(T, [fc.ZERO] * 3, -10.0, False)
    assert [r[3] for r in got] == [12] * 3 and [r[1] for r in got] == sorted(range(15), key=lambda i: (-T[i][4], i))[:3]
    split = [f for f in range(fc.NFRAMES) if 0 < sum(x[4] > 5.0 for x in lists[f]) < sum(x[4] > -10.0 for x in lists[f])]
    assert fc.TWO_FACES in split and fc.TILED in split
    assert lists[fc.NOISE] == [] and fc.resolve_frame([], [fc.ZERO] * 2, -10.0, True) == [(fc.UNTOUCHED, -1, fc.ZERO, 0)] * 2


# ---- header against restatement ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("init_faces_" + request.param) / "init_faces_harness")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "init_faces_harness.cc"), "-o", exe])
    return exe


def _frame_case(faces, windows, thr, flags, status=0, nhits=10, bad=0, cap=1 << 20, collected=0):
    """(packed input, expected records).  faces: (x, y, width, height, confidence, neighbors)"""
    blob = struct.pack("<i2i5Iid", 1, len(windows), len(faces), flags, status, nhits, bad, cap, collected, float(thr))
    blob += b"".join(struct.pack("<5d2i", *[float(v) for v in f[:5]], int(f[5]), 0) for f in faces)
    blob += b"".join(struct.pack("<4i", *w) for w in windows)
    deferred = nhits > cap or bad != 0 or (not collected and (status & OVER_CAP) != 0)
    return blob, fc.resolve_frame(faces, windows, thr, bool(flags & ASSOC), deferred)


def _random_frames(n):
    rng = np.random.RandomState(20240607)
    grid = [0, 0, 8, 8, 16, 16, 24, 32, 40, -8]   # coordinates and sizes from a small grid: equal overlaps and equal windows are frequent
    out = []
    for _ in range(n):
        k, m = int(rng.randint(1, 17)), int(rng.randint(0, 41))
        faces = [(grid[rng.randint(10)] + 0.5 * rng.randint(2), grid[rng.randint(10)], grid[rng.randint(10)], grid[rng.randint(10)] + 0.25,
                  float(rng.randint(1, 5)), int(rng.randint(0, 3))) for _ in range(m)]
        windows = [(grid[rng.randint(10)], grid[rng.randint(10)], grid[rng.randint(10)], grid[rng.randint(10)]) for _ in range(k)]
        out.append(_frame_case(faces, windows, (-10.0, 1.0, 2.5)[rng.randint(3)], int(rng.randint(2))))
    return out


def _extreme_frames():
    nan, inf = float("nan"), float("inf")
    out = []
    big = [(1e300, -1e300, inf, inf, 3.0, 1), (2147483000.0, 2147483000.0, 4e9, 4e9, 2.0, 1), (-3e9, -3e9, 5e9, 5e9, 2.0, 2), (nan, nan, 10.0, 10.0, 1.0, 1)]
    wins = [(I32_MAX, I32_MAX, I32_MAX, I32_MAX), (I32_MIN, I32_MIN, I32_MAX, I32_MAX), (I32_MAX - 5, 0, 100, I32_MAX), (0, 0, I32_MAX, I32_MAX),
            (2147483000, 2147483000, 1000, 1000)]
    for flags in (0, ASSOC):
        out.append(_frame_case(big, wins, -10.0, flags))          # saturated rects, x near INT32_MAX: x + width must not wrap
        out.append(_frame_case(big[::-1], wins[::-1], -10.0, flags))
        sizes = [(10, 10, 0, 20), (10, 10, 20, 0), (10, 10, -5, 20), (10, 10, 20, -5), (10, 10, I32_MIN, I32_MIN), (12, 12, 6, 6), (0, 0, 0, 0)]
        faces = [(12.0, 12.0, 6.0, 6.0, 1.0, 1), (10.0, 10.0, -4.0, 8.0, 2.0, 1), (10.0, 10.0, 0.0, 0.0, 3.0, 1), (11.5, 11.5, 4.0, 4.0, 1.0, 1)]
        out.append(_frame_case(faces, sizes, -10.0, flags))       # negative and zero sizes on either side: no overlap, a window not live
        conf = [(0.0, 0.0, 8.0, 8.0, nan, 3), (8.0, 0.0, 8.0, 8.0, inf, 1), (16.0, 0.0, 8.0, 8.0, -inf, 1), (24.0, 0.0, 8.0, 8.0, inf, 2),
                (32.0, 0.0, 8.0, 8.0, 1.0, 0), (40.0, 0.0, 8.0, 8.0, 1.0, -1), (48.0, 0.0, 8.0, 8.0, -10.0, 1)]
        w8 = [(24, 0, 8, 8), (0, 0, 8, 8), (8, 0, 8, 8)]
        for thr in (-10.0, -inf, inf, 1e308):                     # NaN never eligible; -inf only above a threshold of -inf ... not even then
            out.append(_frame_case(conf, w8, thr, flags))
        face = [(23.35, 31.88, 42.66, 42.66, 8.5, 9)]
        for collected in (0, 1):                                  # each way of being not final
            out += [_frame_case(face, w8, -10.0, flags, status=OVER_CAP, collected=collected), _frame_case(face, w8, -10.0, flags, status=2, collected=collected),
                    _frame_case(face, w8, -10.0, flags, nhits=11, cap=10, collected=collected), _frame_case(face, w8, -10.0, flags, nhits=10, cap=10, collected=collected),
                    _frame_case(face, w8, -10.0, flags, bad=1, collected=collected)]
        full = [(8.0 * i, 0.0, 8.0, 8.0, 1.0 + (i % 3), 1) for i in range(40)]
        out.append(_frame_case(full, [(8 * (39 - j), 0, 8, 8) for j in range(16)], -10.0, flags))   # k = 16, every slot matched
        out.append(_frame_case(full, [(0, 0, 320, 8)] * 16, -10.0, flags))                           # sixteen equal windows: ties everywhere
    return out


def _plan_case(pairs, grouped, thr, flags):
    blob = struct.pack("<i2iIid", 2, len(pairs), grouped, flags, 0, float(thr))
    blob += b"".join(struct.pack("<2i", *p) for p in pairs)
    return blob, fc.plan(pairs, grouped, thr, flags)


def _plan_cases():
    """the header's own refusals; the rules it shares with ht_camshift_init_pairs live in csp_plan and are refused on the GPU"""
    ok = [(5, 0), (0, 1), (3, 0), (1, 3), (4, 1), (2, 0)]
    sixteen = [(s, 2) for s in range(16)]
    out = [_plan_case(ok, 4, -10.0, 0), _plan_case(ok, 4, 5.0, ASSOC), _plan_case(sixteen, 3, -10.0, ASSOC), _plan_case(sixteen + [(16, 1)], 3, float("inf"), 0),
           _plan_case([(7, 3)], 4, float("-inf"), 0)]
    refusals = {
        "flags": _plan_case(ok, 4, -10.0, 2), "flags>": _plan_case(ok, 4, -10.0, 0x80000001), "nan": _plan_case(ok, 4, float("nan"), 0),
        "outside": _plan_case([(0, 0), (1, 3)], 3, -10.0, 0), "outside<": _plan_case([(0, 0), (1, -1)], 3, -10.0, 0),
        "slots": _plan_case(sixteen + [(16, 2)], 3, -10.0, 0),
    }
    for name, (_b, (why, _t)) in refusals.items():
        assert why == name.rstrip("<>"), (name, why)
    return out + list(refusals.values())


def test_header_gives_the_restatements_records(harness, tmp_path):
    frames = _random_frames(20000) + _extreme_frames()
    plans = _plan_cases()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(b"".join(c[0] for c in frames) + b"".join(c[0] for c in plans))
    r = subprocess.run([harness, fin, fout], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    nref = sum(1 for c in plans if c[1][0] is not None)
    assert r.returncode == 0 and r.stdout.strip() == f"frames {len(frames)} plans {len(plans)} refused {nref}", (r.returncode, r.stdout, r.stderr[-3000:])
    assert nref == 6
    got = np.fromfile(fout, dtype=np.int32)
    pos = 0
    seen = {"codes": set(), "dropped": 0}
    for i, (_blob, want) in enumerate(frames):
        rec = got[pos:pos + 8 * len(want)].reshape(-1, 8)
        pos += 8 * len(want)
        have = [(int(r[0]), int(r[1]), tuple(int(v) for v in r[2:6]), int(r[6])) for r in rec]
        assert have == want and not rec[:, 7].any(), (i, have, want)
        seen["codes"] |= {w[0] for w in want}
        seen["dropped"] += want[0][3] > 0
    for i, (_blob, (why, table)) in enumerate(plans):
        st, ng = int(got[pos]), int(got[pos + 1])
        pos += 2
        if why is not None:
            assert (st, ng) == (native.HT_ERR_INVALID, 0), (i, why, st, ng)
            continue
        groups, order = table
        assert st == 0 and ng == len(groups), (i, st, ng)
        assert [tuple(int(v) for v in got[pos + 3 * g:pos + 3 * g + 3]) for g in range(ng)] == groups
        pos += 3 * ng
        assert [int(v) for v in got[pos:pos + len(order)]] == order
        pos += len(order)
    assert pos == len(got)
    assert seen["codes"] == {fc.UNTOUCHED, fc.FACE, fc.DEFERRED} and seen["dropped"] > 1000


def test_random_frames_are_full_of_ties():
    """the condition on the generator: equal confidences among the kept faces and equal best overlaps occur in most frames"""
    conf_ties = ov_ties = 0
    for blob, _want in _random_frames(300):
        k, m, flags = struct.unpack_from("<2iI", blob, 4)
        thr = struct.unpack_from("<d", blob, 36)[0]
        faces = [struct.unpack_from("<5d2i", blob, 44 + 48 * i)[:6] for i in range(m)]
        wins = [struct.unpack_from("<4i", blob, 44 + 48 * m + 16 * j) for j in range(k)]
        el = [f for f in faces if f[5] > 0 and f[4] > thr]
        conf_ties += len({f[4] for f in el}) < len(el)
        ovs = [fc.overlap(w, fc.floor_rect(f)) for w in wins for f in el]
        pos = [o for o in ovs if o > 0]
        ov_ties += len(set(pos)) < len(pos)
    assert conf_ties > 200 and ov_ties > 150, (conf_ties, ov_ties)


# ---- the build and the Python layer -------------------------------------------------------------------------------------------------------

def test_resolve_kernel_resources_and_code_object():
    import importlib.util

    from headtrackr_amd import build
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_csf_resolve" in o]
    assert len(mine) == 1 and b"k_csb_resolve" in mine[0] and b"k_csp_init" in mine[0]
    assert "ht_cs_faces.hip" not in build.HIP_SOURCES
    pairs_src = open(os.path.join(CSRC, "ht_cs_pairs.hip")).read()
    assert pairs_src.index('#include "ht_cs_best.hip"') < pairs_src.index('#include "ht_cs_faces.hip"')
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    r = res["k_csf_resolve"]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] <= 4096 and r["max_flat_workgroup_size"] == 64, r
    # the three recorded units are what profiles/traffic.json recorded
    from benchlib import fingerprint

    for marker in fingerprint.UNITS.values():
        assert marker.decode() not in "k_csf_resolve"
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])


def test_python_layer_binds_the_new_entry_points():
    from headtrackr_amd import build
    from headtrackr_amd.api import Context

    build.build_lib()
    L = native.lib()
    for name in ("ht_camshift_init_faces", "ht_camshift_init_faces_result"):
        assert hasattr(L, name) and name in native.SYMBOLS
    assert L.ht_camshift_init_faces(None, None, 0, 0.0, 0) == -1 and L.ht_camshift_init_faces_result(None, 0, None) == -1
    assert callable(Context.camshift_init_faces) and callable(Context.camshift_init_faces_result)
    hdr = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    assert f"enum {{ HT_CSF_ASSOCIATE = {native.HT_CSF_ASSOCIATE} }};" in hdr and f"#define HT_CSF_MAX_SLOTS {native.HT_CSF_MAX_SLOTS}\n" in hdr
    assert native.HT_CSF_MAX_SLOTS == fc.MAX_SLOTS == 16 and native.CSF_RECORD_DTYPE.itemsize == 32
    assert "int32_t code, face;" in hdr and "int32_t dropped, reserved;" in hdr
    assert list(native.CSF_RECORD_DTYPE.names) == ["code", "face", "x", "y", "width", "height", "dropped", "reserved"]


# ---- the N-API shim and the JavaScript layer ------------------------------------------------------------------------------------------------

NEW_EXPORTS = ("ht_camshift_init_faces", "ht_camshift_init_faces_result")
JS_CALLS = ("camshiftInitFaces", "camshiftInitFacesResult")
NODE = shutil.which("node")
HAVE_NODE = NODE is not None and os.path.exists("/usr/include/node/node_api.h")


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_exports_the_new_calls_and_refuses_malformed_arguments():
    from headtrackr_amd import build

    addon = build.build_addon()
    assert addon is not None
    js = ("const A = require(%r); const out = [typeof A.camshiftInitFaces, typeof A.camshiftInitFacesResult, A.CSF_ASSOCIATE, A.CSF_MAX_SLOTS];"
          " [[], [{}], [{}, new Int32Array(2)]].forEach(function (a) { try { A.camshiftInitFaces.apply(null, a); out.push('silent'); }"
          " catch (e) { out.push(e instanceof TypeError ? 'TypeError' : 'Error'); } }); try { A.camshiftInitFacesResult({}); out.push('silent'); } catch (e)"
          " { out.push(e instanceof TypeError ? 'TypeError' : 'Error'); } console.log(JSON.stringify(out));" % addon)
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function", "function", native.HT_CSF_ASSOCIATE, native.HT_CSF_MAX_SLOTS] + ["TypeError"] * 4
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "addon_args.js")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert not set(out["silent"]) & set(JS_CALLS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_still_loads_against_a_c_abi_without_the_new_symbols(tmp_path):
    """tests/js/abi_stub.cc defines neither export: the shim calls them directly, so the addon linked against the stub loads and
    reproduces its recorded transcript unchanged"""
    import addon_stub

    got = addon_stub.run(addon_stub.NAPI_SRC, tmp_path)
    assert got["transcript"] == json.load(open(addon_stub.GOLDEN))
    src = open(addon_stub.NAPI_SRC).read()
    for sym in NEW_EXPORTS:
        assert ("&" + sym) not in src and sym + "(" in src
    assert not any(sym in open(os.path.join(ROOT, "tests", "js", "abi_stub.cc")).read() for sym in NEW_EXPORTS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_js_init_faces_on_the_cpu_mock(tmp_path, cascade):
    """ccv.DeviceBatch.initFaces / initFacesResult on the oracle-backed mock: the Python restatement's records for a rank-order call and an
    associate call that is not the rank order; a deferred frame retried once after the collect; the refusals, grouping 'host' among them"""
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    job = fc.js_job(tmp_path, cascade.blob)
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "init_faces_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] == 13 and out["deferred"] == out["retried"] == 3 and out["reread"] == 1 and out["refusals"] == 6

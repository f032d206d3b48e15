"""CPU side of the (stream, frame) pair calls (ht_camshift_init_pairs / ht_camshift_track_pairs): the inputs of tests/pair_cases.py are
proved, from the oracle alone, to be inputs on which the reference does not depend on the summation order and loses no object — so
tests/test_gpu_camshift_pairs.py may demand the oracle's integers on every call —, the oracle is pinned to a recording of several
reference camshift.Tracker instances on one canvas, the new entry points exist at every layer, the new kernels live in the fourth code
object within their budgets, and the JavaScript layer runs on the oracle-backed mock addon.  No compute calls (no GPU here)."""
import importlib.util
import json
import os
import re
import shutil
import subprocess

import pytest

import cs_cases as cc
import pair_cases as pc
from conftest import ROOT, load_golden
from headtrackr_amd import build, native

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NODE = shutil.which("node")
NEW_KERNELS = ("k_csp_hist", "k_csp_meanshift", "k_csp_init")
NEW_SYMBOLS = ("ht_camshift_init_pairs", "ht_camshift_track_pairs")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------------

def _flat(per_seq):
    return [(si, j, k, call) for si, trackers in enumerate(per_seq) for j, calls in enumerate(trackers) for k, call in enumerate(calls)]


def test_no_multi_tracker_sequence_loses_an_object():
    """every call of every tracker of every sequence: width > 0, height > 0, a non-empty next search window"""
    seqs = pc.all_multi_sequences()
    n = 0
    for s in seqs:
        for j, calls in enumerate(s.oracle_calls()):
            assert len(calls) == s.ncalls
            for k, (_b, sw, to) in enumerate(calls):
                assert to["width"] > 0 and to["height"] > 0 and sw[2] > 0 and sw[3] > 0, (s.name, j, k, to, sw)
                n += 1
    assert n == 6 * 3 * 4 + 2 * 2 * 4 + 50 * 4 * 2 + 2 * 2 + 3 * 8


def test_every_multi_tracker_sequence_is_insensitive_to_the_summation_order():
    """the method of tests/test_cs_cases_cpu.py: the oracle under the three order variants returns the same track object and search
    window on every call — zero order-sensitive calls, two same-coloured blobs on one frame included"""
    seqs = pc.all_multi_sequences()
    ref = [s.oracle_calls() for s in seqs]
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            alt = [s.oracle_calls() for s in seqs]
        bad = [(seqs[si].name, j, k, flag) for (si, j, k, a), (_si, _j, _k, b) in zip(_flat(ref), _flat(alt)) if not cc.same_call(a, b)]
        assert not bad, bad
    assert ref == [s.oracle_calls() for s in seqs]  # the real oracle is bound again


def test_multi_blob_frames_are_what_they_are_built_from():
    """inside blob j's rect the frame is blob_frame's, far from every blob it is the noise frame's; the same-coloured blobs share their
    colour bins; the 1080p windows are beyond the LDS region (the uncached path), the others inside it"""
    from headtrackr_amd import synth

    s = pc.feed_scene(0)
    base = synth.noise_frame(s.w, s.h, s.seeds[0])
    for (cx, cy, a, b, rot, col) in s.blobs[0]:
        bf = synth.blob_frame(s.w, s.h, cx, cy, a, b, rot, col, s.seeds[0])
        assert (s.frames[0][cy, cx] == bf[cy, cx]).all() and (bf[cy, cx] != base[cy, cx]).any()
    assert (s.frames[0][0, 0] == base[0, 0]).all()
    assert len({bl[5] for bl in s.blobs[0]}) == 3  # three colours on one frame
    for w, h in pc.SAME_COLOUR_SIZES:
        t = pc.same_colour(w, h)
        assert t.blobs[0][0][5] == t.blobs[0][1][5]
        m0, m1 = (cc.model_histogram(t.frames[0], r) for r in t.rects)
        assert ((m0 > 0) & (m1 > 0)).sum() >= 4  # both models match both blobs: only the search windows tell the trackers apart
    assert 641 % 4 != 0
    big = pc.large_1080p()
    for calls in big.oracle_calls():
        for (b, _sw, _to) in calls:
            assert cc.region_rect(big.w, big.h, b) is None
    for calls in pc.feed_scene(3).oracle_calls():
        for (b, _sw, _to) in calls:
            assert cc.region_rect(320, 240, b) is not None


def test_scattered_streams_have_gaps_and_the_pair_order_changes():
    st = pc.scattered_streams(18, 40, 9111)
    assert len(set(st)) == 18 and max(st) < 40 and st != sorted(st) and sorted(st) != list(range(18))
    orders = [pc.shuffled(18, 9200 + k) for k in range(1, 5)]
    assert all(sorted(o) == list(range(18)) for o in orders) and len({tuple(o) for o in orders}) == 4


def test_loop_scenario_loses_exactly_the_planned_feeds_at_the_planned_steps(cascade):
    """four independent per-feed loops on the oracle (VJ until confidence > -10, initTracker on the floored rect, CS until width or
    height is 0, VJ again): the planned feeds are lost at the planned steps and nowhere else, they find their face again two steps later,
    and at some step one feed detects while three track"""
    L = pc.loop_oracle(cascade.blob)
    assert len(L) == pc.LOOP_FEEDS == 4 and all(len(r) == pc.LOOP_STEPS for r in L)
    lost = {(f, k) for f, recs in enumerate(L) for k, r in enumerate(recs) if r["mode"] == "CS" and r["lost"]}
    assert lost == set(pc.LOOP_LOST.items()) and len(lost) == 2
    assert len(set(pc.LOOP_LOST.values())) == 2  # at different steps
    for f, recs in enumerate(L):
        assert recs[0]["mode"] == "VJ" and recs[0]["found"]
        if f in pc.LOOP_LOST:
            k = pc.LOOP_LOST[f]
            assert recs[k]["to"]["width"] == 0 and recs[k]["to"]["height"] == 0
            assert recs[k + 1]["mode"] == "VJ" and not recs[k + 1]["found"]          # no face yet: nothing is initialised
            assert recs[k + 2]["mode"] == "VJ" and recs[k + 2]["found"]              # the face is back two steps later
            assert all(r["mode"] == "CS" and not r["lost"] for r in recs[k + 3:]) and len(recs[k + 3:]) >= 2
        else:
            assert all(r["mode"] == "CS" and not r["lost"] for r in recs[1:])
    modes = [[L[f][k]["mode"] for f in range(4)] for k in range(pc.LOOP_STEPS)]
    assert any(m.count("VJ") == 1 and m.count("CS") == 3 for m in modes)


def test_loop_scenario_is_insensitive_to_the_summation_order(cascade):
    """every CS call of the loop outside the two lost ones passes the order check; the lost calls are 0 x 0 under every order"""
    ref = pc.loop_oracle(cascade.blob)
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            alt = [pc.loop_feed_oracle(f, cascade.blob) for f in range(pc.LOOP_FEEDS)]
        for f, (ra, rb) in enumerate(zip(ref, alt)):
            for k, (a, b) in enumerate(zip(ra, rb)):
                assert a["mode"] == b["mode"], (f, k, flag)
                if a["mode"] == "VJ":
                    assert a["found"] == b["found"] and a["best"] == b["best"], (f, k, flag)
                elif a["lost"]:
                    assert b["lost"] and b["to"]["width"] == 0 and b["to"]["height"] == 0 and list(a["sw"]) == list(b["sw"]), (f, k, flag)
                else:
                    assert cc.same_call((a["before"], a["sw"], a["to"]), (b["before"], b["sw"], b["to"])), (f, k, flag)


def test_oracle_reproduces_the_recorded_multi_tracker_runs():
    """tests/golden/multitrack.json: three reference camshift.Tracker instances on one canvas over 5 frames of a three-blob scene, and two
    on two blobs of one colour.  The per-stream oracle gives the recorded integers; the angle as tests/test_oracle_golden.py compares it"""
    g = load_golden("multitrack.json")
    assert [len(c["trackers"]) for c in g["cases"]] == [3, 2] and all(len(c["gen"]) == 5 for c in g["cases"])
    for c in g["cases"]:
        s = pc.seq_from_specs(c["name"], c["w"], c["h"], c["gen"])
        assert [list(r) for r in s.rects] == c["rects"]
        for j, calls in enumerate(s.expected()):
            assert len(calls) == len(c["trackers"][j]) == 4
            for k, (sw, to) in enumerate(calls):
                r = c["trackers"][j][k]
                assert list(sw) == r["sw"], (c["name"], j, k)
                for q in ("x", "y", "width", "height"):
                    assert to[q] == r[q], (c["name"], j, k, q)
                assert abs(to["angle"] - r["angle"]) <= 1e-12
    # and they are the sequences the GPU tests use
    assert pc.feed_scene(0).specs() == g["cases"][0]["gen"] and pc.same_colour(320, 240).specs() == g["cases"][1]["gen"]


# ---- the entry points at every layer ----------------------------------------------------------------------------------------------------------

def test_new_symbols_exist_at_every_layer():
    build.build_lib()
    L = native.lib()
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    napi = open(os.path.join(CSRC, "ht_napi.cc")).read()
    exported = set(re.findall(r'\{"(\w+)",\s*\w+\}', napi))
    for name, js in zip(NEW_SYMBOLS, ("camshiftInitPairs", "camshiftTrackPairs")):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in native.SYMBOLS
        row = re.search(r"^\| `%s` \|.*\| ([^|]*) \|$" % name, doc, flags=re.M)
        assert row and js in row.group(1), name
        assert js in exported
    assert "typedef struct ht_cs_pair { int32_t stream, frame; } ht_cs_pair;" in header
    assert native.PAIR_DTYPE.itemsize == 8 and native.PAIR_DTYPE.names == ("stream", "frame")
    assert L.ht_abi_version() == 2
    # all-zero arguments: a status, never a crash
    assert L.ht_camshift_init_pairs(None, None, 0, None) == -1 and L.ht_camshift_track_pairs(None, None, 0, 0, None) == -1
    from headtrackr_amd.api import Context

    assert callable(Context.camshift_init_pairs) and callable(Context.camshift_track_pairs)
    js = open(os.path.join(ROOT, "headtrackr_amd", "js", "headtrackr.js")).read()
    for m in ("this.initPairs", "this.trackPairs", "this.trackPairsEnqueue", "headtrackr.camshift.MultiTracker", "opts.trackers", "sel.feeds"):
        assert m in js, m


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_addon_exports_the_pair_calls_and_refuses_malformed_arguments():
    build.build_lib()
    addon = build.build_addon()
    js = ("const A = require(%r); const r = [typeof A.camshiftInitPairs, typeof A.camshiftTrackPairs];"
          "for (const f of [A.camshiftInitPairs, A.camshiftTrackPairs]) for (const args of [[], [1], [{}, new Int32Array(2)], [null, 3, 4, 5]])"
          "{ try { f.apply(null, args); r.push('no throw'); } catch (e) { r.push(e instanceof TypeError ? 'TypeError' : String(e)); } }"
          "console.log(JSON.stringify(r));" % addon)
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function", "function"] + ["TypeError"] * 8


def test_cs_pairs_force_is_an_option_of_the_product_library():
    """checked by source, like the other keys without a device: the parser knows the key, the header lists it with the result-preserving
    keys, and it is not behind HT_DEBUG_KNOBS"""
    src = open(os.path.join(CSRC, "ht_context.hip")).read()
    parser = src[src.index("static bool apply_options"):src.index('extern "C" ht_status ht_create')]
    product, _sep, knobs = parser.partition("#ifdef HT_DEBUG_KNOBS")
    assert 'key == "cs_pairs_force"' in product and "cs_pairs_force" not in knobs
    header = open(os.path.join(ROOT, "include", "headtrackr_hip.h")).read()
    assert "cs_pairs_force=1" in header[header.index("const char *options;"):header.index("} ht_config;")]
    build.build_lib()
    assert b"cs_pairs_force" in open(build.LIB, "rb").read()


# ---- the kernels --------------------------------------------------------------------------------------------------------------------------

def test_pair_kernels_live_in_the_fourth_code_object_within_their_budgets():
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_csp_meanshift" in o]
    assert len(mine) == 1 and b"k_csp_hist" in mine[0] and b"k_csp_init" in mine[0] and b"k_bp_project" in mine[0]
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0], marker
        for k in NEW_KERNELS:
            assert marker.decode() not in k
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in NEW_KERNELS:
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
    assert res["k_csp_meanshift"]["vgpr_count"] <= res["k_cs_meanshift"]["vgpr_count"]
    # the same workgroups as the kernels they mirror: same wavefront count = same summation order
    for mine_k, theirs in (("k_csp_meanshift", "k_cs_meanshift"), ("k_csp_hist", "k_cs_hist"), ("k_csp_init", "k_cs_init")):
        assert res[mine_k]["max_flat_workgroup_size"] == res[theirs]["max_flat_workgroup_size"], mine_k
        assert res[mine_k]["group_segment_fixed_size"] == res[theirs]["group_segment_fixed_size"], mine_k
    assert "ht_backproject.hip" not in build.EXTRA_FLAGS  # the unit is compiled without -disable-machine-licm
    assert '#include "ht_cs_pairs.hip"' in open(os.path.join(CSRC, "ht_backproject.hip")).read()
    assert "ht_cs_pairs.hip" not in build.HIP_SOURCES


def _included(text):
    return re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M)


def _times_seen(unit, header, texts):
    """how often the translation unit `unit` sees `header`, directly or through the files it includes"""
    return sum(1 if inc == header else _times_seen(inc, header, texts) for inc in _included(texts[unit]) if inc in texts)


def test_shared_helpers_have_one_definition():
    """the device helpers live in ht_cs_device.h and the init / histogram / mean-shift kernels in ht_cs_kernels.inc; ht_camshift.hip and
    ht_cs_pairs.hip define none of them again, and each translation unit sees the header exactly once"""
    texts = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".inc", ".hip", ".cc"))}
    hdr = texts["ht_cs_device.h"]
    units = [texts[f] for f in ("ht_camshift.hip", "ht_cs_pairs.hip")]
    for sig in ("void hist_add_wave(", "int32_t toint32(", "struct Mom {", "double wave_sum_f64(", "struct CsRegion {", "CsRegion cs_cache_region(",
                "Mom window_moments(", "Mom window_moments_any(", "void meanshift_body(", "#define CS_BATCH_LOADED", "uint32_t cs_bin(uint32_t px) {"):
        assert hdr.count(sig) == 1, sig
        assert sum(t.count(sig) for t in texts.values()) == 1, sig
        for u in units:
            assert sig not in u, sig
    # the three kernel bodies: one __global__ definition each in all of csrc/, in the shared file, under the name the unit gives it
    kern = re.compile(r"__global__[^;{]*?\b(k_csp?_(?:hist|meanshift|init)|CS_K\((?:hist|meanshift|init)\))\s*\(")
    found = {f: kern.findall(t) for f, t in texts.items()}
    assert sorted(found.pop("ht_cs_kernels.inc")) == ["CS_K(hist)", "CS_K(init)", "CS_K(meanshift)"]
    assert not any(found.values()), found
    for f in ("ht_camshift.hip", "ht_cs_pairs.hip"):
        assert "ht_cs_kernels.inc" in _included(texts[f]) and re.search(r"#define CS_K\(name\) k_csp?_##name\n", texts[f]), f
    # each translation unit sees the header exactly once, directly or through the file it is included by
    assert "ht_cs_pairs.hip" in _included(texts["ht_backproject.hip"]) and "ht_cs_pairs.hip" not in build.HIP_SOURCES
    for tu in build.HIP_SOURCES:
        uses = any(n in texts[tu] or any(n in texts[i] for i in _included(texts[tu]) if i in texts) for n in ("cs_bin(", "CS_BATCH_LOADED("))
        assert _times_seen(tu, "ht_cs_device.h", texts) == (1 if uses else 0), tu
    assert _times_seen("ht_camshift.hip", "ht_cs_device.h", texts) == _times_seen("ht_backproject.hip", "ht_cs_device.h", texts) == 1


# ---- the JavaScript layer on the mock -------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not installed")
def test_js_pair_layer_on_the_cpu_mock(tmp_path, cascade):
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    job = pc.js_job(tmp_path, cascade.blob, load_golden("multitrack.json"))
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "pairs_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    loop_cs = sum(1 for recs in job["loop"]["expect"] for e in recs if e["mode"] == "CS")
    assert out["calls_total"] == out["calls_exact"] == 6 * 4 + loop_cs + (3 + 2) * 4
    assert out["loop_lost"] == 2 and out["loop_mixed_steps"] >= 1 and out["multi_done"] == 2
    assert out["loop_detects"] == sum(1 for recs in job["loop"]["expect"] for e in recs if e["mode"] == "VJ")
    assert out["pair_calls"][0] >= 4 and out["pair_calls"][1] >= 4 + 8
    assert out["missing_checks"] == 4
    # a DeviceBatch used without the new options: the addon calls it made before this feature, no more and no fewer
    assert out["legacy_calls"] == {"createContext": 1, "setGeometry": 1, "deviceAlloc": 1, "deviceUpload": 1, "bindDevice": 3, "detectEnqueue": 1,
                                   "collectBest": 1, "camshiftReserve": 1, "camshiftInitBound": 1, "camshiftTrackBound": 2,
                                   "camshiftTrackCollect": 2, "deviceFree": 1, "destroy": 1}

"""CPU-side checks of the device grouping (ht_group.hip): every synthetic hit list of tests/group_cases.py reaches the state it is named
after — proven from oracle.ht_oracle alone, the full-workgroup, over-cap and > 1024-frame cases and the scan batches included —, the host part of the route (ht_group_plan.h) runs under AddressSanitizer + UBSan in a
stand-alone harness and equals the oracle, the new entry points exist at every layer, and the new kernels sit in the fourth code object
within their budgets.  No compute calls (no GPU here)."""
import importlib.util
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import group_cases as gc
from conftest import ROOT, load_golden
from headtrackr_amd import build, native
from oracle import ht_oracle as ho

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
NEW_KERNELS = ("k_grp_bucket", "k_grp_frames<64>", "k_grp_frames<1024>")
NEW_EXPORTS = ("ht_detect_best_enqueue", "ht_detect_best_collect", "ht_detect_best_collect_requeue", "ht_detect_grouped",
               "ht_detect_best_records_device", "ht_group_hits")


NODE = shutil.which("node")
HAVE_NODE = NODE is not None and os.path.exists("/usr/include/node/node_api.h")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the cases are what their names say -----------------------------------------------------------------------------------------------


def _adjacency(seq):
    n = len(seq)
    adj = [[] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if gc.similar(seq, i, j):
                adj[i].append(j)
                adj[j].append(i)
    return adj


def test_chain_is_one_component_that_plain_label_propagation_needs_20_rounds_for():
    seq = gc.frame_seq(gc.cases()["chain"]["hits"], 0)
    n = len(seq)
    assert n >= 40
    adj = _adjacency(seq)
    deg = sorted(len(a) for a in adj)
    assert deg == [1, 1] + [2] * (n - 2)  # only neighbours are similar: a path
    g = ho.group(seq, 1)
    assert len(g) == 1 and g[0]["neighbors"] == n  # one component
    lab, rounds = list(range(n)), 0
    while True:  # plain (Jacobi) min-label propagation until nothing changes
        new = [min([lab[i]] + [lab[j] for j in adj[i]]) for i in range(n)]
        if new == lab:
            break
        lab, rounds = new, rounds + 1
    assert lab == [0] * n and rounds >= 20, rounds
    # and the path does not run along the emission order: label 0 has to travel through larger indices to reach smaller ones
    assert any(abs(i - j) > 1 for i in range(n) for j in adj[i])


def _averaged(vals, n):
    s = np.float64(0.0)
    for v in vals:
        s = s + np.float64(v)
    return (s * 2 + n) / (2 * n)


def test_interleaved_classes_alternate_and_their_sums_depend_on_the_order():
    seq = gc.frame_seq(gc.cases()["interleaved"]["hits"], 0)
    n = len(seq)
    adj = _adjacency(seq)
    comp = list(range(n))
    for _ in range(n):
        comp = [min([comp[i]] + [comp[j] for j in adj[i]]) for i in range(n)]
    ids = sorted(set(comp))
    assert len(ids) == 2
    switches = sum(1 for i in range(1, n) if comp[i] != comp[i - 1])
    assert switches >= 5  # the members alternate in emission order (level-major), block by block
    g = ho.group(seq, 1)
    assert len(g) == 2
    changed = False
    for k, cid in enumerate(ids):
        members = [i for i in range(n) if comp[i] == cid]
        assert g[k]["neighbors"] == len(members)
        for fld in ("x", "y", "width", "height"):
            fwd = _averaged([seq[i][fld] for i in members], len(members))
            rev = _averaged([seq[i][fld] for i in reversed(members)], len(members))
            assert fwd == g[k][fld]  # ascending member order from 0 is what the reference computes (ccv.js:274-289) ...
            changed |= fwd != rev
    assert changed  # ... and the reversed order gives other bits


def test_nested_second_pass_drops_with_the_neighbour_threshold_of_three_on_both_sides():
    hits = gc.cases()["nested"]["hits"]
    want = {0: (4, 3, True), 1: (3, 2, True), 2: (3, 3, False), 3: (4, 4, False)}  # (large class, small class, small one dropped)
    for f, (nb, ns, dropped) in want.items():
        seq = gc.frame_seq(hits, f)
        big, small = seq[seq["width"] > 40], seq[seq["width"] < 40]
        assert (len(big), len(small)) == (nb, ns)
        gb, gs = ho.group(big, 1), ho.group(small, 1)
        assert len(gb) == 1 and len(gs) == 1 and gb[0]["neighbors"] == nb and gs[0]["neighbors"] == ns
        assert gs[0]["x"] > gb[0]["x"] and gs[0]["x"] + gs[0]["width"] < gb[0]["x"] + gb[0]["width"]  # inside
        g = ho.group(seq, 1)
        assert len(g) == (1 if dropped else 2), f
        assert gs[0]["confidence"] > gb[0]["confidence"]  # the dropped rect would have been the best face
        best = gc.expected("nested", 1)[0][f]
        assert best["neighbors"] == (nb if dropped else ns)


def test_size_overflow_and_layout_cases_have_the_stated_shapes():
    cs = gc.cases()
    assert [int((cs["sizes"]["hits"]["frame"] == f).sum()) for f in range(len(gc.SIZES))] == list(gc.SIZES) == [0, 1, 63, 64, 65, 256, 257]
    assert set(cs["sizes"]["min_neighbors"]) == set(cs["one_frame"]["min_neighbors"]) == {0, 1, 2, 3}
    assert cs["sizes_in_order"]["hits"].tobytes() != cs["sizes"]["hits"].tobytes()
    assert sorted(cs["sizes_in_order"]["hits"].tolist()) == sorted(cs["sizes"]["hits"].tolist())
    f = cs["sizes"]["hits"]["frame"]
    assert (np.diff(f.astype(np.int64)) < 0).any()  # shuffled across frames
    assert {cs[k]["nframes"] for k in ("one_frame", "last_frame_only", "frames_257")} == {1, 2, 257}
    for k in ("last_frame_only", "last_of_257_only"):
        assert set(cs[k]["hits"]["frame"].tolist()) == {cs[k]["nframes"] - 1}
    ov = cs["overflow"]
    assert ov["options"] == "group_cap=64" and [int((ov["hits"]["frame"] == f).sum()) for f in range(3)] == [64, 65, 9]
    for name, c in cs.items():
        h = c["hits"]
        assert np.isfinite(h["sum"]).all() and (h["frame"] < c["nframes"]).all() and (h["scale"] < 27).all(), name
        assert len({(a, b, q, y, x) for a, b, q, y, x in zip(h["frame"].tolist(), h["scale"].tolist(), h["q"].tolist(), h["y"].tolist(), h["x"].tolist())}) == len(h)
    # every grouping outcome occurs somewhere: frames without a face, with one, with several, and a min_neighbors filter that bites
    ng = np.concatenate([gc.expected(n, m)[2] for n, m in gc.case_ids()])
    assert (ng == 0).any() and (ng == 1).any() and (ng > 3).any()
    assert gc.expected("sizes", 3)[2].sum() < gc.expected("sizes", 1)[2].sum() < gc.expected("sizes", 0)[2].sum()


# ---- the full-workgroup cases: k_grp_frames<1024> at 511 .. 1024 hits, every launch width, the default cap, > 1024 frames ------------------

NEW_CASES = ("full_wide", "full_dense", "chains", "two_chains", "over_default_cap", "caps_128", "caps_256", "caps_512", "caps_300", "frames_1025",
             "frames_2500", "last_of_2500_only")


def _adjacency_matrix(seq):
    """ccv.js:252-261 in either direction on the oracle's seq rects, as one boolean matrix (gc.similar pair by pair is a million oracle
    calls at n = 1024): r2 is similar to r1 when it lies within floor(r1.width * 0.25 + 0.5) of it in x and y and the widths are within
    a factor of 1.5 of each other, both rounded as the reference rounds them"""
    x, y, w = seq["x"], seq["y"], seq["width"]
    d, w15 = np.floor(w * 0.25 + 0.5), np.floor(w * 1.5 + 0.5)
    p = ((x[None, :] <= (x + d)[:, None]) & (x[None, :] >= (x - d)[:, None]) & (y[None, :] <= (y + d)[:, None]) & (y[None, :] >= (y - d)[:, None])
         & (w[None, :] <= w15[:, None]) & (w15[None, :] >= w[:, None]))  # p[i, j]: r1 = i, r2 = j
    a = p | p.T
    np.fill_diagonal(a, False)
    return a


def _kernel_rounds(adj):
    """the kernel's label rounds in plain numpy: every rect takes the minimum label over itself and its similar rects, then jumps once
    through the labels of the round's start; (final labels, rounds in which a label changed)"""
    n = len(adj)
    lab, rounds = np.arange(n), 0
    while rounds <= n:
        m = np.minimum(lab, np.where(adj, lab[None, :], n).min(axis=1))
        new = lab[m]
        if np.array_equal(new, lab):
            break
        lab, rounds = new, rounds + 1
    return lab, rounds


def _component_sizes(adj):
    lab, _ = _kernel_rounds(adj)
    roots = np.unique(lab)
    assert np.array_equal(lab[roots], roots)  # every label is its class's smallest member
    return np.sort(np.bincount(lab, minlength=len(adj))[roots])[::-1]


def test_adjacency_matrix_is_the_oracles_pair_predicate():
    """the vectorised predicate against oracle.group on pairs: every pair of the 65-hit chain and of a 129-hit blob frame, and seeded
    pairs of the 1024-hit frames"""
    cs = gc.cases()
    for name, f, pairs in (("chains", 0, None), ("caps_128", 3, None), ("full_dense", 0, 3000), ("full_wide", 4, 3000)):
        seq = gc.frame_seq(cs[name]["hits"], f)
        adj, n = _adjacency_matrix(seq), len(seq)
        if pairs is None:
            ij = [(i, j) for i in range(n) for j in range(i + 1, n)]
        else:
            r = np.random.default_rng(n).integers(0, n, size=(pairs, 2))
            near = np.argwhere(adj)[:: max(1, int(adj.sum()) // pairs)]  # and joined pairs, which a uniform draw seldom meets
            ij = [(int(i), int(j)) for i, j in np.concatenate([r, near]) if i != j]
        assert any(adj[i, j] for i, j in ij) and not all(adj[i, j] for i, j in ij)
        for i, j in ij:
            # (a class of two, not gc.similar's "one rect comes back": a rect nested in another one that is not similar to it is dropped
            # by ccv.js:307-330 and leaves one rect of one member)
            g = ho.group(seq[[i, j]], 1)
            assert bool(adj[i, j]) == (len(g) == 1 and g[0]["neighbors"] == 2), (name, f, i, j)


def test_full_workgroup_cases_have_the_stated_shapes():
    cs = gc.cases()
    assert list(cs)[-len(NEW_CASES):] == list(NEW_CASES)
    counts = {name: gc.frame_counts(name).tolist() for name in NEW_CASES}
    assert counts["full_wide"] == [511, 512, 513, 1023, 1024] and cs["full_wide"]["min_neighbors"] == (0, 1, 2, 3)
    assert counts["full_dense"] == [1024, 700] and cs["full_dense"]["min_neighbors"] == (1, 3)
    assert counts["chains"] == [65, 200, 513, 1024] and cs["chains"]["min_neighbors"] == (1, 2)
    assert counts["two_chains"] == [1024]
    assert counts["over_default_cap"] == [1024, 1025, 1500, 9] and cs["over_default_cap"]["min_neighbors"] == (0, 1, 2)
    assert cs["over_default_cap"]["options"] is None
    for cap in (128, 256, 512, 300):
        c = cs["caps_%d" % cap]
        assert counts["caps_%d" % cap] == [64, 65, 128, 129, 256, 257, 512, 513] and c["options"] == "group_cap=%d" % cap
        assert c["hits"].tobytes() == cs["caps_128"]["hits"].tobytes()  # one hit list
    for name, nfr in (("frames_1025", 1025), ("frames_2500", 2500)):
        n = np.array(counts[name])
        assert len(n) == nfr == cs[name]["nframes"] and n[1023] == 65 and n[1024] == 70
        rest = np.delete(n, [1023, 1024, 2300, 2499][: 2 if nfr == 1025 else 4])
        assert rest.max() == 3 and {0, 1, 2, 3} <= set(rest.tolist())
        empty_runs = [r for r in range(nfr // 37) if not n[37 * r: 37 * r + 37].any()]
        assert len(empty_runs) >= 3  # whole runs of frames without a hit
        assert n[:1024].sum() < n.sum() and n[-1] > 0  # the second pass of the bucket kernel's frame loop carries a start, to the last frame
    n = np.array(counts["frames_2500"])
    assert n[2300] == 200 and n[2499] == 30 and n[2048:].sum() > 230  # the third pass
    assert [k for k, v in enumerate(counts["last_of_2500_only"]) if v] == [2499] and cs["last_of_2500_only"]["nframes"] == 2500
    for name in NEW_CASES:
        h, nfr = cs[name]["hits"], cs[name]["nframes"]
        assert np.isfinite(h["sum"]).all() and (h["frame"] < nfr).all() and (h["scale"] < 27).all(), name
        assert (h["x"] < 1 << 16).all() and (h["y"] < 1 << 16).all() and (h["q"] < 4).all(), name  # the kernel's key fields
        keys = set(zip(h["frame"].tolist(), h["scale"].tolist(), h["q"].tolist(), h["y"].tolist(), h["x"].tolist()))
        assert len(keys) == len(h), name
        if name not in ("two_chains", "last_of_2500_only") and not name.startswith("caps_"):
            assert (np.diff(h["frame"].astype(np.int64)) < 0).any(), name  # arrival order: the frames interleaved


def test_cap_rule_and_the_frames_each_case_leaves_to_the_host():
    assert [gc.cap_of(o) for o in (None, "", "force_rccl=1", "group_cap=1024", "group_cap=5000")] == [1024] * 5
    assert [gc.cap_of("group_cap=%d" % n) for n in (-5, 0, 1, 64, 65, 127, 128, 255, 256, 300, 511, 512, 1023)] == \
        [64, 64, 64, 64, 64, 64, 128, 128, 256, 256, 256, 512, 512]  # (the rows of tests/host/group_harness.cc's plan checks among them)
    assert gc.cap_of("force_rccl=1,group_cap=300") == 256
    assert gc.over_cap_frames("overflow") == 1 and gc.over_cap_frames("overflow", None) == 0
    assert gc.over_cap_frames("over_default_cap") == 2  # 1025 and 1500; 1024 is a full workgroup, not one over the cap
    # more hits than the cap, counted by hand from 64, 65, 128, 129, 256, 257, 512, 513: a frame of exactly `cap` hits stays on the device
    assert [gc.over_cap_frames("caps_%d" % cap) for cap in (128, 256, 512, 300)] == [5, 3, 1, 3]
    assert gc.over_cap_frames("caps_128", None) == 0
    for name in gc.cases():
        if name not in ("overflow", "over_default_cap") and not name.startswith("caps_"):
            assert gc.over_cap_frames(name) == 0, name


def test_chains_are_paths_that_take_the_label_rounds_across_wavefronts():
    cs = gc.cases()
    for f, n in enumerate(gc.CHAIN_SIZES):
        seq = gc.frame_seq(cs["chains"]["hits"], f)
        assert len(seq) == n
        adj = _adjacency_matrix(seq)
        assert sorted(adj.sum(axis=1).tolist()) == [1, 1] + [2] * (n - 2)  # a path
        for mn in (1, 2):
            g = ho.group(seq, mn)
            assert len(g) == 1 and g[0]["neighbors"] == n  # one class of n members
        lab, rounds = _kernel_rounds(adj)
        assert not lab.any() and rounds <= n
        i, j = np.nonzero(adj)
        # (emission order is q-major: a 6-pixel step's two windows are half a frame apart)
        assert np.abs(i - j).max() > (64 if n > 128 else 16)  # neighbours in other wavefronts: label 0 travels through larger indices
        if n == 1024:
            assert rounds >= 8, rounds
    assert int(cs["chains"]["hits"]["x"].max()) == 1278  # fits the key's 16-bit field


def test_two_chains_are_two_components_the_second_rooted_far_from_index_zero():
    seq = gc.frame_seq(gc.cases()["two_chains"]["hits"], 0)
    adj = _adjacency_matrix(seq)
    lab, _ = _kernel_rounds(adj)
    assert sorted(np.bincount(lab)[np.unique(lab)].tolist()) == [500, 524]
    assert np.unique(lab)[0] == 0 and np.unique(lab)[1] >= 100  # the second class's smallest member
    g = ho.group(seq, 1)
    assert sorted(int(r["neighbors"]) for r in g) == [500, 524]


def test_full_wide_frames_have_many_components_of_every_size():
    cs = gc.cases()
    for f, n in enumerate(gc.FULL_WIDE_SIZES):
        seq = gc.frame_seq(cs["full_wide"]["hits"], f)
        sizes = _component_sizes(_adjacency_matrix(seq))
        assert sizes.sum() == n
        assert len(sizes) >= 30 and (sizes >= 3).sum() >= 20 and sizes[0] <= n // 4, (f, sizes)
        assert len(ho.group(seq, 1)) <= len(sizes)
        ng = [int(gc.expected("full_wide", mn)[2][f]) for mn in (1, 2, 3)]
        assert ng[0] > ng[1] > ng[2] > 0, (f, ng)
        assert int(gc.expected("full_wide", 0)[2][f]) == n
    # labels above 255 are roots of classes (the uint16 label array), and the nested-rect pass sees dozens of averaged rects
    seq = gc.frame_seq(cs["full_wide"]["hits"], 4)
    lab, _ = _kernel_rounds(_adjacency_matrix(seq))
    assert (np.unique(lab) > 255).sum() >= 10 and gc.expected("full_wide", 1)[2][4] >= 30


def test_full_dense_frame_is_one_long_class_and_strays():
    cs = gc.cases()
    for f, n in enumerate(gc.FULL_DENSE_SIZES):
        seq = gc.frame_seq(cs["full_dense"]["hits"], f)
        sizes = _component_sizes(_adjacency_matrix(seq))
        assert sizes.sum() == n and sizes[0] > n // 2 and len(sizes) >= 5, (f, sizes)
        if f == 0:
            assert sizes[0] > 512
            assert max(int(r["neighbors"]) for r in ho.group(seq, 1)) == sizes[0]  # one thread sums it in order


def test_scan_batches_crowd_a_frame_into_the_regimes_they_are_named_after(cascade):
    """from the oracle alone: the tiled 640x480 frame fills more than half of a 1024-thread workgroup, the 960x540 one is over the cap"""
    raw = gc.scan_raw("full_640x480", cascade.blob)
    assert [len(r) for r in raw] == [755, len(raw[1]), 0, 755] and 512 < len(raw[0]) <= 1024 and 0 < len(raw[1]) < 64
    _, lists = gc.scan_expected("full_640x480", cascade.blob, 1)
    assert [len(g) for g in lists] == [88, 1, 0, 88]
    raw = gc.scan_raw("over_960x540", cascade.blob)
    assert len(raw[0]) == 1473 and len(raw[0]) > 1024 and 0 < len(raw[1]) < 64
    assert [len(g) for g in gc.scan_expected("over_960x540", cascade.blob, 1)[1]] == [153, 1]
    for batch in gc.SCAN_BATCHES:  # what the scan emits: distinct keys per frame, in emission order
        for r in gc.scan_raw(batch, cascade.blob):
            keys = list(zip(r["scale"].tolist(), r["q"].tolist(), r["y"].tolist(), r["x"].tolist()))
            assert keys == sorted(set(keys))


# ---- the host part of the route under the sanitizers -------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("group") / "group_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread",
                           "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "host", "group_harness.cc"), "-o", exe])
    return exe


def _run_harness(exe, tmp_path, hits, nframes, min_neighbors):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.array([nframes, len(hits), min_neighbors, 5], dtype=np.int32).tobytes())
        fh.write(np.ascontiguousarray(hits).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    blob = open(fout, "rb").read()
    if not int(np.frombuffer(blob[:4], dtype=np.uint32)[0]):
        return None
    o = 4
    best = np.frombuffer(blob[o:o + 48 * nframes], dtype=native.RECT_DTYPE); o += 48 * nframes
    ng = np.frombuffer(blob[o:o + 4 * nframes], dtype=np.uint32); o += 4 * nframes
    return best, np.frombuffer(blob[o:], dtype=native.RECT_DTYPE), ng


@pytest.mark.parametrize("name,mn", gc.case_ids(), ids=lambda v: str(v))
def test_host_completion_under_asan_equals_the_oracle(harness, tmp_path, name, mn):
    """ht_grp_complete_frame is what finishes a frame the kernel flags: every case, every frame, byte for byte"""
    c = gc.cases()[name]
    got = _run_harness(harness, tmp_path, c["hits"], c["nframes"], mn)
    assert got is not None
    want = gc.expected(name, mn)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])


def test_host_completion_rejects_a_frame_outside_the_batch(harness, tmp_path):
    hits = gc.cases()["one_frame"]["hits"].copy()
    hits["frame"][3] = 1
    assert _run_harness(harness, tmp_path, hits, 1, 1) is None


# ---- the build --------------------------------------------------------------------------------------------------------------------------


def test_library_exports_and_python_layer_bind_the_new_entry_points():
    build.build_lib()
    L = native.lib()
    for name in NEW_EXPORTS:
        assert hasattr(L, name), f"libheadtrackr_hip.so does not export {name}"
        assert name in native.SYMBOLS
    assert L.ht_detect_best_enqueue(None, 0, 0) < 0 and L.ht_detect_best_collect(None, None, None) < 0
    assert L.ht_detect_best_collect_requeue(None, None, None, 0) < 0 and L.ht_detect_grouped(None, 0, None, 0, None) < 0
    assert L.ht_detect_best_records_device(None, None, None) < 0 and L.ht_group_hits(None, None, 0, 0, 0, None, None, None) < 0
    from headtrackr_amd.api import Context

    for m in ("detect_best_enqueue", "detect_best_collect", "detect_best_collect_requeue", "detect_grouped", "detect_best_records_ptr", "group_hits"):
        assert callable(getattr(Context, m))


def test_new_kernels_live_in_the_fourth_code_object_and_the_recorded_ones_are_unchanged():
    from benchlib import fingerprint
    from test_backproject_cpu import _gfx950_code_objects

    build.build_lib()
    recorded = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))["_build"]
    now = fingerprint.code_objects()
    for unit in ("pyramid", "scan", "camshift"):
        assert now.get(unit) == recorded[unit], (unit, now.get(unit), recorded[unit])
    objs = _gfx950_code_objects(build.LIB)
    assert len(objs) == 4
    mine = [o for o in objs if b"k_grp_frames" in o]
    assert len(mine) == 1 and b"k_bp_project" in mine[0]
    kr = _tool("kernel_resources")
    names = [kr.short(k) for k, v in kr.kernel_resources().items() if "vgpr_count" in v]
    for k in NEW_KERNELS:
        assert k in names and k.split("<")[0].encode() in mine[0], (k, names)
        for marker in fingerprint.UNITS.values():
            assert marker.decode() not in k
    for marker in fingerprint.UNITS.values():
        assert marker not in mine[0]
    assert "ht_group.hip" not in build.HIP_SOURCES
    assert "__global__" not in open(os.path.join(CSRC, "ht_context.hip")).read()
    assert '#include "ht_group.hip"' in open(os.path.join(CSRC, "ht_backproject.hip")).read()


def test_new_kernels_fit_their_budgets():
    """code-object metadata: no spills, no scratch, static LDS within 64 KB; the per-frame kernel runs 1024 threads per workgroup
    (<= 128 VGPRs) and its per-hit records are what sets the cap: twice the cap would not fit"""
    build.build_lib()
    kr = _tool("kernel_resources")
    res = {kr.short(k): v for k, v in kr.kernel_resources().items() if "vgpr_count" in v}
    for k in NEW_KERNELS:
        r = res[k]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (k, r)
        assert r["group_segment_fixed_size"] <= 64 * 1024, (k, r)
    lds = res["k_grp_frames<1024>"]["group_segment_fixed_size"]
    assert res["k_grp_frames<1024>"]["vgpr_count"] <= 128 and 32 * 1024 < lds and 2 * (lds - 4096) > 64 * 1024
    assert res["k_grp_frames<64>"]["group_segment_fixed_size"] <= 8 * 1024  # the one-wavefront form: many frames per CU


def test_kernel_takes_its_arithmetic_as_separately_rounded_operations():
    """the unit is compiled with -ffp-contract=off; the source says so too: no fused multiply-add, no fmax, explicit _rn operations"""
    src = open(os.path.join(CSRC, "ht_group.hip")).read()
    dev = src[:src.index("// ---- host side")]
    assert "fma(" not in dev and "fmax" not in dev and "pow(" not in dev
    assert dev.count("__dmul_rn") >= 8 and dev.count("__dadd_rn") >= 12 and dev.count("__ddiv_rn") == 4
    assert "atomicCAS" not in dev and "while (" not in dev  # no spin; every loop is a counted for


# ---- the N-API shim and the JavaScript layer ---------------------------------------------------------------------------------------------

JS_CALLS = ("detectBestEnqueue", "collectBestDevice", "detectGrouped", "detectBestRecords", "groupHits")


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_exports_the_new_calls_and_refuses_malformed_arguments():
    """the product addon has the five bindings and each of them answers a malformed call with an exception (tests/js/addon_args.js throws
    14 kinds of wrong values at every export, these included)"""
    addon = build.build_addon()
    assert addon is not None
    js = "const A = require(%r); console.log(JSON.stringify(%r.map(function (k) { return typeof A[k]; })));" % (addon, list(JS_CALLS))
    r = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-800:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == ["function"] * len(JS_CALLS)
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "addon_args.js")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-800:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert not set(out["silent"]) & set(JS_CALLS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_addon_still_loads_against_a_c_abi_without_the_new_symbols(tmp_path):
    """tests/js/abi_stub.cc defines none of the new exports: the shim binds them lazily (direct calls, no table of function pointers), so
    the addon linked against the stub loads and reproduces its recorded transcript"""
    import addon_stub

    got = addon_stub.run(addon_stub.NAPI_SRC, tmp_path)
    want = json.load(open(addon_stub.GOLDEN))
    assert len(want) > 900 and got["transcript"] == want
    src = open(addon_stub.NAPI_SRC).read()
    for sym in NEW_EXPORTS:
        assert ("&" + sym) not in src and sym + "(" in src  # called, never taken the address of
    assert not any(sym in open(os.path.join(ROOT, "tests", "js", "abi_stub.cc")).read() for sym in NEW_EXPORTS)


@pytest.mark.skipif(not HAVE_NODE, reason="node / node_api.h not installed")
def test_js_device_grouping_on_the_cpu_mock(tmp_path, cascade):
    """new ccv.DeviceBatch(.., {grouping: 'device'}) on the oracle-backed mock: detectBest, detect, whitebalance and the C5 loop's step
    functions return what the default route returns; the default route makes none of the new addon calls"""
    from test_js_host import _build_oracle_addon

    _build_oracle_addon()
    job = gc.js_job(tmp_path, cascade.blob, load_golden("detect.json"))
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "group_cpu.js"), str(jf)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"], out["errors"]
    assert out["compared"] >= 20 and out["grouped_rects"] == 8 and out["initialised"] == 2 and out["missing_checks"] == 4
    assert not set(out["host_calls"]) & set(JS_CALLS)
    assert out["host_calls"]["collectBest"] == 5 and out["host_calls"]["detectCollect"] == 1
    dc = out["device_calls"]
    assert "collectBest" not in dc and "detectCollect" not in dc
    # 3 detectBest batches over 2 contexts (2 enqueued by the host, 1 inside the library's requeue), detect, whitebalance, detectStep
    assert dc["collectBestDevice"] == 6 and dc["detectBestEnqueue"] == 5 and dc["detectGrouped"] == job["n"]

"""CPU-side checks of the canvas-draw calls' host path, written once (headtrackr_amd/csrc/ht_draw_calls.hip): the host-only plan of a
call's destination in headtrackr_amd/csrc/ht_draw_dest_plan.h against a Python restatement — the form, the effective stride, the range the
call will write, every refusal of each of the four call kinds and, by adjacent double faults, each kind's ORDER of them — plain and under
AddressSanitizer + UBSan, as a program of its own; and where the family's text lives.  No compute calls (no GPU here)."""
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "headtrackr_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
FRAMES, YUV, LIST, FILTERED = range(4)
KINDS = {FRAMES: "ht_draw_frames_device", YUV: "ht_draw_frames_yuv_device", LIST: "ht_draw_list_device", FILTERED: "ht_draw_list_filtered_device"}
OK, MISALIGNED, BAD_STRIDE, SOURCES, CAPACITY = range(5)
W, H = 97, 81
FB = W * H * 4
DST, OWN, MAX_BATCH = 0x100000, 0x900000, 4
MESSAGES = {
    MISALIGNED: {FRAMES: "NULL source or misaligned pointer (4-byte alignment required)", YUV: "misaligned destination (4-byte alignment required)",
                 LIST: "misaligned destination (4-byte alignment required)", FILTERED: "misaligned destination (4-byte alignment required)"},
    BAD_STRIDE: dict.fromkeys(KINDS, "destination frame stride smaller than a frame or not a multiple of 4"),
    CAPACITY: {FRAMES: "more frames than the geometry's batch capacity", YUV: "more frames than the geometry's batch capacity",
               LIST: "more entries than the geometry's batch capacity", FILTERED: "more entries than the geometry's batch capacity"},
}


def _build_harness(tmp_path_factory, sanitize):
    exe = str(tmp_path_factory.mktemp("draw_dest_plan") / ("draw_dest_plan_harness" + ("_san" if sanitize else "")))
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "host", "draw_dest_plan_harness.cc"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return _build_harness(tmp_path_factory, False)


@pytest.fixture(scope="module")
def harness_san(tmp_path_factory):
    """the same program with AddressSanitizer + UBSan linked in: a stand-alone executable, run directly"""
    return _build_harness(tmp_path_factory, True)


def call(kind, n=2, dst=DST, stride=0, max_batch=MAX_BATCH, own=OWN, own_bytes=0, fault=False, src=0, src_bytes=0, w=W, h=H):
    return dict(kind=kind, w=w, h=h, n=n, dst=dst, stride=stride, max_batch=max_batch, own=own, own_bytes=own_bytes, fault=fault, src=src, src_bytes=src_bytes)


def run(exe, tmp_path, calls):
    path = str(tmp_path / "calls.txt")
    with open(path, "w") as f:
        for c in calls:
            f.write("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (c["kind"], c["w"], c["h"], c["n"], c["dst"], c["stride"], c["max_batch"], c["own"], c["own_bytes"],
                                                              c["fault"], c["src"], c["src_bytes"]))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    out = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(out) == len(calls)
    return out


def want(c):
    """the Python restatement.  Each kind's order as its entry point had it before the host path was written once:
         ht_draw_frames_device         source pointer and destination alignment in ONE check; bind: capacity | caller's buffer: stride
         ht_draw_frames_yuv_device     destination alignment; bind: capacity | caller's buffer: stride
         the two list calls            destination alignment; stride (caller's buffer only); the entries; bind: capacity
       A stride given with no destination is not looked at by any call."""
    kind, fb, bind = c["kind"], c["w"] * c["h"] * 4, c["dst"] == 0
    stride = c["stride"] if (not bind and c["stride"]) else fb
    bad_stride = stride % 4 != 0 or stride < fb
    checks = {"pointers": c["dst"] % 4 != 0 or (kind == FRAMES and c["fault"]), "stride": bad_stride, "sources": kind in (LIST, FILTERED) and c["fault"],
              "capacity": bind and c["n"] > c["max_batch"]}
    order = ["pointers", "stride", "sources", "capacity"] if kind in (LIST, FILTERED) else ["pointers", "capacity", "stride"]
    status = dict(pointers=MISALIGNED, stride=BAD_STRIDE, sources=SOURCES, capacity=CAPACITY)
    for name in order:
        if checks[name]:
            st = status[name]
            return dict(status=st, behind_device=int(st == CAPACITY or (st == BAD_STRIDE and kind in (FRAMES, YUV))))
    base, nbytes = (c["own"], max(c["own_bytes"], fb * c["n"])) if bind else (c["dst"], (c["n"] - 1) * stride + fb)
    meets = c["src"] != 0 and base != 0 and c["src"] < base + nbytes and base < c["src"] + c["src_bytes"]
    return dict(status=OK, behind_device=0, bind=int(bind), fbytes=fb, stride=stride, base=base, bytes=nbytes, overlap=0 if meets else -1)


def check(got, calls):
    for g, c in zip(got, calls):
        w = want(c)
        assert {k: g[k] for k in w} == w, (c, g, w)
        if w["status"] in MESSAGES:
            assert g["message"] == MESSAGES[w["status"]][c["kind"]], (c, g)
        if w["status"] == OK:
            own = "the source lies inside" if c["kind"] == FRAMES else "a source plane lies inside"
            met = "source and destination overlap" if c["kind"] == FRAMES else "a source plane and the destination overlap"
            assert g["overlap_message"] == (own + " the context's own frame buffer" if w["bind"] else met), (c, g)


def plan_cases():
    """-> (calls, {index: the status the case is about}) — every case of every kind"""
    calls, about = [], {}

    def add(c, status=None):
        if status is not None:
            about[len(calls)] = status
        calls.append(c)

    for kind in KINDS:
        # every refusal on its own
        add(call(kind, dst=DST + 2), MISALIGNED)
        add(call(kind, dst=DST + 1), MISALIGNED)
        add(call(kind, fault=True), {FRAMES: MISALIGNED, YUV: OK, LIST: SOURCES, FILTERED: SOURCES}[kind])
        add(call(kind, stride=FB - 4), BAD_STRIDE)
        add(call(kind, stride=FB + 2), BAD_STRIDE)
        add(call(kind, stride=FB + 1), BAD_STRIDE)
        add(call(kind, dst=0, n=MAX_BATCH + 1), CAPACITY)
        # the stride default, stride == fbytes, a larger one; n == max_batch in the bind form and above it in a caller's buffer
        add(call(kind), OK)
        add(call(kind, stride=FB), OK)
        add(call(kind, stride=FB + 4 * 41, n=3), OK)
        add(call(kind, dst=0, n=MAX_BATCH), OK)
        add(call(kind, n=MAX_BATCH + 1), OK)
        add(call(kind, dst=0, n=1, stride=FB - 4), OK)  # a stride without a destination is not looked at
        # the own buffer smaller and larger than fbytes * n, and not allocated yet
        add(call(kind, dst=0, n=3, own_bytes=FB), OK)
        add(call(kind, dst=0, n=3, own_bytes=4 * FB + 64), OK)
        add(call(kind, dst=0, n=3, own=0, own_bytes=0), OK)
        # n = 1: the range is fbytes whatever the stride
        add(call(kind, n=1, stride=FB + 400), OK)
        add(call(kind, n=1, stride=FB + 400, src=DST + FB, src_bytes=16), OK)
        # a source that touches the last written byte, and one that starts one byte past it; one that ends at the first byte and one in front
        last = DST + 2 * (FB + 8) + FB - 1
        add(call(kind, n=3, stride=FB + 8, src=last, src_bytes=64), OK)
        add(call(kind, n=3, stride=FB + 8, src=last + 1, src_bytes=64), OK)
        add(call(kind, n=3, stride=FB + 8, src=DST - 64, src_bytes=65), OK)
        add(call(kind, n=3, stride=FB + 8, src=DST - 64, src_bytes=64), OK)
        add(call(kind, dst=0, n=2, own_bytes=3 * FB, src=OWN + 3 * FB - 1, src_bytes=8), OK)  # the bind form: the buffer as it is now ...
        add(call(kind, dst=0, n=2, own_bytes=3 * FB, src=OWN + 3 * FB, src_bytes=8), OK)
        add(call(kind, dst=0, n=4, own_bytes=3 * FB, src=OWN + 4 * FB - 1, src_bytes=8), OK)  # ... and as far as this call writes it
        add(call(kind, dst=0, n=4, own_bytes=3 * FB, src=OWN + 4 * FB, src_bytes=8), OK)
        # adjacent double faults: both present, the earlier check's status is reported
        add(call(kind, dst=DST + 2, stride=FB + 2), MISALIGNED)
        if kind == FRAMES:
            add(call(kind, fault=True, stride=FB + 2), MISALIGNED)
            add(call(kind, fault=True, dst=0, n=MAX_BATCH + 1), MISALIGNED)
        if kind == YUV:  # (its sources are checked in front of the plan: the flag is not looked at)
            add(call(kind, fault=True, stride=FB + 2), BAD_STRIDE)
            add(call(kind, fault=True, dst=0, n=MAX_BATCH + 1), CAPACITY)
        if kind in (LIST, FILTERED):
            add(call(kind, stride=FB - 4, fault=True), BAD_STRIDE)
            add(call(kind, dst=DST + 2, fault=True), MISALIGNED)
            add(call(kind, fault=True, dst=0, n=MAX_BATCH + 1), SOURCES)
            add(call(kind, fault=True, dst=0, n=MAX_BATCH + 1, stride=FB - 4), SOURCES)
        add(call(kind, dst=0, n=MAX_BATCH + 1, stride=FB - 4), CAPACITY)  # bind form: the capacity, never the stride
    return calls, about


def test_plan_matches_the_restatement(harness, tmp_path):
    calls, about = plan_cases()
    got = run(harness, tmp_path, calls)
    check(got, calls)
    for i, status in about.items():
        assert got[i]["status"] == status, (calls[i], got[i])  # the case is the case it was written as
    overlaps = [g["overlap"] for g in got if g["status"] == OK]
    assert 0 in overlaps and -1 in overlaps
    # the boundary pairs, spelled out for one kind: the last written byte is met, the byte behind it is not
    pairs = [(c, g) for c, g in zip(calls, got) if c["kind"] == LIST and c["src"]]
    assert [g["overlap"] for _, g in pairs] == [-1, 0, -1, 0, -1, 0, -1, 0, -1]


def test_plan_under_the_sanitizers(harness, harness_san, tmp_path):
    calls, _ = plan_cases()
    assert run(harness_san, tmp_path, calls) == run(harness, tmp_path, calls)


def test_the_host_path_exists_once():
    """the draw family's host path is ht_draw_calls.hip, included last; what it replaced is gone from every file"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc", ".cc"))}
    ingest = text["ht_ingest.hip"]
    assert ingest.rstrip().endswith('#include "ht_draw_calls.hip"') and ingest.count('#include "ht_draw_calls.hip"') == 1
    assert "hip" not in re.sub(r"\.hip\b", "", text["ht_draw_dest_plan.h"].split("#pragma once")[1]).lower()  # behind its header comment: no HIP
    everything = "".join(text.values())
    for gone in ("ig_draw_bound", "igy_draw_bound", "or_stage_reserve", "ig_overlap"):
        assert gone not in everything, gone
    others = "".join(t for f, t in text.items() if f not in ("ht_context.hip", "ht_frames.hip", "ht_internal.h"))  # the defining unit (ht_frames.hip is part of it)
    assert others.count("ht_frames_own_reserve(") == 1 and others.count("ht_frames_bind_own(") == 1
    assert everything.count("hipMalloc(reinterpret_cast<void **>(&c->d_ingest_src)") == 1
    calls = text["ht_draw_calls.hip"]
    assert calls.count("ht_frames_own_reserve(") == 1 and calls.count("hipMalloc(reinterpret_cast<void **>(&c->d_ingest_src)") == 1
    assert calls.count("ht_draw_dest_plan(") == 1 and everything.count("ht_draw_dest_plan(") == 2  # every device call's one resolve; the definition
    # every entry point of the family is defined here and nowhere else
    exports = ("ht_draw_frames_device", "ht_draw_frames", "ht_draw_frames_yuv_device", "ht_draw_frames_yuv", "ht_draw_list_device", "ht_draw_list_filtered_device",
               "ht_draw_filter_factors")
    for fn in exports:
        assert len(re.findall(r'^extern "C" ht_status %s\(' % fn, calls, re.M)) == 1, fn
        assert sum(len(re.findall(r'^extern "C" ht_status %s\(' % fn, t, re.M)) for t in text.values()) == 1, fn
    # no function of the family is declared ahead of its definition, but the one the face-patch calls need
    for name, declared in (("dm_launch_unfiltered", 0), ("or_launch", 0), ("dm_orient_first", 0), ("dm_unpack_sources", 1)):
        assert len(re.findall(r"^ht_status %s\([^{]*\);" % name, everything, re.M)) == declared, name
        assert len(re.findall(r"^ht_status %s\([^;{]*\) \{" % name, everything, re.M)) == 1, name
    assert len(re.findall(r"^ht_status dm_unpack_sources\(", text["ht_face_calls.hip"], re.M)) == 1
    # the RGBA entry of an upright frame is spelled once, the staging buffer is carved in one place
    assert everything.count("format = HT_DRAW_RGBA, e.d.kc = HtYuvCoef{}") == 1 and everything.count("or_upright(c, fn, jobs, frames)") == 1
    assert everything.count("c->d_ingest_src + at") == 1 and calls.count("c->d_ingest_src + at") == 1
